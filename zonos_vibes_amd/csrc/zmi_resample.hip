// Sample-rate conversion: torchaudio's default polyphase resampler (Hann-windowed sinc, speaker.resample_kernel's
// table) for many independent pieces of audio in one launch, one-shot or streamed (zonos_hip.h: ZmiResampleSeg).
//
//   y[j] = sum_{t < T} xz[(j / n) o - W + t] * kern[j % n][t],   T = 2 W + o,  xz = x inside the utterance, 0 outside
//
// Summation order (a function of t alone, the same for every phase, lane, launch shape and chunking): four fp32
// accumulators a0..a3 start at +0; tap t, in ascending t, goes into a[t & 3] by one fused multiply-add
// a = fma(x, k, a); the result is (a0 + a1) + (a2 + a3). Taps that fall outside the utterance take part with x = 0,
// so a streamed frame (emitted only once all its taps are there) and the one-shot frame see the same operands.
#include "zmi_common.h"
#include "zmi_kernels.h"

namespace {
constexpr int RS_TILE = 1024;     // outputs of the packed buffer one workgroup owns
constexpr int RS_THREADS = 256;
constexpr int RS_LDS = 12288;     // most floats of input a part may stage (48 KiB); a longer span is read from memory

// sample `i` (absolute index in the utterance) of a segment: 0 outside the utterance and outside what the segment holds
__device__ __forceinline__ float seg_sample(const ZmiResampleSeg& sg, int64_t i) {
  if (i < 0 || (sg.n_total >= 0 && i >= sg.n_total)) return 0.0f;
  const int64_t r = i - sg.i0;
  if (r < 0) return 0.0f;
  if (r < sg.n_carry) return sg.carry[r];
  if (r < sg.n_carry + sg.n_src) return sg.src[r - sg.n_carry];
  return 0.0f;
}

// one output's chain; x(t) is tap t's input sample, k points at kern_t[0][p] (stride n between taps, n T <= 2^22)
template <class X>
__device__ __forceinline__ float chain(X x, const float* __restrict__ k, int T, int n) {
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
  int t = 0;
  for (; t + 4 <= T; t += 4) {
    a0 = fmaf(x(t), k[t * n], a0);
    a1 = fmaf(x(t + 1), k[(t + 1) * n], a1);
    a2 = fmaf(x(t + 2), k[(t + 2) * n], a2);
    a3 = fmaf(x(t + 3), k[(t + 3) * n], a3);
  }
  if (t < T) a0 = fmaf(x(t), k[t * n], a0);
  if (t + 1 < T) a1 = fmaf(x(t + 1), k[(t + 1) * n], a1);
  if (t + 2 < T) a2 = fmaf(x(t + 2), k[(t + 2) * n], a2);
  return (a0 + a1) + (a2 + a3);
}

// Workgroup b owns out[b TILE, min((b + 1) TILE, total)): it finds the first segment that reaches into its tile by
// bisection (the segments' ends ascend with their dst) and walks the table from there; almost always the tile lies in
// one segment. Of each segment's part in the tile, outputs ja .. je - 1 (absolute), the input span
// [(ja / n) o - W, ((je - 1) / n) o - W + T) is staged into LDS once (zeros where the utterance has no sample), and
// thread r runs the chains of outputs ja + r, ja + r + 256, ... from it. Lanes of one frame read the same LDS address
// (a broadcast); a wave touches at most 64 / n + 2 frames, o floats apart, so at worst that many distinct addresses
// share a bank. The table is kern_t[t][p]: neighbouring lanes are neighbouring phases, so its reads coalesce. A span
// longer than RS_LDS floats (o or W in the thousands) is read from memory through the same seg_sample, same order.
// The LDS is dynamic: the launch asks for lds_floats = the longest span any part of this table can have (lds_span
// below; 1.3k floats for 48 -> 44.1 kHz, 6.7k for 44.1 -> 8 kHz), capped at RS_LDS, so LDS does not bound occupancy
// at the common rates.
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const ZmiResampleSeg* __restrict__ segs, int n_segs,
                                                              int64_t total, const float* __restrict__ kern_t, int o,
                                                              int n, int W, float* __restrict__ out, int lds_floats) {
  extern __shared__ float xs[];
  const int T = 2 * W + o;
  const int64_t p0 = (int64_t)blockIdx.x * RS_TILE;
  const int64_t p1 = p0 + RS_TILE < total ? p0 + RS_TILE : total;
  int lo = 0, hi = n_segs;  // first segment with dst + n_out > p0
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (segs[mid].dst + segs[mid].n_out > p0) hi = mid; else lo = mid + 1;
  }
  for (int s = lo; s < n_segs; ++s) {
    const ZmiResampleSeg sg = segs[s];
    if (sg.dst >= p1) break;
    const int64_t a = sg.dst > p0 ? sg.dst : p0;
    const int64_t e = sg.dst + sg.n_out < p1 ? sg.dst + sg.n_out : p1;
    if (e <= a) continue;  // an empty segment
    const int64_t ja = sg.j0 + (a - sg.dst);
    const int cnt = (int)(e - a);           // <= RS_TILE
    const int64_t fa = ja / n;
    const int ph0 = (int)(ja - fa * n);
    const int64_t s0 = fa * o - W;          // absolute input index of the span's first sample
    const int frames = (ph0 + cnt - 1) / n + 1;
    const int64_t span = (int64_t)(frames - 1) * o + T;
    if (span <= lds_floats) {
      __syncthreads();  // the previous part's chains have read xs
      for (int i = threadIdx.x; i < (int)span; i += RS_THREADS) xs[i] = seg_sample(sg, s0 + i);
      __syncthreads();
      for (int r = threadIdx.x; r < cnt; r += RS_THREADS) {
        const int q = ph0 + r, f = q / n, p = q - f * n;
        const float* xf = xs + f * o;
        out[a + r] = chain([&](int t) { return xf[t]; }, kern_t + p, T, n);
      }
    } else {
      for (int r = threadIdx.x; r < cnt; r += RS_THREADS) {
        const int q = ph0 + r, f = q / n, p = q - f * n;
        const int64_t x0 = s0 + (int64_t)f * o;
        out[a + r] = chain([&](int t) { return seg_sample(sg, x0 + t); }, kern_t + p, T, n);
      }
    }
  }
}

// carry_out[0 .. n_keep) = the last n_keep samples of (carry, src): one workgroup per segment
__global__ __launch_bounds__(RS_THREADS) void resample_carry_kernel(const ZmiResampleSeg* __restrict__ segs) {
  const ZmiResampleSeg sg = segs[blockIdx.x];
  const int64_t have = sg.n_carry + sg.n_src, first = have - sg.n_keep;
  for (int64_t i = threadIdx.x; i < sg.n_keep; i += RS_THREADS) {
    const int64_t r = first + i;
    sg.carry_out[i] = r < sg.n_carry ? sg.carry[r] : sg.src[r - sg.n_carry];
  }
}

// The host's copy of the table is checked before anything is launched: the kernels never index outside what a
// segment declares, and this makes sure that what it declares is coherent.
const char* check_segs(const ZmiResampleSeg* h, int n_segs, int64_t total_out, int o, int n, int W) {
  const int64_t T = 2 * (int64_t)W + o;
  int64_t end = 0;
  for (int s = 0; s < n_segs; ++s) {
    const ZmiResampleSeg& g = h[s];
    if (g.n_carry < 0 || g.n_src < 0 || g.n_out < 0 || g.n_keep < 0 || g.i0 < 0 || g.j0 < 0 || g.n_total < -1)
      return "resample: a segment has a negative count or index";
    if ((g.n_carry && !g.carry) || (g.n_src && !g.src) || (g.n_keep && !g.carry_out))
      return "resample: a segment has a NULL pointer with a non-zero count";
    if (((uintptr_t)g.carry | (uintptr_t)g.src | (uintptr_t)g.carry_out) & 3u)
      return "resample: a segment's pointers must be 4-byte aligned";
    if (g.dst < end || g.dst + g.n_out > total_out)
      return "resample: segments must ascend in dst, without overlap, inside total_out";
    end = g.dst + g.n_out;
    const int64_t have = g.i0 + g.n_carry + g.n_src;  // the utterance's samples the segment knows: [i0, have)
    if (g.n_keep > g.n_carry + g.n_src || g.n_keep > T) return "resample: n_keep exceeds the segment's samples or T";
    if (g.n_keep && g.carry_out == g.carry) return "resample: carry_out must not be the carry it is made from";
    if (g.n_total >= 0 && g.n_total != have) return "resample: a final segment must end at n_total";
    if (g.n_out) {
      const int64_t first = (g.j0 / n) * o - W, last = ((g.j0 + g.n_out - 1) / n) * o - W + T - 1;
      if ((first > 0 ? first : 0) < g.i0) return "resample: a segment's outputs need samples before its carry";
      if (g.n_total < 0 && last >= have)
        return "resample: a segment that is not final emits a frame with taps missing";
      if (g.n_total >= 0 && g.j0 + g.n_out > ((int64_t)n * g.n_total + o - 1) / o)
        return "resample: a final segment emits past ceil(n n_total / o)";
    }
  }
  return nullptr;
}

// The longest input span a tile part of this table can have: at most min(RS_TILE, the longest n_out) outputs,
// starting at the last phase of a frame.
int64_t lds_span(const ZmiResampleSeg* h, int n_segs, int o, int n, int W) {
  int64_t cnt = 0;
  for (int s = 0; s < n_segs; ++s) cnt = h[s].n_out > cnt ? h[s].n_out : cnt;
  if (cnt > RS_TILE) cnt = RS_TILE;
  if (cnt < 1) cnt = 1;
  const int64_t frames = (n - 1 + cnt - 1) / n + 1;
  return (frames - 1) * o + 2 * (int64_t)W + o;
}

int check_args(const char*& err, const ZmiResampleSeg* segs, const ZmiResampleSeg* segs_host, int n_segs,
               int64_t total_out, int o, int n, int W) {
  if (n_segs < 0 || total_out < 0) { err = "resample: n_segs and total_out must be >= 0"; return 1; }
  if (o < 1 || n < 1 || W < 1) { err = "resample: o, n and W must be >= 1"; return 1; }
  if ((int64_t)n * (2 * (int64_t)W + o) > ((int64_t)1 << 22)) {
    err = "resample: the table n (2 W + o) exceeds 2^22 floats";
    return 1;
  }
  if (n_segs && (!segs || !segs_host)) { err = "resample: segs and segs_host must not be NULL"; return 1; }
  err = check_segs(segs_host, n_segs, total_out, o, n, W);
  return err != nullptr;
}
}  // namespace

extern "C" int zmi_resample(const ZmiResampleSeg* segs, const ZmiResampleSeg* segs_host, int n_segs, int64_t total_out,
                            const float* kern_t, int o, int n, int W, float* out, void* stream) {
  const char* err = nullptr;
  if (check_args(err, segs, segs_host, n_segs, total_out, o, n, W)) return zmi_fail_msg(err);
  if (n_segs == 0 || total_out == 0) return 0;
  if (!kern_t || !out) return zmi_fail_msg("resample: kern_t and out must not be NULL");
  if (((uintptr_t)kern_t | (uintptr_t)out) & 3u) return zmi_fail_msg("resample: kern_t and out must be 4-byte aligned");
  const int64_t tiles = (total_out + RS_TILE - 1) / RS_TILE;
  if (tiles > 0x7fffffff) return zmi_fail_msg("resample: total_out too large for one launch");
  const int64_t span = lds_span(segs_host, n_segs, o, n, W);
  const int lds_floats = (int)(span < RS_LDS ? span : RS_LDS);
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles), dim3(RS_THREADS), (size_t)lds_floats * sizeof(float),
                     (hipStream_t)stream, segs, n_segs, total_out, kern_t, o, n, W, out, lds_floats);
  ZMI_CHECK(hipGetLastError());
  return 0;
}

extern "C" int zmi_resample_carry(const ZmiResampleSeg* segs, const ZmiResampleSeg* segs_host, int n_segs, int o, int n,
                                  int W, void* stream) {
  const char* err = nullptr;
  int64_t total = 0;
  for (int s = 0; segs_host && s < n_segs; ++s)
    if (segs_host[s].dst + segs_host[s].n_out > total) total = segs_host[s].dst + segs_host[s].n_out;
  if (check_args(err, segs, segs_host, n_segs, total, o, n, W)) return zmi_fail_msg(err);
  if (n_segs == 0) return 0;
  hipLaunchKernelGGL(resample_carry_kernel, dim3((unsigned)n_segs), dim3(RS_THREADS), 0, (hipStream_t)stream, segs);
  ZMI_CHECK(hipGetLastError());
  return 0;
}
