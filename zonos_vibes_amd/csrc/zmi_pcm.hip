// PCM16 egress: many fp32 waveform segments -> one packed int16 buffer in one launch (the reference server's
// np.clip(wav, -1, 1) * 32767 -> astype(int16), server.py:142-146, for every lane of a serving round at once).
#include "zmi_common.h"
#include "zmi_kernels.h"

namespace {
constexpr int PCM_PIECE = 2048;   // int16 samples of the packed output one workgroup converts (8 KiB in, 4 KiB out)
constexpr int PCM_THREADS = 256;

// q = (int16) trunc(fl32(clamp(x, -1, 1) * 32767.0f)): the product is a separate fp32 rounding (the library is built
// with -ffp-contract=off), |product| <= 32767 so the cast is defined, and it truncates toward zero. NaN -> 0 is
// written out: the C cast of a NaN is undefined (numpy and torch on x86 give 0). -0.0 and subnormals give 0.
__device__ __forceinline__ int pcm16(float x) {
  if (x != x) return 0;
  const float c = fminf(fmaxf(x, -1.0f), 1.0f);
  return (int)(c * 32767.0f);
}

__device__ __forceinline__ uint32_t pcm16_pair(float a, float b) {
  return ((uint32_t)pcm16(a) & 0xffffu) | ((uint32_t)pcm16(b) << 16);
}

// Workgroup b owns out[b PIECE, min((b + 1) PIECE, total)). It finds the first segment that reaches into its piece
// by bisection (the segments' ends ascend with their dst) and walks the table from there. Of each segment's part in
// the piece, the samples up to the first 8-byte-aligned address of `out` and the last (< 4) go one int16 store each;
// the middle goes 4 samples per thread: one 8-byte store, fed by one 16-byte load where the source is aligned so and
// by four 4-byte loads where it is not (src is any fp32 address, dst any int16 index: their alignments are unrelated).
__global__ __launch_bounds__(PCM_THREADS) void pcm16_pack_kernel(const ZmiPcmSeg* __restrict__ segs, int n_segs,
                                                                 int64_t total, int16_t* __restrict__ out) {
  const int64_t p0 = (int64_t)blockIdx.x * PCM_PIECE;
  const int64_t p1 = p0 + PCM_PIECE < total ? p0 + PCM_PIECE : total;
  int lo = 0, hi = n_segs;  // first segment with dst + n > p0
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (segs[mid].dst + segs[mid].n > p0) hi = mid; else lo = mid + 1;
  }
  for (int s = lo; s < n_segs; ++s) {
    const ZmiPcmSeg sg = segs[s];
    if (sg.dst >= p1) break;
    const int64_t a = sg.dst > p0 ? sg.dst : p0;
    const int64_t e = sg.dst + sg.n < p1 ? sg.dst + sg.n : p1;
    if (e <= a) continue;  // an empty segment
    const float* sp = sg.src;
    const int64_t off = sg.dst;  // sp[i - off] is the sample of out[i], for i in [a, e) only
    // head: up to the first i >= a with out + i 8-byte aligned
    int64_t m0 = a + (int64_t)(((8u - (unsigned)((uintptr_t)(out + a) & 7u)) & 7u) >> 1);
    if (m0 > e) m0 = e;
    const int64_t units = (e - m0) >> 2, m1 = m0 + 4 * units;
    const int t = threadIdx.x;
    if (a + t < m0) out[a + t] = (int16_t)pcm16(sp[a + t - off]);
    if (m1 + t < e) out[m1 + t] = (int16_t)pcm16(sp[m1 + t - off]);
    const bool wide = ((uintptr_t)(sp + (m0 - off)) & 15u) == 0;
    for (int64_t u = t; u < units; u += PCM_THREADS) {
      const int64_t i = m0 + 4 * u;
      const float* x = sp + (i - off);
      float4 v;
      if (wide) {
        v = *reinterpret_cast<const float4*>(x);
      } else {
        v.x = x[0]; v.y = x[1]; v.z = x[2]; v.w = x[3];
      }
      *reinterpret_cast<uint2*>(out + i) = make_uint2(pcm16_pair(v.x, v.y), pcm16_pair(v.z, v.w));
    }
  }
}
}  // namespace

extern "C" int zmi_pcm16_pack(const ZmiPcmSeg* segs, int n_segs, int64_t total, int16_t* out, void* stream) {
  if (n_segs < 0 || total < 0) return zmi_fail_msg("pcm16_pack: n_segs and total must be >= 0");
  if (n_segs == 0 || total == 0) return 0;
  if (!segs || !out) return zmi_fail_msg("pcm16_pack: segs and out must not be NULL");
  if ((uintptr_t)out & 1u) return zmi_fail_msg("pcm16_pack: out must be 2-byte aligned");
  const int64_t pieces = (total + PCM_PIECE - 1) / PCM_PIECE;
  if (pieces > 0x7fffffff) return zmi_fail_msg("pcm16_pack: total too large for one launch");
  hipLaunchKernelGGL(pcm16_pack_kernel, dim3((unsigned)pieces), dim3(PCM_THREADS), 0, (hipStream_t)stream, segs,
                     n_segs, total, out);
  ZMI_CHECK(hipGetLastError());
  return 0;
}
