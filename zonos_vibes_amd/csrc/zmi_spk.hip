// Speaker encoder (ResNet293 + SimAM, reference zonos/speaker_cloning.py:64-192) on MFMA, gfx950.
//
// Activations are fp16 channels-last [H][W][C] (H the mel axis, W time); conv weights fp16,
// channel-blocked per tap [tap][Ci / 32][Co][32] (tap = ky * k + kx) as the DAC's; fp32 accumulation
// (v_mfma_f32_16x16x32_f16). Every 3x3 / 1x1 convolution is one implicit GEMM per output tile:
//     y[ho][wo][co] = act( scale[co] * sum_tap sum_ci W[tap][co][ci] * x[ho s - p + ky][wo s - p + kx][ci] + shift[co] )
// M = the TH x TW output positions of a tile (flattened row-major), N = 16 NB output channels, K = taps x Ci.
// Per 32-channel K step a workgroup copies the tile's input halo ((TH - 1) s + k rows of (TW - 1) s + k positions)
// and the step's [tap][16 NB co][32 ci] weights into LDS once; all taps read their fragments from that halo at
// their row / column offset. scale / shift are eval-mode BatchNorm in fp32 (never folded into the fp16 weights).
// No floating-point atomics anywhere: every reduction runs in a fixed order, so two runs give the same bits.
//
// Every kernel runs over ragged lanes: clips of one H and their own W in one launch (ZmiSpkLanes, by value in the
// kernel arguments). blockIdx.z is the lane, a pointer offset of lane * stride elements; blockIdx.x covers the widest
// lane, and a workgroup past its own lane's tiles / chunks / positions returns before any barrier. Everything a
// workgroup computes (tile index, padding, chunk, row counts) comes from its own lane's W, so a lane has the bits of
// its single-clip launch. The single entry points are one lane.
#include <atomic>

#include "zmi_common.h"
#include "zmi_kernels.h"

namespace {

constexpr int TH = 8, TW = 16, NT = 256;  // output tile (rows x columns) and threads: 4 waves x 2 tile rows
constexpr int SPK_MAX_C = 2048;           // 256 threads x 8 channels: one position row of a SimAM reduction
constexpr int SIMAM_CHUNK = 128;          // positions per workgroup of the SimAM reductions

struct SpkConv {  // W, Wo, tiles_w: the kernel fills them in from its lane's width
  const f16_t* x;
  int H, W, Ci;
  const f16_t* w;
  const float* scale;
  const float* shift;
  int Co, k, stride, Ho, Wo, relu, tiles_w;
  f16_t* y;
  float* psum;
  int64_t ls_x, ls_y, ls_psum;  // lane strides in elements
};

struct SpkRows { int n[ZMI_SPK_MAX_LANES]; };  // per-lane row counts of a SimAM finish

__host__ __device__ constexpr int conv_out_dim(int n, int k, int stride) { return (n + 2 * (k >> 1) - k) / stride + 1; }

// LDS rows are 64 B (32 channels); chunk c of row r sits at chunk c ^ swz(r), the DAC conv's swizzle
// (zmi_dac.hip conv_load): 16 consecutive rows read by one 16-lane group land on distinct banks.
__device__ __forceinline__ int swz(int r) { return ((r >> 2) & 1) << 1; }

constexpr int PF = 9;  // 16 B pieces per thread and K step, of the halo and of the weights (host-checked)

template <int BN>
__device__ __forceinline__ void spk_gload(const SpkConv& a, const int (&goff)[PF], uint4 (&hv)[PF], uint4 (&wv)[PF],
                                          int cs, int tid, int nw, int nci, int co_blk) {
#pragma unroll
  for (int it = 0; it < PF; ++it) {
    uint4 v = {0u, 0u, 0u, 0u};  // the conv's zero padding, and the rows / columns past a partial tile
    if (goff[it] >= 0) v = *reinterpret_cast<const uint4*>(a.x + goff[it] + cs * 32);
    hv[it] = v;
  }
#pragma unroll
  for (int it = 0; it < PF; ++it) {
    const int i = tid + it * NT, r = i >> 2, tap = r / BN, col = r - tap * BN;
    uint4 v = {0u, 0u, 0u, 0u};
    if (i < nw) v = *reinterpret_cast<const uint4*>(a.w + (((size_t)tap * nci + cs) * a.Co + co_blk + col) * 32 + (i & 3) * 8);
    wv[it] = v;
  }
}

__device__ __forceinline__ void spk_lstore(char* halo, char* wts, const uint4 (&hv)[PF], const uint4 (&wv)[PF], int tid,
                                           int nh, int nw) {
#pragma unroll
  for (int it = 0; it < PF; ++it) {
    const int i = tid + it * NT, r = i >> 2, ch = i & 3;
    if (i < nh) *reinterpret_cast<uint4*>(halo + r * 64 + ((ch ^ swz(r)) * 16)) = hv[it];
    if (i < nw) *reinterpret_cast<uint4*>(wts + r * 64 + ((ch ^ swz(r)) * 16)) = wv[it];
  }
}

template <int NB>
__global__ __launch_bounds__(NT) void spk_conv_kernel(const SpkConv a0, const ZmiSpkLanes L) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int BN = 16 * NB;
  SpkConv a = a0;
  a.W = L.w[blockIdx.z];
  a.Wo = conv_out_dim(a.W, a.k, a.stride);
  a.tiles_w = (a.Wo + TW - 1) / TW;
  if ((int)blockIdx.x >= ((a.Ho + TH - 1) / TH) * a.tiles_w) return;  // past this lane's tiles: the whole workgroup
  a.x += blockIdx.z * a.ls_x;
  a.y += blockIdx.z * a.ls_y;
  if (a.psum) a.psum += blockIdx.z * a.ls_psum;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int taps = a.k * a.k, pad = a.k >> 1, nci = a.Ci / 32;
  const int hh = (TH - 1) * a.stride + a.k, hw = (TW - 1) * a.stride + a.k, npos = hh * hw;
  char* const halo = lds;
  char* const wts = lds + npos * 64;
  const int tile = blockIdx.x, co_blk = blockIdx.y * BN;
  const int ho0 = (tile / a.tiles_w) * TH, wo0 = (tile % a.tiles_w) * TW;
  const int hi0 = ho0 * a.stride - pad, wi0 = wo0 * a.stride - pad;

  f32x4_t acc[NB][2];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // Each thread copies up to PF 16 B pieces of the halo and PF of the weights per step (the stride-2 3x3 halo is
  // 17 x 33 positions x 4 pieces = 9 per thread; 9 taps x 64 channels x 4 = 9 per thread). The pieces of step
  // cs + 1 are loaded into registers before step cs's MFMAs and written to LDS after them, so the global latency
  // runs under the MFMAs. A halo piece's offset in x is the same at every step but for the channel block.
  const int nh = npos * 4, nw = taps * BN * 4;
  int goff[PF];  // element offset of the halo piece in x at channel block 0; < 0: zero padding / past the tensor
#pragma unroll
  for (int it = 0; it < PF; ++it) {
    const int i = tid + it * NT, r = i >> 2;
    const int hi = hi0 + r / hw, wi = wi0 + r % hw;
    goff[it] = (i < nh && hi >= 0 && hi < a.H && wi >= 0 && wi < a.W) ? (hi * a.W + wi) * a.Ci + (i & 3) * 8 : -1;
  }
  uint4 hv[PF], wv[PF];

  spk_gload<BN>(a, goff, hv, wv, 0, tid, nw, nci, co_blk);
  for (int cs = 0; cs < nci; ++cs) {
    __syncthreads();  // the previous step's fragments are read
    spk_lstore(halo, wts, hv, wv, tid, nh, nw);
    __syncthreads();
    if (cs + 1 < nci) spk_gload<BN>(a, goff, hv, wv, cs + 1, tid, nw, nci, co_blk);
    for (int tap = 0; tap < taps; ++tap) {
      const int ky = tap / a.k, kx = tap - ky * a.k;
      uint4 fa[NB], fb[2];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int r = tap * BN + i * 16 + lr;  // A: co = lane & 15, ci = 8 (lane >> 4) ..
        fa[i] = *reinterpret_cast<const uint4*>(wts + r * 64 + ((lq ^ swz(r)) * 16));
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = ((wave * 2 + j) * a.stride + ky) * hw + lr * a.stride + kx;  // B: position = lane & 15
        fb[j] = *reinterpret_cast<const uint4*>(halo + r * 64 + ((lq ^ swz(r)) * 16));
      }
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, fa[i]),
                                                             __builtin_bit_cast(f16x8_t, fb[j]), acc[i][j], 0, 0, 0);
    }
  }

  // epilogue: the accumulator's column is the position (lane & 15), its rows 4 (lane >> 4) + r the channel, so a
  // lane stores 4 consecutive channels (8 B) of its position. SimAM partial sums are of the STORED (fp16) values.
  float* const red = reinterpret_cast<float*>(lds);  // [4 waves][BN]
  if (a.psum) __syncthreads();                       // the last step's fragments are read
  const int wo = wo0 + lr;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int co = co_blk + i * 16 + lq * 4;
    const float4 sc = *reinterpret_cast<const float4*>(a.scale + co);
    const float4 sh = *reinterpret_cast<const float4*>(a.shift + co);
    const float s4[4] = {sc.x, sc.y, sc.z, sc.w}, b4[4] = {sh.x, sh.y, sh.z, sh.w};
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ho = ho0 + wave * 2 + j;
      const bool ok = ho < a.Ho && wo < a.Wo;
      uint32_t h[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float y = acc[i][j][r] * s4[r] + b4[r];
        if (a.relu) y = fmaxf(y, 0.f);
        h[r] = f2h(y);
        sum[r] += ok ? h2f(h[r]) : 0.f;
      }
      if (ok) {
        uint2 o;
        o.x = h[0] | (h[1] << 16);
        o.y = h[2] | (h[3] << 16);
        *reinterpret_cast<uint2*>(a.y + ((size_t)ho * a.Wo + wo) * a.Co + co) = o;
      }
    }
    if (a.psum) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = row16_sum(sum[r]);  // over the 16 positions of the wave's two rows
        if (lr == 0) red[wave * BN + i * 16 + lq * 4 + r] = s;
      }
    }
  }
  if (a.psum) {
    __syncthreads();
    if (tid < BN)
      a.psum[(size_t)tile * a.Co + co_blk + tid] = ((red[tid] + red[BN + tid]) + red[2 * BN + tid]) + red[3 * BN + tid];
  }
}

// The stem (Ci = 1, K = 9): a direct kernel, one thread per position x 8 output channels; w fp16 [9][Co].
__global__ __launch_bounds__(256) void spk_stem_kernel(const f16_t* x, int H, const ZmiSpkLanes L, const f16_t* w,
                                                       const float* scale, const float* shift, int Co, f16_t* y,
                                                       int64_t ls_x, int64_t ls_y) {
  const int c8n = Co / 8, W = L.w[blockIdx.z];
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)H * W * c8n) return;  // past this lane's positions
  x += blockIdx.z * ls_x;
  y += blockIdx.z * ls_y;
  const int cg = (int)(idx % c8n);
  const long pos = idx / c8n;
  const int h = (int)(pos / W), wq = (int)(pos % W);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int hi = h + tap / 3 - 1, wi = wq + tap % 3 - 1;
    if (hi < 0 || hi >= H || wi < 0 || wi >= W) continue;
    const float xv = h2f(x[(size_t)hi * W + wi]);
    const uint4 wv = *reinterpret_cast<const uint4*>(w + (size_t)tap * Co + cg * 8);
    const uint32_t u[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] += xv * h2f(u[r >> 1] >> ((r & 1) * 16));
  }
  uint32_t o[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) o[r] = f2h(fmaxf(acc[r] * scale[cg * 8 + r] + shift[cg * 8 + r], 0.f));
  *reinterpret_cast<uint4*>(y + (size_t)pos * Co + cg * 8) =
      uint4{o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16)};
}

// ---- SimAM (speaker_cloning.py:91-96) + the block tail (:87-88) ------------------------------------------
// Launches, every sum in a fixed order: [0] per-chunk channel sums of x (skipped when the producing conv wrote its
// per-tile sums), [1] mean[c] from those rows, [2] per-chunk sums of (x - mean)^2 (two-pass variance), [3] the
// denominator 4 (v + 1e-4) from those rows, [4] the elementwise pass.
__device__ __forceinline__ void unpack8(const uint4& v, float (&f)[8]) {
  const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int r = 0; r < 8; ++r) f[r] = h2f(u[r >> 1] >> ((r & 1) * 16));
}

// out[c] = the column sum of rows[n][C], finished as mean (sum / P) or as SimAM's denominator 4 (sum / (P - 1) +
// 1e-4). 8 row groups per channel (group g: rows g, g + 8, .. in order), combined in group order.
template <bool DEN>
__global__ __launch_bounds__(256) void spk_simam_finish_kernel(const float* rows, const SpkRows R, int C, int H,
                                                               const ZmiSpkLanes L, float* out, int64_t ls_rows,
                                                               int64_t ls_out) {
  __shared__ float s_part[8][32];
  const int n = R.n[blockIdx.z], P = H * L.w[blockIdx.z];
  rows += blockIdx.z * ls_rows;
  out += blockIdx.z * ls_out;
  const int g = threadIdx.x >> 5, cl = threadIdx.x & 31, c = blockIdx.x * 32 + cl;
  float s = 0.f;
  if (c < C)
    for (int t = g; t < n; t += 8) s += rows[(size_t)t * C + c];
  s_part[g][cl] = s;
  __syncthreads();
  if (g == 0 && c < C) {
    float t = s_part[0][cl];
#pragma unroll
    for (int q = 1; q < 8; ++q) t += s_part[q][cl];
    out[c] = DEN ? 4.f * (t / (float)(P - 1) + 1e-4f) : t / (float)P;
  }
}

// part[blockIdx.x][c] = sum over the chunk's positions of x (SQ = false) or (x - mean[c])^2 (SQ = true)
template <bool SQ>
__global__ __launch_bounds__(256) void spk_simam_reduce_kernel(const f16_t* x, int H, const ZmiSpkLanes L, int C,
                                                               const float* mean, float* part, int64_t ls_x,
                                                               int64_t ls_ws) {
  __shared__ float s_red[2048];
  const int P = H * L.w[blockIdx.z];
  if ((int)blockIdx.x * SIMAM_CHUNK >= P) return;  // past this lane's chunks: the whole workgroup
  x += blockIdx.z * ls_x;
  if (SQ) mean += blockIdx.z * ls_ws;
  part += blockIdx.z * ls_ws;
  const int tid = threadIdx.x, c8n = C / 8, rows = 256 / c8n;
  const int pr = tid / c8n, cg = tid - pr * c8n;
  const int p0 = blockIdx.x * SIMAM_CHUNK, p1 = min(P, p0 + SIMAM_CHUNK);
  if (pr < rows) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (SQ) {
#pragma unroll
      for (int r = 0; r < 8; ++r) m[r] = mean[cg * 8 + r];
    }
    for (int p = p0 + pr; p < p1; p += rows) {
      float f[8];
      unpack8(*reinterpret_cast<const uint4*>(x + (size_t)p * C + cg * 8), f);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float d = f[r] - m[r];
        acc[r] += SQ ? d * d : f[r];
      }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) s_red[pr * C + cg * 8 + r] = acc[r];
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float s = 0.f;
    for (int q = 0; q < rows; ++q) s += s_red[q * C + c];
    part[(size_t)blockIdx.x * C + c] = s;
  }
}

// one thread per position x 8 channels
__global__ __launch_bounds__(256) void spk_simam_apply_kernel(const f16_t* x, const f16_t* res, int H,
                                                              const ZmiSpkLanes L, int C, const float* mean,
                                                              const float* den, f16_t* y, int64_t ls_x, int64_t ls_res,
                                                              int64_t ls_ws, int64_t ls_y) {
  const int c8n = C / 8, P = H * L.w[blockIdx.z];
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)P * c8n) return;  // past this lane's positions
  x += blockIdx.z * ls_x;
  res += blockIdx.z * ls_res;
  mean += blockIdx.z * ls_ws;
  den += blockIdx.z * ls_ws;
  y += blockIdx.z * ls_y;
  const int cg = (int)(idx % c8n);
  const size_t off = (size_t)(idx / c8n) * C + cg * 8;
  float f[8], g[8];
  unpack8(*reinterpret_cast<const uint4*>(x + off), f);
  unpack8(*reinterpret_cast<const uint4*>(res + off), g);
  uint32_t o[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const float d = f[r] - mean[cg * 8 + r];
    const float e = (d * d) / den[cg * 8 + r] + 0.5f;
    const float sg = 1.f / (1.f + expf(-e));
    o[r] = f2h(fmaxf(f[r] * sg + g[r], 0.f));
  }
  *reinterpret_cast<uint4*>(y + off) =
      uint4{o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16)};
}

// The lane checks every lanes entry point shares; out = the caller's lanes with the unused widths zero (the copy
// that goes into the kernel arguments), wmax = the widest lane.
int check_lanes(const ZmiSpkLanes* L, const char* what, ZmiSpkLanes* out, int* wmax) {
  char msg[160];
  *out = ZmiSpkLanes{};
  if (!L || L->n < 1 || L->n > ZMI_SPK_MAX_LANES) {
    snprintf(msg, sizeof(msg), "%s: the lane count must be 1 .. %d", what, ZMI_SPK_MAX_LANES);
    return zmi_fail_msg(msg);
  }
  *wmax = 0;
  for (int l = 0; l < L->n; ++l) {
    if (L->w[l] < 1) {
      snprintf(msg, sizeof(msg), "%s: lane %d has width %d < 1", what, l, L->w[l]);
      return zmi_fail_msg(msg);
    }
    *wmax = L->w[l] > *wmax ? L->w[l] : *wmax;
    out->w[l] = L->w[l];
  }
  out->n = L->n;
  return 0;
}

// With more than one lane, a lane stride covers the widest lane's extent (and keeps an fp16 lane 16-byte aligned).
int check_stride(const ZmiSpkLanes* L, const char* what, const char* buf, int64_t ls, int64_t extent, bool half) {
  if (L->n == 1 || (ls >= extent && !(half && ls % 8))) return 0;
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: lane stride of %s is %lld: the widest lane needs %lld%s", what, buf, (long long)ls,
           (long long)extent, half ? ", in multiples of 8" : "");
  return zmi_fail_msg(msg);
}

template <int NB>
int launch_spk_conv(const SpkConv& a, const ZmiSpkLanes& L, int tiles, hipStream_t s) {
  const int hh = (TH - 1) * a.stride + a.k, hw = (TW - 1) * a.stride + a.k;
  const size_t lds = (size_t)hh * hw * 64 + (size_t)a.k * a.k * 16 * NB * 64;
  if (lds > 96 * 1024 || hh * hw * 4 > PF * NT || a.k * a.k * 16 * NB * 4 > PF * NT)
    return zmi_fail_msg("spk_conv2d: tile too large for the LDS / register staging");
  // the stride-2 3x3 form needs 71 KiB: above the 64 KiB a kernel gets without the opt-in, which is per device.
  // Two host threads may both find the flag clear and both opt in: the call is idempotent.
  static std::atomic<bool> opted[64];
  int dev = 0;
  ZMI_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return zmi_fail_msg("spk_conv2d: device index out of range");
  if (!opted[dev].load(std::memory_order_acquire)) {
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&spk_conv_kernel<NB>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    if (attr != hipSuccess) return zmi_fail(attr, "hipFuncSetAttribute(spk_conv)", __FILE__, __LINE__);
    opted[dev].store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL(spk_conv_kernel<NB>, dim3((unsigned)tiles, (unsigned)(a.Co / (16 * NB)), (unsigned)L.n), dim3(NT),
                     lds, s, a, L);
  ZMI_CHECK(hipGetLastError());
  return 0;
}

ZmiSpkLanes one_lane(int W) {
  ZmiSpkLanes L{};
  L.n = 1;
  L.w[0] = W;
  return L;
}

}  // namespace

extern "C" int zmi_spk_conv2d_tiles(int H, int W, int k, int stride) {
  if (H <= 0 || W <= 0 || (k != 1 && k != 3) || (stride != 1 && stride != 2)) return 0;
  const int ho = conv_out_dim(H, k, stride), wo = conv_out_dim(W, k, stride);
  return ((ho + TH - 1) / TH) * ((wo + TW - 1) / TW);
}

extern "C" int zmi_spk_max_lanes(void) { return ZMI_SPK_MAX_LANES; }

extern "C" int zmi_spk_conv2d_lanes(const void* x, int H, const ZmiSpkLanes* lanes, int Ci, const void* w,
                                    const float* scale, const float* shift, int Co, int k, int stride, int relu,
                                    void* y, float* psum, int64_t ls_x, int64_t ls_y, int64_t ls_psum, void* stream) {
  ZmiSpkLanes L;
  int W = 0;  // the widest lane
  if (check_lanes(lanes, "spk_conv2d", &L, &W)) return -1;
  if (!x || !w || !scale || !shift || !y) return zmi_fail_msg("spk_conv2d: missing buffers");
  if (H <= 0 || Ci <= 0 || Ci % 32 || Co <= 0 || Co % 32)
    return zmi_fail_msg("spk_conv2d: H, W > 0 and Ci, Co multiples of 32 (the Ci = 1 stem is zmi_spk_stem)");
  if ((k != 1 && k != 3) || (stride != 1 && stride != 2)) return zmi_fail_msg("spk_conv2d: k in {1, 3}, stride in {1, 2}");
  if ((long)H * W * (long)(Ci > Co ? Ci : Co) >= (1l << 31)) return zmi_fail_msg("spk_conv2d: tensor too large");
  const int Ho = conv_out_dim(H, k, stride), tiles = zmi_spk_conv2d_tiles(H, W, k, stride);
  if (check_stride(&L, "spk_conv2d", "x", ls_x, (int64_t)H * W * Ci, true) ||
      check_stride(&L, "spk_conv2d", "y", ls_y, (int64_t)Ho * conv_out_dim(W, k, stride) * Co, true) ||
      (psum && check_stride(&L, "spk_conv2d", "psum", ls_psum, (int64_t)tiles * Co, false)))
    return -1;
  const SpkConv a{(const f16_t*)x, H, 0, Ci, (const f16_t*)w, scale, shift, Co, k, stride, Ho, 0, relu, 0, (f16_t*)y,
                  psum, ls_x, ls_y, ls_psum};
  return Co % 64 == 0 ? launch_spk_conv<4>(a, L, tiles, (hipStream_t)stream)
                      : launch_spk_conv<2>(a, L, tiles, (hipStream_t)stream);
}

extern "C" int zmi_spk_conv2d(const void* x, int H, int W, int Ci, const void* w, const float* scale,
                              const float* shift, int Co, int k, int stride, int relu, void* y, float* psum,
                              void* stream) {
  const ZmiSpkLanes L = one_lane(W);
  return zmi_spk_conv2d_lanes(x, H, &L, Ci, w, scale, shift, Co, k, stride, relu, y, psum, 0, 0, 0, stream);
}

extern "C" int zmi_spk_stem_lanes(const void* x, int H, const ZmiSpkLanes* lanes, const void* w, const float* scale,
                                  const float* shift, int Co, void* y, int64_t ls_x, int64_t ls_y, void* stream) {
  ZmiSpkLanes L;
  int W = 0;  // the widest lane
  if (check_lanes(lanes, "spk_stem", &L, &W)) return -1;
  if (!x || !w || !scale || !shift || !y) return zmi_fail_msg("spk_stem: missing buffers");
  if (H <= 0 || Co <= 0 || Co % 8) return zmi_fail_msg("spk_stem: H, W > 0 and Co a multiple of 8");
  const long n = (long)H * W * (Co / 8);
  if (n * 8 >= (1l << 31)) return zmi_fail_msg("spk_stem: tensor too large");
  if (check_stride(&L, "spk_stem", "x", ls_x, (int64_t)H * W, false) ||
      check_stride(&L, "spk_stem", "y", ls_y, n * 8, true))
    return -1;
  hipLaunchKernelGGL(spk_stem_kernel, dim3((unsigned)((n + 255) / 256), 1, (unsigned)L.n), dim3(256), 0,
                     (hipStream_t)stream, (const f16_t*)x, H, L, (const f16_t*)w, scale, shift, Co, (f16_t*)y, ls_x,
                     ls_y);
  ZMI_CHECK(hipGetLastError());
  return 0;
}

extern "C" int zmi_spk_stem(const void* x, int H, int W, const void* w, const float* scale, const float* shift,
                            int Co, void* y, void* stream) {
  const ZmiSpkLanes L = one_lane(W);
  return zmi_spk_stem_lanes(x, H, &L, w, scale, shift, Co, y, 0, 0, stream);
}

extern "C" int64_t zmi_spk_simam_ws_floats(int H, int W, int C) {
  if (H <= 0 || W <= 0 || C <= 0) return 0;
  const int64_t nblk = ((int64_t)H * W + SIMAM_CHUNK - 1) / SIMAM_CHUNK;
  return 2 * (int64_t)C + 2 * nblk * C;
}

extern "C" int zmi_spk_simam_lanes(const void* x, const void* residual, int H, const ZmiSpkLanes* lanes, int C,
                                   const float* psum, const int* n_psum, float* ws, void* y, int64_t ls_x,
                                   int64_t ls_res, int64_t ls_psum, int64_t ls_ws, int64_t ls_y, void* stream) {
  ZmiSpkLanes L;
  int W = 0;  // the widest lane
  if (check_lanes(lanes, "spk_simam", &L, &W)) return -1;
  if (!x || !residual || !ws || !y) return zmi_fail_msg("spk_simam: missing buffers");
  if (H <= 0 || C < 8 || C % 8 || C > SPK_MAX_C || 256 % (C / 8))
    return zmi_fail_msg("spk_simam: H W >= 2 and C in {8, 16, .. 2048} with C / 8 dividing 256");
  if ((long)H * W * C >= (1l << 31)) return zmi_fail_msg("spk_simam: tensor too large");
  if (psum && !n_psum) return zmi_fail_msg("spk_simam: psum without rows");
  const int nblk = (H * W + SIMAM_CHUNK - 1) / SIMAM_CHUNK;  // of the widest lane: the grid, and the ws layout
  SpkRows rows_s{}, rows_d{};  // rows of the sums of x (psum or spart) and of the squared deviations, per lane
  int max_psum = 0;
  for (int l = 0; l < L.n; ++l) {
    if ((long)H * L.w[l] < 2) return zmi_fail_msg("spk_simam: H W >= 2 in every lane");
    rows_d.n[l] = (H * L.w[l] + SIMAM_CHUNK - 1) / SIMAM_CHUNK;
    rows_s.n[l] = psum ? n_psum[l] : rows_d.n[l];
    if (rows_s.n[l] <= 0) return zmi_fail_msg("spk_simam: psum without rows");
    max_psum = rows_s.n[l] > max_psum ? rows_s.n[l] : max_psum;
  }
  const int64_t ext = (int64_t)H * W * C;
  if (check_stride(&L, "spk_simam", "x", ls_x, ext, true) ||
      check_stride(&L, "spk_simam", "residual", ls_res, ext, true) ||
      check_stride(&L, "spk_simam", "y", ls_y, ext, true) ||
      check_stride(&L, "spk_simam", "ws", ls_ws, zmi_spk_simam_ws_floats(H, W, C), false) ||
      (psum && check_stride(&L, "spk_simam", "psum", ls_psum, (int64_t)max_psum * C, false)))
    return -1;
  const hipStream_t s = (hipStream_t)stream;
  float* const mean = ws;                            // [C]
  float* const den = ws + C;                         // [C]
  float* const spart = ws + 2 * (size_t)C;           // [nblk][C] sums of x, when the conv gave none
  float* const dpart = spart + (size_t)nblk * C;     // [nblk][C] sums of squared deviations
  const f16_t* xh = (const f16_t*)x;
  const unsigned nl = (unsigned)L.n;
  const dim3 fin((unsigned)((C + 31) / 32), 1, nl), red((unsigned)nblk, 1, nl);
  if (!psum) {
    hipLaunchKernelGGL(spk_simam_reduce_kernel<false>, red, dim3(256), 0, s, xh, H, L, C, (const float*)nullptr, spart,
                       ls_x, ls_ws);
    ZMI_CHECK(hipGetLastError());
    psum = spart;
    ls_psum = ls_ws;
  }
  hipLaunchKernelGGL(spk_simam_finish_kernel<false>, fin, dim3(256), 0, s, psum, rows_s, C, H, L, mean, ls_psum, ls_ws);
  ZMI_CHECK(hipGetLastError());
  hipLaunchKernelGGL(spk_simam_reduce_kernel<true>, red, dim3(256), 0, s, xh, H, L, C, (const float*)mean, dpart, ls_x,
                     ls_ws);
  ZMI_CHECK(hipGetLastError());
  hipLaunchKernelGGL(spk_simam_finish_kernel<true>, fin, dim3(256), 0, s, (const float*)dpart, rows_d, C, H, L, den,
                     ls_ws, ls_ws);
  ZMI_CHECK(hipGetLastError());
  const long n = (long)H * W * (C / 8);
  hipLaunchKernelGGL(spk_simam_apply_kernel, dim3((unsigned)((n + 255) / 256), 1, nl), dim3(256), 0, s, xh,
                     (const f16_t*)residual, H, L, C, (const float*)mean, (const float*)den, (f16_t*)y, ls_x, ls_res,
                     ls_ws, ls_y);
  ZMI_CHECK(hipGetLastError());
  return 0;
}

extern "C" int zmi_spk_simam(const void* x, const void* residual, int H, int W, int C, const float* psum, int n_psum,
                             float* ws, void* y, void* stream) {
  const ZmiSpkLanes L = one_lane(W);
  return zmi_spk_simam_lanes(x, residual, H, &L, C, psum, &n_psum, ws, y, 0, 0, 0, 0, 0, stream);
}
