// The stand-alone row norms (gfx950), on zmi_rownorm.h's arithmetic: the bits of the GEMV prologues that fuse the same
// norms into the decode step. bf16 rows in, bf16 rows out, k in {512, 1024, 2048, 4096}; a row's bits do not depend
// on M.
//   zmi_layernorm_rows  nn.LayerNorm (norm_f of the backbone plugin, zonos_vibes_amd/backbone.py)
//   zmi_add_layernorm   layer_norm_fn(x, w, b, residual, prenorm=True, residual_in_fp32=False) of the hybrid blocks
//                       (mamba_ssm/ops/triton/layer_norm.py)
//   zmi_gated_rmsnorm   RMSNormGated(norm_before_gate=False, one group) of the Mamba2 mixer
//                       (mamba_ssm/ops/triton/layernorm_gated.py)
#include <type_traits>

#include "zmi_kernels.h"
#include "zmi_rownorm.h"

namespace {

// f(integral_constant<int, k>) for a width the kernels are built for; false for any other
template <class F>
bool for_width(int k, F&& f) {
  switch (k) {
    case 512: f(std::integral_constant<int, 512>{}); return true;
    case 1024: f(std::integral_constant<int, 1024>{}); return true;
    case 2048: f(std::integral_constant<int, 2048>{}); return true;
    case 4096: f(std::integral_constant<int, 4096>{}); return true;
    default: return false;
  }
}

// One wave per row, its parts one after the other (the GEMV prologue spreads the same parts over waves)
template <int K>
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const bf16_t* x, int ldx, int m, const bf16_t* w,
                                                             const bf16_t* b, float eps, bf16_t* out, int ldo) {
  constexpr int NQ = ln_parts(K), CPQ = ln_chunks(K);
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= m) return;
  const bf16_t* xr = x + (size_t)r * ldx;
  uint4 xv[NQ][CPQ], gw[NQ][CPQ], gb[NQ][CPQ];
  float p[NQ];
  // the row, gamma and beta loads all in flight together (one memory round trip, not two)
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int i = 0; i < CPQ; ++i) {
      const int off = ln_chunk_off(K, q, lane, i);
      xv[q][i] = ld_chunk(xr + off);
      gw[q][i] = ld_chunk(w + off);
      gb[q][i] = ld_chunk(b + off);
    }
  auto pass = [&](float mean, bool sq) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < CPQ; ++i) t += ln_chunk_sum(xv[q][i], mean, sq);
      p[q] = wave_sum(t);
    }
    return ln_combine<NQ>(p);
  };
  const float mean = pass(0.f, false) / (float)K;
  const float rstd = 1.0f / sqrtf(pass(mean, true) / (float)K + eps), nbias = -mean * rstd;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int i = 0; i < CPQ; ++i)
      st_chunk(out + (size_t)r * ldo + ln_chunk_off(K, q, lane, i),
               ln_apply(xv[q][i], gw[q][i], gb[q][i], rstd, nbias));
}

// The two hybrid norms: one 256-thread workgroup per row, wave q < ln_parts(K) owns part q (the others idle). The
// row total of the waves' sums t, in every thread: the parts meet in p[NQ] and are combined by ln_combine.
template <int NQ>
__device__ __forceinline__ float row_total(float t, float* p) {
  const int q = threadIdx.x >> 6;
  t = wave_sum(t);
  if ((threadIdx.x & 63) == 0 && q < NQ) p[q] = t;
  __syncthreads();
  return ln_combine<NQ>(p);
}

// hid == nullptr: the residual alone is normalised (and stays as it is)
template <int K>
__global__ __launch_bounds__(256) void add_ln_kernel(const bf16_t* hid, int ldh, bf16_t* res, int ldr,
                                                     const bf16_t* w, const bf16_t* b, float eps, bf16_t* out, int ldo,
                                                     int store_res) {
  constexpr int NQ = ln_parts(K), CPQ = ln_chunks(K);
  __shared__ float part[2][NQ];
  const int r = blockIdx.x, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const bool on = q < NQ, add = hid != nullptr;
  uint4 hv[CPQ], rv[CPQ];
#pragma unroll
  for (int i = 0; i < CPQ; ++i) {
    hv[i] = rv[i] = uint4{0u, 0u, 0u, 0u};
    if (!on) continue;
    const int off = ln_chunk_off(K, q, lane, i);
    rv[i] = ld_chunk(res + (size_t)r * ldr + off);
    if (add) hv[i] = ld_chunk(hid + (size_t)r * ldh + off);
  }
  auto pass = [&](float mean, bool sq) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < CPQ; ++i) t += addln_chunk_sum(hv[i], rv[i], mean, sq, add);  // an idle wave's t is not used
    return row_total<NQ>(t, part[sq]);
  };
  const float mean = pass(0.f, false) / (float)K;
  const float rstd = 1.0f / sqrtf(pass(mean, true) / (float)K + eps);
  if (!on) return;
#pragma unroll
  for (int i = 0; i < CPQ; ++i) {
    const int off = ln_chunk_off(K, q, lane, i);
    const AddLnChunk o = addln_apply(hv[i], rv[i], ld_chunk(w + off), ld_chunk(b + off), mean, rstd, add);
    st_chunk(out + (size_t)r * ldo + off, o.y);
    if (store_res && add) st_chunk(res + (size_t)r * ldr + off, o.s);
  }
}

// z is read as bf16 (the in_proj output); g is kept in registers between the sum and the apply
template <int K>
__global__ __launch_bounds__(256) void gated_rms_kernel(const bf16_t* y, int ldy, const bf16_t* z, int ldz,
                                                        const bf16_t* w, float eps, bf16_t* out, int ldo) {
  constexpr int NQ = ln_parts(K), CPQ = ln_chunks(K);
  __shared__ float part[NQ];
  const int r = blockIdx.x, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const bool on = q < NQ;
  float g[CPQ][8];
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < CPQ; ++i) {
#pragma unroll
    for (int e = 0; e < 8; ++e) g[i][e] = 0.f;
    if (!on) continue;
    const int off = ln_chunk_off(K, q, lane, i);
    const uint4 yv = ld_chunk(y + (size_t)r * ldy + off);
    const uint4 zv = ld_chunk(z + (size_t)r * ldz + off);
    const uint32_t uy[4] = {yv.x, yv.y, yv.z, yv.w}, uz[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) g[i][e] = gate_of(bf2f(uz[e >> 1] >> (16 * (e & 1))));
#pragma unroll
    for (int e = 0; e < 8; ++e) g[i][e] = gate_elem(uy, g[i], e);
    sq = grms_chunk_sq(g[i], sq);
  }
  const float rstd = 1.0f / sqrtf(row_total<NQ>(sq, part) / (float)K + eps);
  if (!on) return;
#pragma unroll
  for (int i = 0; i < CPQ; ++i) {
    const int off = ln_chunk_off(K, q, lane, i);
    st_chunk(out + (size_t)r * ldo + off, grms_apply(g[i], ld_chunk(w + off), rstd));
  }
}

}  // namespace

extern "C" int zmi_layernorm_rows(const void* x, int ldx, int m, int k, const void* w, const void* b, float eps,
                                  void* out, int ldo, void* stream) {
  if (ldx % 8 || ldo % 8) return zmi_fail_msg("layernorm_rows: ldx and ldo must be multiples of 8");
  if (m <= 0) return 0;
  if (!for_width(k, [&](auto kk) {
        hipLaunchKernelGGL(layernorm_rows_kernel<decltype(kk)::value>, dim3((unsigned)((m + 3) / 4)), dim3(256), 0,
                           (hipStream_t)stream, (const bf16_t*)x, ldx, m, (const bf16_t*)w, (const bf16_t*)b, eps,
                           (bf16_t*)out, ldo);
      }))
    return zmi_fail_msg("layernorm_rows: k must be 512, 1024, 2048 or 4096");
  ZMI_CHECK(hipGetLastError());
  return 0;
}

extern "C" int zmi_add_layernorm(const void* hidden, int ldh, void* residual, int ldr, int m, int k, const void* w,
                                 const void* b, float eps, void* out, int ldo, int store_residual, void* stream) {
  if (ldh % 8 || ldr % 8 || ldo % 8) return zmi_fail_msg("add_layernorm: leading dimensions must be multiples of 8");
  if (!residual || !w || !b || !out) return zmi_fail_msg("add_layernorm: missing buffers");
  if (m <= 0) return 0;
  if (!for_width(k, [&](auto kk) {
        hipLaunchKernelGGL(add_ln_kernel<decltype(kk)::value>, dim3((unsigned)m), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)hidden, ldh, (bf16_t*)residual, ldr, (const bf16_t*)w, (const bf16_t*)b, eps,
                           (bf16_t*)out, ldo, store_residual);
      }))
    return zmi_fail_msg("add_layernorm: k must be 512, 1024, 2048 or 4096");
  ZMI_CHECK(hipGetLastError());
  return 0;
}

extern "C" int zmi_gated_rmsnorm(const void* y, int ldy, const void* z, int ldz, int m, int k, const void* w,
                                 float eps, void* out, int ldo, void* stream) {
  if (ldy % 8 || ldz % 8 || ldo % 8) return zmi_fail_msg("gated_rmsnorm: leading dimensions must be multiples of 8");
  if (!y || !z || !w || !out) return zmi_fail_msg("gated_rmsnorm: missing buffers");
  if (m <= 0) return 0;
  if (!for_width(k, [&](auto kk) {
        hipLaunchKernelGGL(gated_rms_kernel<decltype(kk)::value>, dim3((unsigned)m), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)y, ldy, (const bf16_t*)z, ldz, (const bf16_t*)w, eps, (bf16_t*)out, ldo);
      }))
    return zmi_fail_msg("gated_rmsnorm: k must be 512, 1024, 2048 or 4096");
  ZMI_CHECK(hipGetLastError());
  return 0;
}
