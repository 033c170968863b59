// Row-norm arithmetic, stated once: nn.LayerNorm (reference _torch.py:62,88,90), mamba-ssm's add + LayerNorm
// (layer_norm_fn prenorm) and RMSNormGated (norm_before_gate=False, one group). Decode runs the norms as GEMV
// prologues (zmi_gemv_impl.h), prefill as stand-alone kernels (zmi_rownorm.hip, the split-K reduce); an utterance is
// prefilled by one form and continued by the other, so both call the chunk functions below and give the same bits.
// Who owns which (row, part), and where the parts' sums meet, is the caller's; the operation order is fixed here
// (-ffp-contract=off: nothing relies on contraction).
#pragma once
#include "zmi_common.h"

// ---- the row partition. A row of K elements is cut into ln_parts(K) contiguous parts, each reduced by one wave:
// lane L owns ln_chunks(K) 8-element chunks of part q, chunk i at element ln_chunk_off(K, q, L, i). fp32 sums: a
// chunk from zero in element order, the chunks of a lane added in order, a DPP wave sum per part, the parts combined
// as (p0 + p1) + (p2 + p3).
__host__ __device__ constexpr int ln_parts(int K) { return K >= 2048 ? 4 : (K >= 1024 ? 2 : 1); }
__host__ __device__ constexpr int ln_chunks(int K) { return K / (512 * ln_parts(K)); }
__host__ __device__ constexpr int ln_chunk_off(int K, int q, int lane, int i) {
  return q * (K / ln_parts(K)) + (lane + 64 * i) * 8;
}
// One chunk, moved as one 128-bit access (a uint4 copied member by member may be split into halves)
__device__ __forceinline__ uint4 ld_chunk(const bf16_t* p) {
  const u32x4_t v = *reinterpret_cast<const u32x4_t*>(p);
  return uint4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ void st_chunk(bf16_t* p, const uint4& v) {
  *reinterpret_cast<u32x4_t*>(p) = u32x4_t{v.x, v.y, v.z, v.w};
}
template <int NQ>
__device__ __forceinline__ float ln_combine(const float* p) {
  if (NQ == 4) return (p[0] + p[1]) + (p[2] + p[3]);
  if (NQ == 2) return p[0] + p[1];
  return p[0];
}

// ---- LayerNorm: two passes (the mean, then the squared deviations)
__device__ __forceinline__ float ln_chunk_sum(const uint4& xv, float mean, bool sq) {
  const uint32_t u[4] = {xv.x, xv.y, xv.z, xv.w};
  float t = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (sq) {
      const float d0 = bf2f(u[j]) - mean, d1 = bf2f(u[j] >> 16) - mean;
      t += d0 * d0 + d1 * d1;
    } else {
      t += bf2f(u[j]) + bf2f(u[j] >> 16);
    }
  }
  return t;
}
// y = bf16((x * rstd - mean * rstd) * w + b) on one 8-element chunk
__device__ __forceinline__ uint4 ln_apply(const uint4& xv, const uint4& gw, const uint4& gb, float rstd, float nbias) {
  uint32_t u[4] = {xv.x, xv.y, xv.z, xv.w};
  const uint32_t uw[4] = {gw.x, gw.y, gw.z, gw.w}, ub[4] = {gb.x, gb.y, gb.z, gb.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float y0 = (bf2f(u[j]) * rstd + nbias) * bf2f(uw[j]) + bf2f(ub[j]);
    const float y1 = (bf2f(u[j] >> 16) * rstd + nbias) * bf2f(uw[j] >> 16) + bf2f(ub[j] >> 16);
    u[j] = f2bf(y0) | (f2bf(y1) << 16);
  }
  return uint4{u[0], u[1], u[2], u[3]};
}

// ---- add + LayerNorm: s = x + residual in fp32 (add = false: the residual alone, a block with no hidden input yet),
// the statistics and ((s - mean) * rstd) * w + b on the fp32 s; bf16(s) is the next block's residual.
// The sum of one chunk of s, or of its squared deviations; pairs added as (a + b), ln_chunk_sum's order
__device__ __forceinline__ float addln_chunk_sum(const uint4& hv, const uint4& rv, float mean, bool sq, bool add = true) {
  const uint32_t h[4] = {hv.x, hv.y, hv.z, hv.w}, r[4] = {rv.x, rv.y, rv.z, rv.w};
  float t = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float s0 = add ? bf2f(h[j]) + bf2f(r[j]) : bf2f(r[j]);
    const float s1 = add ? bf2f(h[j] >> 16) + bf2f(r[j] >> 16) : bf2f(r[j] >> 16);
    if (sq) {
      const float d0 = s0 - mean, d1 = s1 - mean;
      t += d0 * d0 + d1 * d1;
    } else {
      t += s0 + s1;
    }
  }
  return t;
}
struct AddLnChunk {
  uint4 y, s;  // the normalised chunk and bf16(s)
};
__device__ __forceinline__ AddLnChunk addln_apply(const uint4& hv, const uint4& rv, const uint4& gw, const uint4& gb,
                                                  float mean, float rstd, bool add = true) {
  const uint32_t h[4] = {hv.x, hv.y, hv.z, hv.w}, r[4] = {rv.x, rv.y, rv.z, rv.w};
  const uint32_t uw[4] = {gw.x, gw.y, gw.z, gw.w}, ub[4] = {gb.x, gb.y, gb.z, gb.w};
  uint32_t o[4], so[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float s0 = add ? bf2f(h[j]) + bf2f(r[j]) : bf2f(r[j]);
    const float s1 = add ? bf2f(h[j] >> 16) + bf2f(r[j] >> 16) : bf2f(r[j] >> 16);
    const float y0 = ((s0 - mean) * rstd) * bf2f(uw[j]) + bf2f(ub[j]);
    const float y1 = ((s1 - mean) * rstd) * bf2f(uw[j] >> 16) + bf2f(ub[j] >> 16);
    o[j] = f2bf(y0) | (f2bf(y1) << 16);
    so[j] = f2bf(s0) | (f2bf(s1) << 16);
  }
  return {uint4{o[0], o[1], o[2], o[3]}, uint4{so[0], so[1], so[2], so[3]}};
}

// ---- RMSNormGated: gate = z * sigmoid(z), g = y * gate (fp32, y a bf16 value), out = (g * rstd) * w with
// rstd = 1 / sqrt(mean(g^2) + eps); the sum of g^2 runs element by element through a lane's chunks (one accumulator)
__device__ __forceinline__ float gate_of(float z) { return z * (1.0f / (1.0f + expf(-z))); }
__device__ __forceinline__ float gated(float y, float gate) { return y * gate; }
// g of element e of a chunk: y packed bf16, gz its eight fp32 gates
__device__ __forceinline__ float gate_elem(const uint32_t (&y)[4], const float (&gz)[8], int e) {
  return gated(bf2f(y[e >> 1] >> (16 * (e & 1))), gz[e]);
}
__device__ __forceinline__ void load_gate(const float* p, float (&gz)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  gz[0] = a.x; gz[1] = a.y; gz[2] = a.z; gz[3] = a.w; gz[4] = b.x; gz[5] = b.y; gz[6] = b.z; gz[7] = b.w;
}
__device__ __forceinline__ float grms_chunk_sq(const float (&g)[8], float acc) {
#pragma unroll
  for (int e = 0; e < 8; ++e) acc += g[e] * g[e];
  return acc;
}
__device__ __forceinline__ uint4 grms_apply(const float (&g)[8], const uint4& gw, float rstd) {
  const uint32_t uw[4] = {gw.x, gw.y, gw.z, gw.w};
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    o[j] = f2bf((g[2 * j] * rstd) * bf2f(uw[j])) | (f2bf((g[2 * j + 1] * rstd) * bf2f(uw[j] >> 16)) << 16);
  return uint4{o[0], o[1], o[2], o[3]};
}
