// The arithmetic of one GEMV output row, defined once for every launch form (gemv_body and gemm_rows_kernel in
// zmi_gemv_impl.h, the split-K GEMM, the fp8 form, the GEMV roles of zmi_attn_block / zmi_mamba_block), so that a row
// has the same bits whatever launch computes it: a wave's weight-slice loads, its MFMA chain over a k-segment, the
// segment value and its (row, column), the segment sums in wave order; and the block -> (column block, row group) map
// next to its host-side block count.
#pragma once
#include "zmi_common.h"

namespace zmi_gemv {

// DPP row_ror:8 — lane i of each 16-lane row reads lane (i + 8) & 15 of the same row
__device__ __forceinline__ float ror8(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));
}

// Weight-only FP8 (FMT == ZMI_WFMT_FP8, layout M8F8): W[n][k] = 2^e[n] q[n][k] with q OCP E4M3. A 64-k x 8-column
// chunk is 512 B and a lane's 16-byte load holds its 8 weights of chunk 2p (dwords 0, 1) and of chunk 2p + 1 (dwords
// 2, 3), in the k order of M8. The bytes become the bf16 B operand in registers (exact: E4M3 has 3 mantissa bits)
// and the products, the k-segments and the segment order are those of the bf16 form; the column's power of two
// scales its finished fp32 sum before any epilogue sees it. Every step being exact or scale-invariant, the result
// is the bf16 form's on the dequantised weights 2^e q, bit for bit (away from fp32 subnormal sums).
__device__ __forceinline__ uint32_t fp8x2_to_bf16x2(uint32_t d, bool hi) {
  // two E4M3 bytes (the low or the high half of d) -> two fp32 -> their high halves
  const auto f = hi ? __builtin_amdgcn_cvt_pk_f32_fp8((int)d, true) : __builtin_amdgcn_cvt_pk_f32_fp8((int)d, false);
  // v_perm_b32: bytes 2, 3 of f[0] (selectors 2, 3) below bytes 2, 3 of f[1] (selectors 6, 7)
  return __builtin_amdgcn_perm(__float_as_uint(f[1]), __float_as_uint(f[0]), 0x07060302u);
}
__device__ __forceinline__ bf16x8_t fp8x8_to_bf16x8(uint32_t d0, uint32_t d1) {
  const u32x4_t v = {fp8x2_to_bf16x2(d0, false), fp8x2_to_bf16x2(d0, true), fp8x2_to_bf16x2(d1, false),
                     fp8x2_to_bf16x2(d1, true)};
  return __builtin_bit_cast(bf16x8_t, v);
}
// 2^e of column c (0..7) of a group from its 8 int8 exponents; |e| <= 119 (quant.py), so the float is normal
__device__ __forceinline__ float fp8_col_scale(uint2 ex, int c) {
  const uint32_t lo = ex.x, hi = ex.y;  // both read first: a select of the two addresses keeps `ex` in scratch
  const uint32_t w = c < 4 ? lo : hi;
  const int e = (int)(w << (24 - 8 * (c & 3))) >> 24;
  return __uint_as_float((uint32_t)(e + 127) << 23);
}

// ---- weight-slice loads: a lane's NWL 16-byte loads (1 KiB apart), all in flight at once, through one buffer
// descriptor per wave (wave-uniform base = the wave's first chunk, `span` its byte range; lane offset in the VGPR, j KiB
// folded into the instruction, cdna_hip_programming.md T8). POLICY: 2 non-temporal (each weight read once), 0 re-read
// from L2. Layout M8 (zmi_gemv_impl.h); fp8 (M8F8) chunks are 512 B, so a load holds two and NWL = NL / 2.
template <int NWL, int POLICY>
__device__ __forceinline__ void load_weights_m8(const char* base, int span, int lane, u32x4_t (&wf)[NWL]) {
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), (short)0, span, 0x00020000);
#pragma unroll
  for (int j = 0; j < NWL; ++j) wf[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * 16, j * 1024, POLICY);
}
// DN (dense pairs): a wave owns a PAIR of groups and feeds the MFMA a 16-column B operand per k-half: lane l = column
// l & 7 of the pair's group dn_member(l), k = 32 h + 8 (l >> 4) .. + 7 of the chunk, which is M8 lane (l & 7) + 8 h +
// 16 (l >> 4) of that group's chunk (at base + group_off, per lane). wh[h][j] = k-half h of chunk j.
__device__ __forceinline__ int dn_member(int lane) { return (lane >> 3) & 1; }
template <int NL, int POLICY>
__device__ __forceinline__ void load_weights_dn(const char* base, int span, int group_off, int lane,
                                                u32x4_t (&wh)[2][NL]) {
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), (short)0, span, 0x00020000);
  const int vo = group_off + ((lane & 7) + 16 * (lane >> 4)) * 16;
#pragma unroll
  for (int j = 0; j < NL; ++j)
#pragma unroll
    for (int h = 0; h < 2; ++h) wh[h][j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, vo + 128 * h, j * 1024, POLICY);
}

// DN over M8F8 bytes: the same M8 lane of the pair's group, in the 1 KiB fp8 pieces (group_off in fp8 bytes, 512 per
// chunk). The 16 bytes at that lane of piece p are k-half h of chunk 2p (bytes 0..7) and of chunk 2p + 1 (bytes 8..15):
// NL / 2 loads per k-half. raw[h][p] expands to wh[h][2p], wh[h][2p + 1] (expand_fp8).
template <int NL, int POLICY>
__device__ __forceinline__ void load_weights_dn_f8(const char* base, int span, int group_off, int lane,
                                                   u32x4_t (&raw)[2][NL / 2]) {
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), (short)0, span, 0x00020000);
  const int vo = group_off + ((lane & 7) + 16 * (lane >> 4)) * 16;
#pragma unroll
  for (int p = 0; p < NL / 2; ++p)
#pragma unroll
    for (int h = 0; h < 2; ++h) raw[h][p] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, vo + 128 * h, p * 1024, POLICY);
}
// The many-row forms (gemm_rows_kernel, the split-K GEMM) run many row tiles over one weight slice, so they expand
// the landed fp8 pieces ONCE into the bf16 registers the bf16 form holds and run its tile loop unchanged: raw[p] ->
// wf[2p] (dwords 0, 1), wf[2p + 1] (dwords 2, 3), the operands chain_m8<NL, true> builds per tile. Through
// fp8x8_to_bf16x8 (v_cvt_pk_f32_fp8 + v_perm_b32, exact) rather than gfx950's scaled packed fp8 -> bf16 converts: this
// runs once per workgroup, off the tile loop, and stays the conversion every other fp8 form is tested with.
template <int NL>
__device__ __forceinline__ void expand_fp8(const u32x4_t (&raw)[NL / 2], u32x4_t (&wf)[NL]) {
#pragma unroll
  for (int p = 0; p < NL / 2; ++p) {
    wf[2 * p] = __builtin_bit_cast(u32x4_t, fp8x8_to_bf16x8(raw[p][0], raw[p][1]));
    wf[2 * p + 1] = __builtin_bit_cast(u32x4_t, fp8x8_to_bf16x8(raw[p][2], raw[p][3]));
  }
}

// ---- MFMA chain over a wave's k-segment of NL 64-k chunks. `xa`: the lane's A fragment in the LDS rows, row l & 15 of
// the tile (the caller clamps rows past it), k = 8 (l >> 4) .. + 7; chunk j's k-half 0 at xa + 64 j, k-half 1 at + 32.
// Against k-half 0 the tile's columns 0..7 are exact partial sums (acc0), against k-half 1 its columns 8..15 (acc1).
// F8: the raw E4M3 bytes stay in the registers and become the bf16 operand here (every row tile converts them again).
template <int NL, bool F8>
__device__ __forceinline__ void chain_m8(const bf16_t* xa, const u32x4_t (&wf)[F8 ? NL / 2 : NL], f32x4_t& acc0,
                                         f32x4_t& acc1) {
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const uint4 x0 = *reinterpret_cast<const uint4*>(xa + j * 64);
    const uint4 x1 = *reinterpret_cast<const uint4*>(xa + j * 64 + 32);
    bf16x8_t wv;
    if constexpr (F8)
      wv = fp8x8_to_bf16x8(wf[j >> 1][2 * (j & 1)], wf[j >> 1][2 * (j & 1) + 1]);
    else
      wv = __builtin_bit_cast(bf16x8_t, wf[j]);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, x0), wv, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, x1), wv, acc1, 0, 0, 0);
  }
}
// DN: acc0 holds every column's k-half-0 chain and acc1 its k-half-1 chain: the M8 form's products and accumulations
// (a column's MFMA result does not depend on its place in the tile) in half the MFMAs.
template <int NL>
__device__ __forceinline__ void chain_dn(const bf16_t* xa, const u32x4_t (&wh)[2][NL], f32x4_t& acc0, f32x4_t& acc1) {
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const uint4 x0 = *reinterpret_cast<const uint4*>(xa + j * 64);
    const uint4 x1 = *reinterpret_cast<const uint4*>(xa + j * 64 + 32);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, x0), __builtin_bit_cast(bf16x8_t, wh[0][j]),
                                                   acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, x1), __builtin_bit_cast(bf16x8_t, wh[1][j]),
                                                   acc1, 0, 0, 0);
  }
}

// ---- segment value of accumulator element q = k-half 0 + k-half 1 (tile columns 8..15 moved down by DPP, every lane
// active; DN: both in place), and where it belongs: row rb + q of the tile, column c, a real column (`live`) when
// c < 8 (DN: all 16, column c & 7 of the pair's group c >> 3). The caller stores the live values where it keeps its
// segment sums (LDS `red`, split-K `part`), element by element (q a constant of its unrolled loop).
struct SegPos {
  int c, rb;
  bool live;
};
template <bool DN>
__device__ __forceinline__ SegPos segment_pos(int lane) {
  return {lane & 15, (lane >> 4) * 4, DN || (lane & 15) < 8};
}
template <bool DN>
__device__ __forceinline__ float segment_value(const f32x4_t& acc0, const f32x4_t& acc1, int q) {
  return DN ? acc0[q] + acc1[q] : acc0[q] + ror8(acc1[q]);
}

// ---- a group's finished column sum for epilogue(): its segment sums [W][8][RT] in wave (= k) order, then the fp8
// column's power of two (exact)
template <int W, int RT, bool F8 = false>
struct ColSum {
  const float* seg;
  uint2 wexp = {0u, 0u};  // F8: the group's 8 column exponents
  __device__ __forceinline__ float operator()(int c, int r) const {
    float v = seg[c * RT + r];
#pragma unroll
    for (int w = 1; w < W; ++w) v += seg[(w * 8 + c) * RT + r];
    if constexpr (F8) v *= fp8_col_scale(wexp, c);
    return v;
  }
};

// ---- block -> (column block, group of rpw row tiles): the row groups of a column block take block ids 8 apart (one
// XCD, consecutive in dispatch order: they re-read the weights from its L2). Column blocks are padded to a multiple of
// 8: a block whose cb >= n_cb returns before any barrier.
struct BlockPos {
  int cb, rg;
};
__device__ __forceinline__ BlockPos block_pos(int b, int n_rt, int rpw) {
  const int idx = b >> 3, n_rg = (n_rt + rpw - 1) / rpw;
  return {(idx / n_rg) * 8 + (b & 7), idx - (idx / n_rg) * n_rg};
}
inline int64_t block_count(int n_cb, int n_rt, int rpw) { return (int64_t)((n_cb + 7) / 8) * 8 * ((n_rt + rpw - 1) / rpw); }

}  // namespace zmi_gemv
