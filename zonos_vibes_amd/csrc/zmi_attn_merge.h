// Attention tile steps, chunk partials and their merge: the one statement of the arithmetic every attention
// form runs (zmi_attn.hip, zmi_attn_ds.h, zmi_attn_prefill.hip, zmi_attnblk.hip), so "the chunked kernel's
// arithmetic, operation for operation" is a call and not a copy. Defined here:
//   mfma16, score_tile   the 4-MFMA score chain of one 16-key tile from a zero accumulator (dim blocks 0..3)
//   exp_lane, exp_chunk  e = exp(s - M_j), P = bf16(e), l of one (chunk, head): lane L takes keys L, L + 64
//   v_keep               a V^T fragment with the positions past the key count zeroed
//   p_frag, pv_tile      the P fragment (zero rows past the G heads) and P.V of one 32-key group from zero
//   fold_l, fold_acc, fold_block   one step of the block recursion; ChunkFold: chunk -> block -> running sums
//   mergeN               ChunkFold over a unit's chunk partials in memory (the last-arriving chunk's merge)
//   q_frag_lds, k_row_lds, patch_v_slot   this position's q / K row / V value from staged {q | k | v} bf16 pairs
//
// A query's keys are cut into chunks of CH keys; a 512-key softmax block (the reference CPU
// kernel's kvSplitSize) is CPB chunks. Chunk c of unit u (= query row x kv head) leaves, per
// query head g of the group:
//   o[u][c][g][0..128)  = sum over the chunk's keys of P_k V_k     (fp32)
//   lm[u][c][g]         = {sum over the chunk's keys of e_k, M_j}   (fp32; M_j of the chunk's block)
// The merge is a fixed sequence of fp32 operations (independent of batch and scheduling):
//   per block: ob = o_c0 + o_c0+1 + ...,  lb = l_c0 + l_c0+1 + ...          (chunk order)
//   blocks:    acc = ob_0, l = lb_0;  then l = lb_j + exp(M_{j-1} - M_j) * l,
//              acc = acc * exp(M_{j-1} - M_j) + ob_j                        (reference recursion)
//   out = bf16(acc * (1 / l))
#pragma once
#include "zmi_common.h"

namespace zmi_attn {

constexpr int HD = 128;
constexpr int BLK = 512;  // kvSplitSize of the reference's CPU attention
#ifndef ZMI_ATTN_NWC
#define ZMI_ATTN_NWC 4
#endif
constexpr int NWC = ZMI_ATTN_NWC;  // waves per chunk workgroup (32 keys each); CH fixes the arithmetic
constexpr int CH = 32 * NWC;
constexpr int CPG = CH / 32;  // 32-key groups per chunk (the chunked kernel's waves)
constexpr int CPB = BLK / CH;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float2 ld2(const float* p) { return *reinterpret_cast<const float2*>(p); }

// Chunks of the query at position pos (pos < 0: inactive row, 0 chunks; the fused and whole-query bodies return
// on such a row before they ask).
__device__ __forceinline__ int chunks_of(int pos) { return pos < 0 ? 0 : pos / CH + 1; }
// 32-key groups that hold the nk keys of a query.
__device__ __forceinline__ int groups_of(int nk) { return (nk + 31) >> 5; }

// ---- per-element steps every form built on 32-key tiles shares: one statement of each, so the forms cannot
// drift apart ----

__device__ __forceinline__ f32x4_t mfma16(const uint4& a, const uint4& b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c,
                                                 0, 0, 0);
}

// Scores of one 16-key tile: q fragments (A: row = head) against a key's K fragments (B), dim blocks 0..3 in order
// from a zero accumulator. Column = key c16, rows 4 h4 + i.
__device__ __forceinline__ f32x4_t score_tile(const uint4 (&qf)[4], const uint4 (&kf)[4]) {
  f32x4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int db = 0; db < 4; ++db) s = mfma16(qf[db], kf[db], s);
  return s;
}

// The per-lane part of exp_chunk: e = exp(s - M) and P = bf16(e) of keys lane and lane + 64 of one (chunk, head);
// returns the lane's e[L] + e[L + 64]. s and p point at the chunk's CH scores / probabilities of that head, nk = the
// head's keys in the chunk (<= 0: none).
__device__ __forceinline__ float exp_lane(const float* s, bf16_t* p, float M, int nk, int lane) {
  float l = 0.f;
#pragma unroll
  for (int i = 0; i < CH / 64; ++i) {
    const int kk = lane + 64 * i;
    const float e = kk < nk ? expf(s[kk] - M) : 0.f;
    l += e;
    p[kk] = (bf16_t)f2bf(e);
  }
  return l;
}

// e, P and l of one (chunk, query head), run by one wave: l = wave_sum(exp_lane) in every lane. (A wave that
// interleaves several tasks calls exp_lane for each, then the wave_sums.)
__device__ __forceinline__ float exp_chunk(const float* s, bf16_t* p, float M, int nk, int lane) {
  return wave_sum(exp_lane(s, p, M, nk, lane));
}

// A V^T fragment (8 positions kbase .. kbase + 7 of one dim) with the positions >= nkeys zeroed: stale cache
// bytes past the bound never enter a product.
__device__ __forceinline__ uint4 v_keep(const uint4& v, int kbase, int nkeys) {
  if (kbase + 8 <= nkeys) return v;
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t lo = kbase + 2 * e < nkeys ? 0x0000ffffu : 0u;
    const uint32_t hi = kbase + 2 * e + 1 < nkeys ? 0xffff0000u : 0u;
    w[e] &= lo | hi;
  }
  return uint4{w[0], w[1], w[2], w[3]};
}

// The P fragment of a 32-key group (A: row = head c16, the lane's 8 keys from k8 of the row) out of the P image
// pb[G][..]; rows past the G heads are zeros.
template <int G, int LD>
__device__ __forceinline__ uint4 p_frag(const bf16_t (&pb)[G][LD], int c16, int k8) {
  uint4 pf = uint4{0u, 0u, 0u, 0u};
  if (c16 < G) pf = *reinterpret_cast<const uint4*>(&pb[c16][k8]);
  return pf;
}

// P.V of one 32-key group and one 16-dim column tile, from a zero accumulator (column = dim c16, row = head i).
__device__ __forceinline__ f32x4_t pv_tile(const uint4& pf, const uint4& v) {
  return mfma16(pf, v, f32x4_t{0.f, 0.f, 0.f, 0.f});
}

// One step of the block recursion, the part per head: block sum lb and running maximum mb of block b folded into
// l (mprev = the maximum after block b - 1; first: b == 0). Returns the step's rescale exp(M_{b-1} - M_b) for
// fold_acc (first: none).
__device__ __forceinline__ float fold_l(float& l, float& mprev, float lb, float mb, bool first) {
  float et = 0.f;
  if (first) {
    l = lb;
  } else {
    et = expf(mprev - mb);
    l = lb + et * l;
  }
  mprev = mb;
  return et;
}
// ... and the part per (head, dim): block sum ob folded into acc.
__device__ __forceinline__ void fold_acc(float& acc, float ob, float et, bool first) {
  acc = first ? ob : acc * et + ob;
}
// Both for one (head, dim).
__device__ __forceinline__ void fold_block(float& acc, float& l, float& mprev, float ob, float lb, float mb, bool first) {
  const float et = fold_l(l, mprev, lb, mb, first);
  fold_acc(acc, ob, et, first);
}

// The chunk -> block -> running-sum recursion of N dims of one head (they share l). It takes values: where they
// come from (memory ahead of use, LDS, registers) is each site's own staging.
template <int N = 1>
struct ChunkFold {
  float acc[N] = {}, ob[N] = {}, l = 0.f, lb = 0.f, mprev = 0.f;
  // chunk c of nc, in chunk order: partials oc and l lc into the block sums; the block's last chunk folds it. mb =
  // M_j of c's block (the caller reads it at the block's first chunk).
  __device__ __forceinline__ void add(int c, int nc, const float (&oc)[N], float lc, float mb) {
    const bool head = c % CPB == 0;
#pragma unroll
    for (int i = 0; i < N; ++i) ob[i] = head ? oc[i] : ob[i] + oc[i];
    lb = head ? lc : lb + lc;
    if (c % CPB == CPB - 1 || c == nc - 1) block(ob, lb, mb, c < CPB);
  }
  __device__ __forceinline__ void add(int c, int nc, float oc, float lc, float mb) {
    static_assert(N == 1, "one dim");
    const float o[1] = {oc};
    add(c, nc, o, lc, mb);
  }
  // a whole block's sums at once (the block form's partials)
  __device__ __forceinline__ void block(const float (&ob_)[N], float lb_, float mb, bool first) {
    const float et = fold_l(l, mprev, lb_, mb, first);
#pragma unroll
    for (int i = 0; i < N; ++i) fold_acc(acc[i], ob_[i], et, first);
  }
  __device__ __forceinline__ void block(float ob_, float lb_, float mb, bool first) {
    static_assert(N == 1, "one dim");
    const float o[1] = {ob_};
    block(o, lb_, mb, first);
  }
  __device__ __forceinline__ float out(int i = 0) const { return acc[i] * (1.0f / l); }
};

// Merged output of dims d .. d + N - 1 (N = 2 or 4) of query head g of one unit. o / lm point at the unit's chunk 0;
// g_heads = heads per kv head. Loads are issued for up to MG chunks at a time before any is used. Every dim runs
// the same operations, so every N gives the same bits.
template <int N, int MG>
__device__ __forceinline__ void mergeN(float (&r)[N], const float* o, const float* lm, int nc, int g, int d,
                                       int g_heads) {
  static_assert(N == 2 || N == 4, "one 8- or 16-byte load per chunk");
  const size_t os = (size_t)g_heads * HD, ls = (size_t)g_heads * 2;
  ChunkFold<N> f;
  float mb = 0.f;
  for (int c0 = 0; c0 < nc; c0 += MG) {
    float ov[MG][N];
    float2 lv[MG];
#pragma unroll
    for (int u = 0; u < MG; ++u) {
      const int cc = min(c0 + u, nc - 1);  // clamped loads past the end are never used
      const float* op = o + cc * os + (size_t)g * HD + d;
      if constexpr (N == 4) {
        const float4 v = ld4(op);
        ov[u][0] = v.x, ov[u][1] = v.y, ov[u][2] = v.z, ov[u][3] = v.w;
      } else {
        const float2 v = ld2(op);
        ov[u][0] = v.x, ov[u][1] = v.y;
      }
      lv[u] = ld2(lm + cc * ls + (size_t)g * 2);
    }
#pragma unroll
    for (int u = 0; u < MG; ++u) {
      const int cc = c0 + u;
      if (cc >= nc) continue;  // (a break here would index ov / lv dynamically: scratch)
      if (cc % CPB == 0) mb = lv[u].y;  // first chunk of its block
      f.add(cc, nc, ov[u], lv[u].x, mb);
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = f.out(i);
}

// ---- this position's q, K row and V row as the fused forms stage them in LDS: bf16 pairs {q of the G heads | k |
// v}, HD / 2 words each (q4p = the same area as uint4) ----

// q fragments (A: row = head c16, zero rows past G) of the lane's dims 8 h4 + 32 db; also any [G][HD] bf16 q image
template <int G>
__device__ __forceinline__ void q_frag_lds(uint4 (&qf)[4], const uint4* q4p, int c16, int h4) {
#pragma unroll
  for (int db = 0; db < 4; ++db) qf[db] = c16 < G ? q4p[(c16 * HD + 8 * h4 + 32 * db) >> 3] : uint4{0u, 0u, 0u, 0u};
}

// the K row of pos replaces the fragments of the lane whose key it is
template <int G>
__device__ __forceinline__ void k_row_lds(uint4 (&kf)[4], const uint4* q4p, int h4) {
#pragma unroll
  for (int db = 0; db < 4; ++db) kf[db] = q4p[(G * HD + 8 * h4 + 32 * db) >> 3];
}

// the V value of pos (dim d, from its pair word) into the V^T fragment whose 8 positions kb .. kb + 7 hold pos
__device__ __forceinline__ void patch_v_slot(uint4& v, int kb, int pos, uint32_t pair_word, int d) {
  const int sl = pos - kb, wi = sl >> 1, sh = (sl & 1) * 16;
  const uint32_t val = (d & 1) ? (pair_word >> 16) : (pair_word & 0xffffu);
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e == wi) w[e] = (w[e] & ~(0xffffu << sh)) | (val << sh);
  v = uint4{w[0], w[1], w[2], w[3]};
}

}  // namespace zmi_attn
