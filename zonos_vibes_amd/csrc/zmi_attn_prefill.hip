// Causal prefill attention, gfx950: 16 / G consecutive query positions of one sequence share every K / V tile.
//
// The decode-shaped forms of zmi_attn.hip take one query per (query, kv head) unit: the A operand of their
// MFMAs holds that query's G heads in a 16-row tile (the other 16 - G rows are zeros), and a prefill of S
// positions reads S (S + 1) / 2 keys per (sequence, kv head). Here a workgroup owns (a tile of QT = 16 / G
// consecutive positions of one sequence, kv head): the 16 rows are QT positions x G heads, every K / V byte of
// the tile's keys is read once for all of them, and the workgroup walks the tile's 512-key blocks in order with
// the block recursion's state (acc, l, M) in registers. No workgroup waits on another: no granules, tickets,
// partial buffers or error word.
//
// Arithmetic: the chunked kernel's, bit for bit, for every row (tests/test_gpu_attn_prefill.py compares with
// zmi_attention_variant(variant = 1)). An MFMA output element does not depend on the other rows of its tile, and
// every other step is stated per (row, key) or (row, dim) in zmi_attn_merge.h. For the row at position p:
//   scores   score_tile (the mfma16 chain over dim blocks 0..3) per 16-key sub-tile, * scale; keys > p are -inf;
//   M_j      max over the row's own keys of blocks 0..j;
//   e, l, P  exp_chunk per 128-key chunk (lane L takes keys L and L + 64, wave_sum), P = bf16(e);
//   P.V      per 32-key tile from a zero accumulator, a chunk's 4 tiles summed in tile order, the row's own
//            chunks of the block in chunk order, the row's own blocks by fold_block;
//   out      bf16(acc * (1 / l)).
// A block or chunk that exists for a later row of the tile but not for this one never enters this row's sums.
// One deliberate difference: the decode forms zero V for the keys past the query's position; in a B operand
// shared by QT positions that is only possible past the TILE's last position, which is done (stale cache bytes
// beyond the sequence never enter a product). Keys between a row's position and the tile's last meet P = 0, and
// 0 x V = 0 for every finite V, so the sums keep their bits. A non-finite V at a later position of the same tile
// would reach the earlier rows of that tile (0 x inf = NaN); such a V poisons every later row in any form.
//
// Work split of the 8 waves per block: wave w scores keys 64 w .. 64 w + 63 (two 32-key tiles, as the block
// form); for P.V, wave w takes the 4 tiles of chunk w / 2 and the 64 output dims of half w % 2, so a chunk's
// tile sum stays in registers and the LDS holds one partial per chunk (it reuses the scores' 32 KiB).
#include "zmi_common.h"
#include "zmi_kernels.h"
#include "zmi_attn_merge.h"
#include "zmi_attn_ds.h"

namespace {

using namespace zmi_attn;

constexpr int PNW = 8, PNT = PNW * 64;
constexpr int ROWS = 16;  // rows of the MFMA A tile: QT positions x G heads

struct PrefillArgs {
  const bf16_t* q;
  int ldq;
  const bf16_t* k;
  const bf16_t* v;
  const ZmiAttnSeq* seqs;
  const ZmiAttnTile* tiles;
  int n_seq, hkv, smax;
  float scale;
  bf16_t* out;
  int ldo;
};

template <int G>
__global__ __launch_bounds__(PNT) __attribute__((amdgpu_waves_per_eu(4, 8))) void attn_prefill_kernel(const PrefillArgs a) {
  constexpr int QT = ROWS / G;
  static_assert(ROWS * BLK == CPB * ROWS * HD, "the chunk partials reuse the score image");
  __shared__ __attribute__((aligned(16))) float so[ROWS * BLK];  // scores [row][BLK], then P.V sums [chunk][row][HD]
  __shared__ __attribute__((aligned(16))) bf16_t pb[ROWS][BLK + 8];  // (rows 16 B apart in the banks)
  __shared__ __attribute__((aligned(16))) bf16_t qs[ROWS][HD + 8];
  __shared__ float mrun[ROWS], mold[ROWS], lch[CPB][ROWS];

  const int tile = blockIdx.x / a.hkv, kh = blockIdx.x - tile * a.hkv;
  const ZmiAttnTile tl = a.tiles[tile];
  if ((unsigned)tl.seq >= (unsigned)a.n_seq) return;
  const ZmiAttnSeq sq = a.seqs[tl.seq];
  // the launcher checked the host copy of the table; a device copy that disagrees with it writes nothing
  if (sq.len < 0 || sq.pos0 < 0 || sq.len > a.smax - sq.pos0 || tl.off < 0 || tl.off >= sq.len || sq.q_row0 < 0 ||
      sq.kv_row < 0)
    return;
  const int nq = min(QT, sq.len - tl.off);  // real positions of the tile; the rows past them repeat the last one
  const int p_first = sq.pos0 + tl.off, p_last = p_first + nq - 1;
  const int nb = p_last / BLK + 1;
  const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t >> 6);  // (provably uniform)
  const size_t kvbase = ((size_t)sq.kv_row * a.hkv + kh) * a.smax * HD;
  const bf16_t* kb = a.k + kvbase;
  const bf16_t* vb = a.v + kvbase;
  const size_t qrow0 = (size_t)sq.q_row0 + tl.off;

  // q (A operand: row r = position r / G, head r % G) into LDS once: 16 rows x 256 B, one 16 B piece per thread
  if (t < ROWS * HD / 8) {
    const int r = t >> 4;
    *reinterpret_cast<uint4*>(&qs[r][(t & 15) * 8]) = *reinterpret_cast<const uint4*>(
        a.q + (qrow0 + min(r / G, nq - 1)) * a.ldq + (kh * G + r % G) * HD + (t & 15) * 8);
  }
  // the fold: thread t owns (row (t >> 7) + 4 i, dim t & 127), i < 4
  float acc[4], lrun[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = lrun[i] = 0.f;
  __syncthreads();

  const int t_in = t, p_first_in = p_first, nq_in = nq;
  for (int j = 0; j < nb; ++j) {
    // The lane's indices and the rows' positions are re-derived per block from values the compiler cannot see
    // through: hoisted out of the loop, the ~35 addresses and bounds they feed are held across the K and V^T
    // fragments (64 registers each) and spill.
    int t = t_in, p_first = p_first_in, nq = nq_in;
    asm volatile("" : "+v"(t), "+s"(p_first), "+s"(nq));
    const int lane = t & 63, c16 = lane & 15, h4 = lane >> 4, d = t & (HD - 1);
    // position of A-tile row r (the rows past the tile's real positions repeat the last one and are never stored)
    const auto row_pos = [&](int r) { return p_first + min(r / G, nq - 1); };
    const int key0 = j * BLK;
    const int nkeys = min(BLK, p_last + 1 - key0), last_key = key0 + nkeys - 1;  // the tile's keys in this block
    // ---- scores of this wave's keys (waves wholly past the tile's keys only mask) ----
    f32x4_t st[2][2] = {};
    if (64 * wave < nkeys) {
      uint4 kf[2][2][4];
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          // (uniform base + 32-bit lane offset: one address register per fragment row, not a pointer per load)
          const unsigned key = min(key0 + 32 * (2 * wave + k) + 16 * tt + c16, last_key);
          const unsigned ko = key * HD + 8 * h4;
#pragma unroll
          for (int db = 0; db < 4; ++db) kf[k][tt][db] = *reinterpret_cast<const uint4*>(kb + ko + 32 * db);
        }
      uint4 qf[4];
#pragma unroll
      for (int db = 0; db < 4; ++db) qf[db] = *reinterpret_cast<const uint4*>(&qs[c16][8 * h4 + 32 * db]);
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) st[k][tt] = score_tile(qf, kf[k][tt]);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int key = 32 * (2 * wave + k) + 16 * tt + c16;  // block-local; accumulator: column = key, row = 4 h4 + i
#pragma unroll
        for (int i = 0; i < 4; ++i)
          so[(4 * h4 + i) * BLK + key] = key < row_pos(4 * h4 + i) + 1 - key0 ? st[k][tt][i] * a.scale : -INFINITY;
      }
    __syncthreads();
    // ---- V^T fragments of the wave's chunk and dim half (in flight during the softmax) ----
    const int cc = wave >> 1, dh = wave & 1;
    const bool live = cc * CH < nkeys;  // the chunk holds keys of the tile
    uint4 vf[4][4];
    if (live) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned vo = (unsigned)c16 * a.smax + min(key0 + 32 * (4 * cc + k) + 8 * h4, last_key & ~7);
#pragma unroll
        for (int d4 = 0; d4 < 4; ++d4)
          vf[k][d4] = *reinterpret_cast<const uint4*>(vb + (size_t)(16 * (4 * dh + d4)) * a.smax + vo);
      }
    }
    // ---- M_j per row (a row with no key in this block keeps M_{j-1}) ----
#pragma unroll
    for (int r = wave; r < ROWS; r += PNW) {
      float m = -INFINITY;
#pragma unroll
      for (int i = 0; i < BLK / 64; ++i) m = fmaxf(m, so[r * BLK + lane + 64 * i]);
      m = wave_max(m);
      if (lane == 0) {  // M_{j-1} stays beside M_j for the fold (one value per row, not per thread)
        const float old = j == 0 ? m : mrun[r];
        mold[r] = old;
        mrun[r] = fmaxf(old, m);
      }
    }
    __syncthreads();
    // ---- e, l, P per (chunk, row) ----
    for (int task = wave; task < CPB * ROWS; task += PNW) {
      const int c = task / ROWS, r = task - c * ROWS;
      if (c * CH >= nkeys) break;
      const int nk = row_pos(r) + 1 - key0 - c * CH;
      const float l = exp_chunk(&so[r * BLK + c * CH], &pb[r][c * CH], mrun[r], nk, lane);
      if (lane == 0) lch[c][r] = l;
    }
    __syncthreads();
    // ---- P.V: the chunk's 4 tiles from zero each, summed in tile order (V past the tile's last position zeroed) ----
    if (live) {
      f32x4_t os[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int kbase = 32 * (4 * cc + k) + 8 * h4;
        const uint4 pf = p_frag(pb, c16, kbase);
#pragma unroll
        for (int d4 = 0; d4 < 4; ++d4) {
          const f32x4_t o = pv_tile(pf, v_keep(vf[k][d4], kbase, nkeys));
          os[d4] = k == 0 ? o : os[d4] + o;
        }
      }
#pragma unroll
      for (int d4 = 0; d4 < 4; ++d4)
#pragma unroll
        for (int i = 0; i < 4; ++i) so[(cc * ROWS + 4 * h4 + i) * HD + 16 * (4 * dh + d4) + c16] = os[d4][i];
    }
    __syncthreads();
    // ---- the row's own chunks in chunk order, then the block folded into the running sums ----
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (t >> 7) + 4 * i;
      const int nk = min(BLK, row_pos(r) + 1 - key0);
      if (nk <= 0) continue;  // the row ended in an earlier block
      const int ncb = (nk + CH - 1) / CH;
      float ob = 0.f, lb = 0.f;
      for (int c = 0; c < ncb; ++c) {
        const float o = so[(c * ROWS + r) * HD + d];
        ob = c == 0 ? o : ob + o;
        lb = c == 0 ? lch[0][r] : lb + lch[c][r];
      }
      float mprev = mold[r];
      fold_block(acc[i], lrun[i], mprev, ob, lb, mrun[r], j == 0);
    }
    __syncthreads();  // the next block's scores overwrite so
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (t >> 7) + 4 * i;
    if (r / G < nq)
      a.out[(qrow0 + r / G) * a.ldo + (kh * G + r % G) * HD + (t & (HD - 1))] = (bf16_t)f2bf(acc[i] * (1.0f / lrun[i]));
  }
}

template <int G>
hipError_t launch_prefill(const PrefillArgs& a, unsigned blocks, hipStream_t s) {
  hipLaunchKernelGGL((attn_prefill_kernel<G>), dim3(blocks), dim3(PNT), 0, s, a);
  return hipGetLastError();
}

}  // namespace

extern "C" int zmi_attention_prefill_queries(int hq, int hkv) {
  const int g = hkv > 0 && hq % hkv == 0 ? hq / hkv : 0;
  return g == 1 || g == 2 || g == 4 ? ROWS / g : -1;
}

extern "C" int zmi_attention_prefill(const void* q, int ldq, const void* k_cache, const void* v_cache,
                                     const ZmiAttnSeq* seqs, int n_seq, int64_t n_tiles, const ZmiAttnTile* tiles,
                                     const ZmiAttnSeq* seqs_host, int hq, int hkv, int hd, int smax, void* out, int ldo,
                                     void* stream) {
  if (hd != HD) return zmi_fail_msg("attention_prefill: head_dim must be 128");
  if (smax <= 0 || smax % 8) return zmi_fail_msg("attention_prefill: smax must be a positive multiple of 8");
  const int qt = zmi_attention_prefill_queries(hq, hkv);
  if (qt < 0) return zmi_fail_msg("attention_prefill: hq / hkv must be 1, 2 or 4");
  if (ldq % 8 || ldo % 4) return zmi_fail_msg("attention_prefill: ldq must be a multiple of 8, ldo of 4");
  if (n_seq < 0 || n_tiles < 0) return zmi_fail_msg("attention_prefill: negative n_seq or n_tiles");
  if (n_seq == 0) return 0;
  if (!seqs_host) return zmi_fail_msg("attention_prefill: the host copy of the sequence table is required");
  int64_t want = 0;
  for (int i = 0; i < n_seq; ++i) {
    const ZmiAttnSeq& s = seqs_host[i];
    if (s.len < 0) return zmi_fail_msg("attention_prefill: negative sequence length");
    if (s.pos0 < 0 || s.q_row0 < 0 || s.kv_row < 0) return zmi_fail_msg("attention_prefill: negative row or position");
    if ((int64_t)s.pos0 + s.len > smax) return zmi_fail_msg("attention_prefill: pos0 + len must be <= smax");
    want += (s.len + qt - 1) / qt;
  }
  if (want != n_tiles) return zmi_fail_msg("attention_prefill: n_tiles does not match the sequences' tile count");
  if (n_tiles == 0) return 0;
  if (!q || !k_cache || !v_cache || !seqs || !tiles || !out) return zmi_fail_msg("attention_prefill: null argument");
  if (n_tiles * hkv > 0x7fffffff) return zmi_fail_msg("attention_prefill: grid too large");
  PrefillArgs a{};
  a.q = (const bf16_t*)q;
  a.ldq = ldq;
  a.k = (const bf16_t*)k_cache;
  a.v = (const bf16_t*)v_cache;
  a.seqs = seqs;
  a.tiles = tiles;
  a.n_seq = n_seq;
  a.hkv = hkv;
  a.smax = smax;
  a.scale = 1.0f / sqrtf((float)hd);
  a.out = (bf16_t*)out;
  a.ldo = ldo;
  const unsigned blocks = (unsigned)(n_tiles * hkv);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  switch (hq / hkv) {
    case 1: e = launch_prefill<1>(a, blocks, s); break;
    case 2: e = launch_prefill<2>(a, blocks, s); break;
    default: e = launch_prefill<4>(a, blocks, s); break;
  }
  ZMI_CHECK(e);
  return 0;
}
