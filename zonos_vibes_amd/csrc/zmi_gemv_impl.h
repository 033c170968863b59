// Weight-streaming GEMV / skinny GEMM for the decode step and the prefill, gfx950.
//
// out[m, n] = sum_k A[m, k] * W[n, k]   (nn.Linear, reference zonos/backbone/_torch.py:114-115,147-152,
//                                        heads: zonos/model.py:100-101)
//
// One kernel for every row count M (decode: M = 2 x slots; prefill: M = 2 x prefill length), so a row's result never
// depends on how many rows share the launch (batched output must equal the reference's batch_size=1
// output, model.py:194):
//
//  * a workgroup owns G groups of 8 output columns over the WHOLE K, and a tile of RT rows; W waves per group split K
//    into fixed segments; every lane issues all of its weight loads (NL x 16 B, straight into VGPRs) before it needs
//    the first one. Row tiles of one column block re-read the weights (from L2 when they run together: the block ->
//    tile map puts them on one XCD, consecutive in dispatch order; speed only, never correctness).
//  * the products run on MFMA v_mfma_f32_16x16x32_bf16 with 8 real columns per 16-column tile: lane l of a 1 KiB
//    weight chunk holds column 8g + (l & 7) at k = 64 kc + 32 ((l >> 3) & 1) + 8 (l >> 4) .. +7 (layout "M8",
//    zmi_pack_weight): each chunk costs two MFMAs (k-half 0 / 1) and no lane movement, and a tile carries up to 16 rows
//    for the same cost as one.
//  * fixed reduction order, independent of M and of the tile a row lands in: per wave a chain of MFMAs over its
//    k-segment, their sum, then the W segment sums in wave order (the row arithmetic, zmi_gemv_row.h).
//  * optional LayerNorm prologue (nn.LayerNorm, _torch.py:62,88,90): (row, part) tasks over the waves, fp32 two-pass
//    statistics, bf16-rounded output, the same arithmetic for every row.
//  * fused epilogues: bf16 store, residual add, RoPE + KV-cache write, SwiGLU, logits, raw f32.
#pragma once
#include <algorithm>
#include "zmi_common.h"
#include "zmi_kernels.h"
#include "zmi_gemv_row.h"
#include "zmi_rownorm.h"

namespace zmi_gemv {

constexpr int PRO_PLAIN = 0, PRO_LN = 1, PRO_ADDLN = 2, PRO_GRMS = 3;
// GRMSG: RMSNormGated from aux rows that already hold g = y * gate (f32): no y rows staged (zmi_mamba_block's step
// writes g; the same bits as GRMS, one third fewer activation bytes per workgroup)
constexpr int PRO_GRMSG = 4;
constexpr size_t LDS_MAX = 160 * 1024;  // gfx950 LDS per workgroup

__device__ __forceinline__ void dma_piece(const bf16_t* gsrc, bf16_t* ldp) {
  // one 1 KiB LDS-DMA piece (64 lanes x 16 B, lane-linear). Inline asm: the compiler does not
  // count it, so the covering wait is the explicit vmcnt after the weight loads
  // (cdna_hip_programming.md §5.7).
  const unsigned ldst =
      __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) void*)ldp);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(ldst)
               : "memory");
}

// LDS image: rows of x at a stride of K + 8 bf16 (2K + 16 bytes: the 16 rows of an MFMA
// A-fragment read fall on distinct 16-byte bank slots), the aux rows (ADDLN residual / GRMS z) at the
// same stride, gamma (/ beta), then the segment sums. Img owns the layout: the host sizes the launch (bytes) and the
// kernel carves its pointers (View) from the same byte offsets, for `rows` staged rows and prologue `pro`.
template <int K>
struct Img {
  static constexpr int XROW = K + 8, GROW = K + 8;  // bf16 x / aux rows; f32 gate rows (GRMS)
  __host__ __device__ static constexpr bool grms(int pro) { return pro == PRO_GRMS || pro == PRO_GRMSG; }
  __host__ __device__ static constexpr size_t aux_off(int rows) { return (size_t)rows * XROW * 2; }
  __host__ __device__ static constexpr size_t gamma_off(int rows, int pro) {
    return aux_off(rows) + (size_t)rows * (pro == PRO_ADDLN ? XROW * 2 : (grms(pro) ? GROW * 4 : 0));
  }
  __host__ __device__ static constexpr size_t red_off(int rows, int pro) {  // after gamma (+ beta)
    return gamma_off(rows, pro) + (size_t)K * ((pro == PRO_LN || pro == PRO_ADDLN) ? 4 : (grms(pro) ? 2 : 0));
  }
  __host__ __device__ static constexpr size_t bytes(int rows, int nwv, int rt, int pro) {
    return red_off(rows, pro) + (size_t)nwv * 8 * rt * 4;
  }
  // x rows; aux rows (xa: ADDLN bf16 residual, xg: the same bytes as GRMS f32 gate / g rows); gamma; beta; segment sums
  struct View {
    bf16_t *xs, *xa, *gam, *bet;
    float *xg, *red;
  };
  __device__ static View carve(char* smem, int rows, int pro) {
    char *aux = smem + aux_off(rows), *gamma = smem + gamma_off(rows, pro);
    return {reinterpret_cast<bf16_t*>(smem), reinterpret_cast<bf16_t*>(aux), reinterpret_cast<bf16_t*>(gamma),
            reinterpret_cast<bf16_t*>(gamma) + K, reinterpret_cast<float*>(aux),
            reinterpret_cast<float*>(smem + red_off(rows, pro))};
  }
};
template <int K>
using View = typename Img<K>::View;

// Diagnostic build only (-DZMI_GEMV_STAMPS, tools/gemv_stamps.py): thread 0 of every workgroup
// writes s_memrealtime (100 MHz) at phase boundaries into diag[reserved][block][8].
#ifdef ZMI_GEMV_STAMPS
#define ZMI_GSTAMP(i)                                                                              \
  do {                                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                                             \
    if (threadIdx.x == 0 && a.diag)                                                                \
      reinterpret_cast<unsigned long long*>(a.diag)[((size_t)a.reserved * 4096 + blockIdx.x) * 8 + (i)] = \
          __builtin_amdgcn_s_memrealtime();                                                        \
    __builtin_amdgcn_sched_barrier(0);                                                             \
  } while (0)
#else
#define ZMI_GSTAMP(i) \
  do {                \
  } while (0)
#endif

// In-launch hand-off of the QKV projection to the attention workgroups of zmi_attn_block
// (zmi_attnblk.hip): every bf16 pair of q and of this step's K / V rows is ALSO stored as an 8-byte
// {pair, tag = position + 1} granule (one sc1 store: the data is its own flag, cdna_hip_programming.md
// §6 Guideline 16 R2), so the consumer needs no counter and nothing is re-armed.
// Per query row and kv head the granule area holds QKV_GRAN words: q of the G heads (G HD / 2 pairs),
// then k (HD / 2) and v (HD / 2); the score granules follow (zmi_attnblk.hip).
struct QkvFuse {
  uint64_t* gran;   // [M][hkv][gran_stride] u64
  int gran_stride;
  // FUSE == 3 (zmi_attn_block's out_proj role): the GEMV's activation rows are the attention output, gathered
  // from the units' output granules (word og_off of a unit's area: 256 {bf16 pair, tag} words, dims in order)
  // once the unit's 8 merge-workgroup flags (word of_off + c: {0, tag}) carry the row's tag (position + 1)
  int og_off = 0, of_off = 0, hkv = 0;
  const int* pos = nullptr;
  unsigned* err = nullptr;
  // FUSE == 2 (zmi_mamba_block's in_proj role): granules of columns < l2_cols are stored workgroup-scope, kept in
  // the XCD's L2 for a step workgroup on the same XCD (st_xc64); the others write through
  int l2_cols = 0;
};

// the RoPE cos / sin pair of q or k column n (an even column below (hq + hkv) hd) at position q_pos
__device__ __forceinline__ const float2* rope_pair(const ZmiGemvArgs& a, int q_pos, int n) {
  const int qcols = a.hq * a.hd, d = (n < qcols ? n : n - qcols) % a.hd;
  return reinterpret_cast<const float2*>(a.rope + ((size_t)q_pos * (a.hd >> 1) + (d >> 1)) * 2);
}

// (6) fused epilogues of one group's 8 columns over a row tile, run by one wave; colsum(c, r) = the
// group's finished column sum (ColSum). Shared by every launch form (gemv_body, gemm_rows_kernel): the same bits.
template <int EPI, int RT, int FUSE, class Sum>
__device__ __forceinline__ void epilogue(const ZmiGemvArgs& a, const Sum& colsum, int lane, int rows, int row0,
                                         int g, const uint32_t (&res_pre)[(8 * RT + 63) / 64], int q_pos, int q_kvr,
                                         const QkvFuse& fz, unsigned act_rows = ~0u, const float2* rope_pre = nullptr) {
  constexpr int NE = (8 * RT + 63) / 64;
  const int col0 = g * 8;
  if (EPI == ZMI_EPI_STORE && FUSE == 2) {
    // plain bf16 store, and every column pair of an active row also goes out as an 8-byte {pair,
    // tag = position + 1} granule (zmi_mamba_block's step role reads the in_proj output from these)
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = lane + 64 * i, r = e >> 3, c = e & 7, n = col0 + c;
      const bool ok = r < rows && n < a.n_valid;
      const uint32_t hv = ok ? f2bf(colsum(c, r)) : 0u;
      const uint32_t nb = (uint32_t)__shfl_down((int)hv, 1);
      if (ok) {
        const size_t m = (size_t)(row0 + r);
        reinterpret_cast<bf16_t*>(a.out)[m * a.ldo + n] = (bf16_t)hv;
        const int pos = a.row_pos[m];
        if ((c & 1) == 0 && pos >= 0)
          st_xc64(fz.gran + m * fz.gran_stride + (n >> 1), (uint64_t)(hv | (nb << 16)) | ((uint64_t)(unsigned)(pos + 1) << 32),
                  n < fz.l2_cols);
      }
    }
  } else if (EPI == ZMI_EPI_STORE || EPI == ZMI_EPI_RESIDUAL || EPI == ZMI_EPI_F32 || EPI == ZMI_EPI_LOGITS) {
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = lane + 64 * i, r = e >> 3, c = e & 7, n = col0 + c;
      if (r >= rows || n >= a.n_valid || !((act_rows >> r) & 1u)) continue;  // act_rows: FUSE 3's rows with pos >= 0
      const float v = colsum(c, r);
      const size_t m = (size_t)(row0 + r);
      if (EPI == ZMI_EPI_F32) {
        reinterpret_cast<float*>(a.out)[m * a.ldo + n] = v;
      } else if (EPI == ZMI_EPI_STORE) {
        reinterpret_cast<bf16_t*>(a.out)[m * a.ldo + n] = (bf16_t)f2bf(v);
      } else if (EPI == ZMI_EPI_RESIDUAL) {
        // x + bf16(linear(x))  (_torch.py:100-101)
        reinterpret_cast<bf16_t*>(a.out)[m * a.ldo + n] = (bf16_t)f2bf(bf2f(res_pre[i]) + bfround(v));
      } else {
        // 9 heads back to back, 1026 columns each (1025 real + the zero pad row)
        const int cbk = n / 1026, vv = n - cbk * 1026;
        reinterpret_cast<float*>(a.out)[(m * 9 + cbk) * 1026 + vv] = bfround(v);
      }
    }
  } else if (EPI == ZMI_EPI_SWIGLU) {
    // M8 SwiGLU packing: columns 0..3 = value rows 4g.., 4..7 = gate rows F + 4g..  (_torch.py:150-152)
    const int r = lane >> 2, c = lane & 3;
    if (r < rows) {
      const float y = bfround(colsum(c, r));
      const float gt = bfround(colsum(c + 4, r));
      const float sg = bfround(gt / (1.0f + expf(-gt)));
      reinterpret_cast<bf16_t*>(a.out)[(size_t)(row0 + r) * a.ldo + g * 4 + c] = (bf16_t)f2bf(y * sg);
    }
  } else if (EPI == ZMI_EPI_QKV) {
    // q | k | v split, interleaved-pair RoPE in fp32 on q and k, KV-cache write (_torch.py:18-49,117-126)
    const int r = lane >> 2, c = (lane & 3) * 2;
    if (r < rows && q_pos >= 0 && q_pos < a.smax) {  // the launchers check positions against smax; never write past it
      const int n = col0 + c;
      const int qcols = a.hq * a.hd, kcols = a.hkv * a.hd;
      float x0 = bfround(colsum(c, r)), x1 = bfround(colsum(c + 1, r));
      if (n < qcols + kcols) {
        // rope_pre: the cos / sin pair loaded by the caller before its LayerNorm (a load here is a memory round trip on
        // the decode step's critical path)
        const float2 cs = rope_pre ? *rope_pre : *rope_pair(a, q_pos, n);
        const float co = cs.x, si = cs.y;
        const float r0 = x0 * co - x1 * si;
        const float r1 = x1 * co + x0 * si;
        x0 = r0;
        x1 = r1;
      }
      const uint32_t packed = f2bf(x0) | (f2bf(x1) << 16);
      int gkh = 0, gslot = 0;  // granule of this pair (FUSE)
      if (n < qcols) {
        *reinterpret_cast<uint32_t*>(reinterpret_cast<bf16_t*>(a.out) + (size_t)(row0 + r) * a.ldo + n) = packed;
        const int gq = a.hq / a.hkv;
        gkh = n / (gq * a.hd);
        gslot = (n - gkh * gq * a.hd) >> 1;
      } else if (n < qcols + kcols) {  // K cache [row][kv head][position][hd]
        const int nn = n - qcols, kh = nn / a.hd, d = nn - kh * a.hd;
        const size_t o = (((size_t)q_kvr * a.hkv + kh) * a.smax + q_pos) * a.hd + d;
        *reinterpret_cast<uint32_t*>(reinterpret_cast<bf16_t*>(a.k_cache) + o) = packed;
        gkh = kh;
        gslot = (a.hq / a.hkv) * (a.hd >> 1) + (d >> 1);
      } else {  // V cache, transposed: [row][kv head][hd][position] (zmi_attn.hip's P.V operand)
        const int nn = n - qcols - kcols, kh = nn / a.hd, d = nn - kh * a.hd;
        bf16_t* vt = reinterpret_cast<bf16_t*>(a.v_cache) + (((size_t)q_kvr * a.hkv + kh) * a.hd + d) * a.smax + q_pos;
        vt[0] = (bf16_t)(packed & 0xffffu);
        vt[a.smax] = (bf16_t)(packed >> 16);
        gkh = kh;
        gslot = (a.hq / a.hkv + 1) * (a.hd >> 1) + (d >> 1);
      }
      if (FUSE)
        st_wt64(fz.gran + ((size_t)(row0 + r) * a.hkv + gkh) * fz.gran_stride + gslot,
                (uint64_t)packed | ((uint64_t)(unsigned)(q_pos + 1) << 32));
    }
  }
}

// ---- The phases of gemv_body, in the order it runs them: what each needs on entry and what it leaves.
// (1) Activation staging: the tile's x rows (GRMSG: none), its aux rows (ADDLN residual / GRMS gate) and, for the
// workgroup's first tile, gamma / beta, into the LDS image by DMA, 1 KiB pieces spread over the waves. Entry: no wave
// still reads the image. Leaves: uncounted LDS-DMA loads in flight; the caller's next vmcnt wait, then a barrier.
template <int K, int PRO, int NWV>
__device__ __forceinline__ void stage_rows(const ZmiGemvArgs& a, const View<K>& L, int wave, int lane,
                                           bool first, int s_row0, int s_rows) {
  constexpr int XROW = Img<K>::XROW, GROW = Img<K>::GROW;
  constexpr bool GRMS = Img<K>::grms(PRO), AUX = PRO == PRO_ADDLN || GRMS;
  constexpr int GB = (PRO == PRO_LN || PRO == PRO_ADDLN) ? 2 : (GRMS ? 1 : 0);  // gamma / beta rows
  constexpr int PPR = K / 512;
  const int n_x = PRO == PRO_GRMSG ? 0 : s_rows * PPR;  // GRMSG: no y rows
  constexpr int APR = GRMS ? 2 * PPR : PPR;  // aux pieces per row (f32 gate rows: twice the bytes)
  const int n_a = AUX ? s_rows * APR : 0;
  const int n_pc = n_x + n_a + (first ? GB * PPR : 0);
  const bf16_t* s_X = reinterpret_cast<const bf16_t*>(a.X) + (size_t)s_row0 * a.ldx;
  const bf16_t* XA = AUX ? reinterpret_cast<const bf16_t*>(a.aux) + (size_t)s_row0 * a.ld_aux * (GRMS ? 2 : 1)
                         : nullptr;
  for (int pc = wave; pc < n_pc; pc += NWV) {
    if (pc < n_x) {
      const int r = pc / PPR, p = pc - r * PPR;
      dma_piece(s_X + (size_t)r * a.ldx + p * 512 + lane * 8, L.xs + r * XROW + p * 512);
    } else if (pc < n_x + n_a) {
      const int r = (pc - n_x) / APR, p = (pc - n_x) - r * APR;
      if (GRMS)  // 1 KiB = 256 f32 of the gate (GRMSG: g) row
        dma_piece(XA + ((size_t)r * a.ld_aux + p * 256) * 2 + lane * 8,
                  reinterpret_cast<bf16_t*>(L.xg + r * GROW + p * 256));
      else
        dma_piece(XA + (size_t)r * a.ld_aux + p * 512 + lane * 8, L.xa + r * XROW + p * 512);
    } else {
      const int q = pc - n_x - n_a, which = q / PPR, p = q - which * PPR;
      const bf16_t* src = reinterpret_cast<const bf16_t*>(which ? a.ln_b : a.ln_w);
      dma_piece(src + p * 512 + lane * 8, (which ? L.bet : L.gam) + p * 512);
    }
  }
}

// (1b) Epilogue-operand staging: the epilogue inputs that need no other load (residual inputs, or the rows' positions
// and cache rows) into registers of the group's epilogue wave `ew`. Leaves: counted loads, older than the weight stream.
template <int EPI, int RT>
__device__ __forceinline__ void stage_epilogue_operands(const ZmiGemvArgs& a, bool ew, int lane, int rows, int row0,
                                                        int col0, uint32_t (&res_pre)[(8 * RT + 63) / 64], int& q_pos,
                                                        int& q_kvr) {
  constexpr int NE = (8 * RT + 63) / 64;
#pragma unroll
  for (int i = 0; i < NE; ++i) res_pre[i] = 0;
  q_pos = -1, q_kvr = 0;
  if (EPI == ZMI_EPI_RESIDUAL && ew) {
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = lane + 64 * i, r = e >> 3, n = col0 + (e & 7);
      if (r < rows && n < a.n_valid)
        res_pre[i] = reinterpret_cast<const bf16_t*>(a.out)[(size_t)(row0 + r) * a.ldo + n];
    }
  }
  if (EPI == ZMI_EPI_QKV && ew && (lane >> 2) < rows) {
    q_pos = a.row_pos[row0 + (lane >> 2)];
    q_kvr = a.row_kv[row0 + (lane >> 2)];
  }
}

// (1') FUSE 3 (zmi_attn_block's out_proj role): the activation rows are the attention output, gathered from the
// units' output granules instead of staged by DMA. Layout as zmi_attnblk.hip passes it in QkvFuse: a unit = (row, kv
// head), 256 {bf16 pair, tag} words per unit at og_off (4 heads x 128 dims = 512 columns of K: the attention block
// checks hq = 4 hkv, hd = 128), 8 merge-workgroup flags per unit at of_off, tag = position + 1.
// Entry: every wave (two barriers inside); the weight stream may be in flight; `qpos` is the segment-sum area. Leaves:
// the rows in LDS (position < 0: zero rows), visible after the tile barrier. Returns the mask of rows with position >= 0.
template <int K, int NWV>
__device__ __forceinline__ unsigned gather_attention_rows(const ZmiGemvArgs& a, const QkvFuse& fz, bf16_t* xs, int* qpos,
                                                          int rows, int row0, int tid) {
  constexpr int XROW = Img<K>::XROW;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the rows' positions (tags) in LDS first: every later check reads them without a dependent global load
  if (tid < rows) qpos[tid] = fz.pos[row0 + tid];
  __syncthreads();
  unsigned act_rows = 0u;
  for (int r = 0; r < rows; ++r) act_rows |= (qpos[r] >= 0 ? 1u : 0u) << r;
  // wave 0 polls the merge workgroups' flags of the launch's units (rows whose position is < 0 run no attention and
  // contribute zero rows), sleeping between sweeps, until ANY unit has a flag up: the merges finish within ~0.4 us of
  // each other (64 cheap flags instead of 2048 granules while the attention runs; a granule published after a sweep
  // is picked up by the next one). Waiting for every unit's flag measured C2 step 922 us, no flag wait 908, this form
  // 902-904 (profiles/r06_oproj_flag_wait_ab.jsonl).
  const int n_units = rows * fz.hkv;
  if (wave == 0) {
    for (unsigned spins = 0;; ++spins) {
      bool ok = false;
      for (int u0 = 0; u0 < n_units; u0 += 8) {  // lane = (unit u0 + lane / 8, merge workgroup lane % 8)
        const int u = u0 + (lane >> 3), qp = u < n_units ? qpos[u / fz.hkv] : -1;
        const bool up = qp < 0 || (uint32_t)(ld_wt64(fz.gran + (size_t)(row0 * fz.hkv + u) * fz.gran_stride + fz.of_off +
                                                        (lane & 7)) >> 32) == (uint32_t)qp + 1u;
        // any flag of the unit: OR over the 8 lanes of the unit (DPP within each 8-lane group)
        float f = up ? 1.f : 0.f;
        f = fmaxf(f, dpp_mov<DPP_XOR1>(f));
        f = fmaxf(f, dpp_mov<DPP_XOR2>(f));
        f = fmaxf(f, dpp_mov<DPP_HALF_MIRROR>(f));
        ok = ok || (u < n_units && f > 0.f);
      }
      if (__any(ok)) break;
      if (spins > (1u << 18)) {
        if (lane == 0) __hip_atomic_store(fz.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
  }
  ZMI_GSTAMP(7);
  __syncthreads();
  // every thread polls its own granules of the units' outputs (unit (r, kh), pair j: dims kh hq/hkv hd + 2 j, + 1 of
  // row r) until each carries its row's tag, then writes them into the LDS rows. GPT granules per thread per batch
  // (2 rows x 4 kv heads: one batch), every load of a sweep issued before the first check, s_sleep 1 between sweeps.
  constexpr int GPT = 4;
  for (int e0 = tid; e0 < n_units * 256; e0 += GPT * NWV * 64) {
    uint64_t gv[GPT];
    int gq[GPT];
    unsigned need = 0;
#pragma unroll
    for (int i = 0; i < GPT; ++i) {
      const int e = e0 + NWV * 64 * i;
      gq[i] = e < n_units * 256 ? qpos[(e >> 8) / fz.hkv] : -1;
      gv[i] = 0ull;
      if (gq[i] >= 0) need |= 1u << i;
    }
    for (unsigned spins = 0; need; ++spins) {
#pragma unroll
      for (int i = 0; i < GPT; ++i)
        if ((need >> i) & 1)
          gv[i] = ld_wt64(fz.gran + (size_t)(row0 * fz.hkv + ((e0 + NWV * 64 * i) >> 8)) * fz.gran_stride + fz.og_off +
                          ((e0 + NWV * 64 * i) & 255));
#pragma unroll
      for (int i = 0; i < GPT; ++i)
        if (((need >> i) & 1) && (uint32_t)(gv[i] >> 32) == (uint32_t)gq[i] + 1u) need &= ~(1u << i);
      if (!need) break;
      if (spins > (1u << 18)) {
        __hip_atomic_store(fz.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int i = 0; i < GPT; ++i) {
      const int e = e0 + NWV * 64 * i;
      if (e < n_units * 256) {
        const int u = e >> 8, j = e & 255, r = u / fz.hkv, kh = u - r * fz.hkv;
        *reinterpret_cast<uint32_t*>(xs + r * XROW + kh * 512 + 2 * j) = gq[i] >= 0 ? (uint32_t)gv[i] : 0u;
      }
    }
  }
  return act_rows;
}

// (3) The normalisation prologues (zmi_rownorm.h arithmetic): task (row, part) per wave, so the few rows of a decode
// step use every wave; partial sums meet in the segment-sum area `part` (free until the MFMA chain); each pass re-reads
// its chunks from LDS (no row copy in VGPRs: the weight slice in flight already holds 4 NL of them, and occupancy
// decides whether every workgroup of a wide GEMV is resident at once). One wave per row with no barriers between the
// passes measured slower: C2 step 1001 vs 973 us.
// Entry: every wave, after the tile barrier. Each ends with a barrier: the normalised bf16 rows visible, `part` free.
// The fp32 two-pass statistics of LayerNorm and (ADD) add+LayerNorm: part[r NQ + q] = the sum of part q of row r,
// part[RT NQ + r NQ + q] = the sum of its squared deviations from the row mean; a chunk's sum is ln_chunk_sum of x or
// addln_chunk_sum of x + aux. A workgroup barrier after each pass.
template <int K, int RT, int NWV, bool ADD>
__device__ __forceinline__ void ln_statistics(const ZmiGemvArgs& a, const View<K>& L, int rows, int wave, int lane) {
  constexpr int XROW = Img<K>::XROW, NQ = ln_parts(K), CPQ = ln_chunks(K);
  float* part = L.red;
  const int ntask = rows * NQ;
  auto pass = [&](int task, float mean, bool sq) {
    const int r = task / NQ, q = task - r * NQ;
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < CPQ; ++i) {
      const int off = r * XROW + ln_chunk_off(K, q, lane, i);
      const uint4 xv = ld_chunk(L.xs + off);
      if constexpr (ADD)
        t += addln_chunk_sum(xv, ld_chunk(L.xa + off), mean, sq);
      else
        t += ln_chunk_sum(xv, mean, sq);
    }
    return wave_sum(t);
  };
  for (int task = wave; task < ntask; task += NWV) {
    const float v = pass(task, 0.f, false);
    if (lane == 0) part[task] = v;
  }
  __syncthreads();
#if defined(ZMI_LN_STAMP) && ZMI_LN_STAMP == 1  // diagnostic builds only (tools/build_attnblk_stamps.sh)
  ZMI_GSTAMP(7);
#endif
  for (int task = wave; task < ntask; task += NWV) {
    const float mean = ln_combine<NQ>(part + (task / NQ) * NQ) / (float)K;
    const float v = pass(task, mean, true);
    if (lane == 0) part[RT * NQ + task] = v;
  }
  __syncthreads();
#if defined(ZMI_LN_STAMP) && ZMI_LN_STAMP == 2
  ZMI_GSTAMP(7);
#endif
}

// LayerNorm (nn.LayerNorm): x * rstd + nbias through ln_apply, in place
template <int K, int RT, int NWV>
__device__ __forceinline__ void prologue_layernorm(const ZmiGemvArgs& a, const View<K>& L, int rows, int wave, int lane) {
  constexpr int XROW = Img<K>::XROW, NQ = ln_parts(K), CPQ = ln_chunks(K);
  ln_statistics<K, RT, NWV, false>(a, L, rows, wave, lane);  // L.red: the parts' sums, then their squared deviations
  for (int task = wave; task < rows * NQ; task += NWV) {
    const int r = task / NQ, q = task - r * NQ;
    const float mean = ln_combine<NQ>(L.red + r * NQ) / (float)K;
    const float rstd = 1.0f / sqrtf(ln_combine<NQ>(L.red + RT * NQ + r * NQ) / (float)K + a.eps), nbias = -mean * rstd;
#pragma unroll
    for (int i = 0; i < CPQ; ++i) {
      const int off = ln_chunk_off(K, q, lane, i);
      bf16_t* xp = L.xs + r * XROW + off;
      st_chunk(xp, ln_apply(ld_chunk(xp), ld_chunk(L.gam + off), ld_chunk(L.bet + off), rstd, nbias));
    }
  }
  __syncthreads();
}

// layer_norm_fn prenorm: s = x + residual (fp32), LayerNorm(s) with ((s - mean) rstd) w + b, in place over x; with
// `wres` (the column block 0 workgroup of each row tile) bf16(s) also goes to res_out, the next block's residual
template <int K, int RT, int NWV>
__device__ __forceinline__ void prologue_add_layernorm(const ZmiGemvArgs& a, const View<K>& L, int rows,
                                                       int row0, bool wres, int wave, int lane) {
  constexpr int XROW = Img<K>::XROW, NQ = ln_parts(K), CPQ = ln_chunks(K);
  ln_statistics<K, RT, NWV, true>(a, L, rows, wave, lane);  // L.red: the parts' sums, then their squared deviations
  for (int task = wave; task < rows * NQ; task += NWV) {
    const int r = task / NQ, q = task - r * NQ;
    const float mean = ln_combine<NQ>(L.red + r * NQ) / (float)K;
    const float rstd = 1.0f / sqrtf(ln_combine<NQ>(L.red + RT * NQ + r * NQ) / (float)K + a.eps);
#pragma unroll
    for (int i = 0; i < CPQ; ++i) {
      const int off = ln_chunk_off(K, q, lane, i);
      bf16_t* hp = L.xs + r * XROW + off;
      const AddLnChunk o = addln_apply(ld_chunk(hp), ld_chunk(L.xa + r * XROW + off), ld_chunk(L.gam + off),
                                       ld_chunk(L.bet + off), mean, rstd);
      st_chunk(hp, o.y);
      if (wres) st_chunk(reinterpret_cast<bf16_t*>(a.res_out) + (size_t)(row0 + r) * a.ld_aux + off, o.s);
    }
  }
  __syncthreads();
}

// RMSNormGated (norm_before_gate=False): g = y (z sigmoid(z)), out = g rstd w into the x rows; g recomputed in the
// apply pass (the same bits), zmi_rownorm.h's chunk sums and apply as in zmi_gated_rmsnorm (PRO_GRMSG: g read from the
// aux rows). A wave takes its (row, part) tasks two at a time (the second clamped, its results dropped): two independent
// dependent-add chains in one straight-line body instead of one after the other (the K = 4096 out_proj has 4 waves
// for 2 rows x 4 parts). One workgroup barrier between the passes. The order of the loads (y, gamma, gate) is the
// measured one: equivalent spellings that loaded the gate first moved the hybrid decode step by 0.3 %.
template <int K, int RT, int NWV, int PRO>
__device__ __forceinline__ void prologue_gated_rmsnorm(const ZmiGemvArgs& a, const View<K>& L, int rows,
                                                       int wave, int lane) {
  constexpr int XROW = Img<K>::XROW, GROW = Img<K>::GROW, NQ = ln_parts(K), CPQ = ln_chunks(K);
  float* part = L.red;
  const int ntask = rows * NQ;
  // g of the chunk at `off` of row r: y * gate, or (GRMS_G) as the aux row holds it
  auto load_g = [&](int r, int off, float (&g)[8]) {
    uint32_t y[4] = {0u, 0u, 0u, 0u};
    if constexpr (PRO == PRO_GRMS) {
      const uint4 yv = *reinterpret_cast<const uint4*>(L.xs + r * XROW + off);
      y[0] = yv.x; y[1] = yv.y; y[2] = yv.z; y[3] = yv.w;
    }
    float gz[8];
    load_gate(L.xg + r * GROW + off, gz);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = PRO == PRO_GRMSG ? gz[e] : gate_elem(y, gz, e);
  };
  for (int task0 = wave; task0 < ntask; task0 += 2 * NWV) {
    float t[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int task = min(task0 + u * NWV, ntask - 1);
      const int r = task / NQ, q = task - r * NQ;
      t[u] = 0.f;
#pragma unroll
      for (int i = 0; i < CPQ; ++i) {
        float g[8];
        load_g(r, ln_chunk_off(K, q, lane, i), g);
        t[u] = grms_chunk_sq(g, t[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) t[u] = wave_sum(t[u]);
    if (lane == 0) {
      part[task0] = t[0];
      if (task0 + NWV < ntask) part[task0 + NWV] = t[1];
    }
  }
  __syncthreads();
  for (int task0 = wave; task0 < ntask; task0 += 2 * NWV) {
    uint4 res[2][CPQ];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int task = min(task0 + u * NWV, ntask - 1);
      const int r = task / NQ, q = task - r * NQ;
      const float rstd = 1.0f / sqrtf(ln_combine<NQ>(part + r * NQ) / (float)K + a.eps);
#pragma unroll
      for (int i = 0; i < CPQ; ++i) {
        const int off = ln_chunk_off(K, q, lane, i);
        const uint4 gw = *reinterpret_cast<const uint4*>(L.gam + off);
        float g[8];
        load_g(r, off, g);
        res[u][i] = grms_apply(g, gw, rstd);
      }
    }
    // stores after both tasks' reads: the clamped duplicate task reads what the real one overwrites
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int task = task0 + u * NWV;
      if (task < ntask) {
        const int r = task / NQ, q = task - r * NQ;
        bf16_t* yr = L.xs + r * XROW;
#pragma unroll
        for (int i = 0; i < CPQ; ++i) *reinterpret_cast<uint4*>(yr + ln_chunk_off(K, q, lane, i)) = res[u][i];
      }
    }
  }
  __syncthreads();
}

// One workgroup of the GEMV: block b's column block over its row tiles. The phases above and the row arithmetic of
// zmi_gemv_row.h in order; spelled out here is what decides the LDS-DMA waits: the order of issue, the barriers and the
// s_waitcnt / sched_barrier placement. The DMA pieces are inline asm the compiler does not count: the explicit
// vmcnt(NWL) is their only wait, so no load may move between the staging calls and it except the NWL weight loads.
template <int G, int W, int NL, int RT, int PRO, int EPI, int NTW, int FUSE = 0, int FMT = ZMI_WFMT_BF16>
__device__ __forceinline__ void gemv_body(const ZmiGemvArgs& a, int n_cb, int n_rt, int b, char* smem,
                                          const QkvFuse& fz, int rpw = 1) {
  constexpr int K = W * NL * 64;
  constexpr int KC = K / 64;
  constexpr int NWV = G * W;
  constexpr int XROW = Img<K>::XROW;
  constexpr bool F8 = FMT == ZMI_WFMT_FP8;
  constexpr int CHB = F8 ? 512 : 1024;    // bytes of a 64-k x 8-column weight chunk
  constexpr int NWL = F8 ? NL / 2 : NL;   // 16-byte weight loads per lane
  static_assert(FMT == ZMI_WFMT_BF16 || F8, "weight format");
  static_assert(!F8 || (NL % 2 == 0 && (FUSE == 0 || FUSE == 2)),
                "fp8 weights: every prologue; the plain hand-offs and zmi_mamba_block's granule store");
  static_assert(RT == 8 || RT == 16, "row tile");
  static_assert(!FUSE || EPI == ZMI_EPI_QKV || EPI == ZMI_EPI_STORE || FUSE == 3, "in-launch hand-off: QKV or plain store");
  static_assert(FUSE != 2 || NTW, "the store hand-off runs on single-tile (decode) launches");
  static_assert(FUSE != 3 || (NTW && (EPI == ZMI_EPI_RESIDUAL || EPI == ZMI_EPI_STORE) && PRO == PRO_PLAIN && K == 2048 &&
                              RT == 16),
                "the gathered-input form is zmi_attn_block's out_proj role (one tile, plain, residual or store epilogue)");

  // A workgroup keeps its weight slice in registers and runs its rpw row tiles one after the other, each with the
  // arithmetic of a lone tile (a row's result does not depend on rpw or M).
  const auto [cb, rg] = block_pos(b, n_rt, rpw);
  if (cb >= n_cb) return;  // padding block: exits before any barrier
  ZMI_GSTAMP(0);
  int rt = rg * rpw;
  const int rt_end = min(n_rt, rt + rpw);
  int row0 = rt * RT;
  int rows = min(RT, a.M - row0);
  const View<K> L = Img<K>::carve(smem, a.M < RT ? a.M : RT, PRO);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: SGPR descriptors, no waterfalls
  const int gi = wave / W, wk = wave - gi * W;
  const int ngroups = a.N >> 3;
  const int g_raw = cb * G + gi;
  const bool g_ok = g_raw < ngroups;
  const int g = g_ok ? g_raw : ngroups - 1;  // clamped: every wave joins the barriers
  const int col0 = g * 8;
  const bool ew = (wk == 0) && g_ok;  // the group's first wave runs the epilogue
  constexpr int NE = (8 * RT + 63) / 64;
  uint32_t res_pre[NE];
  int q_pos = -1, q_kvr = 0;
  unsigned act_rows = ~0u;  // FUSE 3: rows whose position is >= 0 (the others ran no attention: no residual store)

  // (1) the first tile's rows (FUSE 3: gathered below) and epilogue operands (split: the tile loop issues the next
  // tile's rows as soon as every chain has left the LDS image, under the current tile's reduction and epilogue)
  if (FUSE != 3) stage_rows<K, PRO, NWV>(a, L, wave, lane, true, row0, rows);
  stage_epilogue_operands<EPI, RT>(a, ew, lane, rows, row0, col0, res_pre, q_pos, q_kvr);
  // fp8: the group's 8 column exponents, one 8-byte load per epilogue lane, older than the weights
  uint2 wexp = {0u, 0u};
  if constexpr (F8) {
    if (ew) wexp = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(a.w_exp) + col0);
  }
  __builtin_amdgcn_sched_barrier(0);
  // (2) the lane's whole weight slice, in flight at once; non-temporal when each weight is read once (one row tile)
  u32x4_t wf[NWL];
  load_weights_m8<NWL, NTW ? 2 : 0>(reinterpret_cast<const char*>(a.W) + ((size_t)g * KC + wk * NL) * CHB, NL * CHB,
                                    lane, wf);
  __builtin_amdgcn_sched_barrier(0);
  ZMI_GSTAMP(1);
  // DMA pieces + epilogue operands landed: everything but this lane's NWL weight loads
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWL) : "memory");
  if constexpr (F8) {  // landed, and the same for every lane of the wave: kept in SGPRs through the prologue
    wexp.x = __builtin_amdgcn_readfirstlane(wexp.x);
    wexp.y = __builtin_amdgcn_readfirstlane(wexp.y);
  }
  // single-tile QKV launches (every decode step): the epilogue's RoPE cos / sin pair, issued now that the row's
  // position has landed, so it arrives under the LayerNorm and the MFMA chain instead of after them
  float2 rope_cs = {1.f, 0.f};
  if (EPI == ZMI_EPI_QKV && NTW && ew && (lane >> 2) < rows && q_pos >= 0 && q_pos < a.smax) {
    const int n = col0 + (lane & 3) * 2;
    if (n < a.hq * a.hd + a.hkv * a.hd) rope_cs = *rope_pair(a, q_pos, n);
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (FUSE == 3)  // (1') with its own two barriers; the segment-sum area holds the rows' positions meanwhile
    act_rows = gather_attention_rows<K, NWV>(a, fz, L.xs, reinterpret_cast<int*>(L.red), rows, row0, tid);
  for (;;) {  // the workgroup's row tiles
    __builtin_amdgcn_s_barrier();  // the tile's rows (and gamma / beta) are visible to every wave
    __builtin_amdgcn_sched_barrier(0);
    ZMI_GSTAMP(2);
    // (3) the prologue normalises the rows in place; each ends with a workgroup barrier
    if constexpr (PRO == PRO_LN) prologue_layernorm<K, RT, NWV>(a, L, rows, wave, lane);
    if constexpr (PRO == PRO_ADDLN)
      prologue_add_layernorm<K, RT, NWV>(a, L, rows, row0, a.res_out != nullptr && cb == 0, wave, lane);
    if constexpr (PRO == PRO_GRMS || PRO == PRO_GRMSG) prologue_gated_rmsnorm<K, RT, NWV, PRO>(a, L, rows, wave, lane);
    ZMI_GSTAMP(3);

    // (4) MFMA chain over this wave's k-segment (rows past the tile re-read its last row). The weights' first use.
    f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    chain_m8<NL, F8>(L.xs + min(lane & 15, rows - 1) * XROW + wk * NL * 64 + (lane >> 4) * 8, wf, acc0, acc1);
    ZMI_GSTAMP(4);
    const SegPos sp = segment_pos<false>(lane);  // (5) the wave's segment sums into red[wave][column][row]
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float v = segment_value<false>(acc0, acc1, q);
      if (sp.live && sp.rb + q < RT) L.red[(wave * 8 + sp.c) * RT + sp.rb + q] = v;
    }
    __syncthreads();
    ZMI_GSTAMP(5);
    if (!NTW && rt + 1 < rt_end) {  // every chain is done with the LDS image: the next tile's rows go in now
      const int n_row0 = (rt + 1) * RT;
      stage_rows<K, PRO, NWV>(a, L, wave, lane, false, n_row0, min(RT, a.M - n_row0));
    }
    if (ew)  // (6) the group's W segment sums in wave order, then the fused epilogue
      epilogue<EPI, RT, FUSE>(a, ColSum<W, RT, F8>{L.red + gi * W * 8 * RT, wexp}, lane, rows, row0, g, res_pre, q_pos,
                              q_kvr, fz, act_rows, (EPI == ZMI_EPI_QKV && NTW) ? &rope_cs : nullptr);
    ZMI_GSTAMP(6);
    // one tile when each weight is read once (NTW: M <= RT, every decode launch): no loop state there
    if (NTW || ++rt >= rt_end) break;
    __syncthreads();  // every wave is done with this tile's LDS image and segment sums
    row0 = rt * RT;
    rows = min(RT, a.M - row0);
    stage_epilogue_operands<EPI, RT>(a, ew, lane, rows, row0, col0, res_pre, q_pos, q_kvr);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this tile's rows (the weights landed long ago)
  }  // row tiles
}

template <int G, int W, int NL, int RT, int PRO, int EPI, int NTW>
__global__ __launch_bounds__(G * W * 64) void gemv_kernel(const ZmiGemvArgs a, int n_cb, int n_rt, int rpw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_body<G, W, NL, RT, PRO, EPI, NTW>(a, n_cb, n_rt, blockIdx.x, smem, QkvFuse{nullptr, 0}, rpw);
}
// the same launch over fp8 weights (a kernel of its own name: the bf16 kernels keep theirs in traces and profiles)
template <int G, int W, int NL, int RT, int PRO, int EPI, int NTW>
__global__ __launch_bounds__(G * W * 64) void gemv_kernel_f8(const ZmiGemvArgs a, int n_cb, int n_rt, int rpw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_body<G, W, NL, RT, PRO, EPI, NTW, 0, ZMI_WFMT_FP8>(a, n_cb, n_rt, blockIdx.x, smem, QkvFuse{nullptr, 0}, rpw);
}

template <int FMT, int... A>
constexpr auto gemv_fn() {  // the kernel of a weight format (only the one asked for is instantiated)
  if constexpr (FMT == ZMI_WFMT_FP8)
    return &gemv_kernel_f8<A...>;
  else
    return &gemv_kernel<A...>;
}

// s_waitcnt vmcnt(n) as the builtin (gfx9 encoding, expcnt / lgkmcnt left at their maxima): unlike an asm
// wait, the compiler's own wait insertion sees it, so loads it covers are not waited for again after
// later (uncounted) LDS-DMA issues
#define ZMI_WAIT_VM(n) __builtin_amdgcn_s_waitcnt(((n) & 15) | (((n) >> 4) << 14) | 0x0F70)

// Many-row form of the K = 2048 GEMV (multi-slot decode and prefill, M > 16), the same per-row arithmetic as
// gemv_body's (W, NL, RT) = (4, 8, 16) shape: a wave's chain of MFMAs over one k-segment (k-half 0 / 1 in
// two accumulators, their segment_value), then the 4 segment sums in segment order, then epilogue(): the row arithmetic
// of zmi_gemv_row.h.
// What changes is the reuse and the pipelining:
//  * a workgroup owns 8 groups (64 columns) and each wave GPW of them over one segment (GPW x 32 weight
//    VGPRs), so every activation tile it stages serves 64 columns (gemv_body's 4-group form: 32, twice the
//    activation traffic per column) and each A fragment read from LDS feeds GPW groups;
//  * the activation tiles (and the epilogue operands) come by LDS-DMA two tiles ahead into two buffers;
//  * one barrier per tile: group gi's epilogue runs on wave gi after it, while the other waves start the
//    next tile's chains; an LDS arrival counter keeps those from overwriting the segment sums before every
//    epilogue of the tile has read them.
// One workgroup per CU.
constexpr int GR_G = 8, GR_RT = 16, GR_XROW = 2048 + 8;
constexpr size_t GR_RED = (size_t)2 * GR_RT * GR_XROW * 2;             // after the two activation tiles
constexpr size_t GR_OPS = GR_RED + (size_t)GR_G * 4 * 8 * GR_RT * 4;   // epilogue operands, 2 x 2 KiB
constexpr size_t GR_CNT = GR_OPS + 2 * 2048;
constexpr size_t GR_LDS = GR_CNT + 16;

// one 256-byte LDS-DMA piece (64 lanes x 4 B, lane-linear)
__device__ __forceinline__ void dma_dword(const void* gsrc, void* ldp) {
  const unsigned ldst =
      __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) void*)ldp);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(ldst)
               : "memory");
}

//  * DN (dense pairs, zmi_gemv_row.h): each wave owns one PAIR of groups; half the MFMAs of the M8 form, same bits.
//  * FMT fp8 (layout M8F8): half the weight loads (512-byte chunks, two per 16-byte load); once they have landed the
//    bytes are expanded into the bf16 registers of the bf16 form (expand_fp8: once per workgroup, not per tile as
//    gemv_body's chain does), the tile loop is the bf16 one, and the epilogue wave scales its group's finished sums by
//    the columns' 2^e (ColSum), as gemv_body does. No wait is added: the exponents land under the ZMI_WAIT_VM(0) below.
template <int EPI, int GPW, bool DN, int FMT>
__device__ __forceinline__ void gemm_rows_body(const ZmiGemvArgs& a, int n_cb, int n_rt, int rpw, char* smem) {
  constexpr int W = 4, NL = 8, RT = GR_RT, K = 2048, KC = K / 64, XROW = GR_XROW, NE = 2;
  constexpr bool F8 = FMT == ZMI_WFMT_FP8;
  static_assert(FMT == ZMI_WFMT_BF16 || F8, "weight format");
  static_assert(!F8 || EPI == ZMI_EPI_SWIGLU || EPI == ZMI_EPI_RESIDUAL || EPI == ZMI_EPI_F32,
                "fp8 weights: the MLP epilogues (pro_built)");
  // group sets (DN: pair sets, GPW pairs per wave), waves
  constexpr int NGS = DN ? GR_G / 2 / GPW : GR_G / GPW, NWV = NGS * W;
  static_assert(!DN || GPW == 1, "dense pairs: one pair per wave");
  // the activation tiles are DMA'd by the upper half of the waves only (PPW pieces each): the epilogue waves
  // (wave < 8) then never wait on memory inside the tile loop, so their output stores stay in flight
  constexpr int NDW = NWV / 2, PPW = RT * (K / 512) / NDW;
  static_assert(NDW >= GR_G, "the epilogue waves and the DMA waves are disjoint");
  // operand pieces per tile, issued by the last wave: residual inputs (16 rows x 8 groups x 16 B), or the rows'
  // positions and cache rows (dwords)
  constexpr int EP = EPI == ZMI_EPI_RESIDUAL ? 2 : (EPI == ZMI_EPI_QKV ? 1 : 0);
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);                 // [2][RT][XROW] activation tiles
  float* red = reinterpret_cast<float*>(smem + GR_RED);          // [group][segment][8][RT] segment sums
  char* ops = smem + GR_OPS;                                     // [2][2 KiB]
  unsigned* cnt = reinterpret_cast<unsigned*>(smem + GR_CNT);    // epilogues finished
  const BlockPos bp = block_pos(blockIdx.x, n_rt, rpw);
  const int cb = bp.cb, rg = bp.rg;
  if (cb >= n_cb) return;
  ZMI_GSTAMP(0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gs = wave % NGS, wk = wave / NGS;  // groups gs + NGS h (h < GPW) over segment wk
  const int ngroups = a.N >> 3;
  int gg[GPW];
#pragma unroll
  for (int h = 0; h < GPW; ++h) gg[h] = min(cb * GR_G + gs + NGS * h, ngroups - 1);  // clamped: discarded
  const int n_ew = min(GR_G, ngroups - cb * GR_G);  // epilogue waves: group cb * 8 + wave on wave < n_ew
  const bool ew = wave < n_ew;
  const int eg = cb * GR_G + wave;
  const int t0 = rg * rpw;
  const int rt_end = min(n_rt, t0 + rpw);
  const bf16_t* X = reinterpret_cast<const bf16_t*>(a.X);
  const bool opw = EP && wave == NWV - 1;  // the operand-piece wave
  const bool dw = wave >= NDW;              // a DMA wave
  if (tid == 0) *cnt = 0;
  volatile __attribute__((address_space(3))) unsigned* lcnt = (volatile __attribute__((address_space(3))) unsigned*)cnt;

  // tile t = 16 rows x 4 KiB = 64 DMA pieces, PPW per wave (rows past M re-read row M - 1: their outputs are
  // discarded, and the waves' counts are fixed, which the vmcnt waits rely on), then its epilogue operands
  auto dma_tile = [&](int t) {
    if (!dw) return;
    bf16_t* dst = xs + (t & 1) * RT * XROW;
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int pc = wave - NDW + NDW * i, r = pc >> 2, p = pc & 3;
      const int sr = min(t * RT + r, a.M - 1);
      dma_piece(X + (size_t)sr * a.ldx + p * 512 + lane * 8, dst + r * XROW + p * 512);
    }
    if (opw) {
      char* od = ops + (t & 1) * 2048;
      if (EPI == ZMI_EPI_RESIDUAL) {  // [row][group] 16 B: out[row][8 g .. 8 g + 7]
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int e = lane + 64 * i, r = e >> 3, gi = min(cb * GR_G + (e & 7), ngroups - 1);
          dma_piece(reinterpret_cast<const bf16_t*>(a.out) + (size_t)min(t * RT + r, a.M - 1) * a.ldo + gi * 8,
                    reinterpret_cast<bf16_t*>(od + i * 1024));
        }
      } else if (EPI == ZMI_EPI_QKV) {  // dwords 0..15 the rows' positions, 16..31 their cache rows
        const int r = min(t * RT + (lane & 15), a.M - 1);
        dma_dword((lane & 16) ? a.row_kv + r : a.row_pos + r, od);
      }
    }
  };

  dma_tile(t0);
  if (t0 + 1 < rt_end) dma_tile(t0 + 1);
  __builtin_amdgcn_sched_barrier(0);
  // the weight slices of the wave's groups (GPW NL x 16 B per lane), in flight at once (all waited for below, before
  // the first chain). Re-read by the other row groups of this column block from L2 (temporal).
  u32x4_t wf[DN ? 2 : GPW][NL];  // DN: wf[h][j] = k-half h of chunk j for the wave's pair
  u32x4_t raw[F8 ? (DN ? 2 : GPW) : 1][NL / 2];  // fp8: the landed pieces, dead once expanded into wf
  uint2 wexp = {0u, 0u};                         // fp8: the 8 column exponents of this wave's epilogue group
  if constexpr (F8) {
    // (every wave loads: the address is wave-uniform and clamped like gg[]; only the epilogue waves use it)
    wexp = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(a.w_exp) + 8 * min(eg, ngroups - 1));
    if constexpr (DN) {
      const int grp = min(cb * GR_G + 2 * gs + dn_member(lane), ngroups - 1) - cb * GR_G;
      load_weights_dn_f8<NL, 0>(reinterpret_cast<const char*>(a.W) + (size_t)cb * GR_G * KC * 512, GR_G * KC * 512,
                                (grp * KC + wk * NL) * 512, lane, raw);
    } else {
#pragma unroll
      for (int h = 0; h < GPW; ++h)
        load_weights_m8<NL / 2, 0>(reinterpret_cast<const char*>(a.W) + ((size_t)gg[h] * KC + wk * NL) * 512, NL * 512,
                                   lane, raw[h]);
    }
  } else if constexpr (DN) {
    // lane l: column l & 15 of pair gs (group cb * 8 + 2 gs + dn_member(l), clamped: discarded); the descriptor
    // spans the column block's 8 groups
    const int grp = min(cb * GR_G + 2 * gs + dn_member(lane), ngroups - 1) - cb * GR_G;
    load_weights_dn<NL, 0>(reinterpret_cast<const char*>(a.W) + (size_t)cb * GR_G * KC * 1024, GR_G * KC * 1024,
                           (grp * KC + wk * NL) * 1024, lane, wf);
  } else {
#pragma unroll
    for (int h = 0; h < GPW; ++h)
      load_weights_m8<NL, 0>(reinterpret_cast<const char*>(a.W) + ((size_t)gg[h] * KC + wk * NL) * 1024, NL * 1024, lane,
                             wf[h]);
  }
  __builtin_amdgcn_sched_barrier(0);
  // every weight slice and the first two tiles' pieces: waiting here for all of them keeps the compiler's own
  // waits for the weights out of the tile loop (a vmcnt(0) there would also wait for the DMA of later tiles
  // and for the epilogue stores)
  ZMI_WAIT_VM(0);
  if constexpr (F8) {  // the landed bytes become the bf16 form's registers, once for all of the workgroup's tiles
#pragma unroll
    for (int h = 0; h < (DN ? 2 : GPW); ++h) expand_fp8<NL>(raw[h], wf[h]);
    wexp.x = __builtin_amdgcn_readfirstlane(wexp.x);
    wexp.y = __builtin_amdgcn_readfirstlane(wexp.y);
  }
  __syncthreads();

  for (int t = t0;; ++t) {  // invariant: tile t's rows and operands are in LDS, visible to every wave
    const int ti = t - t0;
    if (ti == 1) ZMI_GSTAMP(2);
    const int row0 = t * RT, rows = min(RT, a.M - row0);
    const bool more = t + 1 < rt_end;
    f32x4_t acc0[GPW], acc1[GPW];
#pragma unroll
    for (int h = 0; h < GPW; ++h) acc0[h] = acc1[h] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    {  // the chains of the wave's groups over the same A fragments (every row of the tile is staged: no clamp)
      const bf16_t* xa = xs + (t & 1) * RT * XROW + (lane & 15) * XROW + wk * NL * 64 + (lane >> 4) * 8;
      if constexpr (DN) {
        chain_dn<NL>(xa, wf, acc0[0], acc1[0]);
      } else {
#pragma unroll
        for (int h = 0; h < GPW; ++h) chain_m8<NL, false>(xa, wf[h], acc0[h], acc1[h]);
      }
    }
    if (ti == 0) ZMI_GSTAMP(1);
    if (ti == 1) ZMI_GSTAMP(3);
    // the previous tile's epilogues have read the segment sums (bounded: they are a few hundred cycles of work)
    if (ti > 0) {
      const unsigned want = (unsigned)(n_ew * ti);
      for (int spin = 0; *lcnt < want && spin < (1 << 20); ++spin)
        __builtin_amdgcn_s_sleep(1);
    }
    {  // the segment sums into red[group][segment][column][row] (DN: the lane's own group of the pair)
      const SegPos sp = segment_pos<DN>(lane);
#pragma unroll
      for (int h = 0; h < (DN ? 1 : GPW); ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float v = segment_value<DN>(acc0[h], acc1[h], q);
          const int grp = DN ? 2 * gs + (sp.c >> 3) : gs + NGS * h;
          if (sp.live) red[((grp * W + wk) * 8 + (sp.c & 7)) * RT + sp.rb + q] = v;
        }
    }
    // this tile's epilogue operands into registers before the buffer is re-filled
    uint32_t res_pre[NE] = {0u, 0u};
    int q_pos = -1, q_kvr = 0;
    if (ew) {
      const char* od = ops + (t & 1) * 2048;
      if (EPI == ZMI_EPI_RESIDUAL) {
#pragma unroll
        for (int i = 0; i < NE; ++i) {
          const int e = lane + 64 * i, r = e >> 3, c = e & 7;
          res_pre[i] = *reinterpret_cast<const uint16_t*>(od + (r * GR_G + wave) * 16 + c * 2);
        }
      }
      if (EPI == ZMI_EPI_QKV && (lane >> 2) < rows) {
        q_pos = reinterpret_cast<const int*>(od)[lane >> 2];
        q_kvr = reinterpret_cast<const int*>(od)[16 + (lane >> 2)];
      }
    }
    if (dw) ZMI_WAIT_VM(0);  // the next tile's pieces (DMA waves; the epilogue waves' stores stay in flight)
    // segment sums complete; the next tile's rows visible; this tile's buffers free (LDS-only fence: no wait
    // for global stores)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    if (ti == 1) ZMI_GSTAMP(4);
    if (t + 2 < rt_end) dma_tile(t + 2);
    if (ew) {  // group cb * 8 + wave: its segment sums in segment order (gemv_body's wave order)
      epilogue<EPI, RT, 0>(a, ColSum<W, RT, F8>{red + wave * W * 8 * RT, wexp}, lane, rows, row0, eg, res_pre, q_pos,
                           q_kvr, QkvFuse{nullptr, 0});
      if (more && lane == 0) __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (ti == 1) ZMI_GSTAMP(5);
    if (!more) break;
  }
  ZMI_GSTAMP(7);
}

template <int EPI, int GPW, bool DN = false>
__global__ __launch_bounds__(GR_G * 4 / GPW * 64 / (DN ? 2 : 1)) void gemm_rows_kernel(const ZmiGemvArgs a, int n_cb,
                                                                                       int n_rt, int rpw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemm_rows_body<EPI, GPW, DN, ZMI_WFMT_BF16>(a, n_cb, n_rt, rpw, smem);
}
// the same launch over fp8 weights (a kernel of its own name, as gemv_kernel_f8)
template <int EPI, int GPW, bool DN = false>
__global__ __launch_bounds__(GR_G * 4 / GPW * 64 / (DN ? 2 : 1)) void gemm_rows_kernel_f8(const ZmiGemvArgs a, int n_cb,
                                                                                          int n_rt, int rpw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemm_rows_body<EPI, GPW, DN, ZMI_WFMT_FP8>(a, n_cb, n_rt, rpw, smem);
}

// row tiles per workgroup: enough workgroups to fill the chip (~4 per CU), each re-reading its weight
// slice as few times as that allows (speed only: a row's arithmetic does not depend on it)
inline int rows_per_wg(int n_cb, int n_rt, int target) {
  if (n_rt <= 1) return 1;
  // about `target` workgroups: fewer row groups re-read each weight slice. Measured on the C3 sample:
  // 512 (K = 2048) against ~1024: 102 -> 104x, 256 and 2048 slower, the prefill unmoved; 256 for the
  // K = 8192 fc2 (1024-thread workgroups, 256 KB weight slices): 9,740 -> 9,960 frames/s, 128 slower
  const int n_rg = std::max(1, std::min(n_rt, target / std::max(1, n_cb)));
  return (n_rt + n_rg - 1) / n_rg;
}

// (W, NL, RT) from K: K = 64 W NL. The shape fixes a row's reduction order, so it depends on K
// only (every M, every launch form: decode, prefill and zmi_attn_block's QKV role agree bit for
// bit). K = 2048 streams 8 chunks per lane from 4 waves per group (with G = 2: 512 threads, the
// fused QKV + attention launch's block size); K = 8192 holds 8 rows per tile (8 x 16 KiB of LDS).
struct Shape {
  int W, NL, RT;
};
inline bool shape_for(int K, Shape* s) {
  switch (K) {
    case 512: *s = {2, 4, 16}; return true;
    case 1024: *s = {4, 4, 16}; return true;
    case 2048: *s = {4, 8, 16}; return true;
    case 4096: *s = {4, 16, 16}; return true;
    case 8192: *s = {8, 16, 8}; return true;
  }
  return false;
}

// column groups per block: 2 for the many-group K = 2048 projections with a prologue or many rows (qkv, fc1, heads: the
// block's LayerNorm and activation staging are then shared by 16 columns), 4 for the plain ones over many rows;
// `groups` > 0 overrides.
// Speed only: a group's arithmetic does not depend on G.
inline int groups_for(const ZmiGemvArgs& a, const Shape& s) {
  if (a.groups > 0) return a.groups;
  // two groups also for plain rows when there are many of them: each workgroup's activation tiles
  // then serve 16 columns (a 128-row fc1 re-read its rows from L2 per 8-column group: ~1 GB a launch)
  // (from 5 rows: the pre-normalised plans; C5's 16-row step 2.03 -> 1.87 ms with both K = 2048 and 8192 at 2)
  if (a.K == 8192 && a.M > 4 && a.N / 8 >= 256) return 2;  // fc2 over many rows: 16 KB activation rows
  // 4 groups (1024 threads) for the plain K = 2048 GEMVs over many rows (qkv, out_proj, fc1, heads of the
  // multi-slot decode and the prefill): each staged activation tile serves 32 columns, halving the tile
  // re-reads of 2 groups (C3 sample 9,050 -> 9,710 frames/s)
  if (a.K == 2048 && a.M > 16 && a.N / 8 >= 256 && a.ln_w == nullptr && a.pro == ZMI_PRO_AUTO) return 4;
  return (a.K == 2048 && a.N / 8 >= 384 && (a.ln_w != nullptr || a.pro != ZMI_PRO_AUTO || a.M > 4)) ? 2 : 1;
}

// where the many-row form beats gemv_body's 4-group tile loop (C3 decode shapes, tools/kernel_bench.py
// --gemm-rows 1,0): 128 rows qkv 18.1 -> 13.0 us, fc1 41.9 -> 31.1, heads 36.9 -> 24.0, out_proj 9.8 -> 7.0;
// 64 rows qkv 12.1 -> 9.6, fc1 26.2 -> 22.8, heads 21.3 -> 15.3 but out_proj 5.8 -> 6.8; 32 rows only the
// wide ones (heads 13.3 -> 11.6; qkv 7.6 -> 9.7, out_proj 5.8 -> 8.3)
inline bool rows_form(int M, int N) { return M > 64 || (M > 32 && N >= 3072) || N >= 8192; }
// the launches that take the many-row form: plain K = 2048 rows past one tile, no forced group count; over fp8 weights
// the MLP epilogues pro_built(2048, epi, PRO_PLAIN, true) names other than STORE (the plain fp8 STORE at K = 2048 is
// not built in any form), while ZMI_OPT_FP8_ROWS is set (0: gemv_body's tile loop, the same bits). rows_form's
// thresholds hold for fp8 as they are: fc1 (N 16384, SWIGLU, weights streamed from HBM) per launch, fp8 tile loop ->
// fp8 many-row form, median of 5 (max - min of both arms): 24 rows 13.4 -> 11.5 us (0.3), 32 14.2 -> 11.7 (0.2), 48
// 17.5 -> 13.2 (0.6), 64 21.8 -> 14.9 (0.8), 128 36.7 -> 21.2 (1.1), 322 84.4 -> 41.8 (1.4); the bf16 many-row form
// 18.6 / 18.8 / 20.4 / 21.9 / 28.1 / 48.3 (tools/bench_fp8_rows.py, profiles/fp8_rows_bench.json)
inline bool rows_launch(const ZmiGemvArgs& a, int epi) {
  if (a.w_fmt == ZMI_WFMT_FP8) {
    if (!zmi_option(ZMI_OPT_FP8_ROWS) || (epi != ZMI_EPI_SWIGLU && epi != ZMI_EPI_RESIDUAL && epi != ZMI_EPI_F32))
      return false;
  } else if (a.w_fmt != ZMI_WFMT_BF16) {
    return false;
  }
  return a.K == 2048 && a.M > GR_RT && a.ln_w == nullptr && a.pro == ZMI_PRO_AUTO && a.groups == 0 &&
         zmi_option(ZMI_OPT_GEMM_ROWS) && rows_form(a.M, a.N);
}

// gemv_body's (G, W, NL, RT) instantiations that are built with every prologue / tile form of launch_g; the 4-group
// (4, 4, 8, 16) one is built as the plain tile loop only (groups_for's many-row plain case)
#define ZMI_GEMV_SHAPES(X) X(1, 2, 4, 16) X(1, 4, 4, 16) X(1, 4, 8, 16) X(2, 4, 8, 16) X(1, 4, 16, 16) X(1, 8, 16, 8) X(2, 8, 16, 8)

// the prologue of a shape, where it is built: ADDLN (the hybrid blocks' d_model GEMVs) for K 512 / 2048; GRMS (the
// Mamba2 out_proj, K = d_ssm) for K 1024 / 4096 with the store epilogue, GRMS_G (the same from g = y * gate rows) on one
// tile (decode). fp8 weights: the MLP projections (SWIGLU / RESIDUAL / F32, LayerNorm'd or plain rows, not K = 4096)
// and the Mamba2 mixers' projections with the store epilogue: in_proj under ADDLN only, out_proj under GRMS / GRMS_G
// or plain at K = d_ssm (1024 / 4096; no other projection has that K). QKV and LOGITS read bf16 only.
constexpr bool pro_built(int K, int epi, int pro, bool f8) {
  if (f8 && epi != ZMI_EPI_STORE && epi != ZMI_EPI_SWIGLU && epi != ZMI_EPI_RESIDUAL && epi != ZMI_EPI_F32) return false;
  if (pro == PRO_ADDLN)
    return (K == 512 || K == 2048) && epi != ZMI_EPI_RESIDUAL && epi != ZMI_EPI_F32 && (!f8 || epi == ZMI_EPI_STORE);
  if (pro == PRO_GRMS || pro == PRO_GRMSG) return (K == 1024 || K == 4096) && epi == ZMI_EPI_STORE;
  if (f8 && epi == ZMI_EPI_STORE) return pro == PRO_PLAIN && (K == 1024 || K == 4096);
  return !f8 || K != 4096;
}

inline size_t img_bytes(int K, int rows, int nwv, int rt, int pro) {
  switch (K) {
    case 512: return Img<512>::bytes(rows, nwv, rt, pro);
    case 1024: return Img<1024>::bytes(rows, nwv, rt, pro);
    case 2048: return Img<2048>::bytes(rows, nwv, rt, pro);
    case 4096: return Img<4096>::bytes(rows, nwv, rt, pro);
    default: return Img<8192>::bytes(rows, nwv, rt, pro);
  }
}

// The form a launch takes: the kernel (gemv_body / the many-row form, M8 or dense pairs), its (G, W, NL, RT)
// instantiation, single-tile or tile loop, the resolved prologue and the grid's geometry. Every launch<EPI>() dispatches
// on what this returns and zmi_gemv_form reports it; false = not built (zmi_gemv_launch refuses).
inline bool form_for(const ZmiGemvArgs& a, int epi, ZmiGemvForm* f) {
  Shape sh;
  if (!shape_for(a.K, &sh)) return false;
  const bool f8 = a.w_fmt == ZMI_WFMT_FP8;
  // fp8 weights take the many-row form where bf16 ones do (the MLP epilogues; ZMI_OPT_FP8_ROWS 0: gemv_body's tile
  // loop for every M). All forms agree bit for bit, so the choice is speed, never bits. (Which fp8 launches exist:
  // pro_built; fc2's split-K over fp8 bytes is zmi_gemv_splitk_f8.)
  if (rows_launch(a, epi)) {
    const int n_cb = (a.N / 8 + GR_G - 1) / GR_G, n_rt = (a.M + GR_RT - 1) / GR_RT;
    *f = {(zmi_option(ZMI_OPT_GEMM_ROWS) & 2) ? ZMI_FORM_ROWS_DENSE : ZMI_FORM_ROWS, GR_G, 4, 8, GR_RT, 0, PRO_PLAIN,
          n_cb, n_rt, rows_per_wg(n_cb, n_rt, zmi_cu_count())};  // one workgroup per CU
    return true;
  }
  const int g = groups_for(a, sh);
  const int pro = a.pro != ZMI_PRO_AUTO ? a.pro : (a.ln_w != nullptr ? PRO_LN : PRO_PLAIN);  // ZMI_PRO_* = PRO_*
  const int ntw = a.M <= sh.RT;  // one row tile: each weight is read once, the non-temporal single-tile instantiation
  bool built = g == 4 && sh.W == 4 && sh.NL == 8 && sh.RT == 16 && !ntw && pro == PRO_PLAIN;
#define ZMI_SHAPE(G_, W_, NL_, RT_) built = built || (g == G_ && sh.W == W_ && sh.NL == NL_ && sh.RT == RT_);
  ZMI_GEMV_SHAPES(ZMI_SHAPE)
#undef ZMI_SHAPE
  if (!built) return false;  // e.g. groups = 2 outside the K = 2048 / 8192 shapes
  if (!pro_built(a.K, epi, pro, f8) || (pro == PRO_GRMSG && !ntw)) return false;
  if (img_bytes(a.K, a.M < sh.RT ? a.M : sh.RT, g * sh.W, sh.RT, pro) > LDS_MAX) return false;
  const int n_cb = (a.N / 8 + g - 1) / g, n_rt = (a.M + sh.RT - 1) / sh.RT;
  *f = {ZMI_FORM_BODY, g, sh.W, sh.NL, sh.RT, ntw, pro, n_cb, n_rt, rows_per_wg(n_cb, n_rt, a.K == 8192 ? 256 : 512)};
  return true;
}

template <int G, int W, int NL, int RT, int PRO, int EPI, int NTW, int FMT = ZMI_WFMT_BF16>
hipError_t launch_p(const ZmiGemvArgs& a, hipStream_t s, const ZmiGemvForm& f) {
  constexpr int K = W * NL * 64;
  auto fn = gemv_fn<FMT, G, W, NL, RT, PRO, EPI, NTW>();
  size_t lds = Img<K>::bytes(a.M < RT ? a.M : RT, G * W, RT, PRO);
  const int64_t blocks = block_count(f.n_cb, f.n_rt, f.rpw);
  if (NTW && zmi_option(ZMI_OPT_GEMV_SPREAD)) {
    // a decode launch streams each weight once: its rate is the number of CUs it keeps busy (one CU
    // pulls ~25 GB/s), so reserve LDS such that at most ceil(blocks / CUs) workgroups share a CU
    // (ZMI_OPT_GEMV_SPREAD > 1 caps the workgroups per CU at that value: an occupancy probe; 2 cost fc1 ~0.85 us per
    // launch, 3 measured the same as 4, profiles/r06_gemv_spread_ab.jsonl)
    int64_t per_cu = (blocks + zmi_cu_count() - 1) / zmi_cu_count();
    if (zmi_option(ZMI_OPT_GEMV_SPREAD) > 1) per_cu = std::min<int64_t>(per_cu, zmi_option(ZMI_OPT_GEMV_SPREAD));
    if (per_cu < 8) lds = std::max(lds, LDS_MAX / (size_t)(per_cu + 1) + 1024);
  }
  if (lds > 64 * 1024) {
    static const hipError_t attr =  // once per instantiation: allow > 64 KiB of dynamic LDS
        hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)LDS_MAX);
    if (attr != hipSuccess) return attr;
  }
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(G * W * 64), lds, s, a, f.n_cb, f.n_rt, f.rpw);
  return hipGetLastError();
}

// one row tile (M <= RT: the single-tile instantiation) or the row-tile loop
template <int G, int W, int NL, int RT, int PRO, int EPI, int FMT = ZMI_WFMT_BF16>
hipError_t launch_tiles(const ZmiGemvArgs& a, hipStream_t s, const ZmiGemvForm& f) {
  return f.ntw ? launch_p<G, W, NL, RT, PRO, EPI, 1, FMT>(a, s, f) : launch_p<G, W, NL, RT, PRO, EPI, 0, FMT>(a, s, f);
}

// the prologues of a shape: only those pro_built names are instantiated
template <int G, int W, int NL, int RT, int EPI, int FMT>
hipError_t launch_g(const ZmiGemvArgs& a, hipStream_t s, const ZmiGemvForm& f) {
  constexpr int K = W * NL * 64;
  constexpr bool F8 = FMT == ZMI_WFMT_FP8;
  if constexpr (pro_built(K, EPI, PRO_ADDLN, F8))
    if (f.pro == PRO_ADDLN) return launch_tiles<G, W, NL, RT, PRO_ADDLN, EPI, FMT>(a, s, f);
  if constexpr (pro_built(K, EPI, PRO_GRMS, F8)) {
    if (f.pro == PRO_GRMS) return launch_tiles<G, W, NL, RT, PRO_GRMS, EPI, FMT>(a, s, f);
    if (f.pro == PRO_GRMSG && f.ntw) return launch_p<G, W, NL, RT, PRO_GRMSG, EPI, 1, FMT>(a, s, f);
  }
  if constexpr (pro_built(K, EPI, PRO_LN, F8))
    if (f.pro == PRO_LN) return launch_tiles<G, W, NL, RT, PRO_LN, EPI, FMT>(a, s, f);
  if constexpr (pro_built(K, EPI, PRO_PLAIN, F8))
    if (f.pro == PRO_PLAIN) return launch_tiles<G, W, NL, RT, PRO_PLAIN, EPI, FMT>(a, s, f);
  return hipErrorInvalidValue;
}

template <int FMT, int EPI, int GPW, bool DN>
constexpr auto gemm_rows_fn() {  // the many-row kernel of a weight format (only the one asked for is instantiated)
  if constexpr (FMT == ZMI_WFMT_FP8)
    return &gemm_rows_kernel_f8<EPI, GPW, DN>;
  else
    return &gemm_rows_kernel<EPI, GPW, DN>;
}

template <int EPI, int GPW, bool DN, int FMT = ZMI_WFMT_BF16>
hipError_t launch_rows(const ZmiGemvArgs& a, hipStream_t s, const ZmiGemvForm& f) {
  auto fn = gemm_rows_fn<FMT, EPI, GPW, DN>();
  const int64_t blocks = block_count(f.n_cb, f.n_rt, f.rpw);
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
  if (attr != hipSuccess) return attr;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(GR_G * 4 / GPW * 64 / (DN ? 2 : 1)), GR_LDS, s, a, f.n_cb, f.n_rt,
                     f.rpw);
  return hipGetLastError();
}

// gemv_body's launches of one weight format
template <int EPI, int FMT>
hipError_t launch_shape(const ZmiGemvArgs& a, hipStream_t s, const ZmiGemvForm& f) {
  if (f.G == 4) {
    if constexpr (pro_built(2048, EPI, PRO_PLAIN, FMT == ZMI_WFMT_FP8))
      return launch_p<4, 4, 8, 16, PRO_PLAIN, EPI, 0, FMT>(a, s, f);
    return hipErrorInvalidValue;
  }
#define ZMI_SHAPE(G_, W_, NL_, RT_) \
  if (f.G == G_ && f.W == W_ && f.NL == NL_ && f.RT == RT_) return launch_g<G_, W_, NL_, RT_, EPI, FMT>(a, s, f);
  ZMI_GEMV_SHAPES(ZMI_SHAPE)
#undef ZMI_SHAPE
  return hipErrorInvalidValue;
}

template <int EPI>
hipError_t launch(const ZmiGemvArgs& a, hipStream_t s) {
  ZmiGemvForm f;
  if (!form_for(a, EPI, &f)) return hipErrorInvalidValue;
  if (a.w_fmt == ZMI_WFMT_FP8 && (f.kind == ZMI_FORM_ROWS_DENSE || f.kind == ZMI_FORM_ROWS)) {
    if constexpr (EPI == ZMI_EPI_SWIGLU || EPI == ZMI_EPI_RESIDUAL || EPI == ZMI_EPI_F32)  // rows_launch's fp8 epilogues
      return f.kind == ZMI_FORM_ROWS_DENSE ? launch_rows<EPI, 1, true, ZMI_WFMT_FP8>(a, s, f)
                                           : launch_rows<EPI, 2, false, ZMI_WFMT_FP8>(a, s, f);
    return hipErrorInvalidValue;
  }
  if (f.kind == ZMI_FORM_ROWS_DENSE) return launch_rows<EPI, 1, true>(a, s, f);
  if (f.kind == ZMI_FORM_ROWS) return launch_rows<EPI, 2, false>(a, s, f);
  if (a.w_fmt == ZMI_WFMT_FP8) {
    if constexpr (EPI == ZMI_EPI_STORE || EPI == ZMI_EPI_SWIGLU || EPI == ZMI_EPI_RESIDUAL || EPI == ZMI_EPI_F32)
      return launch_shape<EPI, ZMI_WFMT_FP8>(a, s, f);
    return hipErrorInvalidValue;
  }
  return launch_shape<EPI, ZMI_WFMT_BF16>(a, s, f);
}

}  // namespace zmi_gemv
