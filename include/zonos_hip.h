/*
 * zonos_hip.h — C ABI of libzonos_hip.so, the MI355X (gfx950) hot path of Zonos generate() +
 * DACAutoencoder.decode().
 *
 * The reference (BreakTheBeta/Zonos_Vibes) is pure Python with no FFI; its device work is
 * ATen ops called from the functions cited below. This ABI is the boundary the Python host
 * (zonos_vibes_amd/) binds with ctypes to replace them. Conventions:
 *   - every pointer is a device pointer owned by the caller (allocated by torch), unless noted;
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream);
 *   - every function returns 0 on success or a nonzero status; zmi_last_error() explains it;
 *   - no function allocates or synchronises, so every launcher can be hipGraph-captured;
 *   - gfx950 only: several launchers size their workgroups for its 160 KB of LDS (the SSD prefill scan ~148 KB, the
 *     staged split-K GEMM ~132 KB, the DAC's staged convs up to 156 KB) and return an error, with no smaller-LDS
 *     fallback, where the device grants less.
 */
#ifndef ZONOS_HIP_H
#define ZONOS_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * Weight-streaming GEMV / skinny GEMM:  out[m, n] = sum_k A[m, k] W[n, k]  (+ fused epilogue)
 * Replaces nn.Linear in zonos/backbone/_torch.py:114-115 (in_proj/out_proj), :147-152 (fc1/fc2)
 * and zonos/model.py:100-101 (apply_heads); the LayerNorm prologue replaces nn.LayerNorm at
 * _torch.py:62,88,90 (norm, norm2, norm_f).
 * ------------------------------------------------------------------------------------- */
enum {
  ZMI_EPI_STORE = 0,    /* out bf16 [M][ldo]                                                   */
  ZMI_EPI_RESIDUAL = 1, /* out bf16 [M][ldo] += bf16(acc)          (_torch.py:100-101)          */
  ZMI_EPI_QKV = 2,      /* q -> out, rope(k) / v -> KV cache        (_torch.py:18-49, 117-126)  */
  ZMI_EPI_SWIGLU = 3,   /* out bf16 [M][F] = y * silu(gate)        (_torch.py:150-152)          */
  ZMI_EPI_LOGITS = 4,   /* out f32 [M][9][1026] = bf16(acc).float() (model.py:100-101,111)      */
  ZMI_EPI_F32 = 5       /* out f32 [M][ldo] raw fp32 sums (tests)                              */
};
enum { ZMI_PACK_IDENTITY = 0, ZMI_PACK_SWIGLU = 1 };
/* prologue of the activation rows (ZmiGemvArgs.pro):
 *   AUTO   LayerNorm if ln_w, else the rows as they are;
 *   ADDLN  mamba-ssm layer_norm_fn(X, ln_w, ln_b, residual = aux, prenorm=True): s = X + aux in fp32,
 *          LayerNorm(s); res_out (may be NULL) <- bf16(s), written by one workgroup per row tile
 *          (res_out must not alias aux: other workgroups still read aux);
 *   GRMS   mamba-ssm RMSNormGated(X, z) * ln_w (norm_before_gate=False, one group), aux = the f32 gate
 *          z * sigmoid(z) (zmi_mamba2_step's gz), at most 4 rows. */
enum { ZMI_PRO_AUTO = 0, ZMI_PRO_ADDLN = 2, ZMI_PRO_GRMS = 3, ZMI_PRO_GRMS_G = 4 };
/* weight format (ZmiGemvArgs.w_fmt):
 *   BF16  bf16 weights in layout M8 (zmi_pack_weight);
 *   FP8   weight-only 8-bit: W[n][k] = 2^w_exp[n] * q[n][k], q OCP float8_e4m3fn (never NaN), one signed exponent per
 *         packed column; layout M8F8 (zonos_vibes_amd/quant.py pack_m8f8): the bytes of the M8 chunks 2p and 2p + 1 of
 *         a column group share one 1 KiB piece, lane l holding its 8 weights of chunk 2p then its 8 of chunk 2p + 1.
 *         Every 2^w_exp q is a bf16 value, and zmi_gemv_launch returns the bits of the BF16 launch on those dequantised
 *         weights. Built for
 *           - the SWIGLU, RESIDUAL and F32 epilogues with the plain / LayerNorm prologue, K in {512, 1024, 2048, 8192}
 *             (the MLP projections);
 *           - the STORE epilogue of the Mamba2 mixers' projections: in_proj under ADDLN (K 512 / 2048, any M), out_proj
 *             under GRMS / GRMS_G (K 1024 / 4096, M <= 4) or plain at K 1024 / 4096 (any M). A plain STORE launch at
 *             K 512 / 2048 / 8192, the QKV and LOGITS epilogues and the LayerNorm prologue with STORE are refused;
 *           - zmi_mamba_block / zmi_mamba_block_pf (the in_proj role; a kernel of its own name).
 *         The MLP launches take every launch form the bf16 ones do: over more than 16 plain rows at K = 2048 (fc1) the
 *         many-row form (zmi_gemv_form reports ZMI_FORM_ROWS / ZMI_FORM_ROWS_DENSE while ZMI_OPT_FP8_ROWS is set), its
 *         bytes expanded to bf16 registers once per workgroup; fc2 (K = 8192, RESIDUAL) also as a split-K GEMM through
 *         entry points of its own, zmi_gemv_splitk_f8 / zmi_gemv_splitk_f8_ln. Every form gives the same bits.
 *         zmi_gemv_splitk / zmi_gemv_splitk_ln and zmi_attn_block read bf16 only, and no many-row form reads the
 *         Mamba2 mixers' fp8 projections: a prefill expands such a projection with zmi_unpack_fp8 and runs the bf16
 *         forms on the result. */
enum { ZMI_WFMT_BF16 = 0, ZMI_WFMT_FP8 = 1 };

typedef struct ZmiGemvArgs {
  const void* W;        /* packed weight (zmi_pack_weight, layout M8; w_fmt FP8: layout M8F8)   */
  const void* X;        /* bf16 [M][ldx] activations                                          */
  int M, N, K, ldx;     /* N = packed (padded) columns, multiple of 8; K in {512 .. 8192}, pow2  */
  int groups;           /* 8-column groups per workgroup: 0 = library choice, else 1 or 2      */
  int reserved;
  const void* ln_w;     /* bf16 [K] LayerNorm weight, or NULL for a plain GEMV                */
  const void* ln_b;     /* bf16 [K] LayerNorm bias                                             */
  float eps;
  void* out;
  int ldo;
  int n_valid;          /* real (unpadded) columns                                             */
  const int* row_kv;    /* QKV: [M] KV-cache row of each activation row                        */
  const int* row_pos;   /* QKV: [M] position (<0: inactive row, nothing written)               */
  void* k_cache;        /* QKV: bf16 K cache [rows][hkv][smax][hd] of this layer               */
  void* v_cache;        /* QKV: bf16 V cache, transposed: [rows][hkv][hd][smax]                 */
  int smax, hq, hkv, hd;
  const float* rope;    /* [16384][hd/2][2] (cos, sin) fp32 (_torch.py:9-15)                  */
  void* diag;           /* NULL; diagnostic builds only (-DZMI_GEMV_STAMPS): phase stamps       */
  int pro;              /* ZMI_PRO_*                                                            */
  int ld_aux;           /* row stride of aux and res_out (elements)                             */
  const void* aux;      /* ADDLN: bf16 residual rows; GRMS: f32 gate rows z * sigmoid(z); GRMS_G: f32 rows g = y * gate (X unused) */
  void* res_out;        /* ADDLN: bf16 [M][ld_aux] new residual, or NULL                         */
  int w_fmt;            /* ZMI_WFMT_*: 0 = bf16 (layout M8), 1 = E4M3 bytes (layout M8F8) with w_exp */
  int reserved2;
  const void* w_exp;    /* FP8: int8 [N] power-of-two exponent of each packed column              */
} ZmiGemvArgs;

int zmi_pack_weight(const void* src, void* dst, int n_src, int k, int n_pad, int mode, void* stream);
/* Expand an FP8 weight (n_pad * k bytes in layout M8F8, int8 w_exp[n_pad] in packed column order) into the bf16 layout
 * M8 (2 * n_pad * k bytes at m8_out): byte for byte zmi_pack_weight of the dequantised weight 2^w_exp q. n_pad % 8 == 0,
 * k % 128 == 0, both weights 16-byte aligned. A streaming kernel (16 bytes in, 32 out per lane): no reduction, exact. */
int zmi_unpack_fp8(const void* m8f8, const void* w_exp, int n_pad, int k, void* m8_out, void* stream);
/* One kernel for every M: a row's result is bit-identical whatever the batch it is computed in. */
int zmi_gemv_launch(const ZmiGemvArgs* args, int epi, void* stream);
/* The launch form zmi_gemv_launch(args, epi) would take, computed by the code it dispatches on; launches nothing and
 * reads no pointer's target (host only: callable without a GPU). kind: the gemv_body kernel, or the K = 2048 many-row
 * form on M8 or dense-pair MFMAs (ZMI_OPT_GEMM_ROWS); (G, W, NL, RT): column groups per workgroup, waves per group,
 * 1 KiB weight chunks per lane, rows per tile; ntw: 1 = the single-tile instantiation (M <= RT), 0 = the tile loop;
 * pro: the resolved prologue (0 plain, 1 LayerNorm, else ZMI_PRO_*); the grid: n_cb column blocks x n_rt row tiles,
 * rpw row tiles per workgroup. Returns non-zero (zmi_last_error) exactly where zmi_gemv_launch refuses the arguments. */
enum { ZMI_FORM_BODY = 0, ZMI_FORM_ROWS = 1, ZMI_FORM_ROWS_DENSE = 2 };
typedef struct ZmiGemvForm {
  int kind;             /* ZMI_FORM_*                                                          */
  int G, W, NL, RT;
  int ntw, pro;
  int n_cb, n_rt, rpw;
} ZmiGemvForm;
int zmi_gemv_form(const ZmiGemvArgs* args, int epi, ZmiGemvForm* out);
/* Many-row fc2 (K = 8192) or out_proj (K = 2048), EPI_RESIDUAL, plain (reference _torch.py:100-101,141,152), or
 * the hybrid's Mamba2 out_proj (K = 4096 = d_ssm, EPI_STORE: mamba_ssm out_proj of the prefill): a split-K GEMM
 * (one workgroup per 64-column block, K segment -- 8 x 1024 / 4 x 1024 / 4 x 512, the GEMV's wave split -- and
 * row group, ZMI_OPT_SPLITK_WGS), fp32 segment sums in `part`, then a reduce launch adding the segments in K
 * order + the residual / store epilogue. Bit-identical to zmi_gemv_launch for every row (the GEMV's per-segment
 * MFMA chains and segment order); reads the activation rows once per column block instead of once per column
 * group. part: zmi_gemv_splitk_floats(M, N) floats. */
int zmi_gemv_splitk(const ZmiGemvArgs* args, int epi, float* part, int64_t part_floats, void* stream);
/* The same with ln_w != NULL (N = 2048): the reduce also writes LayerNorm(new row; ln_w, ln_b, eps) to xn [M][ldxn],
 * bit-identical to zmi_layernorm_rows of the new rows, so the next op's LayerNorm pre-pass is not launched. */
int zmi_gemv_splitk_ln(const ZmiGemvArgs* args, int epi, float* part, int64_t part_floats, const void* ln_w,
                       const void* ln_b, float eps, void* xn, int ldxn, void* stream);
int64_t zmi_gemv_splitk_floats(int M, int N);
/* The split-K GEMM over FP8 weights, for fc2: w_fmt == ZMI_WFMT_FP8 with w_exp (8-byte aligned), K = 8192 and
 * EPI_RESIDUAL only; the other conditions are zmi_gemv_splitk_ln's, and everything else is refused before any launch
 * with `out` and `part` untouched. `part` holds the unscaled segment sums; the reduce adds the 8 segments in order,
 * multiplies by the column's 2^w_exp[n] and applies the residual epilogue (and the LayerNorm): the bits of
 * zmi_gemv_launch over the same FP8 weights, hence of the BF16 launch on the dequantised ones. */
int zmi_gemv_splitk_f8(const ZmiGemvArgs* args, int epi, float* part, int64_t part_floats, void* stream);
int zmi_gemv_splitk_f8_ln(const ZmiGemvArgs* args, int epi, float* part, int64_t part_floats, const void* ln_w,
                          const void* ln_b, float eps, void* xn, int ldxn, void* stream);
/* out[r] = LayerNorm(x[r]) bf16, r < m (nn.LayerNorm, _torch.py:62: norm_f for the backbone plugin),
 * with the GEMV LayerNorm prologue's arithmetic; k in {512, 1024, 2048, 4096}. */
int zmi_layernorm_rows(const void* x, int ldx, int m, int k, const void* w, const void* b, float eps, void* out,
                       int ldo, void* stream);

/* ---------------------------------------------------------------------------------------
 * Attention: GQA scaled-dot-product attention over the KV cache, one query position per
 * (query row). Replaces F.scaled_dot_product_attention(q, k, v, is_causal, enable_gqa)
 * at zonos/backbone/_torch.py:136 for decode (1 query) and prefill (causal = position bound).
 * ------------------------------------------------------------------------------------- */
/* K cache [rows][hkv][smax][hd], V cache transposed [rows][hkv][hd][smax] (bf16, as the QKV
 * epilogue writes them). q_kv_row may be NULL: query i then reads KV-cache row i (decode).
 * Softmax in the 512-key block structure of the reference's CPU kernel (probabilities rounded to
 * bf16 before P.V). Keys are processed in chunks of zmi_attention_chunk() keys whose partials go
 * to part_o [n_query*hkv][chunks][hq/hkv][hd] and part_lm [..][2] (zmi_attention_partial_floats
 * floats of o; 1/64 of that for lm), merged in-kernel by each query's last-arriving chunk.
 * `work` holds zmi_attention_work_bytes(...) zero-initialised bytes, re-armed by every launch; its
 * first 4 bytes become nonzero if a cross-chunk hand-off timed out. */
int zmi_attention(const void* q, int ldq, const void* k_cache, const void* v_cache, const int* q_kv_row,
                  const int* q_pos, int n_query, int hq, int hkv, int hd, int smax, int max_pos, void* out,
                  int ldo, float* part_o, float* part_lm, void* work, void* stream);
/* Same op with an explicit kernel choice: 0 = library choice (as zmi_attention), 1 = the chunked
 * kernel above (any length, one launch), 2 = the chunked kernel as two launches (scores and maxima, then the
 * rest: no workgroup waits on another), 3 = three launches (the merge as its own launch), 4 / 8 = the
 * whole-query kernel with that many output-dim slices per (query, kv head): every slice reads all of the
 * query's keys and no workgroup waits on another (max_pos < zmi_attention_max_keys_whole()). All variants
 * return identical bits. */
int zmi_attention_variant(const void* q, int ldq, const void* k_cache, const void* v_cache, const int* q_kv_row,
                          const int* q_pos, int n_query, int hq, int hkv, int hd, int smax, int max_pos, void* out,
                          int ldo, float* part_o, float* part_lm, void* work, int variant, void* stream);
int zmi_attention_max_keys_whole(void);
/* The kernel variant zmi_attention_variant / zmi_attention_pf run for `variant` (0 = library choice: 5, the
 * 512-key block form, from 32 (query, kv head) units, else 1, the chunked kernel); no launch. */
int zmi_attention_pick(int n_query, int hkv, int variant);
/* Fused decode block (reference _torch.py:114-136 for one decode step): the LayerNorm'd QKV
 * projection `qkv` (EPI_QKV arguments as for zmi_gemv_launch: M <= 16 rows, K = 2048, 4 query heads
 * per kv head, row_kv set) and the attention of every row at its position, in ONE launch whose
 * attention workgroups load the cached K / V while the projection streams its weights. q, the KV
 * cache writes and attn_out (bf16 [M][ldo]) are bit-identical to zmi_gemv_launch(QKV) followed by
 * zmi_attention. gran: zmi_attn_block_gran_words(M, hkv) u64 words of {value, tag = position + 1}
 * hand-off granules; a row's words must not hold tag pos + 1 from an earlier use when it runs at
 * position pos (zero them when a row starts a new utterance; consecutive steps need nothing).
 * err: set nonzero if a wait gave up (or a row's position exceeds the form's reach, see below).
 * slices: 4 or 8 workgroups per (row, kv head), optionally | ZMI_ATTNBLK_SELF:
 *   plain      the slices exchange scores (each scores 1/slices of the keys); positions < 1280;
 *   SELF       every slice scores all keys itself, nothing is exchanged between slices; positions < 1024;
 *   SPLIT      (slices 8) one workgroup per 128-key chunk: each reads only its chunk's K / V, the chunks
 *              exchange their maxima and P.V partials (two small hand-offs); positions < 1024.
 * zmi_attn_block_max_pos(slices) is the last position the form accepts; any smax is allowed (the engine
 * picks the form per step from the rows' positions). The projection's prologue is LayerNorm (pro AUTO with ln_w) or
 * ADDLN (pro ZMI_PRO_ADDLN: the hybrid's layer_norm_fn(hidden, residual), aux / ld_aux / res_out as for
 * zmi_gemv_launch). */
int zmi_attn_block(const ZmiGemvArgs* qkv, void* gran, unsigned* err, void* attn_out, int ldo, int slices,
                   void* stream);
enum { ZMI_ATTNBLK_SELF = 256, ZMI_ATTNBLK_SPLIT = 512 };
int zmi_attn_block_max_pos(int slices);
int64_t zmi_attn_block_gran_words(int rows, int hkv);
/* zmi_attn_block plus `blocks` prefetch-only workgroups that read ptr[0..1][0 .. bytes) once during the
 * attention phase (HBM is nearly idle there): the next launches' weights (out_proj, the head of fc1) are
 * then served from the Infinity Cache. Results are those of zmi_attn_block; `sink` is a scratch word the
 * prefetch may write (never read). */
typedef struct ZmiPrefetch {
  const void* ptr[2];
  int64_t bytes[2];
  unsigned* sink;
  int blocks, reserved;
} ZmiPrefetch;
int zmi_attn_block_pf(const ZmiGemvArgs* qkv, void* gran, unsigned* err, void* attn_out, int ldo, int slices,
                      const ZmiPrefetch* prefetch, void* stream);
/* zmi_attn_block_pf with the layer's out_proj in the same launch (the chunk-split forms: slices = 8 or 24 |
 * ZMI_ATTNBLK_SPLIT). With the LayerNorm prologue `oproj` holds the plain EPI_RESIDUAL GEMV arguments as for zmi_gemv_launch;
 * with the ADDLN prologue (the hybrid's MHA blocks) the role stores bf16(out_proj) to oproj->out (EPI_STORE: the hidden
 * rows the next block's add + LayerNorm reads; not the residual buffers). The LayerNorm case:
 * (W = out_proj weights, K = hq hd, N % 16 == 0, X = attn_out, out = the residual rows x, M = qkv->M), replacing
 * reference _torch.py:115,140 and the residual add :100. Its workgroups follow the attention ones: they load their
 * weight slice at their start and gather the attention output from the merging workgroups' {pair, tag} granules
 * (in the unit's granule area) once those workgroups' flags carry the row's tag, so no out_proj launch follows.
 * attn_out is still written. Results are bit-identical to zmi_attn_block_pf + zmi_gemv_launch(oproj). */
int zmi_attn_block_oproj(const ZmiGemvArgs* qkv, const ZmiGemvArgs* oproj, void* gran, unsigned* err, void* attn_out,
                         int ldo, int slices, const ZmiPrefetch* prefetch, void* stream);
/* zmi_attention_variant plus prefetch-only workgroups (variant 0 / 1: `prefetch->blocks` of them at the end
 * of the grid) that read prefetch->ptr[0..1][0 .. bytes) once, so the next launches (out_proj, the head of
 * fc1) find those weights in the Infinity Cache: they run on the CUs the chunks vacate, while the chunks
 * exchange maxima and merge (HBM nearly idle). prefetch may be NULL. Results are zmi_attention_variant's. */
int zmi_attention_pf(const void* q, int ldq, const void* k_cache, const void* v_cache, const int* q_kv_row,
                     const int* q_pos, int n_query, int hq, int hkv, int hd, int smax, int max_pos, void* out, int ldo,
                     float* part_o, float* part_lm, void* work, int variant, const ZmiPrefetch* prefetch,
                     void* stream);
int64_t zmi_attention_work_bytes(int n_query, int hq, int hkv, int hd, int max_pos);
int64_t zmi_attention_partial_floats(int n_query, int hq, int hkv, int hd, int max_pos);
int zmi_attention_chunk(void);
/* Causal prefill attention: many query positions per sequence in one launch, QT = zmi_attention_prefill_queries(hq,
 * hkv) = 16 / (hq / hkv) consecutive positions sharing every K / V tile they read (hq / hkv in {1, 2, 4}; -1
 * otherwise). Sequence i owns rows q_row0 .. q_row0 + len - 1 of q and out; they sit at positions pos0 .. pos0 +
 * len - 1 of KV-cache row kv_row, and the row at position p attends keys 0 .. p of that cache row (caches as for
 * zmi_attention, already written for those positions). One workgroup per (tile, kv head); `tiles` lists the tiles
 * in dispatch order, most keys first: {seq, off} = positions pos0 + off .. pos0 + min(off + QT, len) - 1 of sequence
 * seq, off a multiple of QT, every sequence covered exactly once, so n_tiles = sum of ceil(len / QT).
 * seqs and tiles are device arrays; seqs_host is the host copy of seqs, which the call checks before it launches
 * (len >= 0, pos0 + len <= smax, no negative row, n_tiles as above). n_seq == 0 or every len == 0: nothing is
 * launched. No work or partial buffers, no hand-off between workgroups. Every out row holds the bits
 * zmi_attention_variant gives for the same (kv_row, position); only rows of a sequence are written.
 * V is zeroed past each TILE's last position, not each row's: a non-finite V at a later position of the same tile
 * reaches the tile's earlier rows (it poisons every later row in any form). */
typedef struct ZmiAttnSeq { int q_row0, len, kv_row, pos0; } ZmiAttnSeq;
typedef struct ZmiAttnTile { int seq, off; } ZmiAttnTile;
int zmi_attention_prefill(const void* q, int ldq, const void* k_cache, const void* v_cache, const ZmiAttnSeq* seqs,
                          int n_seq, int64_t n_tiles, const ZmiAttnTile* tiles, const ZmiAttnSeq* seqs_host, int hq,
                          int hkv, int hd, int smax, void* out, int ldo, void* stream);
int zmi_attention_prefill_queries(int hq, int hkv);

/* ---------------------------------------------------------------------------------------
 * Sampler + EOS state machine + delay-pattern frame write, per utterance slot.
 * Replaces model.py:112-115 (CFG), :266-267/280 (EOS logit bias), sampling.py:99-182
 * (repetition penalty, greedy / softmax / unified / top-p / top-k / min-p / exponential race)
 * and model.py:283-299 (EOS diagonal, masked_scatter_ frame compaction, counters).
 * ------------------------------------------------------------------------------------- */
typedef struct ZmiSampling {
  float temperature, top_p, min_p, linear, conf, quad, rep_penalty, cfg_scale;
  int top_k, rep_window;
  uint64_t seed;
} ZmiSampling;

typedef struct ZmiSlots {
  int* active;      /* [S] 1 while generating                                              */
  int* pos;         /* [S] tokens in the KV cache (= next position)                         */
  int* offset;      /* [S] last written delayed-frame index (reference `offset`)            */
  int* remaining;   /* [S] reference `remaining_steps`                                      */
  int* stopping;    /* [S] reference `stopping`                                             */
  int* step;        /* [S] decode steps done                                                */
  int* delayed;     /* [S][9][tcap] delayed codes (int32; -1 unknown, 1024 EOS, 1025 mask)   */
  const ZmiSampling* params; /* [S]                                                           */
  const int* total_len; /* [S] delayed length P + N + 9 (frames at or past it are not written) */
  int tcap;
  int n_slots;
  int rows_per_slot; /* the row layout of zmi_sample_step (modes 0, 1), zmi_sample_step_greedy and zmi_embed_step:
                      * 0 or 2 = paired: slot s owns logits / activation / KV rows 2s (conditional) and 2s + 1
                      *          (unconditional), the CFG pair of model.py:142; the score is u + (c - u) * cfg_scale;
                      * 1      = single (guidance-free generation, the reference's cfg_scale == 1: model.py:112,
                      *          134-136, 193): slot s owns row s, the score is that row's logit as it is
                      *          (ZmiSampling.cfg_scale is ignored, no second row is read), the kernels write
                      *          row_kv[s] = s, row_pos[s] and x[s] and touch nothing of rows >= n_slots;
                      * anything else is an error before any launch. A zero-initialised trailing field, so a caller
                      * that fills the eleven fields above keeps the paired layout (zmi_version 10). */
} ZmiSlots;

/* mode 0 = decode step (bias + penalty + FSM), 1 = prefill (no bias, no penalty, no FSM).
 * With emb != NULL the slot's next input frame is embedded in the same launch (x[2s], x[2s+1],
 * model.py:97-98,142; single layout: x[s]) and row_kv/row_pos (optional) receive the next step's KV row / position.
 * Everything after the score (column 1025 = -inf, EOS bias, penalty, sampling, the EOS state machine, the frame
 * write, the noise counters) is the same code in both layouts. */
int zmi_sample_step(const ZmiSlots* slots, const float* logits_rows, const float* noise, int* next_tokens,
                    unsigned* counters, int mode, int slot_begin, int slot_count, const void* emb, int d, void* x,
                    int* row_kv, int* row_pos, void* stream);
/* zmi_sample_step mode 0 for a launch whose slots all sample greedily (temperature <= 0; the caller
 * guarantees it): one workgroup per slot, no in-launch hand-off between codebooks; identical results. */
int zmi_sample_step_greedy(const ZmiSlots* slots, const float* logits_rows, int* next_tokens, int slot_begin,
                           int slot_count, const void* emb, int d, void* x, int* row_kv, int* row_pos, void* stream);
/* sample_from_logits (sampling.py:117-182) on its own: logits f32 [batch][9][1026] as given (no CFG,
 * no EOS bias), optional generated_tokens int32 [batch][9][gen_len] for the repetition penalty,
 * one parameter block (device), optional exponential noise [batch][9][1026]; tokens int32 [batch][9]. */
int zmi_sample_logits(const float* logits, const int* generated, int gen_len, int batch, const ZmiSampling* params,
                      const float* noise, int* tokens, void* stream);
/* apply_delay_pattern / revert_delay_pattern (codebook_pattern.py:5-12) on int64 [batch][9][T]
 * (apply: out [batch][9][T + 9]; revert: T >= 9, out [batch][9][T - 9]). */
int zmi_apply_delay_pattern(const int64_t* codes, int64_t* out, int batch, int T, int64_t mask_token, void* stream);
int zmi_revert_delay_pattern(const int64_t* codes, int64_t* out, int batch, int T, void* stream);
/* x[2s], x[2s+1] = sum_k emb_k[delayed[s][k][offset[s]]]  (model.py:97-98,142; single layout: x[s]) and the
 * per-row (kv row, position) tables of the step (-1 position for inactive slots). Refused before any launch:
 * d not a positive multiple of 8, NULL emb or x. */
int zmi_embed_step(const ZmiSlots* slots, const void* emb, int d, void* x, int* row_kv, int* row_pos,
                   void* stream);
/* prefill embedding rows: x[s] = sum_k emb_k[codes[k][s]] for s < n (model.py:195). Refused before any launch:
 * n <= 0, d not a positive multiple of 8, ldx < d, ld_codes < n, NULL codes, emb or x. */
int zmi_embed_codes(const int* codes, int ld_codes, int n, const void* emb, int d, void* x, int ldx, void* stream);
/* delayed[slot] = apply_delay_pattern(prefix codes | -1)    (codebook_pattern.py:5-7). Refused before any launch:
 * slot out of range, total_len > tcap, a negative prefix_len or total_len, prefix_len > 0 with a NULL prefix. */
int zmi_delay_init(const ZmiSlots* slots, int slot, const int* prefix, int prefix_len, int total_len, void* stream);
/* out[9][T] int64 = revert_delay_pattern(delayed[slot]) with >=1024 -> 0 (model.py:309-311). Refused before any
 * launch: slot out of range, t_out + 9 > tcap, NULL out with t_out > 0. */
int zmi_delay_revert(const ZmiSlots* slots, int slot, int64_t* out, int t_out, void* stream);
/* frames t0 .. t0 + n - 1 of that result, out[9][n] int64: out[k][i] = delayed[slot][k][t0 + i + k + 1] with
 * >=1024 -> 0 (codebook_pattern.py:9-12, model.py:309-311). Frames below offset - 9 of a running slot are final,
 * so a streaming caller reads them before the utterance ends. Error when t0 < 0, n < 0 or t0 + n + 9 > tcap;
 * n == 0 launches nothing. */
int zmi_delay_revert_range(const ZmiSlots* slots, int slot, int t0, int n, int64_t* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * DAC 44.1 kHz decoder (DACAutoencoder.decode, autoencoder.py:25-27 -> transformers DacModel).
 * Activations are fp16, channels-last [T][C]; weights fp16 channel-blocked per tap [tap][Ci/32][Co][32] (one
 * 32-channel step of 16 output channels is 1 KiB contiguous: one LDS-DMA piece), except 1x1 convs (taps == 1):
 * [Co][Ci].
 * ------------------------------------------------------------------------------------- */
/* z[t][c] = sum_i (out_proj_i(codebook_i[codes[i][t]]))   (modeling_dac.py:347-371)          */
int zmi_dac_from_codes(const int64_t* codes, int T, const float* codebooks, const float* proj_w,
                       const float* proj_b, void* z, void* stream);
/* out[t_out][co] = epi( bias + sum_tap sum_ci W[tap][co][ci] * x[t_in][ci] ) with
 *   t_in = q + in_off + tap * tap_step, t_out = q * out_stride + out_phase, q in [0, n_out)
 * epilogue: + skip (fp16, optional), store raw (optional), snake(alpha) (optional) and/or the
 * raw fp32 value (optional, the encoder's latents). */
int zmi_dac_conv(const void* x, int t_in, int c_in, const void* w, const float* bias, int c_out, int taps,
                 int tap_step, int in_off, int n_out, int out_stride, int out_phase, int t_out, const void* skip,
                 void* out_raw, void* out_snake, const float* alpha, float* out_f32, void* stream);
/* DAC encode (DACAutoencoder.encode, autoencoder.py:22-23 -> DacModel.encode, modeling_dac.py:583-608).
 * col fp16 [T][32] = the 7 taps of encoder.conv1 around each sample (im2col, zero padded). */
int zmi_dac_im2col7(const float* wav, int t, void* col, void* stream);
/* residual VQ of latents f32 [T][1024] -> codes int64 [9][T] (modeling_dac.py:283-345, 123-173);
 * in_w [9][8][1024], in_b [9][8], codebooks [9][1024][8] raw and l2-normalised, codebooks_n2 =
 * |normalised row|^2 [9][1024], out_w [9][1024][8], out_b [9][1024]; all fp32. */
int zmi_dac_vq(const float* latents, int t, const float* in_w, const float* in_b, const float* codebooks,
               const float* codebooks_n, const float* codebooks_n2, const float* out_w, const float* out_b,
               int64_t* codes, void* stream);
/* polyphase ConvTranspose1d(c_in, c_out, k = 2 stride, stride, pad) of a DacDecoderBlock (modeling_dac.py:222-240),
 * every phase in one launch: w_phases fp16 [stride][2][c_in/32][c_out][32], phase rho's taps (rho + pad) % stride and
 * + stride, transposed; out [stride t_in][c_out] raw and / or Snake'd with alpha. */
int zmi_dac_conv_t(const void* x, int t_in, int c_in, const void* w_phases, const float* bias, int c_out, int stride,
                   int pad, void* out_raw, void* out_snake, const float* alpha, void* stream);
/* final Snake'd [T][c_in] -> conv k7 (c_in->1) -> tanh -> f32 [T]  (modeling_dac.py:438-441), on the
 * MFMA conv kernel: w_pad fp16 [7][c_in/32][32][32] (output channel 0 = the filter, 1..31 zero), bias_pad f32 [32]. */
int zmi_dac_conv_out(const void* x, int t, int c_in, const void* w_pad, const float* bias_pad, float* out,
                     void* stream);
/* samples q0 .. q0 + n - 1 of that result only, out f32 [n] (the streaming decoder's crop of a window: each sample
 * with the bits zmi_dac_conv_out gives it). Error unless 0 <= q0, 0 <= n, q0 + n <= t. */
int zmi_dac_conv_out_range(const void* x, int t, int c_in, const void* w_pad, const float* bias_pad, int q0, int n,
                           float* out, void* stream);
/* The decoder's entry points over `lanes` independent utterances of one shape in one launch (the batched streaming
 * window, DACAutoencoder._decode_lanes): the arguments of the single-utterance entry point, then lanes and, for every
 * activation buffer the call touches, its lane stride in elements (lane l's buffer starts l strides after the
 * pointer given; codes int64 [9][T] per lane). Weights, bias and alpha are shared; t_in, n_out and the crop are the
 * same for every lane. A lane is a pointer offset (grid z = lane * phases + phase): each output element has the K
 * order and MFMA chain the single-utterance launch gives it, so the bits are the same, and rows outside a lane's
 * [0, t_in) are zeros, never a neighbour's data. The tile choice counts every lane's workgroups. The single entry
 * points are these with lanes = 1 (strides ignored). Error (no launch) when lanes < 1, when lanes > 1 and a present
 * buffer's stride is smaller than one lane's extent (t_in c_in for x, t_out c_out for skip / raw / snake / f32, n
 * for conv_out_range's out, 9 T for codes, 1024 T for z), or when lanes * phases (from_codes: lanes) > 65535. */
int zmi_dac_from_codes_lanes(const int64_t* codes, int T, const float* codebooks, const float* proj_w,
                             const float* proj_b, void* z, int lanes, int64_t ls_codes, int64_t ls_z, void* stream);
int zmi_dac_conv_lanes(const void* x, int t_in, int c_in, const void* w, const float* bias, int c_out, int taps,
                       int tap_step, int in_off, int n_out, int out_stride, int out_phase, int t_out, const void* skip,
                       void* out_raw, void* out_snake, const float* alpha, float* out_f32, int lanes, int64_t ls_x,
                       int64_t ls_skip, int64_t ls_raw, int64_t ls_snake, int64_t ls_f32, void* stream);
int zmi_dac_conv_t_lanes(const void* x, int t_in, int c_in, const void* w_phases, const float* bias, int c_out,
                         int stride, int pad, void* out_raw, void* out_snake, const float* alpha, int lanes,
                         int64_t ls_x, int64_t ls_raw, int64_t ls_snake, void* stream);
int zmi_dac_conv_out_range_lanes(const void* x, int t, int c_in, const void* w_pad, const float* bias_pad, int q0,
                                 int n, float* out, int lanes, int64_t ls_x, int64_t ls_out, void* stream);
/* Range form of zmi_dac_conv_t_lanes (the carried-state streaming decoder's transposed conv): output rows n0 .. n0 + n
 * - 1 only, written to out rows 0 .. n - 1 (out_raw / out_snake point at row n0; lane strides as above, extent n c_out).
 * x row 0 is input row x0 of the utterance and t_in rows are given; rows outside them are zeros. The range need not
 * be aligned to the stride (a streaming frontier is stride F - pad): every phase has its own q range. Each row has the
 * bits zmi_dac_conv_t_lanes gives it and nothing outside the range is written; n = 0 launches nothing. Error (no
 * launch) unless stride >= 2, 0 <= n0, 0 <= n, n0 + n <= stride (x0 + t_in) and the first row read, (n0 + pad) / stride - 1, is
 * >= x0 or is the zero padding before row 0 (x0 = 0). */
int zmi_dac_conv_t_range_lanes(const void* x, int x0, int t_in, int c_in, const void* w_phases, const float* bias,
                               int c_out, int stride, int pad, int n0, int n, void* out_raw, void* out_snake,
                               const float* alpha, int lanes, int64_t ls_x, int64_t ls_raw, int64_t ls_snake,
                               void* stream);
/* Carried-state streaming decode: copies between a per-lane state pool (pool_lanes lanes of pool_lane_units each) and
 * the dense scratch of one launch sequence, ONE launch over all lanes and segments. Units are 16 bytes (one vector
 * load / store). For group lane l = 0 .. lanes - 1, pool lane lane_ids[l] (DEVICE int32 array; any subset of the
 * pool, in any order, no id twice in a scatter) and every segment: pool[id][pool_off .. + count) <->
 * scratch[scratch_off + l scratch_ls .. + count); mode ZMI_DAC_MOVE_GATHER copies pool -> scratch, _SCATTER scratch ->
 * pool, _ZERO writes zeros to the scratch segments (the zero state of an utterance's first push; the pool is not
 * read). segs is a HOST array of n_segs <= ZMI_DAC_MOVE_SEGS segments. Nothing outside the segments is written; an id
 * outside the pool moves nothing. Error (no launch) on another mode, when a segment leaves a lane's state or the
 * scratch, or scratch_ls < count with lanes > 1. */
#define ZMI_DAC_MOVE_SEGS 48
#define ZMI_DAC_MOVE_GATHER 0
#define ZMI_DAC_MOVE_SCATTER 1
#define ZMI_DAC_MOVE_ZERO 2
typedef struct ZmiDacMoveSeg { uint32_t pool_off, scratch_off, count, scratch_ls; } ZmiDacMoveSeg;
int zmi_dac_state_move(void* pool, int64_t pool_lane_units, int pool_lanes, void* scratch, int64_t scratch_units,
                       const int* lane_ids, int lanes, const ZmiDacMoveSeg* segs, int n_segs, int mode, void* stream);

/* ---------------------------------------------------------------------------------------
 * PCM16 egress (the reference server's float -> 16-bit PCM conversion, server.py:142-146:
 *   wav_numpy = np.clip(wav_numpy, -1.0, 1.0); wav_int16 = (wav_numpy * 32767).astype(np.int16)
 * which numpy evaluates in fp32 and truncates), for many waveform pieces in one launch.
 * ------------------------------------------------------------------------------------- */
typedef struct ZmiPcmSeg { const float* src; int64_t n; int64_t dst; } ZmiPcmSeg;  /* n samples -> out[dst .. dst + n) */
/* out[dst + j] = (int16) trunc(fl32(clamp(src[j], -1, 1) * 32767.0f)) for every segment: truncation toward zero,
 * +-inf -> +-32767, -0.0 and subnormals -> 0, NaN -> 0. segs: DEVICE array of n_segs segments, dst ascending and
 * non-overlapping (n may be 0); total = the last dst + n. src needs 4-byte alignment only and dst is any int16 index
 * (out 2-byte aligned): a segment's ends go elementwise, its aligned middle in 8-byte stores. Nothing outside the
 * segments' ranges is written; n_segs = 0 or total = 0 launches nothing. */
int zmi_pcm16_pack(const ZmiPcmSeg* segs, int n_segs, int64_t total, int16_t* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Sample-rate conversion orig_rate -> new_rate (the reference's torchaudio.functional.resample with its defaults,
 * autoencoder.py:17-20): g = gcd, o = orig_rate / g, n = new_rate / g, W the table's half width and T = 2 W + o
 * (speaker.resample_kernel(o, n)). For an utterance x[0 .. N), output j < ceil(n N / o) is
 *   y[j] = sum_{t < T} xz[(j / n) o - W + t] * kern[j % n][t],   xz = x inside [0, N), 0 outside,
 * in fp32: four accumulators a0..a3 from +0, tap t (ascending) into a[t & 3] by one fused multiply-add, result
 * (a0 + a1) + (a2 + a3); the order depends on t alone, never on the lane, the launch shape or the chunking.
 * One launch converts many independent pieces, each a stretch of one utterance's outputs:
 * ------------------------------------------------------------------------------------- */
typedef struct ZmiResampleSeg {
  const float* carry; int64_t n_carry;   /* the lane's kept tail: the utterance's samples i0 .. i0 + n_carry          */
  const float* src;   int64_t n_src;     /* new samples: i0 + n_carry .. i0 + n_carry + n_src                         */
  int64_t i0, n_total;                   /* n_total: the utterance's length if this piece ends it, else -1            */
  int64_t j0, n_out, dst;                /* the utterance's outputs j0 .. j0 + n_out -> out[dst .. dst + n_out)       */
  float* carry_out;   int64_t n_keep;    /* zmi_resample_carry: the last n_keep samples of (carry, src) go here       */
} ZmiResampleSeg;
/* Samples below 0, at or above n_total (when >= 0) and outside [i0, i0 + n_carry + n_src) read as 0. segs: DEVICE
 * array of n_segs segments, dst ascending and non-overlapping inside total_out (n_out may be 0); segs_host: the HOST
 * copy of the same table, checked before anything is launched (counts, pointers, dst order, that every tap of a piece
 * that is not final lies in its carry or src, that a final piece ends at n_total and emits no more than
 * ceil(n n_total / o)): a bad table or a NULL pointer returns non-zero and nothing is written. kern_t: DEVICE
 * [T][n] fp32, the table transposed (phases contiguous). n (2 W + o) <= 2^22. Nothing outside the segments' output
 * ranges is written; n_segs = 0 or total_out = 0 launches nothing. */
int zmi_resample(const ZmiResampleSeg* segs, const ZmiResampleSeg* segs_host, int n_segs, int64_t total_out,
                 const float* kern_t, int o, int n, int W, float* out, void* stream);
/* carry_out[0 .. n_keep) = the last n_keep (<= n_carry + n_src, <= T) samples of (carry, src) for every segment:
 * the tail a streaming lane keeps for its next piece. carry_out is never the carry it is made from (the caller
 * double-buffers), so this launch and zmi_resample on the same table may run in either order. */
int zmi_resample_carry(const ZmiResampleSeg* segs, const ZmiResampleSeg* segs_host, int n_segs, int o, int n, int W,
                       void* stream);

/* ---------------------------------------------------------------------------------------
 * Speaker encoder (Zonos.make_speaker_embedding, model.py:90-95 -> SpeakerEmbeddingLDA, speaker_cloning.py:388-412:
 * ResNet293 with SimAM blocks). Activations are fp16 channels-last [H][W][C] (H the mel axis, W time; the _lanes
 * entry points take many clips of their own W); conv weights fp16 channel-blocked per tap
 * [tap = ky k + kx][Ci/32][Co][32]; fp32 accumulation on MFMA. Every reduction runs in a fixed order (no
 * floating-point atomics): two runs give the same bits. The LDS opt-in of the conv kernel failing is an error.
 * ------------------------------------------------------------------------------------- */
/* Conv2d(Ci, Co, k, stride, padding = k / 2, bias = False) + eval-mode BatchNorm2d (+ ReLU) (speaker_cloning.py:69-72,
 * 79-80, 84-85): y[ho][wo][co] = act(acc * scale[co] + shift[co]) in fp32, stored fp16; k in {1, 3}, stride in {1, 2},
 * Ci and Co multiples of 32. psum (optional): fp32 [zmi_spk_conv2d_tiles(H, W, k, stride)][Co], the per-tile channel
 * sums of the stored y (SimAM's mean). */
int zmi_spk_conv2d(const void* x, int H, int W, int Ci, const void* w, const float* scale, const float* shift, int Co,
                   int k, int stride, int relu, void* y, float* psum, void* stream);
int zmi_spk_conv2d_tiles(int H, int W, int k, int stride);
/* The stem, Conv2d(1, Co, 3, padding = 1) + BatchNorm2d + ReLU (speaker_cloning.py:170-171, 187): x fp16 [H][W],
 * w fp16 [9][Co], y fp16 [H][W][Co]; a direct kernel (K = 9). */
int zmi_spk_stem(const void* x, int H, int W, const void* w, const float* scale, const float* shift, int Co, void* y,
                 void* stream);
/* SimAMBasicBlock.SimAM and the block tail (speaker_cloning.py:83-96): per channel mean over H W, d = (x - mean)^2,
 * v = sum d / (H W - 1) (two passes), y = relu(x sigmoid(d / (4 (v + 1e-4)) + 0.5) + residual); x, residual, y fp16
 * [H][W][C] (y may be x). psum / n_psum: the producing conv's per-tile sums, or NULL / 0 (one more pass computes
 * them). ws: >= zmi_spk_simam_ws_floats(H, W, C) floats. */
int zmi_spk_simam(const void* x, const void* residual, int H, int W, int C, const float* psum, int n_psum, float* ws,
                  void* y, void* stream);
int64_t zmi_spk_simam_ws_floats(int H, int W, int C);
/* The three trunk entry points over `n` clips of one H and their own widths in one launch (ragged lanes,
 * SpeakerEmbeddingLDA.embed_features_batch). The HOST struct is copied into the kernel arguments: no device table.
 * Lane l's buffer is base + l * ls (ls_* in elements of the buffer's type), laid out [H][w[l]][C] exactly as the single
 * form lays it out; w, scale and shift are shared. The grid's z is the lane and its x is sized for the widest lane; a
 * workgroup past its own lane's tiles / chunks / positions returns at once. A lane's tile index (psum row), padding
 * tests, SimAM chunks and row counts are those of its own width, so every element has the bits the single entry point
 * gives that lane alone, and nothing outside a lane's own extent is written. The single entry points are these with
 * n = 1 (strides ignored). Error (no launch): n < 1 or > ZMI_SPK_MAX_LANES, a w[l] < 1 (SimAM: H w[l] < 2), whatever
 * the single form rejects (its size limit applies to the widest lane), and, when n > 1, a present buffer's stride
 * below the widest lane's extent (H wmax C for activations, zmi_spk_conv2d_tiles(H, wmax, k, stride) Co for psum,
 * max n_psum[l] C for SimAM's psum, zmi_spk_simam_ws_floats(H, wmax, C) for ws) or an fp16 activation stride that is
 * no multiple of 8 (the 16-byte accesses). */
#define ZMI_SPK_MAX_LANES 32
typedef struct ZmiSpkLanes { int n; int w[ZMI_SPK_MAX_LANES]; } ZmiSpkLanes;
int zmi_spk_max_lanes(void);  /* ZMI_SPK_MAX_LANES of this build */
int zmi_spk_conv2d_lanes(const void* x, int H, const ZmiSpkLanes* lanes, int Ci, const void* w, const float* scale,
                         const float* shift, int Co, int k, int stride, int relu, void* y, float* psum, int64_t ls_x,
                         int64_t ls_y, int64_t ls_psum, void* stream);
int zmi_spk_stem_lanes(const void* x, int H, const ZmiSpkLanes* lanes, const void* w, const float* scale,
                       const float* shift, int Co, void* y, int64_t ls_x, int64_t ls_y, void* stream);
/* n_psum: HOST array of n row counts (lane l's psum holds n_psum[l] rows: its own conv's tiles), with psum or NULL.
 * Within a lane's ws the layout is the single form's at the widest lane's chunk count. y may be x (then ls_y = ls_x). */
int zmi_spk_simam_lanes(const void* x, const void* residual, int H, const ZmiSpkLanes* lanes, int C, const float* psum,
                        const int* n_psum, float* ws, void* y, int64_t ls_x, int64_t ls_res, int64_t ls_psum,
                        int64_t ls_ws, int64_t ls_y, void* stream);

/* ---------------------------------------------------------------------------------------
 * Prefix conditioner (Zonos.prepare_conditioning, model.py:204-212 -> PrefixConditioner.forward,
 * conditioning.py:300-310): one output row per conditioning token, then LayerNorm, bf16 out.
 * Each row names a parameter block and how to produce its d values before the LayerNorm.
 * ------------------------------------------------------------------------------------- */
enum {
  ZMI_COND_EMBED = 0,       /* table[index] (phoneme embedding :233, IntegerConditioner :270)      */
  ZMI_COND_VECTOR = 1,      /* table[0..d) (learned uncond_vector, conditioning.py:45-46)          */
  ZMI_COND_FOURIER = 2,     /* [cos f | sin f], f = 2 pi xn @ W^T (FourierConditioner :253-258)     */
  ZMI_COND_LINEAR = 3,      /* x @ W^T + b (PassthroughConditioner + projection "linear" :24-25)   */
  ZMI_COND_PASSTHROUGH = 4  /* x (PassthroughConditioner, projection "none")                      */
};
typedef struct ZmiCondParam {
  const void* table;   /* bf16 [rows][d] (EMBED) or [d] (VECTOR)                                */
  const void* weight;  /* bf16 [d/2][in_dim] (FOURIER) or [d][in_dim] (LINEAR)                  */
  const void* bias;    /* bf16 [d] (LINEAR) or NULL                                             */
  int in_dim;          /* input width (<= 256)                                                  */
  int pad;
  float min_val, max_val; /* FOURIER input normalisation                                         */
} ZmiCondParam;
typedef struct ZmiCondRow {
  int param;  /* index into the parameter array                                                 */
  int kind;   /* ZMI_COND_*                                                                      */
  int index;  /* EMBED row                                                                       */
  int x_off;  /* offset of this row's inputs in x (FOURIER / LINEAR / PASSTHROUGH)               */
} ZmiCondRow;
/* out[r][0..d) = LayerNorm(row r) for r < n_rows; params / rows / x are device arrays. Refused before any launch:
 * d odd, <= 0 or > 4096, a negative n_rows, and with n_rows > 0 a NULL params, rows, x, ln_w, ln_b or out. */
int zmi_prefix_condition(const ZmiCondParam* params, const ZmiCondRow* rows, int n_rows, const float* x, int d,
                         const void* ln_w, const void* ln_b, float eps, void* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Hybrid backbone (Zonos-v0.1-hybrid, zonos/backbone/_mamba_ssm.py:9-57): the blocks mamba-ssm
 * 2.2.4's create_block builds (Mamba2 mixer, MHA at attn_layer_idx, fused add + LayerNorm).
 * mamba-ssm is not in this image: parity unpinned (oracle/hybrid_cpu.py restates it).
 * ------------------------------------------------------------------------------------- */
typedef struct ZmiMamba2Args {
  const void* zxbcdt;   /* bf16 [M][ld_zx] in_proj output: z [d_ssm] | xBC [d_ssm + 2 d_state] | dt [nheads] */
  int ld_zx, M;
  int d_ssm, nheads, headdim, d_state, d_conv, ngroups; /* headdim 64, d_state 128, d_conv 4, ngroups 1 */
  const void* conv_w;   /* bf16 [d_ssm + 2 d_state][d_conv] depthwise conv1d weight                  */
  const void* conv_b;   /* bf16 [d_ssm + 2 d_state]                                                  */
  const float* dt_bias; /* f32 [nheads]                                                              */
  const float* A;       /* f32 [nheads] = -exp(A_log)                                                */
  const float* D;       /* f32 [nheads]                                                              */
  void* conv_ring;      /* bf16 [rows][d_conv][d_ssm + 2 d_state]: raw xBC of position q in slot q % 4 */
  void* ssm;            /* bf16 [rows][nheads][headdim][d_state]                                    */
  void* y;              /* bf16 [M][ldy] out: C.h + D x (before the gated norm)                      */
  int ldy, gz_g;        /* gz_g: 1 = gz receives g = y * gate (for ZMI_PRO_GRMS_G), 0 = the gate     */
  const int* row_pos;   /* [M] position of the row's token (< 0: inactive row; step only)           */
  const int* row_kv;    /* [M] state row of each activation row (NULL: row m)                       */
  float* gz;            /* step only, optional: f32 [M][ldy] the gate z * sigmoid(z) of RMSNormGated */
} ZmiMamba2Args;
/* Decode: causal_conv1d_update + SiLU + selective_state_update(dt_softplus) for one token per row
 * (mamba_ssm/modules/mamba2.py Mamba2.step). */
int zmi_mamba2_step(const ZmiMamba2Args* args, void* stream);
/* Prefill from an empty state: M / seq_len sequences of seq_len rows (causal_conv1d_fn +
 * mamba_chunk_scan_combined of Mamba2.forward), leaving each sequence's final state and conv ring. */
int zmi_mamba2_scan(const ZmiMamba2Args* args, int seq_len, void* stream);
/* The same prefill, parallel forms (the one HybridEngine runs): a conv + SiLU / dt launch into `ws`, then either
 * the state-space-dual matrix form (ZMI_OPT_SCAN_PQ 0, the default, sequences <= 256: y = (C B^T o decay) dt x on
 * MFMA, one workgroup for y and one for the final state per (sequence, head)) or the recurrence on PQ workgroups per
 * (sequence, head), fused multiply-adds (fp32 rounding differs from zmi_mamba2_scan's; all are checked against the
 * oracle). ws: >= zmi_mamba2_scan_ws_bytes(M, d_ssm, nheads). */
int zmi_mamba2_scan_ws(const ZmiMamba2Args* args, int seq_len, void* ws, int64_t ws_bytes, void* stream);
int64_t zmi_mamba2_scan_ws_bytes(int m, int d_ssm, int nheads);
/* zmi_mamba2_scan_ws over ragged sequences, one pass for all of them. Sequence i of the ZmiAttnSeq table owns rows
 * q_row0 .. q_row0 + len - 1 of zxbcdt and y, starts from an empty state (pos0 must be 0) and leaves its final SSM
 * state and conv ring in state row kv_row (args->row_kv is not read). args->M is the row count of the buffers: it
 * bounds the table and sizes ws (>= zmi_mamba2_scan_ws_bytes(M, d_ssm, nheads)). The form is chosen per sequence,
 * as zmi_mamba2_scan_ws would for it alone (ZMI_OPT_SCAN_PQ 0: up to 256 positions the SSD form, longer ones the
 * recurrence on 4 workgroups; a mixed table is two scan launches), the longest sequences dispatched first, and each
 * sequence's y, state and ring are bit for bit those of zmi_mamba2_scan_ws on it alone. Only the listed rows of y and
 * the listed state rows are written; sequences of len 0 are skipped. seqs is the device table, seqs_host its host
 * copy, checked before anything is launched: a negative n_seq, len, q_row0 or kv_row, rows past M, pos0 != 0, two
 * live sequences sharing rows or a kv_row, or a small ws are refused (non-zero, zmi_last_error, nothing written). */
int zmi_mamba2_scan_seqs(const ZmiMamba2Args* args, const ZmiAttnSeq* seqs, int n_seq, const ZmiAttnSeq* seqs_host,
                         void* ws, int64_t ws_bytes, void* stream);
/* zmi_mamba2_scan_seqs for sequences that may continue: the same table and buffers, pos0 >= 0 per sequence.
 * pos0 == 0: the sequence starts empty (stale state and ring are not read); y, state and ring are bit for bit those of
 * zmi_mamba2_scan_seqs. pos0 > 0: it continues from what state row kv_row holds, the bf16 SSM state and the conv ring
 * (slot q & 3 = raw xBC of position q for q in pos0 - 3 .. pos0 - 1; positions below 0 read as zero whatever their slot
 * holds), and leaves the final state in the same row and the ring slots of its last min(len, 4) positions (with
 * len < 4 the other slots keep their bits, as after zmi_mamba2_step). The form is chosen per sequence by len, as in
 * zmi_mamba2_scan_seqs; the continued SSD form adds y_t += exp(cum[t]) (C_t . h0) (one more bf16 MFMA, fp32 sums) and
 * state = exp(cum[T-1]) h0 + W^T B, the recurrence forms start their registers from h0. Each sequence's results are bit
 * for bit those of the call on it alone, whatever its table mates, the table order and the mix of starting and
 * continuing sequences. Launches: conv + dt (reads the rings, writes none), carry (copies the continued states into ws
 * and updates the rings), then the scans (the SSD roles read the copies, never the state row the state role writes).
 * ws: >= zmi_mamba2_scan_cont_ws_bytes(M, d_ssm, nheads, n_cont), n_cont the table's sequences with pos0 > 0 and
 * len > 0 (one state copy each; starting and empty sequences cost none). Refusals: those of zmi_mamba2_scan_seqs with
 * "pos0 < 0" (or pos0 + len past INT_MAX) in place of "pos0 != 0", on the host copy, before any launch. */
int zmi_mamba2_scan_cont(const ZmiMamba2Args* args, const ZmiAttnSeq* seqs, int n_seq, const ZmiAttnSeq* seqs_host,
                         void* ws, int64_t ws_bytes, void* stream);
int64_t zmi_mamba2_scan_cont_ws_bytes(int m, int d_ssm, int nheads, int n_cont);
/* layer_norm_fn(hidden, w, b, residual, prenorm=True): s = hidden + residual (fp32; hidden may be NULL:
 * s = residual), residual <- bf16(s) if store_residual, out = LayerNorm(s) bf16; k in {512 .. 4096}. */
int zmi_add_layernorm(const void* hidden, int ldh, void* residual, int ldr, int m, int k, const void* w,
                      const void* b, float eps, void* out, int ldo, int store_residual, void* stream);
/* RMSNormGated(norm_before_gate=False): out = rmsnorm(y * silu(z)) * w, bf16; k in {512 .. 4096}. */
int zmi_gated_rmsnorm(const void* y, int ldy, const void* z, int ldz, int m, int k, const void* w, float eps,
                      void* out, int ldo, void* stream);
/* Decode: the Mamba2 in_proj GEMV (ADDLN prologue, K = 2048) and zmi_mamba2_step in ONE launch: the step
 * workgroups load their state / conv-ring / conv-weight operands under the in_proj's weight stream and take
 * the in_proj output from {pair, tag = position + 1} granules (`gran`: zmi_mamba_block_gran_words(M,
 * d_in_proj) words, zeroed when a row starts an utterance); 1 <= M <= 16; bit-identical to the two
 * separate launches; *err becomes nonzero if a wait timed out. in_proj->w_fmt may be ZMI_WFMT_FP8 (w_exp set, 8-byte
 * aligned): the bits of the BF16 block on the dequantised weights. */
int zmi_mamba_block(const ZmiGemvArgs* in_proj, const ZmiMamba2Args* step, void* gran, unsigned* err, void* stream);
int64_t zmi_mamba_block_gran_words(int rows, int d_in_proj);
/* zmi_mamba_block plus `prefetch->blocks` prefetch-only workgroups (ZmiPrefetch, as zmi_attn_block_pf) that
 * read the given ranges (the layer's out_proj weights) once during the step phase; same results. */
int zmi_mamba_block_pf(const ZmiGemvArgs* in_proj, const ZmiMamba2Args* step, void* gran, unsigned* err,
                       const ZmiPrefetch* prefetch, void* stream);

/* ---------------------------------------------------------------------------------------
 * Synthetic weights: fill with the counter-based uniform stream of zonos_vibes_amd/synthetic.py
 * dtype 0 = bf16, 1 = f32.
 * ------------------------------------------------------------------------------------- */
int zmi_fill_uniform(void* dst, int64_t n, uint64_t key, float scale, float offset, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * hipGraph helpers: capture whatever the caller enqueues on `stream` between begin/end and
 * replay it. The decode step (~130 launches) is captured once per batch geometry.
 * ------------------------------------------------------------------------------------- */
int zmi_graph_begin(void* stream);
int zmi_graph_end(void* stream, void** graph_exec);
int zmi_graph_launch(void* graph_exec, int times, void* stream);
int zmi_graph_destroy(void* graph_exec);

const char* zmi_last_error(void);
/* ABI version, bumped whenever a weight layout or an option's meaning changes: 4 = channel-blocked DAC conv weights
 * [tap][ci / 32][co][32] (zmi_dac_conv / conv_t / conv_out) and the round-5 ZMI_OPT_GEMM_ROWS bits; 5 =
 * ZMI_OPT_XC_HANDOFF and zmi_xcd_dealing; 6 = ZMI_PRO_GRMS_G and ZmiMamba2Args.gz_g; 7 = the zmi_dac_*_lanes entry points.
 * (zmi_unpack_fp8 and the FP8 forms of the Mamba2 projections were added at version 10: no layout, struct or option
 * changed meaning, and every launch a version-10 caller could make gives what it gave. Likewise zmi_gemv_splitk_f8,
 * zmi_gemv_splitk_f8_ln and ZMI_OPT_FP8_ROWS, added at version 10: FP8 launches over many rows take another form, and
 * give the same bits.) Check it before packing weights (zonos_vibes_amd/_lib.py refuses a library
 * whose version differs). */
int zmi_version(void);
/* 1 if this device deals a launch's workgroups round-robin over its XCDs (blocks b and b + 8 on one XCD, 8
 * distinct XCDs), 0 if not, negative on a launch error (zmi_last_error). Runs a probe launch and waits for it:
 * call it outside graph capture. Hand-offs through an XCD's L2 (ZMI_OPT_XC_HANDOFF 0) rely on this; the engine
 * calls it once per process and sets ZMI_OPT_XC_HANDOFF to 1 otherwise. */
int zmi_xcd_dealing(void* stream);
/* Launch-geometry knobs of the library (process-wide; speed only, no option changes a result):
 *   ZMI_OPT_GEMV_SPREAD (default 1): single-tile GEMV launches reserve enough LDS per workgroup that the
 *   dispatcher spreads their workgroups evenly over the CUs instead of packing several onto one CU.
 *   ZMI_OPT_GEMM_ROWS (default 3): plain K = 2048 GEMVs over many rows run the many-row form (64 columns per
 *   workgroup, activation tiles DMA'd two ahead, one barrier per tile) where it measured faster than the
 *   32-column tile loop; 0 = always the tile loop; bit 1: the dense-pair MFMA forms of the many-row form and of
 *   zmi_gemv_splitk (16 real columns per MFMA instead of 8, same bits; 1 = the M8 forms).
 *   ZMI_OPT_GEMV_SPREAD > 1: at most that many single-tile GEMV workgroups per CU (an occupancy probe).
 *   ZMI_OPT_XC_HANDOFF (default 0): hand-offs between workgroups the grid places on one XCD (blocks 8 apart under
 *          the round-robin dealing zmi_xcd_dealing checks): the chunk-split fused attention block's chunk maxima,
 *          l / M_j and P.V partials inside a (row, kv head) unit, the block-form attention's block maxima and
 *          partials, and zmi_mamba_block's z / x granules for the step workgroups of their head. 0 = workgroup-scope
 *          stores that keep the lines in that XCD's L2, where the consumers' agent-scope polls read them; 1 =
 *          write-through (agent-scope) stores, correct whatever the dealing (set where zmi_xcd_dealing returns 0).
 *          Speed only: either gives the same bits.
 *   Options 3..9: reserved (knobs of the fused / persistent decode forms measured slower and removed in round 6;
 *          their sources are on the git branch diag-forms).
 *   ZMI_OPT_DAC_WIDE (default 1): DAC convs on 256-row time tiles (512-thread workgroups) when the output has at
 *          least ZMI_OPT_DAC_WIDE_MIN (default 256) 256-row x 32-channel units; 0 = always 128-row tiles, 2 = always
 *          256.
 *   ZMI_OPT_ATTNBLK_SPREAD (default 5): zmi_attn_block's workgroups reserve LDS so the launch spreads over the chip;
 *          bits 0-1 for the 8-chunk split / score-exchange / self forms, bits 2-3 for the 24-chunk split form:
 *          0 = no reserve, 1 = one workgroup per CU, 2 = at most two.
 *   ZMI_OPT_DAC_STAGE (default 29): DAC convs on the staged K loop (one barrier per 32-channel step x all taps, one
 *          512-thread workgroup per CU); bit 0 the k7 convs, bit 1 the 1x1 convs, bit 2 the transposed convs,
 *          bit 3 512-row time tiles for the k7 convs where their grid is large enough (256 otherwise), bit 4 the
 *          256-row forms with 4 dedicated loader waves (768 threads).
 *   ZMI_OPT_DAC_STAGE_MIN (default 128): the staged form only where its grid has at least this many workgroups.
 *   ZMI_OPT_SCAN_PQ (default 0): zmi_mamba2_scan_ws's form: 0 = the quadratic (SSD) form for sequences of up to
 *          256 positions (MFMA tiles of C B^T, the decay matrix and the state sum; longer sequences take PQ 4), else
 *          the recurrence on PQ workgroups per (sequence, head) (1, 2 or 4; each thread then owns 4 / PQ head dims x
 *          8 state columns).
 *   ZMI_OPT_SPLITK_WGS (default 256): zmi_gemv_splitk splits the rows into groups of 16-row tiles until its grid
 *          has about this many workgroups (each row group re-reads its segment's weights); 0 = one row group.
 *   ZMI_OPT_SPLITK_STAGE (default 1): zmi_gemv_splitk stages 2 (K segment 1024) or 4 (512) 16-row tiles per LDS
 *          buffer, so twice the activation bytes are in flight per CU (~132 KB of LDS); 0 = one tile per buffer.
 *          (ZMI_OPT_GEMM_ROWS bit 1, ZMI_OPT_SPLITK_WGS and ZMI_OPT_SPLITK_STAGE shape zmi_gemv_splitk_f8 alike.)
 *   ZMI_OPT_FP8_ROWS (default 1): zmi_gemv_launch over FP8 weights takes the many-row form wherever the same launch
 *          over bf16 weights does (ZMI_OPT_GEMM_ROWS picks M8 or dense pairs); 0 = gemv_body's tile loop for every M. */
enum { ZMI_OPT_GEMV_SPREAD = 0, ZMI_OPT_GEMM_ROWS = 1, ZMI_OPT_XC_HANDOFF = 2, /* 3..9 reserved */
       ZMI_OPT_DAC_WIDE = 10, ZMI_OPT_DAC_WIDE_MIN = 11, ZMI_OPT_ATTNBLK_SPREAD = 12, ZMI_OPT_DAC_STAGE = 13,
       ZMI_OPT_DAC_STAGE_MIN = 14, ZMI_OPT_SCAN_PQ = 15, ZMI_OPT_SPLITK_WGS = 16, ZMI_OPT_SPLITK_STAGE = 17,
       ZMI_OPT_FP8_ROWS = 18, ZMI_OPT_COUNT = 19 };
int zmi_set_option(int which, int value);
int zmi_get_option(int which);

#ifdef __cplusplus
}
#endif
#endif /* ZONOS_HIP_H */
