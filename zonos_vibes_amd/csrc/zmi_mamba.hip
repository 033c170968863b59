// Mamba2 kernels of the hybrid backbone (Zonos-v0.1-hybrid, BASELINE config C4), gfx950: step, scans, SSD.
//
// Reference: zonos/backbone/_mamba_ssm.py:9-57 builds its layers with mamba-ssm 2.2.4's
// `create_block` (absent from this image, so parity is unpinned; oracle/hybrid_cpu.py restates the
// published algorithm). A decode step of one Mamba2 block is
//
//   hidden, residual = layer_norm_fn(hidden, norm.w, norm.b, residual, prenorm=True)  (Block.forward; zmi_rownorm.hip)
//   zxbcdt = in_proj(hidden)                                                            (GEMV kernel)
//   xBC    = silu(causal_conv1d_update(xBC, conv_state, conv1d.w, conv1d.b))            (mamba2_step)
//   y      = selective_state_update(ssm_state, x, dt, A, B, C, D, dt_bias, softplus)    (mamba2_step)
//   y      = RMSNormGated(y, z)                                                         (zmi_rownorm.hip)
//   out    = out_proj(y)                                                                (GEMV kernel)
//
// and the prefill is the same block over a whole sequence (causal_conv1d_fn + mamba_chunk_scan_combined;
// mamba2_scan here: the recurrence in fp32 registers, one workgroup per (sequence, head)).
//
// State layouts (this library's, not the reference's roll buffer):
//   conv ring  bf16 [row][4][conv_dim]: the raw xBC input of position q sits in slot q & 3. A step at
//              position p reads slots of p-3 .. p-1 and writes slot p & 3 (that of p-4, which nobody
//              reads), so the workgroups of one row never race; negative positions read as zero.
//   ssm state  bf16 [row][nheads][headdim 64][d_state 128] (the reference keeps it in the cache dtype).
#include <algorithm>
#include <climits>
#include <utility>
#include <vector>

#include "zmi_common.h"
#include "zmi_kernels.h"
#include "zmi_mamba_step.h"

namespace {

using namespace zmi_mamba;

__global__ __launch_bounds__(MB_ST) void mamba2_step_kernel(const ZmiMamba2Args a) {
  const int m = blockIdx.x / a.nheads, h = blockIdx.x - m * a.nheads;
  const int pos = a.row_pos[m];
  if (pos < 0) return;
  const int kv = a.row_kv ? a.row_kv[m] : m;
  __shared__ float xs[MB_HD], bc[2 * MB_DS];
  __shared__ bf16_t raw[RAW_N];
  StepPre<MB_ST> pre;
  step_prefetch<MB_ST>(a, h, pos, kv, pre);  // the state slice first: the longest loads, under the rest
  const bf16_t* zx = reinterpret_cast<const bf16_t*>(a.zxbcdt) + (size_t)m * a.ld_zx;
  for (int i = threadIdx.x; i < RAW_DT + 1; i += MB_ST) {
    const int col = i < RAW_Z ? a.d_ssm + conv_channel(i, h, a.d_ssm)
                              : (i < RAW_DT ? h * MB_HD + (i - RAW_Z) : 2 * a.d_ssm + 2 * MB_DS + h);
    raw[i] = zx[col];
  }
  __syncthreads();
  step_core<MB_ST>(a, m, h, pos, kv, raw, pre, xs, bc);
}

// ---------------------------------------------------------------------------- prefill scan
constexpr int SC_TT = 32;  // positions staged per tile

__global__ __launch_bounds__(MB_NT) void mamba2_scan_kernel(const ZmiMamba2Args a, int seq_len) {
  const int sq = blockIdx.x / a.nheads, h = blockIdx.x - sq * a.nheads;
  const int row0 = sq * seq_len;
  const int kv = a.row_kv ? a.row_kv[row0] : sq;
  const int conv_dim = a.d_ssm + 2 * MB_DS;
  const bf16_t* zx0 = reinterpret_cast<const bf16_t*>(a.zxbcdt) + (size_t)row0 * a.ld_zx;
  const bf16_t* cw = reinterpret_cast<const bf16_t*>(a.conv_w);
  const bf16_t* cb = reinterpret_cast<const bf16_t*>(a.conv_b);
  __shared__ float xs[SC_TT][MB_HD], bs[SC_TT][MB_DS], cs[SC_TT][MB_DS], dts[SC_TT], das[SC_TT];
  const int t = threadIdx.x, p = t >> 2, nq = t & 3;
  const float Ah = a.A[h], Dh = a.D[h], dtb = a.dt_bias[h];
  auto raw = [&](int q, int c) { return q >= 0 ? bf2f(zx0[(size_t)q * a.ld_zx + a.d_ssm + c]) : 0.f; };

  float s[32];
#pragma unroll
  for (int j = 0; j < 32; ++j) s[j] = 0.f;
  for (int t0 = 0; t0 < seq_len; t0 += SC_TT) {
    const int nt = min(SC_TT, seq_len - t0);
    __syncthreads();  // the previous tile's readers are done
    for (int idx = t; idx < nt * MB_NCH; idx += MB_NT) {
      const int tt = idx / MB_NCH, i = idx - tt * MB_NCH, q = t0 + tt;
      const int c = conv_channel(i, h, a.d_ssm);
      const float o = bfround(conv4(cw + (size_t)c * MB_DC, bf2f(cb[c]), raw(q - 3, c), raw(q - 2, c), raw(q - 1, c),
                                    raw(q, c)));
      if (i < MB_HD) xs[tt][i] = o;
      else if (i < MB_HD + MB_DS) bs[tt][i - MB_HD] = o;
      else cs[tt][i - MB_HD - MB_DS] = o;
    }
    if (t < nt) {
      const float dtv = softplus_f(bf2f(zx0[(size_t)(t0 + t) * a.ld_zx + 2 * a.d_ssm + 2 * MB_DS + h]) + dtb);
      dts[t] = dtv;
      das[t] = expf(Ah * dtv);
    }
    __syncthreads();
    for (int tt = 0; tt < nt; ++tt) {
      const float x = xs[tt][p], dtv = dts[tt], dA = das[tt];
      const float4* B4 = reinterpret_cast<const float4*>(&bs[tt][nq * 32]);
      const float4* C4 = reinterpret_cast<const float4*>(&cs[tt][nq * 32]);
      float out = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float4 b = B4[j], c = C4[j];
        s[4 * j + 0] = s[4 * j + 0] * dA + (b.x * dtv) * x;
        s[4 * j + 1] = s[4 * j + 1] * dA + (b.y * dtv) * x;
        s[4 * j + 2] = s[4 * j + 2] * dA + (b.z * dtv) * x;
        s[4 * j + 3] = s[4 * j + 3] * dA + (b.w * dtv) * x;
        out += s[4 * j + 0] * c.x;
        out += s[4 * j + 1] * c.y;
        out += s[4 * j + 2] * c.z;
        out += s[4 * j + 3] * c.w;
      }
      out = quad_sum(out);
      if (nq == 0)
        reinterpret_cast<bf16_t*>(a.y)[(size_t)(row0 + t0 + tt) * a.ldy + h * MB_HD + p] = (bf16_t)f2bf(out + x * Dh);
    }
  }
  // final state (bf16, the cache dtype) and the ring slots of the last four positions (zero below 0)
  bf16_t* st = reinterpret_cast<bf16_t*>(a.ssm) + (((size_t)kv * a.nheads + h) * MB_HD + p) * MB_DS + nq * 32;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = f2bf(s[8 * j + 2 * e]) | (f2bf(s[8 * j + 2 * e + 1]) << 16);
    reinterpret_cast<uint4*>(st)[j] = uint4{w[0], w[1], w[2], w[3]};
  }
  bf16_t* ring = reinterpret_cast<bf16_t*>(a.conv_ring) + (size_t)kv * MB_DC * conv_dim;
  for (int idx = t; idx < MB_DC * MB_NCH; idx += MB_NT) {
    const int k = idx / MB_NCH, i = idx - k * MB_NCH;
    if (i >= MB_HD && h != 0) continue;
    const int q = seq_len - MB_DC + k, c = conv_channel(i, h, a.d_ssm);
    ring[(size_t)(q & 3) * conv_dim + c] = q >= 0 ? zx0[(size_t)q * a.ld_zx + a.d_ssm + c] : (bf16_t)0;
  }
}

// ---------------------------------------------------------------------------- parallel prefill scan
// zmi_mamba2_scan_ws (sequences of one length) and zmi_mamba2_scan_seqs (ragged sequences from a ZmiAttnSeq table, a
// form per sequence: up to three launches): the same Mamba2.forward from an empty state in two launches.
//  (1) mamba2_conv_kernel, one workgroup per row: causal conv + SiLU of every xBC channel (conv4, bf16-rounded as
//      the reference's conv output tensor) into the workspace, dt = softplus(dt + dt_bias) and dA = exp(A dt) per
//      head, and, on each sequence's last row, the conv ring's four slots (the last raw inputs, zero below 0).
//  (2) mamba2_scan2_kernel, one workgroup per (sequence, head, quarter of the 64 head dims): thread (p, n-block)
//      owns state[p][8 n-block .. + 7] in fp32 registers and walks the positions in order,
//          s = fma(s, dA, (B dt) x),   y_p = sum_n fma(s, C) (+ x D),
//      the 16 n-blocks of a row summed by DPP (each block's 8 terms as two interleaved chains). The (sequence, head) recurrence the single-workgroup kernel runs on
//      256 threads is spread over 1,024 (4x the workgroups, a quarter of each thread's state and FMA chain), and
//      the conv no longer sits inside it. Its arithmetic differs from mamba2_scan_kernel's in fp32 rounding (fused
//      multiply-adds, the readout summed over 8-wide blocks): both are checked against the oracle's recurrence.
// zmi_mamba2_scan_cont (the kernels' CONT instantiations): the same launches for sequences that continue from the state
// row's bf16 state and conv ring (pos0 > 0 in the table), with mamba2_carry_kernel between (1) and the scans. Three
// hazards of a continued scan are excluded by construction, each stated at its kernel: (ring) the conv launch only
// reads rings and the carry launch, next in stream order, only writes them; (state) the SSD roles read h0 from the
// carry launch's copy in the workspace, never from the state row the state role overwrites, and a recurrence workgroup
// reads exactly the state rows it alone writes; (LDS) the y role's h0 fragments live in registers, and its C_blk h0^T
// product is taken between a row block's two barriers, while the C rows in LDS are stable (step (4), which runs while
// faster waves already refill them, reads none). The plain
// instantiations (CONT false: zmi_mamba2_scan_ws, zmi_mamba2_scan_seqs) compile to what they were.
constexpr int S2_NB = MB_DS / 8;        // 16 n-blocks of 8 state columns
constexpr int S2_TT = 32;               // positions staged per tile

// Which rows form which sequence, for the three prefill kernels. Uniform (seqs null, zmi_mamba2_scan_ws): sequence k
// is rows k seq_len .. + seq_len - 1, its state row row_kv[first row] (or k). Ragged (zmi_mamba2_scan_seqs): the
// ZmiAttnSeq table; a scan launch covers the sequences of its form, lo < len <= hi, longest first (ties in table
// order), so the long ones start while the chip is empty. The host has checked the table (rows inside M, no overlap).
struct ScanSeqs {
  const ZmiAttnSeq* seqs;
  int n_seq, seq_len, lo, hi;
};
struct ScanSeq {
  int row0, T, idx;  // T == 0: no sequence
};

__device__ __forceinline__ bool scan_rows_ok(const ZmiAttnSeq& s, int m) {
  return s.len > 0 && s.q_row0 >= 0 && s.q_row0 <= m - s.len;
}

// the k-th sequence of a scan launch; sh: one LDS word (ragged: every thread of the workgroup must call)
__device__ __forceinline__ ScanSeq scan_seq_at(const ZmiMamba2Args& a, const ScanSeqs& q, int k, int* sh) {
  if (!q.seqs) return ScanSeq{k * q.seq_len, q.seq_len, k};
  if (threadIdx.x == 0) *sh = -1;
  __syncthreads();
  for (int i = threadIdx.x; i < q.n_seq; i += blockDim.x) {
    const int len = q.seqs[i].len;
    if (len <= q.lo || len > q.hi) continue;
    int rank = 0;  // sequences of this form ahead of i
    for (int j = 0; j < q.n_seq; ++j) {
      const int lj = q.seqs[j].len;
      rank += (lj > q.lo && lj <= q.hi && (lj > len || (lj == len && j < i))) ? 1 : 0;
    }
    if (rank == k) *sh = i;
  }
  __syncthreads();
  const int i = *sh;
  if (i < 0 || !scan_rows_ok(q.seqs[i], a.M)) return ScanSeq{0, 0, -1};
  return ScanSeq{q.seqs[i].q_row0, q.seqs[i].len, i};
}

// the sequence that holds `row` (ragged: every thread of the workgroup must call; none: T == 0)
__device__ __forceinline__ ScanSeq scan_seq_of_row(const ZmiMamba2Args& a, const ScanSeqs& q, int row, int* sh) {
  if (!q.seqs) return ScanSeq{row / q.seq_len * q.seq_len, q.seq_len, row / q.seq_len};
  if (threadIdx.x == 0) *sh = -1;
  __syncthreads();
  for (int i = threadIdx.x; i < q.n_seq; i += blockDim.x) {
    const ZmiAttnSeq s = q.seqs[i];
    if (scan_rows_ok(s, a.M) && row >= s.q_row0 && row - s.q_row0 < s.len) *sh = i;
  }
  __syncthreads();
  const int i = *sh;
  if (i < 0) return ScanSeq{0, 0, -1};
  return ScanSeq{q.seqs[i].q_row0, q.seqs[i].len, i};
}

// the state row (conv ring, SSM state) a sequence leaves its final state in
__device__ __forceinline__ int scan_kv(const ZmiMamba2Args& a, const ScanSeqs& q, const ScanSeq& s) {
  if (q.seqs) return q.seqs[s.idx].kv_row;
  return a.row_kv ? a.row_kv[s.row0] : s.idx;
}

// CONT (zmi_mamba2_scan_cont): a sequence with pos0 > 0 takes the raw inputs of positions pos0 - 3 .. pos0 - 1 from the
// conv ring of its state row (slot q & 3, zero below position 0), and NO workgroup of this launch writes a ring: the
// rows 0 .. 2 of a sequence read the ring its last row would overwrite, with no order between them. The ring is
// updated by mamba2_carry_kernel, the next launch in stream order.
template <bool CONT>
__global__ __launch_bounds__(256) void mamba2_conv_kernel(const ZmiMamba2Args a, const ScanSeqs sqs, bf16_t* xc,
                                                          float* dts, float* das) {
  // one thread per (row, channel): grid (rows, channel blocks of 256), every load of the launch in flight at once
  __shared__ int seq_sh;
  const int row = blockIdx.x;
  const ScanSeq sq = scan_seq_of_row(a, sqs, row, &seq_sh);
  if (sq.T == 0) return;  // a row of no sequence: nothing read, nothing written
  const int seq_len = sq.T, row0 = sq.row0, q = row - row0;
  const int conv_dim = a.d_ssm + 2 * MB_DS, c = blockIdx.y * 256 + threadIdx.x;
  const bf16_t* zx0 = reinterpret_cast<const bf16_t*>(a.zxbcdt) + (size_t)row0 * a.ld_zx + a.d_ssm;
  if (c < conv_dim) {
    const bf16_t* cw = reinterpret_cast<const bf16_t*>(a.conv_w);
    const bf16_t* cb = reinterpret_cast<const bf16_t*>(a.conv_b);
    float r[MB_DC];
    int pos0 = 0;
    const bf16_t* ring0 = nullptr;  // CONT: the ring the sequence continues from (read only)
    if constexpr (CONT) {
      pos0 = sqs.seqs[sq.idx].pos0;
      ring0 = reinterpret_cast<const bf16_t*>(a.conv_ring) + (size_t)sqs.seqs[sq.idx].kv_row * MB_DC * conv_dim;
    }
#pragma unroll
    for (int k = 0; k < MB_DC; ++k) {
      const int qq = q - (MB_DC - 1) + k;
      if (qq >= 0) r[k] = bf2f(zx0[(size_t)qq * a.ld_zx + c]);
      else if (CONT && pos0 + qq >= 0) r[k] = bf2f(ring0[(size_t)((pos0 + qq) & 3) * conv_dim + c]);
      else r[k] = 0.f;
    }
    xc[(size_t)row * conv_dim + c] = (bf16_t)f2bf(conv4(cw + (size_t)c * MB_DC, bf2f(cb[c]), r[0], r[1], r[2], r[3]));
    if (!CONT && q == seq_len - 1) {  // the conv ring: slot qq % 4 holds the raw input of qq, for the last d_conv positions
      const int kv = scan_kv(a, sqs, sq);
      bf16_t* ring = reinterpret_cast<bf16_t*>(a.conv_ring) + (size_t)kv * MB_DC * conv_dim;
#pragma unroll
      for (int k = 0; k < MB_DC; ++k) {
        const int qq = seq_len - MB_DC + k;
        ring[(size_t)(qq & 3) * conv_dim + c] = qq >= 0 ? zx0[(size_t)qq * a.ld_zx + c] : (bf16_t)0;
      }
    }
  }
  if (blockIdx.y == 0)
    for (int h = threadIdx.x; h < a.nheads; h += 256) {
      const float dtv = softplus_f(bf2f(zx0[(size_t)q * a.ld_zx + a.d_ssm + 2 * MB_DS + h]) + a.dt_bias[h]);
      dts[(size_t)row * a.nheads + h] = dtv;
      das[(size_t)row * a.nheads + h] = expf(a.A[h] * dtv);
    }
}

// where the h0 copy of table entry idx sits in the workspace: its rank among the continuing sequences (pos0 > 0, live
// rows), so starting and empty entries cost no copy
__device__ __forceinline__ int cont_rank(const ZmiMamba2Args& a, const ScanSeqs& q, int idx) {
  int r = 0;
  for (int j = 0; j < idx; ++j) r += (q.seqs[j].pos0 > 0 && scan_rows_ok(q.seqs[j], a.M)) ? 1 : 0;
  return r;
}

// zmi_mamba2_scan_cont's second launch, after the conv launch and before the scans, one workgroup per (table entry,
// head | ring): what a continuing sequence carries, taken out of the other launches' way by stream order alone.
//   blockIdx.y < nheads   a sequence with pos0 > 0: its head's bf16 state h0 copied to the workspace (h0s, by
//                         cont_rank). The SSD form's y workgroup reads h0 while its state workgroup overwrites the state
//                         row, with no order between the two: both read the copy, never the row.
//   blockIdx.y == nheads  the conv ring: slot (pos0 + q) & 3 <- raw input of the sequence's last min(len, 4) positions
//                         (the conv launch, the ring's only reader, is complete). pos0 == 0: the slots of positions
//                         below 0 are zeroed, as zmi_mamba2_scan_seqs leaves them; pos0 > 0: the other slots keep
//                         their bits, as after zmi_mamba2_step.
__global__ __launch_bounds__(256) void mamba2_carry_kernel(const ZmiMamba2Args a, const ScanSeqs sqs, bf16_t* h0s) {
  const ZmiAttnSeq s = sqs.seqs[blockIdx.x];
  if (!scan_rows_ok(s, a.M)) return;
  const int conv_dim = a.d_ssm + 2 * MB_DS;
  if ((int)blockIdx.y == a.nheads) {
    const bf16_t* zx0 = reinterpret_cast<const bf16_t*>(a.zxbcdt) + (size_t)s.q_row0 * a.ld_zx + a.d_ssm;
    bf16_t* ring = reinterpret_cast<bf16_t*>(a.conv_ring) + (size_t)s.kv_row * MB_DC * conv_dim;
    for (int c = threadIdx.x; c < conv_dim; c += 256) {
#pragma unroll
      for (int k = 0; k < MB_DC; ++k) {
        const int qq = s.len - MB_DC + k;
        if (qq >= 0) ring[(size_t)((s.pos0 + qq) & 3) * conv_dim + c] = zx0[(size_t)qq * a.ld_zx + c];
        else if (s.pos0 == 0) ring[(size_t)(qq & 3) * conv_dim + c] = (bf16_t)0;
      }
    }
    return;
  }
  if (s.pos0 <= 0) return;
  constexpr int HV = MB_HD * MB_DS / 8;  // uint4 of one head's state
  const size_t h = blockIdx.y;
  const uint4* src = reinterpret_cast<const uint4*>(a.ssm) + ((size_t)s.kv_row * a.nheads + h) * HV;
  uint4* dst = reinterpret_cast<uint4*>(h0s) + ((size_t)cont_rank(a, sqs, blockIdx.x) * a.nheads + h) * HV;
  for (int i = threadIdx.x; i < HV; i += 256) dst[i] = src[i];
}

// PQ workgroups per (sequence, head), each 64 / PQ head dims; thread (p-group, n-block) owns PR = 4 / PQ rows p
// x 8 state columns, so each B / C value it reads from LDS serves PR rows
#ifdef ZMI_SCAN_STAMPS
// diagnostic builds only (tools/scan_probe.py --stamps): thread 0 of each workgroup stores s_memtime at the start,
// and per tile k < 12 after its operands are in LDS [1 + 2k] and after its positions [2 + 2k]
__device__ unsigned long long g_scan_stamps[1024][32];
extern "C" int zmi_scan_stamps_read(void* dst, size_t bytes) {
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_scan_stamps), bytes) == hipSuccess ? 0 : -1;
}
#define ZMI_SSTAMP(i_)                                                                      \
  do {                                                                                      \
    if (threadIdx.x == 0 && blockIdx.x < 1024) g_scan_stamps[blockIdx.x][i_] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define ZMI_SSTAMP(i_) \
  do {                 \
  } while (0)
#endif

// CONT: a sequence with pos0 > 0 starts its registers from the bf16 state of its state row instead of 0. A workgroup
// reads exactly the state rows it alone writes at the end, so the recurrence forms need no copy of h0.
template <int PQ, bool CONT>
__global__ __launch_bounds__(256) void mamba2_scan2_kernel(const ZmiMamba2Args a, const ScanSeqs sqs, const bf16_t* xc,
                                                           const float* dts, const float* das) {
  constexpr int PW = MB_HD / PQ, PR = PW / 16;  // head dims per workgroup, rows per thread
  __shared__ int seq_sh;
  const int pq = blockIdx.x % PQ, sh = blockIdx.x / PQ, h = sh % a.nheads;
  const ScanSeq sq = scan_seq_at(a, sqs, sh / a.nheads, &seq_sh);
  if (sq.T == 0) return;
  const int seq_len = sq.T, row0 = sq.row0, conv_dim = a.d_ssm + 2 * MB_DS;
  const int kv = scan_kv(a, sqs, sq);
  const int t = threadIdx.x, pg = t / S2_NB, nb = t % S2_NB, p0 = pq * PW + pg * PR;
  __shared__ float xs[S2_TT][PW], bdt[S2_TT][MB_DS], cs[S2_TT][MB_DS], dA[S2_TT];
  const float Dh = a.D[h];
  // a tile's operands, one thread's share: (B dt, C) of (position tt = (t + 256 i) / 128, state column
  // (t + 256 i) % 128) for i < 16, x of (t + 256 i) / PW, % PW, dA of position t; loaded into registers one
  // tile ahead so their latency hides under the previous tile's recurrence
  constexpr int NBC = S2_TT * MB_DS / 256, NX = S2_TT * PW / 256;
  float rb[NBC], rc[NBC], rx[NX], rd = 0.f;
  auto load = [&](int t0) {
    const int nt = min(S2_TT, seq_len - t0);
#pragma unroll
    for (int i = 0; i < NBC; ++i) {
      const int idx = t + 256 * i, tt = idx / MB_DS, n = idx - tt * MB_DS;
      if (tt < nt) {
        const size_t r = (size_t)(row0 + t0 + tt);
        rb[i] = bf2f(xc[r * conv_dim + a.d_ssm + n]) * dts[r * a.nheads + h];
        rc[i] = bf2f(xc[r * conv_dim + a.d_ssm + MB_DS + n]);
      }
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int idx = t + 256 * i, tt = idx / PW, j = idx - tt * PW;
      if (tt < nt) rx[i] = bf2f(xc[(size_t)(row0 + t0 + tt) * conv_dim + h * MB_HD + pq * PW + j]);
    }
    if (t < nt) rd = das[(size_t)(row0 + t0 + t) * a.nheads + h];
  };
  float st[PR][8];
#pragma unroll
  for (int r = 0; r < PR; ++r)
#pragma unroll
    for (int k = 0; k < 8; ++k) st[r][k] = 0.f;
  if constexpr (CONT) {
    if (sqs.seqs[sq.idx].pos0 > 0) {
#pragma unroll
      for (int r = 0; r < PR; ++r) {
        const uint4 v = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(a.ssm) +
                                                        (((size_t)kv * a.nheads + h) * MB_HD + p0 + r) * MB_DS + nb * 8);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) st[r][2 * e] = bf2f(w[e]), st[r][2 * e + 1] = bf2f(w[e] >> 16);
      }
    }
  }
  bf16_t* y = reinterpret_cast<bf16_t*>(a.y);
  ZMI_SSTAMP(0);
  load(0);
  for (int t0 = 0; t0 < seq_len; t0 += S2_TT) {
    const int nt = min(S2_TT, seq_len - t0);
    __syncthreads();  // the previous tile's readers are done
#pragma unroll
    for (int i = 0; i < NBC; ++i) {
      const int idx = t + 256 * i, tt = idx / MB_DS, n = idx - tt * MB_DS;
      bdt[tt][n] = rb[i];
      cs[tt][n] = rc[i];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int idx = t + 256 * i;
      xs[idx / PW][idx % PW] = rx[i];
    }
    if (t < S2_TT) dA[t] = rd;
    __syncthreads();
    if (t0 / S2_TT < 12) ZMI_SSTAMP(1 + 2 * (t0 / S2_TT));
    if (t0 + S2_TT < seq_len) load(t0 + S2_TT);
    // positions in groups of 4 with their stores behind one branch at the end: a position's readout (FMA
    // chains, DPP sums) is off the state's critical path, so the next positions' LDS reads and state updates
    // issue under it
    auto step = [&](int tt, float (&v)[PR]) {
      const float d = dA[tt];
      const float4 b0 = *reinterpret_cast<const float4*>(&bdt[tt][nb * 8]);
      const float4 b1 = *reinterpret_cast<const float4*>(&bdt[tt][nb * 8 + 4]);
      const float4 c0 = *reinterpret_cast<const float4*>(&cs[tt][nb * 8]);
      const float4 c1 = *reinterpret_cast<const float4*>(&cs[tt][nb * 8 + 4]);
      const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
      const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
      for (int r = 0; r < PR; ++r) {
        const float x = xs[tt][pg * PR + r];
        float o0 = 0.f, o1 = 0.f;
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
          st[r][k] = fmaf(st[r][k], d, b[k] * x);
          st[r][k + 1] = fmaf(st[r][k + 1], d, b[k + 1] * x);
          o0 = fmaf(st[r][k], c[k], o0);
          o1 = fmaf(st[r][k + 1], c[k + 1], o1);
        }
        v[r] = row16_sum(o0 + o1) + x * Dh;  // the 16 n-blocks of row p: 16 consecutive lanes
      }
    };
    bf16_t* yp = y + (size_t)(row0 + t0) * a.ldy + h * MB_HD + p0;
    int tt = 0;
    for (; tt + 4 <= nt; tt += 4) {
      float v[4][PR];
      step(tt, v[0]);
      step(tt + 1, v[1]);
      step(tt + 2, v[2]);
      step(tt + 3, v[3]);
      if (nb == 0)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int r = 0; r < PR; ++r) yp[(size_t)(tt + u) * a.ldy + r] = (bf16_t)f2bf(v[u][r]);
    }
    for (; tt < nt; ++tt) {
      float v[PR];
      step(tt, v);
      if (nb == 0)
#pragma unroll
        for (int r = 0; r < PR; ++r) yp[(size_t)tt * a.ldy + r] = (bf16_t)f2bf(v[r]);
    }
    if (t0 / S2_TT < 12) ZMI_SSTAMP(2 + 2 * (t0 / S2_TT));
  }
  // final state, bf16 (the cache dtype): 8 consecutive n per row
#pragma unroll
  for (int r = 0; r < PR; ++r) {
    bf16_t* sp = reinterpret_cast<bf16_t*>(a.ssm) + (((size_t)kv * a.nheads + h) * MB_HD + p0 + r) * MB_DS + nb * 8;
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = f2bf(st[r][2 * e]) | (f2bf(st[r][2 * e + 1]) << 16);
    *reinterpret_cast<uint4*>(sp) = uint4{w[0], w[1], w[2], w[3]};
  }
}

// ---------------------------------------------------------------------------- quadratic (SSD) prefill
// zmi_mamba2_scan_ws with ZMI_OPT_SCAN_PQ = 0, sequences of at most SSD_TMAX positions: the state-space dual of the
// recurrence (the matrix form mamba_chunk_scan_combined evaluates within a chunk; here the whole sequence is one chunk).
// With cum[t] = sum_{tau <= t} A dt_tau (the log of the decays' product),
//     y_t = sum_{s <= t} (C_t . B_s) exp(cum[t] - cum[s]) dt_s x_s + D x_t,
//     state = sum_s exp(cum[T-1] - cum[s]) dt_s x_s B_s^T   (the recurrence's final state),
// as MFMA tiles instead of T dependent steps. Two 1024-thread workgroups per (sequence, head): one writes y, 32 rows at
// a time (the next block's C rows loaded under the current block's tiles), the other the final state.
//   G = C_blk B^T          bf16 MFMA (B, C are the conv output, exactly bf16), fp32 sums;
//   M = G exp(cum_t - cum_s) dt_s (s <= t, else 0), fp32, then split M = hi + lo into two bf16 terms;
//   y = M_hi X + M_lo X    bf16 MFMA (x exactly bf16), fp32 sums, + D x, rounded to bf16;
//   state = W^T B with W[s][p] = exp(cum[T-1] - cum[s]) dt_s x_s[p] split the same way, rounded to bf16 (the cache dtype).
// cum is a fixed-shape scan (lane L owns positions 4L .. 4L + 3, lane totals by a shuffle scan) computed identically by
// every role, in fp64, and cum[t] - cum[s] is taken in fp64 before expf: one fp32 running sum over the sequence carries
// an absolute error of ~ |cum| 2^-23 into every exponent, however small the difference (a head that forgets, A dt ~
// -480 for a few positions, leaves |cum| in the thousands and every later decay wrong by 2^-11; tests/mamba_cases.py,
// regime reset). Arithmetic differs from the recurrence in fp32 rounding (and the hi / lo split keeps ~16 mantissa
// bits of M and W): checked against the fp64 recurrence like the scan forms (tests/test_gpu_mamba_probe.py).
constexpr int SSD_TB = 32;      // y rows per block of the y workgroup
constexpr int SSD_NT = 1024;    // threads: 16 waves
constexpr int SSD_TMAX = 256;   // longest sequence of this form
constexpr int SSD_BROW = MB_DS + 8;  // B / C row stride (bf16): 272 B, MFMA fragment reads spread over the banks
constexpr int SSD_XROW = MB_HD + 8;  // x / W row stride (bf16)

// Every operand stays row-major in LDS (position-major, as the workspace holds it: coalesced 16-byte copies, no
// transposing stores); an MFMA operand whose k runs over positions is gathered as 8 bf16 of one column (8 ds_read_u16).
struct SsdLds {
  int S32;  // positions rounded up to 32
  __device__ __host__ SsdLds(int T) : S32((T + 31) / 32 * 32) {}
  // y role: cum (fp64), dt | B rows [S32][SSD_BROW] | C rows [32][SSD_BROW] | M hi / lo [32][S32 + 8] | x rows
  // [S32][SSD_XROW]: 152,064 bytes at T = 256
  __device__ __host__ int MP() const { return S32 + 8; }
  __device__ __host__ size_t b_off() const { return SSD_TMAX * 8 + SSD_TMAX * 4; }
  __device__ __host__ size_t c_off() const { return b_off() + (size_t)S32 * SSD_BROW * 2; }
  __device__ __host__ size_t mh_off() const { return c_off() + (size_t)SSD_TB * SSD_BROW * 2; }
  __device__ __host__ size_t ml_off() const { return mh_off() + (size_t)SSD_TB * MP() * 2; }
  __device__ __host__ size_t x_off() const { return ml_off() + (size_t)SSD_TB * MP() * 2; }
  __device__ __host__ size_t y_bytes() const { return x_off() + (size_t)S32 * SSD_XROW * 2; }
  // state role: cum, dt | B rows [S32][SSD_BROW] | W hi / lo rows [S32][SSD_XROW]
  __device__ __host__ size_t wh_off() const { return b_off() + (size_t)S32 * SSD_BROW * 2; }
  __device__ __host__ size_t wl_off() const { return wh_off() + (size_t)S32 * SSD_XROW * 2; }
  __device__ __host__ size_t s_bytes() const { return wl_off() + (size_t)S32 * SSD_XROW * 2; }
};

__device__ __forceinline__ f32x4_t mfma_bf16(const uint4& a, const uint4& b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0,
                                                 0, 0);
}

// 8 bf16 of one column, rows r .. r + 7 of a row-major LDS array (stride in elements), packed as an MFMA k-fragment
__device__ __forceinline__ uint4 gather8(const bf16_t* p, int stride) {
  const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
  uint32_t w[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) w[e] = (uint32_t)q[(2 * e) * stride] | ((uint32_t)q[(2 * e + 1) * stride] << 16);
  return uint4{w[0], w[1], w[2], w[3]};
}

__device__ __forceinline__ uint32_t split_bf16(float v, uint32_t* lo) {
  const uint32_t h = f2bf(v);
  *lo = f2bf(v - bf2f(h));
  return h;
}

// CONT (zmi_mamba2_scan_cont): a sequence with pos0 > 0 continues from the bf16 state h0 (mamba2_carry_kernel's copy in
// the workspace, h0s by cont_rank: neither role reads the state row the state role writes). Two more terms,
//     y_t   += exp(cum[t]) (C_t . h0)      one more bf16 MFMA per y tile (C, h0 exactly bf16), fp32 sums; the wave's
//                                           h0 fragments (16 p x 128 n, 4 uint4 per lane) stay in registers: the y
//                                           role's LDS is full at T = 256
//     state  = exp(cum[T-1]) h0 + W^T B    the accumulators start from the decayed h0
// with cum in fp64 as everywhere. A sequence with pos0 == 0 reads no h0 and runs the arithmetic of the plain kernel.
template <bool CONT>
__global__ __launch_bounds__(SSD_NT) void mamba2_ssd_kernel(const ZmiMamba2Args a, const ScanSeqs sqs, const bf16_t* xc,
                                                         const float* dts, const bf16_t* h0s) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // sized for the launch's longest sequence
  __shared__ int seq_sh;
  const int role = blockIdx.x & 1, sh = blockIdx.x >> 1, h = sh % a.nheads;
  const ScanSeq sq = scan_seq_at(a, sqs, sh / a.nheads, &seq_sh);
  if (sq.T == 0 || sq.T > SSD_TMAX) return;
  const int T = sq.T;  // this sequence's own length: its LDS layout and arithmetic are those of a launch of it alone
  const int row0 = sq.row0, conv_dim = a.d_ssm + 2 * MB_DS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const SsdLds L(T);
  double* cum = reinterpret_cast<double*>(smem);
  float* dtl = reinterpret_cast<float*>(cum + SSD_TMAX);
  const float Ah = a.A[h];
  const bool state_role = role == 1;
  const int s32 = L.S32;
  bool cont = false;
  const bf16_t* h0 = nullptr;
  if constexpr (CONT) {
    cont = sqs.seqs[sq.idx].pos0 > 0;
    if (cont) h0 = h0s + ((size_t)cont_rank(a, sqs, sq.idx) * a.nheads + h) * MB_HD * MB_DS;
  }
  bf16_t* Bs = reinterpret_cast<bf16_t*>(smem + L.b_off());
  // (1) B rows s < s_end (zero to s32) for both roles; dt and cum for every position (the same fixed-shape scan in
  // every role: lane L owns positions 4L .. 4L + 3)
  for (int i = t; i < s32 * (MB_DS / 8); i += SSD_NT) {
    const int r = i / (MB_DS / 8), c = i % (MB_DS / 8);
    uint4 v = uint4{0u, 0u, 0u, 0u};
    if (r < T) v = *reinterpret_cast<const uint4*>(xc + (size_t)(row0 + r) * conv_dim + a.d_ssm + 8 * c);
    *reinterpret_cast<uint4*>(Bs + r * SSD_BROW + 8 * c) = v;
  }
  if (wave == 0) {
    double v[4], run = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = 4 * lane + i;
      const float d = q < T ? dts[(size_t)(row0 + q) * a.nheads + h] : 0.f;
      dtl[q] = d;
      run += (double)Ah * (double)d;  // the product of two floats: exact
      v[i] = run;
    }
    double pre = run;  // inclusive scan of the lane totals
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double o = __shfl_up(pre, d, 64);
      if (lane >= d) pre += o;
    }
    const double excl = pre - run;
#pragma unroll
    for (int i = 0; i < 4; ++i) cum[4 * lane + i] = excl + v[i];
  }
  if (!state_role) {
    bf16_t* Cs = reinterpret_cast<bf16_t*>(smem + L.c_off());
    bf16_t* Mh = reinterpret_cast<bf16_t*>(smem + L.mh_off());
    bf16_t* Ml = reinterpret_cast<bf16_t*>(smem + L.ml_off());
    bf16_t* Xs = reinterpret_cast<bf16_t*>(smem + L.x_off());
    const int MP = L.MP();
    // (2) x rows (zero to s32); the first row block's C rows into registers (2 x 16 B per thread), each later block's
    // loaded while the previous one computes
    for (int i = t; i < s32 * (MB_HD / 8); i += SSD_NT) {
      const int r = i / (MB_HD / 8), c = i % (MB_HD / 8);
      uint4 v = uint4{0u, 0u, 0u, 0u};
      if (r < T) v = *reinterpret_cast<const uint4*>(xc + (size_t)(row0 + r) * conv_dim + h * MB_HD + 8 * c);
      *reinterpret_cast<uint4*>(Xs + r * SSD_XROW + 8 * c) = v;
    }
    constexpr int CP = SSD_TB * (MB_DS / 8), CPT = (CP + SSD_NT - 1) / SSD_NT;  // C pieces (16 B), per thread
    uint4 cr[CPT];
    auto load_c = [&](int tb0) {
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        const int i = t + SSD_NT * j, r = i / (MB_DS / 8), c = i % (MB_DS / 8);
        cr[j] = i < CP && tb0 + r < T
                    ? *reinterpret_cast<const uint4*>(xc + (size_t)(row0 + tb0 + r) * conv_dim + a.d_ssm + MB_DS + 8 * c)
                    : uint4{0u, 0u, 0u, 0u};
      }
    };
    load_c(0);
    const float Dh = a.D[h];
    uint4 hf[MB_DS / 32];  // CONT: h0 rows of the wave's p tile as MFMA B fragments (k over the state columns)
    if (CONT && cont && wave < 8) {
#pragma unroll
      for (int kk = 0; kk < MB_DS / 32; ++kk)
        hf[kk] = *reinterpret_cast<const uint4*>(h0 + (size_t)(16 * (wave >> 1) + (lane & 15)) * MB_DS + 32 * kk +
                                                 8 * (lane >> 4));
    }
    for (int t0 = 0; t0 < T; t0 += SSD_TB) {
      const int tn = min(SSD_TB, T - t0), s_end = t0 + tn, sk = (s_end + 31) / 32;  // k-blocks of 32 positions
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        const int i = t + SSD_NT * j, r = i / (MB_DS / 8), c = i % (MB_DS / 8);
        if (i < CP) *reinterpret_cast<uint4*>(Cs + r * SSD_BROW + 8 * c) = cr[j];
      }
      __syncthreads();  // C block (and, the first time, B / x / cum) visible; the previous block's y reads are done
      if (t0 + SSD_TB < T) load_c(t0 + SSD_TB);
      // (3) M tiles (16 t x 16 s) over s < 32 sk: G = C B^T on the tiles that reach s <= t, zeros elsewhere. A wave's
      // tiles share ti = wave & 1 (the stride is even), so its four rows' cum is read once per block
      double ct[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) ct[i] = cum[t0 + 16 * (wave & 1) + 4 * (lane >> 4) + i];  // < S32 <= SSD_TMAX
      // CONT: g0 = C_blk h0^T of this wave's y tile (t tile wave & 1, p tile wave >> 1), taken HERE, between the
      // block's two barriers, where the C rows are stable: after the second barrier the waves that finish step (4)
      // refill Cs with the next block's rows while others are still in (4), so (4) must not read Cs (the plain kernel's
      // (4) reads only M and x). g0 waits in registers for the y tile.
      f32x4_t g0 = {0.f, 0.f, 0.f, 0.f};
      if (CONT && cont && wave < 8) {
#pragma unroll
        for (int kk = 0; kk < MB_DS / 32; ++kk)
          g0 = mfma_bf16(*reinterpret_cast<const uint4*>(Cs + (16 * (wave & 1) + (lane & 15)) * SSD_BROW + 32 * kk +
                                                         8 * (lane >> 4)), hf[kk], g0);
      }
      for (int tile = wave; tile < 4 * sk; tile += SSD_NT / 64) {
        const int ti = tile & 1, si = tile >> 1;
        const bool live = 16 * ti < tn && 16 * si <= t0 + 16 * ti + 15;
        f32x4_t g = {0.f, 0.f, 0.f, 0.f};
        if (live) {
#pragma unroll
          for (int kk = 0; kk < MB_DS / 32; ++kk) {
            const uint4 av = *reinterpret_cast<const uint4*>(Cs + (16 * ti + (lane & 15)) * SSD_BROW + 32 * kk + 8 * (lane >> 4));
            const uint4 bv = *reinterpret_cast<const uint4*>(Bs + (16 * si + (lane & 15)) * SSD_BROW + 32 * kk + 8 * (lane >> 4));
            g = mfma_bf16(av, bv, g);
          }
        }
        const int s = 16 * si + (lane & 15);  // < 32 sk <= S32
        const double cs = cum[s];
        const float ds = dtl[s];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int tl = 16 * ti + 4 * (lane >> 4) + i, tt = t0 + tl;
          float m = 0.f;
          if (live && tl < tn && s <= tt) m = g[i] * expf((float)(ct[i] - cs)) * ds;
          uint32_t lo;
          const uint32_t hi = split_bf16(m, &lo);
          Mh[tl * MP + s] = (bf16_t)hi;
          Ml[tl * MP + s] = (bf16_t)lo;
        }
      }
      __syncthreads();
      // (4) y tiles (16 t x 16 p): wave w < 8 -> t tile w & 1, p tile w >> 1; the x fragment of a k-block (8 consecutive
      // positions of column p) gathered from the row-major x rows
      const int ti = wave & 1;
      if (wave < 8 && 16 * ti < tn) {
        {
          const int pj = wave >> 1, p = 16 * pj + (lane & 15);
          f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
          for (int kk = 0; kk < sk; ++kk) {
            const int mo = (16 * ti + (lane & 15)) * MP + 32 * kk + 8 * (lane >> 4);
            const uint4 bv = gather8(Xs + (32 * kk + 8 * (lane >> 4)) * SSD_XROW + p, SSD_XROW);
            acc = mfma_bf16(*reinterpret_cast<const uint4*>(Mh + mo), bv, acc);
            acc = mfma_bf16(*reinterpret_cast<const uint4*>(Ml + mo), bv, acc);
          }
          if (CONT && cont) {  // + exp(cum[t]) (C_t . h0): g0 from step (3)'s phase, ct this wave's rows' cum
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] += expf((float)ct[i]) * g0[i];
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int tl = 16 * ti + 4 * (lane >> 4) + i;
            if (tl < tn) {
              const float x = bf2f((uint32_t)reinterpret_cast<const uint16_t*>(Xs)[(t0 + tl) * SSD_XROW + p]);
              reinterpret_cast<bf16_t*>(a.y)[(size_t)(row0 + t0 + tl) * a.ldy + h * MB_HD + p] =
                  (bf16_t)f2bf(acc[i] + x * Dh);
            }
          }
        }
      }
    }
  } else {
    bf16_t* Wh = reinterpret_cast<bf16_t*>(smem + L.wh_off());
    bf16_t* Wl = reinterpret_cast<bf16_t*>(smem + L.wl_off());
    __syncthreads();  // cum / dt
    const double cT = cum[T - 1];
    // (2) W rows [s][p] = exp(cum[T-1] - cum[s]) dt_s x_s[p] as hi / lo bf16, zero past T
    for (int i = t; i < s32 * (MB_HD / 8); i += SSD_NT) {
      const int r = i / (MB_HD / 8), c = i % (MB_HD / 8);
      uint32_t hv[4] = {0u, 0u, 0u, 0u}, lv[4] = {0u, 0u, 0u, 0u};
      if (r < T) {
        const uint4 v = *reinterpret_cast<const uint4*>(xc + (size_t)(row0 + r) * conv_dim + h * MB_HD + 8 * c);
        const float w = expf((float)(cT - cum[r])) * dtl[r];
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          uint32_t l0, l1;
          const uint32_t h0 = split_bf16(w * bf2f(u[e]), &l0), h1 = split_bf16(w * bf2f(u[e] >> 16), &l1);
          hv[e] = h0 | (h1 << 16);
          lv[e] = l0 | (l1 << 16);
        }
      }
      *reinterpret_cast<uint4*>(Wh + r * SSD_XROW + 8 * c) = uint4{hv[0], hv[1], hv[2], hv[3]};
      *reinterpret_cast<uint4*>(Wl + r * SSD_XROW + 8 * c) = uint4{lv[0], lv[1], lv[2], lv[3]};
    }
    __syncthreads();
    // (3) state tiles (16 p x 16 n): wave w -> p tile w & 3, n tiles 4 (w >> 2) .. + 3; A = W^T and B fragments
    // gathered per k-block
    constexpr int NPW = MB_DS / 16 / (SSD_NT / 64 / 4);  // n tiles per wave
    const int kv = scan_kv(a, sqs, sq);
    bf16_t* st = reinterpret_cast<bf16_t*>(a.ssm) + ((size_t)kv * a.nheads + h) * MB_HD * MB_DS;
    const int pi = wave & 3, nb = (wave >> 2) * NPW;
    f32x4_t acc[NPW];
#pragma unroll
    for (int ni = 0; ni < NPW; ++ni) acc[ni] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (CONT && cont) {  // exp(cum[T-1]) h0
      const float eT = expf((float)cT);
#pragma unroll
      for (int ni = 0; ni < NPW; ++ni)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[ni][i] = eT * bf2f((uint32_t)reinterpret_cast<const uint16_t*>(
                                h0)[(size_t)(16 * pi + 4 * (lane >> 4) + i) * MB_DS + 16 * (nb + ni) + (lane & 15)]);
    }
    for (int kk = 0; kk < s32 / 32; ++kk) {
      const int r = 32 * kk + 8 * (lane >> 4);
      const uint4 ah = gather8(Wh + r * SSD_XROW + 16 * pi + (lane & 15), SSD_XROW);
      const uint4 al = gather8(Wl + r * SSD_XROW + 16 * pi + (lane & 15), SSD_XROW);
#pragma unroll
      for (int ni = 0; ni < NPW; ++ni) {
        const uint4 bv = gather8(Bs + r * SSD_BROW + 16 * (nb + ni) + (lane & 15), SSD_BROW);
        acc[ni] = mfma_bf16(ah, bv, acc[ni]);
        acc[ni] = mfma_bf16(al, bv, acc[ni]);
      }
    }
#pragma unroll
    for (int ni = 0; ni < NPW; ++ni) {
      const int n = 16 * (nb + ni) + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) st[(size_t)(16 * pi + 4 * (lane >> 4) + i) * MB_DS + n] = (bf16_t)f2bf(acc[ni][i]);
    }
  }
}

int check_mamba(const ZmiMamba2Args* a) {
  if (!a || !a->zxbcdt || !a->conv_w || !a->conv_b || !a->dt_bias || !a->A || !a->D || !a->conv_ring || !a->ssm ||
      !a->y || !a->row_pos)
    return zmi_fail_msg("mamba2: missing buffers");
  if (a->headdim != MB_HD || a->d_state != MB_DS || a->d_conv != MB_DC || a->ngroups != 1)
    return zmi_fail_msg("mamba2: built for headdim 64, d_state 128, d_conv 4, ngroups 1");
  if (a->nheads <= 0 || a->d_ssm != a->nheads * MB_HD) return zmi_fail_msg("mamba2: d_ssm = nheads x 64");
  if (a->ld_zx < 2 * a->d_ssm + 2 * MB_DS + a->nheads || a->ldy < a->d_ssm)
    return zmi_fail_msg("mamba2: ld_zx >= 2 d_ssm + 2 d_state + nheads, ldy >= d_ssm");
  return 0;
}

}  // namespace

extern "C" int zmi_mamba2_step(const ZmiMamba2Args* a, void* stream) {
  if (int e = check_mamba(a)) return e;
  if (a->M <= 0) return 0;
  hipLaunchKernelGGL(mamba2_step_kernel, dim3((unsigned)(a->M * a->nheads)), dim3(MB_ST), 0, (hipStream_t)stream, *a);
  ZMI_CHECK(hipGetLastError());
  return 0;
}

extern "C" int zmi_mamba2_scan(const ZmiMamba2Args* a, int seq_len, void* stream) {
  if (int e = check_mamba(a)) return e;
  if (seq_len <= 0 || a->M % seq_len) return zmi_fail_msg("mamba2_scan: M must be a multiple of seq_len > 0");
  hipLaunchKernelGGL(mamba2_scan_kernel, dim3((unsigned)(a->M / seq_len * a->nheads)), dim3(MB_NT), 0,
                     (hipStream_t)stream, *a, seq_len);
  ZMI_CHECK(hipGetLastError());
  return 0;
}

extern "C" int64_t zmi_mamba2_scan_ws_bytes(int m, int d_ssm, int nheads) {
  if (m <= 0 || d_ssm <= 0 || nheads <= 0) return 0;
  const int64_t xc = ((int64_t)m * (d_ssm + 2 * MB_DS) * 2 + 255) / 256 * 256;
  return xc + 2 * (((int64_t)m * nheads * 4 + 255) / 256 * 256);
}

// + one bf16 state [nheads][64][128] per continuing sequence (pos0 > 0, len > 0): mamba2_carry_kernel's copies
extern "C" int64_t zmi_mamba2_scan_cont_ws_bytes(int m, int d_ssm, int nheads, int n_cont) {
  const int64_t base = zmi_mamba2_scan_ws_bytes(m, d_ssm, nheads);
  if (base <= 0 || n_cont < 0) return 0;
  return base + (int64_t)n_cont * nheads * MB_HD * MB_DS * 2;
}

namespace {

// The conv + dt launch over the a->M rows, then the scan launches: n_ssd sequences in the SSD form (LDS for the
// longest, t_max positions) and n_scan in mamba2_scan2_kernel<PQ>; `sq` says which rows are which sequence.
// CONT (zmi_mamba2_scan_cont, ragged tables only): mamba2_carry_kernel between the conv launch and the scans, h0s its
// copies of the continuing sequences' states.
template <bool CONT>
int launch_scan(const ZmiMamba2Args* a, ScanSeqs sq, int n_ssd, int t_max, int n_scan, int pq, void* ws,
                hipStream_t s) {
  const int64_t xcb = ((int64_t)a->M * (a->d_ssm + 2 * MB_DS) * 2 + 255) / 256 * 256;
  const int64_t hb = ((int64_t)a->M * a->nheads * 4 + 255) / 256 * 256;
  bf16_t* xc = (bf16_t*)ws;
  float* dts = (float*)((char*)ws + xcb);
  float* das = (float*)((char*)ws + xcb + hb);
  bf16_t* h0s = CONT ? (bf16_t*)((char*)ws + xcb + 2 * hb) : nullptr;
  const int conv_dim = a->d_ssm + 2 * MB_DS;
  sq.lo = 0, sq.hi = INT_MAX;
  hipLaunchKernelGGL(mamba2_conv_kernel<CONT>, dim3((unsigned)a->M, (unsigned)((conv_dim + 255) / 256)), dim3(256), 0,
                     s, *a, sq, xc, dts, das);
  ZMI_CHECK(hipGetLastError());
  if constexpr (CONT) {
    hipLaunchKernelGGL(mamba2_carry_kernel, dim3((unsigned)sq.n_seq, (unsigned)(a->nheads + 1)), dim3(256), 0, s, *a,
                       sq, h0s);
    ZMI_CHECK(hipGetLastError());
  }
  if (n_ssd > 0) {  // the quadratic (SSD) form
    const SsdLds L(t_max);
    const size_t lds = std::max(L.y_bytes(), L.s_bytes());
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&mamba2_ssd_kernel<CONT>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       160 * 1024 - 16);  // the kernel's static LDS word comes off
    ZMI_CHECK(attr);
    sq.lo = 0, sq.hi = SSD_TMAX;
    hipLaunchKernelGGL(mamba2_ssd_kernel<CONT>, dim3((unsigned)((int64_t)n_ssd * a->nheads * 2)), dim3(SSD_NT), lds, s,
                       *a, sq, (const bf16_t*)xc, (const float*)dts, (const bf16_t*)h0s);
    ZMI_CHECK(hipGetLastError());
  }
  if (n_scan > 0) {
    sq.lo = pq == 0 ? SSD_TMAX : 0, sq.hi = INT_MAX;  // 0: the sequences past the quadratic form's reach
    const dim3 grid((unsigned)((int64_t)n_scan * a->nheads * (pq == 0 ? 4 : pq)));
    if (pq == 1)
      hipLaunchKernelGGL((mamba2_scan2_kernel<1, CONT>), grid, dim3(256), 0, s, *a, sq, (const bf16_t*)xc,
                         (const float*)dts, (const float*)das);
    else if (pq == 2)
      hipLaunchKernelGGL((mamba2_scan2_kernel<2, CONT>), grid, dim3(256), 0, s, *a, sq, (const bf16_t*)xc,
                         (const float*)dts, (const float*)das);
    else
      hipLaunchKernelGGL((mamba2_scan2_kernel<4, CONT>), grid, dim3(256), 0, s, *a, sq, (const bf16_t*)xc,
                         (const float*)dts, (const float*)das);
    ZMI_CHECK(hipGetLastError());
  }
  return 0;
}

bool scan_pq_ok(int pq) { return pq == 0 || pq == 1 || pq == 2 || pq == 4; }

}  // namespace

extern "C" int zmi_mamba2_scan_ws(const ZmiMamba2Args* a, int seq_len, void* ws, int64_t ws_bytes, void* stream) {
  if (int e = check_mamba(a)) return e;
  if (seq_len <= 0 || a->M % seq_len) return zmi_fail_msg("mamba2_scan_ws: M must be a multiple of seq_len > 0");
  if (!ws || ws_bytes < zmi_mamba2_scan_ws_bytes(a->M, a->d_ssm, a->nheads))
    return zmi_fail_msg("mamba2_scan_ws: workspace smaller than zmi_mamba2_scan_ws_bytes");
  const int pq = zmi_option(ZMI_OPT_SCAN_PQ);
  if (!scan_pq_ok(pq)) return zmi_fail_msg("mamba2_scan_ws: ZMI_OPT_SCAN_PQ must be 0, 1, 2 or 4");
  const bool ssd = pq == 0 && seq_len <= SSD_TMAX;
  const int n = a->M / seq_len;
  return launch_scan<false>(a, ScanSeqs{nullptr, 0, seq_len, 0, 0}, ssd ? n : 0, seq_len, ssd ? 0 : n, pq, ws,
                     (hipStream_t)stream);
}

namespace {

// zmi_mamba2_scan_seqs (CONT false: every sequence from an empty state) and zmi_mamba2_scan_cont: the host checks on
// the table's host copy, before any launch, then launch_scan
template <bool CONT>
int scan_table(const ZmiMamba2Args* a, const ZmiAttnSeq* seqs, int n_seq, const ZmiAttnSeq* seqs_host, void* ws,
               int64_t ws_bytes, void* stream) {
#define ZMI_SCAN_FAIL(text_) return zmi_fail_msg(CONT ? "mamba2_scan_cont: " text_ : "mamba2_scan_seqs: " text_)
  if (int e = check_mamba(a)) return e;
  if (n_seq < 0) ZMI_SCAN_FAIL("n_seq < 0");
  if (n_seq > 0 && (!seqs || !seqs_host))
    ZMI_SCAN_FAIL("the device table and its host copy are required");
  const int pq = zmi_option(ZMI_OPT_SCAN_PQ);
  if (!scan_pq_ok(pq)) ZMI_SCAN_FAIL("ZMI_OPT_SCAN_PQ must be 0, 1, 2 or 4");
  std::vector<std::pair<int, int>> rows, kvs;  // (first row, row past the last), (state row, index) of the live ones
  int n_ssd = 0, n_scan = 0, t_max = 0, n_cont = 0;
  for (int i = 0; i < n_seq; ++i) {
    const ZmiAttnSeq& s = seqs_host[i];
    if (s.len < 0 || s.q_row0 < 0) ZMI_SCAN_FAIL("negative len or q_row0");
    if (s.q_row0 > a->M - s.len) ZMI_SCAN_FAIL("a sequence's rows end past M");
    if (!CONT && s.pos0 != 0) ZMI_SCAN_FAIL("pos0 must be 0 (prefill from an empty state)");
    if (CONT && s.pos0 < 0) ZMI_SCAN_FAIL("negative pos0");
    if (CONT && s.pos0 > INT_MAX - s.len) ZMI_SCAN_FAIL("pos0 + len overflows");
    if (s.kv_row < 0) ZMI_SCAN_FAIL("negative kv_row");
    if (s.len == 0) continue;
    n_cont += s.pos0 > 0 ? 1 : 0;
    rows.emplace_back(s.q_row0, s.q_row0 + s.len);
    kvs.emplace_back(s.kv_row, i);
    if (pq == 0 && s.len <= SSD_TMAX) {
      ++n_ssd;
      t_max = std::max(t_max, s.len);
    } else {
      ++n_scan;
    }
  }
  std::sort(rows.begin(), rows.end());
  std::sort(kvs.begin(), kvs.end());
  for (size_t i = 1; i < rows.size(); ++i) {
    if (rows[i].first < rows[i - 1].second) ZMI_SCAN_FAIL("two sequences share rows");
    if (kvs[i].first == kvs[i - 1].first) ZMI_SCAN_FAIL("two sequences share a kv_row");
  }
  if (!CONT && (!ws || ws_bytes < zmi_mamba2_scan_ws_bytes(a->M, a->d_ssm, a->nheads)))
    ZMI_SCAN_FAIL("workspace smaller than zmi_mamba2_scan_ws_bytes");
  if (CONT && (!ws || ws_bytes < zmi_mamba2_scan_cont_ws_bytes(a->M, a->d_ssm, a->nheads, n_cont)))
    ZMI_SCAN_FAIL("workspace smaller than zmi_mamba2_scan_cont_ws_bytes");
  if (rows.empty()) return 0;
  return launch_scan<CONT>(a, ScanSeqs{seqs, n_seq, 0, 0, 0}, n_ssd, t_max, n_scan, pq, ws, (hipStream_t)stream);
#undef ZMI_SCAN_FAIL
}

}  // namespace

extern "C" int zmi_mamba2_scan_seqs(const ZmiMamba2Args* a, const ZmiAttnSeq* seqs, int n_seq,
                                    const ZmiAttnSeq* seqs_host, void* ws, int64_t ws_bytes, void* stream) {
  return scan_table<false>(a, seqs, n_seq, seqs_host, ws, ws_bytes, stream);
}

extern "C" int zmi_mamba2_scan_cont(const ZmiMamba2Args* a, const ZmiAttnSeq* seqs, int n_seq,
                                    const ZmiAttnSeq* seqs_host, void* ws, int64_t ws_bytes, void* stream) {
  return scan_table<true>(a, seqs, n_seq, seqs_host, ws, ws_bytes, stream);
}
