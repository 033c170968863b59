// Weight-streaming GEMV / skinny GEMM entry points (kernel: zmi_gemv_impl.h) and the weight packer.
//
// out[m, n] = sum_k A[m, k] * W[n, k]   (nn.Linear, reference zonos/backbone/_torch.py:114-115,147-152,
//                                        heads: zonos/model.py:100-101)
#include "zmi_common.h"
#include "zmi_kernels.h"
#include "zmi_gemv_impl.h"

namespace zmi_gemv {
hipError_t launch_epi0(const ZmiGemvArgs& a, hipStream_t s);
hipError_t launch_epi1(const ZmiGemvArgs& a, hipStream_t s);
hipError_t launch_epi2(const ZmiGemvArgs& a, hipStream_t s);
hipError_t launch_epi3(const ZmiGemvArgs& a, hipStream_t s);
hipError_t launch_epi4(const ZmiGemvArgs& a, hipStream_t s);
hipError_t launch_epi5(const ZmiGemvArgs& a, hipStream_t s);
}  // namespace zmi_gemv

namespace {

// Pack a row-major [N_src][K] bf16 weight into the M8 layout (zmi_gemv_impl.h): 1 KiB chunk (g, kc),
// lane l = column 8g + (l & 7), k = 64 kc + 32 ((l >> 3) & 1) + 8 (l >> 4) .. +7; zero rows beyond
// N_src. SwiGLU mode interleaves fc1's value and gate halves per group: rows 0..3 of group g are
// value rows 4g.., rows 4..7 their gates F + 4g.. (F = N_src / 2).
__global__ void pack_kernel(const bf16_t* __restrict__ src, uint4* __restrict__ dst, int n_src, int k, int n_pad,
                            int mode) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int kc_n = k >> 6;
  const size_t total = (size_t)(n_pad >> 3) * kc_n * 64;
  if (idx >= total) return;
  const int l = idx & 63;
  const size_t t = idx >> 6;
  const int kc = (int)(t % kc_n), g = (int)(t / kc_n);
  const int r = l & 7, n = g * 8 + r, kk = kc * 64 + 32 * ((l >> 3) & 1) + 8 * (l >> 4);
  int srow = n;
  if (mode == ZMI_PACK_SWIGLU) {
    const int f = n_src >> 1;
    srow = r < 4 ? g * 4 + r : f + g * 4 + (r - 4);
  }
  uint4 v = {0u, 0u, 0u, 0u};
  if (srow < n_src) v = *reinterpret_cast<const uint4*>(src + (size_t)srow * k + kk);
  dst[idx] = v;
}

// Expand an fp8 weight (layout M8F8 + one int8 exponent per packed column, quant.py) into the bf16 layout M8: the
// bytes zmi_pack_weight gives for the dequantised weight 2^e q. A thread takes one lane of a 1 KiB M8F8 piece (g, p):
// its 16 bytes are column 8g + (l & 7)'s 8 weights of the 64-k chunks 2p and 2p + 1, which are lane l of the M8
// chunks (g, 2p) and (g, 2p + 1). E4M3 -> f32 is exact, 2^e q is a normal bf16 or a signed zero (quant.py), so the
// product's high half is the weight. No reduction: nothing to round.
__global__ void unpack_fp8_kernel(const uint4* __restrict__ src, const signed char* __restrict__ w_exp,
                                  uint4* __restrict__ dst, int n_pad, int k) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int np = k >> 7;  // pieces per group
  const size_t total = (size_t)(n_pad >> 3) * np * 64;
  if (idx >= total) return;
  const int l = idx & 63;
  const size_t t = idx >> 6;
  const int p = (int)(t % np), g = (int)(t / np);
  const float scale = __uint_as_float((uint32_t)((int)w_exp[g * 8 + (l & 7)] + 127) << 23);
  const uint4 q = src[idx];
  auto pair = [&](uint32_t d, bool hi) {  // two E4M3 bytes -> two scaled bf16
    const auto f = hi ? __builtin_amdgcn_cvt_pk_f32_fp8((int)d, true) : __builtin_amdgcn_cvt_pk_f32_fp8((int)d, false);
    return (__float_as_uint(f[0] * scale) >> 16) | (__float_as_uint(f[1] * scale) & 0xffff0000u);
  };
  const uint4 c0 = {pair(q.x, false), pair(q.x, true), pair(q.y, false), pair(q.y, true)};
  const uint4 c1 = {pair(q.z, false), pair(q.z, true), pair(q.w, false), pair(q.w, true)};
  uint4* o = dst + ((size_t)g * (2 * np) + 2 * p) * 64 + l;
  o[0] = c0;
  o[64] = c1;
}

}  // namespace

// the argument checks of zmi_gemv_launch (0 = accepted; else zmi_last_error is set)
static int check_args(const ZmiGemvArgs& a, int epi) {
  zmi_gemv::Shape sh;
  if (a.N % 8) return zmi_fail_msg("gemv: N must be a multiple of 8");
  if (!zmi_gemv::shape_for(a.K, &sh))
    return zmi_fail_msg("gemv: K must be 512, 1024, 2048, 4096 or 8192");
  if (a.M < 1) return zmi_fail_msg("gemv: M must be >= 1");
  if (a.ldx % 8) return zmi_fail_msg("gemv: ldx must be a multiple of 8 (16-byte rows)");
  if (a.groups < 0 || a.groups > 2 || (a.groups == 2 && a.K != 2048 && a.K != 8192))
    return zmi_fail_msg("gemv: groups must be 0 (library choice), 1, or 2 for K = 2048 / 8192");
  if (a.pro != ZMI_PRO_AUTO && a.pro != ZMI_PRO_ADDLN && a.pro != ZMI_PRO_GRMS && a.pro != ZMI_PRO_GRMS_G)
    return zmi_fail_msg("gemv: unknown prologue");
  if (a.pro == ZMI_PRO_ADDLN && (!a.ln_w || !a.ln_b || !a.aux || a.ld_aux % 8 || a.res_out == a.aux))
    return zmi_fail_msg("gemv: ADDLN needs ln_w, ln_b, aux (ld_aux % 8 == 0) and res_out != aux");
  if ((a.pro == ZMI_PRO_GRMS || a.pro == ZMI_PRO_GRMS_G) && (!a.ln_w || !a.aux || a.ld_aux % 8 || a.M > 4))
    return zmi_fail_msg("gemv: GRMS needs ln_w (the norm weight), aux = the f32 gate or g rows (ld_aux % 8 == 0), M <= 4");
  if (epi == ZMI_EPI_QKV && (a.hd % 8 || a.smax <= 0 || !a.row_pos || !a.row_kv || !a.rope))
    return zmi_fail_msg("gemv: the QKV epilogue needs row_pos, row_kv, rope, smax and hd % 8 == 0");
  if (a.w_fmt != ZMI_WFMT_BF16 && a.w_fmt != ZMI_WFMT_FP8) return zmi_fail_msg("gemv: unknown weight format");
  if (epi < ZMI_EPI_STORE || epi > ZMI_EPI_F32) return zmi_fail_msg("gemv: unknown epilogue");
  if (a.w_fmt == ZMI_WFMT_FP8) {  // ZMI_PRO_* = PRO_*; ZMI_PRO_AUTO: LayerNorm with ln_w, else plain
    const int pro = a.pro != ZMI_PRO_AUTO ? a.pro : (a.ln_w ? zmi_gemv::PRO_LN : zmi_gemv::PRO_PLAIN);
    if (!a.w_exp || ((size_t)a.w_exp & 7) || !zmi_gemv::pro_built(a.K, epi, pro, true))
      return zmi_fail_msg("gemv: fp8 weights need w_exp (8-byte aligned) and are built for the SWIGLU, RESIDUAL and F32 "
                          "epilogues with the plain / LayerNorm prologue (K = 512, 1024, 2048 or 8192), and for the STORE "
                          "epilogue with ADDLN (K = 512 or 2048), GRMS / GRMS_G (K = 1024 or 4096) or plain rows at "
                          "K = 1024 or 4096");
  }
  return 0;
}

static int not_built(const ZmiGemvArgs& a) {
  if (a.pro != ZMI_PRO_AUTO)
    return zmi_fail_msg("gemv: prologue not built for this K / epilogue / row count (ADDLN: K 512 or 2048; GRMS: K "
                        "1024 or 4096, ZMI_EPI_STORE, rows within the LDS image)");
  return zmi_fail_msg("gemv: form not built for these arguments (groups, rows within the LDS image)");
}

extern "C" int zmi_gemv_form(const ZmiGemvArgs* args, int epi, ZmiGemvForm* out) {
  if (const int rc = check_args(*args, epi)) return rc;
  if (!zmi_gemv::form_for(*args, epi, out)) return not_built(*args);
  return 0;
}

extern "C" int zmi_gemv_launch(const ZmiGemvArgs* args, int epi, void* stream) {
  const ZmiGemvArgs& a = *args;
  if (const int rc = check_args(a, epi)) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  switch (epi) {
    case ZMI_EPI_STORE: e = zmi_gemv::launch_epi0(a, s); break;
    case ZMI_EPI_RESIDUAL: e = zmi_gemv::launch_epi1(a, s); break;
    case ZMI_EPI_QKV: e = zmi_gemv::launch_epi2(a, s); break;
    case ZMI_EPI_SWIGLU: e = zmi_gemv::launch_epi3(a, s); break;
    case ZMI_EPI_LOGITS: e = zmi_gemv::launch_epi4(a, s); break;
    case ZMI_EPI_F32: e = zmi_gemv::launch_epi5(a, s); break;
    default: return zmi_fail_msg("gemv: unknown epilogue");
  }
  if (e == hipErrorInvalidValue && a.pro != ZMI_PRO_AUTO) return not_built(a);
  ZMI_CHECK(e);
  return 0;
}

extern "C" int zmi_pack_weight(const void* src, void* dst, int n_src, int k, int n_pad, int mode, void* stream) {
  if (n_pad % 8 || k % 64 || n_pad < n_src || (mode == ZMI_PACK_SWIGLU && (n_src % 8 || n_pad != n_src)))
    return zmi_fail_msg("pack: bad shape");
  const size_t total = (size_t)(n_pad / 8) * (k / 64) * 64;
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)src, (uint4*)dst, n_src, k, n_pad, mode);
  ZMI_CHECK(hipGetLastError());
  return 0;
}

extern "C" int zmi_unpack_fp8(const void* m8f8, const void* w_exp, int n_pad, int k, void* m8_out, void* stream) {
  if (!m8f8 || !w_exp || !m8_out || n_pad < 8 || n_pad % 8 || k < 128 || k % 128 || ((size_t)m8f8 & 15) ||
      ((size_t)m8_out & 15))
    return zmi_fail_msg("unpack_fp8: n_pad % 8, k % 128, 16-byte aligned weights, w_exp set");
  const size_t total = (size_t)(n_pad / 8) * (k / 128) * 64;
  if ((total + 255) / 256 > 0x7fffffffu) return zmi_fail_msg("unpack_fp8: weight too large");
  hipLaunchKernelGGL(unpack_fp8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const uint4*)m8f8, (const signed char*)w_exp, (uint4*)m8_out, n_pad, k);
  ZMI_CHECK(hipGetLastError());
  return 0;
}
