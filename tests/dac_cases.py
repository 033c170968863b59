"""Cases, fp64 references and the derived error bound shared by the CPU and GPU per-kernel tests of the DAC conv
stack (zmi_dac.hip: zmi_dac_conv / conv_t / conv_out(_range) / from_codes / im2col7 / vq).

Inputs are seeded and exactly representable in the format the kernel reads (activations, weights and skip in fp16;
bias and Snake alpha in fp32), so the fp64 reference and the kernel start from the same numbers and every fp16 x fp16
product is exact in fp32. Activations are channels-last [T][C], as the kernels read them.

References are built from the UNPACKED torch-layout weights with torch.nn.functional in float64; `emulate_conv` is a
float64 restatement of the kernel's documented index arithmetic over the PACKED weights (include/zonos_hip.h), which
ties the packing helpers of zonos_vibes_amd/autoencoder.py to those references on the CPU.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle.dac_cpu import snake as _snake

U32 = 2.0 ** -24      # fp32 unit roundoff
U16 = 2.0 ** -11      # fp16 unit roundoff
SUB16 = 2.0 ** -25    # half the spacing of fp16 subnormals (values below 2^-14)

# Measured on an MI355X against fp64 over the cases of tests/test_gpu_dac_kernels.py; each constant is
# twice the measured maximum, because the inputs sample the argument range and do not exhaust it.
#   delta_sin: max over the Snake cases that also write out_f32 of
#              (|z_gpu - snake64(out_f32_gpu)| - 2^-11 |z| - 2^-25) alpha / 2
#       measured -3.83e-9 (per shape -1.9e-8 .. -3.8e-9): NEGATIVE, the Snake epilogue (v_sin_f32, the fp32
#       reciprocal, square and add) never left the fp16 rounding allowance of its own result, so the constant is
#       2 max(measured, 0) = 0: out_snake gets no allowance beyond 2 e_acc and its fp16 rounding
#   delta_tanh: max |conv_out - tanh64(y_gpu)|, y_gpu from the same padded weights through zmi_dac_conv(out_f32)
#       measured 5.545e-8 (c_in 96; 5.362e-8 at c_in 32), about one fp32 ulp of a value in [0.5, 1)
# Required: delta_sin <= 2^-14, delta_tanh <= 2^-20 (the kernel's "far below fp16 rounding" claim): both hold.
DELTA_SIN = 0.0
DELTA_TANH = 2 * 5.545e-8
DELTA_SIN_MAX = 2.0 ** -14
DELTA_TANH_MAX = 2.0 ** -20

# zmi_dac_conv "same" convs (c_in, c_out, taps, dil): in_off = -dil (taps - 1) / 2, n_out = t_in = t_out = T
SAME_SHAPES = (
    (32, 32, 7, 1),     # one 32-channel tile
    (64, 96, 7, 3),     # WM 3
    (96, 128, 7, 9),    # WM 4, c_in not a multiple of 64
    (64, 160, 7, 1),    # five WM-1 tiles
    (64, 128, 3, 1),    # the encoder's k3
    (64, 64, 7, 10),    # span 60, the largest k7 span the staged form takes
    (32, 64, 3, 32),    # span 64, exactly the halo buffer
    (32, 64, 7, 11),    # span 66: the tap-major ring (conv_kernel HALO = false), never run by the model
    (64, 64, 1, 0),     # 1x1: staged CG 2
    (96, 96, 1, 0),     # 1x1: staged CG 3 at WM 3
    (96, 128, 1, 0),    # 1x1: staged CG 3 at WM 4
    (192, 128, 1, 0),   # 1x1: staged CG 2, three stages
    (160, 64, 1, 0),    # 1x1: unstaged fallback (c_in neither a multiple of 64 nor of 96)
    (32, 64, 1, 0),     # 1x1: unstaged fallback, one channel step
)
LENGTHS = (1, 129, 513)
EDGE_LENGTHS = (15, 16, 17, 127, 128, 255, 256, 257, 511, 512)  # the 128 / 256 / 512-row tile edges
EDGE_SHAPES = ((32, 32, 7, 1), (64, 64, 1, 0))                  # the first k7 and the first 1x1 shape
EPILOGUE_SHAPES = ((32, 32, 7, 1), (64, 64, 1, 0))              # run every epilogue combination
EPILOGUES = (("f32",), ("raw", "f32"), ("snake", "f32"), ("skip", "raw", "snake", "f32"), ("skip", "snake"))
DEFAULT_EPILOGUE = ("raw", "snake", "f32")

# (ZMI_OPT_DAC_WIDE, ZMI_OPT_DAC_STAGE, ZMI_OPT_DAC_STAGE_MIN) as test_dac_wide_time_tiles_bit_identical; None = the
# library's defaults. The first form is the one compared with fp64, every other must give its bits.
FORMS = ((0, 0, 256), (2, 0, 256), (1, 7, 1), (1, 15, 1), (1, 23, 1), None)

CONV_T_SHAPES = ((64, 32, 2, 1), (128, 64, 4, 2), (64, 64, 8, 4), (96, 96, 8, 4), (32, 32, 3, 2))  # ci, co, s, pad
CONV_T_LENGTHS = (1, 2, 16, 33, 129, 257)


def lengths_of(shape):
    return LENGTHS + (EDGE_LENGTHS if shape in EDGE_SHAPES else ())


def epilogues_of(shape):
    return EPILOGUES if shape in EPILOGUE_SHAPES else (DEFAULT_EPILOGUE,)


# ------------------------------------------------------------------------------------------------ inputs
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def f16_values(shape, g, scale=1.0):
    """Normal draws rounded to fp16, widened to float64."""
    return (torch.randn(shape, generator=g) * scale).half().double()


def conv_inputs(c_in, c_out, taps, t_in, t_skip, *key):
    """x [t_in][c_in], w [c_out][c_in][taps] scaled 1 / sqrt(taps c_in) (outputs O(1)), skip [t_skip][c_out]: fp16
    values; bias [c_out] and alpha [c_out] in [0.5, 2]: fp32 values. All float64."""
    g = _gen(c_in, c_out, taps, t_in, t_skip, *key)
    return dict(x=f16_values((t_in, c_in), g), w=f16_values((c_out, c_in, taps), g, 1.0 / math.sqrt(taps * c_in)),
                bias=(0.5 * torch.randn(c_out, generator=g)).float().double(),
                alpha=(0.5 + 1.5 * torch.rand(c_out, generator=g)).float().double(),
                skip=f16_values((t_skip, c_out), g))


def conv_t_inputs(c_in, c_out, stride, t_in, *key):
    """As conv_inputs for ConvTranspose1d(c_in, c_out, k = 2 stride): w [c_in][c_out][2 stride]; every output sums
    2 c_in terms."""
    g = _gen(c_in, c_out, stride, t_in, *key)
    return dict(x=f16_values((t_in, c_in), g), w=f16_values((c_in, c_out, 2 * stride), g, 1.0 / math.sqrt(2 * c_in)),
                bias=(0.5 * torch.randn(c_out, generator=g)).float().double(),
                alpha=(0.5 + 1.5 * torch.rand(c_out, generator=g)).float().double())


# ------------------------------------------------------------------------------------------------ fp64 references
def snake64(y, alpha):
    """Snake over channels-last y [T][C] with alpha [C], oracle/dac_cpu.snake in float64."""
    return _snake(y.double().t()[None], alpha.double().view(1, -1, 1))[0].t()


def tanh64(y):
    return torch.tanh(y.double())


def ref_conv_same(x, w, bias, dil):
    """Conv1d(dilation = dil, padding = dil (taps - 1) / 2) on x [T][ci] -> [T][co]."""
    taps = w.shape[2]
    return F.conv1d(x.t()[None], w, bias, dilation=max(dil, 1), padding=max(dil, 1) * (taps - 1) // 2)[0].t()


def ref_conv(x, w, bias, tap_step, in_off, n_out):
    """y[q][co] = bias[co] + sum_tap sum_ci w[co][ci][tap] x[q + in_off + tap tap_step][ci] for q < n_out, rows outside
    x reading as zero: conv1d(dilation = tap_step) over x zero-padded on both sides (tap_step >= 0)."""
    t_in, taps = x.shape[0], w.shape[2]
    step = tap_step if taps > 1 else 1
    assert step >= 1
    hi = n_out - 1 + in_off + (taps - 1) * step  # last input row touched
    left, right = max(0, -in_off), max(0, hi - (t_in - 1))
    y = F.conv1d(F.pad(x.t()[None], (left, right)), w, bias, dilation=step)[0].t()
    return y[in_off + left: in_off + left + n_out]


def ref_conv_t(x, wt, bias, stride, pad):
    """ConvTranspose1d(k = 2 stride, stride, padding = pad) on x [t][ci] with wt [ci][co][2 stride] -> [stride t][co]
    (output_padding = 2 pad - stride makes the length stride t)."""
    y = F.conv_transpose1d(x.t()[None], wt, bias, stride=stride, padding=pad, output_padding=2 * pad - stride)[0].t()
    assert y.shape[0] == stride * x.shape[0]
    return y


def ref_strided(x, w, bias, stride, pad):
    """Conv1d(k = 2 stride, stride, padding = pad) on x [t][c] with w [co][c][2 stride] -> [t / stride][co]."""
    return F.conv1d(x.t()[None], w, bias, stride=stride, padding=pad)[0].t()


# ------------------------------------------------------------------------------------------------ packed-layout emulation
def unpack_tap(packed, c_in, c_out, taps, tap, base=0):
    """W[tap] as [c_out][c_in] float64, read from the packed halfs at the documented index: 1x1 convs [co][ci];
    otherwise channel-blocked [tap][ci / 32][co][32] (include/zonos_hip.h)."""
    flat = packed.reshape(-1).double()
    co = torch.arange(c_out)[:, None]
    ci = torch.arange(c_in)[None, :]
    idx = co * c_in + ci if taps == 1 else ((tap * (c_in // 32) + ci // 32) * c_out + co) * 32 + ci % 32
    return flat[base + idx]


def emulate_conv(packed, x, bias, c_out, taps, tap_step, in_off, n_out, out_stride=1, out_phase=0, t_out=None,
                 skip=None, nphase=1, phase_pad=0):
    """The header's formula in float64 over the packed weights:
        out[t_out][co] = bias + sum_tap sum_ci W[tap][co][ci] x[t_in][ci] (+ skip[t_out][co]),
        t_in = q + in_off + tap tap_step (zero outside x), t_out = q out_stride + out_phase, q in [0, n_out);
    nphase > 1 (zmi_dac_conv_t): phase rho reads its own weights at rho taps c_out c_in halfs, in_off =
    (rho + phase_pad) / out_stride, out_phase = rho. Returns [t_out][c_out], NaN in the rows no q writes."""
    t_in, c_in = x.shape
    t_out = n_out if t_out is None else t_out
    out = torch.full((t_out, c_out), float("nan"), dtype=torch.float64)
    q = torch.arange(n_out)
    for rho in range(nphase):
        off, phase = ((rho + phase_pad) // out_stride, rho) if nphase > 1 else (in_off, out_phase)
        y = bias.double()[None, :].repeat(n_out, 1)
        for tap in range(taps):
            rows = q + off + tap * tap_step
            ok = (rows >= 0) & (rows < t_in)
            xg = torch.zeros(n_out, c_in, dtype=torch.float64)
            xg[ok] = x.double()[rows[ok]]
            y += xg @ unpack_tap(packed, c_in, c_out, taps, tap, rho * taps * c_out * c_in).t()
        rows_out = q * out_stride + phase
        assert n_out == 0 or int(rows_out[-1]) < t_out
        if skip is not None:
            y += skip.double()[rows_out]
        out[rows_out] = y
    return out


# ------------------------------------------------------------------------------------------------ the error bound
def e_acc(M, K):
    """Bound of the fp32 accumulation error of one output: M = sum |w| |x| + |bias| (+ |skip|) from the same conv on
    absolute values, K = taps c_in terms. fp16 x fp16 products are exact in fp32, (K - 1) u M bounds fp32 accumulation
    in any order (plus the bias and skip adds: K + 1); the factor 2 is slack, because the MFMA's internal add order
    and rounding are not documented as one IEEE add per term."""
    return 2.0 * (K + 1) * U32 * M


def bound(kind, ref, M, K, alpha=None):
    """Allowed |got - ref| per element. kind: 'f32' (out_f32), 'raw' (fp16 out_raw), 'snake' (fp16 out_snake, ref =
    snake64 of the fp64 conv; Snake's slope 1 + sin(2 a y) is at most 2), 'tanh' (zmi_dac_conv_out, slope <= 1)."""
    e = e_acc(M, K)
    if kind == "f32":
        return e
    if kind == "raw":
        return e + U16 * ref.abs() + SUB16
    if kind == "snake":
        return 2 * e + U16 * ref.abs() + SUB16 + 2 * DELTA_SIN / (alpha + 1e-9)
    if kind == "tanh":
        return e + DELTA_TANH
    raise ValueError(kind)


def worst_ratio(got, ref, bnd):
    """max |got - ref| / bound (NaN-safe: a NaN anywhere gives inf); the check passes when this is <= 1."""
    r = (got.double() - ref).abs() / bnd
    return float("inf") if not torch.isfinite(r).all() else float(r.max()) if r.numel() else 0.0


SMALL = 2.0 ** -14  # below this fp16 is subnormal


def raw_matches_f32(raw, f32):
    """out_raw (fp16) against out_f32.half() of the same launch: bit-identical, except that elements with
    |y| < 2^-14 may differ by 2^-24 (one subnormal step). Returns (elements breaking that rule, fraction of
    elements with |y| < 2^-14); a case fails if the fraction exceeds 0.1 %."""
    want = f32.half()
    small = f32.abs() < SMALL
    same = raw.view(torch.int16) == want.view(torch.int16)
    near = (raw.double() - want.double()).abs() <= 2.0 ** -24
    bad = ~(same | (small & near))
    return int(bad.sum()), float(small.double().mean()) if f32.numel() else 0.0


def delta_sin_of(z_gpu, y_gpu, alpha):
    """The Snake epilogue's own error in units of the sin^2 term's argument error (the issue's definition):
    max (|z_gpu - snake64(y_gpu)| - 2^-11 |z| - 2^-25) alpha / 2, with y_gpu the fp32 value the same launch wrote."""
    z = snake64(y_gpu, alpha)
    d = ((z_gpu.double() - z).abs() - U16 * z.abs() - SUB16) * alpha.double()[None, :] / 2
    return float(d.max())


# ------------------------------------------------------------------------------------------------ VQ
def near_tie_violations(got, ref, margins, eps):
    """Per frame, the first codebook whose code differs must be a near-tie of the oracle (margin < eps); later
    codebooks quantize a residual that already differs (tests/test_dac_encode.py). got, ref, margins: [9][T]."""
    bad = []
    for t in range(ref.shape[1]):
        diff = (got[:, t] != ref[:, t]).nonzero()
        if diff.numel() and margins[int(diff[0]), t] >= eps:
            bad.append((int(diff[0]), t, float(margins[int(diff[0]), t])))
    return bad
