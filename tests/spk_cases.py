"""Cases, fp64 references and derived bounds shared by the CPU and GPU probes of the speaker encoder's kernels
(csrc/zmi_spk.hip: spk_conv_kernel<2 | 4>, spk_stem_kernel, the SimAM reduce / finish / apply kernels). CPU only; the
library is not imported here. U32, U16, SUB16, e_acc and worst_ratio are those of tests/dac_cases.py.

Every input is seeded and exactly representable in what the kernel reads: activations, weights and the residual are
fp16 values, scale and shift fp32 values, all held as float64. Activations are channels-last [H][W][C].

CONV AND STEM. conv_ref is F.conv2d in float64 on the unpacked [Co][Ci][k][k] weights. With acc64 the sum, M the same
conv on |x| and |w|, K = k^2 Ci, z64 = acc64 scale + shift and y64 = relu(z64) or z64, an element may differ by

    |got - y64| <= |scale| e_acc(M, K) + 2 U32 (|acc64 scale| + |shift|) + U16 |y64| + SUB16

the MFMA accumulation bound of the DAC probe carried through the scale, two fp32 roundings of the epilogue (the
product and the sum, fused or not), then the fp16 store. ReLU has slope <= 1. Nothing in it is measured on a kernel.
The `integers` and `border` regimes are exact in fp32 instead and are compared bit for bit. Where the conv writes psum
(per 8 x 16 output tile and channel, the fp32 sum of the values it STORED), |psum - sum_tile stored| is at most
128 U32 sum_tile |stored|: at most 127 additions of at most 128 terms, in any order.

  integers  x in [-3, 3], asymmetric w in [-2, 2], scale 1, shift 0: every sum is below 2^24, bit equality; psum exact
  ordinary  x ~ N(0,1), w ~ N(0,1) / sqrt(K), scale in [0.8, 1.2] with both signs, shift ~ N(0,1); with and without ReLU
  cancel    x constant over the channels of a position (a sign and a magnitude per position); w is one magnitude per
            output channel times (1 + j / 64), j in -2 .. 2, with the sign + for the first half of the input channels
            and - for the second, swapped on odd taps: |acc64| < 2^-6 M, shift 0, so the bound is e_acc and next to no
            fp16 rounding. The sign is constant over most 32-channel K steps (all of them where Ci / 32 is even), so
            one step of one tap is a large term: dropping it, or reading it twice, cannot hide behind the cancellation
            (under a sign that alternated from channel to channel, a step's own sum would cancel, too).
  range     ordinary x and w; scale (and, on odd channels, shift) per channel such that the channel's largest |z64| is a
            target that sweeps 2^-17 .. 6e4 geometrically over the channels: fp16 subnormals, the ordinary range, the
            top. The builder asserts |y64| (1 + 2^-10) + bound < 65504.
  border    x non-zero only in the outermost ring of positions, w only in the outer taps (k = 3: all but the centre;
            a 1 x 1 conv keeps its one tap): integers, bit equality. Padding and halo offsets are all there is.

SIMAM TAIL. simam_ref evaluates, in float64 from the fp16 x and residual, over the P = H W positions of a channel:
m = mean x, d = x - m, S = sum d^2, v = S / (P - 1), den = 4 (v + 1e-4), q = d^2 / den, e = q + 0.5,
sigma = sigmoid(e), y64 = relu(x sigma + res). simam_bound is first-order error propagation with fp32 unit roundoff:

    dm   = (n_s + 1) U32 mean|x|
    dd   = dm + U32 |d|
    dd2  = 2 |d| dd + dd^2 + U32 d^2
    dS   = (n_s + 1) U32 S + sum_positions dd2
    dv   = dS / (P - 1)
    dden = 4 dv + 3 U32 den
    dq   = dd2 / den + q dden / den + U32 q
    de   = dq + U32 e
    dsig = sigma'(max(e - de, 0.5)) de + 4 U32 sigma      (sigma' decreases for e >= 0.5, e itself is >= 0.5)
    B    = |x| dsig + 2 U32 (|x sigma| + |res|)
    allowed = B + U16 |y64| + SUB16

n_s is the longest chain of additions the kernels' documented order gives one sum (zmi_spk.hip "Launches, every sum
in a fixed order", "8 row groups per channel"). A reduce workgroup takes a chunk of 128 positions with
rows = 256 / (C / 8) position rows; a thread adds ceil(128 / rows) terms, a column of s_red adds `rows` partial sums,
the finish kernel adds ceil(n_rows / 8) chunk rows per row group and then the 8 groups:

    n_s = ceil(128 / rows) + rows + ceil(n_rows / 8) + 8,        n_rows = ceil(P / 128)

e.g. C = 32: 2 + 64 + 1 + 8 = 75 for P <= 1024; C = 8: 1 + 256; C = 2048: 128 + 1; the long case (C = 64, 257
chunks): 4 + 32 + 33 + 8 = 77. With the conv's tile sums the mean's chain is the 128 positions of a tile plus the
finish, 128 + ceil(n_psum / 8) + 8, while S still comes from the reduce kernels; simam_n_s returns the larger of the
two.

A case is [P][C] with the six regimes dealt round-robin over the channels (channel c has REGIMES[c % 6]):

  ordinary  N(0,1)
  offset64  64 + j / 16, j uniform in 0 .. 3: the mean is not dyadic, |mean| ~ 1000 deviations
  offset16  16 + j / 64
  const     1.5 everywhere: sum and mean exact, d = 0, v = 0, the output relu(1.5 sigmoid(0.5) + res); 1e-4 stands alone
  outlier   0.01 N(0,1) with position P // 3 at 1000. One position carries all of S, so its e is (P - 1)^2 / (4 P) + 0.5
            to within 1e-4: below P / 4 whatever the outlier's size. From P = 129 on 1 + expf(-e) rounds to 1, in the
            long case (e = 8200) expf(-e) is 0
  tiny      2e-3 N(0,1): v ~ 4e-6 << 1e-4, the lambda term dominates den (3e-3 has variance 9e-6, and the sample
            variance of some channel then passes the 1e-5 that the regime is to stay below)

and two residuals: `rand` ~ N(0,1), and `cancel` = fp16(-0.62 x), which puts x sigma + res around 0 and the ReLU edge,
where the result's own ulp gives no cover. On the psum path x is the STORED output of a C -> C 3 x 3 conv of the library
(or of its fp32 emulation, on the CPU) and the reference starts from those stored values. That conv is diagonal
(psum_conv): a channel reads its own channel only, so a channel keeps its regime; const and the offsets pass through an
identity (centre tap 1, scale 1, shift 0: the stored x is the crafted one exactly), the others through a random
3 x 3 filter of their own with a scale in [0.8, 1.2] (ordinary: and a shift).

EMULATIONS AND MUTANTS (tests/test_spk_cases_cpu.py) restate the kernels' arithmetic in float32 and in their order:
emu_conv per K step of 32 channels, tap by tap, scale and shift as two roundings, fp16, and the tile sums; emu_simam
with chunked sums, the 8 row groups, the two-pass variance and the fp16 store. The condition on the inputs is that these
pass every case; it involves no GPU.
"""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

from tests.dac_cases import SUB16, U16, U32, e_acc, worst_ratio  # noqa: F401  (re-exported)

F64 = torch.float64
TH, TW, CHUNK = 8, 16, 128        # the conv's output tile, SimAM's positions per workgroup
LAM = 1e-4
FP16_MAX = 65504.0

# (Ci, Co, k, stride)
CONV_SHAPES = (
    (128, 128, 3, 1),   # 4 K steps, 2 column blocks (NB = 4)
    (64, 128, 3, 2),    # the stage change: conv1 ..
    (64, 128, 1, 2),    # .. and the downsample
    (96, 96, 3, 1),     # NB = 2 with 3 column blocks, odd K-step count
    (256, 512, 3, 2),   # 8 K steps, 8 column blocks, the 71 KiB LDS form
    (256, 512, 1, 2),
    (512, 512, 3, 1),   # 16 K steps: the model's largest conv
)
# one partial tile; 2 x 2 tiles partial on both edges; 3 x 3 tiles; all odd under stride 2
CONV_HW = ((3, 5), (9, 17), (17, 33))
CONV_REGIMES = ("integers", "ordinary", "ordinary_relu", "cancel", "range", "border")
LARGE_REGIMES = ("integers", "ordinary", "ordinary_relu")
EXACT = ("integers", "border")

STEM_CO = 64
STEM_HW = ((24, 37), (3, 2))
STEM_REGIMES = ("integers", "ordinary", "range")

REGIMES = ("ordinary", "offset64", "offset16", "const", "outlier", "tiny")
RESIDUALS = ("rand", "cancel")
SIMAM_SHAPES = (
    (1, 2, 32),       # P = 2: the divisor P - 1 is 1
    (1, 128, 32),     # exactly one chunk
    (3, 43, 64),      # P = 129: one position into a second chunk
    (5, 205, 128),    # P = 1025: 9 chunks, finish group 0 adds two rows
    (3, 43, 8),       # rows = 256: the 256 x 8 edge of s_red
    (3, 43, 2048),    # rows = 1: the 1 x 2048 edge of s_red
    (3, 43, 256),
    (3, 43, 512),
    (80, 410, 64),    # long: 257 chunks and 260 conv tiles, the finish loop runs 33 deep
)
PSUM_EXTRA = ((20, 60, 128),)  # 12 tile rows
PSUM_SHAPES = tuple(s for s in SIMAM_SHAPES if s[2] >= 32) + PSUM_EXTRA


def conv_hw_of(shape):
    return CONV_HW[:2] if shape == (512, 512, 3, 1) else CONV_HW


def conv_regimes_of(shape):
    return LARGE_REGIMES if shape[0] >= 256 else CONV_REGIMES


def out_dim(n, k, stride):
    return (n + 2 * (k // 2) - k) // stride + 1


def n_tiles(H, W, k, stride):
    return math.ceil(out_dim(H, k, stride) / TH) * math.ceil(out_dim(W, k, stride) / TW)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _h(t):
    """Rounded to fp16, as float64."""
    return t.half().to(F64)


def _f(t):
    """Rounded to fp32, as float64."""
    return t.float().to(F64)


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


# ------------------------------------------------------------------------------------------------ conv: reference
class ConvRef:
    """acc64, M, K, y64 and the allowed error of one conv."""

    def __init__(self, x, w, scale, shift, stride, relu):
        k, ci = w.shape[-1], w.shape[1]
        xin = x.permute(2, 0, 1)[None]
        self.acc = F.conv2d(xin, w, None, stride, k // 2)[0].permute(1, 2, 0)
        self.M = F.conv2d(xin.abs(), w.abs(), None, stride, k // 2)[0].permute(1, 2, 0)
        self.K = k * k * ci
        z = self.acc * scale + shift
        self.y = torch.relu(z) if relu else z
        self.bound = (scale.abs() * e_acc(self.M, self.K) + 2 * U32 * ((self.acc * scale).abs() + shift.abs())
                      + U16 * self.y.abs() + SUB16)


def conv_ref(x, w, scale, shift, stride, relu):
    return ConvRef(x, w, scale, shift, stride, relu)


def tile_sums(y):
    """Per 8 x 16 tile (row-major over the tile grid) and channel: the sums of y [Ho][Wo][Co] -> [tiles][Co], in the
    dtype of y."""
    ho, wo, co = y.shape
    p = F.pad(y, (0, 0, 0, -wo % TW, 0, -ho % TH))
    return p.reshape(p.shape[0] // TH, TH, p.shape[1] // TW, TW, co).sum((1, 3)).reshape(-1, co)


def psum_bound(stored):
    """Allowed |psum - tile_sums(stored)| for the fp16 values a launch stored (float64 [Ho][Wo][Co])."""
    return 128 * U32 * tile_sums(stored.abs())


# ------------------------------------------------------------------------------------------------ conv: cases
class ConvCase:
    def __init__(self, x, w, scale, shift, stride, relu, exact):
        self.x, self.w, self.scale, self.shift = x, w, scale, shift
        self.stride, self.relu, self.exact = stride, relu, exact
        self.ref = conv_ref(x, w, scale, shift, stride, relu)
        y = self.ref.y
        assert bool((y.abs() * (1 + 2.0 ** -10) + self.ref.bound < FP16_MAX).all()), "the case overflows fp16"
        assert torch.equal(_h(x), x) and torch.equal(_h(w), w), "activations and weights are fp16 values"
        assert torch.equal(_f(scale), scale) and torch.equal(_f(shift), shift), "scale and shift are fp32 values"


def _ordinary_xw(H, W, ci, co, k, g):
    return _h(torch.randn(H, W, ci, generator=g)), _h(torch.randn(co, ci, k, k, generator=g) / math.sqrt(k * k * ci))


def _range_affine(acc, co, g):
    """Per-channel scale and shift (fp32 values) such that channel c's largest |acc scale + shift| is at most a
    target sweeping 2^-17 .. 6e4 geometrically; odd channels give half of it to a shift of either sign."""
    lo, hi = math.log2(2.0 ** -17), math.log2(6.0e4)
    target = torch.exp2(lo + (hi - lo) * torch.arange(co, dtype=F64) / (co - 1))
    amax = acc.abs().amax((0, 1)).clamp_min(2.0 ** -20)
    odd = (torch.arange(co) % 2 == 1)
    sign = torch.where(torch.rand(co, generator=g) < 0.5, -1.0, 1.0).to(F64)
    scale = torch.where(odd, 0.5, 1.0) * target / amax * sign
    shift = torch.where(odd, 0.5 * target, torch.zeros_like(target)) * torch.where(torch.arange(co) % 4 == 1, -1.0, 1.0)
    return _f(scale * (1 - 2.0 ** -20)), _f(shift * (1 - 2.0 ** -20))  # the fp32 rounding cannot pass the target


@functools.lru_cache(maxsize=None)
def conv_case(shape, hw, regime):
    (ci, co, k, stride), (H, W) = shape, hw
    g = _gen(ci, co, k, stride, H, W, CONV_REGIMES.index(regime))
    one, zero = torch.ones(co, dtype=F64), torch.zeros(co, dtype=F64)
    if regime == "integers":
        x, w = _ints((H, W, ci), -3, 3, g), _ints((co, ci, k, k), -2, 2, g)
        assert k == 1 or not torch.equal(w, w.flip(2, 3))
        return ConvCase(x, w, one, zero, stride, False, True)
    if regime in ("ordinary", "ordinary_relu"):
        x, w = _ordinary_xw(H, W, ci, co, k, g)
        sign = torch.where(torch.arange(co) % 3 == 1, -1.0, 1.0)
        scale = _f((0.8 + 0.4 * torch.rand(co, generator=g)) * sign)
        return ConvCase(x, w, scale, _f(torch.randn(co, generator=g)), stride, regime == "ordinary_relu", False)
    if regime == "cancel":
        mag = 0.5 + torch.randn(H, W, generator=g).abs()
        sgn = torch.where(torch.rand(H, W, generator=g) < 0.5, -1.0, 1.0)
        x = _h((mag * sgn)[:, :, None].expand(H, W, ci).contiguous())
        a = (0.5 + torch.rand(co, generator=g)) / math.sqrt(k * k * ci)
        j = torch.randint(-2, 3, (co, ci, k, k), generator=g)
        half = torch.where(torch.arange(ci) < ci // 2, 1.0, -1.0)[None, :, None, None]
        tap = torch.where(torch.arange(k * k) % 2 == 0, 1.0, -1.0).reshape(1, 1, k, k)
        w = _h(a[:, None, None, None] * (1 + j / 64.0) * half * tap)
        sign = torch.where(torch.arange(co) % 3 == 1, -1.0, 1.0)
        return ConvCase(x, w, _f((0.8 + 0.4 * torch.rand(co, generator=g)) * sign), zero, stride, False, False)
    if regime == "range":
        x, w = _ordinary_xw(H, W, ci, co, k, g)
        acc = F.conv2d(x.permute(2, 0, 1)[None], w, None, stride, k // 2)[0].permute(1, 2, 0)
        scale, shift = _range_affine(acc, co, g)
        return ConvCase(x, w, scale, shift, stride, False, False)
    if regime == "border":
        x = _ints((H, W, ci), 1, 3, g) * torch.where(torch.rand(H, W, ci, generator=g) < 0.5, -1.0, 1.0)
        ring = torch.zeros(H, W, dtype=torch.bool)
        ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
        x = torch.where(ring[:, :, None], x, torch.zeros_like(x))
        w = _ints((co, ci, k, k), -2, 2, g)
        if k == 3:
            w[:, :, 1, 1] = 0
            assert not torch.equal(w, w.flip(2, 3))
        return ConvCase(x, w, one, zero, stride, False, True)
    raise ValueError(regime)


@functools.lru_cache(maxsize=None)
def stem_case(hw, regime):
    """The stem as a conv with Ci = 1 (x [H][W][1], w [Co][1][3][3]), always with ReLU."""
    (H, W), co = hw, STEM_CO
    g = _gen(1, co, H, W, STEM_REGIMES.index(regime))
    if regime == "integers":
        x, w = _ints((H, W, 1), -3, 3, g), _ints((co, 1, 3, 3), -2, 2, g)
        return ConvCase(x, w, torch.ones(co, dtype=F64), torch.zeros(co, dtype=F64), 1, True, True)
    x, w = _ordinary_xw(H, W, 1, co, 3, g)
    if regime == "ordinary":
        sign = torch.where(torch.arange(co) % 3 == 1, -1.0, 1.0)
        return ConvCase(x, w, _f((0.8 + 0.4 * torch.rand(co, generator=g)) * sign), _f(torch.randn(co, generator=g)), 1,
                        True, False)
    acc = F.conv2d(x.permute(2, 0, 1)[None], w, None, 1, 1)[0].permute(1, 2, 0)
    scale, shift = _range_affine(acc, co, g)
    return ConvCase(x, w, scale, shift, 1, True, False)


# ------------------------------------------------------------------------------------------------ conv: fp32 emulation
def emu_conv(c, flip_taps=False, clamp=False, drop=None, psum_f32=False):
    """The conv kernel's arithmetic in float32: per K step of 32 channels (of all Ci for the stem), tap by tap, then
    acc * scale and + shift as two roundings, ReLU, fp16. -> (stored fp16 [Ho][Wo][Co], psum fp32 [tiles][Co]: per wave
    its two tile rows added per column, the 16 columns in a tree, the four waves in order).
    Mutants: flip_taps (w[k - 1 - ky][k - 1 - kx]), clamp (edge-replicated padding), drop = (K step, tap) left out,
    psum_f32 (the tile sums taken before the fp16 rounding)."""
    x, w = c.x.float(), (c.w.flip(2, 3) if flip_taps else c.w).float()
    (H, W, ci), (co, _, k, _), s = x.shape, w.shape, c.stride
    ho, wo, pad = out_dim(H, k, s), out_dim(W, k, s), k // 2
    xp = x.permute(2, 0, 1)[None]
    xp = F.pad(xp, (pad,) * 4, mode="replicate" if clamp else "constant")[0].permute(1, 2, 0) if pad else x
    acc = torch.zeros(ho, wo, co)
    step = min(32, ci)
    for cs in range(ci // step):
        for tap in range(k * k):
            if drop == (cs, tap):
                continue
            ky, kx = divmod(tap, k)
            xs = xp[ky: ky + s * (ho - 1) + 1: s, kx: kx + s * (wo - 1) + 1: s, cs * step:(cs + 1) * step]
            acc = acc + xs @ w[:, cs * step:(cs + 1) * step, ky, kx].t()
    y = acc * c.scale.float()
    y = y + c.shift.float()
    if c.relu:
        y = torch.relu(y)
    stored = y.half()
    v = y if psum_f32 else stored.float()
    p = F.pad(v, (0, 0, 0, -wo % TW, 0, -ho % TH))
    p = p.reshape(p.shape[0] // TH, 4, 2, p.shape[1] // TW, TW, co)    # [tile row][wave][j][tile col][column][co]
    t = p[:, :, 0] + p[:, :, 1]
    while t.shape[3] > 1:
        t = t[:, :, :, 0::2] + t[:, :, :, 1::2]
    t = t[:, :, :, 0]
    psum = ((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]
    return stored, psum.reshape(-1, co)


# ------------------------------------------------------------------------------------------------ SimAM: reference
class SimamRef:
    def __init__(self, x, res):
        """x, res: [P][C] float64 (fp16 values)."""
        self.x, self.res, self.P = x, res, x.shape[0]
        self.m = x.mean(0)
        self.d = x - self.m
        self.S = (self.d * self.d).sum(0)
        self.v = self.S / (self.P - 1)
        self.den = 4 * (self.v + LAM)
        self.q = self.d * self.d / self.den
        self.e = self.q + 0.5
        self.sig = torch.sigmoid(self.e)
        self.y = torch.relu(x * self.sig + res)


def simam_ref(x, res):
    return SimamRef(x, res)


def simam_n_s(P, C, n_psum=0):
    rows = 256 // (C // 8)
    n = math.ceil(CHUNK / rows) + rows + math.ceil(math.ceil(P / CHUNK) / 8) + 8
    return max(n, 128 + math.ceil(n_psum / 8) + 8) if n_psum else n


def simam_bound(r, n_s):
    """Allowed |got - r.y| per element (the module docstring's propagation)."""
    x, d = r.x, r.d.abs()
    dm = (n_s + 1) * U32 * x.abs().mean(0)
    dd = dm + U32 * d
    dd2 = 2 * d * dd + dd * dd + U32 * d * d
    dS = (n_s + 1) * U32 * r.S + dd2.sum(0)
    dv = dS / (r.P - 1)
    dden = 4 * dv + 3 * U32 * r.den
    dq = dd2 / r.den + r.q * dden / r.den + U32 * r.q
    de = dq + U32 * r.e
    sl = torch.sigmoid((r.e - de).clamp_min(0.5))
    dsig = sl * (1 - sl) * de + 4 * U32 * r.sig
    B = x.abs() * dsig + 2 * U32 * ((x * r.sig).abs() + r.res.abs())
    return B + U16 * r.y.abs() + SUB16


def regime_max(ratio):
    """ratio [P][C] -> {regime: its channels' maximum} (channel c has REGIMES[c % 6]; NaN counts as inf)."""
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, math.inf))
    return {n: float(ratio[:, i::len(REGIMES)].max()) for i, n in enumerate(REGIMES)}


def simam_ratio(got, r, n_s):
    return (got.to(F64).reshape(r.y.shape) - r.y).abs() / simam_bound(r, n_s)


# ------------------------------------------------------------------------------------------------ SimAM: cases
def _regime_column(name, P, g):
    if name == "ordinary":
        return torch.randn(P, generator=g)
    if name == "offset64":
        return 64 + torch.randint(0, 4, (P,), generator=g) / 16.0
    if name == "offset16":
        return 16 + torch.randint(0, 4, (P,), generator=g) / 64.0
    if name == "const":
        return torch.full((P,), 1.5)
    if name == "outlier":
        o = 0.01 * torch.randn(P, generator=g)
        o[P // 3] = 1000.0
        return o
    if name == "tiny":
        return 2e-3 * torch.randn(P, generator=g)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def simam_x(shape):
    """[P][C] fp16 values (float64), channel c of regime REGIMES[c % 6]."""
    H, W, C = shape
    g = _gen(H, W, C, 11)
    return _h(torch.stack([_regime_column(REGIMES[c % len(REGIMES)], H * W, g) for c in range(C)], 1))


def residual(kind, x, shape):
    """The residual [P][C] for the x SimAM reads (on the psum path: the conv's stored output)."""
    if kind == "cancel":
        return _h(-0.62 * x.float())
    H, W, C = shape
    return _h(torch.randn(H * W, C, generator=_gen(H, W, C, 12)))


def psum_conv(shape):
    """The diagonal C -> C 3 x 3 conv ahead of SimAM on the psum path, as a ConvCase-like set of inputs (no reference:
    that is the caller's, from the stored values): channel c reads channel c alone; const and the offsets through an
    identity, the others through a random filter, scale in [0.8, 1.2], ordinary with a shift. Built on demand and in
    float32 (fp16 values): at C = 2048 the weights are 38 M numbers."""
    H, W, C = shape
    g = _gen(H, W, C, 13)
    x = simam_x(shape).reshape(H, W, C)
    w = torch.zeros(C, C, 3, 3)
    scale, shift = torch.ones(C, dtype=F64), torch.zeros(C, dtype=F64)
    for c in range(C):
        name = REGIMES[c % len(REGIMES)]
        if name in ("const", "offset64", "offset16"):
            w[c, c, 1, 1] = 1.0
        else:
            w[c, c] = _h(torch.randn(3, 3, generator=g) / 3.0)
            scale[c] = _f(0.8 + 0.4 * torch.rand((), generator=g))
            if name == "ordinary":
                shift[c] = _f(0.1 * torch.randn((), generator=g))
    return PsumConv(x, w, scale, shift)


class PsumConv:
    stride, relu = 1, False

    def __init__(self, x, w, scale, shift):
        self.x, self.w, self.scale, self.shift = x, w, scale, shift


# ------------------------------------------------------------------------------------------------ SimAM: fp32 emulation
def _ordered_sum(t, C):
    """Column sums of t [P][C] float32 in the kernels' order: chunks of 128 positions; in a chunk thread row pr adds
    positions pr, pr + rows, .. in order, then the rows are added in order; the chunk rows go to 8 row groups (group g:
    rows g, g + 8, ..), added in order, and the groups are added in order."""
    P = t.shape[0]
    rows = min(256 // (C // 8), CHUNK)
    n = math.ceil(P / CHUNK)
    t = F.pad(t, (0, 0, 0, n * CHUNK - P)).reshape(n, CHUNK // rows, rows, C)
    a = torch.zeros(n, rows, C)
    for i in range(t.shape[1]):
        a = a + t[:, i]
    part = torch.zeros(n, C)
    for q in range(rows):
        part = part + a[:, q]
    return _finish(part)


def _finish(part):
    n, C = part.shape
    part = F.pad(part, (0, 0, 0, -n % 8)).reshape(-1, 8, C)
    grp = torch.zeros(8, C)
    for i in range(part.shape[0]):
        grp = grp + part[i]
    out = grp[0]
    for q in range(1, 8):
        out = out + grp[q]
    return out


def emu_simam(x, res, psum=None, mode="ok"):
    """The SimAM launches in float32 and in their order; x, res [P][C] (fp16 values), psum [rows][C] float32 or None.
    -> the stored fp16 [P][C]. Modes (mutants): onepass (v from sum x^2 - P m^2), meanh (the mean rounded to fp16),
    divP (S / P), nolam (no 1e-4), lam3 (1e-3), no4 (den = v + 1e-4)."""
    x32, r32 = x.float(), res.float()
    P, C = x32.shape
    Pf = torch.tensor(float(P))
    m = (_finish(psum.float()) if psum is not None else _ordered_sum(x32, C)) / Pf
    if mode == "meanh":
        m = m.half().float()
    d = x32 - m
    if mode == "onepass":
        S = _ordered_sum(x32 * x32, C) - Pf * (m * m)
    else:
        S = _ordered_sum(d * d, C)
    v = S / torch.tensor(float(P if mode == "divP" else P - 1))
    lam = torch.tensor({"nolam": 0.0, "lam3": 1e-3}.get(mode, 1e-4), dtype=torch.float32)
    den = (v + lam) if mode == "no4" else 4.0 * (v + lam)
    e = (d * d) / den + 0.5
    sg = 1.0 / (1.0 + torch.exp(-e))
    return torch.relu(x32 * sg + r32).half()
