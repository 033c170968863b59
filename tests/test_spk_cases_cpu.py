"""tests/spk_cases.py judged on the CPU: the fp64 references agree with F.conv2d in fp32 and with the restatement's
SimAM tail, every builder does what its name says, float32 emulations of the kernels' arithmetic in the kernels' order
meet every bound on every case (this is the condition on the inputs), and each mutant of that arithmetic misses on the
regime named for it. No GPU.

A SimAM mutant is judged on the channels of the named regime, at the worse of the two residual kinds: `rand` puts a
value of order 1 on every output, whose fp16 rounding (5e-4) covers what a wrong statistic does to a channel of 2e-3
values; `cancel` removes that cover, which is what it is for. No regime had to be changed for a mutant to be rejected.
Two builder properties were planned differently: `tiny` draws 2e-3 N(0,1) rather than 3e-3, whose variance of 9e-6 left
some channel's sample variance above 1e-5; and the largest e of `outlier` is (P - 1)^2 / (4 P) + 0.5 whatever the
outlier's size (one position carries all of S), so the planned 1e4 is out of reach below P = 40,000: asserted instead
are that value, that 1 + expf(-e) rounds to 1 from P = 129 on, and that expf(-e) is 0 in the long case.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import spk_cases as sc
from tests import spk_cpu
from tests.spk_cases import F64, REGIMES


def _ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------------------------------ the references themselves
@pytest.mark.parametrize("shape", [(128, 128, 3, 1), (64, 128, 3, 2), (64, 128, 1, 2)], ids=_ids)
def test_conv_ref_agrees_with_fp32_conv2d(shape):
    for regime in ("ordinary", "ordinary_relu"):
        c = sc.conv_case(shape, (9, 17), regime)
        k = c.w.shape[-1]
        y = F.conv2d(c.x.float().permute(2, 0, 1)[None], c.w.float(), None, c.stride, k // 2)[0].permute(1, 2, 0)
        y = y * c.scale.float() + c.shift.float()
        y = torch.relu(y) if c.relu else y
        worst = sc.worst_ratio(y, c.ref.y, c.ref.bound)
        print(f"F.conv2d fp32 {shape} {regime}: {worst:.3f}")
        assert worst <= 1.0
        assert c.ref.K == k * k * shape[0] and bool((c.ref.M >= c.ref.acc.abs()).all())


@pytest.mark.parametrize("shape", [(3, 43, 64), (5, 205, 128)], ids=_ids)
def test_simam_ref_agrees_with_the_restatement(shape):
    """spk_cpu.SpeakerCPU.simam_tail (fp32 statistics, fp16 store) on the ordinary channels, within the bound."""
    H, W, C = shape
    x = sc.simam_x(shape)
    res = sc.residual("rand", x, shape)
    cpu = spk_cpu.SpeakerCPU({}, {}, C, (1, 1, 1, 1), torch.float16)
    nchw = lambda t: t.float().reshape(H, W, C).permute(2, 0, 1)[None]  # noqa: E731
    got = cpu.simam_tail(nchw(x), nchw(res))[0].permute(1, 2, 0).reshape(H * W, C)
    worst = sc.regime_max(sc.simam_ratio(got, sc.simam_ref(x, res), sc.simam_n_s(H * W, C)))
    print(f"simam_tail {shape}: {worst}")
    assert worst["ordinary"] <= 1.0


def test_n_s_counts():
    assert sc.simam_n_s(129, 32) == 2 + 64 + 1 + 8
    assert sc.simam_n_s(129, 8) == 1 + 256 + 1 + 8
    assert sc.simam_n_s(129, 2048) == 128 + 1 + 1 + 8
    assert sc.simam_n_s(1025, 128) == 8 + 16 + 2 + 8
    assert sc.simam_n_s(32800, 64) == 4 + 32 + 33 + 8
    assert sc.simam_n_s(32800, 64, 260) == 128 + 33 + 8
    assert sc.n_tiles(80, 410, 3, 1) == 260 and sc.n_tiles(20, 60, 3, 1) == 12 and sc.n_tiles(17, 33, 3, 2) == 4


def test_tile_sums():
    y = torch.arange(9 * 17 * 2, dtype=F64).reshape(9, 17, 2)
    t = sc.tile_sums(y)
    assert t.shape == (4, 2)
    assert torch.equal(t[0], y[:8, :16].sum((0, 1))) and torch.equal(t[1], y[:8, 16:].sum((0, 1)))
    assert torch.equal(t[2], y[8:, :16].sum((0, 1))) and torch.equal(t[3], y[8:, 16:].sum((0, 1)))


# ------------------------------------------------------------------------------------------ the builders
@pytest.mark.parametrize("shape", sc.CONV_SHAPES, ids=_ids)
def test_conv_builders(shape):
    """cancel: |acc64| < 2^-6 M; range: subnormals and values above 3e4; integers and border: integer sums below 2^24;
    border: nothing but the ring and the outer taps. That no case overflows fp16 is asserted where a case is built."""
    for hw in sc.conv_hw_of(shape):
        for regime in sc.conv_regimes_of(shape):
            c = sc.conv_case(shape, hw, regime)
            y = c.ref.y
            assert bool(torch.isfinite(y).all()) and float(y.abs().max()) < sc.FP16_MAX
            if regime == "cancel":
                rel = float((c.ref.acc.abs() / c.ref.M).max())
                print(f"cancel {shape} {hw}: max |acc| / M = 2^{math.log2(rel):.1f}")
                assert rel < 2.0 ** -6
                assert not c.shift.any()
            if regime == "range":
                a = y.abs()
                assert bool(((a > 0) & (a < 2.0 ** -14)).any()) and float(a.max()) > 3e4
            if regime in sc.EXACT:
                assert float(c.ref.M.max()) < 2.0 ** 24 and torch.equal(c.ref.acc, c.ref.acc.round())
                assert torch.equal(c.ref.y, c.ref.acc)
            if regime == "border":
                assert not c.x[1:-1, 1:-1].any() and bool(c.x[0].any()) and bool(c.x[:, -1].any())
                assert shape[2] == 1 or (not c.w[:, :, 1, 1].any() and bool(c.w[:, :, 0, 0].any()))
                assert bool(y.any())


def test_stem_builders():
    for hw in sc.STEM_HW:
        c = sc.stem_case(hw, "range")
        a = c.ref.y.abs()
        assert bool(((a > 0) & (a < 2.0 ** -14)).any()) and float(a.max()) > 3e4
        c = sc.stem_case(hw, "integers")
        assert torch.equal(c.ref.y, torch.relu(c.ref.acc)) and c.ref.K == 9


@pytest.mark.parametrize("shape", sc.SIMAM_SHAPES + sc.PSUM_EXTRA, ids=_ids)
def test_simam_builders(shape):
    H, W, C = shape
    x = sc.simam_x(shape)
    assert torch.equal(x, x.half().to(F64))
    for kind in sc.RESIDUALS:
        r = sc.simam_ref(x, sc.residual(kind, x, shape))
        assert bool(torch.isfinite(r.y).all()) and float(r.y.max()) * (1 + 2.0 ** -10) < sc.FP16_MAX
        per = {n: slice(i, None, len(REGIMES)) for i, n in enumerate(REGIMES)}
        assert not r.v[per["const"]].any() and not r.d[:, per["const"]].any()
        # the sample variance of TWO draws scatters by a factor around 4e-6: at P = 2, below lambda itself
        assert float(r.v[per["tiny"]].max()) < (1e-5 if H * W > 2 else sc.LAM / 4)
        # one position carries all of S: e = (P - 1)^2 / (4 P) + 0.5 there (an e of 1e4 would take P > 40,000)
        P, e_max = H * W, r.e[:, per["outlier"]].amax(0)
        assert bool(((e_max / ((P - 1) ** 2 / (4 * P) + 0.5) - 1).abs() < 1e-3).all())
        if P >= 129:
            assert float(e_max.min()) > 17.4 and bool((1 + torch.exp(-e_max.float()) == 1).all())
        if P == 32800:
            assert float(e_max.min()) > 8000 and not torch.exp(-e_max.float()).any()
        assert float((r.m[per["offset64"]].abs()).min()) >= 64 and float(r.m[per["offset16"]].abs().min()) >= 16
        if H * W >= 129:  # |mean| of about 1000 deviations, and not a dyadic number of a few bits
            assert float((r.m[per["offset16"]] / r.v[per["offset16"]].sqrt()).min()) > 500
            assert bool((r.m[per["offset64"]] * 16 != (r.m[per["offset64"]] * 16).round()).all())
        if kind == "cancel":  # x sigma + res sits around 0: far below the |x| of the channel
            xo = x[:, per["ordinary"]]
            assert float((r.x * r.sig + r.res).abs()[:, per["ordinary"]].max()) < 0.5 * float(xo.abs().max())


# ------------------------------------------------------------------------------------------ emulations meet the bounds
def _judge_conv(c, stored, psum):
    """-> (worst ratio of the stored values, worst ratio of psum against the sums of those stored values)."""
    worst = sc.worst_ratio(stored, c.ref.y, c.ref.bound)
    if c.exact and not torch.equal(stored, c.ref.y.half()):
        worst = math.inf
    st = stored.to(F64)
    wp = sc.worst_ratio(psum, sc.tile_sums(st), sc.psum_bound(st).clamp_min(1e-300))
    if c.exact and not torch.equal(psum.to(F64), sc.tile_sums(st)):
        wp = math.inf
    return worst, wp


@pytest.mark.parametrize("shape", sc.CONV_SHAPES, ids=_ids)
def test_fp32_conv_emulation_meets_the_bound(shape):
    table = {}
    for hw in sc.conv_hw_of(shape):
        for regime in sc.conv_regimes_of(shape):
            c = sc.conv_case(shape, hw, regime)
            w, wp = _judge_conv(c, *sc.emu_conv(c))
            t = table.setdefault(regime, [0.0, 0.0])
            t[0], t[1] = max(t[0], w), max(t[1], wp)
    print(f"conv emulation {shape}: " + ", ".join(f"{r} {a:.3f} psum {b:.3f}" for r, (a, b) in table.items()))
    assert all(a <= 1.0 and b <= 1.0 for a, b in table.values()), table


def test_fp32_stem_emulation_meets_the_bound():
    for hw in sc.STEM_HW:
        for regime in sc.STEM_REGIMES:
            c = sc.stem_case(hw, regime)
            stored, _ = sc.emu_conv(c)
            worst = sc.worst_ratio(stored, c.ref.y, c.ref.bound)
            print(f"stem emulation {hw} {regime}: {worst:.3f}")
            assert worst <= 1.0 and (not c.exact or torch.equal(stored, c.ref.y.half()))


def _simam_emulated(shape, kind, with_psum, mode="ok"):
    """-> per-regime worst ratio of the emulation (or a mutant) on one case."""
    H, W, C = shape
    if with_psum:
        stored, psum = sc.emu_conv(sc.psum_conv(shape))
        x = stored.to(F64).reshape(H * W, C)
        assert psum.shape[0] == sc.n_tiles(H, W, 3, 1)
    else:
        x, psum = sc.simam_x(shape), None
    res = sc.residual(kind, x, shape)
    got = sc.emu_simam(x, res, psum, mode)
    n_s = sc.simam_n_s(H * W, C, 0 if psum is None else psum.shape[0])
    return sc.regime_max(sc.simam_ratio(got, sc.simam_ref(x, res), n_s))


@pytest.mark.parametrize("shape", sc.SIMAM_SHAPES, ids=_ids)
def test_fp32_simam_emulation_meets_the_bound(shape):
    for kind in sc.RESIDUALS:
        worst = _simam_emulated(shape, kind, False)
        print(f"simam emulation {shape} {kind}: " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))
        assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("shape", sc.PSUM_SHAPES, ids=_ids)
def test_fp32_simam_emulation_with_tile_sums_meets_the_bound(shape):
    c = sc.psum_conv(shape)
    stored, _ = sc.emu_conv(c)
    for i, n in enumerate(REGIMES):  # the identity channels are the crafted ones exactly
        if n in ("const", "offset64", "offset16"):
            assert torch.equal(stored[:, :, i::6].to(F64), c.x[:, :, i::6])
    for kind in sc.RESIDUALS:
        worst = _simam_emulated(shape, kind, True)
        print(f"simam emulation after conv {shape} {kind}: " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))
        assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------ conv mutants
S128 = (128, 128, 3, 1)


@pytest.mark.parametrize("shape", [S128, (64, 128, 3, 2)], ids=_ids)
def test_mutant_taps_flipped_misses_on_integers(shape):
    for hw in sc.CONV_HW:
        c = sc.conv_case(shape, hw, "integers")
        assert _judge_conv(c, *sc.emu_conv(c, flip_taps=True))[0] > 1.0


@pytest.mark.parametrize("shape", [S128, (64, 128, 3, 2)], ids=_ids)
def test_mutant_edge_clamp_misses_on_border(shape):
    for hw in sc.CONV_HW:
        c = sc.conv_case(shape, hw, "border")
        assert _judge_conv(c, *sc.emu_conv(c, clamp=True))[0] > 1.0


@pytest.mark.parametrize("regime", ["ordinary", "ordinary_relu", "cancel"])
def test_mutant_dropped_k_step_misses(regime):
    """One K step (channels 32 .. 63) of the centre tap left out, at Ci = 128."""
    for hw in sc.CONV_HW:
        c = sc.conv_case(S128, hw, regime)
        worst = _judge_conv(c, *sc.emu_conv(c, drop=(1, 4)))[0]
        print(f"dropped K step {hw} {regime}: {worst:.1f}")
        assert worst > 1.0


@pytest.mark.parametrize("shape", [S128, (64, 128, 3, 2)], ids=_ids)
def test_mutant_psum_before_the_fp16_rounding_misses_on_ordinary(shape):
    for hw in sc.CONV_HW:
        c = sc.conv_case(shape, hw, "ordinary")
        w, wp = _judge_conv(c, *sc.emu_conv(c, psum_f32=True))
        print(f"psum of the fp32 values {shape} {hw}: {wp:.1f}")
        assert w <= 1.0 and wp > 1.0


# ------------------------------------------------------------------------------------------ SimAM mutants
P2, P129, P1025 = (1, 2, 32), (3, 43, 64), (5, 205, 128)


def _mutant(shape, mode):
    """Per regime, the worse of the two residual kinds."""
    a, b = (_simam_emulated(shape, kind, False, mode) for kind in sc.RESIDUALS)
    worst = {n: max(a[n], b[n]) for n in REGIMES}
    print(f"{mode} {shape}: " + ", ".join(f"{n} {v:.3g}" for n, v in worst.items()))
    return worst


@pytest.mark.parametrize("shape", [P129, P1025], ids=_ids)
def test_mutant_one_pass_variance_misses_on_the_offsets(shape):
    worst = _mutant(shape, "onepass")
    assert worst["offset64"] > 1.0 and worst["offset16"] > 1.0


@pytest.mark.parametrize("shape", [P129, P1025, (3, 43, 8), (3, 43, 2048)], ids=_ids)
def test_mutant_fp16_mean_misses_on_the_offsets(shape):
    worst = _mutant(shape, "meanh")
    assert worst["offset64"] > 1.0 and worst["offset16"] > 1.0


def test_mutant_divisor_p_misses():
    worst = _mutant(P2, "divP")
    assert all(worst[n] > 1.0 for n in REGIMES if n != "const"), worst
    assert _mutant(P1025, "divP")["ordinary"] > 1.0


@pytest.mark.parametrize("shape", [P2, P129, P1025], ids=_ids)
def test_mutant_without_lambda_misses_on_const_and_tiny(shape):
    worst = _mutant(shape, "nolam")
    assert worst["const"] == math.inf and worst["tiny"] > 1.0  # const: 0 / 0


@pytest.mark.parametrize("shape", [P2, P129, P1025], ids=_ids)
def test_mutant_lambda_1e3_misses_on_tiny(shape):
    assert _mutant(shape, "lam3")["tiny"] > 1.0


@pytest.mark.parametrize("shape", [P129, P1025], ids=_ids)
def test_mutant_without_the_factor_4_misses_on_ordinary(shape):
    assert _mutant(shape, "no4")["ordinary"] > 1.0
