"""tests/mamba_cases.py judged on the CPU: the fp64 reference agrees with oracle/hybrid_cpu.py, every case meets its
input conditions, float32 emulations of the kernels' arithmetic meet the criterion on every regime, and each mutant of
that arithmetic misses it on the regime built to catch it. No GPU."""
import math

import pytest
import torch

from oracle.hybrid_cpu import mamba2_scan_ref, mamba2_step_ref, ssd_chunked
from tests import mamba_cases as mc
from tests.mamba_cases import CASES, D_SSM, DS, E, HD, LENS, MD, NH

ALL = [(c, T) for c in CASES for T in LENS]


def _ids(v):
    return f"{v[0]}-{v[1]}"


def _worst(got_y, got_s, r):
    """Per-head max(error / bound) of y and of the state."""
    return mc.head_max(mc.ratio(got_y, r.y64, r.y_abs)), mc.head_max(mc.ratio(got_s, r.state64, r.state_abs))


def _show(tag, case, T, wy, ws):
    heads = CASES[case][0]
    print(f"{tag} {case} T={T}: " + ", ".join(f"{h} y {a:.3f} state {b:.3f}" for h, a, b in zip(heads, wy, ws)))


# ------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("T", [17, 257])
def test_ref64_agrees_with_the_oracle(T):
    """Ordinary regime (case mix): ref64's recurrence equals ssd_chunked (fp64, chunks of 64) to fp64 rounding, and
    mamba2_scan_ref (fp32, bf16 out) lies within the criterion of it; conv output and ring are the oracle's bits."""
    i, r = mc.build("mix", T), mc.reference("mix", T)
    x = r.xc[:, :D_SSM].double().view(1, T, NH, HD)
    B, C = r.xc[None, :, D_SSM:D_SSM + DS].double(), r.xc[None, :, D_SSM + DS:].double()
    y, st = ssd_chunked(x, r.dt[None], i.A.double(), B, C, 64)
    y = y[0].reshape(T, D_SSM) + (i.D.double()[None, :, None] * x[0]).reshape(T, D_SSM)
    assert ((y - r.y64).abs() <= 1e-12 * r.y_abs).all()
    assert ((st[0] - r.state64).abs() <= 1e-12 * r.state_abs).all()
    oy, os_, oconv = mamba2_scan_ref(i.zx[None], *i.params, MD)
    wy, ws = _worst(oy[0], os_[0], r)
    _show("oracle", "mix", T, wy, ws)
    assert max(wy) <= 1.0 and max(ws) <= 1.0
    for k in range(4):
        q = T - 4 + k
        assert torch.equal(r.ring[q & 3], oconv[0, :, k])


def test_ref64_step_agrees_with_the_oracle():
    """One step at position 2 from a crafted state and a ring with a stale slot below position 0."""
    i = mc.build("mix", 3)
    st0 = mc.crafted_state(0)
    ring0 = torch.full((4, MD["conv_dim"]), 7.0, dtype=torch.bfloat16)
    raw = i.zx[:, D_SSM:D_SSM + MD["conv_dim"]]
    ring0[0], ring0[1] = raw[0], raw[1]
    r = mc.ref64(i.zx[2:3], *i.params, MD, state0=st0, ring0=ring0, pos0=2)
    win = torch.stack([torch.zeros_like(raw[0]), raw[0], raw[1], raw[2]], dim=-1)[None]
    oy, os_ = mamba2_step_ref(i.zx[2:3], win, st0[None], *i.params, MD)
    assert max(mc.head_max(mc.ratio(oy, r.y64, r.y_abs))) <= 1.0
    assert max(mc.head_max(mc.ratio(os_[0], r.state64, r.state_abs))) <= 1.0
    assert torch.equal(r.ring[2], raw[2]) and torch.equal(r.ring[0], raw[0]) and (r.ring[3] == 7.0).all()
    assert torch.equal(r.xc, mc.reference("mix", 3).xc[2:3])


def test_ulp_and_bound():
    v = torch.tensor([1.0, 1.5, 2.0, 255.0, 0.0, 2.0 ** -130, 3e38], dtype=torch.float64)
    want = [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 1.0, 2.0 ** -133, 2.0 ** -133, 2.0 ** 120]
    assert mc.ulp_bf16(v).tolist() == want
    r = mc.ratio(torch.tensor([math.inf, math.nan, 1.0]), torch.ones(3, dtype=torch.float64),
                 torch.ones(3, dtype=torch.float64))
    assert r[0] == math.inf and r[1] == math.inf and r[2] == 0


# ------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("case_T", ALL, ids=_ids)
def test_inputs_are_safe(case_T):
    """Every conv + SiLU value is clear of a bf16 rounding tie by the derived margin, an fp32 evaluation rounds to the
    same bits, every S_abs is clear of the underflow range, and the regime's own property holds."""
    case, T = case_T
    i, r = mc.build(case, T), mc.reference(case, T)
    assert not mc.unsafe(r.acc, r.acc_abs).any()
    assert torch.equal(torch.from_numpy(mc.emu_conv(i)).to(torch.bfloat16), r.xc)
    assert mc.clear_of_underflow(r.y_abs, 128 * T) and mc.clear_of_underflow(r.state_abs, T)
    assert torch.isfinite(r.y64).all() and torch.isfinite(r.state64).all()
    if case == "conv":
        assert not r.state64.any() and torch.equal(r.y64, r.xc[:, :D_SSM].double())
    if case == "cancel" and T >= 17:
        small = (r.y64.abs() / r.y_abs)[:, :2 * HD].median().item()
        assert small < 0.1, small  # heads a and b: |y| << S_abs
        x = r.xc[:, :D_SSM].double()
        assert torch.equal(x[1:], -x[:-1]) and torch.equal(r.xc[1:, D_SSM:], r.xc[:-1, D_SSM:])
    if case == "dt":
        tot = (i.zx[:, D_SSM + MD["conv_dim"]].double() + i.dtb[0].double()).tolist()
        assert tot == [mc.THRESHOLD_TOTALS[t % 8] for t in range(T)]
        assert (r.dt[:min(T, 8), 1] == 30.0).all() and (T <= 8 or (r.dt[8:, 1] < 0.02).all())
    if case == "mix" and T >= 17:
        dA = torch.exp(i.A.double()[None] * r.dt)
        assert (1 - dA[:, 1]).max() < 4e-4 and dA[:, 2].max() < 1e-27 and (dA[:, 2].float() == 0).any()
    if case == "tails":
        assert r.xc.double().abs().max() == 64.0 and 0 < r.xc.double().abs().min() < 2e-26


def test_handover_inputs_are_safe():
    for case in CASES:
        i = mc.build(case, sum(mc.HANDOVER))
        assert not mc.unsafe(*mc.conv64(i.zx, i.cw, i.cb)).any()
    for seed in range(3):  # the three sequences of the permuted-state-row probe
        i = mc.build("dt", 33, 0, seed)
        assert not mc.unsafe(*mc.conv64(i.zx, i.cw, i.cb)).any()


# ------------------------------------------------------------------------------------------ emulations and mutants
@pytest.mark.parametrize("case_T", ALL, ids=_ids)
def test_fp32_recurrence_meets_the_bound(case_T):
    case, T = case_T
    i, r = mc.build(case, T), mc.reference(case, T)
    wy, ws = _worst(*mc.emu_recurrence(i), r)
    _show("recurrence", case, T, wy, ws)
    assert max(wy) <= 1.0 and max(ws) <= 1.0


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_step_meets_the_bound(case):
    """One step from a crafted state (huge and tiny magnitudes; the conv case: its own all-zero state) at positions
    0, 1, 3, 4 and 530 of the regimes: the rows of the GPU step probe."""
    for pos in mc.STEP_POS[:-1]:
        i, n, st0, ring0 = mc.step_probe(case, pos)
        assert not mc.unsafe(*mc.conv64(i.zx, i.cw, i.cb)).any()
        r = mc.ref64(i.zx[n:], *i.params, MD, state0=st0, ring0=ring0, pos0=pos)
        assert mc.clear_of_underflow(r.y_abs, 256) and mc.clear_of_underflow(r.state_abs, 2)
        last = mc.Inputs(case, i.zx[n:], *i.params)
        xc = mc.emu_conv(last, ring0, pos)
        assert torch.equal(torch.from_numpy(xc).to(torch.bfloat16), r.xc)
        wy, ws = _worst(*mc.emu_recurrence(last, xc=xc, state0=st0), r)
        _show(f"step pos {pos}", case, 1, wy, ws)
        assert max(wy) <= 1.0 and max(ws) <= 1.0


@pytest.mark.parametrize("case_T", [(c, T) for c in CASES for T in LENS if T <= 256], ids=_ids)
def test_ssd_with_fp64_cum_meets_the_bound(case_T):
    """The SSD arithmetic (two-term bf16 split) with the running sum of A dt and its differences in fp64."""
    case, T = case_T
    i, r = mc.build(case, T), mc.reference(case, T)
    wy, ws = _worst(*mc.emu_ssd(i, cum64=True), r)
    _show("ssd cum64", case, T, wy, ws)
    assert max(wy) <= 1.0 and max(ws) <= 1.0


def test_mutant_ssd_with_an_fp32_running_sum_misses_on_reset():
    """exp(cum[t] - cum[s]) from ONE fp32 running sum over the sequence has an absolute error of ~ |cum| 2^-23 in the
    exponent, whatever the size of the difference. Simulated at T = 256, max |y - y64| / S_abs before y is rounded to
    bf16 (the criterion allows E = 2^-14 of S_abs plus half a bf16 ulp of y):

        regime      |cum[T-1]|   SSD, fp32 sum   SSD, fp64 sum   fp32 recurrence
        ordinary         135        2^-18.2         2^-19.4          2^-23.3
        reset          3,880        2^-12.3         2^-18.9          2^-22.0
        reset130      62,420        2^-7.8          2^-18.8          2^-21.7

    (a sequential fp32 sum; the kernel's shuffle scan adds in a tree and erred about a third as much on reset130.)
    Asserted: with the fp32 sum the reset regimes err by more than half an ulp of their |cum| (2^-13 and 2^-9), the
    ordinary one by less than E; with the sum and its differences in fp64 every regime stays below E / 4, as the
    recurrence does (and passes the criterion: test_ssd_with_fp64_cum_meets_the_bound)."""
    rows = {}
    for case, h, name in (("mix", 0, "ordinary"), ("dt", 1, "reset"), ("dt", 2, "reset130")):
        i, r = mc.build(case, 256), mc.reference(case, 256)
        rel = lambda y: mc.head_max((y - r.y64).abs() / r.y_abs)[h]
        rows[name] = (rel(mc.emu_ssd(i, round_out=False)[0]), rel(mc.emu_ssd(i, cum64=True, round_out=False)[0]),
                      rel(mc.emu_recurrence(i, round_out=False)[0]))
        cum = (i.A.double()[h] * r.dt[:, h]).sum().abs().item()
        print(f"{name}: |cum| {cum:.0f}, max err / S_abs: " + ", ".join(f"2^{math.log2(v):.1f}" for v in rows[name]))
    assert rows["ordinary"][0] < E
    assert rows["reset"][0] > 2.0 ** -13 and rows["reset130"][0] > 2.0 ** -9
    assert all(v[1] < E / 4 and v[2] < E / 4 for v in rows.values())
    i, r = mc.build("dt", 256), mc.reference("dt", 256)
    wy, ws = _worst(*mc.emu_ssd(i), r)
    _show("ssd fp32 cum", "dt", 256, wy, ws)
    assert wy[1] > 1.5 and wy[2] > 8.0 and ws[1] > 1.5 and ws[2] > 8.0, (wy, ws)


def test_mutant_ssd_without_lo_misses_on_cancel():
    for T in (33, 256):
        i, r = mc.build("cancel", T), mc.reference("cancel", T)
        wy, ws = _worst(*mc.emu_ssd(i, cum64=True, drop_lo=True), r)
        _show("ssd without lo", "cancel", T, wy, ws)
        assert max(wy) > 2.0 and max(ws) > 2.0


def test_mutant_softplus_without_threshold_misses_on_threshold():
    i, r = mc.build("dt", 17), mc.reference("dt", 17)
    y, s = mc.emu_recurrence(i, threshold=False)
    wy, ws = _worst(y, s, r)
    assert wy[0] == math.inf, wy  # log1p(exp(96)) = inf in fp32
    assert max(_worst(*mc.emu_recurrence(i), r)[0]) <= 1.0


def test_mutant_conv_taps_reversed_misses_on_conv():
    i, r = mc.build("conv", 17), mc.reference("conv", 17)
    wy, _ = _worst(*mc.emu_recurrence(i, xc=mc.emu_conv(i, taps_reversed=True)), r)
    assert min(wy) > 8.0, wy


def test_mutant_bias_added_last_after_bf16_rounding_misses_on_conv():
    """The tap sum rounded to bf16 before the bias: a second rounding a criterion of half an ulp cannot absorb."""
    i, r = mc.build("conv", 257), mc.reference("conv", 257)
    xc = mc.emu_conv(i, bias_last_bf16=True)
    wy, _ = _worst(*mc.emu_recurrence(i, xc=xc), r)
    assert min(wy) > 1.5, wy
    assert not torch.equal(torch.from_numpy(xc).to(torch.bfloat16), r.xc)


def test_mutant_state_rounded_between_positions_misses_on_slow():
    """bf16 state between the positions of a scan: 2^-9 per position where every term stays live."""
    i, r = mc.build("mix", 33), mc.reference("mix", 33)
    wy, ws = _worst(*mc.emu_recurrence(i, round_state=True), r)
    _show("state rounded per position", "mix", 33, wy, ws)
    assert wy[1] > 2.0 or ws[1] > 2.0, (wy, ws)
    assert wy[0] > 2.0, wy  # and on the ordinary regime
