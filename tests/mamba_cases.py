"""Cases, the fp64 reference and the criterion shared by the CPU and GPU probes of the Mamba2 kernels (zmi_mamba.hip:
zmi_mamba2_step, zmi_mamba2_scan, zmi_mamba2_scan_ws in its 1 / 2 / 4-workgroup and SSD forms, zmi_mamba2_scan_seqs).

Geometry: nheads = 3, d_ssm = 192, so conv_dim = 448 (two channel blocks of 256, the second partial) and d_in_proj = 643
(odd row stride). A head carries a REGIME of its own (its A, D, dt_bias, its x channels and its dt column); B and C are
shared by the heads, so a CASE is three regimes plus one kind of B / C. Three regimes cost one launch.

  case     heads                                  B / C
  mix      ordinary, slow, fast                   random taps and bias, N(0,1) raw inputs
  dt       threshold, reset, reset130             identity conv, N(0,1)
  tails    tails under ordinary / slow / reset dt identity conv, a quarter of the raw values in {+-8, +-64}
  cancel   cancel_a / _b / _c                     identity conv, constant in time
  conv     conv under ordinary / threshold / fast random taps; B: raw inputs and bias 0, so B = 0 and the state stays 0

  ordinary   the family of tests/test_gpu_hybrid.py: random taps, dt_bias in [-3, -1], A in [-16, -1], D ~ 1
  slow       A = -1, dt ~ 1e-4: dA within 1e-4 of 1, every term of the sequence stays live
  fast       A = -16, dt in [4, 8]: dA = exp(-64 .. -128) runs through tiny, subnormal and 0
  threshold  dt_raw + dt_bias cycles through 19.875, 20, 20.125, 96 (exact in bf16 and in the fp32 sum) and four
             ordinary values: both sides of softplus's branch at 20, and 96 where log1p(exp(v)) is inf in fp32
  reset      8 positions with dt_raw + dt_bias = 30 (the head forgets: A dt = -480), then dt ~ 0.01, A = -16:
             the running sum of A dt is ~ -3,840 while the live differences are ~ 0.16
  reset130   the same with 130 forgetting positions (the sum reaches ~ -62,400)
  cancel_*   x of one magnitude and alternating sign, B and C constant, D = 0 (a, b): |y| << S_abs. A dt per position
             -0.25 (a), -0.03 (b), -0.003 (c)
  tails      raw x values up to +-64: SiLU from -64 e^-64 to 64
  conv       y is exactly the x channels' conv + SiLU output (D = 1, state 0): tap order, bias first, zero below
             position 0 and the channel mapping, bit for bit

THE REFERENCE. ref64 evaluates the operation in fp64 with ONE internal rounding: the conv + SiLU output to bf16 (the
reference implementation's conv output tensor is bf16; oracle/hybrid_cpu.py). The state is rounded to bf16 only where the
library stores it, i.e. by the caller between ref64 calls. Besides y64 and state64 it returns

    S_abs[t, p] = sum_{s <= t} sum_n |C_tn| |B_sn| decay(t, s) dt_s |x_sp| + |D x_tp|  (+ sum_n |C_tn| decay |state0_pn|)

and the same for the state: the sum of the magnitudes a kernel adds up, the scale of its rounding error.

THE CRITERION, for every form alike, elementwise, no floor relative to the tensor:

    |got - y64| <= E S_abs + 0.5 ulp_bf16(|y64| + E S_abs),   E = 2^-14

E is derived, not measured: the fp32 recurrence accumulates at most (T + 128 + a few) 2^-24 ~ 2^-15.4 of S_abs at
T = 257; the SSD form's two-term bf16 split keeps ~ 2^-17 per entry; E is the larger with a 2x margin and still 16x
below the 2^-10 of a single bf16 M. ulp_bf16 is that of the number format: below 2^-126 (the smallest normal) it is
the subnormal spacing 2^-133.

INPUT SAFETY. The bf16 rounding of the conv output is a decision, so a kernel's fp32 evaluation and the fp64 one must
take it alike. A builder redraws raw values until every fp64 conv + SiLU value v = silu(acc) lies further from a bf16
rounding tie than

    margin = 1.25 |silu'(acc)| 4 2^-24 (|b| + sum_k |w_k x_k|)  +  2^-21 |v|

the first term: four fused multiply-adds, each rounding at most 2^-24 of the absolute sum, carried through SiLU's
slope; the second: expf (2 ulp), 1 + e, the division (one rounding each) on v itself. Where nothing cancels this is
~ 2^-12 of a bf16 ulp. A margin of 0 (all products 0) is exact arithmetic and always safe. This is a condition on the
inputs, asserted by tests/test_mamba_cases_cpu.py for every case, not a tolerance on the kernels.

UNDERFLOW. The criterion is fp32's relative-error model; it has no term for a product lost below 2^-126 (gradual
underflow or flush to zero: at most 2^-126 each). SiLU's tail makes x and B as small as 64 e^-64 ~ 1e-26, so the cases
are built to keep every output's scale away from that range: an S_abs that sums n terms (T for a state element, 128 T
for y, one more position for a carried state) is either at least n 2^-110, so that n lost products stay below a quarter
of E S_abs, or below 2^-140, where the fp64 value and a kernel's 0 differ by less than half the subnormal spacing. The
tails regime therefore runs under ordinary, slow and reset decay, not under the fast one, where a decayed term of
~ 1e-40 is all that is left of an element whose newest x and B are both tiny. The CPU test asserts the condition
(clear_of_underflow).
"""
from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass

import numpy as np
import torch

E = 2.0 ** -14
LENS = (1, 4, 17, 32, 33, 256, 257)  # tile edges of 16 and 32, the SSD form's reach and the fallback past it
MD = dict(d_ssm=192, d_state=128, nheads=3, headdim=64, d_conv=4, ngroups=1, conv_dim=448, d_in_proj=643)
NH, HD, DS, D_SSM, CD = 3, 64, 128, 192, 448
BF = torch.bfloat16
F64 = torch.float64

CASES = {
    "mix": (("ordinary", "slow", "fast"), "rand_conv"),
    "dt": (("threshold", "reset", "reset130"), "id"),
    "tails": (("tails_ordinary", "tails_slow", "tails_reset"), "tails"),
    "cancel": (("cancel_a", "cancel_b", "cancel_c"), "const"),
    "conv": (("conv_ordinary", "conv_threshold", "conv_fast"), "zero_b"),
}
THRESHOLD_TOTALS = (19.875, -1.0, 20.0, -1.5, 20.125, -0.5, 96.0, -2.0)  # dt_raw + dt_bias, by position % 8

# regime -> A, D, dt_bias (None: drawn from the ordinary family), the x channels' kind and conv, the dt column's kind
_DT = {
    "ordinary": dict(A=None, D=None, dtb=None, dt="normal"),
    "slow": dict(A=-1.0, D=1.0, dtb=-9.25, dt="jitter"),
    "fast": dict(A=-16.0, D=1.0, dtb=2.0, dt="fast"),
    "threshold": dict(A=-1.0, D=1.0, dtb=-2.0, dt="threshold"),
    "reset": dict(A=-16.0, D=1.0, dtb=-4.5, dt="reset8"),
    "reset130": dict(A=-16.0, D=1.0, dtb=-4.5, dt="reset130"),
    "cancel_a": dict(A=-1.0, D=0.0, dtb=-1.25, dt="zero"),
    "cancel_b": dict(A=-1.0, D=0.0, dtb=-3.5, dt="zero"),
    "cancel_c": dict(A=-16.0, D=1.0, dtb=-8.5, dt="zero"),
}


def regime(name):
    """-> dict(A, D, dtb, dt, x, conv) of a head regime."""
    if name in _DT:
        r = dict(_DT[name])
        r["x"] = "pairs" if name.startswith("cancel") else "normal"
        r["conv"] = "rand" if name == "ordinary" else "id"
        return r
    kind, under = name.split("_")
    r = dict(_DT[under])
    if kind == "tails":
        r.update(x="tails", conv="id")
    else:
        r.update(x="normal", conv="rand", D=1.0)
    return r


def bf(x):
    """Round to bf16 (nearest-even) and come back as fp64."""
    return x.to(BF).to(F64)


def ulp_bf16(v):
    """Spacing of bf16 at |v| (fp64 tensor): 2^(floor(log2 |v|) - 7), the subnormal spacing 2^-133 below 2^-126."""
    v = v.abs()
    e = torch.frexp(v)[1].to(torch.int64) - 1
    e = torch.where(v > 0, e, torch.full_like(e, -126)).clamp_min(-126)
    return torch.ldexp(torch.ones_like(v), (e - 7).to(torch.int32))


def bound(ref, s_abs):
    """The criterion's right-hand side."""
    return E * s_abs + 0.5 * ulp_bf16(ref.abs() + E * s_abs)


def ratio(got, ref, s_abs):
    """|got - ref| / bound, elementwise (inf where got is not finite)."""
    got = got.to(F64)
    r = (got - ref).abs() / bound(ref, s_abs)
    return torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))


def head_max(r):
    """Per-head maxima of a ratio tensor [..., d_ssm] (y) or [nheads, 64, 128] (state)."""
    if r.shape[-1] == D_SSM:
        return [r[..., h * HD:(h + 1) * HD].max().item() for h in range(NH)]
    return [r[h].max().item() for h in range(NH)]


# ---------------------------------------------------------------------------------------------- the fp64 reference
@dataclass
class Ref:
    xc: torch.Tensor       # [T, conv_dim] bf16: conv + SiLU, the one internal rounding
    y64: torch.Tensor      # [T, d_ssm]
    y_abs: torch.Tensor    # S_abs of y
    state64: torch.Tensor  # [nheads, 64, 128]
    state_abs: torch.Tensor
    ring: torch.Tensor     # [4, conv_dim] bf16: slot q & 3 holds the raw input of position q
    dt: torch.Tensor       # [T, nheads] fp64
    acc: torch.Tensor      # [T, conv_dim] fp64 conv sums (before SiLU)
    acc_abs: torch.Tensor  # |b| + sum |w_k x_k|


def _softplus20(v):
    return torch.where(v <= 20.0, torch.log1p(torch.exp(v.clamp_max(20.0))), v)


def _silu64(a):
    return a / (1.0 + torch.exp(-a))


def _window(zx, ring0, pos0):
    """[T + 3, conv_dim] fp64 raw inputs of positions pos0 - 3 .. pos0 + T - 1 (the ring's below pos0, zero below 0)."""
    raw = zx[:, D_SSM:D_SSM + CD].to(F64)
    hist = torch.zeros(3, CD, dtype=F64)
    if ring0 is not None:
        for j in range(3):
            q = pos0 - 3 + j
            if q >= 0:
                hist[j] = ring0[q & 3].to(F64)
    return torch.cat([hist, raw])


def conv64(zx, cw, cb, ring0=None, pos0=0):
    """-> (acc, |b| + sum |w x|) of the causal depthwise conv in fp64, [T, conv_dim] each."""
    T = zx.shape[0]
    ext, w = _window(zx, ring0, pos0), cw.to(F64)
    acc = cb.to(F64)[None].expand(T, CD).clone()
    mag = acc.abs()
    for k in range(4):
        term = w[:, k][None] * ext[k:k + T]
        acc = acc + term
        mag = mag + term.abs()
    return acc, mag


def ref64(zx, cw, cb, dt_bias, A, D, md, state0=None, ring0=None, pos0=0):
    """One sequence zx [T, d_in_proj] bf16 from position pos0; state0 [nheads, 64, 128] and ring0 [4, conv_dim] (slot
    q & 3 = raw input of q) are what the cache holds before it (None: empty, as a prefill starts)."""
    assert (md["d_ssm"], md["nheads"], md["d_state"], md["headdim"]) == (D_SSM, NH, DS, HD)
    T = zx.shape[0]
    acc, mag = conv64(zx, cw, cb, ring0, pos0)
    xc = _silu64(acc).to(BF)
    x = xc[:, :D_SSM].to(F64).view(T, NH, HD)
    B, C = xc[:, D_SSM:D_SSM + DS].to(F64), xc[:, D_SSM + DS:].to(F64)
    dt = _softplus20(zx[:, D_SSM + CD:].to(F64) + dt_bias.to(F64)[None])
    dA = torch.exp(A.to(F64)[None] * dt)
    Dd = D.to(F64)
    st = torch.zeros(NH, HD, DS, dtype=F64) if state0 is None else state0.to(F64).clone()
    sa = st.abs()
    y, ya = torch.empty(T, NH, HD, dtype=F64), torch.empty(T, NH, HD, dtype=F64)
    for t in range(T):
        dbx = (B[t][None, None, :] * dt[t][:, None, None]) * x[t][:, :, None]
        st = st * dA[t][:, None, None] + dbx
        sa = sa * dA[t][:, None, None] + dbx.abs()
        dx = Dd[:, None] * x[t]
        y[t] = (st * C[t][None, None, :]).sum(-1) + dx
        ya[t] = (sa * C[t].abs()[None, None, :]).sum(-1) + dx.abs()
    ring = torch.zeros(4, CD, dtype=BF) if ring0 is None else ring0.clone()
    for q in range(pos0 + max(0, T - 4), pos0 + T):
        ring[q & 3] = zx[q - pos0, D_SSM:D_SSM + CD]
    return Ref(xc, y.view(T, D_SSM), ya.view(T, D_SSM), st, sa, ring, dt, acc, mag)


def clear_of_underflow(s_abs, terms):
    """The UNDERFLOW condition of the module docstring on an S_abs tensor whose elements sum `terms` products."""
    return bool(((s_abs >= terms * 2.0 ** -110) | (s_abs < 2.0 ** -140)).all())


def unsafe(acc, mag):
    """Where the bf16 rounding of silu(acc) could fall differently in an fp32 evaluation (module docstring)."""
    v = _silu64(acc)
    sig = torch.sigmoid(acc)
    slope = (sig * (1.0 + acc * (1.0 - sig))).abs()
    margin = 1.25 * slope * 4 * 2.0 ** -24 * mag + 2.0 ** -21 * v.abs()
    u = ulp_bf16(v)
    frac = torch.remainder(v.abs() / u, 1.0)
    dist = (frac - 0.5).abs() * u
    return (margin > 0) & (dist <= margin)


# ---------------------------------------------------------------------------------------------- builders
@dataclass
class Inputs:
    case: str
    zx: torch.Tensor  # [T, d_in_proj] bf16
    cw: torch.Tensor  # [conv_dim, 4] bf16
    cb: torch.Tensor  # [conv_dim] bf16
    dtb: torch.Tensor  # [nheads] fp32
    A: torch.Tensor
    D: torch.Tensor

    @property
    def params(self):
        return self.cw, self.cb, self.dtb, self.A, self.D


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def _pairs():
    """Raw (a, b), a > 0 > b, with bf16(silu(a)) = -bf16(silu(b)): x of one magnitude and either sign (identity conv)."""
    pos = torch.arange(0.25, 0.75, 2.0 ** -9, dtype=F64)
    neg = -torch.arange(0.5, 1.25, 2.0 ** -8, dtype=F64)
    pos, neg = pos[bf(pos) == pos], neg[bf(neg) == neg]  # the values bf16 holds
    sp, sn = bf(_silu64(pos)), bf(_silu64(neg))
    ok_p, ok_n = ~unsafe(pos, pos.abs()), ~unsafe(neg, neg.abs())
    out = [(pos[i].item(), neg[j].item()) for i in range(len(pos)) for j in range(len(neg))
           if ok_p[i] and ok_n[j] and sp[i] == -sn[j]]
    assert len(out) >= 16
    return out


def _draw(kind, T, n, g, t0):
    """Raw values [T, n] (fp32, rounded to bf16 by the caller) of one kind."""
    if kind == "normal":
        return torch.randn(T, n, generator=g)
    if kind == "tails":
        v = torch.randn(T, n, generator=g)
        big = torch.tensor([8.0, 64.0])[torch.randint(0, 2, (T, n), generator=g)]
        big = big * (torch.randint(0, 2, (T, n), generator=g) * 2 - 1)
        return torch.where(torch.rand(T, n, generator=g) < 0.25, big, v)
    if kind == "const":
        return torch.randn(1, n, generator=g).expand(T, n).clone()
    if kind == "zero":
        return torch.zeros(T, n)
    if kind == "pairs":
        pr = _pairs()
        pick = torch.randint(0, len(pr), (n,), generator=g)
        ab = torch.tensor([pr[i] for i in pick.tolist()], dtype=torch.float32)  # [n, 2]
        first = torch.randint(0, 2, (n,), generator=g)
        par = (torch.arange(t0, t0 + T)[:, None] + first[None]) & 1
        return torch.where(par == 0, ab[:, 0][None], ab[:, 1][None])
    raise KeyError(kind)


def _dt_raw(kind, dtb, T, g, t0):
    """The dt column (raw, before dt_bias) of one head at positions t0 .. t0 + T - 1."""
    pos = torch.arange(t0, t0 + T)
    if kind == "normal":
        return torch.randn(T, generator=g)
    if kind == "jitter":
        return 0.25 * torch.randn(T, generator=g)
    if kind == "fast":
        return 2.0 + 4.0 * torch.rand(T, generator=g)
    if kind == "zero":
        return torch.zeros(T)
    if kind == "threshold":
        return torch.tensor(THRESHOLD_TOTALS)[pos % 8] - dtb
    if kind in ("reset8", "reset130"):
        n = 8 if kind == "reset8" else 130
        after = -0.1 + 0.1 * torch.randn(T, generator=g)  # dt_raw + dt_bias ~ -4.6: dt ~ 0.01
        return torch.where(pos < n, torch.full((T,), 30.0 - dtb), after)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def params(case):
    """-> (cw, cb, dtb, A, D) of a case: they depend on the case alone, so launches of several lengths share them."""
    heads, bc = CASES[case]
    g = torch.Generator().manual_seed(_seed("params", case))
    cw = torch.zeros(CD, 4)
    cw[:, 3] = 1.0
    cb = torch.zeros(CD)
    rw, rb = torch.rand(CD, 4, generator=g) - 0.5, 0.1 * torch.randn(CD, generator=g)
    dtb, A, D = torch.zeros(NH), torch.zeros(NH), torch.zeros(NH)
    fam = ((torch.rand(NH, generator=g) * 2 - 3), -torch.exp(torch.rand(NH, generator=g) * 2.77),
           1 + 0.1 * torch.randn(NH, generator=g))
    for h, name in enumerate(heads):
        r = regime(name)
        sl = slice(h * HD, (h + 1) * HD)
        if r["conv"] == "rand":
            cw[sl], cb[sl] = rw[sl], rb[sl]
        dtb[h] = fam[0][h] if r["dtb"] is None else r["dtb"]
        A[h] = fam[1][h] if r["A"] is None else r["A"]
        D[h] = fam[2][h] if r["D"] is None else r["D"]
    if bc in ("rand_conv", "zero_b"):
        cw[D_SSM:], cb[D_SSM:] = rw[D_SSM:], rb[D_SSM:]
    if bc == "zero_b":
        cb[D_SSM:D_SSM + DS] = 0.0
    rnd = lambda v: v.to(BF).float()
    return cw.to(BF), cb.to(BF), rnd(dtb), rnd(A), rnd(D)


def _raw(case, T, t0, seed):
    """-> (xBC raw [T, conv_dim] bf16, whole_col [conv_dim] bool): a candidate draw; whole_col marks the channels whose
    values hang together in time (a redraw replaces the column)."""
    heads, bc = CASES[case]
    g = torch.Generator().manual_seed(seed)
    raw = torch.empty(T, CD)
    whole = torch.zeros(CD, dtype=torch.bool)
    for h, name in enumerate(heads):
        kind = regime(name)["x"]
        raw[:, h * HD:(h + 1) * HD] = _draw(kind, T, HD, g, t0)
        whole[h * HD:(h + 1) * HD] = kind == "pairs"
    kb = {"rand_conv": "normal", "id": "normal", "tails": "tails", "const": "const", "zero_b": "normal"}[bc]
    raw[:, D_SSM:] = _draw(kb, T, 2 * DS, g, t0)
    if bc == "zero_b":
        raw[:, D_SSM:D_SSM + DS] = 0.0
    whole[D_SSM:] = bc == "const"
    return raw.to(BF), whole


@functools.lru_cache(maxsize=None)
def build(case, T, t0=0, seed=0):
    """Inputs of one sequence of T positions whose regimes' position index starts at t0 (the conv window starts empty
    at the first row). Raw values are redrawn one by one until the input-safety condition holds."""
    heads, _ = CASES[case]
    cw, cb, dtb, A, D = params(case)
    g = torch.Generator().manual_seed(_seed("rows", case, T, t0, seed))
    zx = torch.zeros(T, MD["d_in_proj"], dtype=BF)
    z = 2.0 * torch.randn(T, D_SSM, generator=g)
    edge = torch.tensor([-96.0, -64.0, -20.0, 0.0, 20.0, 64.0, 96.0])[torch.randint(0, 7, (T, D_SSM), generator=g)]
    zx[:, :D_SSM] = torch.where(torch.rand(T, D_SSM, generator=g) < 0.125, edge, z).to(BF)  # the gate's input
    for h, name in enumerate(heads):
        zx[:, D_SSM + CD + h] = _dt_raw(regime(name)["dt"], dtb[h].item(), T, g, t0).to(BF)
    raw, whole = _raw(case, T, t0, _seed("raw", case, T, t0, seed, 0))
    for it in range(1, 64):
        zx[:, D_SSM:D_SSM + CD] = raw
        bad = unsafe(*conv64(zx, cw, cb))
        if not bad.any():
            return Inputs(case, zx, cw, cb, dtb, A, D)
        cand, _ = _raw(case, T, t0, _seed("raw", case, T, t0, seed, it))
        bad = bad | (whole[None] & bad.any(0)[None])
        raw = torch.where(bad, cand, raw)
    raise AssertionError(f"no safe draw for {case} T={T}")


@functools.lru_cache(maxsize=None)
def reference(case, T, t0=0, seed=0):
    """ref64 of build(...) as a prefill from an empty cache: computed once, shared, never modified."""
    i = build(case, T, t0, seed)
    return ref64(i.zx, *i.params, MD)


def crafted_state(seed):
    """A bf16 state [nheads, 64, 128] of mixed huge and tiny magnitudes: 2^k, k in [-60, 60], random sign and mantissa."""
    g = torch.Generator().manual_seed(_seed("state", seed))
    k = torch.randint(-60, 61, (NH, HD, DS), generator=g)
    m = (1.0 + torch.rand(NH, HD, DS, generator=g)) * (torch.randint(0, 2, (NH, HD, DS), generator=g) * 2 - 1)
    return torch.ldexp(m, k.to(torch.int32)).to(BF)


def step_state(case, seed):
    """The state a step probe starts from: crafted, but all zero in the conv case (B = 0 keeps a state at 0, which is
    what makes y the conv output itself; a decaying crafted state with no new term would sink into the underflow range)."""
    return torch.zeros(NH, HD, DS, dtype=BF) if case == "conv" else crafted_state(seed)


STEP_POS = (0, 1, 3, 4, 530, -1)  # positions of the step probes: ring slots below 0, the ring's wrap, an inactive row
STALE_RING = 7.0
HANDOVER = (33, 5)                # a prefill of 33 positions, then 5 steps


def step_probe(case, pos):
    """One row of a step launch at position pos (< 0: an inactive row, built as position 0): -> (inputs of the last
    n = min(pos, 3) positions and this one, n, state0, ring0 with stale values in the slots no position has written)."""
    p = max(pos, 0)
    n = min(p, 3)
    i = build(case, n + 1, p - n, seed=p)
    ring0 = torch.full((4, CD), STALE_RING, dtype=BF)
    for k in range(n):
        ring0[(p - n + k) & 3] = i.zx[k, D_SSM:D_SSM + CD]
    return i, n, step_state(case, p), ring0


# ---------------------------------------------------------------------------------------------- fp32 emulations
# What the kernels' arithmetic can and cannot do, on the CPU: numpy float32 operations round once each, as the kernels'
# do. Every emulation takes switches that turn it into one of the mutants tests/test_mamba_cases_cpu.py requires the
# criterion to catch.
f32 = np.float32


def _np32(t):
    return t.to(torch.float32).numpy()


def _bf_np(a):
    """numpy float32 -> rounded to bf16 -> float32."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(BF).to(torch.float32).numpy()


def emu_conv(inp, ring0=None, pos0=0, taps_reversed=False, bias_last_bf16=False):
    """conv4 of zmi_mamba_step.h in float32: bias first, four fused multiply-adds oldest tap first, SiLU, bf16.
    Mutants: the taps in reverse order; the tap sum rounded to bf16 and the bias added last."""
    T = inp.zx.shape[0]
    ext = _window(inp.zx, ring0, pos0).numpy()
    w = inp.cw.to(F64).numpy()
    if taps_reversed:
        w = w[:, ::-1]
    b = inp.cb.to(F64).numpy()[None]
    acc = np.zeros((T, CD), f32) if bias_last_bf16 else np.broadcast_to(b, (T, CD)).astype(f32)
    for k in range(4):
        acc = (w[:, k][None] * ext[k:k + T] + acc.astype(np.float64)).astype(f32)  # one rounding: a fused multiply-add
    if bias_last_bf16:
        acc = _bf_np(acc) + b.astype(f32)
    with np.errstate(over="ignore"):
        v = acc / (f32(1) + np.exp(-acc))
    return _bf_np(v)


def _dt32(inp, threshold=True):
    v = _np32(inp.zx[:, D_SSM + CD:]) + _np32(inp.dtb)[None]
    with np.errstate(over="ignore"):
        sp = np.log1p(np.exp(v))
    return (np.where(v <= f32(20), sp, v) if threshold else sp).astype(f32)


def _out(a, round_out):
    a = np.ascontiguousarray(a, dtype=f32)
    return torch.from_numpy(_bf_np(a) if round_out else a).to(F64)


def emu_recurrence(inp, xc=None, state0=None, threshold=True, round_state=False, round_out=True):
    """The recurrence of mamba2_scan_kernel / the step in float32 -> (y, state) rounded to bf16 (round_out False: the
    fp32 values before that rounding), as fp64 tensors. xc: the conv output to use (default emu_conv's). Mutants: softplus without its branch at 20; the state rounded to
    bf16 between positions."""
    xc = emu_conv(inp) if xc is None else xc
    T = xc.shape[0]
    x = xc[:, :D_SSM].reshape(T, NH, HD)
    B, C = xc[:, D_SSM:D_SSM + DS], xc[:, D_SSM + DS:]
    dt = _dt32(inp, threshold)
    A, D = _np32(inp.A), _np32(inp.D)
    with np.errstate(all="ignore"):
        dA = np.exp(A[None] * dt)
        st = np.zeros((NH, HD, DS), f32) if state0 is None else _np32(state0).copy()
        y = np.empty((T, NH, HD), f32)
        for t in range(T):
            st = st * dA[t][:, None, None] + (B[t][None, None, :] * dt[t][:, None, None]) * x[t][:, :, None]
            y[t] = (st * C[t][None, None, :]).sum(-1, dtype=f32) + x[t] * D[:, None]
            if round_state:
                st = _bf_np(st)
    return _out(y.reshape(T, D_SSM), round_out), _out(st, round_out)


def emu_ssd(inp, xc=None, drop_lo=False, cum64=False, round_out=True):
    """The quadratic (SSD) form of mamba2_ssd_kernel: M = (C B^T) exp(cum_t - cum_s) dt_s split into two bf16 terms,
    y = M_hi X + M_lo X; the state from W = exp(cum_T-1 - cum_s) dt_s x_s split the same way. The products of bf16
    operands are summed in fp64 and rounded to fp32 once (the MFMA's fp32 sums are not modelled: the emulation is about
    cum, exp and the split). cum: a sequential float32 running sum of A dt (cum64: fp64, differences taken in fp64).
    Mutant: the lo terms dropped. -> (y, state) rounded to bf16 (round_out False: before that rounding), as fp64 tensors."""
    xc = emu_conv(inp) if xc is None else xc
    T = xc.shape[0]
    x = xc[:, :D_SSM].reshape(T, NH, HD).astype(np.float64)
    B, C = xc[:, D_SSM:D_SSM + DS].astype(np.float64), xc[:, D_SSM + DS:].astype(np.float64)
    dt = _dt32(inp)
    A, D = _np32(inp.A), _np32(inp.D)
    G = (C @ B.T).astype(f32)
    tril = np.tril(np.ones((T, T), bool))
    y, st = np.empty((T, NH, HD), f32), np.empty((NH, HD, DS), f32)

    def split(m):
        hi = _bf_np(m)
        lo = np.zeros_like(hi) if drop_lo else _bf_np(m - hi)
        return hi.astype(np.float64), lo.astype(np.float64)
    for h in range(NH):
        if cum64:
            cum = np.cumsum(A[h].astype(np.float64) * dt[:, h].astype(np.float64))
        else:
            cum, run = np.empty(T, f32), f32(0)
            for t in range(T):
                run = f32(run + A[h] * dt[t, h])
                cum[t] = run
        with np.errstate(all="ignore"):
            dec = np.exp((cum[:, None] - cum[None, :]).astype(f32))
            m = np.where(tril, (G * dec) * dt[None, :, h], f32(0)).astype(f32)
            hi, lo = split(m)
            y[:, h] = (hi @ x[:, h] + lo @ x[:, h]).astype(f32) + x[:, h].astype(f32) * D[h]
            wdec = np.exp((cum[T - 1] - cum).astype(f32)) * dt[:, h]
            hi, lo = split((wdec[:, None] * x[:, h].astype(f32)).astype(f32))
            st[h] = (hi.T @ B + lo.T @ B).astype(f32)
    return _out(y.reshape(T, D_SSM), round_out), _out(st, round_out)
