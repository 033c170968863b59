"""Crafted launches of zmi_prefix_condition (csrc/zmi_cond.hip), their reference and the criterion. No GPU library is
imported here: tests/test_cond_cases_cpu.py judges this module on the CPU, tests/test_gpu_cond_probe.py runs the kernel.

A `Launch` is what the C entry point takes, on the host: a parameter block (two entries per conditioner, the second
one the learned unconditional vector), a row table of (param, kind, index, x_off), the fp32 input vector, the LayerNorm
parameters and eps. `launch(d, eps)` mixes all five row kinds in a seeded, permuted order; each row carries a tag
naming the regime it is there for.

Reference. The kernel header states every rounding point, the library is built without fp contraction and its sums
over in_dim are sequential fp32 in index order, so the pre-LayerNorm row v is reproduced exactly in float32 here
(`row_v`), apart from cos / sin: those are evaluated in fp64 and rounded to bf16, and `launch` re-draws every Fourier
weight row for which that rounding could depend on the libm (`trig_unsafe`: the fp64 value within 2^-12 relative of a
bf16 rounding boundary, or of magnitude below 2^-8; rows with f == 0 exactly are exempt: cos 0 = 1 and sin 0 = 0 in
any libm). The LayerNorm is then evaluated in fp64 on v (`reference`).

Criterion: tests/test_conditioning.py::assert_bf16_close against the fp64 result rounded to bf16 (every element
within one bf16 ulp, floor 2^-20; at least 98 % bit-identical), and bit equality with ln_b on the zero-variance rows.

`emulate` restates the whole kernel in float32 (the LayerNorm in the kernel's ownership j = t + 256 i, a tree within
the wave, the four waves in order); it has to meet the criterion on every launch, which is the condition on the
inputs, and its four mutants have to miss it.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

EMBED, VECTOR, FOURIER, LINEAR, PASSTHROUGH = range(5)  # _lib.COND_*
KIND_NAMES = ("embed", "vector", "fourier", "linear", "passthrough")
NT, MAXD = 256, 4096
WIDTHS = (2, 8, 254, 256, 258, 510, 1026, 2048, 4094, 4096)
REFUSED_WIDTHS = (0, 3, 4098)
EPS = (1e-5, 1e-3)
MUTANTS = ("onepass", "s_unrounded", "sin_wj", "drop256")
GUARD_ROWS = 2
F32, F64 = np.float32, np.float64
TWO_PI = F32(6.2831855)


# ----------------------------------------------------------------------------- bf16 on numpy
def bf(x):
    """float32 -> float32 holding the nearest-even bf16 value (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(F32)


def bf64(x):
    """float64 -> float64 holding the nearest-even bf16 value, rounded once (no detour through float32)."""
    x = np.asarray(x, dtype=F64)
    _, e = np.frexp(x)
    q = np.ldexp(1.0, np.maximum(e, -125) - 8)
    return np.rint(x / q) * q


def bits(x) -> np.ndarray:
    """bf16-valued float array -> its uint16 bit patterns."""
    x = np.ascontiguousarray(x, dtype=F32)
    assert np.array_equal(bf(x), x), "not bf16 values"
    return (x.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def to_torch_bf16(x) -> torch.Tensor:
    return torch.from_numpy(bits(x).view(np.int16).copy()).view(torch.bfloat16).reshape(np.shape(x))


def from_torch_bf16(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().float().numpy().astype(F32)


def bf16_ulp(x):
    """One bf16 ulp at |x| (float64), floored at 2^-20 as the criterion does."""
    mag = np.maximum(np.abs(np.asarray(x, dtype=F64)), 2.0 ** -20)
    return np.maximum(np.exp2(np.floor(np.log2(mag)) - 7), 2.0 ** -20)


# ----------------------------------------------------------------------------- the launch
@dataclass
class Param:
    """One ZmiCondParam on the host; bf16-valued float32 arrays, or None for a NULL pointer."""
    table: np.ndarray | None = None   # [n, d] (embed) or [d] (vector)
    weight: np.ndarray | None = None  # [d / 2, in_dim] (fourier) or [d, in_dim] (linear)
    bias: np.ndarray | None = None    # [d]
    in_dim: int = 0
    min_val: float = 0.0
    max_val: float = 1.0
    spill: np.ndarray | None = None   # what the sin_wj mutant finds behind a Fourier weight (never sent to the GPU)


@dataclass
class Launch:
    d: int
    eps: float
    params: list
    rows: list                        # (param, kind, index, x_off)
    x: np.ndarray                     # float32
    ln_w: np.ndarray
    ln_b: np.ndarray
    tags: list = field(default_factory=list)

    def only(self, r: int) -> "Launch":
        return Launch(self.d, self.eps, self.params, [self.rows[r]], self.x, self.ln_w, self.ln_b, [self.tags[r]])


def _rng(*key):
    return np.random.default_rng([0xC0D, *key])


def _randbf(g, shape, scale=1.0):
    return bf((g.standard_normal(shape) * scale).astype(F32))


def table_row(i: int, d: int) -> np.ndarray:
    """Embedding row i as a function of i: a wrong index or a wrong row stride gives another row's values."""
    j = np.arange(d)
    return bf(((i + 1) * 0.5 + ((j * 7 + i * 13) % 64) / 32.0 - 1.0).astype(F32) * F32(1 - 2 * (i & 1)))


def outlier_at(d: int) -> int:
    return 256 if d > 256 else d - 1


# rows of the regime table, by index (0 and the last one are table_row: first and last table index)
TABLE = ("first", "const", "pm128", "outlier", "tiny", "last")


def _regime(name: str, d: int, g) -> np.ndarray:
    if name == "const":       # zero variance: out == ln_b exactly (sums of 3.0 are exact up to 4096 terms)
        return np.full(d, 3.0, dtype=F32)
    if name == "pm128":       # 128 +- one bf16 step (0.5 below 128, 1 above): a large mean with a small spread
        return np.where(g.integers(0, 2, d) == 1, F32(129.0), F32(127.5)).astype(F32)
    if name == "outlier":     # one outlier among zeros (at column 256 where the row has one)
        v = np.zeros(d, dtype=F32)
        v[outlier_at(d)] = 100.0
        return v
    if name == "tiny":        # |v| ~ 2^-10: variance ~ 1e-6, far below eps
        return bf((g.uniform(1.0, 2.0, d) * 2.0 ** -10 * g.choice([-1.0, 1.0], d)).astype(F32))
    raise KeyError(name)


def passthrough_ties(d: int, g) -> np.ndarray:
    """fp32 values that are not bf16 values: exact ties between two neighbouring bf16 values, and the fp32 numbers
    next to each tie on either side."""
    lo = bf((g.standard_normal(d) * 2).astype(F32) + F32(0.01))
    lo = np.where(lo == 0, F32(1.0), lo)
    hi = (lo.view(np.uint32) + np.uint32(0x10000)).view(F32)      # the next bf16 value away from zero
    tie = ((lo.astype(F64) + hi.astype(F64)) / 2).astype(F32)     # exact: one more mantissa bit
    out = tie.copy()
    k = np.arange(d) % 3
    out[k == 1] = np.nextafter(tie[k == 1], F32(0))
    out[k == 2] = np.nextafter(tie[k == 2], np.sign(tie[k == 2]) * F32(np.inf))
    return out


def fourier_f(p: Param, xin: np.ndarray, mode: str = "ok") -> np.ndarray:
    """f[jj], jj < d / 2, of one Fourier row, with the kernel's roundings (bf16-valued float32)."""
    xn = bf((xin.astype(F32) - F32(p.min_val)) / (F32(p.max_val) - F32(p.min_val)))
    s = TWO_PI * xn
    if mode != "s_unrounded":
        s = bf(s)
    acc = np.zeros(p.weight.shape[0], dtype=F32)
    for k in range(p.in_dim):
        acc = acc + s[k] * p.weight[:, k]
    return bf(acc)


def trig_unsafe(f: np.ndarray) -> np.ndarray:
    """Per jj: cos or sin of f (fp64) lies within 2^-12 relative of a bf16 rounding boundary, or is below 2^-8 in
    magnitude, so that a libm error could change the bf16 result. f == 0 is exempt."""
    bad = np.zeros(f.shape, dtype=bool)
    for fn in (np.cos, np.sin):
        c = np.abs(fn(f.astype(F64)))
        _, e = np.frexp(c)
        ulp = np.ldexp(1.0, e - 8)
        frac = c / ulp - np.floor(c / ulp)
        bad |= (np.abs(frac - 0.5) * ulp <= 2.0 ** -12 * c) | (c < 2.0 ** -8)
    return bad & (f != 0)


def row_v(L: Launch, r: int, mode: str = "ok") -> np.ndarray:
    """The pre-LayerNorm row (bf16-valued float32), with the kernel's roundings; cos / sin from fp64."""
    pi, kind, index, x_off = L.rows[r]
    p, d = L.params[pi], L.d
    if kind == EMBED:
        return p.table[index].copy()
    if kind == VECTOR:
        return p.table.copy()
    if kind == PASSTHROUGH:
        return bf(L.x[x_off:x_off + d])
    if kind == FOURIER:
        h = d // 2
        f = fourier_f(p, L.x[x_off:x_off + p.in_dim], mode)
        fs = f
        if mode == "sin_wj":  # the sine half reads w[j] instead of w[j - d / 2]: whatever lies behind the weight
            q = Param(weight=p.spill, in_dim=p.in_dim, min_val=p.min_val, max_val=p.max_val)
            fs = fourier_f(q, L.x[x_off:x_off + p.in_dim])
        return np.concatenate([bf64(np.cos(f.astype(F64))), bf64(np.sin(fs.astype(F64)))]).astype(F32)
    if kind == LINEAR:
        xs = bf(L.x[x_off:x_off + p.in_dim])
        acc = np.zeros(d, dtype=F32)
        for k in range(p.in_dim):
            acc = acc + xs[k] * p.weight[:, k]
        return bf(acc + (p.bias if p.bias is not None else F32(0)))
    raise ValueError(kind)


def all_v(L: Launch, mode: str = "ok") -> np.ndarray:
    return np.stack([row_v(L, r, mode) for r in range(len(L.rows))]) if L.rows else np.zeros((0, L.d), dtype=F32)


def reference(L: Launch, v: np.ndarray | None = None) -> np.ndarray:
    """fp64 LayerNorm of v: [n_rows, d] float64, not rounded."""
    v = (all_v(L) if v is None else v).astype(F64)
    mean = v.mean(axis=1, keepdims=True)
    var = ((v - mean) ** 2).mean(axis=1, keepdims=True)
    return (v - mean) / np.sqrt(var + F64(F32(L.eps))) * L.ln_w.astype(F64) + L.ln_b.astype(F64)


def fp32_unsafe(L: Launch, v: np.ndarray | None = None) -> np.ndarray:
    """[n_rows, d] bool: elements whose bf16 rounding any fp32 LayerNorm may miss. y = (v rstd - mean rstd) w + b in
    fp32 carries an absolute error of about E = 2^-23 ((|v| + |mean|) rstd |w| + |b|), half an fp32 ulp of each term
    twice over. Where the terms cancel, or where the mean is hundreds of deviations (pm128: |mean| rstd = 170), E is
    no longer small against the output's bf16 ulp (floored as in the criterion); `launch` re-draws ln_b[j] until
    E <= ulp / 16 on every row. The zero-variance rows are exempt: v rstd and mean rstd are the same fp32 number
    there and the output is ln_b exactly."""
    v = all_v(L) if v is None else v
    bad = fp32_err(L, v) > bf16_ulp(reference(L, v)) / 16
    bad[[t.endswith("const") for t in L.tags]] = False
    return bad


def fp32_err(L: Launch, v: np.ndarray) -> np.ndarray:
    """E of fp32_unsafe, per element."""
    v = v.astype(F64)
    mean = v.mean(axis=1, keepdims=True)
    rstd = 1 / np.sqrt(((v - mean) ** 2).mean(axis=1, keepdims=True) + F64(F32(L.eps)))
    return 2.0 ** -23 * ((np.abs(v) + np.abs(mean)) * rstd * np.abs(L.ln_w.astype(F64)) + np.abs(L.ln_b.astype(F64)))


def boundary_distance(y: np.ndarray) -> np.ndarray:
    """Distance of float64 y to the nearest bf16 rounding boundary (the midpoint of two neighbouring bf16 values)."""
    _, e = np.frexp(y)
    ulp = np.ldexp(1.0, e - 8)
    frac = np.abs(y) / ulp
    return np.abs(frac - np.floor(frac) - 0.5) * ulp


def _block_sum(a: np.ndarray) -> np.ndarray:
    """[n, d] float32 -> [n] float32 in the kernel's shape: thread t adds its j = t + 256 i in order, a tree within
    each wave of 64, the four waves ((0 + 1) + 2) + 3."""
    n, d = a.shape
    pad = np.zeros((n, MAXD), dtype=F32)
    pad[:, :d] = a
    pad = pad.reshape(n, MAXD // NT, NT)
    t = np.zeros((n, NT), dtype=F32)
    for i in range(MAXD // NT):
        t = t + pad[:, i]
    w = t.reshape(n, 4, 64)
    while w.shape[-1] > 1:
        w = w[..., 0::2] + w[..., 1::2]
    w = w[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def emulate(L: Launch, mode: str = "ok") -> np.ndarray:
    """The kernel in float32, or one of MUTANTS: bf16-valued float32 [n_rows, d]."""
    v = all_v(L, mode)
    d = F32(L.d)
    sv = v.copy()
    if mode == "drop256" and L.d > 256:
        sv[:, 256] = 0
    mean = (_block_sum(sv) / d)[:, None]
    if mode == "onepass":
        var = _block_sum(v * v) / d - mean[:, 0] * mean[:, 0]
    else:
        c = v - mean
        var = _block_sum(c * c) / d
    with np.errstate(invalid="ignore", divide="ignore"):
        rstd = (F32(1.0) / np.sqrt(var + F32(L.eps), dtype=F32))[:, None]
    y = v * rstd + -mean * rstd
    with np.errstate(invalid="ignore"):
        return bf(np.nan_to_num(y * L.ln_w + L.ln_b, nan=1e30, posinf=1e30, neginf=-1e30).astype(F32))


def judge(got: np.ndarray, L: Launch) -> dict:
    """Figures of one launch's output against the fp64 reference: the worst |got - ref| / ulp (ref not rounded), the
    bit-identical share against the rounded reference, and the failures of the exact rows."""
    ref = reference(L)
    want = bf64(ref)
    out = {"worst": 0.0, "same": 1.0, "exact_bad": []}
    if got.size:
        out["worst"] = float((np.abs(got.astype(F64) - ref) / bf16_ulp(np.maximum(np.abs(ref), np.abs(got)))).max())
        out["same"] = float((got.astype(F64) == want).mean())
    for r, tag in enumerate(L.tags):
        if tag.endswith("const") and not np.array_equal(got[r], L.ln_b):
            out["exact_bad"].append(r)
    return out


def check(got: np.ndarray, L: Launch) -> dict:
    """The criterion: assert_bf16_close against the rounded fp64 reference, bit equality on the exact rows."""
    from tests.test_conditioning import assert_bf16_close
    fig = judge(got, L)
    assert fig["exact_bad"] == [], f"zero-variance rows {fig['exact_bad']} are not ln_b"
    if got.size:
        assert_bf16_close(torch.from_numpy(got.astype(F32)), torch.from_numpy(bf64(reference(L)).astype(F32)))
    return fig


def passes(got: np.ndarray, L: Launch) -> bool:
    try:
        check(got, L)
    except AssertionError:
        return False
    return True


# ----------------------------------------------------------------------------- the mixed launch
X_PAD = 4097  # the passthrough inputs start at an odd, large x_off


def launch(d: int, eps: float = 1e-5, seed: int = 0) -> Launch:
    """All five kinds in one launch at width d. Parameter entries (even: conditional, odd: learned vector):
    0 regime table; 2 / 4 / 6 Fourier with in_dim 1 / 8 / 256; 8 / 10 / 12 linear with in_dim 1 / 128 (NULL bias) /
    256 (alternating large weights); 14 plain passthrough; 1 / 3 / 5 vectors (random, pm128, const)."""
    assert d % 2 == 0 and 0 < d <= MAXD
    g = _rng(d, seed)
    h = d // 2
    n_tab = len(TABLE)
    tab = np.stack([table_row(i, d) if name in ("first", "last") else _regime(name, d, g)
                    for i, name in enumerate(TABLE)])
    P = [Param() for _ in range(16)]
    P[0] = Param(table=tab)
    P[1] = Param(table=_randbf(g, d))
    P[3] = Param(table=_regime("pm128", d, g))
    P[5] = Param(table=_regime("const", d, g))
    # Fourier: weights scaled so that |f| reaches about 200 rad
    P[2] = Param(in_dim=1, min_val=0.0, max_val=24000.0, weight=_randbf(g, (h, 1), 12.0))
    P[4] = Param(in_dim=8, min_val=-1.5, max_val=2.5, weight=_randbf(g, (h, 8), 4.0))
    P[6] = Param(in_dim=256, min_val=0.25, max_val=1.25, weight=_randbf(g, (h, 256), 1.0))
    # linear
    P[8] = Param(in_dim=1, weight=_randbf(g, (d, 1)), bias=_randbf(g, d))
    P[10] = Param(in_dim=128, weight=_randbf(g, (d, 128), 0.1), bias=None)
    # +A, small, -A, small, ... with A ~ 2^17 and inputs that round to the same bf16 value within each +-A pair: the
    # exact sum is that of the small terms, and what fp32 leaves of it depends on the order of the additions
    w12 = _randbf(g, (d, 256))
    big = bf((g.uniform(1, 2, (d, 64)) * 2.0 ** 17).astype(F32))
    w12[:, 0::4], w12[:, 2::4] = big, -big
    P[12] = Param(in_dim=256, weight=w12, bias=_randbf(g, d))
    P[14] = Param(in_dim=d)

    x = [g.standard_normal(X_PAD).astype(F32)]  # rows never read the pad at the front
    n_x = X_PAD
    rows, tags = [], []

    def add(param, kind, index, vals, tag):
        nonlocal n_x
        off = 0
        if vals is not None:
            off = n_x
            vals = np.asarray(vals, dtype=F32).reshape(-1)
            x.append(vals)
            n_x += vals.size
        rows.append((param, kind, index, off))
        tags.append(tag)

    add(14, PASSTHROUGH, 0, passthrough_ties(d, g), "passthrough/ties")
    for i, name in enumerate(TABLE):
        add(0, EMBED, i, None, f"embed/{name}")
    for pi, name in ((1, "random"), (3, "pm128"), (5, "const")):
        add(pi, VECTOR, 0, None, f"vector/{name}")
    add(14, PASSTHROUGH, 0, (g.standard_normal(d) * 3).astype(F32), "passthrough/random")
    for xv, name in ((0.0, "min"), (24000.0, "max"), (-3000.0, "below"), (31000.5, "above"), (22050.0, "inside")):
        add(2, FOURIER, 0, [xv], f"fourier1/{name}")
    add(4, FOURIER, 0, g.uniform(-1.5, 2.5, 8), "fourier8/inside")
    add(4, FOURIER, 0, [-1.5, 2.5, -2.0, 3.25, 0.3077, 0.0256, -1.5, 2.5], "fourier8/edges")
    add(6, FOURIER, 0, g.uniform(0.25, 1.25, 256), "fourier256/inside")
    add(8, LINEAR, 0, [g.standard_normal() * 1.7 + 0.123], "linear1/bias")
    add(10, LINEAR, 0, g.standard_normal(128) * 0.3, "linear128/nobias")
    x12 = (1.0 + g.standard_normal(256) * 2.0 ** -6).astype(F32)
    pair = bf(g.uniform(0.5, 2.0, 64).astype(F32))
    x12[0::4], x12[2::4] = pair * F32(1 + 2.0 ** -10), pair * F32(1 - 2.0 ** -10)
    add(12, LINEAR, 0, x12, "linear256/alternating")

    # the condition on the Fourier weights: re-draw every row whose cos / sin rounding could depend on the libm
    xcat = np.concatenate(x)
    for pi in (2, 4, 6):
        p = P[pi]
        users = [r for r in rows if r[0] == pi]
        for _ in range(200):
            bad = np.zeros(h, dtype=bool)
            for (_, _, _, off) in users:
                bad |= trig_unsafe(fourier_f(p, xcat[off:off + p.in_dim]))
            if not bad.any():
                break
            p.weight[bad] = _randbf(g, (int(bad.sum()), p.in_dim), {2: 12.0, 4: 4.0, 6: 1.0}[pi])
        else:
            raise AssertionError(f"Fourier weights of param {pi} at d {d} did not settle")
        p.spill = _randbf(g, (h, p.in_dim), {2: 12.0, 4: 4.0, 6: 1.0}[pi])

    order = g.permutation(len(rows))
    rows, tags = [rows[i] for i in order], [tags[i] for i in order]
    ln_w = bf((g.uniform(0.5, 2.0, d) * g.choice([-1.0, 1.0], d)).astype(F32))
    draw_b = lambda n: bf((np.exp2(g.uniform(-6.0, 6.0, n)) * g.choice([-1.0, 1.0], n)).astype(F32))  # noqa: E731
    ln_b = draw_b(d)
    ln_b[g.integers(0, d)] = 64.0
    L = Launch(d, eps, P, rows, xcat, ln_w, ln_b, tags)
    v = all_v(L)
    for _ in range(200):  # the condition on ln_b (fp32_unsafe)
        bad = fp32_unsafe(L, v).any(axis=0)
        if not bad.any():
            return L
        L.ln_b[bad] = draw_b(int(bad.sum()))
    raise AssertionError(f"ln_b at d {d} did not settle")


# ----------------------------------------------------------------------------- launches from a conditioner list
def oracle_conditioners() -> list:
    """The v0.1 conditioner list and one un-projected passthrough: every kind, expressible for the CPU oracle."""
    from zonos_vibes_amd.conditioning import v01_transformer_conditioners
    return v01_transformer_conditioners() + [{"type": "PassthroughConditioner", "name": "plain",
                                              "uncond_type": "learned"}]


def launch_from_conditioner(pc, cond_dict: dict) -> Launch:
    """The Launch that PrefixConditioner `pc` (on the CPU, weights loaded) makes of cond_dict: its _rows, and its
    parameter block with host arrays in the place of device pointers."""
    rows, xs = [], []
    pc._rows(cond_dict, rows, xs)
    P = []
    for i, c in enumerate(pc.cfgs):
        pre, t = f"conditioners.{i}.", c["type"]
        w = lambda n: from_torch_bf16(pc.w[pre + n])  # noqa: E731
        p = Param(min_val=float(c.get("min_val", 0.0)), max_val=float(c.get("max_val", 1.0)))
        if t == "EspeakPhonemeConditioner":
            p.table = w("phoneme_embedder.weight")
        elif t == "IntegerConditioner":
            p.table = w("int_embedder.weight")
        elif t == "FourierConditioner":
            p.weight, p.in_dim = w("weight"), c.get("input_dim", 1)
        else:
            p.in_dim = c.get("cond_dim") or pc.d
            if c.get("projection", "none") == "linear":
                p.weight, p.bias = w("project.weight"), w("project.bias")
        P += [p, Param(table=w("uncond_vector")) if c.get("uncond_type", "none") == "learned" else Param()]
    return Launch(pc.d, pc.eps, P, [tuple(r) for r in rows], np.asarray(xs if xs else [0.0], dtype=F32),
                  from_torch_bf16(pc.w["norm.weight"]), from_torch_bf16(pc.w["norm.bias"]),
                  [KIND_NAMES[r[1]] for r in rows])
