"""Shared, CPU-only pieces of the sampler probe tests (test_sampler_cases_cpu.py, test_gpu_sampler_probe.py).

The sampler returns one token per row and no probabilities, but it takes the exponential race's noise q from the
caller, and argmax(p / q) with a crafted q reads its final probabilities p exactly:

  support probe  q = +inf everywhere except q[v] = 1: every other score is p / inf = 0, so token v wins iff p[v] > 0
                 (otherwise the whole row scores 0 and index 0 wins). Column 0 cannot be probed, so every input row
                 carries its maximum at column 0: the lowest-index maximum, which every filter keeps.
  ratio probe    q[0] = 1, q[b] = rho, everything else +inf: token b wins iff p[b] / rho > p[0]. Two rows per pair,
                 rho = R64 (1 -+ tol), bracket the sampler's p[b] / p[0]; renormalisation cancels in the ratio.

This module holds the inputs, an fp64 restatement of the reference's sampling.py:29-96,164-178 that also returns each
filter's decision margin, the probe builders and decoders, the parameter cases, and a numpy restatement of the
sampler's internal counter-hash noise with the inverse of mix64.
"""
import math

import numpy as np
import torch

from oracle import zonos_cpu as oz
from tests.helpers import load_golden
from zonos_vibes_amd.synthetic import GOLDEN, _mix64_np, mix64

NV, NCB, EOS = 1026, 9, 1024
INF = float("inf")
_M64 = (1 << 64) - 1

BAND = 2.0 ** -16    # a top-p token is "don't care" when its exclusive cumulative sum is this close to top_p
BAND_CAP = 4         # at most this many band tokens per row, and none for top_p <= 0.8
TOL_FLOOR = 2.0 ** -20
TOL_FACTOR = 8.0


def f32(x):
    """The value a float parameter has once it sits in the sampler's fp32 parameter block."""
    return float(np.float32(x))


# ----------------------------------------------------------------------------- inputs
def grid_logits(seed=0):
    """[9, 1026] on a 1/8 grid in [-8, 8]: distinct logits differ by >= 0.125 (never one fp32 probability), every
    value has ~8 exact ties, column 0 carries the maximum, column 1025 is -inf, column 1024 is -inf on codebooks 1..8.
    The seed is one whose fp64 restatement meets the band cap (about half of the seeds do; check_band_cap asserts
    it)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-64, 65, (NCB, NV), generator=g).float() / 8
    x[:, 0] = 8.0
    x[:, 1025] = -INF
    x[1:, 1024] = -INF
    return x


def fixture_logits(batch=1):
    """The bf16-valued logits of the `samplers` fixture (about 340 duplicated values per row) with column 0 raised
    to the row maximum. Batch elements 1 and 2 meet the band cap; element 0 has one band token at top_p 0.3."""
    t, _ = load_golden("samplers")
    x = t["logits"][batch].clone().float()
    x[:, 1025] = -INF
    x[:, 0] = x.max(dim=-1).values
    return x


def decode_logits(seed=21):
    """(cond, uncond) [9, 1026] for the decode step at cfg_scale 2: both on the 1/8 grid, so u + (c - u) * 2 is exact
    in fp32 and the guided logits are again a 1/8 grid with many ties. Column 0 is the guided maximum; column 1024
    ties with it on every codebook, so only the EOS bias can drop it on codebooks 1..8."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(-56, 57, (NCB, NV), generator=g).float() / 8
    u = c - torch.randint(-8, 9, (NCB, NV), generator=g).float() / 8
    for col in (0, EOS):
        c[:, col] = 8.0
        u[:, col] = 8.0  # guided 8.0 = the largest value 2 c - u can take elsewhere (7 + 1)
    return c, u


def guided_logits(c, u, cfg_scale=2.0, decode=True):
    """model.py:112-115,266-267,280 in fp64: CFG, the padding column, the EOS bias on codebooks 1..8."""
    lg = u.double() + (c.double() - u.double()) * f32(cfg_scale)
    lg[..., 1025] = -INF
    if decode:
        lg[..., 1:, EOS] = -INF
    return lg


# ----------------------------------------------------------------------------- fp64 restatement
MUTATIONS = {  # name -> the filter it changes (a case that does not run that filter cannot see it)
    "top_p_drops_crossing": "top_p", "top_p_keeps_one_more": "top_p", "top_p_fp32_sequential": "top_p",
    "ties_higher_index_first": "top_p", "min_p_le": "min_p", "top_k_plus_1": "top_k", "top_k_minus_1": "top_k",
    "top_k_le_pivot": "top_k"}


def _sort_desc(p, mut=None):
    """Stable descending sort: the lower index first among equals (the kernel's keys encode exactly that)."""
    if mut == "ties_higher_index_first":
        srt, idx = torch.sort(p.flip(-1), dim=-1, descending=True, stable=True)
        return srt, p.shape[-1] - 1 - idx
    return torch.sort(p, dim=-1, descending=True, stable=True)


def restate(logits, temperature=1.0, top_p=0.0, top_k=0, min_p=0.0, linear=0.0, conf=0.0, quad=0.0, generated=None,
            repetition_penalty=1.0, repetition_penalty_window=2, mut=None):
    """sampling.py:29-96,164-178 in fp64 on logits [..., V] (float parameters as their fp32 values). Returns a dict:
    `probs` (final, per token), `base` (before the filters: equal entries are the exact ties) and per filter its
    decision margin: `top_p` = exclusive cumulative sum - top_p (dropped iff > 0), `top_k` = 0-based rank in the
    stable descending order, `min_p` = p / (min_p * max) (dropped iff < 1). `mut` applies one of MUTATIONS."""
    lg = logits.double()
    if repetition_penalty != 1.0 and generated is not None:
        recent = generated[..., -repetition_penalty_window:].clamp_max(lg.shape[-1] - 1).to(torch.int64)
        fac = torch.ones_like(lg).scatter_reduce(-1, recent, torch.full_like(lg, f32(repetition_penalty)),
                                                 reduce="prod")
        lg = torch.where(lg <= 0, lg * fac, lg / fac)
    p = torch.softmax(lg / f32(temperature), dim=-1)
    if linear > 0.0:
        lp = torch.log(p.clamp_min(f32(1e-20)))
        ent = -torch.sum(p * lp, dim=-1, keepdim=True)
        p = torch.softmax(lp * (f32(linear) + ent * f32(conf)) - lp ** 2 * f32(quad), dim=-1)
    out = {"base": p.clone()}
    if top_p > 0:
        srt, idx = _sort_desc(p, mut)
        if mut == "top_p_fp32_sequential":
            csum = torch.from_numpy(np.cumsum(srt.float().numpy(), axis=-1, dtype=np.float32)).double()
            excl = (csum.float() - srt.float()).double()
        else:
            excl = torch.cumsum(srt, dim=-1) - srt
        drop = excl > f32(top_p)
        if mut == "top_p_drops_crossing":
            drop = excl + srt > f32(top_p)
        elif mut == "top_p_keeps_one_more":
            drop = torch.cat([torch.zeros_like(drop[..., :1]), drop[..., :-1]], dim=-1)
        out["top_p"] = torch.zeros_like(p).scatter(-1, idx, excl - f32(top_p))
        p = p.scatter(-1, idx, srt * (~drop).double())
        p = p / p.sum(dim=-1, keepdim=True)
    if top_k > 0:
        srt, idx = _sort_desc(p, mut)
        k = min(top_k, p.shape[-1])
        k = {"top_k_plus_1": min(k + 1, p.shape[-1]), "top_k_minus_1": max(k - 1, 1)}.get(mut, k)
        pivot = srt[..., k - 1:k]
        rank = torch.arange(p.shape[-1]).expand(p.shape).contiguous()
        out["top_k"] = torch.zeros(p.shape, dtype=torch.int64).scatter(-1, idx, rank)
        p = torch.where((p <= pivot) if mut == "top_k_le_pivot" else (p < pivot), 0.0, p)
        p = p / p.sum(dim=-1, keepdim=True)
    if min_p > 0:
        thr = f32(min_p) * p.max(dim=-1, keepdim=True).values
        out["min_p"] = p / thr
        p = p.masked_fill((p <= thr) if mut == "min_p_le" else (p < thr), 0.0)
        p = p / p.sum(dim=-1, keepdim=True)
    out["probs"] = p
    return out


def oracle_probs32(logits, temperature=1.0, top_p=0.0, top_k=0, min_p=0.0, linear=0.0, conf=0.0, quad=0.0,
                   generated=None, repetition_penalty=1.0, repetition_penalty_window=2):
    """The fp32 probabilities oracle.zonos_cpu.sample() races: its own functions, in its own order."""
    lg = logits.float()
    if repetition_penalty != 1.0 and generated is not None:
        lg = oz.repetition_penalty(lg.unsqueeze(0), generated.unsqueeze(0), repetition_penalty,
                                   repetition_penalty_window)[0]
    p = torch.softmax(lg / temperature, dim=-1)
    if linear > 0.0:
        p = oz.unified(p, linear, conf, quad)
    if top_p > 0:
        p = oz.top_p(p, top_p)
    if top_k > 0:
        p = oz.top_k(p, top_k)
    if min_p > 0:
        p = oz.min_p(p, min_p)
    return p


def band_mask(r, top_p):
    """Tokens whose top-p decision is within BAND of the threshold: their fate is rounding, in the reference too.
    The first token of the order is never one: its exclusive sum is exactly 0 in any precision (top_p = 1e-6)."""
    if top_p <= 0:
        return torch.zeros(r["probs"].shape, dtype=torch.bool)
    return (r["top_p"].abs() <= BAND) & (r["base"] > 0) & (r["top_p"] != -f32(top_p))


def check_band_cap(band, top_p):
    """The cap on the restatement's own band, asserted before any sampler is looked at."""
    per_row = band.sum(dim=-1)
    assert int(per_row.max()) <= BAND_CAP, per_row.tolist()
    if 0 < top_p <= 0.8:
        assert int(per_row.sum()) == 0, per_row.tolist()
    return per_row.tolist()


# ----------------------------------------------------------------------------- parameter cases
def _kept_cases():
    cases = []
    for t in (0.7, 1.0, 1.3):
        for p in (1e-6, 0.3, 0.8, 0.95, 0.999):
            cases.append((f"top_p{p:g}_T{t:g}", dict(temperature=t, top_p=p)))
    for k in (1, 2, 30, 1024, 1025, 1026, 5000):
        cases.append((f"top_k{k}", dict(top_k=k)))
    for m in (0.05, 0.1, 0.5, 1.0):
        cases.append((f"min_p{m:g}", dict(min_p=m)))
    cases += [
        ("top_p0.3_top_k50", dict(top_p=0.3, top_k=50)),  # top-p leaves fewer than k: the pivot is 0, nothing goes
        ("top_p0.95_top_k30", dict(top_p=0.95, top_k=30)),
        ("top_k50_min_p0.1", dict(top_k=50, min_p=0.1)),
        ("T0.7_top_p0.95_min_p0.05", dict(temperature=0.7, top_p=0.95, min_p=0.05)),
        ("unified_top_k30", dict(linear=0.5, conf=0.4, quad=0.0, top_k=30)),
        ("penalty3_w2_top_p0.95", dict(top_p=0.95, repetition_penalty=3.0, repetition_penalty_window=2)),
    ]
    return cases


KEPT_CASES = _kept_cases()

RATIO_CASES = [
    ("T0.7", dict(temperature=0.7)),
    ("T1", dict(temperature=1.0)),
    ("T1.3", dict(temperature=1.3)),
    ("unified_.5_.4_0", dict(linear=0.5, conf=0.4, quad=0.0)),
    ("unified_.3_-.1_.25", dict(linear=0.3, conf=-0.1, quad=0.25)),
    ("penalty3_w2", dict(repetition_penalty=3.0, repetition_penalty_window=2)),
    ("filtered_top_p0.95_top_k50", dict(top_p=0.95, top_k=50)),  # filters leave the kept tokens' ratios alone
]


def penalty_history(logits):
    """[9, 3] generated tokens whose window of 2 repeats one token (factor penalty^2): per row a token of the
    second-highest logit value, never column 0, so that column 0 stays the row maximum."""
    top = logits[:, 0:1]
    second = torch.where(logits < top, logits, torch.full_like(logits, -INF)).max(dim=-1).values
    rep = torch.stack([torch.nonzero(logits[r] == second[r])[0, 0] for r in range(logits.shape[0])])
    other = (rep + 7) % 1000 + 1
    return torch.stack([other, rep, rep], dim=-1).to(torch.int64)


def case_kwargs(params, logits):
    """Keywords for restate() / oracle_probs32(): the case's parameters, plus the history where it has a penalty."""
    kw = dict(params)
    if kw.get("repetition_penalty", 1.0) != 1.0:
        kw["generated"] = penalty_history(logits)
    return kw


def oracle_sample_kwargs(kw):
    """The same case as keywords of oracle.zonos_cpu.sample()."""
    kw = dict(kw)
    gen = kw.pop("generated", None)
    out = oz.sample_params(kw)
    out.setdefault("rep_penalty", 1.0)
    out["generated"] = gen
    return out


# ----------------------------------------------------------------------------- probes
def support_noise(tokens=None):
    """[len(tokens), 9, 1026] fp32: batch element j probes token tokens[j] on all 9 codebook rows (default: every
    token, the whole kept set in one launch)."""
    tokens = torch.arange(NV) if tokens is None else torch.as_tensor(tokens)
    q = torch.full((len(tokens), NCB, NV), INF)
    q[torch.arange(len(tokens)), :, tokens] = 1.0
    return q


def decode_support(winners, tokens=None):
    """winners [len(tokens), 9] -> kept [9, len(tokens)] bool. A probe answers its own token (kept) or 0 (dropped);
    column 0 itself always reads as kept (it is the maximum, which every filter keeps)."""
    tokens = torch.arange(NV) if tokens is None else torch.as_tensor(tokens)
    w = torch.as_tensor(winners).reshape(len(tokens), NCB).long()
    t = tokens.view(-1, 1)
    assert bool(((w == t) | (w == 0)).all()), "a support probe answers its own token or 0"
    return (w == t).T.contiguous()


def ratio_tokens(p64, n=32):
    """[9, n] tokens per row spread over the ranks of the kept set (column 0 excluded), each with p / p[0] > 2^-20."""
    out = []
    for r in range(p64.shape[0]):
        ratio = p64[r] / p64[r, 0]
        order = torch.sort(p64[r], descending=True, stable=True).indices
        order = order[(order != 0) & (ratio[order] > TOL_FLOOR)]
        assert len(order) >= 2, "the ratio probe needs kept tokens besides column 0"
        pick = torch.linspace(0, len(order) - 1, n).round().long()
        out.append(order[pick])
    return torch.stack(out)


def ratio_noise(tokens, r64, tol):
    """[2 n, 9, 1026] fp32. Rows 0..n-1 carry rho = R64 (1 - tol): token b must win. Rows n..2n-1 carry
    rho = R64 (1 + tol): token 0 must win."""
    n = tokens.shape[1]
    q = torch.full((2 * n, NCB, NV), INF)
    q[:, :, 0] = 1.0
    cb = torch.arange(NCB)
    for j in range(n):
        q[j, cb, tokens[:, j]] = (r64[:, j] * (1 - tol)).float()
        q[n + j, cb, tokens[:, j]] = (r64[:, j] * (1 + tol)).float()
    return q


def ratio_failures(winners, tokens):
    """List of (row, token, side) where the bracket does not hold."""
    n = tokens.shape[1]
    w = torch.as_tensor(winners).reshape(2 * n, NCB).long()
    bad = []
    for j in range(n):
        for r in range(NCB):
            if int(w[j, r]) != int(tokens[r, j]):
                bad.append((r, int(tokens[r, j]), "p[b]/p[0] below R64 (1 - tol)"))
            if int(w[n + j, r]) != 0:
                bad.append((r, int(tokens[r, j]), "p[b]/p[0] above R64 (1 + tol)"))
    return bad


def ratio_tol(p32, p64, tokens):
    """(deviation, tol): the largest relative deviation of the fp32 CPU oracle's ratios from the fp64 restatement's on
    these pairs, and TOL_FACTOR times it with the floor 2^-20. Both from the CPU, never from the sampler under test."""
    r32 = torch.gather(p32.double(), -1, tokens) / p32[:, 0:1].double()
    r64 = torch.gather(p64, -1, tokens) / p64[:, 0:1]
    dev = float(((r32 - r64).abs() / r64).max())
    return dev, max(TOL_FACTOR * dev, TOL_FLOOR)


def race(p, q):
    """argmax(p / q) with the first index on ties: the race every sampler ends with, for restatements that return
    probabilities."""
    return torch.argmax(p / q.to(p.dtype), dim=-1)


def tie_groups(base_row):
    """Index lists of the exact ties of one row (equal fp64 pre-filter probability = equal logit), size >= 2."""
    vals, inv = torch.unique(base_row, return_inverse=True)
    order = torch.argsort(inv, stable=True)
    counts = torch.bincount(inv, minlength=len(vals))
    out, start = [], 0
    for c in counts.tolist():
        if c >= 2:
            out.append(order[start:start + c])
        start += c
    return out


def prefix_violations(kept_row, base_row):
    """Tie groups whose kept members are not a lowest-index prefix of the group."""
    bad = []
    for g in tie_groups(base_row):
        k = kept_row[g]
        n = int(k.sum())
        if not bool(k[:n].all()):
            bad.append(g.tolist())
    return bad


# ----------------------------------------------------------------------------- internal noise
_INV_M1 = pow(0xBF58476D1CE4E5B9, -1, 1 << 64)
_INV_M2 = pow(0x94D049BB133111EB, -1, 1 << 64)


def inv_mix64(z):
    """The inverse of synthetic.mix64: undo each xorshift (x ^= x >> s is undone by x ^ x >> s ^ x >> 2s ... while
    the shift stays below 64) and multiply by the modular inverses of the two odd constants."""
    z &= _M64
    z = z ^ (z >> 31) ^ (z >> 62)
    z = (z * _INV_M2) & _M64
    z = z ^ (z >> 27) ^ (z >> 54)
    z = (z * _INV_M1) & _M64
    z = z ^ (z >> 30) ^ (z >> 60)
    return z


def uniform_from_bits(z, clamp=True):
    """u = fl32(fl32(z >> 40) + 0.5) * 2^-24 in fp32. Without the clamp the all-ones draw gives exactly 1.0
    (16777215 + 0.5 rounds to 16777216), hence q = -log(1) = -0; the sampler clamps u to the largest fp32 below 1,
    which leaves every other draw's bits alone."""
    u = ((z >> np.uint64(40)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    return np.minimum(u, np.float32(1.0 - 2.0 ** -24)) if clamp else u


def ctr_base(cb, step=None, row=0):
    """The counter layout: ((step + 1) * 9 + cb) * 1026 in the decode step, cb * 1026 + row * 9 * 1026 standalone."""
    return ((step + 1) * NCB + cb) * NV if step is not None else cb * NV + row * NCB * NV


def hash_noise(seed, base, clamp=True):
    """q [1026] fp32 of one row: z = mix64(seed + GOLDEN (base + v + 1)), q = -log(u)."""
    with np.errstate(over="ignore"):
        ctr = np.uint64(base) + np.arange(1, NV + 1, dtype=np.uint64)
        z = _mix64_np(np.uint64(seed & _M64) + np.uint64(GOLDEN) * ctr)
    with np.errstate(divide="ignore"):
        return -np.log(uniform_from_bits(z, clamp))


def hash_noise_rows(seed, rows=None, step=None):
    """[rows, 9, 1026] standalone (row = batch index) or [9, 1026] for one decode step."""
    if step is not None:
        return torch.from_numpy(np.stack([hash_noise(seed, ctr_base(cb, step=step)) for cb in range(NCB)]))
    return torch.from_numpy(np.stack([np.stack([hash_noise(seed, ctr_base(cb, row=b)) for cb in range(NCB)])
                                      for b in range(rows)]))


def seed_for_all_ones_draw(base, v, low_bits=0x1234567890):
    """The seed whose draw at counter base + v + 1 has all 24 uniform bits set."""
    z = (0xFFFFFF << 40) | (low_bits & ((1 << 40) - 1))
    seed = (inv_mix64(z) - GOLDEN * (base + v + 1)) & _M64
    assert mix64((seed + GOLDEN * (base + v + 1)) & _M64) >> 40 == 0xFFFFFF
    return seed


def race_margin(p64, q):
    """(winner, relative gap between the two best race scores) per row, in fp64."""
    s = p64 / q.double()
    top = torch.topk(s, 2, dim=-1)
    return top.indices[..., 0], (top.values[..., 0] - top.values[..., 1]) / top.values[..., 0]


NOISE_MARGIN = 1e-4       # rows whose two best scores are closer than this are not compared (device logf ulps)
NOISE_MARGIN_ROWS = 0.01  # at most this fraction of the rows may fall under the margin


def spread_logits(seed=22, n_rows=64, n_kept=30):
    """[n_rows, 9, 1026]: about 30 tokens per row with probabilities spanning 100x, everything else -inf."""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((n_rows, NCB, NV), -INF)
    for b in range(n_rows):
        for cb in range(NCB):
            cols = torch.randperm(1025, generator=g)[:n_kept]
            x[b, cb, cols] = -torch.rand(n_kept, generator=g) * math.log(100.0)
    return x


EIGHT_PROBS = (0.4, 0.25, 0.15, 0.1, 0.05, 0.025, 0.015, 0.01)
EIGHT_COLS = (0, 3, 255, 256, 511, 700, 1023, 1024)  # all four waves, first and last columns of a thread
CHI2_7DF_1M6 = 40.5218  # the 1 - 1e-6 quantile of chi-square with 7 degrees of freedom


def eight_token_logits():
    x = torch.full((NV,), -INF)
    x[list(EIGHT_COLS)] = torch.log(torch.tensor(EIGHT_PROBS, dtype=torch.float64)).float()
    return x


def chi_square(tokens):
    """Pearson chi-square of drawn tokens against EIGHT_PROBS; every draw must be one of the 8 columns."""
    t = torch.as_tensor(tokens).flatten().long()
    counts = torch.bincount(t, minlength=NV).double()
    cols = list(EIGHT_COLS)
    assert int(counts.sum() - counts[cols].sum()) == 0, "a token of probability 0 was drawn"
    exp = torch.tensor(EIGHT_PROBS, dtype=torch.float64) * len(t)
    return float(((counts[cols] - exp) ** 2 / exp).sum())
