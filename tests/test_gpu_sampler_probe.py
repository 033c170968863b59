"""The stochastic half of sample_kernel, read through its noise argument (MI355X only).

tests/sampler_cases.py explains the two probes. Here they run on the HIP sampler (zmi_sample_logits, and the decode
step zmi_sample_step) against the fp64 restatement: the whole kept set of every filter at its edge, tie order,
probability ratios, the per-slot parameter blocks of a decode launch, the internal counter-hash noise draw for draw,
and the all-ones draw whose u rounded to 1.0.
"""
import ctypes

import pytest
import torch

from tests import sampler_cases as sc
from tests.test_gpu_kernels import _set_params, _slots

pytestmark = pytest.mark.gpu
DEV = "cuda"
NV, NCB = sc.NV, sc.NCB
INPUTS = {"grid": sc.grid_logits, "bf16": sc.fixture_logits}


def _lib():
    from zonos_vibes_amd import _lib as L
    return L


def _c_params(L, p, cfg_scale=1.0, seed=0):
    return L.Sampling(p.get("temperature", 1.0), p.get("top_p", 0.0), p.get("min_p", 0.0), p.get("linear", 0.0),
                      p.get("conf", 0.0), p.get("quad", 0.0), p.get("repetition_penalty", 1.0), cfg_scale,
                      int(p.get("top_k", 0)), int(p.get("repetition_penalty_window", 2)), seed & ((1 << 64) - 1))


def sample_logits(logits, params, noise=None, generated=None, seed=0):
    """zmi_sample_logits on device tensors: logits [B, 9, 1026] fp32, noise the same shape or None (internal hash
    noise from `seed`), generated [B, 9, G] int32 or None -> tokens [B, 9] int64 on the host."""
    L = _lib()
    prm = torch.tensor(bytearray(_c_params(L, params, seed=seed)), dtype=torch.uint8).to(DEV)
    b = logits.shape[0]
    assert logits.is_contiguous() and logits.dtype == torch.float32 and logits.shape[1:] == (NCB, NV)
    assert noise is None or (noise.is_contiguous() and noise.shape == logits.shape and noise.dtype == torch.float32)
    assert generated is None or (generated.is_contiguous() and generated.dtype == torch.int32)
    out = torch.full((b, NCB), -7, dtype=torch.int32, device=DEV)
    L.check(L.lib().zmi_sample_logits(logits.data_ptr(), L.ptr(generated), 0 if generated is None else
                                      generated.shape[-1], b, prm.data_ptr(), L.ptr(noise), out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), "sample_logits")
    torch.cuda.synchronize()
    return out.cpu().long()


def sample_step(cond, uncond, slot_params, noise=None, history=None, active=None, step=0):
    """One zmi_sample_step launch in decode mode over S slots. cond / uncond [S, 9, 1026] on the host, slot_params a
    list of (params dict, cfg_scale, seed), history [S, 9, G] tokens (the delayed frames before this one), active a
    list of 0 / 1. Returns (tokens [S, 9] int64 with -7 where nothing was written, slot state dict on the host)."""
    L = _lib()
    S = cond.shape[0]
    sl, st, delayed, params = _slots(S)
    rows = torch.empty(2 * S, NCB, NV)
    rows[0::2], rows[1::2] = cond, uncond
    rows = rows.to(DEV)
    g = 1
    if history is not None:
        g = history.shape[-1]
        delayed[:, :, :g] = history.to(DEV, torch.int32)
    st["active"][:] = torch.tensor([1] * S if active is None else active, dtype=torch.int32)
    st["offset"][:] = g - 1
    st["remaining"][:] = 100
    st["total_len"][:] = 64
    st["step"][:] = step
    for s, (p, cfg, seed) in enumerate(slot_params):
        _set_params(params, s, _c_params(L, p, cfg, seed))
    nxt = torch.full((S, NCB), -7, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(S, dtype=torch.int32, device=DEV)
    nz = None if noise is None else noise.to(DEV).contiguous()
    L.check(L.lib().zmi_sample_step(ctypes.byref(sl), rows.data_ptr(), L.ptr(nz), nxt.data_ptr(), cnt.data_ptr(), 0,
                                    0, S, None, 0, None, None, None, torch.cuda.current_stream().cuda_stream),
            "sample_step")
    torch.cuda.synchronize()
    return nxt.cpu().long(), {k: v.cpu() for k, v in st.items()}


@pytest.fixture(scope="module")
def inputs():
    """Per input set: the [9, 1026] logits on the host and their 1026 copies on the device (one per probed token)."""
    out = {}
    for k, f in INPUTS.items():
        x = f()
        out[k] = (x, x.unsqueeze(0).expand(NV, -1, -1).contiguous().to(DEV))
    return out


@pytest.fixture(scope="module")
def probe_q():
    return sc.support_noise().to(DEV)


def _describe(diff, r, params):
    """(row, token, margins) of the first few tokens whose kept / dropped status is not the restatement's."""
    out = []
    for row, v in torch.nonzero(diff).tolist()[:8]:
        out.append((row, v, {k: float(r[k][row, v]) for k in ("top_p", "top_k", "min_p") if k in r}))
    return out


@pytest.mark.parametrize("case", range(len(sc.KEPT_CASES)), ids=[c[0] for c in sc.KEPT_CASES])
@pytest.mark.parametrize("name", list(INPUTS))
def test_kept_set_matches_fp64(inputs, probe_q, name, case):
    """Full support probe (B = 1026, every token of 9 rows in one launch). Outside the don't-care band (top-p tokens
    whose exclusive cumulative sum is within 2^-16 of top_p; at most 4 per row, none for top_p <= 0.8, asserted on
    the restatement first) every token has exactly the restatement's kept / dropped status; within a group of exactly
    equal logits the kept members are a lowest-index prefix; top-k and min-p keep or drop whole groups; and a second
    launch gives the same winners."""
    cname, params = sc.KEPT_CASES[case]
    logits, dev_logits = inputs[name]
    kw = sc.case_kwargs(params, logits)
    r = sc.restate(logits, **kw)
    top_p = params.get("top_p", 0.0)
    band = sc.band_mask(r, top_p)
    per_row = sc.check_band_cap(band, top_p)
    want = r["probs"] > 0
    gen = None
    if "generated" in kw:
        gen = kw["generated"].to(torch.int32).unsqueeze(0).expand(NV, -1, -1).contiguous().to(DEV)
    win = sample_logits(dev_logits, params, probe_q, gen)
    again = sample_logits(dev_logits, params, probe_q, gen)
    got = sc.decode_support(win)
    print(f"{name} {cname}: kept {got.sum(dim=-1).tolist()} (fp64 {want.sum(dim=-1).tolist()}) band {per_row}")
    assert torch.equal(win, again), "two launches of the same probe differ"
    diff = (got != want) & ~band
    assert not bool(diff.any()), (name, cname, _describe(diff, r, params))
    for row in range(NCB):
        assert sc.prefix_violations(got[row], r["base"][row]) == [], (name, cname, row)
        if set(params) <= {"top_k"} or set(params) <= {"min_p"}:
            for g in sc.tie_groups(r["base"][row]):
                assert int(got[row][g].sum()) in (0, len(g)), (name, cname, row, g.tolist())
    if params in (dict(top_k=1), dict(min_p=1.0)):
        assert torch.equal(got, r["base"] == r["base"].max(dim=-1, keepdim=True).values)
    if top_p == 1e-6:
        assert got.sum(dim=-1).tolist() == [1] * NCB and bool(got[:, 0].all())


@pytest.mark.parametrize("case", range(len(sc.RATIO_CASES)), ids=[c[0] for c in sc.RATIO_CASES])
@pytest.mark.parametrize("name", list(INPUTS))
def test_probability_ratios_match_fp64(inputs, name, case):
    """Ratio probe, 32 tokens per row over the ranks of the kept set: the sampler's p[b] / p[0] lies within
    R64 (1 -+ tol), tol = 8 x the fp32 CPU oracle's largest relative deviation from fp64 on the same pairs (floor
    2^-20). Measured deviations / tol (grid; bf16 rows): T 0.7 6.9e-7 / 5.6e-6; 1.0e-6 / 8.2e-6. T 1 8.5e-8 / 9.5e-7;
    9.2e-8 / 9.5e-7. T 1.3 8.3e-7 / 6.6e-6; 7.3e-7 / 5.8e-6. Unified (.5, .4, 0) 2.5e-6 / 2.0e-5; 2.6e-6 / 2.1e-5.
    Unified (.3, -.1, .25) 2.1e-6 / 1.7e-5; 2.5e-6 / 2.0e-5. Penalty 3 9.2e-8 / 9.5e-7; 2.3e-7 / 1.9e-6. Filtered
    1.4e-7 / 1.1e-6; 1.7e-7 / 1.3e-6."""
    cname, params = sc.RATIO_CASES[case]
    logits, dev_logits = inputs[name]
    kw = sc.case_kwargs(params, logits)
    p64 = sc.restate(logits, **kw)["probs"]
    toks = sc.ratio_tokens(p64)
    dev, tol = sc.ratio_tol(sc.oracle_probs32(logits, **kw), p64, toks)
    print(f"{name} {cname}: fp32 oracle deviation {dev:.2e} tol {tol:.2e}")
    q = sc.ratio_noise(toks, torch.gather(p64, -1, toks) / p64[:, 0:1], tol).to(DEV)
    gen = None
    if "generated" in kw:
        gen = kw["generated"].to(torch.int32).unsqueeze(0).expand(len(q), -1, -1).contiguous().to(DEV)
    win = sample_logits(dev_logits[:len(q)], params, q, gen)
    assert sc.ratio_failures(win, toks) == [], (name, cname, tol)


# ----------------------------------------------------------------------------- decode step
DECODE_TOP_P = dict(temperature=0.9, top_p=0.9)
DECODE_TOP_K = dict(temperature=1.1, top_k=40, repetition_penalty=3.0, repetition_penalty_window=2)


def _boundary_tokens(rs):
    """The probed columns of the decode test: for each restatement and row the 8 tokens on either side of the kept
    set's edge in the sorted order, every 16th column, and the EOS and padding columns."""
    toks = set(range(1, NV, 16)) | {sc.EOS, 1025}
    for r in rs:
        order = torch.sort(r["base"], dim=-1, descending=True, stable=True).indices
        for row in range(NCB):
            n = int((r["probs"][row] > 0).sum())
            toks |= set(order[row, max(n - 8, 0):n + 8].tolist())
    toks.discard(0)
    return torch.tensor(sorted(toks))


def test_decode_step_probes_per_slot_parameter_blocks():
    """The same two probes through zmi_sample_step (decode mode, cfg_scale 2, a random unconditional row) with slots of
    different parameter blocks in one launch: slot 0 greedy, slot 1 inactive, then per probed token one top-p slot and
    one top-k slot (penalty 3 over a history that repeats a token), then the ratio probe's rows on top-p slots. The
    restatement applies u + (c - u) s, the padding column and the EOS bias. Ratio tol as in
    test_probability_ratios_match_fp64: deviation 6.3e-7, tol 5.1e-6."""
    c, u = sc.decode_logits()
    guided = sc.guided_logits(c, u)
    hist = sc.penalty_history(guided.float())
    r_p = sc.restate(guided, **DECODE_TOP_P)
    r_k = sc.restate(guided, generated=hist, **DECODE_TOP_K)
    band = sc.band_mask(r_p, DECODE_TOP_P["top_p"])
    sc.check_band_cap(band, DECODE_TOP_P["top_p"])
    toks = _boundary_tokens((r_p, r_k))
    n = len(toks)
    rt = sc.ratio_tokens(r_p["probs"])
    dev, tol = sc.ratio_tol(sc.oracle_probs32(guided.float(), **DECODE_TOP_P), r_p["probs"], rt)
    print(f"decode: {n} probed columns; ratio deviation {dev:.2e} tol {tol:.2e}")
    rq = sc.ratio_noise(rt, torch.gather(r_p["probs"], -1, rt) / r_p["probs"][:, 0:1], tol)

    S = 2 + 2 * n + len(rq)
    sq = sc.support_noise(toks)
    noise = torch.full((S, NCB, NV), sc.INF)
    bait = torch.sort(r_p["base"], dim=-1, descending=True, stable=True).indices[:, 1]
    noise[0, torch.arange(NCB), bait] = 1.0  # the second-ranked token: a stochastic slot would answer it
    noise[2:2 + 2 * n:2], noise[3:2 + 2 * n:2], noise[2 + 2 * n:] = sq, sq, rq
    slot_params = [(dict(temperature=0.0), 2.0, 1), (DECODE_TOP_P, 2.0, 2)]
    slot_params += [(DECODE_TOP_P, 2.0, 3), (DECODE_TOP_K, 2.0, 4)] * n + [(DECODE_TOP_P, 2.0, 5)] * len(rq)
    active = [1, 0] + [1] * (S - 2)
    nxt, st = sample_step(c.expand(S, -1, -1), u.expand(S, -1, -1), slot_params, noise,
                          hist.unsqueeze(0).expand(S, -1, -1), active)

    assert nxt[0].tolist() == guided.argmax(dim=-1).tolist() == [0] * NCB  # greedy: no race, whatever its noise row
    assert nxt[1].tolist() == [-7] * NCB, "the inactive slot's tokens were written"
    assert [int(st[k][1]) for k in ("step", "pos", "offset", "remaining")] == [0, 0, hist.shape[-1] - 1, 100]
    assert st["step"][0] == 1 and bool((st["step"][2:] == 1).all())
    e = int(torch.nonzero(toks == sc.EOS)[0, 0])
    for kind, r, rows in (("top_p", r_p, nxt[2:2 + 2 * n:2]), ("top_k", r_k, nxt[3:2 + 2 * n:2])):
        got = sc.decode_support(rows, toks)
        want = (r["probs"] > 0)[:, toks]
        print(f"decode {kind}: kept among the probed {got.sum(dim=-1).tolist()}")
        diff = (got != want) & ~(band[:, toks] if kind == "top_p" else torch.zeros_like(want))
        assert not bool(diff.any()), (kind, [(row, int(toks[j])) for row, j in torch.nonzero(diff).tolist()[:8]])
        assert bool(got[0, e]) and not bool(got[1:, e].any()), "EOS: kept on codebook 0 only"
    assert sc.ratio_failures(nxt[2 + 2 * n:], rt) == []


# ----------------------------------------------------------------------------- internal noise
def test_internal_noise_standalone_matches_hash_restatement():
    """noise = NULL, B = 64 rows of ~30 tokens spanning 100x: every token equals argmax(p64 / q) with q from the
    numpy restatement of the counter hash (row b, codebook cb on counter base cb 1026 + b 9 1026), wherever the two
    best race scores differ by more than a relative 1e-4 (at most 1% of the rows do not; asserted first)."""
    lg = sc.spread_logits()
    seed = 77
    p64 = torch.softmax(lg.double(), dim=-1)
    want, gap = sc.race_margin(p64, sc.hash_noise_rows(seed, rows=lg.shape[0]))
    sure = gap >= sc.NOISE_MARGIN
    assert float((~sure).float().mean()) <= sc.NOISE_MARGIN_ROWS
    got = sample_logits(lg.to(DEV), dict(temperature=1.0), None, None, seed)
    assert torch.equal(got[sure], want[sure]), torch.nonzero((got != want) & sure).tolist()[:8]
    assert len(set(map(tuple, got.tolist()))) == lg.shape[0]  # no two batch rows share a stream


def test_internal_noise_decode_depends_on_seed_step_and_codebook():
    """noise = NULL in the decode step at step 0, 1 and 7 with two seeds: the tokens are the restatement's for that
    (seed, step, codebook), counter base ((step + 1) 9 + cb) 1026, and the steps' token vectors differ."""
    lg = sc.spread_logits(seed=23, n_rows=1)
    zero = torch.zeros_like(lg)
    p64 = torch.softmax(sc.guided_logits(lg[0], zero[0], 1.0), dim=-1)
    seen = {}
    for seed in (1234, 0x9E3779B97F4A7C15):
        for step in (0, 1, 7):
            want, gap = sc.race_margin(p64, sc.hash_noise_rows(seed, step=step))
            assert float(gap.min()) >= sc.NOISE_MARGIN, (seed, step)
            nxt, st = sample_step(lg, zero, [(dict(temperature=1.0), 1.0, seed)], step=step)
            assert nxt[0].tolist() == want.tolist(), (seed, step)
            assert int(st["step"][0]) == step + 1
            seen[(seed, step)] = tuple(nxt[0].tolist())
    assert len(set(seen.values())) == len(seen), seen


def test_internal_noise_draws_the_distribution():
    """2048 standalone rows x 9 codebooks of one 8-token distribution (0.4 down to 0.01), one fixed seed: Pearson
    chi-square against the fp64 probabilities below the 1 - 1e-6 quantile for 7 degrees of freedom. Deterministic."""
    lg = sc.eight_token_logits().expand(2048, NCB, -1).contiguous().to(DEV)
    got = sample_logits(lg, dict(temperature=1.0), None, None, 2024)
    x2 = sc.chi_square(got)
    print(f"chi-square {x2:.2f} over {got.numel()} draws (bound {sc.CHI2_7DF_1M6})")
    assert x2 < sc.CHI2_7DF_1M6


# ----------------------------------------------------------------------------- the zero draw
def _one_peak(col):
    lg = torch.full((1, NCB, NV), -8.0)
    lg[..., col] = 8.0
    return lg.to(DEV)


def test_all_ones_draw_on_a_dropped_token_does_not_hide_the_maximum():
    """u = (float(z >> 40) + 0.5) 2^-24 rounded to 1.0 when the 24 bits are all ones: q = -log(1) = -0, and a token of
    probability 0 scored 0 / -0 = NaN. The thread of column 64 (lane 0 of wave 1) kept that NaN, block_argmax neither
    took nor replaced it, and wave 1 reported NaN instead of its maximum at column 577: the sampler answered token 0,
    of probability 0. With u clamped below 1 the draw is finite and the maximum wins. The seed puts the all-ones
    draw on standalone row 0, codebook 0, column 64."""
    seed = sc.seed_for_all_ones_draw(sc.ctr_base(0, row=0), 64)
    got = sample_logits(_one_peak(577), dict(temperature=1.0, top_k=1), None, None, seed)
    assert got[0].tolist() == [577] * NCB


def test_all_ones_draw_on_the_maximum_still_wins():
    """The same draw on the only kept token: it scored 1 / -0 = -inf and lost to the zeros of probability 0."""
    seed = sc.seed_for_all_ones_draw(sc.ctr_base(0, row=0), 577)
    got = sample_logits(_one_peak(577), dict(temperature=1.0, top_k=1), None, None, seed)
    assert got[0].tolist() == [577] * NCB
