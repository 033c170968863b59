"""The sampler probes of tests/sampler_cases.py, proven on the CPU: driven through oracle.zonos_cpu.sample (fp32) they
recover the fp64 restatement's kept set and probability ratios, and every boundary mutation that the `samplers`
fixture lets through changes what they decode. The GPU suite (test_gpu_sampler_probe.py) runs the same probes and
cases on the HIP sampler."""
import numpy as np
import pytest
import torch

from oracle import zonos_cpu as oz
from tests import sampler_cases as sc
from zonos_vibes_amd.synthetic import mix64

INPUTS = {"grid": sc.grid_logits, "bf16": sc.fixture_logits}


@pytest.fixture(scope="module")
def inputs():
    return {k: f() for k, f in INPUTS.items()}


@pytest.fixture(scope="module")
def probe_q():
    return sc.support_noise()


def _oracle_kept(logits, kw, q):
    out = oz.sample(logits.unsqueeze(0).expand(sc.NV, -1, -1), noise=q, **sc.oracle_sample_kwargs(
        {**kw, "generated": kw["generated"].unsqueeze(0).expand(sc.NV, -1, -1)} if "generated" in kw else kw))
    return sc.decode_support(out.squeeze(-1))


def test_inputs_have_the_stated_shape():
    x = sc.grid_logits()
    assert x.shape == (9, 1026) and bool((x[:, 0] == 8.0).all())
    assert bool(torch.isneginf(x[:, 1025]).all()) and bool(torch.isneginf(x[1:, 1024]).all())
    assert torch.isfinite(x[0, 1024])
    fin = x[torch.isfinite(x)]
    assert bool((fin * 8 == (fin * 8).round()).all())
    for r in range(9):
        n_max = int((x[r] == 8.0).sum())
        assert 5 <= n_max <= 18, n_max
    y = sc.fixture_logits()
    assert bool((y[:, 0:1] >= y).all()) and bool((y.bfloat16().float() == y).all())
    assert all(len(torch.unique(y[r])) < 1026 - 250 for r in range(9))  # hundreds of duplicated values per row


@pytest.mark.parametrize("name", list(INPUTS))
def test_probes_recover_the_kept_set_through_the_fp32_oracle(inputs, probe_q, name):
    """Support probe on oracle.zonos_cpu.sample, every kept-set case: the decoded kept set is the fp64 restatement's
    outside the don't-care band, whose cap holds on the restatement."""
    logits = inputs[name]
    for cname, params in sc.KEPT_CASES:
        kw = sc.case_kwargs(params, logits)
        r = sc.restate(logits, **kw)
        band = sc.band_mask(r, params.get("top_p", 0.0))
        per_row = sc.check_band_cap(band, params.get("top_p", 0.0))
        want = r["probs"] > 0
        got = _oracle_kept(logits, kw, probe_q)
        print(f"{name} {cname}: kept {want.sum(dim=-1).tolist()} band {per_row}")
        diff = (got != want) & ~band
        assert not bool(diff.any()), (name, cname, torch.nonzero(diff).tolist()[:8])
        if "min_p" in r:  # only top-p has a band: no min-p decision here is a rounding question (1.0 = the maximum)
            m = r["min_p"][(r["min_p"] > 0) & (r["min_p"] != 1.0)]
            assert float((m - 1).abs().min()) > 1e-4, (name, cname)


@pytest.mark.parametrize("name", list(INPUTS))
def test_probes_recover_the_ratios_through_the_fp32_oracle(inputs, name):
    logits = inputs[name]
    for cname, params in sc.RATIO_CASES:
        kw = sc.case_kwargs(params, logits)
        p64 = sc.restate(logits, **kw)["probs"]
        toks = sc.ratio_tokens(p64)
        dev, tol = sc.ratio_tol(sc.oracle_probs32(logits, **kw), p64, toks)
        print(f"{name} {cname}: fp32 oracle deviation {dev:.2e} tol {tol:.2e}")
        assert tol < 1e-3, "the oracle itself is not this far from fp64"
        q = sc.ratio_noise(toks, torch.gather(p64, -1, toks) / p64[:, 0:1], tol)
        okw = sc.oracle_sample_kwargs(
            {**kw, "generated": kw["generated"].unsqueeze(0).expand(len(q), -1, -1)} if "generated" in kw else kw)
        out = oz.sample(logits.unsqueeze(0).expand(len(q), -1, -1), noise=q, **okw)
        assert sc.ratio_failures(out.squeeze(-1), toks) == [], (name, cname)


def test_every_boundary_mutation_changes_the_decoded_kept_set(inputs, probe_q):
    """What the `samplers` fixture cannot see (it compares only the final token): each mutation of the restatement,
    raced against the support probe's noise, decodes to another kept set than the restatement's on at least one case,
    outside the don't-care band, where the GPU test compares.

    One mutation of the list cannot be seen, by the band's own definition: a top-p cumulative sum in sequential fp32
    stays within 4.5e-6 of the fp64 sum over all cases on these inputs (printed below), under a third of the 2^-16
    band, and changes no token's fate on any case: it is a rounding-level difference, not a boundary error. The test
    asserts that deviation instead."""
    hits = {m: [] for m in sc.MUTATIONS}  # (input, case, tokens changed outside the band)
    seq_dev = 0.0
    for name, logits in inputs.items():
        for cname, params in sc.KEPT_CASES:
            kw = sc.case_kwargs(params, logits)
            r = sc.restate(logits, **kw)
            care = ~sc.band_mask(r, params.get("top_p", 0.0))
            want = r["probs"] > 0
            for m, filt in sc.MUTATIONS.items():
                if filt not in params:
                    continue  # the case does not run the filter this mutation changes
                rm = sc.restate(logits, mut=m, **kw)
                if m == "top_p_fp32_sequential":
                    seq_dev = max(seq_dev, float((rm["top_p"] - r["top_p"]).abs().max()))
                kept = rm["probs"] > 0
                if hits[m]:
                    got = kept
                else:  # until a mutation is seen, through the probe itself
                    got = sc.decode_support(sc.race(rm["probs"].unsqueeze(0), probe_q))
                    assert bool((got == kept)[:, 1:].all())
                n = int(((got != want) & care).sum())
                if n:
                    hits[m].append((name, cname, n))
    for m, h in hits.items():
        print(f"{m}: seen on {len(h)} cases, e.g. {h[:3]}")
    print(f"sequential fp32 cumulative sum: largest deviation from fp64 {seq_dev:.2e} (band {sc.BAND:.2e})")
    assert [m for m, h in hits.items() if not h] == ["top_p_fp32_sequential"]
    assert 0 < seq_dev < sc.BAND / 2


def test_inv_mix64_inverts_mix64():
    rng = np.random.default_rng(3)
    xs = [0, 1, 2, (1 << 64) - 1, (1 << 63), (1 << 32) - 1, 1 << 32, 0xFFFFFF << 40]
    xs += [int(v) for v in rng.integers(0, 1 << 63, 2000, dtype=np.uint64)] + \
          [int(v) | (1 << 63) for v in rng.integers(0, 1 << 63, 2000, dtype=np.uint64)]
    for x in xs:
        assert sc.inv_mix64(mix64(x)) == x and mix64(sc.inv_mix64(x)) == x


def test_all_ones_draw_rounds_to_one_without_the_clamp():
    """16777215 + 0.5 rounds to 16777216 in fp32: u = 1.0 and q = -log(1) = -0, the zero draw. The clamp moves that
    one draw to the largest fp32 below 1 and leaves every other draw's bits alone."""
    z = np.array([0xFFFFFF << 40, (0xFFFFFF << 40) | 0xFFFFFFFFFF, 0xFFFFFE << 40, 0, 1 << 40], dtype=np.uint64)
    raw, cl = sc.uniform_from_bits(z, clamp=False), sc.uniform_from_bits(z)
    assert raw[0] == 1.0 and raw[1] == 1.0 and raw[2] < 1.0
    assert cl[0] == cl[1] == np.float32(1 - 2.0 ** -24) and -np.log(cl[0]) > 0
    assert (raw[2:] == cl[2:]).all() and raw[3] == np.float32(2.0 ** -25)
    seed = sc.seed_for_all_ones_draw(sc.ctr_base(0, row=0), 64)
    assert sc.hash_noise(seed, 0, clamp=False)[64] == 0.0 and sc.hash_noise(seed, 0)[64] > 0
    others = np.arange(sc.NV) != 64
    assert (sc.hash_noise(seed, 0, clamp=False)[others] == sc.hash_noise(seed, 0)[others]).all()


def test_internal_noise_restatement_margins_and_distribution():
    """The CPU side of the GPU internal-noise tests: few rows of the spread distribution are too close to call, and
    the hash restatement's own 18432 draws of the 8-token distribution pass the chi-square bound the kernel is held
    to."""
    lg = sc.spread_logits()
    p64 = torch.softmax(lg.double(), dim=-1)
    _, gap = sc.race_margin(p64, sc.hash_noise_rows(77, rows=lg.shape[0]))
    assert float((gap < sc.NOISE_MARGIN).float().mean()) <= sc.NOISE_MARGIN_ROWS
    p8 = torch.softmax(sc.eight_token_logits().double(), dim=-1)
    toks = sc.race(p8, sc.hash_noise_rows(2024, rows=2048))
    x2 = sc.chi_square(toks)
    print(f"chi-square of the restatement's draws {x2:.2f} (bound {sc.CHI2_7DF_1M6})")
    assert x2 < sc.CHI2_7DF_1M6
