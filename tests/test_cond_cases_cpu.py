"""tests/cond_cases.py judged on the CPU: the builders do what their names say, no Fourier element is left whose bf16
rounding could depend on the libm, the float32 restatement of the kernel meets the criterion on every launch (this is
the condition on the inputs), the restatement agrees bit for bit with the CPU oracle where a launch is expressible as a
conditioner list, and each of the four mutants misses the criterion on a committed launch. No GPU."""
import numpy as np
import pytest
import torch

from oracle.conditioning_cpu import OracleConditioner
from tests import cond_cases as cc
from tests.test_conditioning import assert_bf16_close
from zonos_vibes_amd.conditioning import PrefixConditioner, make_cond_dict

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def launches():
    return {(d, eps): cc.launch(d, eps) for d in cc.WIDTHS for eps in cc.EPS}


@pytest.fixture(scope="module")
def emulated(launches):
    return {k: cc.emulate(L) for k, L in launches.items()}


def test_bf16_helpers():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-5, 257.0, 258.0], dtype=F32)
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    assert np.array_equal(cc.bf(x), want)                       # ties to even, both directions
    assert np.array_equal(cc.bf64(x.astype(F64)), want.astype(F64))
    assert cc.bf64(1.00390625 + 2.0 ** -40) == 1.0078125       # above the tie: a detour through fp32 would lose it
    assert torch.equal(cc.to_torch_bf16(cc.bf(x)).float(), torch.from_numpy(want))
    assert cc.bf16_ulp(1.5) == 2.0 ** -7 and cc.bf16_ulp(0.0) == 2.0 ** -20


@pytest.mark.parametrize("d", cc.WIDTHS)
def test_launch_holds_every_regime(launches, d):
    L = launches[(d, 1e-5)]
    kinds = {r[1] for r in L.rows}
    assert kinds == {cc.EMBED, cc.VECTOR, cc.FOURIER, cc.LINEAR, cc.PASSTHROUGH}
    assert [r[1] for r in L.rows] != sorted(r[1] for r in L.rows)  # permuted
    v = cc.all_v(L)
    tag = {t: r for r, t in enumerate(L.tags)}
    # embed: first and last index, rows that differ from each other
    n_tab = L.params[0].table.shape[0]
    assert L.rows[tag["embed/first"]][2] == 0 and L.rows[tag["embed/last"]][2] == n_tab - 1
    assert np.array_equal(v[tag["embed/last"]], cc.table_row(n_tab - 1, d))
    assert not np.array_equal(cc.table_row(0, d), cc.table_row(n_tab - 1, d))
    # vector rows go through the odd parameter entries
    assert all(L.rows[r][0] % 2 == 1 for r, t in enumerate(L.tags) if t.startswith("vector/"))
    # passthrough: not bf16 values, exact ties and both neighbours; an odd and large x_off; no weight at all
    pr = L.rows[tag["passthrough/ties"]]
    x = L.x[pr[3]:pr[3] + d]
    assert pr[3] % 2 == 1 and pr[3] > 4096 and L.params[pr[0]].weight is None and L.params[pr[0]].table is None
    assert not np.any(cc.bf(x) == x)
    t = x[0::3].astype(F64)
    dn, up = cc.bf64(np.nextafter(t, 0)), cc.bf64(np.nextafter(t, np.sign(t) * np.inf))
    assert np.all(np.abs(t - dn) == np.abs(up - t)) and np.all(dn != up)  # exact ties
    assert all(r[3] != 0 for r in L.rows if r[1] in (cc.FOURIER, cc.LINEAR, cc.PASSTHROUGH))
    # Fourier: in_dim 1, 8, 256; min_val != 0; x at, below and above the range; an exact f == 0 row; |f| ~ 200 rad
    assert [L.params[p].in_dim for p in (2, 4, 6)] == [1, 8, 256] and L.params[4].min_val != 0
    f_of = lambda t_: cc.fourier_f(L.params[L.rows[tag[t_]][0]],  # noqa: E731
                                   L.x[L.rows[tag[t_]][3]:][:L.params[L.rows[tag[t_]][0]].in_dim])
    assert not f_of("fourier1/min").any()
    h = d // 2
    assert np.all(v[tag["fourier1/min"]][:h] == 1) and not v[tag["fourier1/min"]][h:].any()
    xs = {n: float(L.x[L.rows[tag["fourier1/" + n]][3]]) for n in ("min", "max", "below", "above")}
    assert xs["min"] == 0 and xs["max"] == 24000 and xs["below"] < 0 and xs["above"] > 24000
    fmax = max(float(np.abs(f_of(t_)).max()) for t_ in tag if t_.startswith("fourier"))
    assert fmax > (100 if d >= 254 else 10), fmax
    # linear: in_dim 1, 128, 256; a NULL bias; inputs that are not bf16 values; an order-sensitive sum
    assert [L.params[p].in_dim for p in (8, 10, 12)] == [1, 128, 256]
    assert L.params[10].bias is None and L.params[8].bias is not None
    for t_ in ("linear1/bias", "linear128/nobias", "linear256/alternating"):
        r = L.rows[tag[t_]]
        xin = L.x[r[3]:r[3] + L.params[r[0]].in_dim]
        assert np.any(cc.bf(xin) != xin)
    r = L.rows[tag["linear256/alternating"]]
    p, xin = L.params[r[0]], cc.bf(L.x[r[3]:r[3] + 256])
    rev = np.zeros(d, dtype=F32)
    for k in reversed(range(256)):
        rev = rev + xin[k] * p.weight[:, k]
    if d >= 254:  # the reversed order rounds some of the d sums differently
        assert np.any(cc.bf(rev + p.bias) != v[tag["linear256/alternating"]])
    # LayerNorm regimes
    assert np.ptp(v[tag["embed/const"]]) == 0 and np.ptp(v[tag["vector/const"]]) == 0
    assert set(np.unique(v[tag["embed/pm128"]])) <= {127.5, 129.0}
    o = v[tag["embed/outlier"]]
    assert np.count_nonzero(o) == 1 and o[cc.outlier_at(d)] != 0
    tiny = v[tag["embed/tiny"]].astype(F64)
    assert tiny.var() < 0.5e-5 and np.all(np.abs(tiny) >= 2.0 ** -10) and np.all(np.abs(tiny) <= 2.0 ** -9)
    assert (L.ln_w > 0).any() and (L.ln_w < 0).any() and np.abs(L.ln_b).max() == 64
    assert not cc.fp32_unsafe(L).any()


@pytest.mark.parametrize("d", cc.WIDTHS)
def test_no_fourier_element_depends_on_the_libm(launches, d):
    for eps in cc.EPS:
        L = launches[(d, eps)]
        n = 0
        for r, (pi, kind, _, off) in enumerate(L.rows):
            if kind == cc.FOURIER:
                p = L.params[pi]
                f = cc.fourier_f(p, L.x[off:off + p.in_dim])
                assert not cc.trig_unsafe(f).any(), (d, L.tags[r])
                n += 1
        assert n == 8


def test_trig_unsafe_sees_the_boundaries():
    c = np.arccos(np.array([1 - 2.0 ** -9, 0.75 + 2.0 ** -9, 0.5]))  # two rounding boundaries, one bf16 value
    assert cc.trig_unsafe(c.astype(F64)).tolist()[:2] == [True, True]
    assert cc.trig_unsafe(np.array([np.pi / 2 - 1e-3])).all()         # |cos| below 2^-8
    assert not cc.trig_unsafe(np.array([0.0])).any()


@pytest.mark.parametrize("d", cc.WIDTHS)
def test_fp32_restatement_meets_the_criterion(launches, emulated, d):
    for eps in cc.EPS:
        L = launches[(d, eps)]
        fig = cc.check(emulated[(d, eps)], L)
        print(f"restatement d {d} eps {eps}: worst {fig['worst']:.3f} ulp, bit-identical {fig['same']:.5f}")
        for r, t in enumerate(L.tags):  # each row alone is its row of the mixed launch
            if t.endswith("const"):
                assert np.array_equal(cc.emulate(L.only(r))[0], L.ln_b)


@pytest.mark.parametrize("d", [8, 258, 2048])
def test_restatement_equals_the_oracle_bit_for_bit(d):
    """A conditioner list with every kind (v0.1 and one un-projected passthrough): v bit for bit at every width, the
    final rows bit for bit at 8 and 258. At 2048 three LayerNorms (the oracle's fp32 one, the restatement's, fp64)
    disagree on about one element in 30,000, so there a final element may differ from the oracle's only by one ulp
    and only where the fp64 value lies within 4 E (cond_cases.fp32_err) of a bf16 rounding boundary."""
    cfgs = cc.oracle_conditioners()
    pc = PrefixConditioner(cfgs, d, device="cpu")
    g = torch.Generator().manual_seed(17 + d)
    w = {k: torch.randn(s, generator=g).to(torch.bfloat16) for k, s in pc.param_shapes().items()}
    pc.load_state_dict(w)
    spk = (0.3 * torch.randn(1, 128, generator=g)).to(torch.bfloat16)
    cd = make_cond_dict(phonemes="ðɪs ɪz ə tɛst.", language="en-gb", speaker=spk, pitch_std=45.0,
                        speaking_rate=12.5, unconditional_keys={"vqscore_8", "dnsmos_ovrl", "fmax"})
    cd["plain"] = torch.randn(1, 1, d, generator=g).to(torch.bfloat16)
    L = cc.launch_from_conditioner(pc, cd)
    assert {r[1] for r in L.rows} == {cc.EMBED, cc.VECTOR, cc.FOURIER, cc.LINEAR, cc.PASSTHROUGH}
    orc = OracleConditioner(cfgs, d, w)
    want_v = torch.cat([orc._conditioner(i, c, cd.get(c["name"])).reshape(-1, d) for i, c in enumerate(cfgs)])
    v = cc.all_v(L)
    assert torch.equal(cc.to_torch_bf16(v), want_v)
    want = orc.forward(cd)[0]
    ref = cc.reference(L)
    near = cc.boundary_distance(ref) <= 4 * cc.fp32_err(L, v)
    for got in (cc.emulate(L), cc.bf64(ref).astype(F32)):
        diff = cc.to_torch_bf16(got) != want
        print(f"d {d}: {int(diff.sum())} of {diff.numel()} final elements differ from the oracle's")
        if d < 2048:
            assert not diff.any()
        assert bool(torch.from_numpy(near)[diff].all())
        assert_bf16_close(cc.to_torch_bf16(got), want, exact_frac=0.9999)


# ----------------------------------------------------------------------------- mutants
def _misses(launches, mode, pick):
    out = []
    for (d, eps), L in launches.items():
        if pick(d) and not cc.passes(cc.emulate(L, mode), L):
            out.append((d, eps))
    return out


def test_mutant_one_pass_variance_misses(launches):
    """E[x^2] - mean^2 loses the 128 +- one step rows: at the full widths on every launch."""
    got = _misses(launches, "onepass", lambda d: d >= 2048 and d % 256 == 0)
    assert len(got) == 4, got
    L = launches[(4096, 1e-5)]
    r = L.tags.index("embed/pm128")
    assert not cc.passes(cc.emulate(L.only(r), "onepass"), L.only(r))


def test_mutant_unrounded_s_misses(launches):
    assert len(_misses(launches, "s_unrounded", lambda d: d >= 8)) == 2 * (len(cc.WIDTHS) - 1)


def test_mutant_sine_half_reading_w_j_misses(launches):
    assert len(_misses(launches, "sin_wj", lambda d: True)) == 2 * len(cc.WIDTHS)


def test_mutant_column_256_dropped_from_the_mean_misses(launches):
    assert len(_misses(launches, "drop256", lambda d: d > 256)) == 2 * sum(d > 256 for d in cc.WIDTHS)
    assert _misses(launches, "drop256", lambda d: d <= 256) == []  # no column 256 there
