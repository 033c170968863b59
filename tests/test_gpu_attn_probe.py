"""Every attention form against the fp64 softmax of tests/attn_cases.py, on crafted caches (MI355X only).

Forms: zmi_attention_variant with variant 1 (chunked, one launch), 2 and 3 (the split launches), 5 (one workgroup per
512-key block; once with n_query hkv no multiple of 8 and once, v5_x8, with a multiple, which takes the per-XCD
hand-off), 4 and 8 (whole-query kernels, positions < zmi_attention_max_keys_whole()), variant 0 in both of its
resolutions (v0_small: n_query hkv < 32 resolves to 1, v0_large: >= 32 resolves to 5; asserted through
zmi_attention_pick), and zmi_attention_prefill on six sequences. Each form is judged on its own against ref64, not
through bit identity with another form: geometry, score profiles, V kinds, the stale region, the reference and the
criterion

    |got - o64| <= E A_d + 0.5 ulp_bf16(|o64| + E A_d),  E = 2^-8 + 2 2^-24 ((hd + 2) sabs + smag) + 2^-21 + (n + 16) 2^-24

elementwise over every element, are those of tests/attn_cases.py (derived there; tests/test_attn_cases_cpu.py holds the
oracle, a float32 emulation and the mutants). On top: onehot rows equal V_t, flat_count rows equal
oracle.attention_cpu.attend_row and position 0 equals V_0, bit for bit; the inactive row and the prefill's gap rows
keep their sentinel; a second launch gives the bits of the first; the hand-off error word stays 0.

One launch takes all rows of a case (positions 0 .. 2048 and an inactive row, each on a KV row of its own). For
variants 1, 2, 3 and 5 at (16, 4), rand4_count and steps_up_normal are launched once more with a row at position 8320
in front (66 chunks: the second maxima-gather loop of attn_kernel<4, 2 / 3> runs) and smax = 8328 for every row.

Measured on an MI355X, max(error / bound) over the head geometries (16, 4), (8, 4), (4, 1), (4, 4) and every position
of a launch; 1.0 is the criterion. The oracle's own ratios on the same rows (tests/test_attn_cases_cpu.py) are the v1
column's to three digits: what is left is the bf16 rounding of P and of the result, which the reference implementation
has too. v0_small, v4 and v8 see fewer positions, the prefill other rows.

                                v1        v2        v3        v5     v5_x8        v4        v8  v0_small  v0_large   prefill
flat_count                   0.432     0.432     0.432     0.432     0.432     0.413     0.413     0.413     0.432     0.495
onehot_normal                0.000     0.000     0.000     0.000     0.000     0.000     0.000     0.000     0.000     0.000
onehot_tails                 0.000     0.000     0.000     0.000     0.000     0.000     0.000     0.000     0.000     0.000
two_peaks_count              0.807     0.807     0.807     0.807     0.807     0.807     0.807     0.791     0.807     0.785
ramp_up_count                0.865     0.865     0.865     0.865     0.865     0.865     0.865     0.842     0.865     0.918
ramp_down_cancel             0.312     0.312     0.312     0.312     0.312     0.312     0.312     0.205     0.312     0.440
steps_up_normal              0.764     0.764     0.764     0.764     0.764     0.764     0.764     0.642     0.764     0.775
steps_down_tails             0.887     0.887     0.887     0.887     0.887     0.887     0.887     0.559     0.887     0.933
offset_pos_cancel            0.294     0.294     0.294     0.294     0.294     0.294     0.294     0.143     0.294     0.297
offset_neg_normal            0.396     0.396     0.396     0.396     0.396     0.396     0.396     0.187     0.396     0.462
rand1_cancel                 0.455     0.455     0.455     0.455     0.455     0.455     0.455     0.197     0.455     0.523
rand4_count                  0.944     0.944     0.944     0.944     0.944     0.944     0.944     0.880     0.944     0.943
rand12_tails                 0.852     0.852     0.852     0.852     0.852     0.852     0.852     0.815     0.852     0.890
spike0_tail_normal           0.531     0.531     0.531     0.531     0.531     0.531     0.531     0.484     0.531     0.516
rand4_count long             0.936     0.936     0.936     0.936         -         -         -         -         -         -
steps_up_normal long         0.699     0.699     0.699     0.699         -         -         -         -         -         -

What the probe found: no miss. All 120 tests pass on the kernels as they were: every form, case and geometry (G = 1 and
the 8320-key row included) is within the criterion, the exact checks hold, the inactive row keeps its sentinel and the
second launch repeats the first one's bits.
"""
import pytest
import torch

from tests import attn_cases as ac
from tests.attn_cases import CASES, HD, HEADS, LONG_CASES, ONEHOT_PICK, ROWS
from tests.test_gpu_attn_prefill import _prefill
from tests.test_gpu_kernels import stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -77.0  # exact in bf16; _prefill fills with the same value
BF = torch.bfloat16

NEAR = [i for i, p in enumerate(ROWS) if p < 1280]  # every row the whole-query forms reach, the inactive one included
SMALL = [ROWS.index(p) for p in (0, 129, 513, 1279, 1536, 2048, -1)]
ALL = list(range(len(ROWS)))
VARIANT = {"v1": 1, "v2": 2, "v3": 3, "v5": 5, "v5_x8": 5, "v4": 4, "v8": 8, "v0_small": 0, "v0_large": 0}
FORMS = list(VARIANT) + ["prefill"]
TABLE = {}  # (form, case) -> max(error / bound) over the head geometries


def _L():
    from zonos_vibes_amd import _lib
    return _lib, _lib.lib()


def _rows_of(form, hkv):
    """The rows of the case's build a form's launch takes (repeats read the KV row of their original)."""
    if form in ("v4", "v8"):
        return NEAR
    if form == "v0_small":
        return SMALL
    if form == "v0_large":
        return ALL + ALL
    if form == "v5_x8":
        n = len(ALL)
        while n * hkv % 8:
            n += 1
        return ALL + ALL[:n - len(ALL)]
    return ALL


@pytest.fixture(scope="module", autouse=True)
def results_table():
    """After the module's tests: max(error / bound) per form and case, over the head geometries and positions."""
    yield
    cases = [c for c in list(CASES) + [f"{c} long" for c in LONG_CASES] if any((f, c) in TABLE for f in FORMS)]
    forms = [f for f in FORMS if any((f, c) in TABLE for c in cases)]
    print("\n" + " " * 24 + "".join(f"{f:>10}" for f in forms))
    for c in cases:
        print(f"{c:<24}" + "".join(f"{'-':>10}" if (f, c) not in TABLE else f"{TABLE[(f, c)]:>10.3f}" for f in forms))


_DEVICE = {}


def _device(bd, key):
    """K and V^T of a build on the device (those of the newest case only: cases come one after the other)."""
    if key not in _DEVICE:
        if any(k[:2] != key[:2] for k in _DEVICE):
            _DEVICE.clear()
        k = bd.k.to(DEV)
        _DEVICE[key] = (k, bd.v.to(DEV).transpose(-1, -2).contiguous())
    return _DEVICE[key]


def _launch(q, k, vt, pos, kv_rows, hq, hkv, variant):
    """zmi_attention_variant twice into a sentinel-filled output: the error word stays 0, the second launch gives the
    first one's bits (the state a launch leaves re-arms itself)."""
    L, lib = _L()
    n, smax = len(pos), k.shape[-2]
    rp = torch.tensor(pos, dtype=torch.int32, device=DEV)
    rk = torch.tensor(kv_rows, dtype=torch.int32, device=DEV)
    work = torch.zeros(lib.zmi_attention_work_bytes(n, hq, hkv, HD, smax - 1), dtype=torch.uint8, device=DEV)
    nf = lib.zmi_attention_partial_floats(n, hq, hkv, HD, smax - 1)
    po = torch.zeros(nf, dtype=torch.float32, device=DEV)
    plm = torch.zeros(nf // HD * 2, dtype=torch.float32, device=DEV)
    outs = []
    for _ in range(2):
        out = torch.full((n, hq * HD), SENT, dtype=BF, device=DEV)
        L.check(lib.zmi_attention_variant(q.data_ptr(), hq * HD, k.data_ptr(), vt.data_ptr(), rk.data_ptr(), rp.data_ptr(),
                                          n, hq, hkv, HD, smax, smax - 1, out.data_ptr(), hq * HD, po.data_ptr(),
                                          plm.data_ptr(), work.data_ptr(), variant, stream_ptr()), f"variant {variant}")
        torch.cuda.synchronize()
        assert int(work[:4].view(torch.int32).item()) == 0, "cross-chunk hand-off timed out"
        outs.append(out.cpu())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "the second launch gives other bits"
    return outs[0]


_ORACLE = {}


def _flat_oracle(bd, rows, kv_rows, pos):
    """oracle.attention_cpu.attend on the rows of a flat_count launch (computed once per build)."""
    from oracle.attention_cpu import attend
    key = (bd.hkv, tuple(bd.pos), tuple(kv_rows), tuple(pos))
    if key not in _ORACLE:
        out = torch.zeros(len(pos), bd.hkv, 4, HD, dtype=BF)
        for r, p in enumerate(pos):
            if p >= 0:
                out[r] = attend(bd.q[rows[r]].reshape(bd.hkv * 4, HD), bd.k[kv_rows[r]], bd.v[kv_rows[r]], p).view(bd.hkv, 4, HD)
        _ORACLE[key] = out
    return _ORACLE[key]


def _judge(form, case, tag, got, bd, ref, G, q_of, kv_rows, pos, label=None):
    """got [n, hkv * G * 128] (bf16, CPU) of a launch whose row i carries the heads of build row q_of[i], reads KV row
    kv_rows[i] and stands at pos[i]; ref: the launch's reference. Prints and records max(error / bound), returns the
    failures."""
    hkv = bd.hkv
    o = got.view(len(pos), hkv, G, HD)
    r = ac.ratio(o, ref)
    worst = r.max().item()
    print(f"{form} {case} {tag}: max(error / bound) {worst:.3f}")
    key = (form, label or case)
    TABLE[key] = max(TABLE.get(key, 0.0), worst)
    bad = []
    if not worst <= 1.0:
        i, h, g, d = (int(x) for x in (r == r.max()).nonzero()[0])
        bad.append((form, case, tag, f"{worst:.3f} at position {pos[i]} kv head {h} head {g} dim {d}: "
                    f"{o[i, h, g, d].item()} against {ref.o64[i, h, g, d].item()}"))
    kv = torch.arange(hkv)
    for i, p in enumerate(pos):
        if p < 0:
            if not (got[i] == SENT).all():
                bad.append((form, case, tag, f"row {i} (inactive) lost its sentinel"))
            continue
        if p == 0 and not torch.equal(o[i], bd.v[kv_rows[i], :, 0][:, None].expand(hkv, G, HD)):
            bad.append((form, case, tag, "position 0 is not V_0 bit for bit"))
        if bd.profile == "onehot":
            for g in range(G):
                t = bd.t[kv_rows[i], :, ONEHOT_PICK[g]]
                if (t <= p).all() and not torch.equal(o[i, :, g], bd.v[kv_rows[i], kv, t]):
                    bad.append((form, case, tag, f"position {p} head {g} is not V_t bit for bit"))
    if case == "flat_count":
        want = _flat_oracle(bd, q_of, kv_rows, pos)[:, :, :G]
        live = torch.tensor([p >= 0 for p in pos])
        if not torch.equal(o[live], want[live]):
            bad.append((form, case, tag, "flat_count is not attend_row bit for bit"))
    return bad


# ---------------------------------------------------------------------------------------------- single-query forms
@pytest.mark.parametrize("hq,hkv", HEADS)
@pytest.mark.parametrize("case", list(CASES))
def test_single_query_forms(case, hq, hkv):
    """Every zmi_attention_variant form on every row of the case, one launch per form."""
    L, lib = _L()
    G = hq // hkv
    bd, ref = ac.build(case, hkv), ac.reference(case, hkv)
    k, vt = _device(bd, ("rows", case, hkv))
    lim = lib.zmi_attention_max_keys_whole()
    assert lim == 1280 and max(ROWS[i] for i in NEAR) == lim - 1
    k_near, vt_near = k[:, :, :lim].contiguous(), vt[..., :lim].contiguous()
    q_all = bd.q_rows(G).to(DEV)
    picks, bad = {}, []
    for form, variant in VARIANT.items():
        rows = _rows_of(form, hkv)
        pos = [ROWS[i] for i in rows]
        n = len(rows)
        picks[form] = lib.zmi_attention_pick(n, hkv, variant)
        if form.startswith("v5"):
            assert (n * hkv % 8 == 0) == (form == "v5_x8")
        near = form in ("v4", "v8")
        got = _launch(q_all[rows].contiguous(), k_near if near else k, vt_near if near else vt, pos, rows, hq, hkv, variant)
        bad += _judge(form, case, f"{hq}/{hkv}", got, bd, ac.take(ref, rows), G, rows, rows, pos)
    assert picks["v0_small"] == 1 and picks["v0_large"] == 5, picks  # both resolutions of the library's choice ran
    assert not bad, bad


@pytest.mark.parametrize("variant", [1, 2, 3, 5])
@pytest.mark.parametrize("case", LONG_CASES)
def test_long_row(case, variant):
    """Position 8320 (66 chunks, 17 blocks) at (16, 4), with every other row of the case in the same launch."""
    hq, hkv, G = 16, 4, 4
    bd, ref = ac.build_long(case), ac.reference_long(case)
    k, vt = _device(bd, ("long", case, hkv))
    rows = list(range(len(bd.pos)))
    got = _launch(bd.q_rows(G).to(DEV), k, vt, list(bd.pos), rows, hq, hkv, variant)
    bad = _judge(f"v{variant}", case, "long 16/4", got, bd, ref, G, rows, rows, list(bd.pos), label=f"{case} long")
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- prefill
@pytest.mark.parametrize("hq,hkv", HEADS)
@pytest.mark.parametrize("case", list(CASES))
def test_prefill_form(case, hq, hkv):
    """zmi_attention_prefill on (pos0, len) = (0, 40), (120, 16), (505, 16), (1016, 16), (1272, 16), (2040, 16), each on
    its own KV row whose stale region starts after the sequence's last position: every (sequence, position) against
    ref64; the gap rows keep the sentinel."""
    L, lib = _L()
    G = hq // hkv
    bd, ref = ac.build_prefill(case, hkv), ac.reference_prefill(case, hkv)
    seqs, n_rows, kv, pos = ac.prefill_rows()
    q_of = [max(s, 0) for s in kv]
    q = bd.q[q_of][:, :, :G].reshape(n_rows, hq * HD).contiguous().to(DEV)
    kd, vd = bd.k.to(DEV), bd.v.to(DEV)
    outs = []
    for _ in range(2):
        rc, out = _prefill(q, kd, vd, seqs, hq, hkv)
        assert rc == 0, lib.zmi_last_error()
        outs.append(out.cpu())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "the second launch gives other bits"
    bad = _judge("prefill", case, f"{hq}/{hkv}", outs[0], bd, ref, G, q_of, q_of, pos)
    assert not bad, bad
