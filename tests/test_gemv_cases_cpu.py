"""CPU checks of the GEMV case table (tests/gemv_cases.py): the table reaches every launch form the library builds
(asked of the library itself through zmi_gemv_form, which needs no GPU), the library refuses what it does not build,
and the epilogue criteria reject deliberately wrong emulations on the same inputs. The kernels themselves are compared
in tests/test_gpu_gemv_forms.py."""
import pytest
import torch

from tests import gemv_cases as gc
from zonos_vibes_amd import _lib as L


def _v(c, swiglu=False):
    """A stand-in for the kernel's fp32 sums: the fp64 sums rounded to float32."""
    W = gc.weight(c, swiglu)
    if swiglu:
        W = W[gc.swiglu_rows(c.N)]  # the packed column order of ZMI_PACK_SWIGLU
    return (gc.rows_in(c).double() @ W.double().t()).float()


def test_every_case_gets_the_form_it_names():
    for c in gc.CASES:
        for epi in gc.case_epis(c):
            got = gc.query_form(L, gc.case_args(L, c, epi), epi, c.rows_opt)
            assert got is not None, (c.name, epi, L.lib().zmi_last_error())
            assert got[0] == c.form, (c.name, epi, got)
            if c.rpw_gt1:
                assert got[1] > 1, (c.name, epi, got)


def test_case_table_covers_every_built_form():
    seen, rpw = set(), set()
    for c in gc.CASES:
        form, r = gc.query_form(L, gc.case_args(L, c, gc.case_epis(c)[0]), gc.case_epis(c)[0], c.rows_opt)
        seen.add(form[:6])
        if r > 1:
            rpw.add(form[0] != gc.BODY)
    assert seen == gc.built_forms(), (sorted(seen - gc.built_forms()), sorted(gc.built_forms() - seen))
    assert rpw == {False, True}  # several row tiles per workgroup in gemv_body and in the many-row form
    # every prologue, and every epilogue on single-tile, tile-loop and many-row launches
    assert {c.form[6] for c in gc.CASES} == set(gc.PRO.values())
    for epi in ("store", "residual", "swiglu", "qkv"):
        forms = {(c.form[0] != gc.BODY, c.form[5]) for c in gc.CASES if epi in gc.case_epis(c)}
        assert forms == {(False, 0), (False, 1), (True, 0)}, (epi, forms)
    assert {c.form[5] for c in gc.LOGITS_CASES} == {0, 1}


def test_form_query_follows_the_rows_option():
    """The many-row form is an option of the launch, not of the case: with ZMI_OPT_GEMM_ROWS 0 the same arguments take
    gemv_body's tile loop, and the option is back at its value afterwards."""
    c = gc.BY_NAME["R-81x8264"]
    before = L.lib().zmi_get_option(gc.OPT_GEMM_ROWS)
    assert gc.query_form(L, gc.case_args(L, c, "f32"), "f32", 0)[0] == gc.body(2048, 4, False)
    assert gc.query_form(L, gc.case_args(L, c, "f32"), "f32", 1)[0] == gc.rows(False)
    assert gc.query_form(L, gc.case_args(L, c, "f32"), "f32", 3)[0] == gc.rows(True)
    assert L.lib().zmi_get_option(gc.OPT_GEMM_ROWS) == before


@pytest.mark.parametrize("name,grid", [("D-ln-33x9248", (578, 3, 3)), ("R-81x8264", (130, 6, 6)), ("R-65x72", (2, 5, 1)),
                                       ("H-m64", (65, 4, 1)), ("G-m17", (5, 3, 1))])
def test_form_query_reports_the_grid(name, grid):
    """n_cb column blocks (the last one partial in each of these), n_rt row tiles, rpw row tiles per workgroup."""
    import ctypes
    c = gc.BY_NAME[name]
    f = L.GemvForm()
    with gc._rows_opt(c.rows_opt):
        assert L.lib().zmi_gemv_form(ctypes.byref(gc.case_args(L, c, "f32")), gc.EPI["f32"], ctypes.byref(f)) == 0
    assert (f.n_cb, f.n_rt, f.rpw) == grid


@pytest.mark.parametrize("pro,M,N,K,groups", gc.REFUSED)
def test_library_refuses_what_it_does_not_build(pro, M, N, K, groups):
    epi = "store" if pro == "grms_g" else "f32"
    assert gc.query_form(L, gc.make_args(L, M, N, K, pro, groups), epi) is None
    assert L.lib().zmi_last_error()


def test_prologues_are_refused_with_epilogues_they_are_not_built_for():
    assert gc.query_form(L, gc.make_args(L, 3, 72, 2048, "addln"), "f32") is None
    assert gc.query_form(L, gc.make_args(L, 3, 72, 2048, "addln"), "residual") is None
    assert gc.query_form(L, gc.make_args(L, 3, 72, 1024, "addln"), "store") is None
    assert gc.query_form(L, gc.make_args(L, 3, 72, 1024, "grms"), "f32") is None
    assert gc.query_form(L, gc.make_args(L, 3, 72, 2048, "grms"), "store") is None
    assert gc.query_form(L, gc.make_args(L, 3, 72, 2048, "addln"), "store")[0] == gc.body(2048, 1, True, "addln")


def test_swiglu_reference_boundary_share():
    """The share of reference elements where either bf16 neighbour of silu(g) is allowed stays under 1 % for the committed
    seeds, over all SWIGLU cases together: the gates are bf16 values, a few of which (3.1094, -1.4219, ...) have a silu
    that close to a boundary, so a case of a few hundred elements has a clumpy share of its own while the large cases
    and the whole are steady. The allowed zone is 2^-15 |value| wide, a bf16 ulp 2^-8 .. 2^-7 |value|. And the gates
    span about +-8."""
    n_near = n_all = 0
    for c, epi in gc.EPILOGUE_CASES:
        if epi != "swiglu" or c.pro != "plain":
            continue
        v = _v(c, swiglu=True)
        g = gc.bfround(gc.swiglu_split(v)[1]).double()
        near = gc.bf16_neighbours(g / (1 + torch.exp(-g)))[2]
        assert 4.5 < g.abs().max().item() < 12.0, (c.name, g.abs().max().item())
        n_near, n_all = n_near + int(near.sum()), n_all + near.numel()
    assert n_all > 500000 and n_near / n_all < gc.SWIGLU_REF_SHARE_MAX, (n_near, n_all)
    print(f"boundary share {n_near / n_all:.5f} of {n_all}")


def test_bf16_neighbours_are_the_bf16_roundings():
    s = torch.randn(20000, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 3
    r, other, near = gc.bf16_neighbours(s)
    assert torch.equal(r.float(), s.to(torch.bfloat16).float())  # fp64 -> bf16 nearest-even
    assert torch.equal(other.float().to(torch.bfloat16).float(), other.float()) and (other != r).all()
    assert ((other - s).abs() >= (r - s).abs()).all() and ((other - r).abs() == gc.bf16_ulp(s)).all()
    mid = (r + other) / 2
    assert gc.bf16_neighbours(mid * (1 + 2.0 ** -18))[2].all() and not gc.bf16_neighbours(mid * (1 + 2.0 ** -14))[2].any()


# ------------------------------------------------------------------------------------------------ discrimination
def test_swiglu_criterion_rejects_swapped_halves():
    c = gc.BY_NAME["C-m17"]
    v = _v(c, swiglu=True)
    ok, second, _ = gc.swiglu_check(gc.emulate_swiglu(v), v)
    assert ok.all() and second.float().mean().item() <= gc.SWIGLU_SECOND_CAP
    assert not gc.swiglu_check(gc.emulate_swiglu(v, swap=True), v)[0].all()
    assert gc.swiglu_check(gc.emulate_swiglu(v, swap=True), v)[0].float().mean().item() < 0.1


def test_residual_criterion_rejects_an_unrounded_linear_term():
    c = gc.BY_NAME["C-m17"]
    v, res = _v(c), gc.residual_in(c)[:, : c.N]
    good = gc.emulate_residual(v, res)
    assert gc.same_bits(good, gc.emulate_residual(v, res))
    assert not gc.same_bits(good, gc.emulate_residual(v, res, round_linear=False))
    assert (res.float().abs().mean() > 3 * v.abs().mean()).item()  # the residual dominates the linear term


def _qkv(c, **wrong):
    hq, hkv, hd = c.heads
    pos, kv, rope = gc.qkv_inputs(c)
    v = _v(c)
    q0 = gc.sentinel16(c.M, c.ldo)
    k0, vt0 = gc.sentinel16(c.M, hkv, gc.SMAX, hd), gc.sentinel16(c.M, hkv, hd, gc.SMAX)
    return gc.emulate_qkv(v, c.heads, pos, kv, rope, q0, k0, vt0, **wrong), (q0, k0, vt0), (pos, kv)


@pytest.mark.parametrize("name", ["QA-16x4-m17", "QC-4x1-m5", "QD-8x4-m17"])
def test_qkv_criterion_rejects_rope_on_v_and_a_shifted_k(name):
    c = gc.BY_NAME[name]
    (q, k, vt), (q0, k0, vt0), (pos, kv) = _qkv(c)
    assert 0 in pos.tolist() and gc.SMAX - 1 in pos.tolist() and (pos < 0).sum() == 1
    (q1, k1, vt1), _, _ = _qkv(c, rope_v=True)
    assert gc.same_bits(q1, q) and gc.same_bits(k1, k) and not gc.same_bits(vt1, vt)
    (q2, k2, vt2), _, _ = _qkv(c, k_shift=1)
    assert gc.same_bits(q2, q) and gc.same_bits(vt2, vt) and not gc.same_bits(k2, k)
    # the inactive row writes nothing anywhere; every active row writes its q row, one K slot and one V column
    m = int((pos < 0).nonzero()[0])
    assert gc.same_bits(q[m], q0[m]) and gc.same_bits(k[int(kv[m])], k0[int(kv[m])])
    assert gc.same_bits(vt[int(kv[m])], vt0[int(kv[m])])
    hq, hkv, hd = c.heads
    assert (k.view(torch.int16) != gc.SENT16).sum().item() == (c.M - 1) * hkv * hd
    assert (vt.view(torch.int16) != gc.SENT16).sum().item() == (c.M - 1) * hkv * hd
    assert (q.view(torch.int16) != gc.SENT16).sum().item() == (c.M - 1) * hq * hd


def test_logits_criterion_rejects_a_stride_of_1025():
    c = gc.BY_NAME["L-k512-n2056-m2"]
    v = _v(c)
    init = gc.sentinel32((c.M + 1) * 9 * 1026)
    good = gc.emulate_logits(v, c.nv, init)
    assert not gc.same_bits(good, gc.emulate_logits(v, c.nv, init, stride=1025))
    g = good.view(c.M + 1, 9, 1026)
    assert torch.equal(g[:c.M, :2].reshape(c.M, -1), gc.bfround(v[:, : c.nv]))
    assert (g[:, 2:].view(torch.int32) == gc.SENT32).all() and (g[c.M].view(torch.int32) == gc.SENT32).all()
