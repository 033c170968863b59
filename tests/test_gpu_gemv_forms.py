"""Every GEMV launch form, prologue and epilogue against the references of tests/gemv_cases.py (MI355X only): the fp32
sums of each form against fp64 on every element, the fused prologues against their standalone kernels bit for bit, and
each epilogue against a float32 emulation from the kernel's own sums. Every launch first asks zmi_gemv_form and requires
the form its case names."""
import ctypes

import pytest
import torch

from tests import gemv_cases as gc
from tests.helpers import zmi_option

pytestmark = pytest.mark.gpu
DEV = "cuda"
PACK_SWIGLU = 1


def _L():
    from zonos_vibes_amd import _lib
    return _lib


def _sp():
    return torch.cuda.current_stream().cuda_stream


_packed = {}


def _weights(c, swiglu=False):
    """(W on the device, its packed image), shared by the cases of a shape and left unchanged."""
    key = (c.N, c.K, swiglu, swiglu and c.pro == "ln")
    if key not in _packed:
        L = _L()
        if len(_packed) >= 6:
            _packed.pop(next(iter(_packed)))
        W = gc.weight(c, swiglu).to(DEV)
        Wp = torch.empty(c.N * c.K, dtype=torch.bfloat16, device=DEV)
        L.check(L.lib().zmi_pack_weight(W.data_ptr(), Wp.data_ptr(), c.N, c.K, c.N, PACK_SWIGLU if swiglu else 0, _sp()))
        torch.cuda.synchronize()
        _packed[key] = (W, Wp)
    return _packed[key]


def _launch(c, epi, ptr, form=None, pro=None, ldo=None, n_valid=None, heads=()):
    """One zmi_gemv_launch of case c's shape under its ZMI_OPT_GEMM_ROWS; form: what zmi_gemv_form must report first."""
    L = _L()
    a = gc.make_args(L, c.M, c.N, c.K, c.pro if pro is None else pro, c.groups, c.ldo if ldo is None else ldo,
                     c.N if n_valid is None else n_valid, heads, ptr)
    if form is not None:
        got = gc.query_form(L, a, epi, c.rows_opt)
        assert got is not None and got[0] == form, (c.name, epi, got, form)
        assert not c.rpw_gt1 or got[1] > 1, (c.name, got)
    with zmi_option(gc.OPT_GEMM_ROWS, c.rows_opt):
        L.check(L.lib().zmi_gemv_launch(ctypes.byref(a), gc.EPI[epi], _sp()), f"{c.name} {epi}")
    torch.cuda.synchronize()


def _f32(c, ptr, form=None, pro=None, n_valid=None):
    """The fp32 sums [M + 1][ldo] (sentinel outside [M][n_valid]) of a launch."""
    out = gc.sentinel32(c.M + 1, c.ldo, device=DEV)
    _launch(c, "f32", dict(ptr, out=out.data_ptr()), form, pro, n_valid=n_valid)
    nv = c.N if n_valid is None else n_valid
    assert (out[:, nv:].view(torch.int32) == gc.SENT32).all() and (out[c.M].view(torch.int32) == gc.SENT32).all(), c.name
    return out[: c.M, :nv]


def _check_sums(c, X, W, ptr, form=None, pro="plain", n_valid=None):
    out = _f32(c, dict(ptr, X=X.data_ptr()), form, pro, n_valid)
    bad = gc.sums_bad(out, X, W[: out.shape[1]])
    assert bad.numel() == 0, (c.name, bad[:4].tolist())
    return out


def _ln_ptr(c):
    lw, lb = (t.to(DEV) for t in gc.ln_params(c))
    return dict(ln_w=lw.data_ptr(), ln_b=lb.data_ptr()), (lw, lb)


@pytest.mark.parametrize("name", [c.name for c in gc.SUMS_CASES])
def test_f32_sums_of_every_form_match_fp64(name):
    c = gc.BY_NAME[name]
    L = _L()
    W, Wp = _weights(c)
    X = gc.rows_in(c, scale=3.0 if c.pro == "ln" else 1.0).to(DEV)
    ptr = dict(W=Wp.data_ptr())
    if c.pro == "plain":
        _check_sums(c, X, W, ptr, c.form, n_valid=c.nv)
        return
    # LayerNorm: the standalone kernel's rows against fp64, their plain sums against fp64, the fused prologue's bits
    lnp, (lw, lb) = _ln_ptr(c)
    xn = torch.zeros(c.M, c.K, dtype=torch.bfloat16, device=DEV)
    L.check(L.lib().zmi_layernorm_rows(X.data_ptr(), c.K, c.M, c.K, lw.data_ptr(), lb.data_ptr(), gc.EPS, xn.data_ptr(),
                                       c.K, _sp()))
    torch.cuda.synchronize()
    ref, tol = gc.layernorm_ref(X, lw, lb)
    err = (xn.double() - ref).abs()
    print(f"{c.name}: layernorm_rows max err {(err / tol).max().item():.3f} bf16 ulp")
    assert (err <= tol).all(), (c.name, (err / tol).max().item())
    plain = _check_sums(c, xn, W, ptr, n_valid=c.nv)
    fused = _f32(c, dict(ptr, X=X.data_ptr(), **lnp), c.form, n_valid=c.nv)
    assert gc.same_bits(fused, plain), c.name


def _store(c, ptr, form=None, pro=None):
    out = gc.sentinel16(c.M + 1, c.ldo, device=DEV)
    _launch(c, "store", dict(ptr, out=out.data_ptr()), form, pro, n_valid=c.nv)
    assert (out[:, c.nv:].view(torch.int16) == gc.SENT16).all() and (out[c.M].view(torch.int16) == gc.SENT16).all()
    return out


@pytest.mark.parametrize("name", [c.name for c in gc.ADDLN_CASES])
def test_addln_prologue_equals_add_layernorm_then_plain(name):
    """GEMV(ADDLN) == zmi_add_layernorm + plain GEMV, whose sums match fp64; res_out == the standalone kernel's new
    residual, written inside [M][K] only (ld_aux > K: the gap and the row after keep their sentinel)."""
    c = gc.BY_NAME[name]
    L = _L()
    W, Wp = _weights(c)
    lnp, (lw, lb) = _ln_ptr(c)
    lda = c.K + 8
    x = gc.rows_in(c, scale=1.5).to(DEV)
    aux = gc.sentinel16(c.M, lda, device=DEV)
    aux[:, : c.K] = gc.rnd(c.M, c.K, scale=2.0, seed=c.seed + 8).to(DEV)
    r_out = gc.sentinel16(c.M + 1, lda, device=DEV)
    r_ref = aux[:, : c.K].contiguous()
    nrm = torch.zeros(c.M, c.K, dtype=torch.bfloat16, device=DEV)
    L.check(L.lib().zmi_add_layernorm(x.data_ptr(), c.K, r_ref.data_ptr(), c.K, c.M, c.K, lw.data_ptr(), lb.data_ptr(),
                                      gc.EPS, nrm.data_ptr(), c.K, 1, _sp()))
    ptr = dict(W=Wp.data_ptr())
    fused = _store(c, dict(ptr, X=x.data_ptr(), aux=aux.data_ptr(), ld_aux=lda, res_out=r_out.data_ptr(), **lnp), c.form)
    plain = _store(c, dict(ptr, X=nrm.data_ptr()), pro="plain")
    assert gc.same_bits(fused, plain), c.name
    assert gc.same_bits(r_out[: c.M, : c.K].contiguous(), r_ref), c.name
    assert (r_out[:, c.K:].view(torch.int16) == gc.SENT16).all() and (r_out[c.M].view(torch.int16) == gc.SENT16).all()
    _check_sums(c, nrm, W, ptr)


@pytest.mark.parametrize("name", [c.name for c in gc.GRMS_CASES])
def test_grms_and_grms_g_prologues_equal_gated_rmsnorm_then_plain(name):
    """On the Mamba2 step kernel's own y and f32 gate (gz_g = 0) or g = y * gate rows (gz_g = 1): GEMV(GRMS) ==
    GEMV(GRMS_G) == zmi_gated_rmsnorm(y, z) + plain GEMV, whose sums match fp64."""
    from tests.test_gpu_hybrid import _args, _bf, _mamba_params
    from zonos_vibes_amd.config import tiny_hybrid, zonos_v01_hybrid
    c, cg = gc.BY_NAME[name], gc.BY_NAME[name.replace("grms", "grms_g")]
    L = _L()
    lib, M, K = L.lib(), c.M, c.K
    W, Wp = _weights(c)
    w = (gc.rnd(K, scale=0.2, seed=c.seed + 3) + 1).to(DEV)
    md = (zonos_v01_hybrid() if K == 4096 else tiny_hybrid()).backbone.mamba2_dims()
    assert md["d_ssm"] == K
    cw, cb, dtb, A, D = (t.to(DEV) for t in _mamba_params(md, 95))
    zx = _bf(M, md["d_in_proj"], scale=2.0, seed=96).to(DEV)
    rp = torch.full((M,), 9, dtype=torch.int32, device=DEV)
    ys, gzs = [], []
    for gz_g in (0, 1):  # the same step twice, from the same state
        ring = torch.zeros(M, 4, md["conv_dim"], dtype=torch.bfloat16, device=DEV)
        ssm = _bf(M, md["nheads"], 64, 128, scale=0.5, seed=97).to(DEV)
        y = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
        gz = torch.zeros(M, K, dtype=torch.float32, device=DEV)
        a = _args(L, md, zx, cw, cb, dtb, A, D, ring, ssm, y, M, rp)
        a.gz, a.gz_g = gz.data_ptr(), gz_g
        L.check(lib.zmi_mamba2_step(ctypes.byref(a), _sp()), "step")
        ys.append(y)
        gzs.append(gz)
    nrm = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    L.check(lib.zmi_gated_rmsnorm(ys[0].data_ptr(), K, zx.data_ptr(), md["d_in_proj"], M, K, w.data_ptr(), gc.EPS,
                                  nrm.data_ptr(), K, _sp()))
    torch.cuda.synchronize()
    assert gc.same_bits(ys[0], ys[1]) and not gc.same_bits(gzs[0], gzs[1])
    ptr = dict(W=Wp.data_ptr(), ln_w=w.data_ptr(), ld_aux=K)
    fused = _store(c, dict(ptr, X=ys[0].data_ptr(), aux=gzs[0].data_ptr()), c.form)
    fused_g = _store(cg, dict(ptr, X=ys[0].data_ptr(), aux=gzs[1].data_ptr()), cg.form)
    plain = _store(c, dict(W=Wp.data_ptr(), X=nrm.data_ptr()), pro="plain")
    assert gc.same_bits(fused, plain), c.name
    assert gc.same_bits(fused_g, plain), cg.name
    _check_sums(c, nrm, W, dict(W=Wp.data_ptr()))


def _own_sums(c, Wp, X, extra):
    """The kernel's own fp32 sums v [M][N] on the CPU: the F32 launch of the same packed weight, rows and prologue."""
    return _f32(c, dict(W=Wp.data_ptr(), X=X.data_ptr(), **extra), c.form).cpu()


@pytest.mark.parametrize("name,epi", [(c.name, e) for c, e in gc.EPILOGUE_CASES])
def test_epilogue_matches_emulation_of_own_sums(name, epi):
    c = gc.BY_NAME[name]
    swiglu = epi == "swiglu"
    W, Wp = _weights(c, swiglu)
    X = gc.rows_in(c).to(DEV)
    extra, keep = _ln_ptr(c) if c.pro == "ln" else ({}, None)  # keep: the device tensors behind `extra`  # noqa: F841
    v = _own_sums(c, Wp, X, extra)
    if swiglu and c.pro == "plain":  # the sums behind the SWIGLU columns are those of the fc1 rows ZMI_PACK_SWIGLU names
        bad = gc.sums_bad(v.to(DEV), X, W[gc.swiglu_rows(c.N).to(DEV)])
        assert bad.numel() == 0, (name, bad[:4].tolist())
    ptr = dict(W=Wp.data_ptr(), X=X.data_ptr(), **extra)
    if epi == "store":
        got = _store(c, ptr, c.form).cpu()
        assert gc.same_bits(got[: c.M, : c.nv].contiguous(), gc.emulate_store(v)[:, : c.nv].contiguous()), name
    elif epi == "residual":
        init = gc.sentinel16(c.M + 1, c.ldo)
        init[: c.M] = gc.residual_in(c)
        out = init.to(DEV)
        _launch(c, "residual", dict(ptr, out=out.data_ptr()), c.form, n_valid=c.nv)
        exp = init.clone()
        exp[: c.M, : c.nv] = gc.emulate_residual(v, init[: c.M, : c.N])[:, : c.nv]
        assert gc.same_bits(out.cpu(), exp), name
    else:
        F, ldo = c.N // 2, c.N // 2 + 8
        out = gc.sentinel16(c.M + 1, ldo, device=DEV)
        _launch(c, "swiglu", dict(ptr, out=out.data_ptr()), c.form, ldo=ldo)
        out = out.cpu()
        assert (out[:, F:].view(torch.int16) == gc.SENT16).all() and (out[c.M].view(torch.int16) == gc.SENT16).all()
        ok, second, near = gc.swiglu_check(out[: c.M, :F].contiguous(), v)
        print(f"{name}: swiglu second-neighbour share {second.float().mean().item():.4f}, boundary share "
              f"{near.float().mean().item():.4f}, gates span {gc.swiglu_split(v)[1].abs().max().item():.1f}")
        assert ok.all(), (name, (~ok).nonzero()[:4].tolist())
        assert second.float().mean().item() <= gc.SWIGLU_SECOND_CAP, name


@pytest.mark.parametrize("name", [c.name for c in gc.LOGITS_CASES])
def test_logits_epilogue_layout_and_rounding(name):
    c = gc.BY_NAME[name]
    _, Wp = _weights(c)
    X = gc.rows_in(c, scale=3.0).to(DEV)
    extra, keep = _ln_ptr(c)  # noqa: F841
    v = _own_sums(c, Wp, X, extra)
    init = gc.sentinel32((c.M + 1) * 9 * 1026)
    out = init.to(DEV)
    _launch(c, "logits", dict(W=Wp.data_ptr(), X=X.data_ptr(), out=out.data_ptr(), **extra), c.form, n_valid=c.nv)
    assert gc.same_bits(out.cpu(), gc.emulate_logits(v, c.nv, init)), name


@pytest.mark.parametrize("name", [c.name for c in gc.QKV_CASES])
def test_qkv_epilogue_rope_and_cache_slots(name):
    c = gc.BY_NAME[name]
    hq, hkv, hd = c.heads
    _, Wp = _weights(c)
    X = gc.rows_in(c).to(DEV)
    v = _own_sums(c, Wp, X, {})
    pos, kv, rope = gc.qkv_inputs(c)
    q0 = gc.sentinel16(c.M + 1, c.ldo)
    k0, vt0 = gc.sentinel16(c.M, hkv, gc.SMAX, hd), gc.sentinel16(c.M, hkv, hd, gc.SMAX)
    q, kc, vt, dpos, dkv, drope = (t.to(DEV) for t in (q0, k0, vt0, pos, kv, rope))
    _launch(c, "qkv", dict(W=Wp.data_ptr(), X=X.data_ptr(), out=q.data_ptr(), row_kv=dkv.data_ptr(),
                           row_pos=dpos.data_ptr(), k_cache=kc.data_ptr(), v_cache=vt.data_ptr(), rope=drope.data_ptr()),
            c.form, heads=c.heads)
    eq, ek, ev = gc.emulate_qkv(v, c.heads, pos, kv, rope, q0, k0, vt0)
    assert gc.same_bits(q.cpu(), eq), (name, "q", (q.cpu().view(torch.int16) != eq.view(torch.int16)).nonzero()[:4].tolist())
    assert gc.same_bits(kc.cpu(), ek), (name, "k", (kc.cpu().view(torch.int16) != ek.view(torch.int16)).nonzero()[:4].tolist())
    assert gc.same_bits(vt.cpu(), ev), (name, "v", (vt.cpu().view(torch.int16) != ev.view(torch.int16)).nonzero()[:4].tolist())
