"""fp8 MLP weights in the many-row GEMM forms (MI355X only): gemm_rows_kernel over M8F8 bytes and fc2's split-K GEMM
(zmi_gemv_splitk_f8 / _f8_ln). Every test is an equality: the fp8 launch against the bf16 launch of the same form on
the dequantised weights, and against the fp8 tile loop (gemv_body, ZMI_OPT_FP8_ROWS 0).

The weights are test_gpu_fp8's: neighbouring columns of every 8-column group carry exponents 12 or more apart, so a
scale taken from the wrong column cannot pass. Every zmi_gemv_launch first asks zmi_gemv_form and requires the form
the test is about. Options are set per block and put back (tests.helpers.zmi_option)."""
import contextlib
import ctypes

import pytest
import torch

from tests.helpers import zmi_option
from tests.test_gpu_fp8 import _cond, _twins, weights
from tests.test_gpu_kernels import rnd, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
BODY, ROWS, ROWS_DENSE = 0, 1, 2
KIND = {1: ROWS, 3: ROWS_DENSE}
CANARY = -7.0


def _lib():
    from zonos_vibes_amd import _lib as L
    return L


@contextlib.contextmanager
def options(**kw):
    """zmi_option for several knobs: options(GEMM_ROWS=1, FP8_ROWS=0)."""
    L = _lib()
    with contextlib.ExitStack() as st:
        for k, v in kw.items():
            st.enter_context(zmi_option(getattr(L, "OPT_" + k), v))
        yield


def args_for(wt, X, out, ldo, n_valid, f8):
    """ZmiGemvArgs over the fp8 bytes of `wt` (tests.test_gpu_fp8.weights) or over its bf16 twin."""
    L = _lib()
    packed, ep, n_pad, twin = wt[:4]
    M, K = X.shape
    a = L.GemvArgs()
    a.W = (packed if f8 else twin[0]).data_ptr()
    a.X, a.M, a.N, a.K, a.ldx = X.data_ptr(), M, n_pad, K, K
    a.out, a.ldo, a.n_valid = out.data_ptr(), ldo, n_valid
    if f8:
        a.w_fmt, a.w_exp = L.WFMT_FP8, ep.data_ptr()
    return a


def launch(wt, X, epi, out, ldo, n_valid, f8, kind):
    """zmi_gemv_launch in the form `kind`, which zmi_gemv_form must report first."""
    L = _lib()
    a = args_for(wt, X, out, ldo, n_valid, f8)
    f = L.GemvForm()
    L.check(L.lib().zmi_gemv_form(ctypes.byref(a), epi, ctypes.byref(f)), "form")
    assert f.kind == kind, (f.kind, kind, X.shape[0], a.N)
    L.check(L.lib().zmi_gemv_launch(ctypes.byref(a), epi, stream_ptr()), "gemv")
    torch.cuda.synchronize()
    return out


def three_ways(wt, X, epi, make_out, ldo, n_valid, rows_opt):
    """(fp8 many-row form, bf16 many-row form on the twin, fp8 tile loop) outputs of one launch."""
    with options(GEMM_ROWS=rows_opt, FP8_ROWS=1):
        got = launch(wt, X, epi, make_out(), ldo, n_valid, True, KIND[rows_opt])
        ref = launch(wt, X, epi, make_out(), ldo, n_valid, False, KIND[rows_opt])
    with options(GEMM_ROWS=rows_opt, FP8_ROWS=0):
        loop = launch(wt, X, epi, make_out(), ldo, n_valid, True, BODY)
    return got, ref, loop


# ------------------------------------------------------------------ the many-row form
@pytest.mark.parametrize("rows_opt", [1, 3])
@pytest.mark.parametrize("N,n_valid", [(64, 64), (136, 130)])
def test_rows_form_f32_sums(N, n_valid, rows_opt):
    """One column block, and 17 groups (a partial column block; an odd group count: the dense-pair clamp); every
    workgroup runs one tile: a tile past the first, a full last tile, one row into a tile, a partial one."""
    L = _lib()
    wt = weights(n_valid, 2048, n_pad=N)
    for M in (65, 80, 81, 130):
        X = rnd(M, 2048, seed=20 + M)
        got, ref, loop = three_ways(wt, X, L.EPI_F32,
                                    lambda: torch.full((M, N), CANARY, dtype=torch.float32, device=DEV), N, n_valid,
                                    rows_opt)
        assert torch.equal(got, ref), (M, (got != ref).nonzero()[:4].tolist())
        assert torch.equal(got, loop), (M, (got != loop).nonzero()[:4].tolist())
        assert (got[:, n_valid:] == CANARY).all() and (got[:, :n_valid] != CANARY).any()


@pytest.mark.parametrize("rows_opt", [1, 3])
def test_rows_form_tile_loop_in_a_workgroup(rows_opt):
    """N 2048, M 322: 21 tiles in 8 row groups, the last one partial (the two-ahead DMA, the arrival counter)."""
    L = _lib()
    M, N = 322, 2048
    wt = weights(N, 2048)
    X = rnd(M, 2048, seed=7)
    got, ref, loop = three_ways(wt, X, L.EPI_F32, lambda: torch.zeros(M, N, dtype=torch.float32, device=DEV), N, N,
                                rows_opt)
    assert torch.equal(got, ref) and torch.equal(got, loop)
    assert got.abs().max() > 0


@pytest.mark.parametrize("M", [17, 48, 49])
def test_rows_form_real_fc1_swiglu(M):
    """fc1 as the engine launches it: N 16384 in SWIGLU pack mode (value / gate rows interleaved per group, the
    exponents permuted with them), out [M][8192]; 2 to 4 tiles in one workgroup."""
    L = _lib()
    N, F = 16384, 8192
    wt = weights(N, 2048, mode=L.PACK_SWIGLU)
    X = rnd(M, 2048, seed=30 + M)
    for rows_opt in (1, 3):
        got, ref, loop = three_ways(wt, X, L.EPI_SWIGLU, lambda: torch.zeros(M, F, dtype=torch.bfloat16, device=DEV),
                                    F, N, rows_opt)
        assert torch.equal(got, ref), rows_opt
        assert torch.equal(got, loop), rows_opt
        assert got.float().abs().max() > 0


@pytest.mark.parametrize("M", [65, 130])
def test_rows_form_residual(M):
    """out += bf16(sum) over a non-zero residual (the operand pieces of the last wave)."""
    L = _lib()
    N = 64
    wt = weights(N, 2048)
    X = rnd(M, 2048, seed=40 + M)
    res = rnd(M, N, scale=2.0, seed=41)
    for rows_opt in (1, 3):
        got, ref, loop = three_ways(wt, X, L.EPI_RESIDUAL, res.clone, N, N, rows_opt)
        assert torch.equal(got, ref) and torch.equal(got, loop), rows_opt
        assert not torch.equal(got, res)


@pytest.mark.parametrize("rows_opt", [1, 3])
def test_rows_form_is_batch_invariant(rows_opt):
    """Rows of the 130-row many-row launch equal the same rows launched alone on the tile loop."""
    L = _lib()
    N, big = 64, 130
    wt = weights(N, 2048)
    X = rnd(big, 2048, seed=4)
    with options(GEMM_ROWS=rows_opt, FP8_ROWS=1):
        ref = launch(wt, X, L.EPI_F32, torch.zeros(big, N, dtype=torch.float32, device=DEV), N, N, True, KIND[rows_opt])
        for lo, hi in ((0, 1), (3, 20), (129, 130)):
            small = torch.zeros(hi - lo, N, dtype=torch.float32, device=DEV)
            launch(wt, X[lo:hi].contiguous(), L.EPI_F32, small, N, N, True, BODY)
            assert torch.equal(small, ref[lo:hi]), (lo, hi)


# ------------------------------------------------------------------ split-K over fp8 bytes
def splitk8(wt, X, out, N, part=None, ln=None, xn=None):
    L = _lib()
    M = X.shape[0]
    a = args_for(wt, X, out, N, N, True)
    nf = L.lib().zmi_gemv_splitk_floats(M, N)
    part = torch.full((nf,), float("nan"), dtype=torch.float32, device=DEV) if part is None else part
    if ln is None:
        rc = L.lib().zmi_gemv_splitk_f8(ctypes.byref(a), L.EPI_RESIDUAL, part.data_ptr(), part.numel(), stream_ptr())
    else:
        rc = L.lib().zmi_gemv_splitk_f8_ln(ctypes.byref(a), L.EPI_RESIDUAL, part.data_ptr(), part.numel(),
                                           ln[0].data_ptr(), ln[1].data_ptr(), 1e-5, xn.data_ptr(), xn.shape[1],
                                           stream_ptr())
    L.check(rc, "gemv_splitk_f8")
    torch.cuda.synchronize()
    return out


def gemv_residual_refs(wt, X, res, N):
    """zmi_gemv_launch (gemv_body at K = 8192) over the fp8 weights and over the bf16 twin."""
    L = _lib()
    r8 = launch(wt, X, L.EPI_RESIDUAL, res.clone(), N, N, True, BODY)
    rb = launch(wt, X, L.EPI_RESIDUAL, res.clone(), N, N, False, BODY)
    return r8, rb


@pytest.mark.parametrize("N", [64, 128])
def test_splitk_f8_equals_gemv(N):
    """K 8192, RESIDUAL: one and many row groups, M8 and dense pairs, one and several tiles per stage; the partial
    buffer NaN-filled beforehand."""
    wt = weights(N, 8192)
    for M in (1, 16, 17, 65, 130):
        X = rnd(M, 8192, seed=50 + M)
        res = rnd(M, N, scale=2.0, seed=51)
        r8, rb = gemv_residual_refs(wt, X, res, N)
        assert torch.equal(r8, rb) and not torch.equal(r8, res)
        for wgs in (0, 1024):
            for rows_opt in (1, 3):
                for stage in (1, 0):
                    with options(SPLITK_WGS=wgs, GEMM_ROWS=rows_opt, SPLITK_STAGE=stage):
                        got = splitk8(wt, X, res.clone(), N)
                    assert torch.equal(got, r8), (M, wgs, rows_opt, stage, (got != r8).nonzero()[:4].tolist())


def test_splitk_f8_fc2_shape_under_the_defaults():
    N, M = 2048, 322
    wt = weights(N, 8192)
    X = rnd(M, 8192, seed=60)
    res = rnd(M, N, scale=2.0, seed=61)
    r8, rb = gemv_residual_refs(wt, X, res, N)
    got = splitk8(wt, X, res.clone(), N)
    assert torch.equal(got, r8) and torch.equal(got, rb)


@pytest.mark.parametrize("M", [16, 33, 128])
def test_splitk_f8_ln_equals_gemv_then_layernorm(M):
    L = _lib()
    N = 2048
    wt = weights(N, 8192)
    X = rnd(M, 8192, seed=70 + M)
    res = rnd(M, N, scale=2.0, seed=71)
    lw, lb = (rnd(N, scale=0.1, seed=10) + 1).contiguous(), rnd(N, scale=0.02, seed=11)
    r8, _ = gemv_residual_refs(wt, X, res, N)
    xn_ref = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    L.check(L.lib().zmi_layernorm_rows(r8.data_ptr(), N, M, N, lw.data_ptr(), lb.data_ptr(), 1e-5, xn_ref.data_ptr(), N,
                                       stream_ptr()), "ln")
    xn = torch.zeros_like(xn_ref)
    got = splitk8(wt, X, res.clone(), N, ln=(lw, lb), xn=xn)
    assert torch.equal(got, r8) and torch.equal(xn, xn_ref)
    assert xn.float().abs().max() > 0


def test_splitk_f8_refusals_write_nothing():
    L = _lib()
    lib = L.lib()
    M = 16
    wt = weights(64, 8192)
    wt2k = weights(64, 2048)
    wt72 = weights(72, 8192)
    X = rnd(M, 8192, seed=5)

    def call(a, epi, part, nf):
        return lib.zmi_gemv_splitk_f8(ctypes.byref(a), epi, part.data_ptr(), nf, stream_ptr())

    def case(w, N, K, epi, edit=None, short=0):
        out = rnd(M, N, scale=2.0, seed=6)
        before = out.clone()
        nf = lib.zmi_gemv_splitk_floats(M, N)
        part = torch.full((nf,), 3.0, dtype=torch.float32, device=DEV)
        a = args_for(w, X[:, :K].contiguous(), out, N, N, True)
        if edit:
            edit(a)
        assert call(a, epi, part, nf - short) != 0 and lib.zmi_last_error()
        torch.cuda.synchronize()
        assert torch.equal(out, before) and (part == 3.0).all()

    def bf16(a):
        a.w_fmt = L.WFMT_BF16

    def no_exp(a):
        a.w_exp = None

    case(wt, 64, 8192, L.EPI_RESIDUAL, bf16)                 # bf16 w_fmt
    case(wt, 64, 8192, L.EPI_RESIDUAL, no_exp)               # w_exp NULL
    case(wt2k, 64, 2048, L.EPI_RESIDUAL)                     # K 2048
    case(wt, 64, 8192, L.EPI_STORE)                          # EPI_STORE
    case(wt72, 72, 8192, L.EPI_RESIDUAL)                     # N 72
    case(wt, 64, 8192, L.EPI_RESIDUAL, short=1)              # part too small


# ------------------------------------------------------------------ engine level
@pytest.fixture(scope="module")
def prod_twins8():
    from zonos_vibes_amd.config import transformer_config
    return _twins(transformer_config(2048, 2, 16, 4, 8192), max_slots=8, max_seqlen=64, max_prefill=32)


def _kinds(e, rows):
    return [k for k, _ in e._plan(rows, "none")]


def test_engine_fp8_rows_production_dims(prod_twins8):
    """8 utterances x 24 frames over 8 slots (graphs on, as generate_batch always runs): the batched prefill runs
    fc1 in the many-row form and fc2 through zmi_gemv_splitk_f8, the 16-row decode steps fc2 as splitk8ln items.
    fp8_rows on, off (the tile loop) and the bf16 twin agree on every code and on the final logits."""
    L = _lib()
    m8, mb = prod_twins8
    e = m8.engine
    assert e.fp8_rows is True and e.S == 8
    conds = [_cond(80 + i, 9 + (11 * i) // 7, 2048) for i in range(8)]
    assert min(c.shape[1] for c in conds) == 9 and max(c.shape[1] for c in conds) == 20
    seeds = list(range(1, 9))

    def run(m, sp):
        out = m.generate_batch(conds, None, max_new_tokens=24, sampling_params=sp, seeds=seeds, max_slots=8)
        m.engine.check_errors()
        return out, m.engine.logits.clone()

    for sp in (dict(temperature=0.0), dict(min_p=0.1)):
        try:
            e.fp8_rows = True
            e._build_plan()
            fc2 = e._gemv(e.w["layers"][0]["fc2"], e.h, 16, 2048, 8192, L.EPI_RESIDUAL, e.x, 2048)
            assert e._use_splitk8(*fc2) is True and e._use_splitk(*fc2) is False
            # one splitk8ln per layer (fc2); the bf16 out_proj keeps its splitkln
            assert _kinds(e, 16).count("splitk8ln") == 2 and _kinds(e, 16).count("splitkln") == 2
            on, logits_on = run(m8, sp)
            assert m8.engine is e
            e.fp8_rows = False
            e._build_plan()
            assert e._use_splitk8(*fc2) is False
            assert "splitk8ln" not in _kinds(e, 16)
            off, logits_off = run(m8, sp)
            assert L.lib().zmi_get_option(L.OPT_FP8_ROWS) == 1   # put back after every launch
        finally:
            e.fp8_rows = True
            e._build_plan()
        twin, logits_twin = run(mb, sp)
        assert _kinds(mb.engine, 16).count("splitkln") == 4   # the bf16 twin: out_proj and fc2
        assert all(o.shape[-1] == 24 for o in on)
        assert all(torch.equal(a, b) for a, b in zip(on, off)), sp
        assert all(torch.equal(a, b) for a, b in zip(on, twin)), sp
        assert torch.equal(logits_on, logits_off) and torch.equal(logits_on, logits_twin), sp
