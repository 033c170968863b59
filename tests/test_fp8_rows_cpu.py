"""fp8 MLP weights in the many-row launch forms, the host side (no GPU): which form zmi_gemv_form reports for fp8
arguments on both sides of every rows_form edge, what stays refused, the new option and entry points, and the engine's
_use_splitk8 truth table. The bits are tests/test_gpu_fp8_rows.py's."""
import ctypes
import types

import pytest
import torch

from tests.gemv_cases import EPI, make_args
from tests.helpers import zmi_option

FORM_BODY, FORM_ROWS, FORM_ROWS_DENSE = 0, 1, 2
# (M, N) on both sides of each rows_form edge: M > 64; M > 32 with N >= 3072; N >= 8192 with M > 16 (one tile: never)
EDGES = [((64, 64), False), ((65, 64), True), ((32, 3072), False), ((33, 3072), True), ((16, 16384), False),
         ((17, 16384), True)]
# gemv_body's column groups per workgroup at K = 2048, plain rows (groups_for): 4 over > 16 rows x >= 256 groups, 2 for
# >= 384 groups over 5..16 rows, else 1
BODY_G = {(64, 64): 1, (65, 64): 1, (32, 3072): 4, (33, 3072): 4, (16, 16384): 2, (17, 16384): 4}


def _L():
    from zonos_vibes_amd import _lib
    return _lib


def fp8_args(L, M, N, K=2048, w_exp=64):
    a = make_args(L, M, N, K)
    a.w_fmt = L.WFMT_FP8
    a.w_exp = w_exp
    return a


def form(L, a, epi):
    f = L.GemvForm()
    rc = L.lib().zmi_gemv_form(ctypes.byref(a), EPI[epi], ctypes.byref(f))
    return None if rc else (f.kind, f.G, f.W, f.NL, f.RT, f.ntw, f.pro)


@pytest.mark.parametrize("epi", ["swiglu", "residual", "f32"])
@pytest.mark.parametrize("mn,rows", EDGES)
def test_fp8_form_on_both_sides_of_each_rows_form_edge(mn, rows, epi):
    L = _L()
    M, N = mn
    a = fp8_args(L, M, N)
    body = (FORM_BODY, BODY_G[mn], 4, 8, 16, int(M <= 16), 0)
    with zmi_option(L.OPT_FP8_ROWS, 1):
        for opt, kind in ((3, FORM_ROWS_DENSE), (1, FORM_ROWS)):
            with zmi_option(L.OPT_GEMM_ROWS, opt):
                assert form(L, a, epi) == ((kind, 8, 4, 8, 16, 0, 0) if rows else body), (opt, mn)
        with zmi_option(L.OPT_GEMM_ROWS, 0):
            assert form(L, a, epi) == body
    with zmi_option(L.OPT_FP8_ROWS, 0):
        for opt in (3, 1, 0):
            with zmi_option(L.OPT_GEMM_ROWS, opt):
                assert form(L, a, epi) == body, (opt, mn)


def test_fp8_form_follows_the_bf16_form_of_the_same_launch():
    """Same thresholds, same grid: the fp8 launch is dispatched where the bf16 one is."""
    L = _L()
    for (M, N), _ in EDGES:
        a8, ab = fp8_args(L, M, N), make_args(L, M, N, 2048)
        for opt in (3, 1):
            with zmi_option(L.OPT_GEMM_ROWS, opt):
                f8, fb = L.GemvForm(), L.GemvForm()
                assert L.lib().zmi_gemv_form(ctypes.byref(a8), EPI["f32"], ctypes.byref(f8)) == 0
                assert L.lib().zmi_gemv_form(ctypes.byref(ab), EPI["f32"], ctypes.byref(fb)) == 0
                assert all(getattr(f8, k) == getattr(fb, k) for k, _ in L.GemvForm._fields_), (M, N, opt)


def test_fp8_launches_that_stay_refused():
    L = _L()
    M = 130
    assert form(L, fp8_args(L, M, 64), "store") is None            # a plain fp8 STORE at K = 2048
    assert form(L, fp8_args(L, M, 64, K=512), "store") is None
    assert form(L, fp8_args(L, M, 64, K=8192), "store") is None
    q = make_args(L, M, 3072, 2048, heads=(16, 4, 128))
    q.w_fmt, q.w_exp = L.WFMT_FP8, 64
    assert form(L, q, "qkv") is None
    assert form(L, fp8_args(L, M, 64), "logits") is None
    assert form(L, fp8_args(L, M, 64, w_exp=None), "f32") is None   # no exponents
    assert form(L, fp8_args(L, M, 64, w_exp=68), "f32") is None     # not 8-byte aligned
    u = fp8_args(L, M, 64)
    u.w_fmt = 2
    assert form(L, u, "f32") is None                                # unknown format
    assert form(L, fp8_args(L, M, 64), "f32") is not None


def test_new_symbols_and_option():
    L = _L()
    assert "zmi_gemv_splitk_f8" in L.EXPORTED and "zmi_gemv_splitk_f8_ln" in L.EXPORTED
    lib = L.lib()
    assert lib.zmi_gemv_splitk_f8 is not None and lib.zmi_gemv_splitk_f8_ln is not None
    assert L.OPT_FP8_ROWS == 18 and lib.zmi_get_option(18) == 1
    assert lib.zmi_set_option(19, 1) != 0 and b"unknown option" in lib.zmi_last_error()
    assert lib.zmi_version() == L.ABI_VERSION == 10


def test_use_splitk8_truth_table():
    """The method reads the engine's switches and the size of splitk_part only: no GPU needed."""
    L = _L()
    from zonos_vibes_amd.engine import HipEngine
    e = types.SimpleNamespace(fp8_rows=True, splitk_rows=16, splitk_part=torch.empty(8 * 128 * 2048, dtype=torch.float32))
    use8 = lambda a, epi=L.EPI_RESIDUAL: HipEngine._use_splitk8(e, a, epi)  # noqa: E731

    def args(M=16, N=2048, K=8192, fmt=L.WFMT_FP8, **kw):
        a = make_args(L, M, N, K)
        a.w_fmt, a.w_exp = fmt, 64
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert use8(args()) is True and use8(args(M=128)) is True
    assert use8(args(M=15)) is False                       # below splitk_rows
    assert use8(args(M=129)) is False                      # part too small
    assert use8(args(fmt=L.WFMT_BF16)) is False            # bf16: _use_splitk's
    assert use8(args(K=2048)) is False and use8(args(K=4096)) is False
    assert use8(args(), L.EPI_STORE) is False and use8(args(), L.EPI_F32) is False
    assert use8(args(N=2056)) is False                     # N % 64
    assert use8(args(n_valid=2040)) is False               # padded
    assert use8(args(ln_w=64)) is False                    # a LayerNorm prologue
    assert use8(args(pro=L.PRO_ADDLN)) is False
    e.fp8_rows = False
    assert use8(args()) is False
    e.fp8_rows, e.splitk_rows = True, 0
    assert use8(args()) is False
    e.splitk_rows = 64
    assert use8(args(M=63)) is False and use8(args(M=64)) is True
