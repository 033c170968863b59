"""The three stand-alone row-norm kernels (zmi_rownorm.hip) at every width their dispatch accepts, against the fp64
references of tests/gemv_cases.py (MI355X only): every element within 1 bf16 ulp of the fp64 value, the rule of
layernorm_ref. M = 5: zmi_layernorm_rows takes 4 rows per workgroup, so the last one is partial; K = 512 and 1024 leave
waves of the workgroup-per-row kernels idle. Every leading dimension is K + 8 and every output starts as sentinels: the
gap columns and the row after the last keep them."""
import functools

import pytest
import torch

from tests import gemv_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS = (512, 1024, 2048, 4096)
M = 5


def _L():
    from zonos_vibes_amd import _lib
    return _lib


def _sp():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _case(K):
    """The inputs of a width (CPU bf16, read only) and the fp64 references with their tolerances."""
    x, r = gc.rnd(M, K, scale=1.5, seed=K + 1), gc.rnd(M, K, scale=2.0, seed=K + 2)
    w, b = (gc.rnd(K, scale=0.2, seed=K + 3) + 1).contiguous(), gc.rnd(K, scale=0.05, seed=K + 4)
    y, z = gc.rnd(M, K, scale=1.0, seed=K + 5), gc.rnd(M, K, scale=4.0, seed=K + 6)
    refs = {"ln": gc.layernorm_ref(x, w, b), "addln": gc.addln_ref(x, r, w, b), "ln_r": gc.layernorm_ref(r, w, b),
            "grms": gc.grms_ref(y, z, w)}
    return dict(x=x, r=r, w=w, b=b, y=y, z=z), refs


def _rows(t):
    """[M + 1][K + 8] on the device: t in [:M, :K], sentinels in the gap columns and the row after."""
    out = gc.sentinel16(M + 1, t.shape[1] + 8, device=DEV)
    out[:M, : t.shape[1]] = t.to(DEV)
    return out


def _check(name, K, out, ref_tol):
    ref, tol = ref_tol
    assert (out[:, K:].view(torch.int16) == gc.SENT16).all() and (out[M].view(torch.int16) == gc.SENT16).all(), name
    err = (out[:M, :K].double().cpu() - ref).abs() / tol
    print(f"{name} K={K}: max err {err.max().item():.3f} bf16 ulp")
    assert (err <= 1.0).all(), (name, K, err.max().item())


@pytest.mark.parametrize("K", KS)
def test_layernorm_rows_matches_fp64(K):
    L = _L()
    t, refs = _case(K)
    x, w, b = _rows(t["x"]), t["w"].to(DEV), t["b"].to(DEV)
    out = gc.sentinel16(M + 1, K + 8, device=DEV)
    L.check(L.lib().zmi_layernorm_rows(x.data_ptr(), K + 8, M, K, w.data_ptr(), b.data_ptr(), gc.EPS, out.data_ptr(),
                                       K + 8, _sp()))
    torch.cuda.synchronize()
    _check("layernorm_rows", K, out, refs["ln"])


@pytest.mark.parametrize("store", (1, 0))
@pytest.mark.parametrize("hidden", (True, False))
@pytest.mark.parametrize("K", KS)
def test_add_layernorm_matches_fp64(K, hidden, store):
    """hidden given: LayerNorm of x + residual, and with store_residual the residual becomes bf16(x + residual) (the
    same fp32 add and one rounding: compared exactly); hidden NULL: LayerNorm of the residual alone. Without a new
    residual to store the residual buffer is unchanged."""
    L = _L()
    t, refs = _case(K)
    x, r, w, b = _rows(t["x"]), _rows(t["r"]), t["w"].to(DEV), t["b"].to(DEV)
    r0 = r.clone()
    out = gc.sentinel16(M + 1, K + 8, device=DEV)
    L.check(L.lib().zmi_add_layernorm(x.data_ptr() if hidden else None, K + 8, r.data_ptr(), K + 8, M, K, w.data_ptr(),
                                      b.data_ptr(), gc.EPS, out.data_ptr(), K + 8, store, _sp()))
    torch.cuda.synchronize()
    _check(f"add_layernorm hidden={hidden} store={store}", K, out, refs["addln" if hidden else "ln_r"])
    want = r0.clone()
    if hidden and store:
        want[:M, :K] = (t["x"].float() + t["r"].float()).bfloat16().to(DEV)
    assert gc.same_bits(r, want), (K, hidden, store)


@pytest.mark.parametrize("K", KS)
def test_gated_rmsnorm_matches_fp64(K):
    L = _L()
    t, refs = _case(K)
    y, z, w = _rows(t["y"]), _rows(t["z"]), t["w"].to(DEV)
    out = gc.sentinel16(M + 1, K + 8, device=DEV)
    L.check(L.lib().zmi_gated_rmsnorm(y.data_ptr(), K + 8, z.data_ptr(), K + 8, M, K, w.data_ptr(), gc.EPS,
                                      out.data_ptr(), K + 8, _sp()))
    torch.cuda.synchronize()
    _check("gated_rmsnorm", K, out, refs["grms"])
