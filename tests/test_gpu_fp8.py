"""weights="fp8" on the GPU: the GEMV with E4M3 weights equals, bit for bit, the bf16 GEMV on the dequantised weights
(every 2^e q is a bf16, so that twin exists), at the kernel and at the engine level (MI355X only).

The weights are test_quant_cpu's edge rows: neighbouring columns of every 8-column group carry exponents 12 or more
apart, so a scale read from the wrong column or a mis-permuted exponent array cannot pass. Activations are ~1."""
import ctypes
import functools

import pytest
import torch

from tests.stream_cases import random_codes
from tests.test_gpu_kernels import gemv, pack, rnd, stream_ptr
from tests.test_quant_cpu import edge_weight
from zonos_vibes_amd import quant

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lib():
    from zonos_vibes_amd import _lib as L
    return L


@functools.lru_cache(maxsize=None)
def weights(n_src, k, mode=0, n_pad=None):
    """(fp8 packed bytes, packed exponents, n_pad, the bf16 twin packed by zmi_pack_weight, dequantised bf16 [n][k]);
    quantised on the GPU, which must give the CPU's codes."""
    w = edge_weight(n_src, k, seed=n_src + k)
    q, e = quant.quantize_fp8(w.to(DEV))
    qc, ec = quant.quantize_fp8(w)
    assert torch.equal(q.cpu(), qc) and torch.equal(e.cpu(), ec)
    n_pad = n_pad or (n_src + 7) // 8 * 8
    packed, ep = quant.pack_m8f8(q, e, n_pad, mode)
    deq = quant.dequantize_fp8(q, e)
    assert torch.equal(deq.cpu(), quant.dequantize_fp8(qc, ec))
    return packed, ep, n_pad, pack(deq, mode, n_pad), deq


def gemv8(wt, X, epi, out, ldo, n_valid, ln=None, groups=0):
    packed, ep, n_pad = wt[:3]
    L = _lib()

    def fmt(a):
        a.w_fmt, a.w_exp = L.WFMT_FP8, ep.data_ptr()
    return gemv(None, X, epi, out, ldo, n_valid=n_valid, ln=ln, packed=(packed, n_pad), extra=fmt, groups=groups)


def ln_params(k):
    return (rnd(k, scale=0.1, seed=10) + 1).contiguous(), rnd(k, scale=0.02, seed=11)


# (K, N packed columns, n_valid rows of the weight): 130 rows padded to 136 columns (17 groups: odd, so G = 2 clamps its
# last group); 24 = 3 groups. LayerNorm'd launches exist for K <= 2048 only (fc2, K = 8192, is plain)
SHAPES = [(512, 64, 64), (2048, 64, 64), (2048, 136, 130), (8192, 64, 64), (8192, 24, 24)]
CASES = [(k, n, v, ln) for k, n, v in SHAPES for ln in ((False, True) if k <= 2048 else (False,))]


@pytest.mark.parametrize("K,N,n_valid,ln", CASES)
def test_fp8_gemv_equals_bf16_twin(K, N, n_valid, ln):
    """EPI_F32 sums: a lone row, the full tile, one row into a second tile, the multi-tile loop with a partial last
    tile (RT = 16, K = 8192: 8); with and without the LayerNorm prologue (K <= 2048); 1 and 2 column groups."""
    L = _lib()
    wt = weights(n_valid, K, n_pad=N)
    lnp = ln_params(K) if ln else None
    for M in ((1, 2, 8, 9, 19) if K == 8192 else (1, 2, 16, 17, 33)):
        X = rnd(M, K, seed=20 + M)
        for groups in ((1, 2) if K in (2048, 8192) else (1,)):
            ref = torch.full((M, N), -7.0, dtype=torch.float32, device=DEV)
            got = ref.clone()
            gemv(None, X, L.EPI_F32, ref, N, n_valid=n_valid, ln=lnp, packed=wt[3], groups=groups)
            gemv8(wt, X, L.EPI_F32, got, N, n_valid, ln=lnp, groups=groups)
            assert torch.equal(got, ref), (M, groups, (got != ref).nonzero()[:4].tolist())
            assert (got[:, n_valid:] == -7.0).all() and (got[:, :n_valid] != -7.0).any()


@pytest.mark.parametrize("K", [2048, 512])
def test_fp8_swiglu_equals_bf16_twin(K):
    """fc1's epilogue and pack mode (value / gate rows interleaved per group, the exponents with them), decode
    (LayerNorm prologue) and many-row (plain) launches."""
    L = _lib()
    n, f = 128, 64
    wt = weights(n, K, mode=L.PACK_SWIGLU)
    for M, lnp in ((2, ln_params(K)), (17, None), (2, None), (17, ln_params(K))):
        X = rnd(M, K, seed=30 + M)
        ref = torch.zeros(M, f, dtype=torch.bfloat16, device=DEV)
        got = torch.zeros_like(ref)
        gemv(None, X, L.EPI_SWIGLU, ref, f, n_valid=n, ln=lnp, packed=wt[3])
        gemv8(wt, X, L.EPI_SWIGLU, got, f, n, ln=lnp)
        assert torch.equal(got, ref), (M, lnp is not None)
        assert ref.float().abs().max() > 0


def test_fp8_residual_equals_bf16_twin():
    """fc2's epilogue: out += bf16(sum), over a non-zero residual."""
    L = _lib()
    K, N = 8192, 64
    wt = weights(N, K)
    for M in (2, 9):
        X = rnd(M, K, seed=40 + M)
        res = rnd(M, N, scale=2.0, seed=41)
        ref, got = res.clone(), res.clone()
        gemv(None, X, L.EPI_RESIDUAL, ref, N, n_valid=N, packed=wt[3])
        gemv8(wt, X, L.EPI_RESIDUAL, got, N, N)
        assert torch.equal(got, ref), M
        assert not torch.equal(ref, res)


@pytest.mark.parametrize("M,N,K", [(2, 64, 2048), (9, 64, 8192)])
def test_fp8_f32_sums_match_fp64(M, N, K):
    """The bound of test_gemv_f32_sums_match_fp64, on the dequantised weights."""
    L = _lib()
    wt = weights(N, K)
    X = rnd(M, K, seed=2)
    out = torch.zeros(M, N, dtype=torch.float32, device=DEV)
    gemv8(wt, X, L.EPI_F32, out, N, N)
    W = wt[4]
    ref = X.double() @ W.double().t()
    bound = (X.double().abs() @ W.double().abs().t()) * 2e-6 + 1e-30
    assert ((out.double() - ref).abs() <= bound).all()


@pytest.mark.parametrize("K,ln", [(2048, True), (8192, False)])
def test_fp8_gemv_is_batch_invariant(K, ln):
    """Rows [lo:hi] of a 40-row launch equal the same rows launched alone."""
    L = _lib()
    N, big = 64, 40
    wt = weights(N, K)
    lnp = ln_params(K) if ln else None
    X = rnd(big, K, seed=4)
    ref = torch.zeros(big, N, dtype=torch.float32, device=DEV)
    gemv8(wt, X, L.EPI_F32, ref, N, N, ln=lnp)
    for lo, hi in ((0, 1), (0, 16), (3, 20), (39, 40)):
        small = torch.zeros(hi - lo, N, dtype=torch.float32, device=DEV)
        gemv8(wt, X[lo:hi].contiguous(), L.EPI_F32, small, N, N, ln=lnp)
        assert torch.equal(small, ref[lo:hi]), (lo, hi)


def test_splitk_refuses_fp8_weights():
    """The split-K GEMM reads bf16 only: handed fp8 weights it returns an error before any launch and writes nothing."""
    L = _lib()
    K, N, M = 8192, 64, 16
    wt = weights(N, K)
    X = rnd(M, K, seed=5)
    out = rnd(M, N, scale=2.0, seed=6)
    before = out.clone()
    nf = L.lib().zmi_gemv_splitk_floats(M, N)
    part = torch.full((nf,), 3.0, dtype=torch.float32, device=DEV)
    a = L.GemvArgs()
    a.W, a.X, a.M, a.N, a.K, a.ldx = wt[0].data_ptr(), X.data_ptr(), M, N, K, K
    a.out, a.ldo, a.n_valid = out.data_ptr(), N, N
    a.w_fmt, a.w_exp = L.WFMT_FP8, wt[1].data_ptr()
    assert L.lib().zmi_gemv_splitk(ctypes.byref(a), L.EPI_RESIDUAL, part.data_ptr(), nf, stream_ptr()) != 0
    assert b"bf16 weights only" in L.lib().zmi_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, before) and (part == 3.0).all()


def test_gemv_launch_refuses_fp8_where_it_is_not_built():
    L = _lib()
    wt = weights(64, 2048)
    X = rnd(2, 2048, seed=7)
    out = torch.zeros(2, 64, dtype=torch.bfloat16, device=DEV)
    a = L.GemvArgs()
    a.W, a.X, a.M, a.N, a.K, a.ldx = wt[0].data_ptr(), X.data_ptr(), 2, 64, 2048, 2048
    a.out, a.ldo, a.n_valid = out.data_ptr(), 64, 64
    a.w_fmt = L.WFMT_FP8
    assert L.lib().zmi_gemv_launch(ctypes.byref(a), L.EPI_F32, stream_ptr()) != 0      # no exponents
    a.w_exp = wt[1].data_ptr()
    assert L.lib().zmi_gemv_launch(ctypes.byref(a), L.EPI_STORE, stream_ptr()) != 0    # not an MLP epilogue
    a.w_fmt = 2
    assert L.lib().zmi_gemv_launch(ctypes.byref(a), L.EPI_F32, stream_ptr()) != 0      # unknown format
    torch.cuda.synchronize()
    assert not out.any()


# ------------------------------------------------------------------ engine level
def _twins(cfg, **kw):
    """(fp8 model, bf16 model on the same synthetic weights with the quantised tensors replaced by their dequantised
    values)."""
    from zonos_vibes_amd.model import Zonos
    m8 = Zonos.synthetic(cfg, DEV, zero_eos=True, weights="fp8", **kw)
    mb = Zonos.synthetic(cfg, DEV, zero_eos=True, **kw)
    over = m8.engine.dequantized_state_dict_overrides()
    L = cfg.backbone.n_layer
    assert sorted(over) == sorted(f"backbone.layers.{i}.mlp.{n}.weight" for i in range(L) for n in ("fc1", "fc2"))
    sd = mb.engine.synthetic_state_dict(0, zero_eos=True)
    assert all(over[k].shape == sd[k].shape and not torch.equal(over[k], sd[k]) for k in over)
    sd.update(over)
    mb.engine.load_state_dict(sd)
    return m8, mb


def _cond(seed, lc, d):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(2, lc, d, generator=g) * 0.5).to(torch.bfloat16).to(DEV)


@pytest.fixture(scope="module")
def tiny_twins():
    from zonos_vibes_amd.config import tiny_transformer
    return _twins(tiny_transformer(2), max_seqlen=128, max_prefill=64)


@pytest.mark.parametrize("sp", [dict(temperature=0.0), dict(min_p=0.1)], ids=["greedy", "min_p"])
def test_fp8_generate_equals_bf16_twin(tiny_twins, sp):
    m8, mb = tiny_twins
    assert "weights=fp8" in repr(m8) and "weights=bf16" in repr(mb)
    cond = _cond(3, 11, 512)
    out = []
    for m in (m8, mb):
        torch.manual_seed(1234)
        out.append(m.generate(cond, max_new_tokens=24, sampling_params=sp, progress_bar=False))
    assert out[0].shape[-1] == 24 and torch.equal(out[0], out[1])
    assert torch.equal(m8.engine.logits, mb.engine.logits)


def test_fp8_generate_batch_equals_bf16_twin(tiny_twins):
    """3 utterances over 2 slots, one with a 12-frame audio prefix (its prefill runs 2 x 22 > 16 rows through the tile
    loop); the engines are rebuilt for 2 slots (_ensure_capacity) and keep their format."""
    m8, mb = tiny_twins
    conds = [_cond(40 + i, 9 + i, 512) for i in range(3)]
    prefixes = [None, random_codes(12, seed=5).to(DEV), None]
    out = [m.generate_batch(conds, prefixes, max_new_tokens=[20, 14, 9], sampling_params=dict(min_p=0.1),
                            seeds=[1, 2, 3], max_slots=2) for m in (m8, mb)]
    assert m8.engine.S == 2 and m8.engine.weights == "fp8" and mb.engine.weights == "bf16"
    assert m8.engine.w["layers"][0]["fc1"].dtype == torch.uint8
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert [o.shape[-1] for o in out[0]] == [20, 12 + 14, 9]   # (the prefix's frames come back with the new ones)


@pytest.fixture(scope="module")
def prod_twins():
    from zonos_vibes_amd.config import transformer_config
    return _twins(transformer_config(2048, 2, 16, 4, 8192), max_seqlen=64, max_prefill=32)


def test_fp8_generate_equals_bf16_twin_production_dims(prod_twins):
    """d 2048, F 8192, 16 / 4 heads, 2 layers: the real fc1 / fc2 instantiations (decode: 2 groups / K = 8192; the
    24-row prefill: the 4-group tile loop) behind the fused attention block and its prefetch of fc1's head."""
    m8, mb = prod_twins
    cond = _cond(9, 12, 2048)
    out = []
    for m in (m8, mb):
        torch.manual_seed(99)
        out.append(m.generate(cond, max_new_tokens=12, sampling_params=dict(temperature=0.0), progress_bar=False))
    assert out[0].shape[-1] == 12 and torch.equal(out[0], out[1])
    assert torch.equal(m8.engine.logits, mb.engine.logits)
    for m, want in ((m8, False), (mb, True)):  # 16-row fc2: split-K for bf16, never for fp8
        e = m.engine
        item = e._gemv(e.w["layers"][0]["fc2"], e.h_pre, 16, 2048, 8192, _lib().EPI_RESIDUAL, e.x_pre, 2048)
        assert e._use_splitk(*item) is want


def test_fp8_mlp_weights_take_half_the_bytes(prod_twins):
    m8, mb = prod_twins
    for l8, lb in zip(m8.engine.w["layers"], mb.engine.w["layers"]):
        for key, n, k in (("fc1", 2 * 8192, 2048), ("fc2", 2048, 8192)):
            b8, bb = (t.numel() * t.element_size() for t in (l8[key], lb[key]))
            assert bb == 2 * n * k and b8 == bb // 2 + n      # one byte per weight + one exponent per column
        for key in ("qkv", "out", "ln1_w", "ln2_w"):
            assert l8[key].dtype == torch.bfloat16 and l8[key].shape == lb[key].shape
    assert m8.engine.w["heads"].dtype == torch.bfloat16 and m8.engine.w["emb"].dtype == torch.bfloat16


def test_fp8_hybrid_is_not_implemented():
    from zonos_vibes_amd.config import tiny_hybrid
    from zonos_vibes_amd.model import Zonos
    with pytest.raises(NotImplementedError):
        Zonos.synthetic(tiny_hybrid(), DEV, weights="fp8")
    with pytest.raises(ValueError):
        Zonos.synthetic(tiny_hybrid(), DEV, weights="fp4")
