"""mixer_weights="fp8" on the GPU: every launch that reads the Mamba2 projections as E4M3 bytes equals, bit for bit, the
bf16 launch on the dequantised weights (every 2^e q is a bf16, so that twin exists): the ADDLN / GRMS / GRMS_G / plain
store GEMVs, zmi_mamba_block, the expansion kernel of the prefill, and the engine (MI355X only).

As in tests/test_gpu_fp8.py the weights are test_quant_cpu's edge rows: neighbouring columns of every 8-column group
carry exponents 12 or more apart, so a scale taken from the wrong column cannot pass. Every comparison is torch.equal
(on the raw bytes where a NaN would make equal tensors compare unequal); there is no tolerance anywhere."""
import ctypes

import pytest
import torch

from tests.stream_cases import random_codes
from tests.test_gpu_fp8 import weights
from tests.test_gpu_kernels import rnd, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -7.0


def _lib():
    from zonos_vibes_amd import _lib as L
    return L


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _args(W, n_pad, X, M, K, out, n_valid, exp=None, pro=0, aux=None, ld_aux=0, res_out=None, ln_w=None, ln_b=None,
          groups=0):
    L = _lib()
    a = L.GemvArgs()
    a.W, a.X, a.M, a.N, a.K, a.ldx = W.data_ptr(), X.data_ptr(), M, n_pad, K, K
    a.out, a.ldo, a.n_valid, a.eps, a.groups = out.data_ptr(), n_pad, n_valid, 1e-5, groups
    a.pro, a.aux, a.ld_aux, a.res_out = pro, L.ptr(aux), ld_aux, L.ptr(res_out)
    a.ln_w, a.ln_b = L.ptr(ln_w), L.ptr(ln_b)
    if exp is not None:
        a.w_fmt, a.w_exp = L.WFMT_FP8, exp.data_ptr()
    return a


def _both(wt, X, M, K, n_valid, **kw):
    """(fp8 launch's output, bf16 twin's output) of one STORE launch, over canary-filled [M][n_pad] outputs; res_out
    (if given as True) is a canary-filled [M][K] pair returned with them."""
    L = _lib()
    packed, ep, n_pad, (twin, _), _ = wt
    res = kw.pop("res_out", False)
    outs, ress = [], []
    for W, exp in ((packed, ep), (twin, None)):
        out = torch.full((M, n_pad), CANARY, dtype=torch.bfloat16, device=DEV)
        ro = torch.full((M, K), CANARY, dtype=torch.bfloat16, device=DEV) if res else None
        a = _args(W, n_pad, X, M, K, out, n_valid, exp=exp, res_out=ro, **kw)
        L.check(L.lib().zmi_gemv_launch(ctypes.byref(a), L.EPI_STORE, stream_ptr()), "gemv")
        outs.append(out)
        ress.append(ro)
    torch.cuda.synchronize()
    return outs, ress


def _ln(k):
    return (rnd(k, scale=0.1, seed=10) + 1).contiguous(), rnd(k, scale=0.02, seed=11)


# (K, N packed, n_valid): 130 rows padded to 136 columns = 17 groups, so G = 2 clamps its last group
@pytest.mark.parametrize("K,N,n_valid", [(512, 64, 64), (512, 136, 130), (2048, 64, 64), (2048, 136, 130)])
def test_fp8_addln_store_equals_bf16_twin(K, N, n_valid):
    """in_proj's decode launch: add + LayerNorm prologue, bf16 store; one tile (1, 2, 16 rows) and the tile loop (17, 33);
    with the new residual written (res_out) and without (block 0)."""
    L = _lib()
    wt = weights(n_valid, K, n_pad=N)
    lw, lb = _ln(K)
    form = L.GemvForm()
    for M in (1, 2, 16, 17, 33):
        X, aux = rnd(M, K, scale=1.5, seed=20 + M), rnd(M, K, scale=2.0, seed=50 + M)
        for groups in ((1, 2) if K == 2048 else (1,)):
            for res in (True, False):
                (got, ref), (rg, rr) = _both(wt, X, M, K, n_valid, pro=L.PRO_ADDLN, aux=aux, ld_aux=K, ln_w=lw, ln_b=lb,
                                             groups=groups, res_out=res)
                assert _same(got, ref), (M, groups, res, (got != ref).nonzero()[:4].tolist())
                assert (got[:, n_valid:] == CANARY).all() and (got[:, :n_valid] != CANARY).any()
                if res:
                    assert _same(rg, rr) and (rg != CANARY).all()
            a = _args(wt[0], N, X, M, K, got, n_valid, exp=wt[1], pro=L.PRO_ADDLN, aux=aux, ld_aux=K, ln_w=lw, ln_b=lb,
                      groups=groups)
            assert L.lib().zmi_gemv_form(ctypes.byref(a), L.EPI_STORE, ctypes.byref(form)) == 0
            assert (form.G, form.pro, form.ntw) == (groups, L.PRO_ADDLN, int(M <= 16))


@pytest.mark.parametrize("K", [1024, 4096])
def test_fp8_out_proj_equals_bf16_twin(K):
    """out_proj's launches: the gated RMSNorm prologues (GRMS from y and the f32 gate, GRMS_G from g = y * gate) up to 4
    rows, and the plain store behind zmi_gated_rmsnorm from 5 rows on (one tile and the tile loop)."""
    L = _lib()
    nw = (rnd(K, scale=0.1, seed=12) + 1).contiguous()
    for N, n_valid in ((64, 64), (136, 130)):
        wt = weights(n_valid, K, n_pad=N)
        for M in (1, 2, 4):
            y = rnd(M, K, scale=2.0, seed=60 + M)
            gate = rnd(M, K, scale=1.5, seed=70 + M).float().contiguous()
            for pro in (L.PRO_GRMS, L.PRO_GRMS_G):
                (got, ref), _ = _both(wt, y, M, K, n_valid, pro=pro, aux=gate, ld_aux=K, ln_w=nw)
                assert _same(got, ref), (N, M, pro)
                assert (got[:, n_valid:] == CANARY).all() and (got[:, :n_valid] != CANARY).any()
        for M in (1, 5, 16, 17, 33):
            (got, ref), _ = _both(wt, rnd(M, K, seed=80 + M), M, K, n_valid)
            assert _same(got, ref), (N, M)
            assert (got[:, n_valid:] == CANARY).all() and (got[:, :n_valid] != CANARY).any()


def test_fp8_store_launches_that_are_not_built_are_refused():
    """Refused before any launch, nothing written: a plain fp8 STORE at K = 512 (no plain in_proj launch exists), the
    QKV epilogue over fp8 weights, and an fp8 ADDLN launch without exponents."""
    L = _lib()
    lib = L.lib()
    K, M = 512, 2
    wt = weights(64, K)
    X, aux = rnd(M, K, seed=1), rnd(M, K, seed=2)
    lw, lb = _ln(K)
    out = torch.full((M, 64 + 32), CANARY, dtype=torch.bfloat16, device=DEV)  # 32 canary columns behind the rows
    a = _args(wt[0], 64, X, M, K, out, 64, exp=wt[1])
    a.ldo = 96
    assert lib.zmi_gemv_launch(ctypes.byref(a), L.EPI_STORE, stream_ptr()) != 0
    assert b"fp8" in lib.zmi_last_error()
    assert lib.zmi_gemv_form(ctypes.byref(a), L.EPI_STORE, ctypes.byref(L.GemvForm())) != 0
    # fp8 ADDLN, w_exp NULL
    a = _args(wt[0], 64, X, M, K, out, 64, exp=wt[1], pro=L.PRO_ADDLN, aux=aux, ld_aux=K, ln_w=lw, ln_b=lb)
    a.ldo, a.w_exp = 96, None
    assert lib.zmi_gemv_launch(ctypes.byref(a), L.EPI_STORE, stream_ptr()) != 0
    assert b"w_exp" in lib.zmi_last_error()
    # QKV over fp8 weights: 4 / 1 heads of 128, every QKV operand present
    hq, hkv, hd, smax = 4, 1, 128, 8
    n = (hq + 2 * hkv) * hd
    wq = weights(n, K)
    q = torch.full((M, hq * hd), CANARY, dtype=torch.bfloat16, device=DEV)
    kc = torch.full((M, hkv, smax, hd), CANARY, dtype=torch.bfloat16, device=DEV)
    vc = torch.full((M, hkv, hd, smax), CANARY, dtype=torch.bfloat16, device=DEV)
    rope = torch.ones(smax, hd // 2, 2, dtype=torch.float32, device=DEV)
    row = torch.arange(M, dtype=torch.int32, device=DEV)
    a = _args(wq[0], n, X, M, K, q, n, exp=wq[1])
    a.ldo = hq * hd
    a.row_kv, a.row_pos, a.k_cache, a.v_cache = row.data_ptr(), row.data_ptr(), kc.data_ptr(), vc.data_ptr()
    a.smax, a.hq, a.hkv, a.hd, a.rope = smax, hq, hkv, hd, rope.data_ptr()
    assert lib.zmi_gemv_launch(ctypes.byref(a), L.EPI_QKV, stream_ptr()) != 0
    assert b"fp8" in lib.zmi_last_error()
    torch.cuda.synchronize()
    for t in (out, q, kc, vc):
        assert (t == CANARY).all()


# ------------------------------------------------------------------ zmi_mamba_block
def _mamba_params(md, seed):
    g = torch.Generator().manual_seed(seed)
    nh, cd = md["nheads"], md["conv_dim"]
    cw = (torch.rand(cd, md["d_conv"], generator=g) - 0.5).to(torch.bfloat16)
    cb = (torch.randn(cd, generator=g) * 0.1).to(torch.bfloat16)
    dtb = (torch.rand(nh, generator=g) * 2 - 3).to(torch.bfloat16).float()
    A = -torch.exp((torch.rand(nh, generator=g) * 2.77).to(torch.bfloat16).float())
    D = (1 + 0.1 * torch.randn(nh, generator=g)).to(torch.bfloat16).float()
    return [t.to(DEV) for t in (cw, cb, dtb, A, D)]


@pytest.mark.parametrize("M", [1, 2, 16])
def test_fp8_mamba_block_equals_bf16_block(M):
    """The fused in_proj + Mamba2 step launch at the published width (d 2048, 64 heads, d_in_proj 8512: the XCD-local
    column-block map), fp8 in_proj against the bf16 block on the dequantised twin; two consecutive positions per row (the
    granule tag changes), from M = 2 on the last row inactive. zxbcdt, y, g = y * gate, the new residual, the conv ring
    and the SSM state, and the block's error word stays 0."""
    from zonos_vibes_amd.config import zonos_v01_hybrid
    L = _lib()
    lib = L.lib()
    md = zonos_v01_hybrid().backbone.mamba2_dims()
    d, n, ds = 2048, md["d_in_proj"], md["d_ssm"]
    assert (n, ds, md["nheads"]) == (8512, 4096, 64)
    wt = weights(n, d)
    cw, cb, dtb, A, D = _mamba_params(md, 11)
    lw, lb = (rnd(d, scale=0.005, seed=10) + 0.05).contiguous(), rnd(d, scale=0.02, seed=11)  # sums of the 2^3 rows stay ~1
    pos0 = [3 + r for r in range(M)]
    if M > 1:
        pos0[-1] = -1

    def state():
        return dict(zx=torch.full((M, n), CANARY, dtype=torch.bfloat16, device=DEV),
                    y=torch.zeros(M, ds, dtype=torch.bfloat16, device=DEV),
                    gz=torch.zeros(M, ds, dtype=torch.float32, device=DEV),
                    res=torch.full((M, d), CANARY, dtype=torch.bfloat16, device=DEV),
                    ring=rnd(M, 4, md["conv_dim"], seed=13), ssm=rnd(M, md["nheads"], 64, 128, scale=0.5, seed=14),
                    gran=torch.zeros(M, n // 2, dtype=torch.int64, device=DEV),
                    err=torch.zeros(4, dtype=torch.int32, device=DEV))
    assert lib.zmi_mamba_block_gran_words(M, n) == M * (n // 2)
    st8, stb = state(), state()
    for step in range(2):
        X, aux = rnd(M, d, scale=1.5, seed=30 + step), rnd(M, d, scale=2.0, seed=40 + step)
        rp = torch.tensor([p + step if p >= 0 else -1 for p in pos0], dtype=torch.int32, device=DEV)
        for st, (W, exp) in ((st8, (wt[0], wt[1])), (stb, (wt[3][0], None))):
            ia = _args(W, n, X, M, d, st["zx"], n, exp=exp, pro=L.PRO_ADDLN, aux=aux, ld_aux=d, res_out=st["res"],
                       ln_w=lw, ln_b=lb)
            ia.row_pos = rp.data_ptr()
            sa = L.Mamba2Args()
            sa.zxbcdt, sa.ld_zx, sa.M = st["zx"].data_ptr(), n, M
            sa.d_ssm, sa.nheads, sa.headdim, sa.d_state, sa.d_conv, sa.ngroups = ds, md["nheads"], 64, 128, 4, 1
            sa.conv_w, sa.conv_b, sa.dt_bias, sa.A, sa.D = (t.data_ptr() for t in (cw, cb, dtb, A, D))
            sa.conv_ring, sa.ssm, sa.y, sa.ldy = st["ring"].data_ptr(), st["ssm"].data_ptr(), st["y"].data_ptr(), ds
            sa.row_pos, sa.row_kv, sa.gz, sa.gz_g = rp.data_ptr(), None, st["gz"].data_ptr(), 1
            L.check(lib.zmi_mamba_block(ctypes.byref(ia), ctypes.byref(sa), st["gran"].data_ptr(),
                                        st["err"].data_ptr(), stream_ptr()), "mamba_block")
        torch.cuda.synchronize()
        for key in ("zx", "y", "gz", "res", "ring", "ssm"):
            assert _same(st8[key], stb[key]), (step, key)
        assert not st8["err"].any() and not stb["err"].any()
        act = [r for r, p in enumerate(pos0) if p >= 0]
        assert (st8["zx"][act] != CANARY).any() and st8["y"][act].any() and st8["gz"][act].any()
    assert not _same(st8["ssm"], rnd(M, md["nheads"], 64, 128, scale=0.5, seed=14))      # the state did move
    if M > 1:  # the inactive row: no step ran on it
        assert not st8["y"][-1].any() and _same(st8["ssm"][-1], rnd(M, md["nheads"], 64, 128, scale=0.5, seed=14)[-1])
    # fp8 without exponents is refused, nothing launched
    ia.w_fmt, ia.w_exp = L.WFMT_FP8, None
    assert lib.zmi_mamba_block(ctypes.byref(ia), ctypes.byref(sa), stb["gran"].data_ptr(), stb["err"].data_ptr(),
                               stream_ptr()) != 0


# ------------------------------------------------------------------ the prefill's expansion kernel
@pytest.mark.parametrize("n_src,n_pad,k", [(64, 64, 512), (130, 136, 2048), (64, 64, 4096), (2320, 2320, 512)])
def test_unpack_fp8_gives_the_packed_dequantised_weight(n_src, n_pad, k):
    """zmi_unpack_fp8(M8F8 bytes, exponents) == zmi_pack_weight(dequantize_fp8(q, e)), byte for byte, and the 64 bytes
    behind the output stay as they were."""
    L = _lib()
    packed, ep, _, (twin, _), _ = weights(n_src, k, n_pad=n_pad)
    out = torch.full((n_pad * k + 32,), CANARY, dtype=torch.bfloat16, device=DEV)
    L.check(L.lib().zmi_unpack_fp8(packed.data_ptr(), ep.data_ptr(), n_pad, k, out.data_ptr(), stream_ptr()), "unpack")
    torch.cuda.synchronize()
    assert _same(out[: n_pad * k], twin)
    assert (out[n_pad * k:] == CANARY).all()
    assert twin.float().abs().max() > 0
    assert L.lib().zmi_unpack_fp8(packed.data_ptr(), ep.data_ptr(), n_pad, k + 64, out.data_ptr(), stream_ptr()) != 0
    assert L.lib().zmi_unpack_fp8(packed.data_ptr(), None, n_pad, k, out.data_ptr(), stream_ptr()) != 0


# ------------------------------------------------------------------ engine level
def _twins(cfg, **kw):
    """(fp8-mixer model, bf16 model on the same synthetic weights with the quantised tensors replaced by their
    dequantised values)."""
    from zonos_vibes_amd.model import Zonos
    m8 = Zonos.synthetic(cfg, DEV, zero_eos=True, mixer_weights="fp8", **kw)
    mb = Zonos.synthetic(cfg, DEV, zero_eos=True, **kw)
    assert mb.engine.dequantized_state_dict_overrides() == {}
    over = m8.engine.dequantized_state_dict_overrides()
    bb = cfg.backbone
    mamba = [i for i in range(bb.n_layer) if i not in bb.attn_layer_idx]
    assert sorted(over) == sorted(f"backbone.layers.{i}.mixer.{n}.weight" for i in mamba for n in ("in_proj", "out_proj"))
    sd = mb.engine.synthetic_state_dict(0, zero_eos=True)
    assert all(over[k].shape == sd[k].shape and over[k].dtype == torch.bfloat16 and not torch.equal(over[k], sd[k])
               for k in over)
    sd.update(over)
    mb.engine.load_state_dict(sd)
    return m8, mb


def _cond(seed, lc, d):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(2, lc, d, generator=g) * 0.5).to(torch.bfloat16).to(DEV)


def _assert_same_state(m8, mb):
    assert _same(m8.engine.logits, mb.engine.logits)
    c8, cb = m8.engine.inference_cache(), mb.engine.inference_cache()
    assert sorted(c8) == sorted(cb)
    for i in c8:
        for a, b in zip(c8[i], cb[i]):
            assert _same(a, b), i


@pytest.fixture(scope="module")
def tiny_twins():
    from zonos_vibes_amd.config import tiny_hybrid
    return _twins(tiny_hybrid(), max_seqlen=160, max_prefill=64)


@pytest.mark.parametrize("sp,cfg_scale", [(dict(temperature=0.0), 2.0), (dict(min_p=0.1), 2.0), (dict(min_p=0.1), 1)],
                         ids=["greedy", "min_p", "cfg_scale_1"])
def test_fp8_hybrid_generate_equals_bf16_twin(tiny_twins, sp, cfg_scale):
    m8, mb = tiny_twins
    assert "mixer_weights=fp8" in repr(m8) and "mixer_weights=bf16" in repr(mb) and "weights=bf16" in repr(m8)
    cond = _cond(3, 11, 512)
    out = []
    for m in (m8, mb):
        torch.manual_seed(1234)
        out.append(m.generate(cond, max_new_tokens=24, cfg_scale=cfg_scale, sampling_params=sp, progress_bar=False))
        m.engine.check_errors()
    assert out[0].shape[-1] == 24 and torch.equal(out[0], out[1])
    _assert_same_state(m8, mb)


def test_fp8_hybrid_chunked_prefill_equals_bf16_twin(tiny_twins):
    """A 71-row prompt in chunks of 32: the second and third pass continue the Mamba2 state (zmi_mamba2_scan_cont) on
    the expanded projections."""
    m8, mb = tiny_twins
    cond, prefix = _cond(5, 20, 512), random_codes(50, seed=9).to(DEV)
    out = []
    for m in (m8, mb):
        torch.manual_seed(7)
        out.append(m.generate(cond, prefix, max_new_tokens=12, sampling_params=dict(min_p=0.1), progress_bar=False,
                              prefill_chunk=32))
        assert m.engine.max_prefill == 64           # the long prompt ran in chunks: the engine was not rebuilt
    assert out[0].shape[-1] == 50 + 12 and torch.equal(out[0], out[1])
    assert _same(m8.engine.logits_pre, mb.engine.logits_pre)
    _assert_same_state(m8, mb)


def test_fp8_hybrid_generate_batch_equals_bf16_twin(tiny_twins):
    """3 utterances over 2 slots, one with a 12-frame audio prefix; the engines are rebuilt for 2 slots
    (_ensure_capacity) and keep their format and their scratch."""
    m8, mb = tiny_twins
    conds = [_cond(40 + i, 9 + i, 512) for i in range(3)]
    prefixes = [None, random_codes(12, seed=5).to(DEV), None]
    out = [m.generate_batch(conds, prefixes, max_new_tokens=[20, 14, 9], sampling_params=dict(min_p=0.1),
                            seeds=[1, 2, 3], max_slots=2) for m in (m8, mb)]
    assert m8.engine.S == 2 and m8.engine.mixer_weights == "fp8" and mb.engine.mixer_weights == "bf16"
    assert m8.engine.mix_scratch is not None and mb.engine.mix_scratch is None
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert [o.shape[-1] for o in out[0]] == [20, 12 + 14, 9]
    _assert_same_state(m8, mb)


@pytest.fixture(scope="module")
def wide_twins():
    from zonos_vibes_amd.config import hybrid_config
    return _twins(hybrid_config(2048, 3, [1], 16, 4), max_slots=9, max_seqlen=64, max_prefill=32)


def test_fp8_hybrid_full_width_equals_bf16_twin(wide_twins):
    """d 2048, d_ssm 4096, d_in_proj 8512: 2 rows (zmi_mamba_block and GRMS_G at K 4096), 6 rows (the block,
    zmi_gated_rmsnorm and the plain K 4096 launch), 18 rows (the ADDLN tile loop in front of zmi_mamba2_step)."""
    m8, mb = wide_twins
    sp = dict(temperature=0.0)
    cond = _cond(9, 12, 2048)
    one = [m.generate(cond, max_new_tokens=12, sampling_params=sp, progress_bar=False) for m in (m8, mb)]
    assert one[0].shape[-1] == 12 and torch.equal(one[0], one[1])
    _assert_same_state(m8, mb)
    for n in (3, 9):
        conds = [_cond(60 + i, 5 + i, 2048) for i in range(n)]
        out = [m.generate_batch(conds, max_new_tokens=[10] * n, sampling_params=sp, seeds=list(range(n)), max_slots=n)
               for m in (m8, mb)]
        assert all(torch.equal(a, b) for a, b in zip(*out)) and len(out[0]) == n
        _assert_same_state(m8, mb)
        for m in (m8, mb):
            m.engine.check_errors()


def test_fp8_mixer_weights_take_half_the_bytes(wide_twins):
    m8, mb = wide_twins
    md = m8.engine.md
    for l8, lb in zip(m8.engine.w["layers"], mb.engine.w["layers"]):
        assert l8["kind"] == lb["kind"]
        if l8["kind"] == "mamba":
            for key, n, k in (("in_proj", md["d_in_proj"], 2048), ("out", 2048, md["d_ssm"])):
                assert l8[key].dtype == torch.uint8 and l8[key].numel() == n * k + n
                assert lb[key].dtype == torch.bfloat16 and lb[key].numel() == n * k
            same = ("conv_w", "conv_b", "norm_w", "ln1_w", "ln1_b", "dt_bias", "A", "D")
        else:
            same = ("qkv", "out", "ln1_w", "ln1_b")
        for key in same:
            assert l8[key].dtype == lb[key].dtype and l8[key].shape == lb[key].shape, key
    for key in ("heads", "emb", "nf_w"):
        assert m8.engine.w[key].dtype == torch.bfloat16 and m8.engine.w[key].shape == mb.engine.w[key].shape
    sc = m8.engine.mix_scratch
    assert [t.numel() for t in sc] == [md["d_in_proj"] * 2048, 2048 * md["d_ssm"]] and sc[0].dtype == torch.bfloat16
