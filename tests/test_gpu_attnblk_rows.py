"""The fused decode block at odd row counts. The paired layout steps 2, 4, 6, ... rows; the single layout (one row
per utterance, guidance-free generation) steps every count from 1 up, so zmi_attn_block and zmi_attn_block_oproj
run at 1, 3, 5 and 7 rows here: row counts whose (row, kv head) units do not fill the groups of 8 the grid is dealt
in (4 kv heads: 4, 12, 20, 28 units), at chunk and 512-key block edges, with an inactive row among >= 3 rows.
Everything must be bit-identical to the separate launches (QKV GEMV, attention, out_proj GEMV), over three launches
(the second and third find their own granules: equal values, equal tags). The setup mirrors test_gpu_attnblk.py."""
import ctypes

import pytest
import torch

from tests.test_gpu_kernels import DEV, _lib, pack, rnd, stream_ptr

pytestmark = pytest.mark.gpu

D, H, HKV, HD = 2048, 16, 4, 128
QKV_N = (H + 2 * HKV) * HD
SELF, SPLIT = 256, 512  # zmi_attn_block slices flags: self-scoring / chunk-split forms
SMAX = 1280
# chunk (128) and block (512) edges, position 0 and the 8-chunk forms' last position; -1: an inactive row
POSITIONS = {1: [(0,), (127,), (128,), (511,), (512,), (1023,)],
             3: [(0, -1, 1023), (127, 128, -1)],
             5: [(511, 512, -1, 0, 1023)],
             7: [(0, 127, 128, -1, 511, 512, 1023)]}
CASES = [pytest.param(p, id=f"{n}rows-" + "_".join(str(v) for v in p)) for n, ps in POSITIONS.items() for p in ps]


def _setup(positions, smax, seed):
    from zonos_vibes_amd.engine import rope_table
    R = len(positions)
    W = rnd(QKV_N, D, scale=0.03, seed=seed)
    X = rnd(R, D, scale=2.0, seed=seed + 1)
    lw, lb = rnd(D, scale=0.1, seed=seed + 2) + 1, rnd(D, scale=0.02, seed=seed + 3)
    kc = rnd(R, HKV, smax, HD, seed=seed + 4)
    vt = rnd(R, HKV, HD, smax, seed=seed + 5)
    return dict(W=pack(W), X=X, ln=(lw.contiguous(), lb.contiguous()), kc=kc, vt=vt, rope=rope_table(HD).to(DEV),
                row_kv=torch.arange(R, dtype=torch.int32, device=DEV),
                row_pos=torch.tensor(positions, dtype=torch.int32, device=DEV), smax=smax, R=R)


def _args(st, q, kc, vt):
    L = _lib()
    (Wp, n_pad) = st["W"]
    a = L.GemvArgs()
    a.W, a.X, a.M, a.N, a.K, a.ldx = Wp.data_ptr(), st["X"].data_ptr(), st["R"], n_pad, D, D
    a.ln_w, a.ln_b, a.eps = st["ln"][0].data_ptr(), st["ln"][1].data_ptr(), 1e-5
    a.out, a.ldo, a.n_valid = q.data_ptr(), H * HD, QKV_N
    a.row_kv, a.row_pos, a.k_cache, a.v_cache = st["row_kv"].data_ptr(), st["row_pos"].data_ptr(), kc.data_ptr(), \
        vt.data_ptr()
    a.smax, a.hq, a.hkv, a.hd, a.rope = st["smax"], H, HKV, HD, st["rope"].data_ptr()
    return a


def _separate(st):
    L = _lib()
    R, smax = st["R"], st["smax"]
    q = torch.zeros(R, H * HD, dtype=torch.bfloat16, device=DEV)
    kc, vt = st["kc"].clone(), st["vt"].clone()
    a = _args(st, q, kc, vt)
    L.check(L.lib().zmi_gemv_launch(ctypes.byref(a), L.EPI_QKV, stream_ptr()), "gemv")
    out = torch.zeros(R, H * HD, dtype=torch.bfloat16, device=DEV)
    work = torch.zeros(L.lib().zmi_attention_work_bytes(R, H, HKV, HD, smax - 1), dtype=torch.uint8, device=DEV)
    nf = L.lib().zmi_attention_partial_floats(R, H, HKV, HD, smax - 1)
    po = torch.zeros(nf, dtype=torch.float32, device=DEV)
    plm = torch.zeros(nf // HD * 2, dtype=torch.float32, device=DEV)
    L.check(L.lib().zmi_attention_variant(q.data_ptr(), H * HD, kc.data_ptr(), vt.data_ptr(), None,
                                          st["row_pos"].data_ptr(), R, H, HKV, HD, smax, smax - 1, out.data_ptr(),
                                          H * HD, po.data_ptr(), plm.data_ptr(), work.data_ptr(), 1, stream_ptr()))
    torch.cuda.synchronize()
    return q, kc, vt, out


def _stale_granules(R):
    """Hand-off granules holding stale tags of "earlier steps" (no tag is a row's position + 1 <= 1024), as in a
    running decode."""
    L = _lib()
    gran = torch.zeros(L.lib().zmi_attn_block_gran_words(R, HKV), dtype=torch.int64, device=DEV)
    gran.copy_(torch.randint(0, 1 << 30, gran.shape, device=DEV) |
               (torch.randint(1 << 20, 1 << 30, gran.shape, device=DEV) << 32))
    return gran


_REF: dict = {}


def _case(positions):
    """The setup and the separate launches' result of a case, computed once and shared by every form."""
    if positions not in _REF:
        st = _setup(positions, SMAX, seed=170 + len(positions))
        _REF[positions] = (st, _separate(st))
    return _REF[positions]


@pytest.mark.parametrize("positions", CASES)
@pytest.mark.parametrize("slices", [4, 8, 4 | SELF, 8 | SELF, 8 | SPLIT])
def test_attn_block_odd_rows_bit_identical_to_separate_launches(positions, slices):
    L = _lib()
    assert max(positions) <= L.lib().zmi_attn_block_max_pos(slices)
    st, ref = _case(positions)
    R = st["R"]
    q = torch.zeros(R, H * HD, dtype=torch.bfloat16, device=DEV)
    kc, vt = st["kc"].clone(), st["vt"].clone()
    a = _args(st, q, kc, vt)
    gran = _stale_granules(R)
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    out = torch.zeros(R, H * HD, dtype=torch.bfloat16, device=DEV)
    live = [i for i, p in enumerate(positions) if p >= 0]
    for rep in range(3):
        L.check(L.lib().zmi_attn_block(ctypes.byref(a), gran.data_ptr(), err.data_ptr(), out.data_ptr(), H * HD,
                                       slices, stream_ptr()), "attn_block")
        torch.cuda.synchronize()
        assert int(err[0].item()) == 0, "a wait for a hand-off gave up"
        for name, r, g in zip(("q", "k_cache", "v_cache"), ref[:3], (q, kc, vt)):
            assert torch.equal(r, g), (name, rep)
        assert torch.equal(ref[3][live], out[live]), ("attention output", rep)


@pytest.mark.parametrize("positions", CASES)
@pytest.mark.parametrize("chunks", [8, 24])
def test_attn_block_oproj_odd_rows_bit_identical_to_separate_launches(positions, chunks):
    L = _lib()
    slices = chunks | SPLIT
    assert max(positions) <= L.lib().zmi_attn_block_max_pos(slices)
    st, (ref_q, ref_k, ref_v, ref_out) = _case(positions)
    R = st["R"]
    Wo = pack(rnd(D, H * HD, scale=0.03, seed=181))[0]
    x0 = rnd(R, D, scale=2.0, seed=182)

    def oargs(attn, x):
        o = L.GemvArgs()
        o.W, o.X, o.M, o.N, o.K, o.ldx = Wo.data_ptr(), attn.data_ptr(), R, D, H * HD, H * HD
        o.out, o.ldo, o.n_valid = x.data_ptr(), D, D
        return o

    x_ref = x0.clone()
    L.check(L.lib().zmi_gemv_launch(ctypes.byref(oargs(ref_out, x_ref)), L.EPI_RESIDUAL, stream_ptr()), "out_proj")
    q = torch.zeros(R, H * HD, dtype=torch.bfloat16, device=DEV)
    kc, vt = st["kc"].clone(), st["vt"].clone()
    a = _args(st, q, kc, vt)
    gran = _stale_granules(R)
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    out = torch.zeros(R, H * HD, dtype=torch.bfloat16, device=DEV)
    pf = L.Prefetch()
    live = [i for i, p in enumerate(positions) if p >= 0]
    dead = [i for i, p in enumerate(positions) if p < 0]
    for rep in range(3):
        x = x0.clone()
        L.check(L.lib().zmi_attn_block_oproj(ctypes.byref(a), ctypes.byref(oargs(out, x)), gran.data_ptr(),
                                             err.data_ptr(), out.data_ptr(), H * HD, slices, ctypes.byref(pf),
                                             stream_ptr()), "attn_block_oproj")
        torch.cuda.synchronize()
        assert int(err[0].item()) == 0, "a wait for a hand-off gave up"
        for name, r, g in (("q", ref_q, q), ("k_cache", ref_k, kc), ("v_cache", ref_v, vt)):
            assert torch.equal(r, g), (name, rep)
        assert torch.equal(ref_out[live], out[live]), ("attention output", rep)
        assert torch.equal(x_ref[live], x[live]), ("out_proj residual rows", rep)
        assert torch.equal(x0[dead], x[dead]), ("an inactive row's residual is not stored", rep)
