"""The causal prefill attention kernel (zmi_attention_prefill: 16 / G consecutive positions share each K / V tile)
against the chunked kernel it restates (zmi_attention_variant(variant=1)): identical bits for every row, in every
launch shape, and through the engines (MI355X only)."""
import numpy as np
import pytest
import torch

from tests.stream_cases import random_codes
from tests.test_gpu_kernels import _attention, _check_attention, rnd, stream_ptr
from zonos_vibes_amd.prefill_table import prefill_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
HD = 128
SENTINEL = -77.0  # exact in bf16; no attention output of these inputs equals it in every element of a row
HEADS = [(16, 4), (4, 1), (8, 4), (4, 4)]


def _lib():
    from zonos_vibes_amd import _lib as L
    return L


def _qt(hq, hkv):
    return _lib().lib().zmi_attention_prefill_queries(hq, hkv)


def _layout(lens, pos0s, seed=0):
    """ZmiAttnSeq rows for sequences of `lens` at `pos0s`: KV rows a permutation of the sequences, q rows handed out
    in another order with one unowned gap row after each sequence. Returns (seqs, total q rows)."""
    n = len(lens)
    rng = np.random.default_rng(seed)
    kv = rng.permutation(n)
    q_row0, row = [0] * n, 0
    for s in rng.permutation(n):
        q_row0[s] = row
        row += lens[s] + 1
    return [(q_row0[s], lens[s], int(kv[s]), pos0s[s]) for s in range(n)], row + 1


def _prefill(q, kc, vc, seqs, hq, hkv, tables=None, n_tiles=None, smax=None, hd=HD, ldq=None, ldo=None):
    """zmi_attention_prefill over `seqs`; out starts as SENTINEL in every element. Returns (status, out)."""
    L = _lib()
    sa, tiles = tables if tables is not None else prefill_table(seqs, _qt(hq, hkv))
    host = np.concatenate([sa.ravel(), tiles.ravel(), np.zeros(2, np.int32)]).astype(np.int32)  # (never empty)
    dev = torch.from_numpy(host).to(DEV)
    vt = vc.transpose(-1, -2).contiguous()
    out = torch.full((q.shape[0], hq * HD), SENTINEL, dtype=torch.bfloat16, device=DEV)
    rc = L.lib().zmi_attention_prefill(
        q.data_ptr(), hq * HD if ldq is None else ldq, kc.data_ptr(), vt.data_ptr(), dev.data_ptr(), len(sa),
        len(tiles) if n_tiles is None else n_tiles, dev.data_ptr() + sa.nbytes, sa.ctypes.data, hq, hkv, hd,
        kc.shape[-2] if smax is None else smax, out.data_ptr(), hq * HD if ldo is None else ldo, stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def _expand(seqs):
    """(q rows, kv rows, positions) of every (sequence, position), in sequence order."""
    rows, kvs, pos = [], [], []
    for q0, n, kv, p0 in seqs:
        rows += range(q0, q0 + n)
        kvs += [kv] * n
        pos += range(p0, p0 + n)
    return rows, kvs, pos


def _reference(q, kc, vc, seqs, hq, hkv):
    """The chunked kernel, one query per row, on the expanded (kv_row, pos) list -> (q rows, [rows][hq * 128])."""
    rows, kvs, pos = _expand(seqs)
    idx = torch.tensor(rows, device=DEV)
    return idx, _attention(q[idx].contiguous(), kc, vc, pos, kvs, hq=hq, hkv=hkv, variant=1)


def _assert_same_bits(got, ref, rows, what):
    if torch.equal(got, ref):
        return
    bad = (got.view(torch.int16) != ref.view(torch.int16)).nonzero()
    i, e = (int(v) for v in bad[0])
    raise AssertionError(f"{what}: {len(bad)} elements differ, first at q row {rows[i]} head {e // HD} dim {e % HD}: "
                         f"{got[i, e].item()} against {ref[i, e].item()}")


def _caches(n_kv, hkv, smax, seed):
    return rnd(n_kv, hkv, smax, HD, seed=seed), rnd(n_kv, hkv, smax, HD, seed=seed + 1)


def _check_launch(seqs, n_rows, hq, hkv, smax, seed, picked=()):
    kc, vc = _caches(len(seqs), hkv, smax, seed)
    q = rnd(n_rows, hq * HD, scale=3.0, seed=seed + 2)
    rc, out = _prefill(q, kc, vc, seqs, hq, hkv)
    assert rc == 0, _lib().lib().zmi_last_error()
    idx, ref = _reference(q, kc, vc, seqs, hq, hkv)
    rows, kvs, pos = _expand(seqs)
    _assert_same_bits(out[idx], ref, rows, f"{hq}/{hkv} heads")
    owned = torch.zeros(n_rows, dtype=torch.bool, device=DEV)
    owned[idx] = True
    assert (out[~owned] == SENTINEL).all()  # the gap rows and the row after the last one
    pick = [rows.index(seqs[s][0] + i) for s, i in picked]  # the float-level meaning, on a few rows
    if pick:
        _check_attention(out[idx][pick], q[idx][pick], kc, vc, [pos[i] for i in pick], [kvs[i] for i in pick], hq=hq,
                         hkv=hkv)


LAUNCHES = {
    "short": [1, 2, 3, 4, 5, 17, 31, 32, 33, 127, 128, 129, 130],
    "block_edge": [511, 512, 513],
    "three_blocks": [1025, 640],  # the mprev chain runs twice
}


@pytest.mark.parametrize("hq,hkv", HEADS)
@pytest.mark.parametrize("name", list(LAUNCHES))
def test_prefill_bit_identical_to_chunked(name, hq, hkv):
    lens = LAUNCHES[name]
    seqs, n_rows = _layout(lens, [0] * len(lens), seed=len(lens))
    last = len(lens) - 1
    _check_launch(seqs, n_rows, hq, hkv, max(lens) + 7 & ~7, 100,
                  picked=[(0, 0), (last, 0), (last, lens[last] // 2), (last, lens[last] - 1)])


@pytest.mark.parametrize("hq,hkv", HEADS)
@pytest.mark.parametrize("name", ["short", "three_blocks"])
def test_prefill_from_a_later_position(name, hq, hkv):
    """pos0 in {2, 509}: tiles start at positions that are no multiple of QT, and the len-8 sequence at 509
    (positions 509 .. 516) has a tile that straddles position 512, whose rows differ in block count."""
    lens = LAUNCHES[name] + [8, 8]
    pos0s = [(2, 509)[i % 2] for i in range(len(lens) - 2)] + [2, 509]
    seqs, n_rows = _layout(lens, pos0s, seed=3 + len(lens))
    smax = max(p + n for p, n in zip(pos0s, lens)) + 7 & ~7
    _check_launch(seqs, n_rows, hq, hkv, smax, 110, picked=[(len(lens) - 1, 2), (len(lens) - 1, 3), (len(lens) - 1, 7)])


@pytest.mark.parametrize("hq,hkv", HEADS)
def test_prefill_ignores_stale_cache_bytes(hq, hkv):
    """NaN bit patterns in both caches past every sequence's last position: both kernels give the same finite rows."""
    lens = [5, 33, 130, 513]
    seqs, n_rows = _layout(lens, [0, 3, 0, 509], seed=9)
    smax = 1032
    kc, vc = _caches(len(seqs), hkv, smax, 120)
    nan = torch.tensor([0x7FC0, -1, 0x7F81, -64], dtype=torch.int16, device=DEV)  # four bf16 NaN bit patterns
    for _, n, kv, p0 in seqs:
        for c in (kc, vc):
            tail = c[kv, :, p0 + n:].view(torch.int16)
            tail.copy_(nan[torch.arange(tail.numel(), device=DEV) % 4].view(tail.shape))
    assert torch.isnan(kc.float()).any() and torch.isnan(vc.float()).any()
    q = rnd(n_rows, hq * HD, scale=3.0, seed=122)
    rc, out = _prefill(q, kc, vc, seqs, hq, hkv)
    assert rc == 0
    idx, ref = _reference(q, kc, vc, seqs, hq, hkv)
    assert torch.isfinite(ref.float()).all()
    _assert_same_bits(out[idx], ref, _expand(seqs)[0], "stale bytes")


@pytest.mark.parametrize("scales", [(1.0, 2.0, 4.0), (4.0, 1.0, 0.5)], ids=["rising", "max_in_block_0"])
def test_prefill_block_maxima(scales):
    """K scaled per 512-key block so that the running maximum rises in block 1 and again in block 2, or sits in
    block 0 (every later exp(M_{j-1} - M_j) is then 1)."""
    hq, hkv, smax = 16, 4, 1104
    seqs, n_rows = _layout([40, 30, 70], [1016, 500, 1030], seed=5)
    kc, vc = _caches(len(seqs), hkv, smax, 130)
    for j, s in enumerate(scales):
        blk = kc[:, :, 512 * j: 512 * (j + 1)]
        blk.copy_((blk.float() * s).to(torch.bfloat16))
    q = rnd(n_rows, hq * HD, scale=3.0, seed=132)
    # the block maxima do what the case is named for (fp32 scores of one late row)
    q0, n, kv, p0 = seqs[2]
    sc = kc[kv, 0, : p0 + n].float() @ q[q0 + n - 1, :HD].float()
    m = [sc[512 * j: 512 * (j + 1)].max().item() for j in range(3)]
    assert (m[0] < m[1] < m[2]) if scales[0] == 1.0 else (m[0] > m[1] and m[0] > m[2])
    rc, out = _prefill(q, kc, vc, seqs, hq, hkv)
    assert rc == 0
    idx, ref = _reference(q, kc, vc, seqs, hq, hkv)
    _assert_same_bits(out[idx], ref, _expand(seqs)[0], "block maxima")


def test_prefill_batch_invariant_and_guarded():
    hq, hkv, smax = 16, 4, 640
    lens, pos0s = [37, 530, 6, 129], [0, 0, 509, 2]
    seqs, n_rows = _layout(lens, pos0s, seed=2)
    kc, vc = _caches(len(seqs), hkv, smax, 140)
    q = rnd(n_rows, hq * HD, scale=3.0, seed=142)
    rc, out = _prefill(q, kc, vc, seqs, hq, hkv)
    assert rc == 0
    owned = torch.zeros(n_rows, dtype=torch.bool, device=DEV)
    for s, (q0, n, kv, p0) in enumerate(seqs):
        rc, alone = _prefill(q, kc, vc, [seqs[s]], hq, hkv)  # the same sequence launched alone
        assert rc == 0
        assert torch.equal(alone[q0: q0 + n], out[q0: q0 + n]), s
        assert (alone[:q0] == SENTINEL).all() and (alone[q0 + n:] == SENTINEL).all()  # nothing past len (37, 6, 129
        owned[q0: q0 + n] = True                                                       # are no multiples of QT)
        assert not (out[q0: q0 + n] == SENTINEL).all(dim=1).any()
    assert (out[~owned] == SENTINEL).all()
    for empty in ([], [(3, 0, 1, 5), (0, 0, 0, 0)]):  # n_seq = 0, or every len = 0: returns 0, writes nothing
        rc, none = _prefill(q, kc, vc, empty, hq, hkv)
        assert rc == 0 and (none == SENTINEL).all()


def test_prefill_refuses_bad_arguments():
    L = _lib()
    hq, hkv, smax = 16, 4, 64
    kc, vc = _caches(1, hkv, smax, 150)
    q = rnd(40, hq * HD, seed=152)
    good = [(0, 20, 0, 0)]

    good_tables = prefill_table(good, _qt(hq, hkv))

    def refused(what, hq=hq, hkv=hkv, tables=good_tables, **kw):
        rc, out = _prefill(q, kc, vc, good, hq, hkv, tables=tables, **kw)
        msg = L.lib().zmi_last_error().decode()
        assert rc != 0 and "attention_prefill" in msg, (what, rc, msg)
        assert (out == SENTINEL).all(), what  # nothing was launched

    assert _prefill(q, kc, vc, good, hq, hkv)[0] == 0
    refused("hd", hd=64)
    refused("smax % 8", smax=60)
    refused("group of 8", hq=8, hkv=1)
    refused("hq not a multiple of hkv", hq=6, hkv=4)
    refused("ldq % 8", ldq=hq * HD + 4)
    refused("ldo % 4", ldo=hq * HD + 2)
    bad_len = (np.array([[0, -1, 0, 0]], np.int32), np.zeros((0, 2), np.int32))
    refused("len < 0", tables=bad_len)
    past = (np.array([[0, 20, 0, 48]], np.int32), good_tables[1])
    refused("pos0 + len > smax", tables=past)
    refused("n_tiles", n_tiles=3)
    assert _qt(8, 1) == -1 and _qt(6, 4) == -1 and (_qt(16, 4), _qt(8, 4), _qt(4, 4)) == (4, 8, 16)


# ------------------------------------------------------------------ engines
def _cond(seed, lc, d):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(2, lc, d, generator=g) * 0.5).to(torch.bfloat16).to(DEV)


def _model(cfg, **kw):
    from zonos_vibes_amd.model import Zonos
    return Zonos.synthetic(cfg, DEV, zero_eos=True, **kw)


def _generate_state(m, mode, cond, prefix, frames=12):
    """Greedy generate() under prefill_attn = mode from wiped buffers -> (codes, x_pre rows, logits_pre, K, V)."""
    e = m.engine
    e.prefill_attn = mode
    lc = cond.shape[1]
    s_len = lc + (0 if prefix is None else prefix.shape[-1]) + 1
    with torch.cuda.stream(e.stream):
        for t in (e.kc, e.vc, e.x_pre, e.logits_pre):
            t.zero_()
        e.attn_pre.fill_(SENTINEL)  # (the other mode's attention output must not stand in for this one's)
    torch.manual_seed(77)
    codes = m.generate(cond, prefix, max_new_tokens=frames, sampling_params=dict(temperature=0.0), progress_bar=False)
    assert m.engine is e and e.prefill_attn == mode  # (no engine rebuild dropped the setting)
    torch.cuda.synchronize()
    return (codes, e.x_pre[: 2 * s_len].clone(), e.logits_pre.clone(), e.kc[:, :2].clone(), e.vc[:, :2].clone())


def _assert_modes_agree(m, cond, prefix=None):
    rows = _generate_state(m, "rows", cond, prefix)
    tiles = _generate_state(m, "tiles", cond, prefix)
    assert rows[0].shape[-1] == 12 + (0 if prefix is None else prefix.shape[-1])
    for name, a, b in zip(("codes", "x_pre", "logits_pre", "K cache", "V cache"), rows, tiles):
        assert torch.equal(a, b), name
    assert rows[3].any() and rows[1].any()


def _engine_cfg(name):
    from zonos_vibes_amd import config as C
    return {"tiny": lambda: C.tiny_transformer(2), "tiny_hybrid": C.tiny_hybrid,
            "production_dims": lambda: C.transformer_config(2048, 2, 16, 4, 8192)}[name]()


@pytest.mark.parametrize("name", ["tiny", "production_dims", "tiny_hybrid"])
def test_engine_prefill_modes_agree(name):
    cfg = _engine_cfg(name)
    m = _model(cfg, max_seqlen=64, max_prefill=32)
    assert m.engine.prefill_attn in ("tiles", "rows")
    _assert_modes_agree(m, _cond(3, 13, cfg.backbone.d_model))
    m.engine.prefill_attn = "blocks"
    with pytest.raises(ValueError, match="prefill_attn"):
        m.generate(_cond(3, 13, cfg.backbone.d_model), max_new_tokens=2, progress_bar=False)


def test_engine_prefill_modes_agree_two_blocks():
    """Lc 11 and a 520-frame audio prefix: S = 532, two softmax blocks."""
    from zonos_vibes_amd.config import tiny_transformer
    m = _model(tiny_transformer(2), max_seqlen=560, max_prefill=532)
    _assert_modes_agree(m, _cond(4, 11, 512), random_codes(520, seed=6).to(DEV))


def test_prefill_many_equals_slots_alone():
    """3 slots of different lengths in one pass, one with an audio prefix: each slot's rows, caches and first
    frame are what the slot gets prefilled alone, under either attention."""
    from zonos_vibes_amd.config import tiny_transformer
    from zonos_vibes_amd.engine import SamplingParams
    e = _model(tiny_transformer(2), max_slots=3, max_seqlen=96, max_prefill=64).engine
    sp = SamplingParams(temperature=0.0)
    items = [(0, _cond(20, 9, 512), None, 8, sp), (1, _cond(21, 14, 512), random_codes(21, seed=8).to(DEV), 8, sp),
             (2, _cond(22, 5, 512), None, 8, sp)]

    def wipe():
        with torch.cuda.stream(e.stream):
            for t in (e.kc, e.vc, e.x_pre):
                t.zero_()
            e.attn_pre.fill_(SENTINEL)

    def state(slot, off, s_len):
        e.stream.synchronize()
        e.check_errors()
        return (e.x_pre[off: off + 2 * s_len].clone(), e.kc[:, 2 * slot: 2 * slot + 2].clone(),
                e.vc[:, 2 * slot: 2 * slot + 2].clone(), e.delayed[slot].clone())

    e.prefill_attn = "tiles"
    wipe()
    lens = e.prefill_many(items)
    assert lens == [10, 36, 6]
    offs = [0, 20, 92]
    batch = [state(it[0], off, n) for it, off, n in zip(items, offs, lens)]
    for s in range(3):
        e.release(s)
    for mode in ("tiles", "rows"):
        e.prefill_attn = mode
        for it, n, want in zip(items, lens, batch):
            wipe()
            assert e.prefill(*it) == n
            for name, a, b in zip(("x_pre", "K", "V", "delayed"), state(it[0], 0, n), want):
                assert torch.equal(a, b), (mode, it[0], name)
            e.release(it[0])
