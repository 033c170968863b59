"""The token glue kernels through the C ABI on the inputs of tests/glue_cases.py (MI355X only): zmi_embed_codes,
zmi_embed_step and the samplers' fused embedding against the bit-exact sequential bf16 sum; zmi_apply_delay_pattern,
zmi_revert_delay_pattern, zmi_delay_init, zmi_delay_revert and zmi_delay_revert_range against the CPU oracle's delay
pattern, all in guard-filled buffers; and every refused argument form, which must leave its output untouched.
"""
import ctypes
import functools

import pytest
import torch

from tests import glue_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
NCB = gc.NCB
XG = -3.0      # guard fill of bf16 buffers
IG = -99       # guard fill of integer buffers


def _lib():
    from zonos_vibes_amd import _lib as L
    return L


def _sp():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=2)
def _table(d, kind):
    return gc.table(d, kind), gc.table(d, kind).to(DEV)


def _slots(L, delayed, active=None, offset=None, pos=None, rps=0):
    """-> (Slots, the device tensors it points to). delayed [S, 9, tcap] int32 on the device."""
    S, _, tcap = delayed.shape
    st = {k: torch.zeros(S, dtype=torch.int32, device=DEV) for k in
          ("active", "pos", "offset", "remaining", "stopping", "step", "total_len")}
    for k, v in (("active", active), ("offset", offset), ("pos", pos)):
        if v is not None:
            st[k].copy_(v)
    params = torch.zeros(S * ctypes.sizeof(L.Sampling), dtype=torch.uint8, device=DEV)
    sl = L.Slots(*(st[k].data_ptr() for k in ("active", "pos", "offset", "remaining", "stopping", "step")),
                 delayed.data_ptr(), params.data_ptr(), st["total_len"].data_ptr(), tcap, S, rps)
    return sl, (st, params, delayed)


def _refused(rc, name):
    assert rc != 0
    msg = _lib().lib().zmi_last_error()
    assert name.encode() in msg, msg


# ----------------------------------------------------------------------------- embeddings
def _embed_codes(L, emb, codes_pad, n, d, ldx, rows=None):
    """zmi_embed_codes into a guard-filled [n + 2, ldx] buffer (one guard row on either side) -> the buffer."""
    x = torch.full(((n if rows is None else rows) + 2, ldx), XG, dtype=torch.bfloat16, device=DEV)
    c = codes_pad.to(DEV)
    L.check(L.lib().zmi_embed_codes(c.data_ptr(), c.shape[1], n, emb.data_ptr(), d, x.data_ptr() + 2 * ldx, ldx,
                                    _sp()), "embed_codes")
    torch.cuda.synchronize()
    return x.cpu()


@pytest.mark.parametrize("kind", ["seeded", "cancel"])
@pytest.mark.parametrize("d", gc.EMBED_WIDTHS)
def test_embed_codes_is_the_sequential_bf16_sum(d, kind):
    """n = 1 and 3, ld_codes = n + 5, ldx = d + 8: every row bit for bit, the 8 sentinels of every row and the guard
    rows kept."""
    L = _lib()
    tab, emb = _table(d, kind)
    for n in (1, 3):
        codes = gc.code_columns(n)
        x = _embed_codes(L, emb, gc.padded_codes(codes), n, d, d + 8)
        ref = gc.embed_ref(tab, codes)
        assert torch.equal(x[1:1 + n, :d], ref), (d, kind, n, (x[1:1 + n, :d] != ref).nonzero()[:4].tolist())
        assert bool((x[1:1 + n, d:] == XG).all()) and bool((x[0] == XG).all()) and bool((x[-1] == XG).all())


@pytest.mark.parametrize("rps", [0, 1], ids=["paired", "single"])
@pytest.mark.parametrize("d,tcap", [(8, 16), (2056, 300), (4096, 64)])
def test_embed_step_embeds_the_frame_at_offset(d, tcap, rps):
    """Both layouts; slots 0, 2, 3 active with offset 0, tcap - 1 and tcap / 2, slot 1 inactive: its rows of x stay
    untouched and its row_pos is -1; the second row of a pair equals the first."""
    L = _lib()
    tab, emb = _table(d, "cancel")
    st = gc.step_state(tcap)
    R = 2 if rps == 0 else 1
    sl, keep = _slots(L, st["delayed"].to(DEV), st["active"], st["offset"], st["pos"], rps)
    S = 4
    x = torch.full((R * S + 1, d), XG, dtype=torch.bfloat16, device=DEV)
    row_kv = torch.full((R * S + 1,), IG, dtype=torch.int32, device=DEV)
    row_pos = torch.full((R * S + 1,), IG, dtype=torch.int32, device=DEV)
    L.check(L.lib().zmi_embed_step(ctypes.byref(sl), emb.data_ptr(), d, x.data_ptr(), row_kv.data_ptr(),
                                   row_pos.data_ptr(), _sp()), "embed_step")
    torch.cuda.synchronize()
    x, row_kv, row_pos = x.cpu(), row_kv.cpu(), row_pos.cpu()
    ref = gc.embed_ref(tab, gc.step_frames(st))
    for s in range(S):
        for h in range(R):
            r = R * s + h
            if st["active"][s]:
                assert torch.equal(x[r], ref[s]), (s, h)
                assert row_pos[r] == st["pos"][s]
            else:
                assert bool((x[r] == XG).all()) and row_pos[r] == -1
            assert row_kv[r] == r
    assert bool((x[-1] == XG).all()) and row_kv[-1] == IG and row_pos[-1] == IG
    assert torch.equal(keep[2].cpu(), st["delayed"])


@pytest.mark.parametrize("seed", [0, 1])
def test_fused_greedy_embedding_equals_embed_codes(seed):
    """One zmi_sample_step_greedy launch with the fused embedding: the rows it wrote equal zmi_embed_codes (and the
    CPU sum) on the frame it left at the new offset, MASK throughout past the slot's total length."""
    from tests.test_gpu_sampler_greedy import D, S, _run, _state
    from zonos_vibes_amd.engine import SamplingParams
    L = _lib()
    args = _state(seed, [SamplingParams(temperature=0.0, cfg_scale=2.0)] * S)
    st0, emb = args[0], args[4]
    out = _run(*args, greedy=True)
    frames = torch.full((NCB, S), gc.MASK, dtype=torch.int32)
    for s in range(S):
        o = int(out["offset"][s])
        if o < int(st0["total_len"][s]):
            frames[:, s] = out["delayed"][s, :, o]
    x = _embed_codes(L, emb.to(DEV), gc.padded_codes(frames), S, D, D)[1:1 + S]
    assert torch.equal(x, gc.embed_ref(emb, frames))
    n = 0
    for s in range(S):
        if st0["active"][s] and out["active"][s]:
            assert out["offset"][s] == st0["offset"][s] + 1
            assert torch.equal(out["x"][2 * s], x[s]) and torch.equal(out["x"][2 * s + 1], x[s]), s
            n += 1
        else:
            assert not out["x"][2 * s:2 * s + 2].any()
    assert n >= 2


# ----------------------------------------------------------------------------- standalone delay pattern
def _guarded(shape_numel, dtype):
    """A flat guard-filled buffer with 16 guard elements on either side of `shape_numel` payload elements."""
    return torch.full((shape_numel + 32,), IG, dtype=dtype, device=DEV)


@pytest.mark.parametrize("batch,mask", [(1, 1025), (3, 1025), (3, 777)])
@pytest.mark.parametrize("T", gc.APPLY_T)
def test_apply_and_revert_delay_pattern_match_the_oracle(T, batch, mask):
    L = _lib()
    codes = gc.audio_codes(batch, T)
    want = gc.apply_delay_pattern(codes, mask)
    n = want.numel()
    buf = _guarded(n, torch.int64)
    c = codes.to(DEV)
    L.check(L.lib().zmi_apply_delay_pattern(c.data_ptr(), buf.data_ptr() + 16 * 8, batch, T, mask, _sp()), "apply")
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.equal(got[16:16 + n].view(batch, NCB, T + NCB), want)
    assert bool((got[:16] == IG).all()) and bool((got[16 + n:] == IG).all())
    # revert what was applied, and a buffer of other values in the mask positions
    for src in (want, want + 1):
        back = _guarded(codes.numel(), torch.int64)
        s = src.to(DEV)
        L.check(L.lib().zmi_revert_delay_pattern(s.data_ptr(), back.data_ptr() + 16 * 8, batch, T + NCB, _sp()),
                "revert")
        torch.cuda.synchronize()
        got = back.cpu()
        assert torch.equal(got[16:16 + codes.numel()].view(batch, NCB, T), gc.revert_delay_pattern(src))
        assert bool((got[:16] == IG).all()) and bool((got[16 + codes.numel():] == IG).all())


# ----------------------------------------------------------------------------- the slots' delayed buffer
@pytest.mark.parametrize("slot", [0, 2], ids=["first_slot", "last_slot"])
@pytest.mark.parametrize("tcap", gc.INIT_TCAP)
def test_delay_init_matches_the_oracle(tcap, slot):
    """Every (prefix_len, total_len) that fits: the slot's [9, tcap] equals the oracle's pattern of [prefix | -1 ...],
    MASK from total_len on; the other slots' contents and the guard elements are unchanged."""
    L = _lib()
    S = 3
    for tc, p, total in gc.init_cases():
        if tc != tcap:
            continue
        buf = _guarded(S * NCB * tcap, torch.int32)
        delayed = buf[16:16 + S * NCB * tcap].view(S, NCB, tcap)
        sl, keep = _slots(L, delayed)
        prefix = gc.audio_codes(1, p, tcap)[0]
        pre = prefix.to(torch.int32).contiguous().to(DEV) if p else None
        L.check(L.lib().zmi_delay_init(ctypes.byref(sl), slot, L.ptr(pre), p, total, _sp()), "delay_init")
        torch.cuda.synchronize()
        got = buf.cpu()
        d = got[16:16 + S * NCB * tcap].view(S, NCB, tcap)
        assert torch.equal(d[slot], gc.init_ref(tcap, prefix, total)), (tcap, p, total)
        others = [s for s in range(S) if s != slot]
        assert bool((d[others] == IG).all()) and bool((got[:16] == IG).all()) and bool((got[-16:] == IG).all())


@pytest.mark.parametrize("tcap", [64, 300])
def test_delay_revert_and_range_match_the_oracle(tcap):
    """A buffer over -1, 0, 1023, 1024, 1025: values >= 1024 become 0 and -1 stays; first and last slot; the range
    form equals the slice of the full revert for several (t0, n), n = 0 included."""
    L = _lib()
    S = 3
    host = gc.revert_buffer(S, tcap)
    sl, keep = _slots(L, host.to(DEV))
    t_full = tcap - NCB
    for slot in (0, S - 1):
        full = None
        for t_out in (1, 9, t_full):
            buf = _guarded(NCB * t_out, torch.int64)
            L.check(L.lib().zmi_delay_revert(ctypes.byref(sl), slot, buf.data_ptr() + 16 * 8, t_out, _sp()), "revert")
            torch.cuda.synchronize()
            got = buf.cpu()
            full = got[16:16 + NCB * t_out].view(NCB, t_out)
            assert torch.equal(full, gc.revert_ref(host[slot], t_out)), (slot, t_out)
            assert bool((got[:16] == IG).all()) and bool((got[-16:] == IG).all())
        assert set(full.unique().tolist()) == {-1, 0, 1023}
        for t0, n in ((0, 1), (0, t_full), (5, 17), (t_full - 1, 1), (t_full - 40, 40), (3, 0), (t_full, 0)):
            buf = _guarded(NCB * n, torch.int64)
            L.check(L.lib().zmi_delay_revert_range(ctypes.byref(sl), slot, t0, n, buf.data_ptr() + 16 * 8, _sp()),
                    "revert_range")
            torch.cuda.synchronize()
            got = buf.cpu()
            assert torch.equal(got[16:16 + NCB * n].view(NCB, n), full[:, t0:t0 + n]), (slot, t0, n)
            assert bool((got[:16] == IG).all()) and bool((got[16 + NCB * n:] == IG).all())
    assert torch.equal(keep[2].cpu(), host)


# ----------------------------------------------------------------------------- refused arguments
def test_delay_revert_refuses_a_bad_slot_and_a_null_output():
    L = _lib()
    sl, keep = _slots(L, gc.revert_buffer(3, 64).to(DEV))
    out = torch.full((NCB, 12), IG, dtype=torch.int64, device=DEV)
    for slot in (-1, 3, 1 << 20):
        _refused(L.lib().zmi_delay_revert(ctypes.byref(sl), slot, out.data_ptr(), 12, _sp()), "delay_revert")
    _refused(L.lib().zmi_delay_revert(ctypes.byref(sl), 0, None, 12, _sp()), "delay_revert")
    _refused(L.lib().zmi_delay_revert(ctypes.byref(sl), 0, out.data_ptr(), 64 - NCB + 1, _sp()), "delay_revert")
    _refused(L.lib().zmi_delay_revert_range(ctypes.byref(sl), 3, 0, 4, out.data_ptr(), _sp()), "delay_revert_range")
    torch.cuda.synchronize()
    assert bool((out == IG).all())


def test_delay_init_refuses_negative_lengths_and_a_null_prefix():
    L = _lib()
    delayed = torch.full((3, NCB, 64), IG, dtype=torch.int32, device=DEV)
    sl, keep = _slots(L, delayed)
    pre = gc.audio_codes(1, 7)[0].to(torch.int32).to(DEV)
    lib = L.lib()
    _refused(lib.zmi_delay_init(ctypes.byref(sl), 0, pre.data_ptr(), -1, 30, _sp()), "delay_init")
    _refused(lib.zmi_delay_init(ctypes.byref(sl), 0, pre.data_ptr(), 7, -1, _sp()), "delay_init")
    _refused(lib.zmi_delay_init(ctypes.byref(sl), 0, None, 7, 30, _sp()), "delay_init")
    _refused(lib.zmi_delay_init(ctypes.byref(sl), 0, pre.data_ptr(), 7, 65, _sp()), "delay_init")
    _refused(lib.zmi_delay_init(ctypes.byref(sl), 3, pre.data_ptr(), 7, 30, _sp()), "delay_init")
    _refused(lib.zmi_delay_init(ctypes.byref(sl), -1, pre.data_ptr(), 7, 30, _sp()), "delay_init")
    torch.cuda.synchronize()
    assert bool((delayed == IG).all())


def test_embed_codes_refuses_short_strides_and_null_pointers():
    L = _lib()
    d, n = 8, 3
    tab, emb = _table(d, "cancel")
    codes = gc.padded_codes(gc.code_columns(n)).to(DEV)
    x = torch.full((n + 2, d + 8), XG, dtype=torch.bfloat16, device=DEV)
    lib, ld = L.lib(), codes.shape[1]
    call = lambda c, ldc, n_, e, d_, x_, ldx: lib.zmi_embed_codes(c, ldc, n_, e, d_, x_, ldx, _sp())  # noqa: E731
    good = (codes.data_ptr(), ld, n, emb.data_ptr(), d, x.data_ptr() + 2 * (d + 8), d + 8)
    for i, bad in ((6, d - 8), (6, 0), (1, n - 1), (0, None), (3, None), (5, None), (4, 12), (4, 0), (2, 0)):
        a = list(good)
        a[i] = bad
        _refused(call(*a), "embed_codes")
    torch.cuda.synchronize()
    assert bool((x == XG).all())


def test_embed_step_refuses_null_pointers():
    L = _lib()
    d = 8
    tab, emb = _table(d, "cancel")
    st = gc.step_state(16)
    sl, keep = _slots(L, st["delayed"].to(DEV), st["active"], st["offset"], st["pos"])
    x = torch.full((8, d), XG, dtype=torch.bfloat16, device=DEV)
    row_kv = torch.full((8,), IG, dtype=torch.int32, device=DEV)
    row_pos = torch.full((8,), IG, dtype=torch.int32, device=DEV)
    lib = L.lib()
    _refused(lib.zmi_embed_step(ctypes.byref(sl), None, d, x.data_ptr(), row_kv.data_ptr(), row_pos.data_ptr(), _sp()),
             "embed_step")
    _refused(lib.zmi_embed_step(ctypes.byref(sl), emb.data_ptr(), d, None, row_kv.data_ptr(), row_pos.data_ptr(),
                                _sp()), "embed_step")
    _refused(lib.zmi_embed_step(ctypes.byref(sl), emb.data_ptr(), 12, x.data_ptr(), row_kv.data_ptr(),
                                row_pos.data_ptr(), _sp()), "embed_step")
    torch.cuda.synchronize()
    assert bool((x == XG).all()) and bool((row_kv == IG).all()) and bool((row_pos == IG).all())
