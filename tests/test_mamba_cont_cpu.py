"""The continued Mamba2 scan and chunked prefill, without a GPU: zmi_mamba2_scan_cont's host refusals (fake pointers,
never dereferenced), the input conditions of tests/mamba_cases.py on every link and crafted start of
tests/mamba_cont_cases.py, the criterion against float32-emulated mutants of a continuation, the chunk planner
(prefill_plan.ChunkPlanner) and SlotScheduler.fit with and without prefill_chunk."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import mamba_cases as mc
from tests import mamba_cont_cases as cc
from tests.mamba_cases import CASES, MD
from zonos_vibes_amd.config import tiny_hybrid
from zonos_vibes_amd.prefill_plan import ChunkPlanner, check_chunk, chunk_bounds
from zonos_vibes_amd.serving import SlotScheduler

M = 12


# ---------------------------------------------------------------------------------------------- host refusals
def _call(seqs, n_seq=None, ws_bytes=None, m=M):
    from zonos_vibes_amd import _lib as L
    lib = L.lib()
    md = tiny_hybrid().backbone.mamba2_dims()
    a = L.Mamba2Args()
    fake = 0x1000  # non-null, never read: every case below returns from the host checks
    a.zxbcdt, a.ld_zx, a.M = fake, md["d_in_proj"], m
    a.d_ssm, a.nheads, a.headdim, a.d_state, a.d_conv, a.ngroups = md["d_ssm"], md["nheads"], 64, 128, 4, 1
    a.conv_w = a.conv_b = a.dt_bias = a.A = a.D = a.conv_ring = a.ssm = a.y = a.row_pos = fake
    a.ldy = md["d_ssm"]
    sa = np.ascontiguousarray(np.asarray(seqs, dtype=np.int32).reshape(-1, 4))
    n = len(sa) if n_seq is None else n_seq
    n_cont = int(((sa[:, 3] > 0) & (sa[:, 1] > 0)).sum())  # one state copy per continuing, non-empty sequence
    nb = int(lib.zmi_mamba2_scan_cont_ws_bytes(m, md["d_ssm"], md["nheads"], n_cont))
    rc = lib.zmi_mamba2_scan_cont(ctypes.byref(a), fake, n, sa.ctypes.data, fake,
                                  nb if ws_bytes is None else nb + ws_bytes, None)
    return rc, lib.zmi_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(seqs=[(0, 4, 0, 0)], n_seq=-1), b"n_seq"),
    (dict(seqs=[(0, -1, 0, 0)]), b"negative"),
    (dict(seqs=[(-1, 4, 0, 0)]), b"negative"),
    (dict(seqs=[(0, 4, 0, 0), (9, 4, 1, 5)]), b"past M"),
    (dict(seqs=[(0, 2 ** 31 - 1, 0, 0)]), b"past M"),
    (dict(seqs=[(0, 4, 0, -1)]), b"pos0"),
    (dict(seqs=[(0, 4, 0, 2 ** 31 - 2)]), b"pos0"),
    (dict(seqs=[(0, 4, -1, 3)]), b"kv_row"),
    (dict(seqs=[(0, 5, 0, 0), (8, 2, 2, 7), (4, 4, 1, 0)]), b"share rows"),
    (dict(seqs=[(0, 4, 1, 4), (8, 2, 0, 0), (4, 4, 1, 0)]), b"share a kv_row"),
    (dict(seqs=[(0, 4, 0, 1)], ws_bytes=-1), b"workspace"),
])
def test_refused_on_the_host(kw, word):
    rc, msg = _call(**kw)
    assert rc != 0 and word in msg and b"mamba2_scan_cont" in msg, (rc, msg)


def test_a_continuing_sequence_passes_the_checks():
    """pos0 = 1 is accepted as far as the host checks go: with the workspace one byte short the call is refused for
    the workspace, the last check before the launches, and for nothing before it."""
    rc, msg = _call([(0, 4, 0, 1), (4, 3, 1, 0), (8, 4, 2, 530), (12, 0, 3, 7)], ws_bytes=-1)
    assert rc != 0 and b"workspace" in msg, (rc, msg)  # (two copies: the starting and the empty sequence need none)
    assert _call([], n_seq=0)[0] == 0
    assert _call([(0, 0, 0, 9), (5, 0, 0, 0), (M, 0, 2, 3)])[0] == 0  # empty sequences are skipped


def test_workspace_size():
    """zmi_mamba2_scan_ws_bytes plus one bf16 state per continuing sequence."""
    from zonos_vibes_amd import _lib as L
    lib = L.lib()
    base = int(lib.zmi_mamba2_scan_ws_bytes(100, 192, 3))
    assert int(lib.zmi_mamba2_scan_cont_ws_bytes(100, 192, 3, 0)) == base
    assert int(lib.zmi_mamba2_scan_cont_ws_bytes(100, 192, 3, 5)) == base + 5 * 3 * 64 * 128 * 2
    assert int(lib.zmi_mamba2_scan_cont_ws_bytes(100, 192, 3, -1)) == 0


# ---------------------------------------------------------------------------------------------- input conditions
def _conditions(r, T):
    """A link of T positions from a carried state: one more term than a sequence from an empty one."""
    assert not mc.unsafe(r.acc, r.acc_abs).any()
    assert mc.clear_of_underflow(r.y_abs, 128 * (T + 1)) and mc.clear_of_underflow(r.state_abs, T + 1)
    assert torch.isfinite(r.y64).all() and torch.isfinite(r.state64).all()


@pytest.mark.parametrize("case", list(CASES))
def test_chain_links_meet_the_input_conditions(case):
    """Every link, started from the fp64 chain's own state rounded to bf16 where the library stores it (the GPU test
    starts each link from the state the library stored: the same up to the criterion)."""
    for cuts in cc.CHAINS:
        inp = mc.build(case, cuts[-1])
        state, ring = None, None
        for a, b in cc.links(cuts):
            r = cc.link_ref(inp, a, b, state, ring)
            _conditions(r, b - a)
            state, ring = r.state64.to(mc.BF), r.ring
    assert all(a > 1 or b - a > 1 for cuts in cc.CHAINS for a, b in cc.links(cuts)[:1])  # no single-position first link


@pytest.mark.parametrize("case", list(CASES))
def test_crafted_starts_meet_the_input_conditions(case):
    for pos0, T in cc.STARTS:
        i, st, rg = cc.start_probe(case, pos0, T)
        r = mc.ref64(i.zx, *i.params, MD, state0=st, ring0=rg, pos0=pos0)
        _conditions(r, T)
        assert torch.equal(torch.from_numpy(mc.emu_conv(i, rg, pos0)).to(mc.BF), r.xc)
        # the ring keeps STALE_RING exactly in the slots no position has written
        written = {q & 3 for q in range(max(pos0 - 3, 0), pos0 + T)}
        for k in range(4):
            assert bool((r.ring[k] == mc.STALE_RING).all()) == (k not in written)


@pytest.mark.parametrize("case", ["mix", "dt"])
def test_wide_starts_meet_the_input_conditions(case):
    """The 256-position crafted starts of the full-width launch; widen() repeats the regimes head by head."""
    for pos0 in cc.WIDE_POS0:
        i, st, rg = cc.start_probe(case, pos0, cc.WIDE_LEN)
        _conditions(mc.ref64(i.zx, *i.params, MD, state0=st, ring0=rg, pos0=pos0), cc.WIDE_LEN)
    zx, (cw, cb, dtb, A, D), st8, rg8 = cc.widen(i, st, rg, 8)
    assert zx.shape == (cc.WIDE_LEN, 2 * 512 + 256 + 8) and cw.shape == (512 + 256, 4) and rg8.shape == (4, 512 + 256)
    for h in range(8):
        k = h % 3
        assert torch.equal(zx[:, 512 + h * 64: 512 + (h + 1) * 64], i.zx[:, 192 + k * 64: 192 + (k + 1) * 64])  # x
        assert torch.equal(zx[:, h * 64: (h + 1) * 64], i.zx[:, k * 64: (k + 1) * 64])  # z
        assert torch.equal(zx[:, 2 * 512 + 256 + h], i.zx[:, 2 * 192 + 256 + k])  # dt
        assert torch.equal(cw[h * 64: (h + 1) * 64], i.cw[k * 64: (k + 1) * 64]) and A[h] == i.A[k]
        assert torch.equal(st8[h], st[k]) and torch.equal(rg8[:, h * 64: (h + 1) * 64], rg[:, k * 64: (k + 1) * 64])
    assert torch.equal(zx[:, 1024: 1024 + 256], i.zx[:, 384: 384 + 256]) and torch.equal(rg8[:, 512:], rg[:, 192:])


# ---------------------------------------------------------------------------------------------- emulation and mutants
def _worst(y, s, r):
    return max(mc.head_max(mc.ratio(y, r.y64, r.y_abs))), max(mc.head_max(mc.ratio(s, r.state64, r.state_abs)))


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_continuation_meets_the_bound(case):
    """The recurrence in float32 from the carried state and ring: within the criterion on every crafted start of 33
    positions and on the shortest."""
    for pos0, T in [(p, n) for p, n in cc.STARTS if n in (1, 33)]:
        i, st, rg = cc.start_probe(case, pos0, T)
        r = mc.ref64(i.zx, *i.params, MD, state0=st, ring0=rg, pos0=pos0)
        wy, ws = _worst(*mc.emu_recurrence(i, xc=mc.emu_conv(i, rg, pos0), state0=st), r)
        print(f"{case} pos0={pos0} T={T}: y {wy:.3f} state {ws:.3f}")
        assert wy <= 1.0 and ws <= 1.0


def test_mutant_carried_state_dropped():
    """A scan that starts its registers from 0 instead of h0: y misses on every case with a state, the final state
    where a head still remembers its start after 33 positions (the dt case's heads have all forgotten it by then)."""
    for case in ("mix", "dt", "cancel"):
        i, st, rg = cc.start_probe(case, 5, 33)
        r = mc.ref64(i.zx, *i.params, MD, state0=st, ring0=rg, pos0=5)
        wy, ws = _worst(*mc.emu_recurrence(i, xc=mc.emu_conv(i, rg, 5), state0=None), r)
        assert wy > 8.0 and (ws > 8.0 or case == "dt"), (case, wy, ws)


def test_mutant_ring_history_replaced_by_zeros():
    """A conv that reads zero for the three positions before pos0: the conv case's y is the conv output itself."""
    i, st, rg = cc.start_probe("conv", 5, 4)
    r = mc.ref64(i.zx, *i.params, MD, state0=st, ring0=rg, pos0=5)
    xc = mc.emu_conv(i, None, 5)
    assert not torch.equal(torch.from_numpy(xc).to(mc.BF)[:3], r.xc[:3])
    assert torch.equal(torch.from_numpy(xc).to(mc.BF)[3:], r.xc[3:])  # position pos0 + 3 reads no history
    wy, _ = _worst(*mc.emu_recurrence(i, xc=xc, state0=st), r)
    assert wy > 8.0, wy


@pytest.mark.parametrize("pos0", [1, 2])
def test_mutant_stale_slot_read_below_position_0(pos0):
    """A conv that takes slot q & 3 for a position q < 0 instead of zero: at pos0 + 4 the same three slots are read,
    every one as a position that exists."""
    i, st, rg = cc.start_probe("conv", pos0, 3)
    r = mc.ref64(i.zx, *i.params, MD, state0=st, ring0=rg, pos0=pos0)
    good = mc.emu_conv(i, rg, pos0)
    assert torch.equal(torch.from_numpy(good).to(mc.BF), r.xc)
    stale = mc.emu_conv(i, rg, pos0 + 4)
    wy, _ = _worst(*mc.emu_recurrence(i, xc=stale, state0=st), r)
    assert wy > 8.0 and math.isfinite(wy), wy


# ---------------------------------------------------------------------------------------------- the planner
def test_chunk_bounds_and_check():
    assert chunk_bounds(171, 32) == [(0, 32), (32, 64), (64, 96), (96, 128), (128, 160), (160, 171)]
    assert chunk_bounds(64, 64) == [(0, 64)] and chunk_bounds(65, 64) == [(0, 64), (64, 65)]
    assert chunk_bounds(5, 1) == [(k, k + 1) for k in range(5)]
    assert check_chunk(None, 64) is None and check_chunk(64, 64) == 64 and check_chunk(1, 64) == 1
    assert check_chunk(4096) == 4096  # no upper bound where none is given (the model, before it sizes the engine)
    with pytest.raises(ValueError):
        check_chunk(0)
    for bad in (0, -1, 65, 2.5, True):
        with pytest.raises(ValueError):
            check_chunk(bad, 64)


def _drain(pl):
    out = []
    while pl.pending:
        out.append(pl.next_pass())
    assert pl.next_pass() is None
    return out


@pytest.mark.parametrize("rps", [1, 2])
def test_planner_covers_every_position_once_in_order(rps):
    lens = {3: 171, 0: 20, 5: 64, 1: 65, 2: 300}
    pl = ChunkPlanner(pre_rows=256, rows_per_slot=rps, chunk=32)
    for s, n in lens.items():
        pl.add(s, n)
    assert pl.slots() == list(lens)
    passes = _drain(pl)
    seen = {s: [] for s in lens}
    for ps in passes:
        assert 0 < ps.rows <= 256
        assert len({e.slot for e in ps.entries}) == len(ps.entries)  # at most one chunk per slot
        rows = []
        for e in ps.entries:
            seen[e.slot].append((e.begin, e.end))
            assert e.last == (e.end == lens[e.slot])
            rows += list(range(e.off, e.off + rps * (e.end - e.begin)))
        assert rows == list(range(ps.rows))  # packed without gaps or overlap
        sq = ps.seqs(rps)
        assert len(sq) == rps * len(ps.entries)
        for k, e in enumerate(ps.entries):  # a slot's sequences sit in the same pass, on its KV rows, from pos0 = begin
            for half in range(rps):
                assert sq[rps * k + half] == (e.off + half * (e.end - e.begin), e.end - e.begin, rps * e.slot + half,
                                              e.begin)
        assert ps.max_pos == max(e.end for e in ps.entries) - 1
        order = [list(lens).index(e.slot) for e in ps.entries]
        assert order == sorted(order)  # oldest first
    for s, n in lens.items():
        assert seen[s] == chunk_bounds(n, 32)  # every position once, in order, boundaries the prompt's own


def test_planner_boundaries_do_not_depend_on_batch_mates():
    alone = ChunkPlanner(2048, 2, 37)
    alone.add(0, 171)
    a = [(e.begin, e.end) for ps in _drain(alone) for e in ps.entries]
    crowd = ChunkPlanner(128, 2, 37)
    for s, n in ((4, 50), (0, 171), (2, 38), (7, 200)):
        crowd.add(s, n)
    b = [(e.begin, e.end) for ps in _drain(crowd) for e in ps.entries if e.slot == 0]
    assert a == b == chunk_bounds(171, 37)


def test_planner_pass_limit_and_fifo():
    pl = ChunkPlanner(pre_rows=128, rows_per_slot=2, chunk=32)  # two chunks of 32 positions (2 x 2 x 32 rows) a pass
    for s in (0, 1, 2):
        pl.add(s, 40)
    p1 = pl.next_pass()
    assert [(e.slot, e.begin, e.end) for e in p1.entries] == [(0, 0, 32), (1, 0, 32)] and p1.rows == 128
    p2 = pl.next_pass()  # the older prompts' tails first, then the youngest's head: 16 + 16 + 64 rows
    assert [(e.slot, e.begin, e.end, e.last) for e in p2.entries] == [(0, 32, 40, True), (1, 32, 40, True),
                                                                       (2, 0, 32, False)]
    assert pl.slots() == [2]
    pl.add(0, 5, job="payload")  # what add() is given travels with the prompt's chunks
    assert pl.drop(2) and not pl.drop(2)  # a cancelled request's remaining chunks are gone
    assert [(e.slot, e.begin, e.end, e.last, e.job) for e in pl.next_pass().entries] == [(0, 0, 5, True, "payload")]
    assert not pl.pending
    with pytest.raises(ValueError):
        ChunkPlanner(pre_rows=63, rows_per_slot=2, chunk=32)
    pl.add(1, 9)
    with pytest.raises(ValueError):
        pl.add(1, 9)


# ---------------------------------------------------------------------------------------------- SlotScheduler.fit
def test_scheduler_fit_with_and_without_prefill_chunk():
    plain = SlotScheduler(2, max_seqlen=256, max_prefill=64, d_model=512)
    chunked = SlotScheduler(2, max_seqlen=256, max_prefill=64, d_model=512, prefill_chunk=32)
    assert plain.prefill_chunk is None and chunked.prefill_chunk == 32
    long_req = ((2, 20, 512), (1, 9, 150), 40)  # Lc + P + 1 = 171 > max_prefill
    with pytest.raises(ValueError, match="max_prefill"):
        plain.fit(*long_req)
    assert chunked.fit(*long_req) == (20, 150)
    assert plain.fit((2, 20, 512), (1, 9, 43), 40) == chunked.fit((2, 20, 512), (1, 9, 43), 40) == (20, 43)
    for s in (plain, chunked):  # the KV capacity check stays
        with pytest.raises(ValueError, match="max_seqlen"):
            s.fit((2, 20, 512), (1, 9, 150), 80)
    for bad in (0, 65):
        with pytest.raises(ValueError):
            SlotScheduler(2, max_seqlen=256, max_prefill=64, prefill_chunk=bad)
    t = chunked.submit(*long_req)
    assert chunked.begin_round() == ([], [(0, chunked.busy()[0][1])]) and chunked.busy()[0][1].ticket == t
