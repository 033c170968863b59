"""zmi_mamba2_scan_seqs: the Mamba2 prefill scan over ragged sequences in one pass (conv + dt launch, then the SSD
form and / or mamba2_scan2_kernel over the sequence table). Every sequence is held bit for bit to zmi_mamba2_scan_ws
of that sequence alone, and to oracle/hybrid_cpu.py within the bounds of test_mamba2_scan_matches_oracle; rows and
state rows the table does not list keep their bits; the host checks refuse a bad table before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.hybrid_cpu import mamba2_scan_ref
from tests.test_gpu_hybrid import _args, _bf, _mamba_params, _ulps
from zonos_vibes_amd.config import tiny_hybrid, zonos_v01_hybrid

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -77.0  # exact in bf16
STALE_RING, STALE_SSM = 7.0, 3.0

# lengths around the 32-position tile edge and the SSD form's reach (256 | 257: a mixed pass under the default option)
LENS = [1, 3, 32, 33, 45, 256, 257]
KV = [5, 0, 9, 2, 7, 3, 11]  # a permutation with holes of the 12 state rows
N_KV = 12
PLACE = [4, 0, 6, 2, 5, 1, 3]  # the order the sequences lie in the buffers: not the table's, not by length
GAP = {4: 2, 2: 3}  # sentinel rows before the first sequence and between two others


def _L():
    from zonos_vibes_amd import _lib
    return _lib, _lib.lib()


def _table(lens, place, gap, tail=1):
    """ZmiAttnSeq rows (q_row0, len, kv_row, pos0) in table order, the row count, and the rows no sequence owns."""
    q0, row, free = [0] * len(lens), 0, []
    for s in place:
        free += list(range(row, row + gap.get(s, 0)))
        row += gap.get(s, 0)
        q0[s] = row
        row += lens[s]
    free += list(range(row, row + tail))
    return q0, row + tail, free


class Launch:
    """Buffers of one zmi_mamba2_scan_seqs call: stale everywhere, so that only what the call writes changes."""

    def __init__(self, md, m, n_kv, seed=22):
        L, lib = _L()
        self.md, self.m = md, m
        self.p = _mamba_params(md, 21)
        self.pd = [t.to(DEV) for t in self.p]
        self.zx = _bf(m, md["d_in_proj"], seed=seed)
        self.zxd = self.zx.to(DEV)
        self.ring = torch.full((n_kv, 4, md["conv_dim"]), STALE_RING, dtype=torch.bfloat16, device=DEV)
        self.ssm = torch.full((n_kv, md["nheads"], 64, 128), STALE_SSM, dtype=torch.bfloat16, device=DEV)
        self.y = torch.full((m, md["d_ssm"]), SENTINEL, dtype=torch.bfloat16, device=DEV)
        self.rp = torch.zeros(m, dtype=torch.int32, device=DEV)
        self.nb = int(lib.zmi_mamba2_scan_ws_bytes(m, md["d_ssm"], md["nheads"]))
        self.ws = torch.full((max(self.nb, 1),), 0xA5, dtype=torch.uint8, device=DEV)  # stale workspace must not matter
        self.a = _args(L, md, self.zxd, *self.pd, self.ring, self.ssm, self.y, m, self.rp)

    def run(self, seqs, nb=None, n_seq=None):
        """-> the call's status; seqs: (q_row0, len, kv_row, pos0) rows."""
        L, lib = _L()
        sa = np.ascontiguousarray(np.asarray(seqs, dtype=np.int32).reshape(-1, 4))
        dev = torch.from_numpy(np.concatenate([sa.ravel(), np.zeros(4, np.int32)])).to(DEV)  # (never empty)
        rc = lib.zmi_mamba2_scan_seqs(ctypes.byref(self.a), dev.data_ptr(), len(sa) if n_seq is None else n_seq,
                                      sa.ctypes.data, self.ws.data_ptr(), self.nb if nb is None else nb, 0)
        torch.cuda.synchronize()
        return rc

    def snapshot(self):
        return [t.clone() for t in (self.y, self.ssm, self.ring, self.ws)]

    def unchanged(self, snap):
        torch.cuda.synchronize()
        return all(torch.equal(a, b) for a, b in zip(snap, (self.y, self.ssm, self.ring, self.ws)))


def _alone(md, params_dev, zx_rows):
    """zmi_mamba2_scan_ws of one sequence on its own (M = seq_len = len) under the current option -> (y, state, ring)."""
    L, lib = _L()
    n = zx_rows.shape[0]
    zxd = zx_rows.to(DEV).contiguous()
    ring = torch.full((1, 4, md["conv_dim"]), STALE_RING, dtype=torch.bfloat16, device=DEV)
    ssm = torch.full((1, md["nheads"], 64, 128), STALE_SSM, dtype=torch.bfloat16, device=DEV)
    y = torch.zeros(n, md["d_ssm"], dtype=torch.bfloat16, device=DEV)
    rp = torch.arange(n, dtype=torch.int32, device=DEV)
    a = _args(L, md, zxd, *params_dev, ring, ssm, y, n, rp)
    nb = int(lib.zmi_mamba2_scan_ws_bytes(n, md["d_ssm"], md["nheads"]))
    ws = torch.full((nb,), 0x5A, dtype=torch.uint8, device=DEV)
    L.check(lib.zmi_mamba2_scan_ws(ctypes.byref(a), n, ws.data_ptr(), nb, 0), "scan_ws")
    torch.cuda.synchronize()
    return y, ssm[0], ring[0]


def _with_option(pq, fn):
    L, lib = _L()
    old = lib.zmi_get_option(L.OPT_SCAN_PQ)
    lib.zmi_set_option(L.OPT_SCAN_PQ, pq)
    try:
        return fn()
    finally:
        lib.zmi_set_option(L.OPT_SCAN_PQ, old)


@pytest.fixture(scope="module", params=[0, 4], ids=["pq0_mixed", "pq4"])
def ragged(request):
    """One ragged launch over LENS under ZMI_OPT_SCAN_PQ = 0 (SSD up to 256 positions + the 4-workgroup scan for 257)
    or 4, and each sequence alone under the same option."""
    md = tiny_hybrid().backbone.mamba2_dims()
    q0, m, free = _table(LENS, PLACE, GAP)
    seqs = [(q0[s], LENS[s], KV[s], 0) for s in range(len(LENS))]

    def both():
        ln = Launch(md, m, N_KV)
        L, _ = _L()
        L.check(ln.run(seqs), "scan_seqs")
        return ln, [_alone(md, ln.pd, ln.zx[q: q + n]) for q, n, _, _ in seqs]
    ln, alone = _with_option(request.param, both)
    return dict(md=md, ln=ln, seqs=seqs, alone=alone, free=free)


@pytest.fixture(scope="module")
def oracle():
    """mamba2_scan_ref of each sequence of LENS on its own (the inputs do not depend on the option)."""
    md = tiny_hybrid().backbone.mamba2_dims()
    q0, m, _ = _table(LENS, PLACE, GAP)
    zx = _bf(m, md["d_in_proj"], seed=22)
    p = _mamba_params(md, 21)
    return [mamba2_scan_ref(zx[q0[s]: q0[s] + LENS[s]][None], *p, md) for s in range(len(LENS))]


def test_ragged_launch_equals_each_sequence_alone(ragged):
    ln = ragged["ln"]
    for (q, n, kv, _), (y1, s1, r1) in zip(ragged["seqs"], ragged["alone"]):
        assert torch.equal(ln.y[q: q + n], y1), ("y", n)
        assert torch.equal(ln.ssm[kv], s1), ("state", n)
        for k in range(4):
            assert torch.equal(ln.ring[kv, k], r1[k]), ("ring", n, k)
        assert not (y1 == SENTINEL).all(dim=-1).any()


def test_ragged_launch_matches_oracle(ragged, oracle):
    """The bounds of test_mamba2_scan_matches_oracle: y within 4 bf16 ulps, state within 1, ring slots exact."""
    ln = ragged["ln"]
    for (q, n, kv, _), (ry, rs, rconv) in zip(ragged["seqs"], oracle):
        uy, us = _ulps(ln.y[q: q + n], ry[0]), _ulps(ln.ssm[kv], rs[0])
        print(f"len {n}: y {uy:.2f} ulps, state {us:.2f} ulps")
        assert uy <= 4.0, (n, uy)
        assert us <= 1.0, (n, us)
        for k in range(4):
            p = n - 4 + k
            assert torch.equal(ln.ring[kv, p & 3].cpu(), rconv[0, :, k]), (n, k)


def test_nothing_else_is_touched(ragged):
    ln, free = ragged["ln"], ragged["free"]
    assert len(free) == 6 and free[0] == 0
    assert (ln.y[free] == SENTINEL).all()
    for kv in sorted(set(range(N_KV)) - set(KV)):
        assert (ln.ssm[kv] == STALE_SSM).all(), kv
        assert (ln.ring[kv] == STALE_RING).all(), kv


def test_full_width_heads():
    """64 heads, d_ssm 4096 (Zonos-v0.1-hybrid): lengths 161 and 45 in one launch under the default option."""
    md = zonos_v01_hybrid().backbone.mamba2_dims()
    assert (md["nheads"], md["d_ssm"]) == (64, 4096)
    lens = [161, 45]
    q0, m, free = _table(lens, [1, 0], {0: 1})
    seqs = [(q0[0], 161, 2, 0), (q0[1], 45, 0, 0)]
    ln = Launch(md, m, 3)
    L, lib = _L()
    assert lib.zmi_get_option(L.OPT_SCAN_PQ) == 0
    L.check(ln.run(seqs), "scan_seqs")
    for q, n, kv, _ in seqs:
        y1, s1, r1 = _alone(md, ln.pd, ln.zx[q: q + n])
        assert torch.equal(ln.y[q: q + n], y1), ("y", n)
        assert torch.equal(ln.ssm[kv], s1), ("state", n)
        assert torch.equal(ln.ring[kv], r1), ("ring", n)
    assert (ln.y[free] == SENTINEL).all()
    assert (ln.ssm[1] == STALE_SSM).all() and (ln.ring[1] == STALE_RING).all()


def test_edge_counts():
    md = tiny_hybrid().backbone.mamba2_dims()
    ln = Launch(md, 12, 3)
    snap = ln.snapshot()
    assert ln.run([], n_seq=0) == 0 and ln.unchanged(snap)
    assert ln.run([(0, 0, 0, 0), (5, 0, 1, 0), (12, 0, 2, 0)]) == 0 and ln.unchanged(snap)
    # an empty sequence among live ones is skipped: its rows (inside another's) and its state row stay out of it
    seqs = [(1, 4, 2, 0), (2, 0, 1, 0), (6, 5, 0, 0)]
    assert ln.run(seqs) == 0
    for q, n, kv, _ in seqs:
        if n:
            y1, s1, r1 = _alone(md, ln.pd, ln.zx[q: q + n])
            assert torch.equal(ln.y[q: q + n], y1) and torch.equal(ln.ssm[kv], s1) and torch.equal(ln.ring[kv], r1)
    assert (ln.y[[0, 5, 11]] == SENTINEL).all()
    assert (ln.ssm[1] == STALE_SSM).all() and (ln.ring[1] == STALE_RING).all()


REFUSED = {
    "n_seq < 0": dict(seqs=[(0, 4, 0, 0)], n_seq=-1),
    "len < 0": dict(seqs=[(0, -1, 0, 0)]),
    "q_row0 < 0": dict(seqs=[(-1, 4, 0, 0)]),
    "q_row0 + len > M": dict(seqs=[(0, 4, 0, 0), (9, 4, 1, 0)]),
    "pos0 != 0": dict(seqs=[(0, 4, 0, 1)]),
    "kv_row < 0": dict(seqs=[(0, 4, -1, 0)]),
    "overlapping rows": dict(seqs=[(0, 5, 0, 0), (4, 4, 1, 0)]),
    "same kv_row": dict(seqs=[(0, 4, 1, 0), (4, 4, 1, 0)]),
    "ws too small": dict(seqs=[(0, 4, 0, 0)], nb=-1),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refusals(case):
    """Host checks on well-formed buffers: a non-zero return, a message, and nothing written (none reaches a launch)."""
    _, lib = _L()
    md = tiny_hybrid().backbone.mamba2_dims()
    ln = Launch(md, 12, 3)
    snap = ln.snapshot()
    kw = dict(REFUSED[case])
    if kw.get("nb") == -1:
        kw["nb"] = ln.nb - 1
    assert ln.run(**kw) != 0, case
    assert lib.zmi_last_error(), case
    assert ln.unchanged(snap), case
