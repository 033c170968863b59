"""zmi_mamba2_scan_cont: the Mamba2 prefill scan from a carried state (bf16 SSM state + conv ring of a state row), on the
cases of tests/mamba_cont_cases.py, under ZMI_OPT_SCAN_PQ 0 (SSD up to 256 positions, the 4-workgroup recurrence past
it) and 4.

Every link of a chain and every crafted start is held to tests/mamba_cases.ref64 started from the state and ring the
library stored, under that module's criterion (E = 2^-14, elementwise, y and state); ring bits must be equal; in the conv
case y is the conv output bit for bit. A ragged call equals each of its sequences alone bit for bit, its pos0 = 0
sequences equal zmi_mamba2_scan_seqs, and rows / state rows the table does not list keep their sentinels. The full-width
launch (64 heads, 8 continuing sequences of 256 positions) is the one in which a ring, state or LDS race between the
workgroups or waves of a launch would show: it is held to ref64 too. Every test prints max(error / bound) per head regime.

Measured on an MI355X, max(error / bound) of y / of the state (1.0 is the criterion, ~0.98 a result that differs from
fp64 by its own bf16 rounding alone), the same under ZMI_OPT_SCAN_PQ 0 and 4 to the third digit:

                     chains         crafted starts
    ordinary       0.964/0.984       0.981/0.985
    slow           0.984/0.984       0.982/0.984
    fast           0.965/0.985       0.968/0.985
    threshold      0.969/0.984       0.983/0.985
    reset          0.977/0.984       0.977/0.985
    reset130       0.977/0.983       0.980/0.983
    tails_*        0.984/0.984       0.983/0.986
    cancel_a/b/c   0.941/0.983       0.983/0.985
    conv_*         0.000/0.000 everywhere: y is the conv output bit for bit, the state stays 0
and in the full-width launch (64 heads, 256 positions): ordinary 0.981/0.983, slow 0.984/0.983, fast 0.964/0.984,
threshold 0.979/0.985, reset 0.984/0.981, reset130 0.982/0.982.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import mamba_cases as mc
from tests import mamba_cont_cases as cc
from tests.mamba_cases import CASES, D_SSM, DS, HD, MD, NH
from tests.test_gpu_hybrid import _args
from zonos_vibes_amd.config import zonos_v01_hybrid

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -77.0  # exact in bf16
STALE_SSM = 3.0
BF = torch.bfloat16
PQS = [0, 4]


def _L():
    from zonos_vibes_amd import _lib
    return _lib, _lib.lib()


def _with_option(pq, fn):
    L, lib = _L()
    old = lib.zmi_get_option(L.OPT_SCAN_PQ)
    lib.zmi_set_option(L.OPT_SCAN_PQ, pq)
    try:
        return fn()
    finally:
        lib.zmi_set_option(L.OPT_SCAN_PQ, old)


class Launch:
    """Buffers of one call: sentinels in y, the given (or stale) state rows and rings, a stale workspace."""

    def __init__(self, md, params, rows, ssm0, ring0, n_seq):
        L, lib = _L()
        m = rows.shape[0]
        self.md, self.m = md, m
        self.pd = [t.to(DEV) for t in params]
        self.zx = rows.to(DEV).contiguous()
        self.ring, self.ssm = ring0.clone().to(DEV), ssm0.clone().to(DEV)
        self.y = torch.full((m, md["d_ssm"]), SENT, dtype=BF, device=DEV)
        self.rp = torch.zeros(m, dtype=torch.int32, device=DEV)
        self.nb = int(lib.zmi_mamba2_scan_cont_ws_bytes(m, md["d_ssm"], md["nheads"], n_seq))
        self.nb_seqs = int(lib.zmi_mamba2_scan_ws_bytes(m, md["d_ssm"], md["nheads"]))
        self.ws = torch.full((max(self.nb, 1),), 0xA5, dtype=torch.uint8, device=DEV)
        self.a = _args(L, md, self.zx, *self.pd, self.ring, self.ssm, self.y, m, self.rp)

    def run(self, seqs, pq, fn="zmi_mamba2_scan_cont"):
        L, lib = _L()
        sa = np.ascontiguousarray(np.asarray(seqs, dtype=np.int32).reshape(-1, 4))
        dev = torch.from_numpy(sa.ravel().copy()).to(DEV)
        nb = self.nb if fn == "zmi_mamba2_scan_cont" else self.nb_seqs
        L.check(_with_option(pq, lambda: getattr(lib, fn)(ctypes.byref(self.a), dev.data_ptr(), len(sa),
                                                          sa.ctypes.data, self.ws.data_ptr(), nb, 0)), fn)
        torch.cuda.synchronize()


def _stale(n_kv, md=MD):
    return (torch.full((n_kv, md["nheads"], HD, DS), STALE_SSM, dtype=BF),
            torch.full((n_kv, 4, md["conv_dim"]), mc.STALE_RING, dtype=BF))


def _judge(tag, case, y, state, ring, ref, worst):
    wy = mc.head_max(mc.ratio(y.cpu(), ref.y64, ref.y_abs))
    ws = mc.head_max(mc.ratio(state.cpu(), ref.state64, ref.state_abs))
    heads = CASES[case][0]
    print(f"{tag}: " + ", ".join(f"{h} y {a:.3f} state {b:.3f}" for h, a, b in zip(heads, wy, ws)))
    bad = []
    for h, a, b in zip(heads, wy, ws):
        w = worst.setdefault(h, [0.0, 0.0])
        w[0], w[1] = max(w[0], a), max(w[1], b)
        if not (a <= 1.0 and b <= 1.0):
            bad.append((tag, h, a, b))
    if not torch.equal(ring.cpu(), ref.ring):
        bad.append((tag, "ring"))
    if case == "conv" and not torch.equal(y.cpu(), ref.xc[:, :D_SSM]):
        bad.append((tag, "y is not the conv output bit for bit"))
    return bad


def _show(worst):
    print("max(error / bound) y / state: " + ", ".join(f"{h} {a:.3f}/{b:.3f}" for h, (a, b) in worst.items()))


# ---------------------------------------------------------------------------------------------- chains
@pytest.mark.parametrize("pq", PQS)
@pytest.mark.parametrize("case", list(CASES))
def test_chains(case, pq):
    """Each chain's links one call each on state row 1 of 3; the reference of a link starts from the bf16 state and the
    ring the library left (the half ulp of a stored state is far above E of the next y, so a reference carried on
    roundings of its own could not be compared)."""
    bad, worst = [], {}
    for cuts in cc.CHAINS:
        inp = mc.build(case, cuts[-1])
        ssm, ring = _stale(3)
        for a, b in cc.links(cuts):
            ln = Launch(MD, inp.params, inp.zx[a:b], ssm, ring, 1)
            ln.run([(0, b - a, 1, a)], pq)
            ref = cc.link_ref(inp, a, b, ssm[1], ring[1])
            bad += _judge(f"pq{pq} {case} chain {cuts[-1]} [{a},{b})", case, ln.y, ln.ssm[1], ln.ring[1], ref, worst)
            ssm, ring = ln.ssm.cpu(), ln.ring.cpu()
            for k in (0, 2):
                assert (ssm[k] == STALE_SSM).all() and (ring[k] == mc.STALE_RING).all()
    _show(worst)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- crafted starts
def _start_table(case):
    """The ragged table of the crafted starts plus one pos0 = 0 sequence of 33 positions: rows not in table order with
    sentinel rows between, state rows a permutation with holes."""
    probes = [cc.start_probe(case, p, n) for p, n in cc.STARTS]
    entries = [(i.zx, st, rg, p) for (i, st, rg), (p, _) in zip(probes, cc.STARTS)]
    zero = mc.build(case, 33)
    entries.insert(7, (zero.zx, None, None, 0))
    ns = len(entries)
    n_kv = ns + 3
    kvs = [(7 * s + 2) % n_kv for s in range(ns)]  # 7 and n_kv = 34 are coprime: distinct rows
    order = sorted(range(ns), key=lambda s: (s * 11) % ns)
    q0, row, free = [0] * ns, 0, []
    for k, s in enumerate(order):
        gap = 1 if k % 5 == 0 else 0
        free += list(range(row, row + gap))
        q0[s] = row + gap
        row += gap + entries[s][0].shape[0]
    free.append(row)
    m = row + 1
    rows = torch.full((m, MD["d_in_proj"]), SENT, dtype=BF)
    ssm, ring = _stale(n_kv)
    for s, (zx, st, rg, _) in enumerate(entries):
        rows[q0[s]:q0[s] + zx.shape[0]] = zx
        if st is not None:
            ssm[kvs[s]], ring[kvs[s]] = st, rg
    seqs = [(q0[s], entries[s][0].shape[0], kvs[s], entries[s][3]) for s in range(ns)]
    return probes[0][0].params, entries, rows, ssm, ring, seqs, free, n_kv


@pytest.mark.parametrize("pq", PQS)
@pytest.mark.parametrize("case", list(CASES))
def test_crafted_starts_ragged(case, pq):
    params, entries, rows, ssm, ring, seqs, free, n_kv = _start_table(case)
    ln = Launch(MD, params, rows, ssm, ring, len(seqs))
    ln.run(seqs, pq)
    bad, worst = [], {}
    for (q, n, kv, p0), (zx, st, rg, _) in zip(seqs, entries):
        ref = mc.ref64(zx, *params, MD, state0=st, ring0=rg, pos0=p0)
        bad += _judge(f"pq{pq} {case} pos0={p0} len={n}", case, ln.y[q:q + n], ln.ssm[kv], ln.ring[kv], ref, worst)
        # the call on this sequence alone (its own buffers, state row 0): bit for bit
        one = Launch(MD, params, zx, (ssm[kv] if st is not None else _stale(1)[0][0])[None],
                     (ring[kv] if rg is not None else _stale(1)[1][0])[None], 1)
        one.run([(0, n, 0, p0)], pq)
        same = (torch.equal(one.y, ln.y[q:q + n]) and torch.equal(one.ssm[0], ln.ssm[kv])
                and torch.equal(one.ring[0], ln.ring[kv]))
        if not same:
            bad.append((case, p0, n, "ragged differs from the sequence alone"))
        if p0 == 0:  # a starting sequence: zmi_mamba2_scan_seqs's bits, stale state and ring unread
            ref0 = Launch(MD, params, zx, *[t[:1] for t in _stale(1)], 1)
            ref0.run([(0, n, 0, 0)], pq, "zmi_mamba2_scan_seqs")
            if not (torch.equal(ref0.y, one.y) and torch.equal(ref0.ssm, one.ssm) and torch.equal(ref0.ring, one.ring)):
                bad.append((case, "pos0 = 0 differs from zmi_mamba2_scan_seqs"))
    _show(worst)
    assert not bad, bad
    assert (ln.y[free] == SENT).all()
    for kv in sorted(set(range(n_kv)) - {s[2] for s in seqs}):
        assert (ln.ssm[kv] == STALE_SSM).all() and (ln.ring[kv] == mc.STALE_RING).all(), kv
    assert torch.equal(ln.zx.cpu(), rows)


# ---------------------------------------------------------------------------------------------- full width
@pytest.mark.parametrize("pq", PQS)
@pytest.mark.parametrize("case", ["mix", "dt"])
def test_full_width_continuing_sequences(case, pq):
    """64 heads, d_ssm 4096: 8 continuing sequences of 256 positions in one launch (1,024 SSD workgroups of 8 row blocks
    each under PQ 0; 2,048 conv workgroups of which 24 read a ring that the same call rewrites). The 3 regimes of the case
    are repeated over the 64 heads (mamba_cont_cases.widen), so every head is judged against ref64 under the criterion
    (a race on a ring, a state row or an LDS tile gives wrong values, not only unequal ones), the heads of one regime
    must agree bit for bit, and the launch equals each sequence alone."""
    md = zonos_v01_hybrid().backbone.mamba2_dims()
    nh = md["nheads"]
    assert (nh, md["d_ssm"]) == (64, 4096)
    T, ns = cc.WIDE_LEN, len(cc.WIDE_POS0)
    kv = [5, 0, 9, 2, 7, 3, 8, 1]
    probes = [cc.start_probe(case, p0, T) for p0 in cc.WIDE_POS0]
    wide = [cc.widen(i, st, rg, nh) for i, st, rg in probes]
    params = wide[0][1]
    rows = torch.cat([w[0] for w in wide])
    assert rows.shape == (ns * T, md["d_in_proj"])
    ssm, ring = _stale(10, md)
    for s in range(ns):
        ssm[kv[s]], ring[kv[s]] = wide[s][2], wide[s][3]
    seqs = [(s * T, T, kv[s], cc.WIDE_POS0[s]) for s in range(ns)]
    ln = Launch(md, params, rows, ssm, ring, ns)
    ln.run(seqs, pq)
    bad, worst = [], {}
    groups = [list(range(g, g + NH)) for g in range(0, nh - NH + 1, NH)]  # heads 3g .. 3g + 2: the reference's layout
    for (q, n, k, p0), (i, st, rg) in zip(seqs, probes):
        ref = mc.ref64(i.zx, *i.params, MD, state0=st, ring0=rg, pos0=p0)
        y, state, rg_out = ln.y[q:q + n].cpu(), ln.ssm[k].cpu(), ln.ring[k].cpu()
        first = slice(0, D_SSM)
        ring3 = torch.cat([rg_out[:, first], rg_out[:, md["d_ssm"]:]], dim=1)
        bad += _judge(f"pq{pq} {case} wide pos0={p0}", case, y[:, first], state[:NH], ring3, ref, worst)
        for g in groups[1:] + [[nh - 1]]:  # every other head: the bits of its regime's first head
            cols = slice(g[0] * HD, (g[-1] + 1) * HD)
            w = len(g) * HD
            if not (torch.equal(y[:, cols], y[:, :w]) and torch.equal(state[g[0]:g[-1] + 1], state[:len(g)])
                    and torch.equal(rg_out[:, cols], rg_out[:, :w])):
                bad.append((case, p0, "heads of one regime differ", g))
        one = Launch(md, params, rows[q:q + n], ssm[k][None], ring[k][None], 1)
        one.run([(0, n, 0, p0)], pq)
        if not (torch.equal(one.y, ln.y[q:q + n]) and torch.equal(one.ssm[0], ln.ssm[k])
                and torch.equal(one.ring[0], ln.ring[k])):
            bad.append((case, p0, "the launch differs from the sequence alone"))
    _show(worst)
    assert not bad, bad
    for k in (4, 6):
        assert (ln.ssm[k] == STALE_SSM).all() and (ln.ring[k] == mc.STALE_RING).all()
