"""Cases of the continued Mamba2 scan (zmi_mamba2_scan_cont), shared by tests/test_mamba_cont_cpu.py and
tests/test_gpu_mamba_cont.py. Geometry, regimes, the fp64 reference and the criterion are tests/mamba_cases.py's.

CHAINS   one build(case, total) sequence cut into links; link k runs positions cuts[k] .. cuts[k + 1] - 1 from the
         state and ring link k - 1 left. The continuing links are 1, 2, 3, 4, 32, 256 and 257 positions long, at
         aligned and odd pos0, on both sides of the SSD form's reach (256). The raw inputs of a link's conv history are
         the sequence's own rows, so the input-safety condition of build() covers every link.
WIDE     the full-width launch (64 heads): 8 crafted starts of 256 positions whose 3 regimes are repeated over the 64
         heads (head h runs regime h % 3; B and C are shared by the heads anyway), so ref64 at 3 heads is the reference
         of every head of the wide launch, and heads of one regime must agree bit for bit.
STARTS   crafted starts: pos0 in START_POS0 x len in START_LEN, each from step_state(case, seed) and a ring that holds
         STALE_RING in every slot no position has written (pos0 of 1 or 2 leaves slots of positions below 0 stale).
"""
from __future__ import annotations

import torch

from tests import mamba_cases as mc
from tests.mamba_cases import BF, CD, D_SSM, DS, HD, NH

CHAINS = ((0, 33, 34, 36, 40, 296, 553), (0, 4, 5, 7, 10, 266), (0, 256, 513, 545))
START_POS0 = (1, 2, 3, 5, 530)
START_LEN = (1, 2, 3, 4, 5, 33)
STARTS = tuple((p, n) for p in START_POS0 for n in START_LEN)


def links(cuts):
    return list(zip(cuts[:-1], cuts[1:]))


def start_probe(case, pos0, T):
    """-> (Inputs of the T rows at positions pos0 .. pos0 + T - 1, state0, ring0): the min(pos0, 3) positions before
    them exist only as ring slots."""
    n = min(pos0, 3)
    seed = 1000 * pos0 + T
    i = mc.build(case, n + T, pos0 - n, seed=seed)
    ring0 = torch.full((4, CD), mc.STALE_RING, dtype=BF)
    for k in range(n):
        ring0[(pos0 - n + k) & 3] = i.zx[k, D_SSM:D_SSM + CD]
    return mc.Inputs(case, i.zx[n:], *i.params), mc.step_state(case, seed), ring0


def link_ref(inp, a, b, state0, ring0):
    """ref64 of rows a .. b - 1 of a chain's sequence from (state0, ring0) at position a (a == 0: from empty)."""
    if a == 0:
        return mc.ref64(inp.zx[:b], *inp.params, mc.MD)
    return mc.ref64(inp.zx[a:b], *inp.params, mc.MD, state0=state0, ring0=ring0, pos0=a)


WIDE_POS0 = (256, 257, 1, 2, 3, 300, 512, 77)
WIDE_LEN = 256


def _tile_heads(t, nheads, dim):
    """A tensor whose `dim` holds NH head blocks (of any block size) -> the same with nheads blocks, head h = h % NH."""
    blk = t.shape[dim] // NH
    parts = t.split(blk, dim)
    return torch.cat([parts[h % NH] for h in range(nheads)], dim)


def widen(inp, state0, ring0, nheads):
    """The 3-head problem (Inputs, state [3, 64, 128], ring [4, 448]) over nheads heads -> (zx [T, 2 d + 256 + nheads],
    (cw, cb, dtb, A, D), state [nheads, 64, 128], ring [4, d + 256]) with d = 64 nheads."""
    def xbc(t, dim):  # x channels tiled, B / C copied
        x, bc = t.split([D_SSM, 2 * DS], dim)
        return torch.cat([_tile_heads(x, nheads, dim), bc], dim)
    z, rest = inp.zx[:, :D_SSM], inp.zx[:, D_SSM:]
    raw, dt = rest[:, :CD], rest[:, CD:]
    zx = torch.cat([_tile_heads(z, nheads, 1), xbc(raw, 1), _tile_heads(dt, nheads, 1)], 1).contiguous()
    params = (xbc(inp.cw, 0).contiguous(), xbc(inp.cb, 0).contiguous(), _tile_heads(inp.dtb, nheads, 0).contiguous(),
              _tile_heads(inp.A, nheads, 0).contiguous(), _tile_heads(inp.D, nheads, 0).contiguous())
    return zx, params, _tile_heads(state0, nheads, 0).contiguous(), xbc(ring0, 1).contiguous()
