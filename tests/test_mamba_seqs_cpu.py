"""zmi_mamba2_scan_seqs's host checks without a GPU: the table is validated before anything is launched, so a
refused call (and one with nothing to do) never touches its buffers; the pointers here are never dereferenced."""
import ctypes

import numpy as np
import pytest

from zonos_vibes_amd.config import tiny_hybrid

M = 12


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
    nb = int(lib.zmi_mamba2_scan_ws_bytes(m, md["d_ssm"], md["nheads"]))
    rc = lib.zmi_mamba2_scan_seqs(ctypes.byref(a), fake, len(sa) if n_seq is None else n_seq, sa.ctypes.data, fake,
                                  nb if ws_bytes is None else nb + ws_bytes, None)
    return rc, lib.zmi_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(seqs=[(0, 4, 0, 0)], n_seq=-1), b"n_seq"),
    (dict(seqs=[(0, -1, 0, 0)]), b"negative"),
    (dict(seqs=[(-1, 4, 0, 0)]), b"negative"),
    (dict(seqs=[(0, 4, 0, 0), (9, 4, 1, 0)]), b"past M"),
    (dict(seqs=[(0, 2 ** 31 - 1, 0, 0)]), b"past M"),
    (dict(seqs=[(0, 4, 0, 1)]), b"pos0"),
    (dict(seqs=[(0, 4, -1, 0)]), b"kv_row"),
    (dict(seqs=[(0, 5, 0, 0), (8, 2, 2, 0), (4, 4, 1, 0)]), b"share rows"),
    (dict(seqs=[(0, 4, 1, 0), (8, 2, 0, 0), (4, 4, 1, 0)]), b"share a kv_row"),
    (dict(seqs=[(0, 4, 0, 0)], ws_bytes=-1), b"workspace"),
])
def test_refused_on_the_host(kw, word):
    rc, msg = _call(**kw)
    assert rc != 0 and word in msg, (rc, msg)


def test_nothing_to_do_returns_zero():
    assert _call([], n_seq=0)[0] == 0
    # empty sequences may sit anywhere inside M, share rows with live ones' neighbours and repeat a kv_row
    assert _call([(0, 0, 0, 0), (5, 0, 0, 0), (M, 0, 2, 0)])[0] == 0
