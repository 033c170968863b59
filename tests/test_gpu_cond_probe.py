"""zmi_prefix_condition through the C ABI on the crafted launches of tests/cond_cases.py (MI355X only): all five row
kinds mixed in one launch at the widths where the ownership j = t + 256 i changes, against the exact restatement of the
pre-LayerNorm row and the fp64 LayerNorm; each row alone against its bits in the mixed launch; guard rows around the
output; and every refused argument form, which must leave the output untouched.

Measured on an MI355X, per width the worst |got - ref| / ulp against the unrounded fp64 reference (0.5 is a correct
rounding) and the lowest bit-identical share against the rounded one, over eps 1e-5 and 1e-3:
  d 2: 0.4998, 1.00000    d 8: 0.5000, 1.00000     d 254: 0.5000, 1.00000   d 256: 0.5015, 0.99964
  d 258: 0.5005, 0.99982  d 510: 0.4999, 1.00000   d 1026: 0.5073, 0.99973  d 2048: 0.5035, 0.99987
  d 4094: 0.5037, 0.99988 d 4096: 0.5116, 0.99983
The thresholds are those of the criterion (1 ulp, 98 %), not these figures.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import cond_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = cc.GUARD_ROWS
GUARD = -7.0  # bf16 value of the guard fill


def _lib():
    from zonos_vibes_amd import _lib as L
    return L


@functools.lru_cache(maxsize=None)
def _launch(d, eps):
    return cc.launch(d, eps)


class Device:
    """The device copy of a Launch: parameter tensors (kept alive here), the CondParam block, x and the LayerNorm
    parameters. The row table and the guard-filled output are made per call."""

    def __init__(self, L: cc.Launch):
        lib = _lib()
        self.L, self.keep = L, []
        arr = (lib.CondParam * len(L.params))()
        for cp, p in zip(arr, L.params):
            for name in ("table", "weight", "bias"):
                a = getattr(p, name)
                if a is not None:
                    t = cc.to_torch_bf16(a).contiguous().to(DEV)
                    self.keep.append(t)
                    setattr(cp, name, t.data_ptr())
            cp.in_dim, cp.min_val, cp.max_val = p.in_dim, p.min_val, p.max_val
        self.params = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
        self.x = torch.from_numpy(L.x.copy()).to(DEV)
        self.ln_w = cc.to_torch_bf16(L.ln_w).to(DEV)
        self.ln_b = cc.to_torch_bf16(L.ln_b).to(DEV)

    def out_buffer(self, n_rows, d=None):
        return torch.full((n_rows + 2 * G, d or self.L.d), GUARD, dtype=torch.bfloat16, device=DEV)

    def call(self, rows, out, d=None, null=(), n_rows=None):
        """-> status. `null`: argument names passed as NULL; the output starts G guard rows into `out`."""
        lib, d = _lib(), self.L.d if d is None else d
        r = torch.tensor(rows if rows else [(0, 0, 0, 0)], dtype=torch.int32).to(DEV)
        a = dict(params=self.params.data_ptr(), rows=r.data_ptr(), x=self.x.data_ptr(), ln_w=self.ln_w.data_ptr(),
                 ln_b=self.ln_b.data_ptr(), out=out.data_ptr() + 2 * G * d)
        for k in null:
            a[k] = None
        rc = lib.lib().zmi_prefix_condition(a["params"], a["rows"], len(rows) if n_rows is None else n_rows, a["x"], d,
                                            a["ln_w"], a["ln_b"], self.L.eps, a["out"],
                                            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def run(self, rows):
        out = self.out_buffer(len(rows))
        _lib().check(self.call(rows, out), "prefix_condition")
        host = out.cpu()
        assert bool((host[:G] == GUARD).all()) and bool((host[G + len(rows):] == GUARD).all()), "guard rows written"
        return cc.from_torch_bf16(host[G:G + len(rows)])


def _untouched(out):
    return bool((out == GUARD).all().item())


@pytest.mark.parametrize("d", cc.WIDTHS)
def test_mixed_launch_matches_fp64(d):
    """All five kinds in one permuted launch, eps 1e-5 and 1e-3: the criterion of cond_cases.check (one bf16 ulp of the
    fp64 LayerNorm of the exact v, floor 2^-20; 98 % bit-identical; zero-variance rows equal to ln_b), then every row
    launched alone equals its bits in the mixed launch."""
    for eps in cc.EPS:
        L = _launch(d, eps)
        dev = Device(L)
        got = dev.run(L.rows)
        fig = cc.judge(got, L)
        print(f"d {d} eps {eps}: worst |got - ref| / ulp {fig['worst']:.4f}, bit-identical {fig['same']:.5f}")
        pre = cc.all_v(L)
        # the pre-LayerNorm row is exact, so a wrong row shows at full scale; name the kind before the criterion does
        ref = cc.reference(L, pre)
        per_row = (np.abs(got - ref) / cc.bf16_ulp(np.maximum(np.abs(ref), np.abs(got)))).max(axis=1)
        assert per_row.max() <= 1.0, [(L.tags[r], float(per_row[r])) for r in np.nonzero(per_row > 1.0)[0]]
        cc.check(got, L)
        for r in range(len(L.rows)):
            alone = dev.run([L.rows[r]])
            assert np.array_equal(cc.bits(alone[0]), cc.bits(got[r])), (d, eps, L.tags[r])


def test_no_rows_writes_nothing():
    dev = Device(_launch(8, 1e-5))
    out = dev.out_buffer(4)
    assert dev.call([], out) == 0
    assert _untouched(out)


@pytest.mark.parametrize("d", cc.REFUSED_WIDTHS)
def test_refused_widths_leave_the_output_untouched(d):
    L = _launch(8, 1e-5)
    dev = Device(L)
    out = dev.out_buffer(len(L.rows), 4098)
    assert dev.call(L.rows, out, d=d) != 0
    assert b"prefix_condition" in _lib().lib().zmi_last_error()
    assert _untouched(out)


@pytest.mark.parametrize("null", ["params", "rows", "x", "ln_w", "ln_b", "out", "n_rows"])
def test_refused_arguments_leave_the_output_untouched(null):
    """A NULL pointer with n_rows > 0, and a negative n_rows: a nonzero status before any launch."""
    L = _launch(8, 1e-5)
    dev = Device(L)
    out = dev.out_buffer(len(L.rows))
    if null == "n_rows":
        rc = dev.call(L.rows, out, n_rows=-1)
    else:
        rc = dev.call(L.rows, out, null=(null,))
    assert rc != 0
    assert b"prefix_condition" in _lib().lib().zmi_last_error()
    assert _untouched(out)
    # NULL pointers with no rows are nothing to refuse
    assert dev.call([], out, null=("params", "rows", "x", "ln_w", "ln_b", "out")) == 0
