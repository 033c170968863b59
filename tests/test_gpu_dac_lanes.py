"""The zmi_dac_*_lanes entry points against that many calls of the single-utterance entry points, bit for bit.

Every lane has random data of its own and the lane strides are exactly dense, so a read past a lane's first or last
row would land in its neighbour's real data (not in slack) and change the bits. Outputs sit between canary rows
(tests/test_gpu_dac_kernels.Buf) and every launch runs under every form of dac_cases.FORMS: the tile choice counts
the lanes, so a lanes launch may take another tile than the single one, and must still give its bits."""
import math

import pytest
import torch

from tests import dac_cases as dc
from tests.test_gpu_dac_kernels import Buf, forms
from zonos_vibes_amd.autoencoder import pack_conv, pack_conv_out, pack_conv_transpose

pytestmark = pytest.mark.gpu
DEV = "cuda"
LANES = (1, 2, 3)
CONV_SHAPES = ((32, 32, 7, 1), (64, 96, 7, 3), (32, 64, 7, 11), (64, 64, 1, 0))  # c_in, c_out, taps, dilation
CONV_LENGTHS = (1, 17, 129, 257)
CONV_T_SHAPES = ((64, 32, 2, 1), (64, 64, 8, 4))  # c_in, c_out, stride, pad
CONV_T_LENGTHS = (1, 16, 33)
EPI = ("skip", "raw", "snake", "f32")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same_as_singles(batch: Buf, singles, rows: int):
    """Lane l of the dense batched output equals the l-th single launch's output; all canaries hold."""
    assert batch.guards_intact() and all(s.guards_intact() for s in singles)
    for lane, s in enumerate(singles):
        assert torch.equal(batch.full[batch.guard + lane * rows: batch.guard + (lane + 1) * rows],
                           s.full[s.guard: s.guard + rows]), lane


# ------------------------------------------------------------------------------------------------ zmi_dac_conv_lanes
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=str)
def test_conv_lanes(gpu_lib, shape):
    c_in, c_out, taps, dil = shape
    in_off = -dil * (taps - 1) // 2
    types = dict(raw=torch.float16, snake=torch.float16, f32=torch.float32)
    with forms(gpu_lib) as f:
        for T in CONV_LENGTHS:
            cs = [dc.conv_inputs(c_in, c_out, taps, T, T, dil, 900 + lane) for lane in range(max(LANES))]
            w = pack_conv(cs[0]["w"]).to(DEV)  # weights, bias and alpha are shared: lane 0's
            bias, alpha = cs[0]["bias"].float().to(DEV), cs[0]["alpha"].float().to(DEV)
            x = torch.stack([c["x"].half() for c in cs]).to(DEV)        # [L][T][c_in] dense
            skip = torch.stack([c["skip"].half() for c in cs]).to(DEV)  # [L][T][c_out] dense
            for L in LANES:
                def launch():
                    outs = {n: Buf(L * T, c_out, t) for n, t in types.items()}
                    rc = gpu_lib.zmi_dac_conv_lanes(
                        x.data_ptr(), T, c_in, w.data_ptr(), bias.data_ptr(), c_out, taps, dil, in_off, T, 1, 0, T,
                        skip.data_ptr(), outs["raw"].ptr(), outs["snake"].ptr(), alpha.data_ptr(), outs["f32"].ptr(),
                        L, T * c_in, T * c_out, T * c_out, T * c_out, T * c_out, _stream())
                    assert rc == 0, gpu_lib.zmi_last_error()
                    for lane in range(L):
                        for n, t in types.items():
                            outs[f"{n}{lane}"] = Buf(T, c_out, t)
                        rc = gpu_lib.zmi_dac_conv(
                            x[lane].data_ptr(), T, c_in, w.data_ptr(), bias.data_ptr(), c_out, taps, dil, in_off, T, 1,
                            0, T, skip[lane].data_ptr(), outs[f"raw{lane}"].ptr(), outs[f"snake{lane}"].ptr(),
                            alpha.data_ptr(), outs[f"f32{lane}"].ptr(), _stream())
                        assert rc == 0, gpu_lib.zmi_last_error()
                    return outs
                outs = f.run(launch)
                for n in types:
                    _same_as_singles(outs[n], [outs[f"{n}{lane}"] for lane in range(L)], T)
                if L > 1 and T > 1:  # the lanes' data differ: equal outputs would mean a lane read another's rows
                    assert not torch.equal(outs["f320"].mid, outs["f321"].mid)


# ------------------------------------------------------------------------------------------------ zmi_dac_conv_t_lanes
@pytest.mark.parametrize("shape", CONV_T_SHAPES, ids=str)
def test_conv_t_lanes(gpu_lib, shape):
    c_in, c_out, stride, pad = shape
    with forms(gpu_lib) as f:
        for T in CONV_T_LENGTHS:
            cs = [dc.conv_t_inputs(c_in, c_out, stride, T, pad, 900 + lane) for lane in range(max(LANES))]
            w = pack_conv_transpose(cs[0]["w"], stride, pad).to(DEV)
            bias, alpha = cs[0]["bias"].float().to(DEV), cs[0]["alpha"].float().to(DEV)
            x = torch.stack([c["x"].half() for c in cs]).to(DEV)
            to = stride * T
            for L in LANES:
                def launch():
                    outs = {n: Buf(L * to, c_out, torch.float16) for n in ("raw", "snake")}
                    rc = gpu_lib.zmi_dac_conv_t_lanes(x.data_ptr(), T, c_in, w.data_ptr(), bias.data_ptr(), c_out,
                                                      stride, pad, outs["raw"].ptr(), outs["snake"].ptr(),
                                                      alpha.data_ptr(), L, T * c_in, to * c_out, to * c_out, _stream())
                    assert rc == 0, gpu_lib.zmi_last_error()
                    for lane in range(L):
                        outs[f"raw{lane}"], outs[f"snake{lane}"] = (Buf(to, c_out, torch.float16) for _ in range(2))
                        rc = gpu_lib.zmi_dac_conv_t(x[lane].data_ptr(), T, c_in, w.data_ptr(), bias.data_ptr(), c_out,
                                                    stride, pad, outs[f"raw{lane}"].ptr(), outs[f"snake{lane}"].ptr(),
                                                    alpha.data_ptr(), _stream())
                        assert rc == 0, gpu_lib.zmi_last_error()
                    return outs
                outs = f.run(launch)
                for n in ("raw", "snake"):
                    _same_as_singles(outs[n], [outs[f"{n}{lane}"] for lane in range(L)], to)


# ------------------------------------------------------------------------------------------------ conv_out_range_lanes
def test_conv_out_range_lanes(gpu_lib):
    c_in, t = 96, 257
    cs = [dc.conv_inputs(c_in, 1, 7, t, 1, 2, 900 + lane) for lane in range(max(LANES))]
    w, b = (v.to(DEV) for v in pack_conv_out(cs[0]["w"], cs[0]["bias"]))
    x = torch.stack([c["x"].half() for c in cs]).to(DEV)
    with forms(gpu_lib) as f:
        for q0, n in ((0, 257), (5, 128), (250, 7)):
            for L in LANES:
                def launch():
                    outs = dict(out=Buf(L * n, 1, torch.float32))
                    rc = gpu_lib.zmi_dac_conv_out_range_lanes(x.data_ptr(), t, c_in, w.data_ptr(), b.data_ptr(), q0, n,
                                                              outs["out"].ptr(), L, t * c_in, n, _stream())
                    assert rc == 0, gpu_lib.zmi_last_error()
                    for lane in range(L):
                        outs[f"out{lane}"] = Buf(n, 1, torch.float32)
                        rc = gpu_lib.zmi_dac_conv_out_range(x[lane].data_ptr(), t, c_in, w.data_ptr(), b.data_ptr(),
                                                            q0, n, outs[f"out{lane}"].ptr(), _stream())
                        assert rc == 0, gpu_lib.zmi_last_error()
                    return outs
                outs = f.run(launch)
                _same_as_singles(outs["out"], [outs[f"out{lane}"] for lane in range(L)], n)


# ------------------------------------------------------------------------------------------------ from_codes_lanes
@pytest.mark.parametrize("T", (1, 37))
def test_from_codes_lanes(gpu_lib, T):
    g = torch.Generator().manual_seed(40 + T)
    cb = dc.f16_values((9, 1024, 8), g).float().to(DEV)
    pw = dc.f16_values((9, 1024, 8), g, 1 / math.sqrt(8)).float().to(DEV)
    pb = dc.f16_values((9, 1024), g, 0.1).float().to(DEV)
    codes = torch.randint(0, 1024, (max(LANES), 9, T), generator=g).to(DEV)  # [L][9][T] dense
    for L in LANES:
        z = Buf(L * T, 1024, torch.float16)
        rc = gpu_lib.zmi_dac_from_codes_lanes(codes.data_ptr(), T, cb.data_ptr(), pw.data_ptr(), pb.data_ptr(), z.ptr(),
                                              L, 9 * T, 1024 * T, _stream())
        assert rc == 0, gpu_lib.zmi_last_error()
        singles = []
        for lane in range(L):
            singles.append(Buf(T, 1024, torch.float16))
            rc = gpu_lib.zmi_dac_from_codes(codes[lane].data_ptr(), T, cb.data_ptr(), pw.data_ptr(), pb.data_ptr(),
                                            singles[-1].ptr(), _stream())
            assert rc == 0, gpu_lib.zmi_last_error()
        torch.cuda.synchronize()
        _same_as_singles(z, singles, T)
        if L > 1:
            assert not torch.equal(singles[0].mid, singles[1].mid)


# ------------------------------------------------------------------------------------------------ rejected arguments
def test_lanes_rejected_arguments(gpu_lib):
    """lanes < 1, a lane stride below a lane's extent (lanes > 1) and lanes * phases > 65535 are errors with a
    message; none of them launches anything."""
    T, c = 20, 64
    cv = dc.conv_inputs(c, c, 7, T, T, 1)
    x = torch.stack([cv["x"].half()] * 2).to(DEV)
    skip = torch.stack([cv["skip"].half()] * 2).to(DEV)
    w = pack_conv(cv["w"]).to(DEV)
    bias, alpha = cv["bias"].float().to(DEV), cv["alpha"].float().to(DEV)
    dense = dict(ls_x=T * c, ls_skip=T * c, ls_raw=T * c, ls_snake=T * c, ls_f32=T * c)

    def conv(lanes, **kw):
        a = dict(dense, **kw)
        outs = [Buf(2 * T, c, t) for t in (torch.float16, torch.float16, torch.float32)]
        rc = gpu_lib.zmi_dac_conv_lanes(x.data_ptr(), T, c, w.data_ptr(), bias.data_ptr(), c, 7, 1, -3, T, 1, 0, T,
                                        skip.data_ptr(), outs[0].ptr(), outs[1].ptr(), alpha.data_ptr(), outs[2].ptr(),
                                        lanes, a["ls_x"], a["ls_skip"], a["ls_raw"], a["ls_snake"], a["ls_f32"],
                                        _stream())
        torch.cuda.synchronize()
        return rc, outs

    rc, outs = conv(2)
    assert rc == 0 and not any(b.untouched() for b in outs)
    for lanes, kw in ((0, {}), (-3, {}), (65536, {})) + tuple((2, {k: T * c - 1}) for k in dense) + \
            ((2, dict(ls_raw=-T * c)), (2, dict(ls_x=0))):
        rc, outs = conv(lanes, **kw)
        assert rc != 0 and gpu_lib.zmi_last_error().decode().startswith("dac_conv: "), (lanes, kw)
        assert all(b.untouched() for b in outs), (lanes, kw)
    rc, outs = conv(1, ls_x=0, ls_skip=0, ls_raw=0, ls_snake=0, ls_f32=0)  # one lane: the strides are not read
    assert rc == 0

    # conv_t: grid z = lanes * stride
    ct = dc.conv_t_inputs(c, c, 8, T, 4)
    wt = pack_conv_transpose(ct["w"], 8, 4).to(DEV)
    xt = torch.stack([ct["x"].half()] * 2).to(DEV)
    for lanes, ls in ((0, (T * c, 8 * T * c, 8 * T * c)), (8192, (T * c, 8 * T * c, 8 * T * c)),
                      (2, (T * c - 1, 8 * T * c, 8 * T * c)), (2, (T * c, 8 * T * c - 1, 8 * T * c)),
                      (2, (T * c, 8 * T * c, 8 * T * c - 1))):
        raw, snake = Buf(2 * 8 * T, c, torch.float16), Buf(2 * 8 * T, c, torch.float16)
        rc = gpu_lib.zmi_dac_conv_t_lanes(xt.data_ptr(), T, c, wt.data_ptr(), bias.data_ptr(), c, 8, 4, raw.ptr(),
                                          snake.ptr(), alpha.data_ptr(), lanes, *ls, _stream())
        torch.cuda.synchronize()
        assert rc != 0 and raw.untouched() and snake.untouched(), (lanes, ls)

    # conv_out_range
    co = dc.conv_inputs(96, 1, 7, T, 1, 2)
    wo, bo = (v.to(DEV) for v in pack_conv_out(co["w"], co["bias"]))
    xo = torch.stack([co["x"].half()] * 2).to(DEV)
    for lanes, ls_x, ls_out in ((0, T * 96, 8), (65536, T * 96, 8), (2, T * 96 - 1, 8), (2, T * 96, 7)):
        out = Buf(16, 1, torch.float32)
        rc = gpu_lib.zmi_dac_conv_out_range_lanes(xo.data_ptr(), T, 96, wo.data_ptr(), bo.data_ptr(), 3, 8, out.ptr(),
                                                  lanes, ls_x, ls_out, _stream())
        torch.cuda.synchronize()
        assert rc != 0 and out.untouched(), (lanes, ls_x, ls_out)

    # from_codes
    g = torch.Generator().manual_seed(1)
    cb, pw, pb = (torch.randn(s, generator=g).to(DEV) for s in ((9, 1024, 8), (9, 1024, 8), (9, 1024)))
    codes = torch.randint(0, 1024, (2, 9, T), generator=g).to(DEV)
    for lanes, ls_c, ls_z in ((0, 9 * T, 1024 * T), (65536, 9 * T, 1024 * T), (2, 9 * T - 1, 1024 * T),
                              (2, 9 * T, 1024 * T - 1)):
        z = Buf(2 * T, 1024, torch.float16)
        rc = gpu_lib.zmi_dac_from_codes_lanes(codes.data_ptr(), T, cb.data_ptr(), pw.data_ptr(), pb.data_ptr(), z.ptr(),
                                              lanes, ls_c, ls_z, _stream())
        torch.cuda.synchronize()
        assert rc != 0 and z.untouched(), (lanes, ls_c, ls_z)
        assert gpu_lib.zmi_last_error().decode().startswith("dac_from_codes: ")
