"""CPU half of the per-kernel DAC tests: the weight packing of zonos_vibes_amd/autoencoder.py, read back by the
documented index formula (tests/dac_cases.emulate_conv), against float64 torch.nn.functional references, the
references of every GPU case of tests/test_gpu_dac_kernels.py confirmed the same way, and the derived error bound
shown to reject three mutants that whole-network SNR does not see."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import dac_cases as dc
from zonos_vibes_amd.autoencoder import (pack_conv, pack_conv_out, pack_conv_transpose, pack_im2col_conv1,
                                         pack_strided_conv)

TOL = 1e-12


def _close(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    assert err <= TOL, err


# ------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("dil", (1, 3, 9))
def test_pack_conv_k7(dil):
    c = dc.conv_inputs(64, 96, 7, 70, 70, dil)
    got = dc.emulate_conv(pack_conv(c["w"]), c["x"], c["bias"], 96, 7, dil, -3 * dil, 70, skip=c["skip"])
    _close(got, dc.ref_conv_same(c["x"], c["w"], c["bias"], dil) + c["skip"])


def test_pack_conv_1x1():
    c = dc.conv_inputs(96, 64, 1, 40, 40, 0)
    packed = pack_conv(c["w"])
    assert packed.shape == (1, 64, 96) and packed.dtype == torch.float16
    _close(dc.emulate_conv(packed, c["x"], c["bias"], 64, 1, 0, 0, 40), dc.ref_conv_same(c["x"], c["w"], c["bias"], 0))


@pytest.mark.parametrize("stride,pad", ((2, 1), (4, 2), (8, 4), (3, 2)))
def test_pack_conv_transpose(stride, pad):
    c = dc.conv_t_inputs(64, 32, stride, 19, pad)
    packed = pack_conv_transpose(c["w"], stride, pad)
    assert packed.shape == (stride, 2, 2, 32, 32) and packed.dtype == torch.float16
    got = dc.emulate_conv(packed, c["x"], c["bias"], 32, 2, -1, 0, 19, out_stride=stride, t_out=stride * 19,
                          nphase=stride, phase_pad=pad)
    _close(got, dc.ref_conv_t(c["x"], c["w"], c["bias"], stride, pad))


@pytest.mark.parametrize("stride", (2, 4, 8))
def test_pack_strided_conv(stride):
    ch, t = 32, 13 * stride
    c = dc.conv_inputs(ch, 2 * ch, 2 * stride, t, 1, stride)
    pad = math.ceil(stride / 2)
    packed = pack_strided_conv(c["w"], stride, pad)
    assert packed.shape == (3, stride * ch // 32, 2 * ch, 32)
    # the kernel reads x [t][c] as its polyphase view [t / s][s c]: the same memory
    got = dc.emulate_conv(packed, c["x"].reshape(t // stride, stride * ch), c["bias"], 2 * ch, 3, 1, -1, t // stride)
    _close(got, dc.ref_strided(c["x"], c["w"], c["bias"], stride, pad))


def test_pack_conv_out():
    c = dc.conv_inputs(96, 1, 7, 50, 1, 1)
    w, b = pack_conv_out(c["w"], c["bias"])
    assert w.shape == (7, 3, 32, 32) and w.dtype == torch.float16 and b.shape == (32,) and b.dtype == torch.float32
    got = dc.emulate_conv(w, c["x"], b, 32, 7, 1, -3, 50)
    _close(got[:, :1], dc.ref_conv_same(c["x"], c["w"], c["bias"], 1))
    assert got[:, 1:].abs().max() == 0  # channels 1..31: zero weights and bias


def test_pack_im2col_conv1():
    g = torch.Generator().manual_seed(5)
    wav = dc.f16_values((37,), g)
    w1 = dc.f16_values((64, 1, 7), g, 1 / math.sqrt(7))
    b1 = torch.randn(64, generator=g).float().double()
    packed = pack_im2col_conv1(w1)
    assert packed.shape == (1, 64, 32) and packed.dtype == torch.float16
    col = torch.zeros(37, 32, dtype=torch.float64)  # zmi_dac_im2col7's rows: col[t][k] = wav[t + k - 3]
    col[:, :7] = F.pad(wav, (3, 3)).unfold(0, 7, 1)
    got = dc.emulate_conv(packed, col, b1, 64, 1, 0, 0, 37)
    _close(got, F.conv1d(wav[None, None], w1, b1, padding=3)[0].t())


# ------------------------------------------------------------------------------------------------ the GPU cases' references
@pytest.mark.parametrize("shape", dc.SAME_SHAPES, ids=str)
def test_same_conv_case_references(shape):
    """Every shape of the GPU test at a length with both edges and an interior: the F.conv1d reference, the general
    zero-padded reference and the packed-layout emulation agree."""
    c_in, c_out, taps, dil = shape
    T = 129
    c = dc.conv_inputs(c_in, c_out, taps, T, T, dil)
    ref = dc.ref_conv_same(c["x"], c["w"], c["bias"], dil)
    in_off = -dil * (taps - 1) // 2
    _close(dc.ref_conv(c["x"], c["w"], c["bias"], dil, in_off, T), ref)
    _close(dc.emulate_conv(pack_conv(c["w"]), c["x"], c["bias"], c_out, taps, dil, in_off, T), ref)


@pytest.mark.parametrize("shape", dc.CONV_T_SHAPES, ids=str)
def test_conv_t_case_references(shape):
    c_in, c_out, stride, pad = shape
    c = dc.conv_t_inputs(c_in, c_out, stride, 33, pad)
    got = dc.emulate_conv(pack_conv_transpose(c["w"], stride, pad), c["x"], c["bias"], c_out, 2, -1, 0, 33,
                          out_stride=stride, t_out=stride * 33, nphase=stride, phase_pad=pad)
    _close(got, dc.ref_conv_t(c["x"], c["w"], c["bias"], stride, pad))


@pytest.mark.parametrize("in_off", (5, -40))
@pytest.mark.parametrize("out_stride,out_phase,extra", ((1, 0, 0), (3, 2, 0), (3, 2, 7)))
def test_general_indexing_reference(in_off, out_stride, out_phase, extra):
    t_in, n_out, dil = 100, 130, 3
    c = dc.conv_inputs(32, 32, 7, t_in, 1, in_off)
    t_out = out_stride * n_out + extra
    got = dc.emulate_conv(pack_conv(c["w"]), c["x"], c["bias"], 32, 7, dil, in_off, n_out, out_stride, out_phase, t_out)
    rows = torch.arange(n_out) * out_stride + out_phase
    _close(got[rows], dc.ref_conv(c["x"], c["w"], c["bias"], dil, in_off, n_out))
    untouched = torch.ones(t_out, dtype=torch.bool)
    untouched[rows] = False
    assert torch.isnan(got[untouched]).all()
    # rows whose every tap lies past either end are the bias alone
    q = torch.arange(n_out)
    lo, hi = q + in_off, q + in_off + 6 * dil
    outside = (hi < 0) | (lo >= t_in)
    assert outside.any()
    assert torch.equal(got[rows][outside], c["bias"][None].expand(int(outside.sum()), -1))


# ------------------------------------------------------------------------------------------------ the bound
@pytest.fixture(scope="module")
def mutant_case():
    c_in, c_out, taps, dil, T = 64, 96, 7, 3, 129
    c = dc.conv_inputs(c_in, c_out, taps, T, T, 99)
    ref = dc.ref_conv_same(c["x"], c["w"], c["bias"], dil)
    M = dc.ref_conv_same(c["x"].abs(), c["w"].abs(), c["bias"].abs(), dil)
    return dict(c, dil=dil, T=T, ref=ref, M=M, K=taps * c_in)


def _ratios(mc, y):
    """Worst |y - ref| / bound under the fp32 bound and, after fp16 rounding, under the fp16 raw bound."""
    return (dc.worst_ratio(y, mc["ref"], dc.bound("f32", mc["ref"], mc["M"], mc["K"])),
            dc.worst_ratio(y.half(), mc["ref"], dc.bound("raw", mc["ref"], mc["M"], mc["K"])))


def test_bound_accepts_fp32_conv(mutant_case):
    mc = mutant_case
    y = F.conv1d(mc["x"].float().t()[None], mc["w"].float(), mc["bias"].float(), dilation=mc["dil"],
                 padding=3 * mc["dil"])[0].t()
    r32, r16 = _ratios(mc, y)
    assert r32 <= 1 and r16 <= 1, (r32, r16)
    z = dc.snake64(y, mc["alpha"]).half()
    zr = dc.snake64(mc["ref"], mc["alpha"])
    assert dc.worst_ratio(z, zr, dc.bound("snake", zr, mc["M"], mc["K"], mc["alpha"][None])) <= 1


def test_bound_rejects_tap_dropped_at_the_edges(mutant_case):
    """Tap 2 (reading row t - dil) left out in the first and last 3 dil rows only: 18 of 129 rows."""
    mc = mutant_case
    w1 = torch.zeros_like(mc["w"])
    w1[:, :, 2] = mc["w"][:, :, 2]
    term = dc.ref_conv_same(mc["x"], w1, None, mc["dil"])
    edge = torch.zeros(mc["T"], dtype=torch.bool)
    edge[: 3 * mc["dil"]] = edge[-3 * mc["dil"]:] = True
    y = mc["ref"] - term * edge[:, None]
    assert torch.equal(y[~edge], mc["ref"][~edge])
    r32, r16 = _ratios(mc, y)
    assert r32 > 1 and r16 > 1, (r32, r16)


def test_bound_rejects_clamped_padding(mutant_case):
    mc = mutant_case
    p = 3 * mc["dil"]
    xp = F.pad(mc["x"].t()[None], (p, p), mode="replicate")
    y = F.conv1d(xp, mc["w"], mc["bias"], dilation=mc["dil"])[0].t()
    assert torch.equal(y[p:-p], mc["ref"][p:-p])  # only the rows next to the signal's ends change
    r32, r16 = _ratios(mc, y)
    assert r32 > 1 and r16 > 1, (r32, r16)


def test_bound_rejects_swapped_channel_blocks(mutant_case):
    mc = mutant_case
    w = mc["w"].clone()
    w[:, :32], w[:, 32:64] = mc["w"][:, 32:64], mc["w"][:, :32]
    r32, r16 = _ratios(mc, dc.ref_conv_same(mc["x"], w, mc["bias"], mc["dil"]))
    assert r32 > 1 and r16 > 1, (r32, r16)


def test_raw_matches_f32_rule():
    y = torch.tensor([1.0, -0.3333, 3e-5, 2.0 ** -15, 0.5], dtype=torch.float32)
    raw = y.half()
    assert dc.raw_matches_f32(raw, y) == (0, 0.4)
    off = raw.clone()
    off[2] = off[2] + 2.0 ** -24  # one subnormal step on a small element: allowed
    assert dc.raw_matches_f32(off, y)[0] == 0
    off[0] = torch.nextafter(raw[0].float(), torch.tensor(2.0)).half() + 2.0 ** -10  # a normal element: not
    assert dc.raw_matches_f32(off, y)[0] == 1


def test_delta_constants_within_the_issue_limits():
    assert 0 <= dc.DELTA_SIN <= dc.DELTA_SIN_MAX == 2.0 ** -14
    assert 0 < dc.DELTA_TANH <= dc.DELTA_TANH_MAX == 2.0 ** -20
