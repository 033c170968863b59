"""The weight-only FP8 format (zonos_vibes_amd/quant.py) on the CPU: W[n, k] ~= 2^e[n] q[n, k], q OCP E4M3.

Every bound here follows from the format (3 mantissa bits, subnormals at 2^-9, largest value 448), none is measured.
"""
import ctypes

import pytest
import torch

from zonos_vibes_amd import quant

# log2 magnitude of row r of every 8-row group: neighbouring rows (the columns of one 8-column group of the GEMV)
# end up with exponents 12 or more apart, the zero row (exponent 0) between two tiny ones
ROW_LOG2 = (3, -12, None, -20, 0, -14, 2, -10)


def edge_weight(n: int, k: int, seed: int = 0) -> torch.Tensor:
    """bf16 [n][k] whose rows cycle through the format's edges, by r = row % 8 (row magnitude 2^ROW_LOG2[r]):
       0  maximum exactly 448 * 2^e                     4  half of the entries are +0 / -0
       1  maximum one bf16 ulp above 448 * 2^e          5, 6, 7  plain random rows
       2  all zeros                                     (magnitudes 2^-20 .. 2^3 within every group)
       3  maximum 448 * 2^e, the rest in and below the E4M3 subnormals: ties at 2^-10 and 1.5 * 2^-9, values that
          round to zero, signed."""
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros(n, k, dtype=torch.float32)
    for row in range(n):
        r, p = row % 8, ROW_LOG2[row % 8]
        if r == 2:
            continue
        x = (torch.rand(k, generator=g) * 1.6 - 0.8) * 2.0 ** p       # |x| < 0.8 * 2^p < 448 * 2^(p - 9)
        j = int(torch.randint(0, k, (1,), generator=g))
        sign = 1.0 if row % 16 < 8 else -1.0
        if r == 3:
            steps = torch.randint(-44, 45, (k,), generator=g).float()  # quarter steps of the subnormal quantum
            x = steps * 0.25 * 2.0 ** (p - 9 - 9)
        if r == 4:
            z = torch.rand(k, generator=g)
            x = torch.where(z < 0.25, torch.zeros(k), torch.where(z < 0.5, -torch.zeros(k), x))
        if r in (0, 3):
            x[j] = sign * 448.0 * 2.0 ** (p - 9)
        if r == 1:
            x[j] = sign * 450.0 * 2.0 ** (p - 9)                       # 448 + one bf16 ulp (2 at 2^8)
        w[row] = x
    return w.to(torch.bfloat16)


def _pow2(e):
    return torch.ldexp(torch.ones(e.shape), e.to(torch.int32))


def test_round_trip_on_edge_rows():
    """On rows built to hit the format's edges: the dequantised weight is exactly a bf16; no NaN code; |q| <= 448; e
    is minimal; every element is within half an E4M3 ulp (at its own binade, times 2^e) of the original.

    Minimality is max|W| / 2^e > 224 (then e - 1 would put the maximum above 448). The rounded q of such a row is
    >= 224, not > 224: row kind 1 (maximum 450 * 2^e') has max|W| / 2^e = 225, which rounds to the code of 224."""
    w = edge_weight(32, 256, seed=1)
    q, e = quant.quantize_fp8(w)
    assert q.dtype == torch.uint8 and q.shape == w.shape and e.dtype == torch.int8 and e.shape == (32,)
    d = quant.dequantize_fp8(q, e)
    assert d.dtype == torch.bfloat16
    exact = quant.e4m3_table()[q.long()].double() * _pow2(e).double().unsqueeze(1)   # 2^e q in fp64
    assert torch.equal(d.double(), exact)                                           # exactly a bf16
    assert torch.equal(d.float().to(torch.bfloat16), d)
    assert not ((q & 0x7f) == 0x7f).any()
    qv = quant.e4m3_table()[q.long()]
    assert qv.abs().max() <= 448
    amax = w.float().abs().amax(dim=1)
    ratio = amax / _pow2(e)
    for row in range(32):
        if row % 8 == 2:
            assert e[row] == 0 and not (q[row] & 0x7f).any()
        else:
            assert 224 < ratio[row] <= 448, row
            assert qv[row].abs().max() >= 224, row
    # the rows' exponents: exact maximum -> p - 9, one ulp above -> p - 8
    assert e[0] == 3 - 9 and e[1] == -12 - 8 and e[3] == -20 - 9
    # neighbouring rows of a group are far apart (what the GPU tests rely on)
    assert all(abs(int(e[i]) - int(e[i + 1])) >= 10 for i in range(31))
    # half an ulp of E4M3 at the element's binade: y = W / 2^e = m 2^x (0.5 <= m < 1) has quantum 2^max(x - 4, -9)
    y = w.float() / _pow2(e).unsqueeze(1)
    x = torch.frexp(y)[1]
    half_ulp = torch.ldexp(torch.ones_like(y), (x - 4).clamp(min=-9) - 1) * _pow2(e).unsqueeze(1)
    err = (d.double() - w.double()).abs()
    assert (err <= half_ulp.double()).all()
    assert (err > 0).any()            # the rows do exercise the rounding
    # subnormal codes, zeros of both signs and entries rounded to zero are all present
    assert ((q[3] & 0x78) == 0).any() and (q[4] == 0x80).any() and (q[4] == 0x00).any()
    assert ((q[3] & 0x7f) == 0).any()
    # signed zeros survive
    z = w[4].float() == 0
    assert torch.equal(torch.signbit(d[4].float())[z], torch.signbit(w[4].float())[z])


def test_rounding_is_nearest_even_exhaustively():
    """Against torch's float8_e4m3fn conversion on the CPU, over every bf16 value of two normal binades ([1, 4): 7
    mantissa bits onto 3, every tie included) and of two subnormal ones ([2^-8, 2^-6)), both signs; a 448 in each
    row pins e = 0."""
    bits = torch.arange(0x3f80, 0x4080, dtype=torch.int32)                 # bf16 [1, 4)
    hi = (bits << 16).view(torch.float32)
    lo = ((bits - (8 << 7)) << 16).view(torch.float32)                      # bf16 [2^-8, 2^-6)
    rows = [torch.cat([v, -v, torch.tensor([448.0])]) for v in (hi, lo)]
    w = torch.stack(rows).to(torch.bfloat16)
    assert torch.equal(w.float(), torch.stack(rows))
    q, e = quant.quantize_fp8(w)
    assert (e == 0).all()
    ref = w.float().to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(q, ref)
    assert torch.equal(quant.dequantize_fp8(q, e).float(), ref.view(torch.float8_e4m3fn).float())


def test_exponent_range_keeps_normal_bf16():
    """Rows of bf16's extremes: e stays within [E_MIN, E_MAX] and every non-zero dequantised value is a normal bf16."""
    tiny, huge = 2.0 ** -130, 2.9e38
    w = torch.tensor([[tiny, -tiny * 2, 0.0, tiny], [huge, -huge / 3, 1.0, 0.0]] * 4).repeat(1, 32).to(torch.bfloat16)
    q, e = quant.quantize_fp8(w)
    assert e.min() >= quant.E_MIN and e.max() <= quant.E_MAX
    d = quant.dequantize_fp8(q, e).float()
    assert torch.isfinite(d).all()
    assert (d[d != 0].abs() >= 2.0 ** -126).all()
    for bad in (float("inf"), 3.3e38):   # 3.3e38 > 448 * 2^119: E4M3 rounding could leave bf16's range
        with pytest.raises(ValueError):
            quant.quantize_fp8(torch.tensor([[bad] * 128]).to(torch.bfloat16))


@pytest.mark.parametrize("mode,n_src,n_pad", [(quant.PACK_IDENTITY, 24, 24), (quant.PACK_IDENTITY, 20, 24),
                                              (quant.PACK_SWIGLU, 32, 32)])
def test_pack_m8f8_layout_and_inverse(mode, n_src, n_pad):
    """pack -> unpack is the identity, the exponents travel with their rows, and every packed byte sits where the
    kernel reads it: piece (g, p), lane l, byte 8c + b = column 8g + (l & 7), k = 128p + 64c + 32((l>>3)&1) + 8(l>>4) + b."""
    k = 256
    w = edge_weight(n_src, k, seed=2)
    q, e = quant.quantize_fp8(w)
    packed, ep = quant.pack_m8f8(q, e, n_pad, mode)
    assert packed.dtype == torch.uint8 and packed.numel() == n_pad * k and ep.dtype == torch.int8 and ep.numel() == n_pad
    q2, e2 = quant.unpack_m8f8(packed, ep, n_src, k, mode)
    assert torch.equal(q2, q) and torch.equal(e2, e)
    f = n_src // 2
    for n in range(n_pad):
        g, r = n // 8, n % 8
        src = n if mode == quant.PACK_IDENTITY else (4 * g + r if r < 4 else f + 4 * g + r - 4)
        assert ep[n] == (e[src] if src < n_src else 0)
        for p in range(k // 128):
            for lane_hi in range(8):                       # l = r + 8 lane_hi
                l = r + 8 * lane_hi
                for c in range(2):
                    k0 = 128 * p + 64 * c + 32 * ((l >> 3) & 1) + 8 * (l >> 4)
                    o = ((g * (k // 128) + p) * 64 + l) * 16 + 8 * c
                    want = q[src, k0:k0 + 8] if src < n_src else torch.zeros(8, dtype=torch.uint8)
                    assert torch.equal(packed[o:o + 8], want), (n, p, l, c)
    with pytest.raises(ValueError):
        quant.pack_m8f8(q, e, n_pad + 4, mode)
    with pytest.raises(ValueError):
        quant.pack_m8f8(q[:, :192], e, n_pad, mode)


def test_weights_argument_validation():
    """No GPU is touched before the argument is checked: unknown strings are a ValueError, the hybrid with fp8 a
    NotImplementedError (engine, make_engine and Zonos alike)."""
    from zonos_vibes_amd.config import tiny_hybrid, tiny_transformer
    from zonos_vibes_amd.engine import WEIGHT_FORMATS, HipEngine, check_weights, make_engine
    from zonos_vibes_amd.model import Zonos
    assert WEIGHT_FORMATS == ("bf16", "fp8")
    check_weights("bf16", True)
    check_weights("fp8", False)
    for make in (make_engine, HipEngine, Zonos):
        with pytest.raises(ValueError, match="int8"):
            make(tiny_transformer(2), "cpu", weights="int8")
    for make in (make_engine, Zonos):
        with pytest.raises(NotImplementedError):
            make(tiny_hybrid(), "cpu", weights="fp8")


def test_gemv_args_carry_the_weight_format():
    from zonos_vibes_amd import _lib
    a = _lib.GemvArgs()
    assert a.w_fmt == _lib.WFMT_BF16 == 0 and a.w_exp is None and _lib.WFMT_FP8 == 1
    assert ctypes.sizeof(_lib.GemvArgs) % 8 == 0
    names = [f[0] for f in _lib.GemvArgs._fields_]
    assert names[-3:] == ["w_fmt", "reserved2", "w_exp"]      # appended: every earlier field keeps its offset
