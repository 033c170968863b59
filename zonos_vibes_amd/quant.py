"""Weight-only FP8 for the MLP projections: the format, and the M8F8 layout the GEMV reads (pure torch, CPU or GPU).

    W[n, k] ~= 2^e[n] * q[n, k]

q is OCP float8_e4m3fn (bias 7, 3 mantissa bits, subnormals at 2^-9, largest value 448, no infinities; never a
NaN code here), stored as its byte. e[n] is one signed power-of-two exponent per output row n of the nn.Linear
weight: the smallest integer with max_k |W[n, k]| / 2^e[n] <= 448 (0 for an all-zero row), raised to E_MIN where
it would be smaller so that every non-zero 2^e q is a normal bf16 (a weight beyond 448 * 2^E_MAX is refused).
q is W / 2^e (exact) rounded to nearest-even, so nothing saturates.

Every dequantised weight 2^e q has 4 significant bits and is therefore exactly a bf16: the model with fp8 MLP
weights IS the bf16 model loaded with dequantize_fp8(*quantize_fp8(W)), which is what the GEMV kernel is tested
against, bit for bit (include/zonos_hip.h, ZMI_WFMT_FP8).
"""
from __future__ import annotations

import torch

PACK_IDENTITY, PACK_SWIGLU = 0, 1  # zmi_pack_weight's modes (include/zonos_hip.h)
E4M3_MAX = 448.0
E_MIN, E_MAX = -117, 119  # 2^E_MIN * 2^-9 = 2^-126, the smallest normal bf16; 2^E_MAX * 448 < 2^128


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as fp32 for an integer tensor -126 <= e <= 127, from the exponent bits (exact on every device)."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def _round_e4m3(y: torch.Tensor) -> torch.Tensor:
    """fp32 y with |y| <= 448 -> uint8 E4M3 codes, round to nearest, ties to even."""
    a = y.abs()
    ex = (a.view(torch.int32) >> 23) - 127          # floor(log2 a) of a normal fp32 (-127 for zero)
    qe = (ex - 3).clamp_(min=-9)                     # the rounding quantum 2^qe: 3 mantissa bits, subnormals at 2^-9
    r = torch.round(a * _pow2(-qe))                  # 8 .. 16 in a normal binade, 0 .. 8 below 2^-6; ties to even
    v = r * _pow2(qe)                                # the rounded magnitude (exact)
    vb = v.view(torch.int32)
    normal = ((((vb >> 23) - 127 + 7) << 3) | ((vb >> 20) & 7))
    code = torch.where(v >= 2.0 ** -6, normal, r.to(torch.int32))  # a subnormal's code is its count of 2^-9
    code = code | (torch.signbit(y).to(torch.int32) << 7)
    return code.to(torch.uint8)


def e4m3_table(device=None) -> torch.Tensor:
    """The fp32 value of each of the 256 E4M3 codes (0x7f / 0xff, the NaN codes, are never produced here)."""
    c = torch.arange(256, dtype=torch.int32)
    ex, m = (c >> 3) & 15, c & 7
    mag = torch.where(ex == 0, torch.ldexp(m.float(), torch.full_like(m, -9)), torch.ldexp((8 + m).float(), ex - 10))
    return torch.where(c >= 128, -mag, mag).to(device)


def quantize_fp8(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """bf16 [n][k] -> (q uint8 [n][k] E4M3 codes, e int8 [n])."""
    if w.dim() != 2 or w.dtype != torch.bfloat16:
        raise ValueError("quantize_fp8 takes a bf16 [n][k] weight")
    x = w.float()
    amax = x.abs().amax(dim=1)
    if not bool(torch.isfinite(amax).all()):
        raise ValueError("quantize_fp8: the weight has a non-finite element")
    m, ex = torch.frexp(amax)                         # amax = m 2^ex, 0.5 <= m < 1; 448 = 0.875 * 2^9
    e = ex.to(torch.int32) - 9 + (m > 0.875).to(torch.int32)
    e = torch.where(amax == 0, torch.zeros_like(e), e).clamp_(min=E_MIN)
    if bool((e > E_MAX).any()):  # |W| > 448 * 2^119 ~ 2.98e38: its neighbours in E4M3 would round past bf16's range
        raise ValueError("quantize_fp8: a weight's magnitude is beyond 448 * 2^119")
    q = _round_e4m3(x * _pow2(-e).unsqueeze(1))       # a power-of-two scale: exact
    return q, e.to(torch.int8)


def dequantize_fp8(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """(q uint8 [n][k], e int8 [n]) -> bf16 [n][k] = 2^e q, exactly."""
    v = e4m3_table(q.device)[q.to(torch.int32)] * _pow2(e).unsqueeze(1)
    return v.to(torch.bfloat16)


def _source_rows(n_src: int, n_pad: int, mode: int, device) -> torch.Tensor:
    """The weight row that packed column n holds (n_src: a zero padding column)."""
    n = torch.arange(n_pad, device=device)
    if mode == PACK_SWIGLU:  # rows 0..3 of group g are fc1's value rows 4g.., rows 4..7 their gates F + 4g..
        g, r = n >> 3, n & 7
        return torch.where(r < 4, 4 * g + r, n_src // 2 + 4 * g + r - 4)
    return torch.where(n < n_src, n, torch.full_like(n, n_src))


def _check_pack(n_src: int, k: int, n_pad: int, mode: int):
    if mode not in (PACK_IDENTITY, PACK_SWIGLU):
        raise ValueError("pack: unknown mode")
    if n_pad % 8 or k % 128 or n_pad < n_src or (mode == PACK_SWIGLU and (n_src % 8 or n_pad != n_src)):
        raise ValueError("pack: bad shape (n_pad % 8, k % 128, n_pad >= n_src; SwiGLU: n_src % 8, no padding)")


def pack_m8f8(q: torch.Tensor, e: torch.Tensor, n_pad: int | None = None,
              mode: int = PACK_IDENTITY) -> tuple[torch.Tensor, torch.Tensor]:
    """(q [n_src][k], e [n_src]) -> (uint8 [n_pad * k] in layout M8F8, int8 [n_pad] exponents in packed column order).

    M8F8 is the bf16 layout M8 (zmi_pack_weight) at one byte per weight, two 64-k chunks per 1 KiB piece: piece
    (g, p) holds columns 8g .. 8g + 7 over k = 128p .. 128p + 127; lane l's 16 bytes are column 8g + (l & 7) at
    k = 128p + 64c + 32 ((l >> 3) & 1) + 8 (l >> 4) .. + 7 for c = 0 (bytes 0..7) and c = 1 (bytes 8..15). SwiGLU
    mode permutes the columns as zmi_pack_weight does, and the exponents with them; padding columns are zero."""
    n_src, k = q.shape
    n_pad = n_src if n_pad is None else n_pad
    _check_pack(n_src, k, n_pad, mode)
    rows = _source_rows(n_src, n_pad, mode, q.device)
    qz = torch.cat([q, q.new_zeros(1, k)])[rows]
    ez = torch.cat([e, e.new_zeros(1)])[rows]
    # [g][r][p][c][h][q4][b] -> [g][p][q4][h][r][c][b]: lane l = r + 8 h + 16 q4
    packed = qz.view(n_pad // 8, 8, k // 128, 2, 2, 4, 8).permute(0, 2, 5, 4, 1, 3, 6).contiguous().view(-1)
    return packed, ez.contiguous()


def unpack_m8f8(packed: torch.Tensor, e_packed: torch.Tensor, n_src: int, k: int,
                mode: int = PACK_IDENTITY) -> tuple[torch.Tensor, torch.Tensor]:
    """Inverse of pack_m8f8: (q [n_src][k], e [n_src])."""
    n_pad = e_packed.numel()
    _check_pack(n_src, k, n_pad, mode)
    qz = packed.view(n_pad // 8, k // 128, 4, 2, 8, 2, 8).permute(0, 4, 1, 5, 3, 2, 6).contiguous().view(n_pad, k)
    rows = _source_rows(n_src, n_pad, mode, packed.device)
    keep = rows < n_src
    q = packed.new_zeros(n_src, k)
    e = e_packed.new_zeros(n_src)
    q[rows[keep]] = qz[keep]
    e[rows[keep]] = e_packed[keep]
    return q, e
