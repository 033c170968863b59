"""Inputs and bit-exact references for the token glue kernels at the end of csrc/zmi_sample.hip: the embedding sum
(zmi_embed_codes, zmi_embed_step, the embedding fused in the samplers) and the delay pattern (zmi_apply_delay_pattern,
zmi_revert_delay_pattern, zmi_delay_init, zmi_delay_revert, zmi_delay_revert_range). No GPU library is imported here:
tests/test_glue_cases_cpu.py judges this module on the CPU, tests/test_gpu_glue_probe.py runs the kernels.

Embedding (reference model.py:97-98): the sum over codebooks 0 .. 8 in order, rounded to bf16 after every addition.
With random tables that is hardly distinguishable from an fp32 sum rounded once, so `table(d, "cancel")` puts
+A, small, -A, small, ... along the codebook axis with A in [128, 256), where one bf16 step is 1: under the sequential
rounding a small term added to +-A is rounded away or up to a whole step, the fp32 sum keeps it, and the reversed order
meets the large terms at other partial sums.

Delay pattern: oracle.zonos_cpu.apply_delay_pattern / revert_delay_pattern, bit for bit.
"""
from __future__ import annotations

import torch

from oracle.zonos_cpu import apply_delay_pattern, revert_delay_pattern

NCB, NV, MASK, EOS = 9, 1026, 1025, 1024
EMBED_WIDTHS = (8, 2040, 2048, 2056, 4096)  # one thread; a partial first trip; full; a second trip of one thread; two
EDGE_TOKENS = (0, 1023, 1024, 1025, -1, 1026)  # the last two are clamped to 0 and 1025
APPLY_T = (0, 1, 8, 9, 10, 255, 256, 257, 600)
INIT_TCAP = (64, 256, 300)
INIT_PREFIX = (0, 1, 7)
REVERT_VALUES = (-1, 0, 1023, 1024, 1025)


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(0x61C + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))
    return g


# ----------------------------------------------------------------------------- embeddings
def table(d: int, kind: str = "seeded") -> torch.Tensor:
    """[9, 1026, d] bf16. seeded: N(0, 1) scaled by 0.1 .. 1.7 per codebook, so that no two codebooks can be swapped.
    cancel: see the module docstring; the large terms depend on (codebook pair, column) only, so that they cancel
    whatever the tokens are, the small ones on everything."""
    g = _gen(d, kind == "cancel")
    t = torch.randn(NCB, NV, d, generator=g)
    if kind == "seeded":
        return (t * (0.1 + 0.2 * torch.arange(NCB).view(NCB, 1, 1))).to(torch.bfloat16)
    assert kind == "cancel"
    t = (t * 0.2).to(torch.bfloat16)
    for k in (0, 4):
        big = (128.0 * (1.0 + torch.rand(d, generator=g))).to(torch.bfloat16)
        t[k], t[k + 2] = big, -big
    return t


def clamp_tokens(toks: torch.Tensor) -> torch.Tensor:
    return toks.clamp(0, MASK).long()


def embed_ref(tab: torch.Tensor, toks: torch.Tensor) -> torch.Tensor:
    """toks [9, n] (any integers; clamped as the kernels do) -> [n, d] bf16: the sequential bf16 sum."""
    toks = clamp_tokens(toks)
    acc = tab[0, toks[0]]
    for k in range(1, NCB):
        acc = acc + tab[k, toks[k]]  # a bf16 add: the fp32 sum of the two, rounded to bf16
    return acc


def embed_fp32_once(tab: torch.Tensor, toks: torch.Tensor) -> torch.Tensor:
    """Mutant: the fp32 sum, rounded once."""
    toks = clamp_tokens(toks)
    acc = tab[0, toks[0]].float()
    for k in range(1, NCB):
        acc = acc + tab[k, toks[k]].float()
    return acc.to(torch.bfloat16)


def embed_reversed(tab: torch.Tensor, toks: torch.Tensor) -> torch.Tensor:
    """Mutant: the sequential bf16 sum over codebooks 8 .. 0."""
    toks = clamp_tokens(toks)
    acc = tab[NCB - 1, toks[NCB - 1]]
    for k in range(NCB - 2, -1, -1):
        acc = acc + tab[k, toks[k]]
    return acc


def code_columns(n: int, seed: int = 0) -> torch.Tensor:
    """[9, n] int32: every EDGE_TOKENS value in every column (rotated by the column), the rest random."""
    g = _gen(n, seed, 3)
    c = torch.randint(0, NV, (NCB, n), generator=g, dtype=torch.int32)
    for col in range(n):
        for i, tok in enumerate(EDGE_TOKENS):
            c[(i + col) % NCB, col] = tok
    return c


def padded_codes(codes: torch.Tensor, extra: int = 5, fill: int = 7) -> torch.Tensor:
    """[9, n + extra] int32 with codes in the first n columns: ld_codes > n. A kernel that strides by n reads `fill`."""
    out = torch.full((NCB, codes.shape[1] + extra), fill, dtype=torch.int32)
    out[:, :codes.shape[1]] = codes
    return out


# ----------------------------------------------------------------------------- slots of a decode step
def step_state(tcap: int, seed: int = 0) -> dict:
    """Four slots for zmi_embed_step: active and inactive side by side, offset at 0 and at tcap - 1, delayed codes
    over the whole range -1 .. 1026 with the EDGE_TOKENS in the frames that are read."""
    g = _gen(tcap, seed, 5)
    S = 4
    st = dict(active=torch.tensor([1, 0, 1, 1], dtype=torch.int32),
              offset=torch.tensor([0, 3, tcap - 1, tcap // 2], dtype=torch.int32),
              pos=torch.tensor([17, 23, 5, 0], dtype=torch.int32))
    delayed = torch.randint(-1, NV + 1, (S, NCB, tcap), generator=g, dtype=torch.int32)
    for s in range(S):
        delayed[s, :, int(st["offset"][s])] = code_columns(1, seed + s)[:, 0]
    st["delayed"] = delayed
    return st


def step_frames(st: dict) -> torch.Tensor:
    """[9, S]: the frame each slot embeds."""
    S = st["delayed"].shape[0]
    return torch.stack([st["delayed"][s, :, int(st["offset"][s])] for s in range(S)], dim=1)


# ----------------------------------------------------------------------------- delay pattern
def audio_codes(batch: int, T: int, seed: int = 0) -> torch.Tensor:
    return torch.randint(0, 1024, (batch, NCB, T), generator=_gen(batch, T, seed, 7), dtype=torch.int64)


def init_ref(tcap: int, prefix: torch.Tensor, total_len: int) -> torch.Tensor:
    """[9, tcap] int32 of one slot after zmi_delay_init: the delay pattern of [prefix | unknown (-1)] over total_len
    columns, MASK from total_len on."""
    p = prefix.shape[1]
    n_audio = total_len - NCB
    assert 0 <= p <= n_audio and total_len <= tcap
    codes = torch.full((1, NCB, n_audio), -1, dtype=torch.int64)
    codes[0, :, :p] = prefix
    out = torch.full((NCB, tcap), MASK, dtype=torch.int32)
    out[:, :total_len] = apply_delay_pattern(codes, MASK)[0].to(torch.int32)
    return out


def init_cases():
    """(tcap, prefix_len, total_len) over INIT_TCAP x INIT_PREFIX x {9, 10, tcap}, where the prefix fits the audio
    columns (total_len - 9): a longer prefix has no meaning in the reference."""
    return [(tcap, p, total) for tcap in INIT_TCAP for p in INIT_PREFIX for total in (9, 10, tcap) if p <= total - NCB]


def revert_buffer(S: int, tcap: int, seed: int = 0) -> torch.Tensor:
    """[S, 9, tcap] int32 over REVERT_VALUES, each slot different."""
    vals = torch.tensor(REVERT_VALUES, dtype=torch.int32)
    return vals[torch.randint(0, len(vals), (S, NCB, tcap), generator=_gen(S, tcap, seed, 11))]


def revert_ref(delayed_slot: torch.Tensor, t_out: int) -> torch.Tensor:
    """[9, t_out] int64: the reverted frames of one slot's [9, tcap] buffer; values >= 1024 become 0, -1 stays."""
    out = revert_delay_pattern(delayed_slot[None, :, :t_out + NCB].long())[0]
    return torch.where(out >= 1024, torch.zeros_like(out), out)
