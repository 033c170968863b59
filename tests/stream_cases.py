"""Cases shared by the CPU and GPU tests of DACStreamDecoder: utterance lengths and push patterns."""
import torch

from zonos_vibes_amd.streaming import DAC_LOOKAHEAD_FRAMES as R

CHUNKS = (4, 16)
RAGGED = (3, 1, 17, 0, 5, 2, 9, 0, 1, 30)


def lengths(chunk: int):
    """1 frame; the lookahead and one past it (nothing, then one frame, before flush); one frame with both halos
    whole; a steady-state window plus a remainder; many windows."""
    return (1, R, R + 1, 2 * R + 1, 2 * R + chunk + 3, 75)


def pushes(pattern: str, T: int):
    """Sizes of the pushes of a T-frame utterance."""
    if pattern == "all":
        return [T]
    if pattern == "single":
        return [1] * T
    out, i = [], 0
    while sum(out) < T:
        out.append(min(RAGGED[i % len(RAGGED)], T - sum(out)))
        i += 1
    return out


PATTERNS = ("all", "single", "ragged")


def random_codes(T: int, seed: int = 0) -> torch.Tensor:
    return torch.randint(0, 1024, (1, 9, T), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


def run_stream(dec, codes: torch.Tensor, sizes) -> torch.Tensor:
    """Push `codes` [1, 9, T] in pieces of `sizes`, flush, and concatenate what came back."""
    parts, t = [], 0
    for n in sizes:
        piece = codes[..., t: t + n]
        parts.append(dec.push(piece if t % 2 else piece[0]))  # both accepted shapes: [1, 9, n] and [9, n]
        assert parts[-1].shape[-1] % 512 == 0 and parts[-1].shape[:2] == (1, 1)
        t += n
    assert t == codes.shape[-1]
    parts.append(dec.flush())
    return torch.cat(parts, dim=-1)
