"""Shared by the CPU and GPU resampling tests: the fp64 reference and its error bound, a torch restatement of the
kernel contract (resampling.Piece in, outputs and the new carry out), the chunk splits and the sine check."""
import math

import torch

from zonos_vibes_amd import resampling as rs

OUT_RATES = (48000, 24000, 16000, 8000)   # from 44.1 kHz
IN_RATES = (48000, 16000)                 # to 44.1 kHz
SPLIT_HEAD = (1, 0, 7, 511, 512, 513)     # then the rest


def frames_of(x: torch.Tensor, plan) -> torch.Tensor:
    """[.., N] -> [.., F, T]: frame f holds xz[f o - W .. f o - W + T), F = ceil(L / n) frames."""
    o, n, W, T = plan
    L = rs.out_len(x.shape[-1], plan)
    F = -(-L // n)
    need = (max(F, 1) - 1) * o + T  # (at least one window, so that an empty utterance unfolds to zero frames of T)
    xp = torch.nn.functional.pad(x, (W, max(need - W - x.shape[-1], 0)))
    return xp.unfold(-1, T, o)[..., :F, :]


def ref64(x: torch.Tensor, orig: int, new: int):
    """(the fp64 evaluation [.., L] of the fp32 table on x, its error bound for a T-term fp32 chain)."""
    plan = rs.resample_plan(orig, new)
    o, n, W, T = plan
    L = rs.out_len(x.shape[-1], plan)
    kern = rs.table(plan).double()
    fr = frames_of(x.double().cpu(), plan)
    y = (fr @ kern.t()).reshape(*x.shape[:-1], -1)[..., :L]
    # every product is rounded once (or fused) and each of the T additions once; (T + 2) units in the last place of
    # the magnitude sum cover any order of T terms (tests/dac_cases.py's chain bound)
    b = (T + 2) * 2.0 ** -24 * (fr.abs() @ kern.abs().t()).reshape(*x.shape[:-1], -1)[..., :L] + 1e-30
    return y, b


def torch_kernel(plan, drop_carry_head: bool = False):
    """kernel(pieces, out) in torch fp32 with a fixed ascending-t order (one multiply and one add per tap).
    drop_carry_head builds a mutant a bookkeeping test has to reject: the carry is read without its first sample
    (everything behind it one place early)."""
    o, n, W, T = plan
    kern = rs.table(plan)

    def kernel(pieces, out):
        for p in pieces:
            have = torch.cat([p.carry, p.src])
            if drop_carry_head and p.carry.numel():
                have = torch.cat([have[1:], torch.zeros(1)])
            end = p.i0 + have.numel()
            hi = end if p.n_total < 0 else min(end, p.n_total)
            have = torch.cat([have, torch.zeros(1)])  # never empty; index end reads 0
            if p.n_out:
                j = torch.arange(p.j0, p.j0 + p.n_out)
                f, ph = j // n, j % n
                acc = torch.zeros(p.n_out, dtype=torch.float32)
                for t in range(T):
                    i = f * o - W + t
                    ok = (i >= max(p.i0, 0)) & (i < hi)
                    xv = have[torch.where(ok, i - p.i0, torch.full_like(i, end - p.i0))]
                    acc = acc + xv * kern[ph, t]
                out[p.dst: p.dst + p.n_out] = acc
            k = p.carry_out.numel()
            if k:
                p.carry_out.copy_(torch.cat([p.carry, p.src])[-k:])
    return kernel


def whole(x: torch.Tensor, orig: int, new: int, kernel=None) -> torch.Tensor:
    """The one-shot result of a kernel: one piece that is the whole utterance."""
    plan = rs.resample_plan(orig, new)
    kernel = kernel or torch_kernel(plan)
    L = rs.out_len(x.numel(), plan)
    out = torch.empty(L, dtype=torch.float32, device=x.device)
    none = x.new_empty(0)
    kernel([rs.Piece(none, x.contiguous().view(-1), 0, x.numel(), 0, L, 0, none)], out)
    return out


def splits(n: int, which: str) -> list:
    """Chunk lengths that sum to n: "head" = (1, 0, 7, 511, 512, 513, rest), "ones" = every sample alone."""
    if which == "ones":
        return [1] * n
    out, left = [], n
    for s in SPLIT_HEAD:
        s = min(s, left)
        out.append(s)
        left -= s
    return out + [left]


def run_streamed(sr, xs: dict, which: str, check=None) -> dict:
    """Push every lane's utterance through a StreamResampler in `which` splits, lanes side by side (a lane that has
    run out of chunks ends with an empty final push); returns {lane: the concatenated emissions}. check(lane, recv,
    emitted, final) is called after every push."""
    cuts = {lane: splits(x.numel(), which) for lane, x in xs.items()}
    at = {lane: 0 for lane in xs}
    got = {lane: [] for lane in xs}
    live = set(xs)
    k = 0
    while live:
        chunks, final = {}, []
        for lane in sorted(live):
            if k < len(cuts[lane]):
                m = cuts[lane][k]
                chunks[lane] = xs[lane][at[lane]: at[lane] + m]
                at[lane] += m
            if k >= len(cuts[lane]) - 1:
                final.append(lane)
        recv0 = {lane: sr.received(lane) + (chunks[lane].numel() if lane in chunks else 0) for lane in live}
        res = sr.push(chunks, final=final)
        for lane, y in res.items():
            got[lane].append(y.view(-1))
            if check is not None:
                check(lane, recv0[lane], sum(g.numel() for g in got[lane]), lane in final)
        live -= set(final)
        k += 1
    return {lane: torch.cat(g) for lane, g in got.items()}


def sine_error(resample, orig: int, new: int, freq: float = 1000.0) -> float:
    """max |resample(1 kHz sine at orig, orig / 4 samples) - the sine at new| away from the ends."""
    N = orig // 4
    x = torch.sin(2 * math.pi * freq * torch.arange(N, dtype=torch.float64) / orig)
    y = resample(x).double().cpu().view(-1)
    want = torch.sin(2 * math.pi * freq * torch.arange(y.numel(), dtype=torch.float64) / new)
    W = rs.resample_plan(orig, new)[2]
    skip = 4 * W * (new // orig + 1) + 64
    assert y.numel() > 2 * skip + 100
    return float((y - want)[skip:-skip].abs().max())
