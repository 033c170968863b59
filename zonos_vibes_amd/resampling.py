"""Sample-rate conversion on the GPU: torchaudio's default polyphase resampler (speaker.resample_kernel's table) as one
HIP launch over many pieces of audio (zmi_resample), one-shot (GpuResampler) and streamed (StreamResampler).

With g = gcd(orig_rate, new_rate), o = orig_rate / g, n = new_rate / g and (kern [n][T], W) = resample_kernel(o, n),
T = 2 W + o, an utterance x[0 .. N) gives L = ceil(n N / o) samples

    y[j] = sum_{t < T} xz[(j // n) o - W + t] * kern[j % n][t],      xz = x inside [0, N), 0 outside.

A streaming lane that has received I samples and has not ended has emitted E(I) = n max(0, (I - W) // o): the whole
frames whose every tap is there; when it ends it emits the rest, up to L. The summation order depends on the tap alone,
so a lane's emissions concatenated are the one-shot result bit for bit, however the input was cut.

Parity with torchaudio itself is unpinned (torchaudio is absent here, as for the speaker front end): the tests tie the
kernel to an fp64 evaluation of the same table, to speaker.resample() and to an analytic sine.
"""
from __future__ import annotations

import math
import numbers
from dataclasses import dataclass
from typing import Any, Callable, Iterable

MAX_TABLE_FLOATS = 1 << 22  # n T: 44101 -> 44100 would need 7.8 GB


def resample_plan(orig_rate: int, new_rate: int) -> tuple:
    """(o, n, W, T) of orig_rate -> new_rate. ValueError for rates that are not positive integers, and for a table of
    more than 2^22 floats (before anything is allocated)."""
    for r in (orig_rate, new_rate):
        if isinstance(r, bool) or not isinstance(r, numbers.Integral) or r <= 0:
            raise ValueError(f"sample rates must be positive integers, got {orig_rate!r} -> {new_rate!r}")
    g = math.gcd(int(orig_rate), int(new_rate))
    o, n = int(orig_rate) // g, int(new_rate) // g
    W = math.ceil(6 * o / (min(o, n) * 0.99))  # resample_kernel's width, known before its table is built
    T = 2 * W + o
    if o != n and n * T > MAX_TABLE_FLOATS:
        raise ValueError(f"resampling {orig_rate} -> {new_rate} Hz needs a table of {n} x {T} floats "
                         f"(> {MAX_TABLE_FLOATS}): choose rates with a larger common divisor")
    return o, n, W, T


def emitted(received: int, plan: tuple) -> int:
    """E(I): output samples a lane that has not ended has emitted after I input samples."""
    o, n, W, _ = plan
    return n * max(0, (int(received) - W) // o)


def out_len(samples: int, plan: tuple) -> int:
    """L = ceil(n N / o)."""
    o, n = plan[0], plan[1]
    return -((-n * int(samples)) // o)


def table(plan: tuple):
    """speaker.resample_kernel's table [n][T] fp32 for a plan."""
    from .speaker import resample_kernel
    o, n, W, T = plan
    kern, width = resample_kernel(o, n)
    if width != W or tuple(kern.shape) != (n, T):
        raise RuntimeError(f"resample_kernel({o}, {n}) gave width {width}, table {tuple(kern.shape)}; "
                           f"planned {W}, {(n, T)}")
    return kern


@dataclass
class Piece:
    """One ZmiResampleSeg: a stretch of one utterance's outputs (include/zonos_hip.h)."""
    carry: Any      # 1-D fp32 [n_carry]: the utterance's samples i0 .. i0 + n_carry (the lane's kept tail)
    src: Any        # 1-D fp32 [n_src]: the samples that follow
    i0: int
    n_total: int    # the utterance's length if the piece ends it, else -1
    j0: int
    n_out: int
    dst: int        # outputs j0 .. j0 + n_out -> out[dst .. dst + n_out)
    carry_out: Any  # 1-D fp32 [n_keep]: receives the last n_keep samples of (carry, src)


def _device(device):
    """torch.device with the index filled in ("cuda" -> the current cuda device), so that it compares equal to a
    tensor's .device."""
    import torch
    d = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if d.type == "cuda" and d.index is None else d


class HipResampleKernel:
    """kernel(pieces, out) on the HIP library: ONE zmi_resample launch for every piece's outputs and ONE
    zmi_resample_carry launch for every piece's new tail, on the current stream. The table lives on the device; the
    segment tables go through a small ring of (pinned host, device) buffer pairs. A pair's event is recorded behind the
    launches that read it, and the pair is reused or dropped only once that event has passed; the device buffers and
    the table are allocated at construction, on whatever stream was current then, so every call marks them as used
    by the stream it launches on."""
    RING = 4
    WORDS = 11  # int64 words of a ZmiResampleSeg

    def __init__(self, device, plan: tuple):
        import torch
        from . import _lib
        self.dev, self.lib, self.plan = _device(device), _lib.lib(), plan
        self.kern_t = table(plan).t().contiguous().to(self.dev)  # [T][n]: phases contiguous
        torch.cuda.current_stream(self.dev).synchronize()  # the table's copy: later launches may be on another stream
        self._ring, self._at = [], 0
        self._reserve(8)

    def _reserve(self, rows: int):
        import torch
        self._ring = [(torch.empty(rows, self.WORDS, dtype=torch.int64).pin_memory(),
                       torch.empty(rows, self.WORDS, dtype=torch.int64, device=self.dev), torch.cuda.Event())
                      for _ in range(self.RING)]
        self._used = [False] * self.RING

    def __call__(self, pieces: list, out):
        import torch
        from . import _lib
        if not pieces:
            return
        for p in pieces:  # a pointer from another device (or the host) would be dereferenced on this one
            if any(t.numel() and t.device != self.dev for t in (p.carry, p.src, p.carry_out)) or out.device != self.dev:
                raise ValueError(f"resample: every tensor of a piece must be on {self.dev}")
        if len(pieces) > self._ring[0][0].shape[0]:
            for _, _, ev in self._ring:
                ev.synchronize()
            self._reserve(2 * len(pieces))
        k = self._at
        self._at = (k + 1) % self.RING
        host, dev, ev = self._ring[k]
        if self._used[k]:
            ev.synchronize()
        m = len(pieces)
        host.numpy()[:m] = [(p.carry.data_ptr() if p.carry.numel() else 0, p.carry.numel(),
                             p.src.data_ptr() if p.src.numel() else 0, p.src.numel(), p.i0, p.n_total, p.j0, p.n_out,
                             p.dst, p.carry_out.data_ptr() if p.carry_out.numel() else 0, p.carry_out.numel())
                            for p in pieces]
        o, n, W, _ = self.plan
        stream = torch.cuda.current_stream(self.dev)
        dev.record_stream(stream)
        self.kern_t.record_stream(stream)
        dev[:m].copy_(host[:m], non_blocking=True)
        self._used[k] = True
        try:
            _lib.check(self.lib.zmi_resample(dev.data_ptr(), host.data_ptr(), m, out.numel(), self.kern_t.data_ptr(),
                                             o, n, W, out.data_ptr(), stream.cuda_stream), "resample")
            if any(p.carry_out.numel() for p in pieces):
                _lib.check(self.lib.zmi_resample_carry(dev.data_ptr(), host.data_ptr(), m, o, n, W,
                                                       stream.cuda_stream), "resample_carry")
        finally:
            ev.record(stream)  # behind the copy and the launches: they read both halves of the pair


class GpuResampler:
    """One-shot: [..., N] fp32 cuda -> [..., ceil(n N / o)], every leading row a segment of ONE launch (on the
    current stream). o == n returns the input unchanged."""

    def __init__(self, device, orig_rate: int, new_rate: int):
        import torch
        self.plan = resample_plan(orig_rate, new_rate)
        self.dev = _device(device)
        self.identity = self.plan[0] == self.plan[1]
        self.kernel = None if self.identity else HipResampleKernel(self.dev, self.plan)

    def __call__(self, wav):
        import torch
        if self.identity:
            return wav
        if wav.device != self.dev or wav.dtype != torch.float32:
            raise ValueError(f"GpuResampler takes fp32 tensors on {self.dev} (the kernel is the only implementation)")
        N = wav.shape[-1]
        L = out_len(N, self.plan)
        if L == 0:
            return wav.new_empty(*wav.shape[:-1], 0)
        x = wav.contiguous().view(-1, N)
        out = torch.empty(x.shape[0] * L, dtype=torch.float32, device=self.dev)
        none = x.new_empty(0)
        self.kernel([Piece(none, x[r], 0, N, 0, L, r * L, none) for r in range(x.shape[0])], out)
        return out.view(*wav.shape[:-1], L)


class StreamResampler:
    """`lanes` independent streaming resamplers that run together.

        push({lane: chunk [.., m] fp32}, final=lanes that end with this push) -> {lane: [1, 1, k] fp32}
        flush(lanes)   the same as push({}, final=lanes)
        reset(lane)    drop a lane's utterance

    Per lane the state is the counts of samples received and emitted and the carry: the tail of the input that later
    frames still read (fewer than T samples), kept in a per-lane buffer that is double-buffered, so the call that reads
    a lane's carry writes the next one elsewhere. All lanes of a push go to ONE kernel(pieces, out) call (a constant
    number of launches, no per-lane concatenation); `kernel` is HipResampleKernel on the GPU, and the CPU tests drive
    the same bookkeeping with a torch restatement. A lane that ends is ready for a new utterance."""

    def __init__(self, lanes: int, orig_rate: int, new_rate: int, kernel: Callable | None = None, device=None):
        import torch
        if lanes < 1:
            raise ValueError("lanes >= 1")
        self.plan = resample_plan(orig_rate, new_rate)
        self.identity = self.plan[0] == self.plan[1]
        self.device = _device(device) if device is not None else torch.device("cpu")
        self.lanes = int(lanes)
        if kernel is None and not self.identity:
            kernel = HipResampleKernel(self.device, self.plan)
        self.kernel = kernel
        T = self.plan[3]
        self._carry = None if self.identity else torch.empty(2, self.lanes, T, dtype=torch.float32, device=self.device)
        self._side = [0] * self.lanes      # which of the two buffers holds the lane's carry
        self._n_carry = [0] * self.lanes
        self._recv = [0] * self.lanes      # I: input samples received
        self._emit = [0] * self.lanes      # output samples emitted
        self._keep = None                  # the last push's inputs, alive until its launches have run

    def received(self, lane: int) -> int:
        return self._recv[lane]

    def emitted(self, lane: int) -> int:
        return self._emit[lane]

    def reset(self, lane: int):
        self._n_carry[lane] = self._recv[lane] = self._emit[lane] = 0

    def flush(self, lanes: Iterable[int]) -> dict:
        return self.push({}, final=lanes)

    def push(self, chunks: dict, final: Iterable[int] = ()) -> dict:
        import torch
        final = set(final)
        order = sorted(set(chunks) | final)
        for lane in order:
            if not 0 <= lane < self.lanes:
                raise ValueError(f"lane {lane} outside [0, {self.lanes})")
        empty = torch.empty(0, dtype=torch.float32, device=self.device)
        flat = {lane: (chunks[lane].contiguous().view(-1) if lane in chunks else empty) for lane in order}
        for lane, c in flat.items():  # every chunk is checked before any lane's state changes
            if c.dtype != torch.float32:
                raise ValueError("chunks must be fp32")
            if c.device != self.device:  # the kernel would dereference its pointer on self.device
                raise ValueError(f"lane {lane}: the chunk is on {c.device}, the resampler on {self.device}")
        if self.identity:
            for lane in final:
                self.reset(lane)
            return {lane: c.view(1, 1, -1) for lane, c in flat.items()}
        o, n, W, T = self.plan
        pieces, after, total = [], {}, 0
        for lane in order:
            c, side, nc = flat[lane], self._side[lane], self._n_carry[lane]
            recv = self._recv[lane] + c.numel()
            ends = lane in final
            upto = out_len(recv, self.plan) if ends else emitted(recv, self.plan)
            j0, i0 = self._emit[lane], self._recv[lane] - nc
            # the first sample a later frame reads: frame upto / n starts W before upto / n * o
            keep = 0 if ends else recv - max(i0, (upto // n) * o - W, 0)
            pieces.append(Piece(self._carry[side, lane, :nc], c, i0, recv if ends else -1, j0, upto - j0, total,
                                self._carry[1 - side, lane, :keep]))
            total += upto - j0
            after[lane] = (recv, upto, keep, 1 - side)
        out = torch.empty(total, dtype=torch.float32, device=self.device)
        if self._carry.is_cuda:  # allocated at construction, maybe under another stream than the launches'
            self._carry.record_stream(torch.cuda.current_stream(self.device))
        self.kernel(pieces, out)
        for lane, state in after.items():  # committed once the launches are enqueued: a failed call changes nothing
            self._recv[lane], self._emit[lane], self._n_carry[lane], self._side[lane] = state
        self._keep = flat
        res = {p_lane: out[p.dst: p.dst + p.n_out].view(1, 1, -1) for p_lane, p in zip(order, pieces)}
        for lane in final:
            self.reset(lane)
        return res


__all__ = ["resample_plan", "emitted", "out_len", "table", "Piece", "HipResampleKernel", "GpuResampler",
           "StreamResampler", "MAX_TABLE_FLOATS"]
