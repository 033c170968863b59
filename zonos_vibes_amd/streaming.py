"""Streaming DAC decode: the decoder's lookahead and the window / crop bookkeeping of DACStreamDecoder.

The DAC decoder is not causal: the 512 samples of code frame t depend on frames t - R .. t + R. R follows from the
layer list (dac_lookahead_frames), so a frame can be decoded as soon as R frames to its right are known: a window
of frames [a - R, b + R), clipped to the utterance, is decoded like a short utterance and only the samples of [a, b)
are kept. Where the window is clipped, its zero padding is the offline decode's own; where it is not, the R-frame
halo keeps the window's padding out of the kept samples. This module has no GPU dependency: the scheduling runs over
a `decode_window` callable (DACAutoencoder.stream_decoder supplies the HIP one, the CPU tests a restatement).
"""
from __future__ import annotations

import math
from typing import Callable, Sequence

import torch

from . import synthetic as syn
from .config import DAC_HOP, N_CODEBOOKS


def dac_lookahead_frames(strides: Sequence[int], dilations: Sequence[int]) -> int:
    """Frames of context the DAC decoder needs on either side of a frame (DacDecoder, modeling_dac.py:407-441).

    Walks the layer list backward from the output samples [0, hop) of frame 0, keeping the first and last index
    they depend on at each layer's input rate:
      Conv1d k7, dilation d, padding 3 d (the final conv, a residual unit's first conv, conv1): [lo - 3 d, hi + 3 d];
      the residual units' 1x1 convs and the Snakes: pointwise;
      ConvTranspose1d(k = 2 s, stride s, padding p = ceil(s / 2)): out[n] = sum_i x[i] w[n + p - i s] over
        0 <= n + p - i s < 2 s, so i is floor((n + p) / s) - 1 or floor((n + p) / s): [(lo + p) // s - 1, (hi + p) // s].
    At the code rate the interval is [-left, right] frames around frame 0; every frame sees the same one (the network
    is periodic in the hop), and the lookahead is the larger side.
    """
    lo, hi = 0, math.prod(strides) - 1
    lo, hi = lo - 3, hi + 3                      # decoder.conv2 (k7)
    for s in reversed(list(strides)):
        for d in dilations:                      # three residual units: k7 at dilation d, then 1x1
            lo, hi = lo - 3 * d, hi + 3 * d
        p = math.ceil(s / 2)
        lo, hi = (lo + p) // s - 1, (hi + p) // s
    lo, hi = lo - 3, hi + 3                      # decoder.conv1 (k7)
    return max(-lo, hi)


DAC_LOOKAHEAD_FRAMES = dac_lookahead_frames(syn.DAC_STRIDES, syn.DAC_DILATIONS)


class DACStreamDecoder:
    """Incremental DACAutoencoder.decode: push() code frames as they become final, flush() at the utterance's end;
    the concatenated returns equal decode() of all the codes.

    decode_window(codes [9, W] int64, f0, f1) -> [1, 1, 512 (f1 - f0)] fp32 decodes a W-frame window as an utterance
    of its own and returns the samples of its frames f0 .. f1 - 1. Frames are emitted `chunk_frames` at a time (the
    steady-state window is lookahead + chunk_frames + lookahead frames, one fixed shape), the rest of what a push
    made available in one shorter window.
    """

    def __init__(self, decode_window: Callable[[torch.Tensor, int, int], torch.Tensor], chunk_frames: int = 16,
                 lookahead: int = DAC_LOOKAHEAD_FRAMES, device=None):
        if chunk_frames < 1 or lookahead < 0:
            raise ValueError("chunk_frames >= 1 and lookahead >= 0")
        self.decode_window = decode_window
        self.chunk = int(chunk_frames)
        self.R = int(lookahead)
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self._reset()

    def _reset(self):
        self._held = None   # [9, n] codes of frames _base .. _recv - 1
        self._base = 0
        self._recv = 0      # frames pushed so far
        self._emit = 0      # frames whose samples have been returned

    def _state(self):
        """A rollback point (the held codes are never written in place)."""
        return self._held, self._base, self._recv, self._emit

    def _restore(self, state):
        self._held, self._base, self._recv, self._emit = state

    @property
    def frames_received(self) -> int:
        return self._recv

    @property
    def frames_emitted(self) -> int:
        return self._emit

    def _windows(self, upto: int, end: int):
        """Emit frames _emit .. upto - 1 with the utterance known up to frame `end`: (lo, hi, a, b) per window."""
        out = []
        a = self._emit
        while a < upto:
            b = min(a + self.chunk, upto)
            out.append((max(a - self.R, 0), min(b + self.R, end), a, b))
            a = b
        return out

    def _plan(self, upto: int):
        """The decode_window arguments (codes [9, W], f0, f1) that emit frames _emit .. upto - 1."""
        return [(self._held[:, lo - self._base: hi - self._base], a - lo, b - lo)
                for lo, hi, a, b in self._windows(upto, self._recv)]

    def _advance(self, upto: int):
        if upto > self._emit:
            self._emit = upto
            keep = max(self._emit - self.R, 0)  # the next window's left halo
            if keep > self._base:
                self._held = self._held[:, keep - self._base:]
                self._base = keep

    def _join(self, parts) -> torch.Tensor:
        if not parts:
            return torch.empty(1, 1, 0, dtype=torch.float32, device=self.device)
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)

    def _run(self, upto: int) -> torch.Tensor:
        parts = [self.decode_window(w, f0, f1) for w, f0, f1 in self._plan(upto)]
        self._advance(upto)
        return self._join(parts)

    def _take(self, codes: torch.Tensor) -> int:
        """Append pushed codes; returns the frame up to which samples can now be emitted."""
        if codes.dim() == 3:
            if codes.shape[0] != 1:
                raise ValueError("DACStreamDecoder decodes one utterance: codes [1, 9, n] or [9, n]")
            codes = codes[0]
        if codes.dim() != 2 or codes.shape[0] != N_CODEBOOKS:
            raise ValueError(f"codes must be [1, {N_CODEBOOKS}, n] or [{N_CODEBOOKS}, n]")
        if codes.shape[1]:
            codes = codes.to(self.device, torch.int64)
            self._held = codes if self._held is None or self._held.shape[1] == 0 else torch.cat([self._held, codes], 1)
            self._recv += codes.shape[1]
        return max(self._recv - self.R, self._emit)

    @torch.inference_mode()
    def push(self, codes: torch.Tensor) -> torch.Tensor:
        """codes [1, 9, n] or [9, n] int64 (n >= 0) -> [1, 1, 512 m] fp32: the m frames whose right lookahead is now
        available (m may be 0)."""
        return self._run(self._take(codes))

    @torch.inference_mode()
    def flush(self) -> torch.Tensor:
        """The utterance has ended: the samples of the frames not yet emitted. The decoder is then ready for a new one."""
        out = self._run(self._recv)
        self._reset()
        return out


class DACBatchStreamDecoder:
    """`lanes` independent DACStreamDecoders whose windows are decoded together: every lane keeps a DACStreamDecoder's
    held / base / recv / emit state and its `_windows` rule, and all the windows one push() or flush() call makes
    due, over all its lanes, go to ONE call of

        decode_windows(list of (codes [9, W] int64, f0, f1)) -> list of [1, 1, 512 (f1 - f0)] fp32

    so the GPU side can decode windows of equal shape in one launch sequence (DACAutoencoder.stream_decoder_batch).
    Per lane, the concatenated returns are exactly what a DACStreamDecoder of its own returns for the same pushes.
    """

    def __init__(self, decode_windows: Callable[[list], list], lanes: int, chunk_frames: int = 16,
                 lookahead: int = DAC_LOOKAHEAD_FRAMES, device=None):
        if lanes < 1:
            raise ValueError("lanes >= 1")
        self.decode_windows = decode_windows
        self._lanes = [DACStreamDecoder(None, chunk_frames, lookahead, device) for _ in range(int(lanes))]
        self.chunk, self.R, self.device = self._lanes[0].chunk, self._lanes[0].R, self._lanes[0].device

    @property
    def lanes(self) -> int:
        return len(self._lanes)

    def frames_received(self, lane: int) -> int:
        return self._lanes[lane].frames_received

    def frames_emitted(self, lane: int) -> int:
        return self._lanes[lane].frames_emitted

    def _run(self, upto: dict) -> dict:
        """upto {lane: frame}: emit every lane's frames up to its frame, all windows in one decode_windows call."""
        plans = {lane: self._lanes[lane]._plan(u) for lane, u in upto.items()}
        flat = [w for lane in plans for w in plans[lane]]
        wavs = list(self.decode_windows(flat)) if flat else []
        if len(wavs) != len(flat):
            raise RuntimeError(f"decode_windows returned {len(wavs)} waveforms for {len(flat)} windows")
        out, i = {}, 0
        for lane, plan in plans.items():
            dec = self._lanes[lane]
            dec._advance(upto[lane])
            out[lane] = dec._join(wavs[i: i + len(plan)])
            i += len(plan)
        return out

    @torch.inference_mode()
    def push(self, codes: dict) -> dict:
        """{lane: codes [9, n] or [1, 9, n] int64} -> {lane: [1, 1, 512 m] fp32}: per lane, the m frames whose right
        lookahead is now available (m may be 0)."""
        for lane, c in codes.items():  # every lane's arguments are checked before any lane's state changes
            if not 0 <= lane < len(self._lanes):
                raise ValueError(f"lane {lane} outside [0, {len(self._lanes)})")
            if c.dim() not in (2, 3) or c.shape[-2] != N_CODEBOOKS or (c.dim() == 3 and c.shape[0] != 1):
                raise ValueError(f"codes must be [1, {N_CODEBOOKS}, n] or [{N_CODEBOOKS}, n]")
        return self._run({lane: self._lanes[lane]._take(c) for lane, c in codes.items()})

    @torch.inference_mode()
    def flush(self, lanes) -> dict:
        """These lanes' utterances have ended: {lane: the samples of its frames not yet emitted}. The lanes are then
        ready for new utterances."""
        lanes = list(lanes)
        out = self._run({lane: self._lanes[lane]._recv for lane in lanes})
        for lane in lanes:
            self._lanes[lane]._reset()
        return out

    def reset(self, lane: int):
        """Drop a lane's utterance without decoding what is left of it."""
        self._lanes[lane]._reset()


__all__ = ["dac_lookahead_frames", "DAC_LOOKAHEAD_FRAMES", "DACStreamDecoder", "DACBatchStreamDecoder", "DAC_HOP"]
