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


def _snake1(strides, dilations, j: int, u: int) -> str:
    """The Snake alpha in front of residual unit u of block j; past the block's last unit, in front of what follows the
    block (the next block's transposed conv, or decoder.conv2). An activation is stored under the Snake of what
    reads it, so this is the alpha a stage's output is stored under."""
    if u < len(dilations):
        return f"decoder.block.{j}.res_unit{u + 1}.snake1.alpha"
    return f"decoder.block.{j + 1}.snake1.alpha" if j + 1 < len(strides) else "decoder.snake1.alpha"


def dac_stages(strides: Sequence[int], dilations: Sequence[int]) -> list:
    """The DAC decoder's launches (quantizer.from_codes + DacDecoder, modeling_dac.py:347-371, 407-441), stated once:
    one dict per launch, in order. Everything that runs or reasons about the decoder walks this list: decode() and
    the window decoders (DACAutoencoder._decode_lanes), the carried-state decoder (CarryLayout / CarryPlan,
    autoencoder._CarryState.run) and dac_lookahead_frames.

    kind: 'codes' (from_codes), 'k7' (conv of 7 taps at dilation d, padding 3 d: decoder.conv1 and a residual unit's
    first conv), 'convt' (ConvTranspose1d(k = 2 s, stride s, padding p = ceil(s / 2))), 'pw' (a unit's 1x1 conv plus
    the skip) or 'out' (decoder.conv2, k7, + tanh); block / unit where it belongs to one. src / dst / skip / raw name
    its activation buffers: dst holds the output under the Snake `alpha` (a DacModel state_dict key: the Snake of what
    reads it), raw the same rows before the Snake (the skip of the unit that follows; None where nothing follows in the
    block). `w` is the state_dict prefix of its .weight and .bias."""
    strides, dilations = tuple(strides), tuple(dilations)
    U = len(dilations)
    before = lambda j, u: (f"b{j}.x{u}", f"b{j}.h{u}") if u < U else (f"a{j + 1}", None)  # noqa: E731  (Snake'd, raw)
    stages = [dict(kind="codes", dst="z"),
              dict(kind="k7", d=1, src="z", dst="a0", w="decoder.conv1", alpha=_snake1(strides, dilations, -1, U))]
    x = "a0"
    for j, s in enumerate(strides):
        xu, hu = before(j, 0)
        stages.append(dict(kind="convt", s=s, p=math.ceil(s / 2), src=x, dst=xu, raw=hu, block=j,
                           w=f"decoder.block.{j}.conv_t1", alpha=_snake1(strides, dilations, j, 0)))
        for u, d in enumerate(dilations):
            unit, t = f"decoder.block.{j}.res_unit{u + 1}.", f"b{j}.t{u}"
            stages.append(dict(kind="k7", d=d, src=xu, dst=t, block=j, unit=u, w=unit + "conv1",
                               alpha=unit + "snake2.alpha"))
            xn, hn = before(j, u + 1)
            nxt = _snake1(strides, dilations, j, u + 1)
            stages.append(dict(kind="pw", src=t, skip=hu, dst=xn, raw=hn, block=j, unit=u, w=unit + "conv2", alpha=nxt))
            xu, hu = xn, hn
        x = xu
    stages.append(dict(kind="out", d=1, src=x, w="decoder.conv2"))
    return stages


def dac_lookahead_frames(strides: Sequence[int], dilations: Sequence[int]) -> int:
    """Frames of context the DAC decoder needs on either side of a frame (DacDecoder, modeling_dac.py:407-441).

    Walks the stage list backward from the output samples [0, hop) of frame 0, keeping the first and last index
    they depend on at each stage's input rate:
      Conv1d k7, dilation d, padding 3 d (the final conv, a residual unit's first conv, conv1): [lo - 3 d, hi + 3 d];
      the residual units' 1x1 convs and the Snakes: pointwise;
      ConvTranspose1d(k = 2 s, stride s, padding p = ceil(s / 2)): out[n] = sum_i x[i] w[n + p - i s] over
        0 <= n + p - i s < 2 s, so i is floor((n + p) / s) - 1 or floor((n + p) / s): [(lo + p) // s - 1, (hi + p) // s].
    At the code rate the interval is [-left, right] frames around frame 0; every frame sees the same one (the network
    is periodic in the hop), and the lookahead is the larger side.
    """
    lo, hi = 0, math.prod(strides) - 1
    for g in reversed(dac_stages(strides, dilations)):
        if g["kind"] in ("k7", "out"):
            lo, hi = lo - 3 * g["d"], hi + 3 * g["d"]
        elif g["kind"] == "convt":
            lo, hi = (lo + g["p"]) // g["s"] - 1, (hi + g["p"]) // g["s"]
    return max(-lo, hi)


DAC_LOOKAHEAD_FRAMES = dac_lookahead_frames(syn.DAC_STRIDES, syn.DAC_DILATIONS)


def _codes_2d(codes: torch.Tensor) -> torch.Tensor:
    """One utterance's pushed codes, [1, 9, n] or [9, n], as [9, n]."""
    if codes.dim() not in (2, 3) or codes.shape[-2] != N_CODEBOOKS or (codes.dim() == 3 and codes.shape[0] != 1):
        raise ValueError(f"codes must be [1, {N_CODEBOOKS}, n] or [{N_CODEBOOKS}, n]")
    return codes[0] if codes.dim() == 3 else codes


def _lane_codes(codes: dict, lanes: int) -> dict:
    """A batched push's {lane: codes} as {lane: [9, n]}: every lane's arguments are checked before any lane's state
    changes."""
    for lane in codes:
        if not 0 <= lane < lanes:
            raise ValueError(f"lane {lane} outside [0, {lanes})")
    return {lane: _codes_2d(c) for lane, c in codes.items()}


def _join(parts: list, device) -> torch.Tensor:
    """The waveforms of one call, joined: [1, 1, samples] (no parts: an empty waveform)."""
    if not parts:
        return torch.empty(1, 1, 0, dtype=torch.float32, device=device)
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)


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

    def _run(self, upto: int) -> torch.Tensor:
        parts = [self.decode_window(w, f0, f1) for w, f0, f1 in self._plan(upto)]
        self._advance(upto)
        return _join(parts, self.device)

    def _take(self, codes: torch.Tensor) -> int:
        """Append pushed codes; returns the frame up to which samples can now be emitted."""
        codes = _codes_2d(codes)
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
            out[lane] = _join(wavs[i: i + len(plan)], self.device)
            i += len(plan)
        return out

    @torch.inference_mode()
    def push(self, codes: dict) -> dict:
        """{lane: codes [9, n] or [1, 9, n] int64} -> {lane: [1, 1, 512 m] fp32}: per lane, the m frames whose right
        lookahead is now available (m may be 0)."""
        codes = _lane_codes(codes, len(self._lanes))
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


# ----------------------------------------------------------------------------------------------- carried state
# The incremental form of the same decoder: instead of a halo of R frames on both sides of every chunk, every stage
# keeps, per lane, the last rows of its input that it has not finished with, and a push of n frames advances every
# stage from its frontier as far as its input now allows. dac_lookahead_frames' interval arithmetic, run forward:
#   k7 conv, dilation d:   out row q reads in rows q - 3 d .. q + 3 d   -> frontier f_out = f_in - 3 d
#   1x1 conv + skip:       pointwise                                    -> the frontier of the k7 before it
#   ConvTranspose(s, p):   out row n reads in rows (n + p) // s - 1, (n + p) // s
#                                                                      -> f_out = s f_in - p (not a multiple of s)
# never below 0 (rows at negative positions are the zero padding: computing them would add the bias), and at the
# utterance's end every frontier is the stage's whole length (the rows past it are decode()'s right zero padding).
# A buffer's history is a FIXED number of rows below its frontier (zeros at an utterance's start: the zero state is
# the zero padding, every buffer holds post-Snake or raw values whose padding is 0): 6 d for a k7's input (its
# output lags 3 d behind and reads 3 d further back), 3 d for the skip it is added to, 1 for a transposed conv's
# input, and for the last conv's input what keeps frame recv - R computable.


class CarryBuffer:
    """One activation buffer of the incremental decoder: `rate` rows per code frame, `hist` carried rows; `width`
    names its channel count ('z', 'c1' or a block index: the planner knows shapes in rows only)."""

    def __init__(self, name: str, rate: int, hist: int, width):
        self.name, self.rate, self.hist, self.width = name, int(rate), int(hist), width

    def __repr__(self):
        return f"CarryBuffer({self.name}, rate {self.rate}, hist {self.hist})"


class CarryLayout:
    """The decoder's stage list (dac_stages) with a CarryBuffer for every buffer it names, and the planner over it.

    k7_short (a k7 stage's index) and convt_frontier_pad=False build the two wrong plans the tests must reject: one
    row less history at that stage, and a transposed-conv frontier of s F instead of s F - p."""

    def __init__(self, strides: Sequence[int], dilations: Sequence[int], lookahead: int | None = None,
                 k7_short: int | None = None, convt_frontier_pad: bool = True):
        self.strides, self.dilations = tuple(strides), tuple(dilations)
        self.hop = math.prod(self.strides)
        self.R = dac_lookahead_frames(strides, dilations) if lookahead is None else int(lookahead)
        self.convt_frontier_pad = bool(convt_frontier_pad)
        if not self.strides or not self.dilations:
            raise ValueError("at least one block and one residual unit")
        self.stages = stages = dac_stages(strides, dilations)
        # every stage's outputs as buffers at its rate, each with the history its reader needs (above)
        self.buffers, rate = {}, 1
        for g in stages:
            k = g["kind"]
            if k in ("k7", "out"):
                d = g["d"]
                self.buffers[g["src"]].hist = 6 * d
            elif k == "convt":
                self.buffers[g["src"]].hist = 1
                rate *= g["s"]
            elif k == "pw":
                self.buffers[g["skip"]].hist = 3 * d  # the dilation of the unit's k7
            for name in (g.get("dst"), g.get("raw")):
                if name:
                    self.buffers[name] = CarryBuffer(name, rate, 0, "z" if k == "codes" else g.get("block", "c1"))
        self.last = x = stages[-1]["src"]
        # the last conv emits whole frames, up to frame recv - R: its input's history reaches from that frame's first
        # sample (less the conv's 3 rows) to the input's frontier, whose lag behind hop * recv is a constant
        big = 4 * self.R + 64
        lag = self.hop * big - self._frontiers(big, False)[x]
        if self.convt_frontier_pad:
            assert 0 <= lag + 3 <= self.hop * self.R, "the lookahead does not cover the stages' lag"
        self.buffers[x].hist = max(self.hop * self.R - lag, 0) + 3
        if k7_short is not None:
            st = [g for g in stages if g["kind"] in ("k7", "out")][k7_short]
            self.buffers[st["src"]].hist -= 1
        self._short = k7_short is not None
        self._plans: dict = {}
        r = self.R
        while min(self._frontiers(r, False).values()) <= 0:
            r += 1
        self._steady_from = r
        self.k7_stages = sum(g["kind"] in ("k7", "out") for g in stages)  # the last conv is a k7 too

    # ------------------------------------------------------------------------------------------ frontiers
    def _frontiers(self, recv: int, final: bool) -> dict:
        """{buffer: rows [0, f) valid} with `recv` frames received (final: the utterance is recv frames long)."""
        f = {}
        for g in self.stages:
            k = g["kind"]
            if k == "codes":
                f[g["dst"]] = recv
            elif k == "k7":
                fi = f[g["src"]]
                f[g["dst"]] = fi if final else max(fi - 3 * g["d"], 0)
            elif k == "pw":
                f[g["dst"]] = f[g["src"]]
                if g["raw"]:
                    f[g["raw"]] = f[g["src"]]
            elif k == "convt":
                fi = f[g["src"]]
                fo = g["s"] * fi if final else max(g["s"] * fi - (g["p"] if self.convt_frontier_pad else 0), 0)
                f[g["dst"]] = fo
                if g["raw"]:
                    f[g["raw"]] = fo
        return f

    def emitted(self, recv: int, final: bool) -> int:
        """Frames whose samples have been returned once `recv` frames are in: all up to recv - R (at the end: all)."""
        return recv if final else max(recv - self.R, 0)

    def plan(self, recv: int, n: int, final: bool = False) -> "CarryPlan":
        """The launch sequence of a push of n more frames after `recv` (final: they end the utterance)."""
        if recv < 0 or n < 0:
            raise ValueError("recv >= 0 and n >= 0")
        return CarryPlan(self, recv, n, final)

    def step_plan(self, recv: int, n: int, final: bool = False) -> "CarryPlan":
        """plan() for the launch sequence alone, kept: once every stage's frontier has left 0 and frames are being
        emitted, a push's launches (row counts, offsets into [hist | new], tails: CarryPlan.key) no longer depend on
        the position, so every later push takes the plan of the first such position (its absolute rows are that
        position's)."""
        key = (min(recv, self._steady_from), n, bool(final))
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = self.plan(*key).check() if self.convt_frontier_pad and not self._short \
                else self.plan(*key)
        return plan


class CarryPlan:
    """What one push computes. Per buffer b: prev[b] / now[b] its frontier before / after, new[b] = now - prev the rows
    appended, and its scratch is [hist | new] rows whose row 0 is absolute row base[b] = prev[b] - hist. Per stage
    (self.steps, the layout's stages in order) a dict with
      out0, n_out     first output row (absolute) and row count (the stage's dst rows prev .. now);
      lo, hi          absolute input rows read, [lo, hi) (k7: out0 - 3 d .. out0 + n_out + 3 d; convt: (out0 + p) // s - 1
                      .. (out0 + n_out - 1 + p) // s + 1), of which rows below prev[src] come from the history and the
                      rest are new; rows at or past now[src] are read only at the utterance's end (zero padding);
      in_off          the local row of src's scratch that output row 0 reads first (k7: out0 - 3 d - base); skip_off
                      the same for a 1x1 conv's skip; n0 (convt) the first output row counted from s * base[src], the
                      transposed conv's row 0 of an input that starts at src's scratch;
      tail            {buffer: local first row} of the `hist` rows to keep for the next push: rows new .. new + hist.
    key: the tuple that decides every launch's shape (two pushes of equal key are one launch sequence's lanes)."""

    def __init__(self, lay: CarryLayout, recv: int, n: int, final: bool):
        self.layout, self.recv, self.n, self.final, self.first = lay, recv, n, bool(final), recv == 0
        self.prev = lay._frontiers(recv, False)
        self.now = lay._frontiers(recv + n, final)
        B = lay.buffers
        self.new = {b: self.now[b] - self.prev[b] for b in B}
        self.base = {b: self.prev[b] - B[b].hist for b in B}
        self.emit0, self.emit1 = lay.emitted(recv, False), lay.emitted(recv + n, final)
        steps = []
        for g in lay.stages:
            k = g["kind"]
            st = dict(g)
            if k == "codes":
                st.update(out0=recv, n_out=n)
            elif k == "out":
                src = g["src"]
                st.update(out0=lay.hop * self.emit0, n_out=lay.hop * (self.emit1 - self.emit0))
                st.update(lo=st["out0"] - 3, hi=st["out0"] + st["n_out"] + 3, in_off=st["out0"] - 3 - self.base[src])
            else:
                dst, src = g["dst"], g["src"]
                st.update(out0=self.prev[dst], n_out=self.new[dst])
                if k == "k7":
                    d = g["d"]
                    st.update(lo=st["out0"] - 3 * d, hi=st["out0"] + st["n_out"] + 3 * d,
                              in_off=st["out0"] - 3 * d - self.base[src])
                elif k == "pw":
                    st.update(lo=st["out0"], hi=st["out0"] + st["n_out"], in_off=0,
                              skip_off=st["out0"] - self.base[g["skip"]])
                else:
                    s, p = g["s"], g["p"]
                    st.update(lo=(st["out0"] + p) // s - 1, hi=(st["out0"] + st["n_out"] - 1 + p) // s + 1,
                              n0=st["out0"] - s * self.base[src])
            steps.append(st)
        self.steps = steps
        self.tail = {b: self.new[b] for b in B if B[b].hist}
        self.key = (self.first, self.final, tuple((st.get("in_off", 0), st.get("skip_off", 0), st.get("n0", 0),
                                                   st["n_out"]) for st in steps))

    def rows(self, name: str) -> int:
        """Rows of a buffer's [hist | new] scratch."""
        return self.layout.buffers[name].hist + self.new[name]

    def check(self):
        """Every row a stage reads is in its source's [hist | new] and, unless the utterance ends, below the source's
        frontier; no row at a negative position is computed."""
        for st in self.steps:
            if st["kind"] == "codes" or st["n_out"] == 0:
                continue
            assert st["out0"] >= 0, st
            srcs = [(st["src"], st["lo"], st["hi"])]
            if st["kind"] == "pw":
                srcs.append((st["skip"], st["out0"], st["out0"] + st["n_out"]))
            for b, lo, hi in srcs:
                assert lo >= self.base[b], (st, b, lo, self.base[b])
                assert hi <= self.now[b] or self.final, (st, b, hi, self.now[b])
        return self


class _OneLane:
    """A single lane's decode_step as the decode_steps of a one-lane DACCarryBatchStreamDecoder."""

    def __init__(self, decode_step):
        self.decode_step = decode_step

    def __call__(self, plan, ids, codes) -> list:
        return [self.decode_step(plan, codes[0])]

    def reset(self, lane: int):
        self.decode_step.reset()


class DACCarryStreamDecoder:
    """DACStreamDecoder's surface on the carried-state decoder: push() returns the frames up to recv - R, flush() the
    rest, concatenated bit for bit decode() of all the codes; a push costs its own frames, not a window's. It is the
    one-lane case of DACCarryBatchStreamDecoder.

    decode_step(plan, codes [9, n] int64) -> [1, 1, hop (emit1 - emit0)] fp32 runs one CarryPlan on the lane's state
    (DACAutoencoder.stream_decoder(carry=True) supplies the HIP one, the CPU tests a restatement); it has reset() (the
    state is zero again) and snapshot() / restore(s) (stream()'s rollback of a push past the utterance's end)."""

    def __init__(self, decode_step, layout: CarryLayout, chunk_frames: int = 16, device=None):
        self._lane = DACCarryBatchStreamDecoder(_OneLane(decode_step), layout, 1, chunk_frames, device)
        self.decode_step, self.layout = decode_step, layout
        self.chunk, self.R, self.device = self._lane.chunk, self._lane.R, self._lane.device

    frames_received = property(lambda self: self._lane.frames_received(0))
    frames_emitted = property(lambda self: self._lane.frames_emitted(0))

    def _reset(self):
        self._lane.reset(0)

    def _state(self):
        recv = self.frames_received
        return recv, (self.decode_step.snapshot() if recv else None)

    def _restore(self, state):
        self._lane._recv[0], snap = state
        if snap is None:
            self.decode_step.reset()
        else:
            self.decode_step.restore(snap)

    def push(self, codes: torch.Tensor) -> torch.Tensor:
        """codes [1, 9, n] or [9, n] int64 (n >= 0) -> [1, 1, hop m] fp32: the m frames whose right lookahead is now
        available (m may be 0)."""
        return self._lane.push({0: codes})[0]

    def flush(self) -> torch.Tensor:
        """The utterance has ended: the samples of the frames not yet emitted. The decoder is then ready for a new one."""
        return self._lane.flush([0])[0]


class DACCarryBatchStreamDecoder:
    """DACBatchStreamDecoder's surface on the carried-state decoder: `lanes` independent utterances, each with a state
    of its own; the lanes of a call whose plans have one key (in the steady state: equal n) go to ONE call of

        decode_steps(plan, lane ids, list of codes [9, n] int64) -> list of [1, 1, hop m] fp32

    which also has reset(lane). Per lane the returns are exactly a DACCarryStreamDecoder's for the same pushes."""

    def __init__(self, decode_steps, layout: CarryLayout, lanes: int, chunk_frames: int = 16, device=None):
        if lanes < 1 or chunk_frames < 1:
            raise ValueError("lanes >= 1 and chunk_frames >= 1")
        self.decode_steps, self.layout = decode_steps, layout
        self.chunk, self.R = int(chunk_frames), layout.R
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self._recv = [0] * int(lanes)

    @property
    def lanes(self) -> int:
        return len(self._recv)

    def frames_received(self, lane: int) -> int:
        return self._recv[lane]

    def frames_emitted(self, lane: int) -> int:
        return self.layout.emitted(self._recv[lane], False)

    def _run(self, codes: dict, final: bool) -> dict:
        """A push goes in pieces of at most chunk_frames (as the window decoder emits chunk_frames at a time): a long
        one, an audio prefix for instance, takes a chunk's scratch, and its whole chunks the steady-state step. The
        lanes' i-th pieces of one plan key are one decode_steps call."""
        parts = {lane: [] for lane in codes}
        a = 0
        while True:
            groups = {}
            for lane, c in codes.items():
                n = c.shape[1]
                if a >= max(n, 1) or (n == 0 and not (final and self._recv[lane])):
                    continue
                k = min(self.chunk, n - a)
                plan = self.layout.step_plan(self._recv[lane], k, final)
                g = groups.setdefault(plan.key, (plan, [], []))
                g[1].append(lane)
                g[2].append(c[:, a: a + k])
                self._recv[lane] += k
            if not groups:
                break
            for plan, ids, cs in groups.values():
                wavs = list(self.decode_steps(plan, ids, cs))
                if len(wavs) != len(ids):
                    raise RuntimeError(f"decode_steps returned {len(wavs)} waveforms for {len(ids)} lanes")
                for lane, w in zip(ids, wavs):
                    parts[lane].append(w)
            a += self.chunk
        return {lane: _join(p, self.device) for lane, p in parts.items()}

    @torch.inference_mode()
    def push(self, codes: dict) -> dict:
        """{lane: codes [9, n] or [1, 9, n] int64} -> {lane: [1, 1, hop m] fp32}: per lane, the m frames whose right
        lookahead is now available (m may be 0)."""
        codes = _lane_codes(codes, len(self._recv))
        return self._run({lane: c.to(self.device, torch.int64) for lane, c in codes.items()}, False)

    @torch.inference_mode()
    def flush(self, lanes) -> dict:
        """These lanes' utterances have ended: {lane: the samples of its frames not yet emitted}. The lanes are then
        ready for new utterances."""
        lanes = list(lanes)
        empty = torch.empty(N_CODEBOOKS, 0, dtype=torch.int64, device=self.device)
        out = self._run({lane: empty for lane in lanes}, True)
        for lane in lanes:
            self.reset(lane)
        return out

    def reset(self, lane: int):
        """Drop a lane's utterance without decoding what is left of it: its state is zero again."""
        self._recv[lane] = 0
        self.decode_steps.reset(lane)


__all__ = ["dac_stages", "dac_lookahead_frames", "DAC_LOOKAHEAD_FRAMES", "DACStreamDecoder", "DACBatchStreamDecoder",
           "DAC_HOP", "CarryBuffer", "CarryLayout", "CarryPlan", "DACCarryStreamDecoder", "DACCarryBatchStreamDecoder"]
