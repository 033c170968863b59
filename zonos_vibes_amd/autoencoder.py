"""DACAutoencoder with the reference's decode() surface (zonos/autoencoder.py:8-27), on HIP kernels.

The decoder path is on the hot path: quantizer.from_codes + DacDecoder. Its launches are
stated once, as streaming.dac_stages; the weights are bound to that list at load, and two host walks run it:
_decode_lanes (decode() and the window decoders, in four stage buffers reused in place) and _CarryState.run (the
carried-state decoder, on [hist | new] scratch). `encode` (voice-clone audio prefix) runs
DacEncoder + the residual VQ on the same MFMA conv kernel (strided convs in polyphase form) plus a VQ kernel;
`preprocess` resamples to 44.1 kHz on the GPU (zmi_resample, resampling.py) and pads to a multiple of 512 samples.

Weights use transformers' DacModel state_dict names (quantizer.quantizers.{i}.*, decoder.*);
weight-norm pairs (weight_g / weight_v, or parametrizations.weight.original0 / original1) are
folded to plain weights at load time.
"""
from __future__ import annotations

import ctypes
import math
from types import SimpleNamespace

import torch

from . import _lib
from . import synthetic as syn
from .config import DAC_HOP, DAC_SAMPLE_RATE, N_CODEBOOKS
from .resampling import GpuResampler, StreamResampler, resample_plan
from .streaming import (DAC_LOOKAHEAD_FRAMES, CarryLayout, DACBatchStreamDecoder, DACCarryBatchStreamDecoder,  # noqa: F401
                        DACCarryStreamDecoder, DACStreamDecoder, dac_lookahead_frames, dac_stages)

STRIDES = syn.DAC_STRIDES
ENC_STRIDES = syn.DAC_ENC_STRIDES
DILATIONS = syn.DAC_DILATIONS


def _fold_weight_norm(sd: dict) -> dict:
    """Plain conv weights from weight-norm pairs, in either of the two key styles a DAC state_dict
    can carry: `x.weight_g` / `x.weight_v` (torch.nn.utils.weight_norm, the published checkpoint)
    or `x.parametrizations.weight.original0` / `.original1` (torch.nn.utils.parametrizations.weight_norm,
    what transformers' DacModel.apply_weight_norm registers): weight = g * v / ||v|| over all dims
    but the first (dim=0, torch's default)."""
    out = dict(sd)
    for gk, vk, base in [(k, k[: -len("_g")] + "_v", k[: -len(".weight_g")]) for k in sd if k.endswith(".weight_g")] + \
            [(k, k[: -1] + "1", k[: -len(".parametrizations.weight.original0")])
             for k in sd if k.endswith(".parametrizations.weight.original0")]:
        g, v = sd[gk].float(), sd[vk].float()
        norm = v.flatten(1).norm(dim=1).view(-1, *([1] * (v.dim() - 1)))
        out[base + ".weight"] = g * v / norm
        del out[gk], out[vk]
    return out


def _blocked(w: torch.Tensor) -> torch.Tensor:
    """[..., co, ci] conv weights -> fp16 channel-blocked [..., ci / 32, co, 32]: the layout zmi_dac_conv* read for
    convs with more than one tap, in which one 32-channel step of 16 output channels (one LDS-DMA piece, 16 x 64 B)
    is 1 KiB contiguous (1x1 convs keep [co][ci], include/zonos_hip.h)."""
    co, ci = w.shape[-2], w.shape[-1]
    assert ci % 32 == 0, ci
    return w.reshape(*w.shape[:-1], ci // 32, 32).transpose(-3, -2).contiguous().half()


def pack_conv(w: torch.Tensor) -> torch.Tensor:
    """Conv1d weight [co][ci][k] -> what zmi_dac_conv reads: channel-blocked [k][ci / 32][co][32] fp16 (_blocked),
    or [1][co][ci] for a 1x1 conv."""
    w = w.to(torch.float32).permute(2, 0, 1)
    return w.contiguous().half() if w.shape[0] == 1 else _blocked(w)


def pack_conv_transpose(wt: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    """ConvTranspose1d(k = 2 stride, stride, padding = pad) weight [ci][co][2 stride] -> zmi_dac_conv_t's polyphase
    weights [stride][2][ci / 32][co][32] fp16: phase rho uses taps (rho + pad) % stride and + stride, transposed."""
    wt = wt.to(torch.float32)
    assert wt.shape[2] == 2 * stride, (wt.shape, stride)
    phases = []
    for rho in range(stride):
        k0 = (rho + pad) % stride
        phases.append(torch.stack([wt[:, :, k0].t(), wt[:, :, k0 + stride].t()]))  # [2][cout][cin]
    return _blocked(torch.stack(phases))


def pack_strided_conv(wt: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    """Conv1d(c, co, k = 2 s, stride s, padding = pad) weight [co][c][2 s] -> a stride-1, 3-tap conv (in_off -1) over
    the polyphase view x'[t][j*c + ci] = x[s t + j][ci]: out[t] = sum_{a=-1..1} W'[a] x'[t + a] with
    W'[a][co][j*c + ci] = W[co][ci][s a + j + pad] (0 if that tap is outside [0, 2s)); blocked [3][s c / 32][co][32]."""
    wt = wt.to(torch.float32)
    co, c, k2 = wt.shape
    s = stride
    assert k2 == 2 * s, (wt.shape, stride)
    wp = torch.zeros(3, co, s, c, device=wt.device)
    for a in range(3):
        for jj in range(s):
            k = s * (a - 1) + jj + pad
            if 0 <= k < 2 * s:
                wp[a, :, jj, :] = wt[:, :, k]
    return _blocked(wp.reshape(3, co, s * c))


def pack_conv_out(w2: torch.Tensor, b2: torch.Tensor):
    """decoder.conv2 (Conv1d(ci, 1, k7)) weight [1][ci][7] and bias [1] -> zmi_dac_conv_out's 32-channel tile:
    weights [7][ci / 32][32][32] fp16 with output channel 0 the filter and 1..31 zero, bias f32 [32]."""
    w2 = w2.to(torch.float32)
    w = torch.zeros(w2.shape[2], 32, w2.shape[1], device=w2.device)  # [k][co padded to 32][ci]
    w[:, 0, :] = w2[0].t()
    b = torch.zeros(32, device=w2.device)
    b[0] = b2.to(torch.float32).reshape(-1)[0]
    return _blocked(w), b


def pack_im2col_conv1(w1: torch.Tensor) -> torch.Tensor:
    """encoder.conv1 (Conv1d(1, co, k7)) weight [co][1][7] -> the 1x1 weight [1][co][32] fp16 over zmi_dac_im2col7's
    rows (taps 0..6 in columns 0..6, the rest zero)."""
    w1 = w1.to(torch.float32)
    col = torch.zeros(1, w1.shape[0], 32, device=w1.device)
    col[0, :, :w1.shape[2]] = w1[:, 0, :]
    return col.half().contiguous()


# The steady-state streaming window as one hipGraph replay instead of its 31 launches (tools/bench_stream.py
# measures both)
WINDOW_GRAPH = True

STAGE_HALFS_PER_FRAME = 49152  # max over stages of C x time per code frame (blocks 3 and 4: 192 x 256 = 96 x 512)


class _Grow:
    """`count` fp16 device buffers that grow on demand, the old ones freed before the larger ones are allocated."""

    def __init__(self, dev, count: int):
        self.dev, self.count, self.bufs = dev, count, None

    def __call__(self, halfs: int) -> list:
        if self.bufs is None or self.bufs[0].numel() < halfs:
            self.bufs = None
            self.bufs = [torch.empty(halfs, dtype=torch.float16, device=self.dev) for _ in range(self.count)]
        return self.bufs


class _OnStream:
    """The stream hand-off: the autoencoder's stream waits for the caller's, the body runs on it, and the caller's
    stream waits for it. Yields a list: the tensors the body puts there were allocated on the autoencoder's stream and
    are handed to the caller's (record_stream). (A class: a generator-based context manager costs every replay of a
    captured window a microsecond more.)"""
    __slots__ = ("ae", "cur", "ctx", "made")

    def __init__(self, ae: "DACAutoencoder"):
        self.ae = ae

    def __enter__(self) -> list:
        self.cur = torch.cuda.current_stream(self.ae.dev)
        self.ae.stream.wait_stream(self.cur)
        self.ctx = torch.cuda.stream(self.ae.stream)
        self.ctx.__enter__()
        self.made = []
        return self.made

    def __exit__(self, *exc):
        self.ctx.__exit__(*exc)
        if exc[0] is None:
            self.cur.wait_stream(self.ae.stream)
            for t in self.made:
                t.record_stream(self.cur)


class _WindowDecoder:
    """DACStreamDecoder's decode_window on the HIP decoder: a window is decoded by _decode_lanes' launch sequence at
    one lane, in stage buffers of its own (a captured graph keeps their addresses), and the last stage computes only
    the kept samples, so the crop costs no copy of the window and no host sync."""

    def __init__(self, ae: "DACAutoencoder", chunk_frames: int, capture: bool):
        self.ae, self.chunk, self.R, self.capture = ae, int(chunk_frames), DAC_LOOKAHEAD_FRAMES, bool(capture)
        self.wmax = 2 * self.R + self.chunk
        self._bufs = _Grow(ae.dev, 4)
        self._graph = None
        self.graph_replays = 0
        self.frames_computed = 0  # code frames decoded (a window's halo frames count)

    def __call__(self, codes: torch.Tensor, f0: int, f1: int) -> torch.Tensor:
        ae = self.ae
        W = codes.shape[1]
        assert 0 <= f0 < f1 <= W <= self.wmax, (f0, f1, W)
        self.frames_computed += W
        crop = (DAC_HOP * f0, DAC_HOP * (f1 - f0))
        with ae.on_stream() as made:
            bufs = self._bufs(STAGE_HALFS_PER_FRAME * self.wmax)
            if self.capture and W == self.wmax and f0 == self.R and f1 == self.R + self.chunk:
                if self._graph is None:
                    self._gcodes = torch.zeros(1, N_CODEBOOKS, self.wmax, dtype=torch.int64, device=ae.dev)
                    self._gout = torch.empty(1, crop[1], dtype=torch.float32, device=ae.dev)
                    self._graph = _lib.Graph(ae.sptr)
                self._gcodes[0].copy_(codes)
                self._graph.launch(lambda: ae._decode_lanes(self._gcodes, self._gout, bufs, crop))
                self.graph_replays += 1
                out = self._gout.clone()
            else:
                out = torch.empty(1, crop[1], dtype=torch.float32, device=ae.dev)
                ae._decode_lanes(codes.contiguous()[None], out, bufs, crop)
            made.append(out)
        return out.view(1, 1, -1)


class _BatchWindowDecoder:
    """DACBatchStreamDecoder's decode_windows on the HIP decoder: the windows of a call are grouped by shape
    (W, f0, f1) and each group of two or more is ONE _decode_lanes launch sequence over all its lanes (a group of
    one goes through _WindowDecoder, the single-utterance path stream() runs). Stage buffers hold the lanes in use
    and grow on demand. The launches are not captured: a graph per lane count measured no faster on the wall at any
    lane count (7.35 ms replayed against 7.18 ms launched at 64 lanes), and without one a group
    decodes exactly its lanes, with no padding to a captured size."""

    def __init__(self, ae: "DACAutoencoder", max_lanes: int, chunk_frames: int):
        self.ae, self.max_lanes, self.chunk, self.R = ae, int(max_lanes), int(chunk_frames), DAC_LOOKAHEAD_FRAMES
        self.wmax = 2 * self.R + self.chunk
        self.single = _WindowDecoder(ae, chunk_frames, WINDOW_GRAPH)
        self._bufs = _Grow(ae.dev, 4)
        self.lane_launches = 0  # _decode_lanes launch sequences issued
        self.lanes_decoded = 0  # windows decoded in them
        self.frames_computed = 0  # code frames decoded in them (the single windows count theirs)

    def _group(self, windows, W: int, f0: int, f1: int) -> list:
        """One shape's windows (n >= 2) -> their waveforms [1, 1, 512 (f1 - f0)], in order."""
        n = len(windows)
        out = torch.empty(n, DAC_HOP * (f1 - f0), dtype=torch.float32, device=self.ae.dev)
        self.ae._decode_lanes(torch.stack(windows), out, self._bufs(n * STAGE_HALFS_PER_FRAME * self.wmax),
                              (DAC_HOP * f0, DAC_HOP * (f1 - f0)))
        self.lane_launches += 1
        self.lanes_decoded += n
        self.frames_computed += n * W
        return [out[i].view(1, 1, -1) for i in range(n)]

    def __call__(self, windows: list) -> list:
        groups: dict = {}
        for i, (codes, f0, f1) in enumerate(windows):
            W = codes.shape[1]
            assert 0 <= f0 < f1 <= W <= self.wmax, (f0, f1, W)
            groups.setdefault((W, f0, f1), []).append(i)
        res = [None] * len(windows)
        for (W, f0, f1), idx in groups.items():
            for k in range(0, len(idx), self.max_lanes):
                part = idx[k: k + self.max_lanes]
                if len(part) == 1:
                    res[part[0]] = self.single(windows[part[0]][0], f0, f1)
                    continue
                with self.ae.on_stream() as made:
                    made += self._group([windows[i][0] for i in part], W, f0, f1)
                for i, o in zip(part, made):
                    res[i] = o
        return res


class _CarryState:
    """The carried-state decoder's memory and launch sequence, shared by the single-utterance and the batched step:
    a state pool [lanes][state halfs] fp16 (every CarryBuffer's `hist` rows, 425,856 bytes per lane for the DAC) and
    a scratch arena with one dense [group lanes][hist | new][C] buffer per CarryBuffer, so no stage overwrites
    another's input: _decode_lanes' in-place reuse (a unit's 1x1 conv writes over its own k7's input and over the
    skip) would destroy rows the next push needs as history. A run is: gather (or zero, on an utterance's first
    push) the history into the scratch, the decoder's 31 launches on [hist | new] through pointer offsets and in_off
    (zmi_dac_conv_lanes as it is; zmi_dac_conv_t_range_lanes for the transposed convs, whose frontier s F - p is
    not a multiple of the stride), scatter the tails back: 33 launches."""

    def __init__(self, ae: "DACAutoencoder", lanes: int):
        self.ae, self.lanes = ae, int(lanes)
        self.layout = ae.carry_layout()
        self.C = {name: w.c_out for st, w in zip(self.layout.stages, ae.bound)
                  for name in (st.get("dst"), st.get("raw")) if name}
        self.pool_off, off = {}, 0
        for b in self.layout.buffers.values():
            if b.hist:
                self.pool_off[b.name] = off
                off += b.hist * self.C[b.name]
        self.state_halfs = off
        assert off % 8 == 0 and len(self.pool_off) <= 48
        with torch.cuda.stream(ae.stream):
            self.pool = torch.zeros(self.lanes, off, dtype=torch.float16, device=ae.dev)
        self._arena = _Grow(ae.dev, 1)
        self._ids: dict = {}
        self._layouts: dict = {}  # (plan key, lanes) -> scratch_halfs
        self._segs: dict = {}     # (plan key, lanes, mode) -> the state-move table

    def state_bytes_per_lane(self) -> int:
        return 2 * self.state_halfs

    def scratch_halfs(self, plan, B: int):
        """{buffer: arena offset} and the arena's halfs for B lanes of this plan."""
        got = self._layouts.get((plan.key, B))
        if got is None:
            got = self._layouts[(plan.key, B)] = self._scratch_halfs(plan, B)
        return got

    def _scratch_halfs(self, plan, B: int):
        off, o, tmp = {}, 0, 0
        for name, b in self.layout.buffers.items():
            size = (B * plan.rows(name) * self.C[name] + 127) // 128 * 128
            if b.hist:
                off[name] = o
                o += size
            else:  # a k7's output, read by the 1x1 conv that follows and by nothing else: one region for all
                tmp = max(tmp, size)
        off.update({name: o for name, b in self.layout.buffers.items() if not b.hist})
        return off, o + tmp

    def arena(self, plan, B: int) -> torch.Tensor:
        """The kept arena, grown to B lanes of this plan."""
        return self._arena(self.scratch_halfs(plan, B)[1])[0]

    def lane_ids(self, ids) -> torch.Tensor:
        key = tuple(ids)
        if key not in self._ids:
            if len(set(key)) != len(key) or not all(0 <= i < self.lanes for i in key):
                raise ValueError(f"lanes {key}: distinct ids in [0, {self.lanes})")
            if len(self._ids) >= 1024:  # (serve(): the subsets of slots that pushed equal n; kept small)
                self._ids.clear()
            self._ids[key] = torch.tensor(key, dtype=torch.int32, device=self.ae.dev)
        return self._ids[key]

    def _move(self, plan, ids_t, B, arena, off, mode):
        arr = self._segs.get((plan.key, B, mode))
        if arr is None:
            segs = []
            for name, po in self.pool_off.items():
                c, hist = self.C[name], self.layout.buffers[name].hist
                row = plan.tail[name] if mode == 1 else 0
                segs += [po // 8, (off[name] + row * c) // 8, hist * c // 8, plan.rows(name) * c // 8]
            arr = self._segs[(plan.key, B, mode)] = (ctypes.c_uint32 * len(segs))(*segs)
        _lib.check(self.ae.lib.zmi_dac_state_move(self.pool.data_ptr(), self.state_halfs // 8, self.lanes,
                                                  arena.data_ptr(), arena.numel() // 8, ids_t.data_ptr(), B, arr,
                                                  len(arr) // 4, mode, self.ae.sptr), "dac_state_move")

    def run(self, plan, ids_t: torch.Tensor, codes: torch.Tensor, arena: torch.Tensor, out: torch.Tensor):
        """One CarryPlan over the lanes ids_t (int32, device): codes [B, 9, n] int64 contiguous -> out [B, hop m] fp32;
        on the autoencoder's stream. The state is read unless the plan is an utterance's first and written unless
        it is its last. Every stage reads and writes [hist | new] scratch: its output goes behind the dst's (and the
        raw's) history rows."""
        ae, lay = self.ae, self.layout
        B = codes.shape[0]
        off, need = self.scratch_halfs(plan, B)
        assert arena.numel() >= need and codes.is_contiguous() and out.is_contiguous()
        lib, ck, C, s = ae.lib, _lib.check, self.C, ae.sptr
        base = arena.data_ptr()
        P = lambda b, row=0: base + 2 * (off[b] + row * C[b])  # noqa: E731
        LS = lambda b: plan.rows(b) * C[b] if b else 0  # noqa: E731
        new = lambda b: P(b, lay.buffers[b].hist) if b else None  # noqa: E731
        self._move(plan, ids_t, B, arena, off, 2 if plan.first else 0)
        for st, w in zip(plan.steps, ae.bound):
            k, n, src = st["kind"], st["n_out"], st.get("src")
            dst, raw, skip = st.get("dst"), st.get("raw"), st.get("skip")
            if n == 0:
                continue
            if k == "codes":
                ck(lib.zmi_dac_from_codes_lanes(codes.data_ptr(), n, ae.codebooks.data_ptr(), ae.proj_w.data_ptr(),
                                                ae.proj_b.data_ptr(), new(dst), B, N_CODEBOOKS * n, LS(dst), s),
                   "from_codes_lanes")
            elif k == "convt":
                ck(lib.zmi_dac_conv_t_range_lanes(P(src), 0, plan.rows(src), w.c_in, w.w.data_ptr(), w.b.data_ptr(),
                                                  w.c_out, st["s"], st["p"], st["n0"], n, new(raw), new(dst),
                                                  w.alpha.data_ptr(), B, LS(src), LS(raw), LS(dst), s),
                   "dac_conv_t_range_lanes")
            elif k == "out":
                assert out.shape == (B, n), (out.shape, B, n)
                ck(lib.zmi_dac_conv_out_range_lanes(P(src), plan.rows(src), w.c_in, w.w.data_ptr(), w.b.data_ptr(),
                                                    st["in_off"] + 3, n, out.data_ptr(), B, LS(src), n, s),
                   "conv_out_range_lanes")
            else:  # k7, pw
                ck(lib.zmi_dac_conv_lanes(P(src), plan.rows(src), w.c_in, w.w.data_ptr(), w.b.data_ptr(), w.c_out,
                                          w.taps, st.get("d", 0), st["in_off"], n, 1, 0, n,
                                          P(skip, st["skip_off"]) if skip else None, new(raw), new(dst),
                                          w.alpha.data_ptr(), None, B, LS(src), LS(skip), LS(raw), LS(dst), 0, s),
                   "dac_conv_lanes")
        if not plan.final:
            self._move(plan, ids_t, B, arena, off, 1)


class _CarryStep:
    """DACCarryStreamDecoder's decode_step on the HIP decoder: one lane of state; the steady-state step (a push of
    chunk_frames frames past the utterance's start: one plan key whatever the position) is captured as a graph with
    an arena, codes and output of its own."""

    def __init__(self, ae: "DACAutoencoder", chunk_frames: int, capture: bool):
        self.ae, self.chunk, self.capture = ae, int(chunk_frames), bool(capture)
        self.state = _CarryState(ae, 1)
        lay = self.state.layout
        self.steady = lay.plan(lay.R + 1, self.chunk)
        self._ids = self.state.lane_ids((0,))
        self._graph = None
        self.graph_replays = 0
        self.frames_computed = 0  # code frames decoded: a push's own

    def reset(self):
        pass  # an utterance's first push reads no state (ZMI_DAC_MOVE_ZERO)

    def snapshot(self):
        with torch.cuda.stream(self.ae.stream):  # ordered behind the pushes, which run on this stream
            return self.state.pool.clone()

    def restore(self, snap):
        with torch.cuda.stream(self.ae.stream):
            self.state.pool.copy_(snap)

    def __call__(self, plan, codes: torch.Tensor) -> torch.Tensor:
        ae, state = self.ae, self.state
        shape = (1, state.layout.hop * (plan.emit1 - plan.emit0))
        self.frames_computed += plan.n
        with ae.on_stream() as made:
            if self.capture and plan.key == self.steady.key:
                if self._graph is None:
                    self._garena = torch.empty(state.scratch_halfs(plan, 1)[1], dtype=torch.float16, device=ae.dev)
                    self._gcodes = torch.zeros(1, N_CODEBOOKS, self.chunk, dtype=torch.int64, device=ae.dev)
                    self._gout = torch.empty(shape, dtype=torch.float32, device=ae.dev)
                    self._graph = _lib.Graph(ae.sptr)
                self._gcodes[0].copy_(codes)
                self._graph.launch(lambda: state.run(plan, self._ids, self._gcodes, self._garena, self._gout))
                self.graph_replays += 1
                out = self._gout.clone()
            else:
                out = torch.empty(shape, dtype=torch.float32, device=ae.dev)
                state.run(plan, self._ids, codes.contiguous()[None], state.arena(plan, 1), out)
            made.append(out)
        return out.view(1, 1, -1)


class _BatchCarrySteps:
    """DACCarryBatchStreamDecoder's decode_steps on the HIP decoder: the lanes of one plan key, any subset of the
    pool in any order, are ONE launch sequence (their state is gathered into the dense scratch and scattered back,
    since the _lanes entry points need one lane stride). Not captured (as _BatchWindowDecoder); the arena grows on
    demand."""

    def __init__(self, ae: "DACAutoencoder", lanes: int, chunk_frames: int):
        self.ae, self.chunk = ae, int(chunk_frames)
        self.state = _CarryState(ae, lanes)
        self.lane_launches = 0    # launch sequences issued
        self.lanes_decoded = 0    # lanes decoded in them
        self.frames_computed = 0  # code frames decoded in them: the frames pushed
        self.launch_log = []      # (lane ids, n) per launch sequence, the last 64

    def reset(self, lane: int):
        pass  # an utterance's first push reads no state (ZMI_DAC_MOVE_ZERO)

    def __call__(self, plan, ids, codes) -> list:
        ae, state = self.ae, self.state
        B = len(ids)
        ids_t = state.lane_ids(ids)
        with ae.on_stream() as made:
            out = torch.empty(B, state.layout.hop * (plan.emit1 - plan.emit0), dtype=torch.float32, device=ae.dev)
            state.run(plan, ids_t, torch.stack([c.contiguous() for c in codes]), state.arena(plan, B), out)
            made.append(out)
        self.lane_launches += 1
        self.lanes_decoded += B
        self.frames_computed += B * plan.n
        self.launch_log = (self.launch_log + [(tuple(ids), plan.n)])[-64:]
        return [out[i].view(1, 1, -1) for i in range(B)]


class DACAutoencoder:
    codebook_size = 1024
    num_codebooks = N_CODEBOOKS
    sampling_rate = DAC_SAMPLE_RATE

    def __init__(self, device="cuda", state_dict: dict | None = None, seed: int = 0):
        self.dev = torch.device(device)
        self.lib = _lib.lib()
        self.stream = torch.cuda.Stream(self.dev)
        self.sptr = self.stream.cuda_stream
        self._resamplers: dict = {}  # (o, n) -> GpuResampler (its table stays on the device)
        if state_dict is None:
            state_dict = {}
            with torch.cuda.stream(self.stream):
                for sp in syn.dac_specs() + syn.dac_encoder_specs():
                    t = torch.empty(sp.shape, dtype=torch.float32, device=self.dev)
                    _lib.check(self.lib.zmi_fill_uniform(t.data_ptr(), sp.numel, syn.tensor_key(seed, sp.name),
                                                         sp.scale, sp.offset, 1, self.sptr), "fill")
                    state_dict[sp.name] = t
        self._prepare(_fold_weight_norm(state_dict))
        self._bufs = _Grow(self.dev, 4)  # decode() at B = 1
        self._walks: dict = {}  # (B, T, crop, stage buffers) -> _walk

    def on_stream(self) -> "_OnStream":
        """`with ae.on_stream() as made:` is the stream hand-off of every entry point (_OnStream)."""
        return _OnStream(self)

    # --------------------------------------------------------------- weight layout
    def _prepare(self, sd: dict):
        f32 = lambda t: t.to(self.dev, torch.float32).contiguous()  # noqa: E731

        def conv_w(w):  # [co][ci][k] -> channel-blocked [k][ci / 32][co][32] fp16; 1x1: [1][co][ci]
            return pack_conv(w.to(self.dev))

        with torch.cuda.stream(self.stream):
            q = "quantizer.quantizers."
            self.codebooks = torch.stack([f32(sd[f"{q}{i}.codebook.weight"]) for i in range(N_CODEBOOKS)]).contiguous()
            self.proj_w = torch.stack([f32(sd[f"{q}{i}.out_proj.weight"]).reshape(-1, 8)
                                       for i in range(N_CODEBOOKS)]).contiguous()
            self.proj_b = torch.stack([f32(sd[f"{q}{i}.out_proj.bias"]) for i in range(N_CODEBOOKS)]).contiguous()
            # The decoder's weights, bound to its stages once (streaming.dac_stages names them): per stage the packed
            # weight, bias, widths, taps and the alpha its output is stored under, and `slots`, its (src, dst, skip,
            # raw) among the four stage buffers (H, SA, SB, S2) of the whole-utterance walk, which reuses them in
            # place: the raw skip path in H, the Snake'd activations in SA and SB in turn (a transposed conv reads one
            # and writes the other), z and a unit's k7 output in S2 (conv1, which reads z there, writes SA).
            self.stages, self.bound = dac_stages(STRIDES, DILATIONS), []
            slot, x = {}, 1
            for st in self.stages:
                k = st["kind"]
                if k == "convt":
                    x = 3 - x
                if k != "out":
                    slot[st["dst"]] = 3 if k == "codes" or (k == "k7" and slot[st["src"]] != 3) else x
                if st.get("raw"):
                    slot[st["raw"]] = 0
                slots = tuple(slot.get(st.get(role)) for role in ("src", "dst", "skip", "raw"))
                if k == "codes":
                    self.bound.append(SimpleNamespace(c_out=self.proj_b.shape[1], slots=slots))
                    continue
                wt, b = sd[st["w"] + ".weight"].to(self.dev, torch.float32), f32(sd[st["w"] + ".bias"])
                if k == "convt":  # [cin][cout][2s]
                    c_in, c_out, w = wt.shape[0], wt.shape[1], pack_conv_transpose(wt, st["s"], st["p"])
                elif k == "out":  # [1][96][7], in zmi_dac_conv_out's 32-channel tile
                    c_in, c_out, (w, b) = wt.shape[1], 32, pack_conv_out(wt, b)
                else:
                    c_in, c_out, w = wt.shape[1], wt.shape[0], pack_conv(wt)
                self.bound.append(SimpleNamespace(w=w, b=b, c_in=c_in, c_out=c_out, taps=wt.shape[2], slots=slots,
                                                  alpha=f32(sd[st["alpha"]]).reshape(-1) if "alpha" in st else None))
            self.has_encoder = "encoder.conv1.weight" in sd
            if self.has_encoder:
                self._prepare_encoder(sd, f32, conv_w)
        self.stream.synchronize()

    def _prepare_encoder(self, sd, f32, conv_w):
        w1 = f32(sd["encoder.conv1.weight"])                                  # [64][1][7]
        self.e1_w, self.e1_b = pack_im2col_conv1(w1), f32(sd["encoder.conv1.bias"])    # 1x1: [1][co][ci]
        self.eblocks = []
        c = w1.shape[0]
        for j, s in enumerate(ENC_STRIDES):
            p = f"encoder.block.{j}."
            res = [dict(a1=f32(sd[p + f"res_unit{u + 1}.snake1.alpha"]).reshape(-1),
                        w1=conv_w(sd[p + f"res_unit{u + 1}.conv1.weight"]), b1=f32(sd[p + f"res_unit{u + 1}.conv1.bias"]),
                        a2=f32(sd[p + f"res_unit{u + 1}.snake2.alpha"]).reshape(-1),
                        w2=conv_w(sd[p + f"res_unit{u + 1}.conv2.weight"]), b2=f32(sd[p + f"res_unit{u + 1}.conv2.bias"]))
                   for u in range(3)]
            # Conv1d(c, 2c, k=2s, stride s, pad ceil(s/2)) as a stride-1, 3-tap conv with c_in = s*c over the
            # polyphase view of its input (pack_strided_conv)
            wt = f32(sd[p + "conv1.weight"])                                   # [2c][c][2s]
            self.eblocks.append(dict(stride=s, c=c, res=res, alpha=f32(sd[p + "snake1.alpha"]).reshape(-1),
                                     w=pack_strided_conv(wt, s, math.ceil(s / 2)), b=f32(sd[p + "conv1.bias"])))
            c *= 2
        self.e_final_alpha = f32(sd["encoder.snake1.alpha"]).reshape(-1)
        self.e2_w, self.e2_b = conv_w(sd["encoder.conv2.weight"]), f32(sd["encoder.conv2.bias"])
        self.e2_cin, self.e2_cout = sd["encoder.conv2.weight"].shape[1], sd["encoder.conv2.weight"].shape[0]
        q = "quantizer.quantizers."
        self.vq_in_w = torch.stack([f32(sd[f"{q}{i}.in_proj.weight"]).reshape(8, -1) for i in range(N_CODEBOOKS)])
        self.vq_in_b = torch.stack([f32(sd[f"{q}{i}.in_proj.bias"]) for i in range(N_CODEBOOKS)]).contiguous()
        # l2-normalised codebooks and their squared norms: load-time weight preparation (modeling_dac.py:163-168)
        self.cb_n = torch.nn.functional.normalize(self.codebooks, dim=-1).contiguous()
        self.cb_n2 = self.cb_n.pow(2).sum(-1).contiguous()

    # --------------------------------------------------------------- decode
    def _conv(self, x, t_in, c_in, w, b, c_out, taps, step, off, n_out, stride, phase, t_out, skip=None, raw=None,
              snake=None, alpha=None, f32=None):
        p = _lib.ptr
        _lib.check(self.lib.zmi_dac_conv(p(x), t_in, c_in, p(w), p(b), c_out, taps, step, off, n_out, stride, phase,
                                         t_out, p(skip), p(raw), p(snake), p(alpha), p(f32), self.sptr), "dac_conv")

    def _decode_lanes(self, codes: torch.Tensor, out: torch.Tensor, bufs, crop=None):
        """The whole-utterance walk of the stage list (modeling_dac.py:347-371, 407-441), over B utterances of one
        length in its 31 launches (the zmi_dac_*_lanes entry points; B = 1 is what their single forms forward to):
        codes [B, 9, T] int64 contiguous (device) -> out [B, n] fp32 contiguous. bufs: four stage buffers of at least
        B x STAGE_HALFS_PER_FRAME x T halfs each; every stage's activations are [B][t][c] dense, so a lane's stride is
        that stage's t x c. crop = (q0, n): only samples q0 .. q0 + n - 1 of every lane are computed by the last stage
        (the streaming decoders' window crop; default: all 512 T). A lane's samples have the same bits at every B
        (the lanes entry points' contract, tests/test_gpu_dac_lanes.py)."""
        B, _, T = codes.shape
        assert codes.is_contiguous() and out.is_contiguous() and out.shape[0] == B
        assert all(b.numel() >= B * STAGE_HALFS_PER_FRAME * T for b in bufs)
        H, SA, SB, S2 = bufs
        key = (B, T, crop, H.data_ptr(), SA.data_ptr(), SB.data_ptr(), S2.data_ptr())
        walk = self._walks.get(key)
        if walk is None:
            if len(self._walks) >= 256:  # (a stream's first and last windows have shapes of their own; kept small)
                self._walks.clear()
            walk = self._walks[key] = self._walk(*key)
        (_, from_codes, a0), convs, (_, conv_out, a1) = walk
        assert out.shape[1] == a1[6].value
        _lib.check(from_codes(codes.data_ptr(), *a0[1:]), "from_codes_lanes")
        for what, fn, args in convs:
            _lib.check(fn(*args), what)
        _lib.check(conv_out(*a1[:7], out.data_ptr(), *a1[8:]), "conv_out_range_lanes")

    def _walk(self, B: int, T: int, crop, *at) -> tuple:
        """_decode_lanes' launches for one shape in the stage buffers at `at`, each (name, entry point, arguments): the
        first, the 29 convs between, the last, with the first's codes and the last's out left open (0). The arguments are built once per shape, as ctypes objects: at one lane the
        25 arguments of a conv launch cost the host more to work out and convert than the launch itself."""
        lib, s, at, walk, t = self.lib, self.sptr, at + (None,), [], T

        def add(name, *args):
            fn = getattr(lib, "zmi_dac_" + name)
            walk.append((name, fn, tuple(None if v is None else ty(v) for ty, v in zip(fn.argtypes, args))))

        for st, w in zip(self.stages, self.bound):
            k, p = st["kind"], _lib.ptr
            src, dst, skip, raw = (at[-1 if i is None else i] for i in w.slots)
            if k == "codes":
                add("from_codes_lanes", 0, T, p(self.codebooks), p(self.proj_w), p(self.proj_b), dst, B, N_CODEBOOKS * T,
                    w.c_out * T, s)
            elif k == "convt":  # every phase in one launch
                tn = t * st["s"]
                add("conv_t_lanes", src, t, w.c_in, p(w.w), p(w.b), w.c_out, st["s"], st["p"], raw, dst, p(w.alpha), B,
                    t * w.c_in, tn * w.c_out, tn * w.c_out, s)
                t = tn
            elif k == "out":
                q0, n = (0, t) if crop is None else crop
                add("conv_out_range_lanes", src, t, w.c_in, p(w.w), p(w.b), q0, n, 0, B, t * w.c_in, n, s)
            else:  # k7 (padding 3 d), pw (d = 0)
                d, ls = st.get("d", 0), t * w.c_out
                add("conv_lanes", src, t, w.c_in, p(w.w), p(w.b), w.c_out, w.taps, d, -3 * d, t, 1, 0, t, skip, raw, dst,
                    p(w.alpha), None, B, t * w.c_in, ls, ls, ls, 0, s)
        return walk[0], walk[1:-1], walk[-1]

    # stage memory of one decode() launch sequence over several utterances (4 buffers x STAGE_HALFS_PER_FRAME T halfs
    # per lane)
    DECODE_LANES_BYTES = 1 << 30

    @torch.inference_mode()
    def decode(self, codes: torch.Tensor) -> torch.Tensor:
        """[B, 9, T] codes -> [B, 1, 512 T] fp32 waveform (reference autoencoder.py:25-27). B > 1: the utterances
        share T, so they are lanes of one launch sequence (as many at a time as DECODE_LANES_BYTES of stage memory
        hold), each with the bits its own decode() gives. B = 1 decodes in kept stage buffers that grow on demand."""
        B, nq, T = codes.shape
        assert nq == N_CODEBOOKS
        out = torch.empty(B, 1, DAC_HOP * T, dtype=torch.float32, device=self.dev)
        with self.on_stream():
            codes = codes.to(self.dev, torch.int64).contiguous()
            if T > 0:
                per = max(1, min(B, 4096, self.DECODE_LANES_BYTES // (4 * 2 * STAGE_HALFS_PER_FRAME * T)))
                bufs = self._bufs(STAGE_HALFS_PER_FRAME * T) if B == 1 else \
                    [torch.empty(per * STAGE_HALFS_PER_FRAME * T, dtype=torch.float16, device=self.dev) for _ in range(4)]
                for b in range(0, B, per):
                    self._decode_lanes(codes[b: b + per], out[b: b + per, 0], bufs)
        return out

    def carry_layout(self) -> CarryLayout:
        """The carried-state planner of this decoder's stage list (streaming.CarryLayout)."""
        if getattr(self, "_carry_layout", None) is None:
            self._carry_layout = CarryLayout(STRIDES, DILATIONS, DAC_LOOKAHEAD_FRAMES)
            assert self._carry_layout.hop == DAC_HOP and self._carry_layout.stages == self.stages
        return self._carry_layout

    def stream_decoder(self, chunk_frames: int = 16, capture: bool | None = None, carry: bool = False):
        """An incremental decoder: push() code frames as they become final, flush() at the end; the concatenated
        returns are bit for bit decode() of all the codes (streaming.py). capture: replay the steady-state step as
        one hipGraph (default: WINDOW_GRAPH). carry=False: the window decoder (a window of lookahead + chunk_frames +
        lookahead frames per chunk_frames emitted). carry=True: the carried-state decoder with the same returns
        (DACCarryStreamDecoder): every stage keeps its last rows, so a push computes its own frames only."""
        capture = WINDOW_GRAPH if capture is None else capture
        if carry:
            return DACCarryStreamDecoder(_CarryStep(self, chunk_frames, capture), self.carry_layout(), chunk_frames,
                                         device=self.dev)
        win = _WindowDecoder(self, chunk_frames, capture)
        return DACStreamDecoder(win, chunk_frames, DAC_LOOKAHEAD_FRAMES, device=self.dev)

    def stream_decoder_batch(self, lanes: int, chunk_frames: int = 16, carry: bool = False):
        """`lanes` incremental decoders that decode together: push({lane: codes}) / flush(lanes) / reset(lane)
        (streaming.DACBatchStreamDecoder); per lane the concatenated returns are bit for bit decode() of its codes. All
        the windows of equal shape that a call makes due are lanes of one launch sequence (_decode_lanes); stage memory
        is allocated for the lanes in use. carry=True: the carried-state decoder with the same returns
        (DACCarryBatchStreamDecoder): per-lane state, and the lanes of a call whose pushes have one shape (past an
        utterance's start: equal n) are one launch sequence."""
        if carry:
            return DACCarryBatchStreamDecoder(_BatchCarrySteps(self, lanes, chunk_frames), self.carry_layout(), lanes,
                                              chunk_frames, device=self.dev)
        win = _BatchWindowDecoder(self, lanes, chunk_frames)
        return DACBatchStreamDecoder(win, lanes, chunk_frames, DAC_LOOKAHEAD_FRAMES, device=self.dev)

    # --------------------------------------------------------------- encode
    def preprocess(self, wav: torch.Tensor, sr: int) -> torch.Tensor:
        """autoencoder.py:17-20: resample to 44.1 kHz (zmi_resample: fp32 cuda tensors only, the kernel is the only
        implementation; a CPU tensor raises NotImplementedError, another dtype ValueError) and right-pad to a multiple
        of 512 samples. sr == 44100 only pads, whatever the device and dtype."""
        if sr != DAC_SAMPLE_RATE:
            if not wav.is_cuda:
                raise NotImplementedError(f"resampling {sr} Hz -> 44.1 kHz runs on the GPU only: pass a cuda tensor")
            wav = self.resample(wav, sr, DAC_SAMPLE_RATE)
        right = math.ceil(wav.shape[-1] / DAC_HOP) * DAC_HOP - wav.shape[-1]
        return torch.nn.functional.pad(wav, (0, right))

    @torch.inference_mode()
    def resample(self, wav: torch.Tensor, orig_rate: int, new_rate: int) -> torch.Tensor:
        """[..., N] fp32 cuda -> [..., ceil(new_rate N / orig_rate)]: torchaudio.functional.resample's defaults, every
        leading row a segment of one zmi_resample launch on the autoencoder's stream (resampling.py). Equal rates
        return the input; a CPU tensor raises NotImplementedError and a dtype other than fp32 ValueError (nothing is
        cast silently)."""
        key = resample_plan(orig_rate, new_rate)[:2]
        if key[0] == key[1]:
            return wav
        if not wav.is_cuda:
            raise NotImplementedError("resample() runs on the GPU only: pass a cuda tensor")
        if wav.dtype != torch.float32:  # (no silent cast: the 44.1 kHz path of preprocess() keeps the input's dtype)
            raise ValueError(f"resample() takes fp32 audio, got {wav.dtype}")
        rs = self._resamplers.get(key)
        if rs is None:
            rs = self._resamplers[key] = GpuResampler(self.dev, *key)
        with self.on_stream() as made:
            out = rs(wav.to(self.dev))
            made.append(out)
        return out

    def resampler(self, new_rate: int, lanes: int = 1) -> StreamResampler:
        """`lanes` streaming resamplers from 44.1 kHz to new_rate (resampling.StreamResampler): push({lane: chunk},
        final=...) / flush(lanes) / reset(lane); per lane the concatenated returns are bit for bit
        resample(the whole waveform, 44100, new_rate). Its launches go to the stream that is current at each call."""
        return StreamResampler(lanes, DAC_SAMPLE_RATE, new_rate, device=self.dev)

    def _encoder_buffers(self, n: int):
        need = 64 * (n + 8)
        if getattr(self, "_ebufs", None) is None or self._ebufs[0].numel() < need:
            with torch.cuda.stream(self.stream):
                self._ebufs = [torch.empty(need, dtype=torch.float16, device=self.dev) for _ in range(3)]
        return self._ebufs

    def encode_latents(self, wav1: torch.Tensor, lat: torch.Tensor):
        """wav1 [n] fp32 (n % 512 == 0) -> lat [n / 512][1024] fp32 (DacEncoder, modeling_dac.py:464-475)."""
        n = wav1.shape[-1]
        H, SA, S2 = self._encoder_buffers(n)
        col = S2  # [n][32] fp16, consumed by conv1 before S2 is reused
        _lib.check(self.lib.zmi_dac_im2col7(wav1.data_ptr(), n, col.data_ptr(), self.sptr), "im2col7")
        b0 = self.eblocks[0]
        self._conv(col, n, 32, self.e1_w, self.e1_b, b0["c"], 1, 0, 0, n, 1, 0, n, raw=H, snake=SA,
                   alpha=b0["res"][0]["a1"])
        t = n
        for j, blk in enumerate(self.eblocks):
            c, s, res = blk["c"], blk["stride"], blk["res"]
            for u, dil in enumerate(DILATIONS):
                ru = res[u]
                self._conv(SA, t, c, ru["w1"], ru["b1"], c, 7, dil, -3 * dil, t, 1, 0, t, snake=S2, alpha=ru["a2"])
                last = u == len(DILATIONS) - 1
                self._conv(S2, t, c, ru["w2"], ru["b2"], c, 1, 0, 0, t, 1, 0, t, skip=H, raw=None if last else H,
                           snake=SA, alpha=blk["alpha"] if last else res[u + 1]["a1"])
            tn = t // s
            more = j + 1 < len(self.eblocks)
            # strided conv on the polyphase view of SA ([t][c] read as [t/s][s c]): 3 taps, in_off -1
            self._conv(SA, tn, s * c, blk["w"], blk["b"], 2 * c, 3, 1, -1, tn, 1, 0, tn, raw=H if more else None,
                       snake=S2, alpha=self.eblocks[j + 1]["res"][0]["a1"] if more else self.e_final_alpha)
            SA, S2 = S2, SA
            t = tn
        self._conv(SA, t, self.e2_cin, self.e2_w, self.e2_b, self.e2_cout, 3, 1, -1, t, 1, 0, t, f32=lat)

    @torch.inference_mode()
    def encode(self, wav: torch.Tensor) -> torch.Tensor:
        """[B, 1, 512 T] fp32 waveform -> [B, 9, T] int64 codes (reference autoencoder.py:22-23)."""
        if not self.has_encoder:
            raise RuntimeError("this DAC state_dict has no encoder weights")
        B, ch, n = wav.shape
        assert ch == 1 and n % DAC_HOP == 0, "preprocess() first: mono, length a multiple of 512"
        T = n // DAC_HOP
        out = torch.empty(B, N_CODEBOOKS, T, dtype=torch.int64, device=self.dev)
        with self.on_stream():
            wav = wav.to(self.dev, torch.float32).contiguous()
            lat = torch.empty(T, 1024, dtype=torch.float32, device=self.dev)
            for b in range(B):
                self.encode_latents(wav[b, 0], lat)
                self.quantize(lat, out[b])
        return out

    def quantize(self, lat: torch.Tensor, codes: torch.Tensor):
        """lat [T][1024] fp32 -> codes [9][T] int64 (residual VQ, modeling_dac.py:283-345)."""
        T = lat.shape[0]
        _lib.check(self.lib.zmi_dac_vq(lat.data_ptr(), T, self.vq_in_w.data_ptr(), self.vq_in_b.data_ptr(),
                                       self.codebooks.data_ptr(), self.cb_n.data_ptr(), self.cb_n2.data_ptr(),
                                       self.proj_w.data_ptr(), self.proj_b.data_ptr(), codes.data_ptr(), self.sptr),
                   "dac_vq")
