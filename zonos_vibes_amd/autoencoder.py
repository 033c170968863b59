"""DACAutoencoder with the reference's decode() surface (zonos/autoencoder.py:8-27), on HIP kernels.

The decoder path is on the hot path: quantizer.from_codes + DacDecoder.
`encode` (voice-clone audio prefix) runs DacEncoder + the residual VQ on the
same MFMA conv kernel (strided convs in polyphase form) plus a VQ kernel; `preprocess` pads to a
multiple of 512 samples (resampling needs torchaudio, absent here: only 44.1 kHz input is taken).

Weights use transformers' DacModel state_dict names (quantizer.quantizers.{i}.*, decoder.*);
weight-norm pairs (weight_g / weight_v, or parametrizations.weight.original0 / original1) are
folded to plain weights at load time.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from . import synthetic as syn
from .config import DAC_HOP, DAC_SAMPLE_RATE, N_CODEBOOKS
from .resampling import GpuResampler, StreamResampler, resample_plan
from .streaming import (DAC_LOOKAHEAD_FRAMES, CarryLayout, DACBatchStreamDecoder, DACCarryBatchStreamDecoder,  # noqa: F401
                        DACCarryStreamDecoder, DACStreamDecoder, dac_lookahead_frames)

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


class _WindowDecoder:
    """DACStreamDecoder's decode_window on the HIP decoder: a window is decoded by _decode_one's launch sequence in
    stage buffers of its own (a captured graph keeps their addresses), and the last stage computes only the kept
    samples (zmi_dac_conv_out_range), so the crop costs no copy of the window and no host sync."""

    def __init__(self, ae: "DACAutoencoder", chunk_frames: int, capture: bool):
        self.ae, self.chunk, self.R, self.capture = ae, int(chunk_frames), DAC_LOOKAHEAD_FRAMES, bool(capture)
        self.wmax = 2 * self.R + self.chunk
        self._bufs = None
        self._graph = None
        self.graph_replays = 0
        self.frames_computed = 0  # code frames decoded (a window's halo frames count)

    def _alloc(self):
        ae = self.ae
        self._bufs = [torch.empty(49152 * self.wmax, dtype=torch.float16, device=ae.dev) for _ in range(4)]
        self._gcodes = torch.zeros(N_CODEBOOKS, self.wmax, dtype=torch.int64, device=ae.dev)
        self._gout = torch.empty(DAC_HOP * self.chunk, dtype=torch.float32, device=ae.dev)

    def __call__(self, codes: torch.Tensor, f0: int, f1: int) -> torch.Tensor:
        ae = self.ae
        W = codes.shape[1]
        assert 0 <= f0 < f1 <= W <= self.wmax, (f0, f1, W)
        self.frames_computed += W
        cur = torch.cuda.current_stream(ae.dev)
        ae.stream.wait_stream(cur)
        with torch.cuda.stream(ae.stream):
            if self._bufs is None:
                self._alloc()
            crop = (DAC_HOP * f0, DAC_HOP * (f1 - f0))
            if self.capture and W == self.wmax and f0 == self.R and f1 == self.R + self.chunk:
                self._gcodes.copy_(codes)
                if self._graph is None:
                    _lib.check(ae.lib.zmi_graph_begin(ae.sptr), "graph_begin")
                    try:
                        ae._decode_one(self._gcodes, self._gout, self._bufs, crop)
                    finally:
                        g = ctypes.c_void_p()
                        _lib.check(ae.lib.zmi_graph_end(ae.sptr, ctypes.byref(g)), "graph_end")
                    self._graph = g.value
                _lib.check(ae.lib.zmi_graph_launch(self._graph, 1, ae.sptr), "graph_launch")
                self.graph_replays += 1
                out = self._gout.clone()
            else:
                out = torch.empty(crop[1], dtype=torch.float32, device=ae.dev)
                ae._decode_one(codes.contiguous(), out, self._bufs, crop)
        cur.wait_stream(ae.stream)
        out.record_stream(cur)
        return out.view(1, 1, -1)

    def __del__(self):
        if getattr(self, "_graph", None):
            self.ae.lib.zmi_graph_destroy(self._graph)
            self._graph = None


STAGE_HALFS_PER_FRAME = 49152  # max over stages of C x time per code frame (blocks 3 and 4: 192 x 256 = 96 x 512)


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
        self._cap = 0        # lanes the stage buffers hold
        self._bufs = None
        self.lane_launches = 0  # _decode_lanes launch sequences issued
        self.lanes_decoded = 0  # windows decoded in them
        self.frames_computed = 0  # code frames decoded in them (the single windows count theirs)

    def _reserve(self, lanes: int):
        if lanes > self._cap:
            self._bufs = None  # freed before the larger ones are allocated
            self._bufs = [torch.empty(lanes * STAGE_HALFS_PER_FRAME * self.wmax, dtype=torch.float16, device=self.ae.dev)
                          for _ in range(4)]
            self._cap = lanes

    def _group(self, windows, W: int, f0: int, f1: int) -> list:
        """One shape's windows (n >= 2) -> their waveforms [1, 1, 512 (f1 - f0)], in order."""
        n = len(windows)
        self._reserve(n)
        out = torch.empty(n, DAC_HOP * (f1 - f0), dtype=torch.float32, device=self.ae.dev)
        self.ae._decode_lanes(torch.stack(windows), out, self._bufs, (DAC_HOP * f0, DAC_HOP * (f1 - f0)))
        self.lane_launches += 1
        self.lanes_decoded += n
        self.frames_computed += n * W
        return [out[i].view(1, 1, -1) for i in range(n)]

    def __call__(self, windows: list) -> list:
        ae = self.ae
        groups: dict = {}
        for i, (codes, f0, f1) in enumerate(windows):
            W = codes.shape[1]
            assert 0 <= f0 < f1 <= W <= self.wmax, (f0, f1, W)
            groups.setdefault((W, f0, f1), []).append(i)
        res = [None] * len(windows)
        cur = torch.cuda.current_stream(ae.dev)
        for (W, f0, f1), idx in groups.items():
            for k in range(0, len(idx), self.max_lanes):
                part = idx[k: k + self.max_lanes]
                if len(part) == 1:
                    res[part[0]] = self.single(windows[part[0]][0], f0, f1)
                    continue
                ae.stream.wait_stream(cur)
                with torch.cuda.stream(ae.stream):
                    outs = self._group([windows[i][0] for i in part], W, f0, f1)
                cur.wait_stream(ae.stream)
                for i, o in zip(part, outs):
                    o.record_stream(cur)
                    res[i] = o
        return res


class _CarryState:
    """The carried-state decoder's memory and launch sequence, shared by the single-utterance and the batched step:
    a state pool [lanes][state halfs] fp16 (every CarryBuffer's `hist` rows, 425,856 bytes per lane for the DAC) and
    a scratch arena with one dense [group lanes][hist | new][C] buffer per CarryBuffer, so no stage overwrites
    another's input: _decode_one's in-place reuse (a unit's 1x1 conv writes over its own k7's input and over the
    skip) would destroy rows the next push needs as history. A run is: gather (or zero, on an utterance's first
    push) the history into the scratch, the decoder's 31 launches on [hist | new] through pointer offsets and in_off
    (zmi_dac_conv_lanes as it is; zmi_dac_conv_t_range_lanes for the transposed convs, whose frontier s F - p is
    not a multiple of the stride), scatter the tails back: 33 launches."""

    def __init__(self, ae: "DACAutoencoder", lanes: int):
        self.ae, self.lanes = ae, int(lanes)
        self.layout = ae.carry_layout()
        widths = {"z": ae.c1_cin, "c1": ae.c1_cout}
        widths.update({j: blk["cout"] for j, blk in enumerate(ae.blocks)})
        self.C = {b.name: widths[b.width] for b in self.layout.buffers.values()}
        self.pool_off, off = {}, 0
        for b in self.layout.buffers.values():
            if b.hist:
                self.pool_off[b.name] = off
                off += b.hist * self.C[b.name]
        self.state_halfs = off
        assert off % 8 == 0 and len(self.pool_off) <= 48
        with torch.cuda.stream(ae.stream):
            self.pool = torch.zeros(self.lanes, off, dtype=torch.float16, device=ae.dev)
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
        it is its last."""
        ae, lay = self.ae, self.layout
        B = codes.shape[0]
        off, need = self.scratch_halfs(plan, B)
        assert arena.numel() >= need and codes.is_contiguous() and out.is_contiguous()
        lib, ck, C = ae.lib, _lib.check, self.C
        base = arena.data_ptr()
        P = lambda b, row=0: base + 2 * (off[b] + row * C[b])  # noqa: E731
        LS = lambda b: plan.rows(b) * C[b]  # noqa: E731
        hist = lambda b: lay.buffers[b].hist  # noqa: E731
        self._move(plan, ids_t, B, arena, off, 2 if plan.first else 0)

        def conv(st, w, bias, c_in, c_out, taps, alpha, skip=None, raw=None):
            src, dst, n = st["src"], st["dst"], st["n_out"]
            ck(lib.zmi_dac_conv_lanes(P(src), plan.rows(src), c_in, w.data_ptr(), bias.data_ptr(), c_out, taps,
                                      st.get("d", 0), st["in_off"], n, 1, 0, n,
                                      P(skip, st["skip_off"]) if skip else None, P(raw, hist(raw)) if raw else None,
                                      P(dst, hist(dst)), alpha.data_ptr(), None, B, LS(src), LS(skip) if skip else 0,
                                      LS(raw) if raw else 0, LS(dst), 0, ae.sptr), "dac_conv_lanes")

        for st in plan.steps:
            k, n = st["kind"], st["n_out"]
            if n == 0:
                continue
            if k == "codes":
                ck(lib.zmi_dac_from_codes_lanes(codes.data_ptr(), n, ae.codebooks.data_ptr(), ae.proj_w.data_ptr(),
                                                ae.proj_b.data_ptr(), P("z", hist("z")), B, N_CODEBOOKS * n, LS("z"),
                                                ae.sptr), "from_codes_lanes")
            elif k == "k7" and "block" not in st:
                conv(st, ae.c1_w, ae.c1_b, ae.c1_cin, ae.c1_cout, 7, ae.blocks[0]["alpha"])
            elif k == "k7":
                ru, c = ae.blocks[st["block"]]["res"][st["unit"]], ae.blocks[st["block"]]["cout"]
                conv(st, ru["w1"], ru["b1"], c, c, 7, ru["a2"])
            elif k == "pw":
                j, u = st["block"], st["unit"]
                blk = ae.blocks[j]
                ru, c = blk["res"][u], blk["cout"]
                if u + 1 < len(DILATIONS):
                    nxt = blk["res"][u + 1]["a1"]
                else:
                    nxt = ae.blocks[j + 1]["alpha"] if j + 1 < len(ae.blocks) else ae.final_alpha
                conv(st, ru["w2"], ru["b2"], c, c, 1, nxt, skip=st["skip"], raw=st["raw"])
            elif k == "convt":
                blk, src, dst, raw = ae.blocks[st["block"]], st["src"], st["dst"], st["raw"]
                ck(lib.zmi_dac_conv_t_range_lanes(P(src), 0, plan.rows(src), blk["cin"], blk["wt"].data_ptr(),
                                                  blk["bt"].data_ptr(), blk["cout"], blk["stride"], blk["pad"], st["n0"],
                                                  n, P(raw, hist(raw)), P(dst, hist(dst)),
                                                  blk["res"][0]["a1"].data_ptr(), B, LS(src), LS(raw), LS(dst), ae.sptr),
                   "dac_conv_t_range_lanes")
            else:
                src = st["src"]
                assert out.shape == (B, n), (out.shape, B, n)
                ck(lib.zmi_dac_conv_out_range_lanes(P(src), plan.rows(src), C[src], ae.out_w.data_ptr(),
                                                    ae.out_b.data_ptr(), st["in_off"] + 3, n, out.data_ptr(), B, LS(src),
                                                    n, ae.sptr), "conv_out_range_lanes")
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
        self._arena = None
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
        ae, hop = self.ae, self.state.layout.hop
        m = plan.emit1 - plan.emit0
        self.frames_computed += plan.n
        cur = torch.cuda.current_stream(ae.dev)
        ae.stream.wait_stream(cur)
        with torch.cuda.stream(ae.stream):
            if self.capture and plan.key == self.steady.key:
                if self._graph is None:
                    self._garena = torch.empty(self.state.scratch_halfs(plan, 1)[1], dtype=torch.float16, device=ae.dev)
                    self._gcodes = torch.zeros(1, N_CODEBOOKS, self.chunk, dtype=torch.int64, device=ae.dev)
                    self._gout = torch.empty(1, hop * m, dtype=torch.float32, device=ae.dev)
                    self._gcodes[0].copy_(codes)
                    _lib.check(ae.lib.zmi_graph_begin(ae.sptr), "graph_begin")
                    try:
                        self.state.run(plan, self._ids, self._gcodes, self._garena, self._gout)
                    finally:
                        g = ctypes.c_void_p()
                        _lib.check(ae.lib.zmi_graph_end(ae.sptr, ctypes.byref(g)), "graph_end")
                    self._graph = g.value
                else:
                    self._gcodes[0].copy_(codes)
                _lib.check(ae.lib.zmi_graph_launch(self._graph, 1, ae.sptr), "graph_launch")
                self.graph_replays += 1
                out = self._gout.clone()
            else:
                need = self.state.scratch_halfs(plan, 1)[1]
                if self._arena is None or self._arena.numel() < need:
                    self._arena = None
                    self._arena = torch.empty(need, dtype=torch.float16, device=ae.dev)
                out = torch.empty(1, hop * m, dtype=torch.float32, device=ae.dev)
                self.state.run(plan, self._ids, codes.contiguous()[None], self._arena, out)
        cur.wait_stream(ae.stream)
        out.record_stream(cur)
        return out.view(1, 1, -1)

    def __del__(self):
        if getattr(self, "_graph", None):
            self.ae.lib.zmi_graph_destroy(self._graph)
            self._graph = None


class _BatchCarrySteps:
    """DACCarryBatchStreamDecoder's decode_steps on the HIP decoder: the lanes of one plan key, any subset of the
    pool in any order, are ONE launch sequence (their state is gathered into the dense scratch and scattered back,
    since the _lanes entry points need one lane stride). Not captured (as _BatchWindowDecoder); the arena grows on
    demand."""

    def __init__(self, ae: "DACAutoencoder", lanes: int, chunk_frames: int):
        self.ae, self.chunk = ae, int(chunk_frames)
        self.state = _CarryState(ae, lanes)
        self._arena = None
        self.lane_launches = 0    # launch sequences issued
        self.lanes_decoded = 0    # lanes decoded in them
        self.frames_computed = 0  # code frames decoded in them: the frames pushed
        self.launch_log = []      # (lane ids, n) per launch sequence, the last 64

    def reset(self, lane: int):
        pass  # an utterance's first push reads no state (ZMI_DAC_MOVE_ZERO)

    def __call__(self, plan, ids, codes) -> list:
        ae, hop = self.ae, self.state.layout.hop
        B, m = len(ids), plan.emit1 - plan.emit0
        ids_t = self.state.lane_ids(ids)
        cur = torch.cuda.current_stream(ae.dev)
        ae.stream.wait_stream(cur)
        with torch.cuda.stream(ae.stream):
            need = self.state.scratch_halfs(plan, B)[1]
            if self._arena is None or self._arena.numel() < need:
                self._arena = None  # freed before the larger one is allocated
                self._arena = torch.empty(need, dtype=torch.float16, device=ae.dev)
            out = torch.empty(B, hop * m, dtype=torch.float32, device=ae.dev)
            self.state.run(plan, ids_t, torch.stack([c.contiguous() for c in codes]), self._arena, out)
        cur.wait_stream(ae.stream)
        out.record_stream(cur)
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
        self._bufs = None

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
            self.c1_w, self.c1_b = conv_w(sd["decoder.conv1.weight"]), f32(sd["decoder.conv1.bias"])
            self.c1_cin, self.c1_cout = sd["decoder.conv1.weight"].shape[1], sd["decoder.conv1.weight"].shape[0]
            self.blocks = []
            for j, s in enumerate(STRIDES):
                p = f"decoder.block.{j}."
                wt = sd[p + "conv_t1.weight"].to(self.dev, torch.float32)  # [cin][cout][2s]
                pad = math.ceil(s / 2)
                blk = dict(stride=s, pad=pad, cin=wt.shape[0], cout=wt.shape[1],
                           alpha=f32(sd[p + "snake1.alpha"]).reshape(-1),
                           wt=pack_conv_transpose(wt, s, pad), bt=f32(sd[p + "conv_t1.bias"]), res=[])
                for u in range(3):
                    r = p + f"res_unit{u + 1}."
                    blk["res"].append(dict(a1=f32(sd[r + "snake1.alpha"]).reshape(-1),
                                           w1=conv_w(sd[r + "conv1.weight"]), b1=f32(sd[r + "conv1.bias"]),
                                           a2=f32(sd[r + "snake2.alpha"]).reshape(-1),
                                           w2=conv_w(sd[r + "conv2.weight"]), b2=f32(sd[r + "conv2.bias"])))
                self.blocks.append(blk)
            self.final_alpha = f32(sd["decoder.snake1.alpha"]).reshape(-1)
            self.out_w, self.out_b = pack_conv_out(f32(sd["decoder.conv2.weight"]),   # [1][96][7]
                                                   f32(sd["decoder.conv2.bias"]))
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

    def _buffers(self, T: int):
        need = 49152 * T  # max over stages of C x time (blocks 3 and 4: 192 x 256T = 96 x 512T)
        if self._bufs is None or self._bufs[0].numel() < need:
            with torch.cuda.stream(self.stream):
                self._bufs = [torch.empty(need, dtype=torch.float16, device=self.dev) for _ in range(4)]
        return self._bufs

    # --------------------------------------------------------------- decode
    def _conv(self, x, t_in, c_in, w, b, c_out, taps, step, off, n_out, stride, phase, t_out, skip=None, raw=None,
              snake=None, alpha=None, f32=None):
        p = _lib.ptr
        _lib.check(self.lib.zmi_dac_conv(p(x), t_in, c_in, p(w), p(b), c_out, taps, step, off, n_out, stride, phase,
                                         t_out, p(skip), p(raw), p(snake), p(alpha), p(f32), self.sptr), "dac_conv")

    def _decode_one(self, codes: torch.Tensor, out: torch.Tensor, bufs=None, crop=None):
        """codes [9, T] int64 (device) -> out [512 T] fp32 (modeling_dac.py:347-371, 407-441).
        bufs: the four stage buffers (default: the decoder's own, grown to T). crop = (q0, n): only samples
        q0 .. q0 + n - 1 are computed by the last stage, into out [n] (the streaming decoder's window crop)."""
        T = codes.shape[-1]
        H, SA, SB, S2 = self._buffers(T) if bufs is None else bufs
        z = S2
        _lib.check(self.lib.zmi_dac_from_codes(codes.data_ptr(), T, self.codebooks.data_ptr(), self.proj_w.data_ptr(),
                                               self.proj_b.data_ptr(), z.data_ptr(), self.sptr), "from_codes")
        c = self.c1_cout
        # conv1 (k7, pad 3) -> Snake of block 0 (its only consumer is block 0's ConvTranspose)
        self._conv(z, T, self.c1_cin, self.c1_w, self.c1_b, c, 7, 1, -3, T, 1, 0, T, snake=SA,
                   alpha=self.blocks[0]["alpha"])
        t = T
        xin, xalt = SA, SB
        for j, blk in enumerate(self.blocks):
            s, cin, cout = blk["stride"], blk["cin"], blk["cout"]
            tn = t * s
            res = blk["res"]
            # ConvTranspose1d(k=2s, s, pad=ceil(s/2)), every phase in one launch
            _lib.check(self.lib.zmi_dac_conv_t(xin.data_ptr(), t, cin, blk["wt"].data_ptr(), blk["bt"].data_ptr(),
                                               cout, s, blk["pad"], H.data_ptr(), xalt.data_ptr(),
                                               res[0]["a1"].data_ptr(), self.sptr), "dac_conv_t")
            for u, dil in enumerate(DILATIONS):
                ru = res[u]
                self._conv(xalt, tn, cout, ru["w1"], ru["b1"], cout, 7, dil, -3 * dil, tn, 1, 0, tn, snake=S2,
                           alpha=ru["a2"])
                last_unit = u == len(DILATIONS) - 1
                if not last_unit:
                    nxt = res[u + 1]["a1"]
                elif j + 1 < len(self.blocks):
                    nxt = self.blocks[j + 1]["alpha"]
                else:
                    nxt = self.final_alpha
                self._conv(S2, tn, cout, ru["w2"], ru["b2"], cout, 1, 0, 0, tn, 1, 0, tn, skip=H,
                           raw=None if last_unit else H, snake=xalt, alpha=nxt)
            t = tn
            xin, xalt = xalt, xin
        if crop is not None:
            _lib.check(self.lib.zmi_dac_conv_out_range(xin.data_ptr(), t, self.blocks[-1]["cout"],
                                                       self.out_w.data_ptr(), self.out_b.data_ptr(), crop[0], crop[1],
                                                       out.data_ptr(), self.sptr), "conv_out_range")
            return
        _lib.check(self.lib.zmi_dac_conv_out(xin.data_ptr(), t, self.blocks[-1]["cout"], self.out_w.data_ptr(),
                                             self.out_b.data_ptr(), out.data_ptr(), self.sptr), "conv_out")

    def _decode_lanes(self, codes: torch.Tensor, out: torch.Tensor, bufs, crop=None):
        """_decode_one over B utterances of one length in the same 31 launches (the zmi_dac_*_lanes entry points):
        codes [B, 9, T] int64 contiguous (device) -> out [B, n] fp32 contiguous. bufs: four stage buffers of at least
        B x 49152 T halfs each; every stage's activations are [B][t][c] dense, so a lane's stride is that stage's
        t x c. crop = (q0, n): samples q0 .. q0 + n - 1 of every lane (default: all 512 T). Each lane's samples have
        the bits _decode_one gives them (the lanes entry points' contract, tests/test_gpu_dac_lanes.py)."""
        B, _, T = codes.shape
        assert codes.is_contiguous() and out.is_contiguous() and out.shape[0] == B
        assert all(b.numel() >= B * STAGE_HALFS_PER_FRAME * T for b in bufs)
        H, SA, SB, S2 = bufs
        lib, p, ck = self.lib, _lib.ptr, _lib.check

        def conv(x, t_in, c_in, w, b, c_out, taps, step, off, n_out, skip=None, raw=None, snake=None, alpha=None):
            ls_in, ls_out = t_in * c_in, n_out * c_out
            ck(lib.zmi_dac_conv_lanes(p(x), t_in, c_in, p(w), p(b), c_out, taps, step, off, n_out, 1, 0, n_out, p(skip),
                                      p(raw), p(snake), p(alpha), None, B, ls_in, ls_out, ls_out, ls_out, 0,
                                      self.sptr), "dac_conv_lanes")

        z = S2
        ck(lib.zmi_dac_from_codes_lanes(codes.data_ptr(), T, self.codebooks.data_ptr(), self.proj_w.data_ptr(),
                                        self.proj_b.data_ptr(), z.data_ptr(), B, N_CODEBOOKS * T, 1024 * T, self.sptr),
           "from_codes_lanes")
        conv(z, T, self.c1_cin, self.c1_w, self.c1_b, self.c1_cout, 7, 1, -3, T, snake=SA,
             alpha=self.blocks[0]["alpha"])
        t = T
        xin, xalt = SA, SB
        for j, blk in enumerate(self.blocks):
            s, cin, cout = blk["stride"], blk["cin"], blk["cout"]
            tn = t * s
            res = blk["res"]
            ck(lib.zmi_dac_conv_t_lanes(xin.data_ptr(), t, cin, blk["wt"].data_ptr(), blk["bt"].data_ptr(), cout, s,
                                        blk["pad"], H.data_ptr(), xalt.data_ptr(), res[0]["a1"].data_ptr(), B,
                                        t * cin, tn * cout, tn * cout, self.sptr), "dac_conv_t_lanes")
            for u, dil in enumerate(DILATIONS):
                ru = res[u]
                conv(xalt, tn, cout, ru["w1"], ru["b1"], cout, 7, dil, -3 * dil, tn, snake=S2, alpha=ru["a2"])
                last_unit = u == len(DILATIONS) - 1
                if not last_unit:
                    nxt = res[u + 1]["a1"]
                elif j + 1 < len(self.blocks):
                    nxt = self.blocks[j + 1]["alpha"]
                else:
                    nxt = self.final_alpha
                conv(S2, tn, cout, ru["w2"], ru["b2"], cout, 1, 0, 0, tn, skip=H, raw=None if last_unit else H,
                     snake=xalt, alpha=nxt)
            t = tn
            xin, xalt = xalt, xin
        q0, n = (0, t) if crop is None else crop
        assert out.shape[1] == n
        ck(lib.zmi_dac_conv_out_range_lanes(xin.data_ptr(), t, self.blocks[-1]["cout"], self.out_w.data_ptr(),
                                            self.out_b.data_ptr(), q0, n, out.data_ptr(), B,
                                            t * self.blocks[-1]["cout"], n, self.sptr), "conv_out_range_lanes")

    # stage memory of one decode() launch sequence over several utterances (4 buffers x 49152 T halfs per lane)
    DECODE_LANES_BYTES = 1 << 30

    @torch.inference_mode()
    def decode(self, codes: torch.Tensor) -> torch.Tensor:
        """[B, 9, T] codes -> [B, 1, 512 T] fp32 waveform (reference autoencoder.py:25-27). B > 1: the utterances
        share T, so they are lanes of one launch sequence (as many at a time as DECODE_LANES_BYTES of stage memory
        hold), each with the bits its own decode() gives."""
        B, nq, T = codes.shape
        assert nq == N_CODEBOOKS
        out = torch.empty(B, 1, DAC_HOP * T, dtype=torch.float32, device=self.dev)
        cur = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            codes = codes.to(self.dev, torch.int64).contiguous()
            if B == 1:
                self._decode_one(codes[0], out[0, 0])
            elif T > 0:
                per = max(1, min(B, 4096, self.DECODE_LANES_BYTES // (4 * 2 * STAGE_HALFS_PER_FRAME * T)))
                bufs = [torch.empty(per * STAGE_HALFS_PER_FRAME * T, dtype=torch.float16, device=self.dev)
                        for _ in range(4)]
                for b in range(0, B, per):
                    self._decode_lanes(codes[b: b + per], out[b: b + per, 0], bufs)
        cur.wait_stream(self.stream)
        return out

    def carry_layout(self) -> CarryLayout:
        """The carried-state planner of this decoder's layer list (streaming.CarryLayout)."""
        if getattr(self, "_carry_layout", None) is None:
            self._carry_layout = CarryLayout(STRIDES, DILATIONS, DAC_LOOKAHEAD_FRAMES)
            assert self._carry_layout.hop == DAC_HOP
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
        cur = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            out = rs(wav.to(self.dev))
        cur.wait_stream(self.stream)
        out.record_stream(cur)
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
            nxt = self.eblocks[j + 1]["res"][0]["a1"] if j + 1 < len(self.eblocks) else self.e_final_alpha
            # strided conv on the polyphase view of SA ([t][c] read as [t/s][s c]): 3 taps, in_off -1
            self._conv(SA, tn, s * c, blk["w"], blk["b"], 2 * c, 3, 1, -1, tn, 1, 0, tn,
                       raw=H if j + 1 < len(self.eblocks) else None, snake=S2, alpha=nxt)
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
        cur = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            wav = wav.to(self.dev, torch.float32).contiguous()
            lat = torch.empty(T, 1024, dtype=torch.float32, device=self.dev)
            for b in range(B):
                self.encode_latents(wav[b, 0], lat)
                self.quantize(lat, out[b])
        cur.wait_stream(self.stream)
        return out

    def quantize(self, lat: torch.Tensor, codes: torch.Tensor):
        """lat [T][1024] fp32 -> codes [9][T] int64 (residual VQ, modeling_dac.py:283-345)."""
        T = lat.shape[0]
        _lib.check(self.lib.zmi_dac_vq(lat.data_ptr(), T, self.vq_in_w.data_ptr(), self.vq_in_b.data_ptr(),
                                       self.codebooks.data_ptr(), self.cb_n.data_ptr(), self.cb_n2.data_ptr(),
                                       self.proj_w.data_ptr(), self.proj_b.data_ptr(), codes.data_ptr(), self.sptr),
                   "dac_vq")
