"""CPU checks of the carried-state streaming DAC decode (streaming.CarryLayout / CarryPlan and the decoders over
them): the planner, run over a float64 torch restatement of the layer list, against that restatement's decode of the
whole utterance; the steady-state plan's row counts; the two wrong plans the comparison must reject."""
import math

import pytest
import torch
import torch.nn.functional as F
from tests.helpers import dac_weights
from tests.stream_cases import PATTERNS, lengths, pushes, random_codes, run_stream
from tests.test_stream_cpu import thin_weights

from zonos_vibes_amd import synthetic as syn
from zonos_vibes_amd.streaming import (CarryLayout, DACCarryBatchStreamDecoder, DACCarryStreamDecoder, DACStreamDecoder,
                                       dac_lookahead_frames)

CHUNKS = (1, 4, 16)
# Measured with this file (printed by the sweeps below): the restatement's incremental decode differs from its
# whole-utterance decode by at most 2.4e-17 in float64 on the thin DAC decoder (output amplitude 0.023; the conv
# library's blocking depends on the length), against 8.3e-3 for an off-by-one-frame crop of the same decoder
# (test_stream_cpu.py) and 1.1e-8 of fp32 noise; on the toy decoder (random weights of scale 0.3, activations of order
# 10, output of order 1) by at most 2.5e-14. Each bound is two decades above its decoder's float64 noise.
BOUNDS = {}


def snake(x, alpha):
    return x + (alpha + 1e-9).reciprocal() * torch.sin(alpha * x).pow(2)


def toy_weights(strides, dilations, seed=0, width=8):
    """A random decoder of the given layer list in the DAC's state_dict names: 9 codebooks of 16 entries, latent 16,
    hidden widths width * 2^blocks halving per block."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64) * 0.3  # noqa: E731
    w = {}
    for i in range(9):
        p = f"quantizer.quantizers.{i}."
        w[p + "codebook.weight"], w[p + "out_proj.weight"], w[p + "out_proj.bias"] = r(1024, 4), r(16, 4, 1), r(16)
    c = width * 2 ** len(strides)
    w["decoder.conv1.weight"], w["decoder.conv1.bias"] = r(c, 16, 7), r(c)
    for j, s in enumerate(strides):
        p = f"decoder.block.{j}."
        w[p + "snake1.alpha"] = r(1, c, 1).abs() + 0.5
        w[p + "conv_t1.weight"], w[p + "conv_t1.bias"] = r(c, c // 2, 2 * s), r(c // 2)
        c //= 2
        for u in range(len(dilations)):
            q = p + f"res_unit{u + 1}."
            w[q + "snake1.alpha"], w[q + "snake2.alpha"] = r(1, c, 1).abs() + 0.5, r(1, c, 1).abs() + 0.5
            w[q + "conv1.weight"], w[q + "conv1.bias"] = r(c, c, 7), r(c)
            w[q + "conv2.weight"], w[q + "conv2.bias"] = r(c, c, 1), r(c)
    w["decoder.snake1.alpha"] = r(1, c, 1).abs() + 0.5
    w["decoder.conv2.weight"], w["decoder.conv2.bias"] = r(1, c, 7), r(1)
    return w


class Restatement:
    """The decoder of a layer list in float64: decode() of a whole utterance (F.conv1d / F.conv_transpose1d with their
    own padding) and step(), a CarryPlan run on [hist | new] slices with no padding at all: a row the plan reads
    outside a buffer's [hist | new] rows, or one not yet computed, reads as zero (what the kernels' bounds give)."""

    def __init__(self, w, strides, dilations):
        self.w = {k: v.double() for k, v in w.items()}
        self.strides, self.dilations = tuple(strides), tuple(dilations)
        self.state = None

    def from_codes(self, codes):  # [9, n] -> [C, n]
        q = 0.0
        for i in range(codes.shape[0]):
            p = f"quantizer.quantizers.{i}."
            lat = F.embedding(codes[i], self.w[p + "codebook.weight"]).t()[None]
            q = q + F.conv1d(lat, self.w[p + "out_proj.weight"], self.w[p + "out_proj.bias"])
        return q[0]

    def alpha_after(self, j, u):
        """The Snake that follows residual unit u of block j (its 1x1 conv's output is stored Snake'd)."""
        if u + 1 < len(self.dilations):
            return self.w[f"decoder.block.{j}.res_unit{u + 2}.snake1.alpha"][0]
        if j + 1 < len(self.strides):
            return self.w[f"decoder.block.{j + 1}.snake1.alpha"][0]
        return self.w["decoder.snake1.alpha"][0]

    @torch.inference_mode()
    def decode(self, codes):  # [1, 9, T] -> [1, 1, hop T]
        w = self.w
        h = F.conv1d(self.from_codes(codes[0])[None], w["decoder.conv1.weight"], w["decoder.conv1.bias"], padding=3)
        for j, s in enumerate(self.strides):
            p = f"decoder.block.{j}."
            h = F.conv_transpose1d(snake(h, w[p + "snake1.alpha"]), w[p + "conv_t1.weight"], w[p + "conv_t1.bias"],
                                   stride=s, padding=math.ceil(s / 2))
            for u, d in enumerate(self.dilations):
                q = p + f"res_unit{u + 1}."
                y = F.conv1d(snake(h, w[q + "snake1.alpha"]), w[q + "conv1.weight"], w[q + "conv1.bias"], dilation=d,
                             padding=3 * d)
                h = h + F.conv1d(snake(y, w[q + "snake2.alpha"]), w[q + "conv2.weight"], w[q + "conv2.bias"])
        h = F.conv1d(snake(h, w["decoder.snake1.alpha"]), w["decoder.conv2.weight"], w["decoder.conv2.bias"], padding=3)
        return torch.tanh(h)

    # ---------------------------------------------------------------------------------------------- incremental
    def reset(self, lane=None):
        self.state = None

    def snapshot(self):
        return dict(self.state)

    def restore(self, s):
        self.state = dict(s)

    @torch.inference_mode()
    def __call__(self, plan, codes):
        w, lay = self.w, plan.layout
        scratch, written = {}, {}

        def width(b):
            wd = lay.buffers[b].width
            if wd == "z":
                return w["decoder.conv1.weight"].shape[1]
            return w["decoder.conv1.weight"].shape[0] if wd == "c1" else w[f"decoder.block.{wd}.conv_t1.weight"].shape[1]

        for b, info in lay.buffers.items():
            scratch[b] = torch.zeros(width(b), plan.rows(b), dtype=torch.float64)
            if info.hist and not plan.first:
                scratch[b][:, :info.hist] = self.state[b]
            written[b] = info.hist  # local rows [0, written) hold values

        def read(b, lo, hi):  # absolute rows [lo, hi) of b; zero where outside its scratch or not yet written
            out = torch.zeros(scratch[b].shape[0], hi - lo, dtype=torch.float64)
            a, e = max(lo - plan.base[b], 0), min(hi - plan.base[b], written[b])
            if e > a:
                out[:, a + plan.base[b] - lo: e + plan.base[b] - lo] = scratch[b][:, a:e]
            return out

        def write(b, out0, val):
            if b is None:
                return
            a = out0 - plan.base[b]
            assert a == written[b] == lay.buffers[b].hist and val.shape[1] == plan.new[b], (b, a, written[b])
            scratch[b][:, a: a + val.shape[1]] = val
            written[b] = a + val.shape[1]

        wav = None
        for st in plan.steps:
            k, n_out, out0 = st["kind"], st["n_out"], st["out0"]
            if k == "codes":
                write(st["dst"], out0, self.from_codes(codes) if n_out else torch.zeros(scratch["z"].shape[0], 0).double())
            elif k in ("k7", "out"):
                d = st["d"]
                if k == "out":
                    wt, bias = w["decoder.conv2.weight"], w["decoder.conv2.bias"]
                elif "block" not in st:
                    wt, bias = w["decoder.conv1.weight"], w["decoder.conv1.bias"]
                else:
                    q = f"decoder.block.{st['block']}.res_unit{st['unit'] + 1}."
                    wt, bias = w[q + "conv1.weight"], w[q + "conv1.bias"]
                assert st["hi"] - st["lo"] == n_out + 6 * d
                y = F.conv1d(read(st["src"], st["lo"], st["hi"])[None], wt, bias, dilation=d)[0] if n_out else \
                    torch.zeros(wt.shape[0], 0, dtype=torch.float64)
                if k == "out":
                    wav = torch.tanh(y)[None]
                elif "block" not in st:
                    write(st["dst"], out0, snake(y, w["decoder.block.0.snake1.alpha"][0]))
                else:
                    write(st["dst"], out0, snake(y, w[q + "snake2.alpha"][0]))
            elif k == "pw":
                q = f"decoder.block.{st['block']}.res_unit{st['unit'] + 1}."
                y = read(st["skip"], out0, out0 + n_out)
                if n_out:
                    y = y + F.conv1d(read(st["src"], out0, out0 + n_out)[None], w[q + "conv2.weight"],
                                     w[q + "conv2.bias"])[0]
                write(st["raw"], out0, y)
                write(st["dst"], out0, snake(y, self.alpha_after(st["block"], st["unit"])))
            else:  # convt: the whole transposed conv of the rows read, cropped to the rows wanted
                p = f"decoder.block.{st['block']}."
                s, pad = st["s"], st["p"]
                if n_out:
                    x = read(st["src"], st["lo"], st["hi"])
                    full = F.conv_transpose1d(x[None], w[p + "conv_t1.weight"], w[p + "conv_t1.bias"], stride=s)[0]
                    # full[m] is output row s lo - pad + m ... of the unpadded form: row n = s i + k - pad
                    a = out0 - (s * st["lo"] - pad)
                    y = full[:, a: a + n_out]
                    assert y.shape[1] == n_out
                else:
                    y = torch.zeros(scratch[st["dst"]].shape[0], 0, dtype=torch.float64)
                write(st["raw"], out0, y)
                write(st["dst"], out0, snake(y, w[p + "res_unit1.snake1.alpha"][0]))
        if not plan.final:
            self.state = {b: scratch[b][:, plan.tail[b]: plan.tail[b] + lay.buffers[b].hist].clone() for b in plan.tail}
        return wav


DAC = (syn.DAC_STRIDES, syn.DAC_DILATIONS)
TOY = ((2,), (1,))
BOUNDS.update({DAC: 2.4e-15, TOY: 2.5e-12})


@pytest.fixture(scope="module")
def weights():
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    return {DAC: thin_weights(dac_weights(0)), TOY: toy_weights(*TOY)}


def toy_codes(T, seed):
    return random_codes(T, seed)


def sweep(model, layout, chunk, cases):
    """max |incremental - whole| over the cases; asserts the shapes and, per push, the frames a DACStreamDecoder
    returns for the same pushes."""
    hop = layout.hop
    dec = DACCarryStreamDecoder(model, layout, chunk_frames=chunk)
    win = DACStreamDecoder(lambda c, f0, f1: torch.zeros(1, 1, hop * (f1 - f0)), chunk_frames=chunk, lookahead=layout.R)
    worst = 0.0
    for T, pattern in cases:
        codes = random_codes(T, seed=T)
        want = model.decode(codes)
        sizes = pushes(pattern, T)
        got = run_stream(dec, codes, sizes) if hop == 512 else None
        if got is None:  # (run_stream asserts 512-sample frames)
            parts = [dec.push(codes[..., sum(sizes[:i]): sum(sizes[:i + 1])]) for i in range(len(sizes))] + [dec.flush()]
            got = torch.cat(parts, dim=-1)
        # the same pushes through the window decoder's bookkeeping: equal frames per push
        t, m_carry, m_win, dec2 = 0, [], [], DACCarryStreamDecoder(model, layout, chunk_frames=chunk)
        for n in sizes:
            m_carry.append(dec2.push(codes[..., t: t + n]).shape[-1])
            m_win.append(win.push(codes[..., t: t + n]).shape[-1])
            t += n
        m_carry.append(dec2.flush().shape[-1])
        m_win.append(win.flush().shape[-1])
        assert m_carry == m_win, (T, pattern)
        assert got.shape == want.shape, (T, pattern, got.shape, want.shape)
        worst = max(worst, float((got - want).abs().max()))
    return worst


@pytest.mark.parametrize("chunk", CHUNKS)
def test_plan_over_the_restatement_equals_whole_decode(weights, chunk):
    """Every lengths(chunk) x PATTERNS of stream_cases on the thin DAC decoder in float64. Measured: max |incremental -
    whole| 2.4e-17 (printed); the bound, 2.4e-15, is two decades above it and twelve below the 8.3e-3 of an
    off-by-one-frame crop."""
    model = Restatement(weights[DAC], *DAC)
    layout = CarryLayout(*DAC)
    worst = sweep(model, layout, chunk, [(T, p) for T in lengths(chunk) for p in PATTERNS])
    print(f"chunk {chunk}: max |carry - whole| {worst:.2e}")
    assert worst <= BOUNDS[DAC], worst


def test_toy_layer_list(weights):
    """One stride-2 block with one residual unit of dilation 1 (lookahead 7, hop 2): the same comparison. Measured
    2.5e-14 (printed); bound 2.5e-12."""
    model = Restatement(weights[TOY], *TOY)
    layout = CarryLayout(*TOY)
    assert layout.R == dac_lookahead_frames(*TOY) == 7 and layout.hop == 2
    worst = sweep(model, layout, 4, [(T, p) for T in (1, 7, 8, 15, 22, 40) for p in PATTERNS])
    print(f"toy: max |carry - whole| {worst:.2e}")
    assert worst <= BOUNDS[TOY], worst


@pytest.mark.parametrize("lay", [DAC, TOY])
def test_steady_state_plan(lay):
    """Past the start every stage computes exactly rate x n rows; over an utterance no row is computed twice (per stage
    the rows sum to rate x T, each push starting where the last ended); every row read lies in the source's [hist |
    new] and below its frontier (CarryPlan.check)."""
    layout = CarryLayout(*lay)
    rate = {b.name: b.rate for b in layout.buffers.values()}
    for n in (1, 4, 16):
        for recv in (layout.R, layout.R + 5, 40):
            plan = layout.plan(recv, n).check()
            assert plan.key == layout.plan(layout.R, n).key  # one launch shape whatever the position
            for st in plan.steps:
                want = layout.hop * n if st["kind"] == "out" else rate[st["dst"]] * n
                assert st["n_out"] == want, (st, want)
    for T in (1, 9, 10, 11, 37):
        for pattern in PATTERNS:
            sizes, recv = pushes(pattern, T), 0
            done = [0] * len(layout.stages)
            for i, n in enumerate(sizes + [0]):
                plan = layout.plan(recv, n, final=i == len(sizes)).check()
                for k, st in enumerate(plan.steps):
                    assert st["out0"] == done[k], (T, pattern, st)  # contiguous: nothing twice, nothing skipped
                    done[k] += st["n_out"]
                recv += n
            for k, st in enumerate(layout.stages):
                assert done[k] == (layout.hop if st["kind"] == "out" else rate[st["dst"]]) * T


def state_halfs(layout, widths):
    return sum(b.hist * widths[b.width] for b in layout.buffers.values())


def test_state_size_of_the_dac():
    """The carried rows per lane from the layer list: 117 rows per channel of a block (6 + 3 + 18 + 9 + 54 + 27), one row
    ahead of every transposed conv, 6 of z and 369 ahead of the last conv: 425,856 bytes in fp16."""
    layout = CarryLayout(*DAC)
    widths = {"z": 1024, "c1": 1536, 0: 768, 1: 384, 2: 192, 3: 96}
    assert layout.buffers[layout.last].hist == 512 * 10 - 4754 + 3 == 369
    assert 2 * state_halfs(layout, widths) == 425856


def mutants(lay):
    n7 = CarryLayout(*lay).k7_stages
    return [dict(k7_short=i) for i in range(n7)] + [dict(convt_frontier_pad=False)]


@pytest.mark.parametrize("lay", [DAC, TOY])
def test_wrong_plans_are_rejected_by_the_comparison(weights, lay):
    """One row less history at any k7 stage, or a transposed-conv frontier of s F instead of s F - p: the restatement
    over such a plan differs from the whole decode by far more than the bound (a missing row reads as zero). (The
    last k7 stage's history of whole frames ahead of recv - R is counted in the same way: its first row is read by
    the first sample of the next push.)"""
    model = Restatement(weights[lay], *lay)
    T = 40
    codes = random_codes(T, seed=3)
    want = model.decode(codes)
    for kw in mutants(lay):
        layout = CarryLayout(*lay, **kw)
        dec = DACCarryStreamDecoder(model, layout, chunk_frames=4)
        parts = [dec.push(codes[..., t: t + 4]) for t in range(0, T, 4)] + [dec.flush()]
        got = torch.cat(parts, dim=-1)
        err = float((got - want).abs().max()) if got.shape == want.shape else float("inf")
        print(f"{kw}: max |carry - whole| {err:.2e}")
        assert err > 1e3 * BOUNDS[lay], (kw, err)


def test_batch_decoder_groups_lanes_by_plan(weights):
    """DACCarryBatchStreamDecoder: staggered lanes, each equal to its own whole decode; lanes at different positions
    that push equal n in the steady state are one decode_steps call."""
    layout = CarryLayout(*TOY)
    lanes = {i: Restatement(weights[TOY], *TOY) for i in range(3)}
    calls = []

    class Steps:
        def __call__(self, plan, ids, codes):
            calls.append(tuple(ids))
            return [lanes[i](plan, c) for i, c in zip(ids, codes)]

        def reset(self, lane):
            lanes[lane].reset()

    dec = DACCarryBatchStreamDecoder(Steps(), layout, 3, chunk_frames=4)
    cs = {i: random_codes(30 + i, seed=i)[0] for i in range(3)}
    got = {i: [] for i in range(3)}
    got[0].append(dec.push({0: cs[0][:, :9]})[0])
    # lane 0 is mid-stream (9 frames in) when lane 1 starts; both then push 4 at a time
    out = dec.push({0: cs[0][:, 9:13], 1: cs[1][:, :12]})
    for i in out:
        got[i].append(out[i])
    calls.clear()
    out = dec.push({0: cs[0][:, 13:17], 1: cs[1][:, 12:16]})
    assert calls == [(0, 1)]
    for i in out:
        got[i].append(out[i])
    out = dec.push({0: cs[0][:, 17:], 1: cs[1][:, 16:], 2: cs[2]})
    for i in out:
        got[i].append(out[i])
    out = dec.flush([0, 1, 2])
    for i in out:
        got[i].append(out[i])
    ref = Restatement(weights[TOY], *TOY)
    for i in range(3):
        wav = torch.cat(got[i], dim=-1)
        want = ref.decode(cs[i][None])
        assert wav.shape == want.shape and float((wav - want).abs().max()) <= BOUNDS[TOY], i
    assert dec.frames_received(0) == 0


def test_bad_arguments():
    layout = CarryLayout(*TOY)
    with pytest.raises(ValueError):
        DACCarryStreamDecoder(None, layout, chunk_frames=0)
    with pytest.raises(ValueError):
        layout.plan(-1, 3)
    with pytest.raises(ValueError):
        CarryLayout((2,), ())
    dec = DACCarryStreamDecoder(Restatement(toy_weights(*TOY), *TOY), layout, 4)
    with pytest.raises(ValueError):
        dec.push(torch.zeros(2, 9, 3, dtype=torch.int64))
    assert dec.push(torch.zeros(9, 0, dtype=torch.int64)).shape == (1, 1, 0)
    assert dec.flush().shape == (1, 1, 0)
