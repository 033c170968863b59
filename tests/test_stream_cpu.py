"""CPU checks of the streaming DAC decode: the derived lookahead against the oracle's real dependency range, the
derivation on a toy layer list, and DACStreamDecoder's window / crop bookkeeping over the oracle's decode."""
import pytest
import torch
from tests.helpers import dac_weights
from tests.stream_cases import CHUNKS, PATTERNS, lengths, pushes, random_codes, run_stream

from oracle.dac_cpu import OracleDAC
from zonos_vibes_amd import synthetic as syn
from zonos_vibes_amd.streaming import (DAC_LOOKAHEAD_FRAMES, CarryLayout, DACStreamDecoder, dac_lookahead_frames,
                                       dac_stages)


@pytest.fixture(scope="module")
def oracle():
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    return OracleDAC(dac_weights(0))


def test_lookahead_is_derived_from_the_layer_list():
    assert DAC_LOOKAHEAD_FRAMES == dac_lookahead_frames(syn.DAC_STRIDES, syn.DAC_DILATIONS) == 10


def test_lookahead_toy_layer_list():
    """One stride-2 block with one residual unit of dilation 1; a frame is 2 samples [0, 1].
    decoder.conv2 k7: [-3, 4]; the unit's k7: [-6, 7]; ConvTranspose(k4, s2, p1): out[n] reads x[(n + 1) // 2 - 1] and
    x[(n + 1) // 2], so [-5 // 2 - 1, 8 // 2] = [-4, 4]; conv1 k7: [-7, 7]  ->  7 frames."""
    assert dac_lookahead_frames((2,), (1,)) == 7
    # no upsampling, no residual unit: the two k7 convs and the 2-tap transposed conv (k2, s1, p1: x[n], x[n + 1])
    assert dac_lookahead_frames((1,), ()) == 7


TOY_NAMES = [f"decoder.{n}" for n in (
    "conv1.weight", "conv1.bias", "block.0.snake1.alpha", "block.0.conv_t1.weight", "block.0.conv_t1.bias",
    "block.0.res_unit1.snake1.alpha", "block.0.res_unit1.conv1.weight", "block.0.res_unit1.conv1.bias",
    "block.0.res_unit1.snake2.alpha", "block.0.res_unit1.conv2.weight", "block.0.res_unit1.conv2.bias",
    "snake1.alpha", "conv2.weight", "conv2.bias")]


@pytest.mark.parametrize("strides, dilations, names", [
    (syn.DAC_STRIDES, syn.DAC_DILATIONS, [sp.name for sp in syn.dac_specs() if sp.name.startswith("decoder.")]),
    ((2,), (1,), TOY_NAMES)], ids=["dac", "toy"])
def test_stage_list(strides, dilations, names):
    """The one statement of the decoder's launches: their count and order, the state_dict names they carry (every
    decoder tensor exactly once), the Snake a 1x1 conv's output is stored under, and that CarryLayout walks it."""
    stages = dac_stages(strides, dilations)
    kinds = [st["kind"] for st in stages]
    assert len(stages) == 2 + (1 + 2 * len(dilations)) * len(strides) + 1  # three dilations: 2 + 7 blocks + 1
    assert len(stages) == 31 or strides != syn.DAC_STRIDES
    assert kinds == ["codes", "k7"] + (["convt"] + ["k7", "pw"] * len(dilations)) * len(strides) + ["out"]
    units = [(st["block"], st["unit"]) for st in stages if st["kind"] == "pw"]
    assert units == [(j, u) for j in range(len(strides)) for u in range(len(dilations))]
    assert [st["d"] for st in stages if st["kind"] == "k7"] == [1] + list(dilations) * len(strides)
    assert [(st["s"], st["p"]) for st in stages if st["kind"] == "convt"] == [(s, -(-s // 2)) for s in strides]
    carried = [st["w"] + end for st in stages if "w" in st for end in (".weight", ".bias")] + \
        [st["alpha"] for st in stages if "alpha" in st]
    assert len(carried) == len(set(carried)) and sorted(carried) == sorted(names)
    assert "w" not in stages[0] and "alpha" not in stages[0] and "alpha" not in stages[-1]
    for i, st in enumerate(stages):
        if st["kind"] != "pw":
            continue
        reader = stages[i + 1]  # what consumes the unit's output: the next unit's k7, a transposed conv, or conv2
        snake1 = {"k7": lambda r: r["w"][: -len("conv1")] + "snake1.alpha",
                  "convt": lambda r: r["w"][: -len("conv_t1")] + "snake1.alpha",
                  "out": lambda r: r["w"][: -len("conv2")] + "snake1.alpha"}[reader["kind"]](reader)
        assert st["alpha"] == snake1 and reader["src"] == st["dst"], (st, reader)
    assert CarryLayout(strides, dilations).stages == stages


def test_lookahead_against_the_oracle(oracle):
    """Changing frame 24 changes samples only within R frames of it, and R - 1 would not cover them."""
    R = dac_lookahead_frames(syn.DAC_STRIDES, syn.DAC_DILATIONS)
    codes = random_codes(48, seed=1)
    other = codes.clone()
    other[:, :, 24] = (codes[:, :, 24] + 1 + torch.arange(9) * 57) % 1024
    assert (other[:, :, 24] != codes[:, :, 24]).all()
    diff = (oracle.decode(codes) - oracle.decode(other))[0, 0] != 0
    idx = diff.nonzero().flatten()
    first, last = int(idx[0]), int(idx[-1])
    assert 512 * (24 - R) <= first and last < 512 * (25 + R), (first, last)
    assert first < 512 * (24 - (R - 1)) or last >= 512 * (25 + (R - 1)), (first, last)


def thin_weights(w: dict, f: int = 8) -> dict:
    """The synthetic decoder with every hidden width (1536 .. 96) cut to 1 / f: the same layer list (strides, kernels,
    dilations, so the same lookahead) at 1 / f^2 of the cost; OracleDAC takes its widths from the weights."""
    widths = {1536, 768, 384, 192, 96}
    out = {}
    for k, t in w.items():
        for dim, n in enumerate(t.shape):
            if k.startswith("decoder.") and n in widths:
                t = t.narrow(dim, 0, n // f)
        out[k] = t.contiguous()
    return out


@pytest.fixture(scope="module")
def oracle_thin():
    return OracleDAC(thin_weights(dac_weights(0)))


@pytest.mark.parametrize("chunk", CHUNKS)
def test_window_and_crop_bookkeeping(oracle_thin, chunk):
    """DACStreamDecoder's scheduling over the oracle's decode equals the oracle's decode of the whole utterance, for
    every length and push pattern of the GPU test. The full-width oracle takes 7 ms per frame on 8 threads and the
    one-frame pushes alone decode 1600 frames, so this sweep runs the thin decoder (same layer list); the full-width
    one runs one case below. Measured here: thin output amplitude 0.023; cropping one frame early gives max |diff|
    8.3e-3, no halo 1.4e-2; the oracle's own position-dependent fp32 noise (oneDNN blocks by length) 1.1e-8. The
    bound is 1e-6: the issue's atol 1e-4 scaled by the thin decoder's amplitude, two decades above the noise."""
    oracle = oracle_thin
    calls = []

    def decode_window(codes, f0, f1):
        calls.append((codes.shape[1], f0, f1))
        return oracle.decode(codes[None])[..., 512 * f0: 512 * f1]

    dec = DACStreamDecoder(decode_window, chunk_frames=chunk)
    worst = 0.0
    for T in lengths(chunk):
        codes = random_codes(T, seed=T)
        want = oracle.decode(codes)
        for pattern in PATTERNS:
            calls.clear()
            got = run_stream(dec, codes, pushes(pattern, T))
            assert got.shape == want.shape, (T, pattern)
            err = float((got - want).abs().max())
            worst = max(worst, err)
            assert err <= 1e-6, (T, pattern, err)
            assert all(w <= 2 * DAC_LOOKAHEAD_FRAMES + chunk and f1 - f0 <= chunk for w, f0, f1 in calls)
            assert sum(f1 - f0 for _, f0, f1 in calls) == T  # every frame decoded for output exactly once
    print(f"chunk {chunk}: max |stream - offline| {worst:.2e}")


def test_window_and_crop_full_width(oracle):
    """One case on the full-width synthetic decoder at atol 1e-4: an off-by-one crop gives errors of order 0.1 on its
    tanh output (measured: one frame early 0.19), oneDNN's position-dependent fp32 noise is of order 1e-6 (measured
    max |diff| 2.8e-7 over every length and pattern of stream_cases at chunk 4 and 16)."""
    chunk = 16
    T = lengths(chunk)[4]
    codes = random_codes(T, seed=T)
    dec = DACStreamDecoder(lambda c, f0, f1: oracle.decode(c[None])[..., 512 * f0: 512 * f1], chunk_frames=chunk)
    got = run_stream(dec, codes, pushes("ragged", T))
    want = oracle.decode(codes)
    err = float((got - want).abs().max())
    print(f"full width: max |stream - offline| {err:.2e}")
    assert got.shape == want.shape and err <= 1e-4, err


def test_push_returns_every_frame_whose_lookahead_is_known():
    R, hop = DAC_LOOKAHEAD_FRAMES, 512
    dec = DACStreamDecoder(lambda c, f0, f1: torch.zeros(1, 1, hop * (f1 - f0)), chunk_frames=4)
    assert dec.push(torch.zeros(9, 0, dtype=torch.int64)).shape == (1, 1, 0)
    assert dec.push(torch.zeros(9, R, dtype=torch.int64)).shape == (1, 1, 0)
    assert dec.push(torch.zeros(1, 9, 7, dtype=torch.int64)).shape == (1, 1, hop * 7)
    assert dec.flush().shape == (1, 1, hop * R)
    assert dec.flush().shape == (1, 1, 0) and dec.frames_received == 0  # ready for the next utterance
    with pytest.raises(ValueError):
        dec.push(torch.zeros(2, 9, 3, dtype=torch.int64))
