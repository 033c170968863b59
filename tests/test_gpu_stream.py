"""Streaming on the GPU: zmi_delay_revert_range, DACStreamDecoder and Zonos.stream, each bit for bit against the
offline path (zmi_delay_revert, DACAutoencoder.decode, decode(generate()))."""
import ctypes

import numpy as np
import pytest
import torch

from tests.stream_cases import CHUNKS, PATTERNS, lengths, pushes, random_codes, run_stream
from zonos_vibes_amd import synthetic as syn
from zonos_vibes_amd.config import tiny_hybrid, tiny_transformer

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------ zmi_delay_revert_range
@pytest.fixture(scope="module")
def delayed_slots(gpu_lib):
    """Two slots of 320 columns; slot 1 initialised by zmi_delay_init (7-frame prefix), then columns 12 .. 99 written
    by hand with codes, EOS (1024), mask (1025) and the not-yet-sampled marker (-1)."""
    from zonos_vibes_amd import _lib as L
    S, tcap = 2, 320
    st = {k: torch.zeros(S, dtype=torch.int32, device=DEV) for k in
          ("active", "pos", "offset", "remaining", "stopping", "step", "total_len")}
    delayed = torch.full((S, 9, tcap), 1025, dtype=torch.int32, device=DEV)
    params = torch.zeros(S * ctypes.sizeof(L.Sampling), dtype=torch.uint8, device=DEV)
    sl = L.Slots(*(st[k].data_ptr() for k in ("active", "pos", "offset", "remaining", "stopping", "step")),
                 delayed.data_ptr(), params.data_ptr(), st["total_len"].data_ptr(), tcap, S)
    g = torch.Generator().manual_seed(3)
    prefix = torch.randint(0, 1024, (9, 7), generator=g, dtype=torch.int32).to(DEV)
    sp = torch.cuda.current_stream().cuda_stream
    L.check(gpu_lib.zmi_delay_init(ctypes.byref(sl), 1, prefix.data_ptr(), 7, tcap, sp))
    hand = torch.randint(0, 1024, (9, 88), generator=g, dtype=torch.int32)
    hand[torch.rand(9, 88, generator=g) < 0.2] = 1024
    hand[torch.rand(9, 88, generator=g) < 0.1] = 1025
    hand[torch.rand(9, 88, generator=g) < 0.05] = -1
    delayed[1, :, 12:100] = hand.to(DEV)
    full = torch.full((9, tcap - 9), -7, dtype=torch.int64, device=DEV)
    L.check(gpu_lib.zmi_delay_revert(ctypes.byref(sl), 1, full.data_ptr(), tcap - 9, sp))
    torch.cuda.synchronize()
    assert (hand >= 1024).any() and (full[:, :100] == 0).any()
    return sl, full.cpu(), (st, delayed, params, prefix)


@pytest.mark.parametrize("t0", [0, 1, 7])
@pytest.mark.parametrize("n", [1, 9, 300])
def test_delay_revert_range_equals_slice(gpu_lib, delayed_slots, t0, n):
    from zonos_vibes_amd import _lib as L
    sl, full, _ = delayed_slots
    out = torch.full((9, n), -7, dtype=torch.int64, device=DEV)
    L.check(gpu_lib.zmi_delay_revert_range(ctypes.byref(sl), 1, t0, n, out.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), full[:, t0: t0 + n])


def test_delay_revert_range_empty_and_argument_errors(gpu_lib, delayed_slots):
    sl, _, _ = delayed_slots
    sp = torch.cuda.current_stream().cuda_stream
    out = torch.full((9, 4), -7, dtype=torch.int64, device=DEV)
    assert gpu_lib.zmi_delay_revert_range(ctypes.byref(sl), 1, 5, 0, out.data_ptr(), sp) == 0
    assert gpu_lib.zmi_delay_revert_range(ctypes.byref(sl), 1, 311, 0, out.data_ptr(), sp) == 0
    # argument checks: they return the library's error code (-1, as zmi_delay_revert's) before any launch
    assert gpu_lib.zmi_delay_revert_range(ctypes.byref(sl), 1, 7, 305, out.data_ptr(), sp) == -1   # 7 + 305 + 9 > 320
    assert gpu_lib.zmi_delay_revert_range(ctypes.byref(sl), 1, -1, 4, out.data_ptr(), sp) == -1
    assert gpu_lib.zmi_delay_revert_range(ctypes.byref(sl), 1, 0, -1, out.data_ptr(), sp) == -1
    assert gpu_lib.zmi_delay_revert_range(ctypes.byref(sl), 2, 0, 4, out.data_ptr(), sp) == -1     # slot out of range
    assert b"delay_revert_range" in gpu_lib.zmi_last_error()
    torch.cuda.synchronize()
    assert (out == -7).all()  # nothing ran


# ------------------------------------------------------------------ DACStreamDecoder
@pytest.fixture(scope="module")
def dac():
    from zonos_vibes_amd.autoencoder import DACAutoencoder
    return DACAutoencoder(DEV)


@pytest.fixture(scope="module")
def offline(dac):
    """decode() of each test utterance, computed once."""
    out = {}
    for T in sorted({T for c in CHUNKS for T in lengths(c)}):
        codes = random_codes(T, seed=T).to(DEV)
        out[T] = (codes, dac.decode(codes))
    return out


@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_stream_decoder_equals_decode(dac, offline, chunk, capture):
    """Every split of the codes into pushes gives decode()'s bits: the window's K order per output does not depend
    on the window's length or on where in a tile a sample falls. With and without the captured steady-state graph."""
    dec = dac.stream_decoder(chunk, capture=capture)
    win = dec.decode_window
    for T in lengths(chunk):
        codes, want = offline[T]
        for pattern in PATTERNS:
            got = run_stream(dec, codes, pushes(pattern, T))
            assert got.shape == want.shape and got.dtype == torch.float32 and got.device == want.device
            assert torch.equal(got, want), (T, pattern, float((got - want).abs().max()))
    # T = 75 in whole chunks takes the steady-state shape for every window with both halos whole
    assert (win.graph_replays > 0) == capture
    codes, want = offline[75]
    assert torch.equal(run_stream(dec, codes, pushes("ragged", 75)), want)  # same object again: no state left over


def test_stream_decoder_survives_a_larger_offline_decode(dac, offline):
    """The captured window graph keeps its own stage buffers: an offline decode that regrows the decoder's buffers
    between two streams does not disturb it."""
    dec = dac.stream_decoder(4)
    codes, want = offline[75]
    assert torch.equal(run_stream(dec, codes, pushes("all", 75)), want)
    big = random_codes(300, seed=300).to(DEV)
    dac.decode(big)
    assert torch.equal(run_stream(dec, codes, pushes("all", 75)), want)


# ------------------------------------------------------------------ Zonos.stream
def _cond(seed, lc, d=512):
    return torch.from_numpy(syn.synthetic_conditioning_np(seed, 2, lc, d).view(np.int16).copy()).view(torch.bfloat16).to(DEV)


def _build(cfg, **kw):
    from zonos_vibes_amd.model import Zonos
    return Zonos.synthetic(cfg, DEV, max_seqlen=128, max_prefill=64, **kw)


@pytest.fixture(scope="module")
def model_no_eos():
    return _build(tiny_transformer(), zero_eos=True)


@pytest.fixture(scope="module")
def model_eos():
    return _build(tiny_transformer(), eos_row_scale=6.0)


def _both(model, seed, cond, chunk_frames=16, **kw):
    """(codes, decode(generate()), the chunks of stream()) under the same torch.manual_seed."""
    torch.manual_seed(seed)
    codes = model.generate(cond, progress_bar=False, **kw)
    want = model.autoencoder.decode(codes)
    torch.manual_seed(seed)
    chunks = list(model.stream(cond, chunk_frames=chunk_frames, **kw))
    return codes, want, chunks


def _check(codes, want, chunks):
    assert all(c.dim() == 3 and c.shape[:2] == (1, 1) and c.shape[-1] % 512 == 0 and c.shape[-1] > 0 for c in chunks)
    got = torch.cat(chunks, dim=-1)
    assert got.shape == want.shape, (got.shape, want.shape, codes.shape)
    assert torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize("params", [dict(temperature=0.0), dict(min_p=0.1)], ids=["greedy", "min_p"])
@pytest.mark.parametrize("n", [5, 40])
def test_stream_equals_generate_then_decode(model_no_eos, params, n):
    codes, want, chunks = _both(model_no_eos, 100 + n, _cond(11, 12), max_new_tokens=n, sampling_params=params)
    assert codes.shape[-1] == n  # ended by max_new_tokens
    _check(codes, want, chunks)
    if n == 5:
        assert len(chunks) == 1  # shorter than the lookahead: everything comes from flush()
    else:
        assert len(chunks) > 1


@pytest.mark.parametrize("chunk_frames", [4, 16])
def test_stream_with_audio_prefix(model_no_eos, chunk_frames):
    prefix = random_codes(12, seed=5).to(DEV)
    codes, want, chunks = _both(model_no_eos, 7, _cond(12, 9), chunk_frames, audio_prefix_codes=prefix,
                                max_new_tokens=40, sampling_params=dict(min_p=0.1))
    assert codes.shape[-1] == 52 and torch.equal(codes[..., :12], prefix)
    _check(codes, want, chunks)


def test_stream_ended_by_eos(model_eos, model_no_eos):
    """The same request on a model whose EOS row is scaled up ends early (EOS countdown), on the one whose EOS row
    is zero it runs to max_new_tokens: neither case is vacuous."""
    cond = _cond(23, 10)
    kw = dict(max_new_tokens=40, sampling_params=dict(temperature=0.0))
    codes, want, chunks = _both(model_eos, 1, cond, 4, **kw)
    assert 0 < codes.shape[-1] <= 20, codes.shape  # well before max_new_tokens
    _check(codes, want, chunks)
    codes, want, chunks = _both(model_no_eos, 1, cond, 4, **kw)
    assert codes.shape[-1] == 40
    _check(codes, want, chunks)


def test_stream_hybrid():
    model = _build(tiny_hybrid(), zero_eos=True)
    codes, want, chunks = _both(model, 3, _cond(14, 10), 8, max_new_tokens=30, sampling_params=dict(min_p=0.1))
    assert codes.shape[-1] == 30
    _check(codes, want, chunks)


def test_stream_closed_early_leaves_the_model_as_new(model_no_eos):
    cond = _cond(11, 12)
    gen = model_no_eos.stream(cond, max_new_tokens=40, sampling_params=dict(min_p=0.1), chunk_frames=4)
    first = next(gen)
    assert first.shape[-1] > 0
    gen.close()
    torch.manual_seed(9)
    after = model_no_eos.generate(cond, max_new_tokens=24, progress_bar=False)
    fresh = _build(tiny_transformer(), zero_eos=True)
    torch.manual_seed(9)
    assert torch.equal(after, fresh.generate(cond, max_new_tokens=24, progress_bar=False))
    # and a stream after the closed one is whole again
    _check(*_both(model_no_eos, 9, cond, 4, max_new_tokens=24, sampling_params=dict(min_p=0.1)))
