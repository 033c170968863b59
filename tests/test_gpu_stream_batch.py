"""Batched streaming on the GPU: DACAutoencoder.decode over several utterances, stream_decoder_batch and
Zonos.stream_batch, each bit for bit against the per-utterance offline path (decode, decode(generate_batch()))."""
import numpy as np
import pytest
import torch

from tests.stream_cases import RAGGED, random_codes
from zonos_vibes_amd import synthetic as syn
from zonos_vibes_amd.config import tiny_hybrid, tiny_transformer

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def dac():
    from zonos_vibes_amd.autoencoder import DACAutoencoder
    return DACAutoencoder(DEV)


# ------------------------------------------------------------------ decode() over lanes
@pytest.mark.parametrize("T", [5, 37])
def test_decode_batch_equals_per_utterance(dac, T):
    codes = torch.cat([random_codes(T, seed=10 * T + b) for b in range(3)]).to(DEV)  # [3, 9, T]
    got = dac.decode(codes)
    assert got.shape == (3, 1, 512 * T) and got.dtype == torch.float32
    for b in range(3):
        assert torch.equal(got[b: b + 1], dac.decode(codes[b: b + 1])), b
    assert not torch.equal(got[0], got[1])


def test_decode_batch_in_several_launch_sequences(dac):
    """More utterances than the stage-memory budget holds at once: the same bits from sub-batches (here of 2, 1)."""
    codes = torch.cat([random_codes(9, seed=70 + b) for b in range(3)]).to(DEV)
    want = dac.decode(codes)
    old = dac.DECODE_LANES_BYTES
    try:
        dac.DECODE_LANES_BYTES = 2 * 4 * 2 * 49152 * 9
        assert torch.equal(dac.decode(codes), want)
    finally:
        dac.DECODE_LANES_BYTES = old


# ------------------------------------------------------------------ stream_decoder_batch
@pytest.mark.parametrize("chunk", [4, 16])
def test_stream_decoder_batch_equals_decode(dac, chunk):
    """Three lanes of different lengths, pushed raggedly and out of phase: every lane's chunks concatenated are its
    decode(). The lanes meet in windows of equal shape (one launch sequence over them) and of their own."""
    lengths = (75, 40, 58)
    codes = [random_codes(T, seed=300 + T).to(DEV) for T in lengths]
    want = [dac.decode(c) for c in codes]
    dec = dac.stream_decoder_batch(3, chunk)
    win = dec.decode_windows
    for rep in range(2):  # the same object again: no state left over
        sent, got, r = [0] * 3, [[] for _ in range(3)], 0
        while any(sent[lane] < lengths[lane] for lane in range(3)):
            push = {}
            for lane in range(3):
                n = min(RAGGED[(r + 3 * lane) % len(RAGGED)] if rep else chunk, lengths[lane] - sent[lane])
                if sent[lane] < lengths[lane]:
                    push[lane] = codes[lane][0, :, sent[lane]: sent[lane] + n]
                    sent[lane] += n
            done = [lane for lane in push if sent[lane] == lengths[lane]]
            for lane, w in dec.push(push).items():
                got[lane].append(w)
            for lane, w in dec.flush(done).items():
                got[lane].append(w)
            r += 1
        for lane in range(3):
            wav = torch.cat(got[lane], dim=-1)
            assert wav.shape == want[lane].shape and wav.device == want[lane].device
            assert torch.equal(wav, want[lane]), (chunk, rep, lane, float((wav - want[lane]).abs().max()))
    # windows of several lanes did share launch sequences (whole-chunk pushes put the lanes in one shape together),
    # and windows of a shape of their own went the single-lane way
    assert win.lane_launches > 0 and win.lanes_decoded > 2 * win.lane_launches - 1
    assert win.single.graph_replays > 0


# ------------------------------------------------------------------ Zonos.stream_batch
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


MNT = (5, 40, 24, 33, 12)


def _requests():
    conds = [_cond(30 + i, 9 + i) for i in range(len(MNT))]
    prefixes = [None] * len(MNT)
    prefixes[2] = random_codes(12, seed=5).to(DEV)
    return conds, prefixes


def _run(model, conds, prefixes, mnt, **kw):
    """(generate_batch's codes, their decodes, stream_batch's items) with the same seeds."""
    codes = model.generate_batch(conds, prefixes, max_new_tokens=mnt, **kw)
    want = [model.autoencoder.decode(c) for c in codes]
    items = list(model.stream_batch(conds, prefixes, max_new_tokens=mnt, chunk_frames=4, **kw))
    return codes, want, items


def _check(want, items):
    n = len(want)
    assert all(w.dim() == 3 and w.shape[:2] == (1, 1) and w.shape[-1] % 512 == 0 and w.dtype == torch.float32
               for _, w, _ in items)
    assert all(w.shape[-1] > 0 or last for _, w, last in items)
    for i in range(n):
        mine = [(w, last) for j, w, last in items if j == i]
        assert [last for _, last in mine].count(True) == 1 and mine[-1][1], i  # one last item, and it is the last
        got = torch.cat([w for w, _ in mine], dim=-1)
        assert got.shape == want[i].shape, (i, got.shape, want[i].shape)
        assert torch.equal(got, want[i]), (i, float((got - want[i]).abs().max()))
    assert sorted({j for j, _, _ in items}) == list(range(n))


@pytest.mark.parametrize("params", [dict(temperature=0.0), dict(min_p=0.1)], ids=["greedy", "min_p"])
@pytest.mark.parametrize("max_slots", [2, 3])
def test_stream_batch_equals_generate_batch_then_decode(model_no_eos, params, max_slots):
    conds, prefixes = _requests()
    codes, want, items = _run(model_no_eos, conds, prefixes, list(MNT), sampling_params=params,
                              seeds=[50 + i for i in range(len(MNT))], max_slots=max_slots)
    assert [c.shape[-1] for c in codes] == [m + (12 if i == 2 else 0) for i, m in enumerate(MNT)]
    assert torch.equal(codes[2][..., :12], prefixes[2])
    _check(want, items)
    # audio of several utterances is interleaved: an utterance's chunks arrive before an earlier-started one's last
    assert len(items) > len(MNT)
    first_last = next(k for k, (_, _, last) in enumerate(items) if last)
    assert len({j for j, _, _ in items[:first_last + 1]}) > 1


def test_stream_batch_ended_by_eos(model_eos):
    conds, prefixes = _requests()
    conds[1] = _cond(23, 10)  # the request test_gpu_stream ends by EOS within 20 of its 40 frames on this model
    codes, want, items = _run(model_eos, conds, prefixes, list(MNT), sampling_params=dict(temperature=0.0),
                              seeds=[1, 2, 3, 4, 5], max_slots=3)
    new = [c.shape[-1] - (12 if i == 2 else 0) for i, c in enumerate(codes)]
    assert any(0 < n <= m // 2 for n, m in zip(new, MNT)), new  # ended by EOS well before its limit
    _check(want, items)


def test_stream_batch_hybrid():
    model = _build(tiny_hybrid(), zero_eos=True)
    conds, prefixes = _requests()
    codes, want, items = _run(model, conds[:3], None, [30, 11, 22], sampling_params=dict(min_p=0.1),
                              seeds=[7, 8, 9], max_slots=2)
    assert [c.shape[-1] for c in codes] == [30, 11, 22]
    _check(want, items)


def test_stream_batch_closed_early_leaves_the_model_as_new(model_no_eos):
    conds, prefixes = _requests()
    kw = dict(sampling_params=dict(min_p=0.1), seeds=[50 + i for i in range(len(MNT))], max_slots=3)
    gen = model_no_eos.stream_batch(conds, prefixes, max_new_tokens=list(MNT), chunk_frames=4, **kw)
    i, first, last = next(gen)
    assert first.shape[-1] > 0 or last
    gen.close()
    torch.manual_seed(9)
    after = model_no_eos.generate(conds[0], max_new_tokens=24, progress_bar=False)
    fresh = _build(tiny_transformer(), zero_eos=True)
    torch.manual_seed(9)
    assert torch.equal(after, fresh.generate(conds[0], max_new_tokens=24, progress_bar=False))
    # and a stream_batch after the closed one is whole again
    _, want, items = _run(model_no_eos, conds, prefixes, list(MNT), **kw)
    _check(want, items)
