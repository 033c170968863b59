"""sample_rate= on Zonos.stream(), stream_batch() and serve(): the chunks of an utterance concatenated are bit for bit
autoencoder.resample(decode(codes), 44100, rate) (with pcm16, the reference conversion of that), whichever slot it ran
in and whatever ran beside it; None and 44100 are the unchanged default path."""
import pytest
import torch

from tests.test_gpu_pcm16 import reference as pcm_reference
from tests.test_gpu_serve import PARAMS, SERVE, Req, alone, drain
from tests.test_gpu_stream_batch import MNT, _build, _cond, _requests
from zonos_vibes_amd.config import tiny_transformer

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def model():
    return _build(tiny_transformer(), zero_eos=True)


def test_stream_at_24k(model):
    ae = model.autoencoder
    cond = _cond(11, 12)
    kw = dict(max_new_tokens=40, sampling_params=dict(min_p=0.1))
    torch.manual_seed(140)
    codes = model.generate(cond, progress_bar=False, **kw)
    want = ae.resample(ae.decode(codes), 44100, 24000)
    assert want.shape == (1, 1, -(-24000 * 512 * 40 // 44100))
    torch.manual_seed(140)
    chunks = list(model.stream(cond, chunk_frames=4, sample_rate=24000, **kw))
    assert len(chunks) > 1
    assert all(c.shape[:2] == (1, 1) and c.shape[-1] > 0 and c.dtype == torch.float32 for c in chunks)
    assert any(c.shape[-1] % 512 for c in chunks)
    got = torch.cat(chunks, dim=-1)
    assert got.shape == want.shape and torch.equal(got, want)


def test_stream_ended_by_eos_and_after_an_early_close(model):
    """An utterance that ends by EOS inside a round (the DAC decoder is rolled back; the resampler is fed only what
    counts), right after a stream at the same rate was closed before its end (its lane's carry is dropped)."""
    ae = model.autoencoder
    eos = _build(tiny_transformer(), eos_row_scale=6.0)
    cond = _cond(23, 10)  # ends by EOS within 20 of its 40 frames on this model (test_gpu_stream.py)
    kw = dict(max_new_tokens=40, sampling_params=dict(temperature=0.0))
    torch.manual_seed(1)
    codes = eos.generate(cond, progress_bar=False, **kw)
    assert 0 < codes.shape[-1] <= 20
    want = eos.autoencoder.resample(eos.autoencoder.decode(codes), 44100, 8000)
    gen = model.stream(_cond(11, 12), chunk_frames=4, sample_rate=8000, max_new_tokens=40,
                       sampling_params=dict(min_p=0.1))
    assert next(gen).shape[-1] > 0
    gen.close()
    for m in (eos, model):
        torch.manual_seed(1)
        got = torch.cat(list(m.stream(cond, chunk_frames=4, sample_rate=8000, **kw)), dim=-1)
        if m is model:  # no EOS on this model: the full 40 frames
            torch.manual_seed(1)
            want = ae.resample(ae.decode(model.generate(cond, progress_bar=False, **kw)), 44100, 8000)
        assert got.shape == want.shape and torch.equal(got, want)


def test_stream_batch_at_16k_reuses_a_slot(model):
    ae = model.autoencoder
    conds, prefixes = _requests()
    conds, prefixes, mnt = conds[1:4], prefixes[1:4], [40, 24, 33]   # three utterances over two slots
    kw = dict(sampling_params=dict(min_p=0.1), seeds=[61, 62, 63], max_slots=2)
    codes = model.generate_batch(conds, prefixes, max_new_tokens=mnt, **kw)
    want = [ae.resample(ae.decode(c), 44100, 16000) for c in codes]
    items = list(model.stream_batch(conds, prefixes, max_new_tokens=mnt, chunk_frames=4, sample_rate=16000, **kw))
    assert sorted({i for i, _, _ in items}) == [0, 1, 2]
    for i in range(3):
        mine = [(w, last) for j, w, last in items if j == i]
        assert [last for _, last in mine].count(True) == 1 and mine[-1][1], i
        assert all(w.shape[:2] == (1, 1) and w.dtype == torch.float32 and w.is_cuda for w, _ in mine)
        got = torch.cat([w for w, _ in mine], dim=-1)
        assert got.shape == want[i].shape, (i, got.shape, want[i].shape)
        assert torch.equal(got, want[i]), (i, float((got - want[i]).abs().max()))


def test_serve_pcm16_at_48k_with_a_late_and_a_cancelled_ticket(model):
    ae = model.autoencoder
    conds, prefixes = _requests()
    reqs = [alone(model, Req(conds[i], prefixes[i], MNT[i], *PARAMS[i])) for i in (1, 3, 2)]
    with model.serve(max_slots=2, pcm16=True, sample_rate=48000, **SERVE) as session:
        tickets = {reqs[0].submit(session): reqs[0], reqs[1].submit(session): reqs[1]}
        items = []
        while not any(t == 0 for t, _, _ in items):
            items += session.run_round()
        tickets[reqs[2].submit(session)] = reqs[2]      # submitted mid-session: it waits for a slot
        n_before = len(items)
        assert session.cancel(0) is True                # ticket 0 is running
        drain(session, items)
    assert list(tickets) == [0, 1, 2]
    assert all(t != 0 for t, _, _ in items[n_before:])  # no further item of the cancelled ticket
    for t in (1, 2):
        mine = [(w, last) for tk, w, last in items if tk == t]
        assert [last for _, last in mine].count(True) == 1 and mine[-1][1], t
        assert all(w.dtype == torch.int16 and w.device.type == "cpu" and w.shape[:2] == (1, 1) for w, _ in mine)
        got = torch.cat([w for w, _ in mine], dim=-1)
        want = pcm_reference(ae.resample(tickets[t].want, 44100, 48000).cpu())
        assert got.shape == want.shape, (t, got.shape, want.shape)
        assert torch.equal(got, want), (t, int((got != want).sum()))


def test_default_path_is_unchanged(model):
    """None and 44100: the chunks, and their shapes, of the call without the keyword; no resampler is made."""
    cond = _cond(11, 12)
    kw = dict(max_new_tokens=24, sampling_params=dict(min_p=0.1), chunk_frames=4)
    runs = []
    model._stream_resamplers.clear()
    for extra in (dict(), dict(sample_rate=None), dict(sample_rate=44100)):
        torch.manual_seed(77)
        runs.append(list(model.stream(cond, **kw, **extra)))
    for other in runs[1:]:
        assert [c.shape for c in other] == [c.shape for c in runs[0]]
        assert all(torch.equal(a, b) for a, b in zip(other, runs[0]))
    conds, prefixes = _requests()
    bkw = dict(max_new_tokens=[12, 20], sampling_params=dict(min_p=0.1), seeds=[5, 6], max_slots=2, chunk_frames=4)
    runs = [list(model.stream_batch(conds[:2], None, **bkw, **extra))
            for extra in (dict(), dict(sample_rate=None), dict(sample_rate=44100))]
    for other in runs[1:]:
        assert [(i, w.shape, last) for i, w, last in other] == [(i, w.shape, last) for i, w, last in runs[0]]
        assert all(torch.equal(a[1], b[1]) for a, b in zip(other, runs[0]))
    r = alone(model, Req(conds[0], None, 12, *PARAMS[0]))
    served = []
    for extra in (dict(), dict(sample_rate=44100)):
        with model.serve(max_slots=2, pcm16=True, **SERVE, **extra) as session:
            assert session.rs is None
            r.submit(session)
            served.append(drain(session, []))
    assert [(t, w.shape, last) for t, w, last in served[0]] == [(t, w.shape, last) for t, w, last in served[1]]
    assert all(torch.equal(a[1], b[1]) for a, b in zip(*served))
    assert model._stream_resamplers == {}
    for bad in (0, -8000, 16000.0):
        with pytest.raises(ValueError):
            next(iter(model.stream(cond, sample_rate=bad, **kw)))
        with pytest.raises(ValueError):
            model.serve(max_slots=1, sample_rate=bad, **SERVE)
    assert model._serving is None
