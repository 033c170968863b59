"""Zonos.serve() on the GPU: every ticket's chunks concatenated are bit for bit decode(generate_batch()) of the request
alone, whenever it was admitted, whichever slot it got, whatever ran beside it and whatever parameters its neighbours
had; cancellation, capacity errors, the guard on the model's other entry points, close(), and the PCM16 egress."""
import pytest
import torch

from tests.stream_cases import random_codes
from tests.test_gpu_pcm16 import reference as pcm_reference
from tests.test_gpu_stream_batch import MNT, _build, _cond, _requests
from zonos_vibes_amd.config import tiny_hybrid, tiny_transformer

pytestmark = pytest.mark.gpu
DEV = "cuda"
SERVE = dict(max_seqlen=128, max_prefill=64, chunk_frames=4)
# per request: (sampling_params, cfg_scale, seed): greedy, min_p and top_k side by side, two CFG scales
PARAMS = [(dict(temperature=0.0), 2.0, 50), (dict(min_p=0.1), 3.0, 51), (dict(top_k=50), 2.0, 52),
          (dict(temperature=0.0), 3.0, 53), (dict(min_p=0.1), 2.0, 54)]


class Req:
    def __init__(self, cond, prefix, mnt, sp, cfg, seed):
        self.cond, self.prefix, self.mnt, self.sp, self.cfg, self.seed = cond, prefix, mnt, sp, cfg, seed
        self.want = None

    def submit(self, session):
        return session.submit(self.cond, self.prefix, max_new_tokens=self.mnt, cfg_scale=self.cfg,
                              sampling_params=self.sp, seed=self.seed)


def alone(model, r: Req) -> Req:
    """The request's expected waveform: generated alone in one slot, decoded offline."""
    codes = model.generate_batch([r.cond], [r.prefix], max_new_tokens=[r.mnt], cfg_scale=r.cfg, sampling_params=r.sp,
                                 seeds=[r.seed], max_slots=1)[0]
    r.codes, r.want = codes, model.autoencoder.decode(codes)
    return r


def five(model) -> list:
    conds, prefixes = _requests()
    return [alone(model, Req(conds[i], prefixes[i], MNT[i], *PARAMS[i])) for i in range(len(MNT))]


def drain(session, items):
    while not session.idle:
        items += session.run_round()
    return items


def check(reqs: dict, items, pcm16=False):
    """reqs {ticket: Req}: per ticket one `last`, as its final item, and the chunks concatenated are its waveform."""
    assert {t for t, _, _ in items} == set(reqs)
    for t, w, last in items:
        assert w.dim() == 3 and w.shape[:2] == (1, 1) and w.shape[-1] % 512 == 0 and (w.shape[-1] > 0 or last)
        assert (w.dtype, w.device.type) == ((torch.int16, "cpu") if pcm16 else (torch.float32, "cuda"))
    for t, r in reqs.items():
        mine = [(w, last) for tk, w, last in items if tk == t]
        assert [last for _, last in mine].count(True) == 1 and mine[-1][1], t
        got = torch.cat([w for w, _ in mine], dim=-1)
        want = pcm_reference(r.want.cpu()) if pcm16 else r.want
        assert got.shape == want.shape, (t, got.shape, want.shape)
        assert torch.equal(got, want), (t, int((got != want).sum()))


@pytest.fixture(scope="module")
def model_no_eos():
    return _build(tiny_transformer(), zero_eos=True)


@pytest.fixture(scope="module")
def model_eos():
    return _build(tiny_transformer(), eos_row_scale=6.0)


@pytest.fixture(scope="module")
def requests_no_eos(model_no_eos):
    return five(model_no_eos)


def interleaved(items):
    """Audio of several tickets is interleaved: some ticket's items come in two runs with another ticket's between
    them (A .. B .. A), and the late-admitted ticket 2 speaks before ticket 1, admitted in round 1, has ended.
    (Not "two tickets before the first `last`": on this schedule the first `last` is request 0's only item, its 5
    frames being fewer than the decoder's lookahead of 10, and it comes in round 4, when request 1 has 8 final frames
    and so no audio yet.)"""
    runs = [t for k, (t, _, _) in enumerate(items) if k == 0 or items[k - 1][0] != t]
    assert len(runs) > len(set(runs)), runs
    last1 = next(k for k, (t, _, last) in enumerate(items) if t == 1 and last)
    first2 = next(k for k, (t, _, _) in enumerate(items) if t == 2)
    first1 = next(k for k, (t, _, _) in enumerate(items) if t == 1)
    assert first1 < first2 < last1 or first2 < first1 < last1, (first1, first2, last1)


def staggered(session, reqs):
    """Requests 0, 1 before round 1, request 2 after round 2, requests 3, 4 after round 5."""
    items, tickets = [], {}
    for i in (0, 1):
        tickets[reqs[i].submit(session)] = reqs[i]
    for rnd in range(1, 6):
        items += session.run_round()
        if rnd == 2:
            tickets[reqs[2].submit(session)] = reqs[2]
    for i in (3, 4):
        tickets[reqs[i].submit(session)] = reqs[i]
    drain(session, items)
    assert list(tickets) == [0, 1, 2, 3, 4]
    return tickets, items


@pytest.mark.parametrize("max_slots", [2, 3])
def test_staggered_admission_with_mixed_parameters(model_no_eos, requests_no_eos, max_slots):
    reqs = requests_no_eos
    assert [r.codes.shape[-1] for r in reqs] == [m + (12 if i == 2 else 0) for i, m in enumerate(MNT)]
    assert not torch.equal(reqs[0].want[..., :2048], reqs[3].want[..., :2048])
    with model_no_eos.serve(max_slots, **SERVE) as session:
        tickets, items = staggered(session, reqs)
        assert session.run_round() == [] and session.idle
    check(tickets, items)
    interleaved(items)


def test_all_greedy_rounds_take_the_greedy_launch(model_no_eos, requests_no_eos):
    """Two greedy requests alone in the session: the decode graphs captured are keyed greedy (engine.capture's key);
    a stochastic neighbour switches the round to zmi_sample_step. Both are exact."""
    e = model_no_eos.engine
    reqs = [requests_no_eos[0], requests_no_eos[3], requests_no_eos[1]]
    with model_no_eos.serve(2, **SERVE) as session:
        tickets = {reqs[0].submit(session): reqs[0], reqs[1].submit(session): reqs[1]}
        items = session.run_round()
        assert e.greedy_sampler and all(e.slot_greedy[:2]) and e._greedy_step(0, 2)
        assert any(rows == 4 and greedy for rows, _, greedy, _ in e._graphs)  # the 2-slot graph of the greedy launch
        tickets[reqs[2].submit(session)] = reqs[2]
        drain(session, items)
        assert not e._greedy_step(0, 2)  # the stochastic request took a slot
    check(tickets, items)


def test_idle_then_resume(model_no_eos, requests_no_eos):
    reqs = requests_no_eos
    with model_no_eos.serve(2, **SERVE) as session:
        assert session.idle and session.run_round() == []
        tickets = {reqs[i].submit(session): reqs[i] for i in (4, 0)}
        items = drain(session, [])
        assert session.idle and session.run_round() == []
        tickets[reqs[2].submit(session)] = reqs[2]  # slot 0 and lane 0 again, after idle
        assert not session.idle
        drain(session, items)
    check(tickets, items)


def test_ended_by_eos_hands_the_slot_on(model_eos):
    conds, _ = _requests()
    early = alone(model_eos, Req(_cond(23, 10), None, 40, dict(temperature=0.0), 2.0, 2))
    assert 0 < early.codes.shape[-1] <= 20  # ended by EOS well before its 40 frames
    long = alone(model_eos, Req(conds[3], None, 33, dict(min_p=0.1), 2.0, 4))
    waiting = alone(model_eos, Req(conds[4], None, 12, dict(min_p=0.1), 3.0, 5))
    with model_eos.serve(2, **SERVE) as session:
        tickets = {r.submit(session): r for r in (early, long, waiting)}
        items = drain(session, [])
    check(tickets, items)
    first_last = next(k for k, (_, _, last) in enumerate(items) if last)
    assert all(t != 2 for t, _, _ in items[:first_last + 1])  # ticket 2 waited for a slot to free


def test_cancel_running_and_waiting(model_no_eos, requests_no_eos):
    reqs = requests_no_eos
    with model_no_eos.serve(2, **SERVE) as session:
        tickets = {reqs[i].submit(session): reqs[i] for i in (1, 3, 2)}  # ticket 0 = 40 frames, 1 = 33, 2 = 24 + prefix
        t_wait = reqs[4].submit(session)
        items = []
        while not any(t == 0 for t, _, _ in items):
            items += session.run_round()
        n_before = len(items)
        assert session.cancel(0) is True and session.cancel(t_wait) is True
        assert session.cancel(0) is False and session.cancel(t_wait) is False and session.cancel(99) is False
        items += session.run_round()
        assert [(s, r.ticket) for s, r in session.sched.busy()] == [(0, 2), (1, 1)]  # ticket 2 took ticket 0's slot
        drain(session, items)
        assert session.cancel(1) is False  # finished
    assert all(t != 0 for t, _, _ in items[n_before:])  # no further item of the cancelled running ticket
    assert all(t != t_wait for t, _, _ in items)        # the cancelled waiting ticket never ran
    del tickets[0]
    check(tickets, [it for it in items if it[0] != 0])


def test_capacity_errors_and_the_guard(model_no_eos, requests_no_eos):
    reqs = requests_no_eos
    cond = reqs[0].cond
    with model_no_eos.serve(2, **SERVE) as session:
        tickets = {reqs[1].submit(session): reqs[1]}
        items = session.run_round()
        with pytest.raises(ValueError):
            session.submit(cond, max_new_tokens=128)                    # Lc + n + 9 > max_seqlen
        with pytest.raises(ValueError):
            session.submit(_cond(1, 64), max_new_tokens=4)              # Lc + 1 > max_prefill
        with pytest.raises(ValueError):
            session.submit(cond[:1], max_new_tokens=4)                  # wrong shape
        with pytest.raises(ValueError):
            session.submit(cond, random_codes(60, seed=1).to(DEV), max_new_tokens=4)  # Lc + P + 1 > max_prefill
        with pytest.raises(AssertionError):
            session.submit(cond, max_new_tokens=4, cfg_scale=1)
        with pytest.raises(RuntimeError):
            model_no_eos.generate(cond, max_new_tokens=4, progress_bar=False)
        with pytest.raises(RuntimeError):
            model_no_eos.generate_batch([cond], max_new_tokens=4)
        with pytest.raises(RuntimeError):
            next(model_no_eos.stream_batch([cond], max_new_tokens=4))
        with pytest.raises(RuntimeError):
            next(model_no_eos.stream(cond, max_new_tokens=4))
        with pytest.raises(RuntimeError):
            model_no_eos.serve(2, **SERVE)
        tickets[reqs[4].submit(session)] = reqs[4]  # ticket 1: the refused submits used none up
        drain(session, items)
    check(tickets, items)


def test_close_leaves_the_model_as_new(model_no_eos, requests_no_eos):
    reqs = requests_no_eos
    session = model_no_eos.serve(3, **SERVE)
    for r in reqs:
        r.submit(session)
    for _ in range(4):
        session.run_round()
    assert not session.idle
    session.close()
    session.close()  # idempotent
    with pytest.raises(RuntimeError):
        session.run_round()
    with pytest.raises(RuntimeError):
        reqs[0].submit(session)
    torch.manual_seed(9)
    after = model_no_eos.generate(reqs[0].cond, max_new_tokens=24, progress_bar=False)
    fresh = _build(tiny_transformer(), zero_eos=True)
    torch.manual_seed(9)
    assert torch.equal(after, fresh.generate(reqs[0].cond, max_new_tokens=24, progress_bar=False))
    # and a session after the closed one is whole again
    with model_no_eos.serve(3, **SERVE) as session:
        tickets = {r.submit(session): r for r in reqs}
        items = drain(session, [])
    check(tickets, items)


@pytest.mark.parametrize("max_slots", [2, 3])
def test_pcm16(model_no_eos, requests_no_eos, max_slots):
    with model_no_eos.serve(max_slots, pcm16=True, **SERVE) as session:
        tickets, items = staggered(session, requests_no_eos)
    check(tickets, items, pcm16=True)
    stage = session.egress.pcm_host  # the chunks own their memory: none is a view of the staging buffer
    assert all(w.untyped_storage().data_ptr() != stage.untyped_storage().data_ptr() for _, w, _ in items)


def test_hybrid():
    model = _build(tiny_hybrid(), zero_eos=True)
    conds, _ = _requests()
    reqs = [alone(model, Req(conds[i], None, m, dict(min_p=0.1), 2.0, 7 + i)) for i, m in enumerate((30, 11, 22))]
    with model.serve(2, **SERVE) as session:
        tickets = {reqs[i].submit(session): reqs[i] for i in (0, 1)}
        items = session.run_round() + session.run_round()
        tickets[reqs[2].submit(session)] = reqs[2]  # admitted late, into the slot the 11-frame request frees
        drain(session, items)
    check(tickets, items)
