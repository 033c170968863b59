"""HybridEngine.prefill_many: several slots' ragged sequences in one pass through the layers (the Mamba2 scan over
the pass's sequence table, zmi_mamba2_scan_seqs), bit for bit what prefill() of each slot alone leaves: prefill rows,
K / V, conv rings, SSM states and first frames; then generate_batch() and serve() against generate()."""
import pytest
import torch

from tests.stream_cases import random_codes
from tests.test_gpu_attn_prefill import SENTINEL, _cond, _model
from zonos_vibes_amd.config import tiny_hybrid

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _items(sp):
    return [(0, _cond(20, 9, 512), None, 8, sp), (1, _cond(21, 14, 512), random_codes(21, seed=8).to(DEV), 8, sp),
            (2, _cond(22, 5, 512), None, 8, sp)]


LENS, OFFS = [10, 36, 6], [0, 20, 92]
NAMES = ("x_pre", "hid_pre", "K", "V", "conv ring", "ssm state", "delayed")


def _wipe(e):
    with torch.cuda.stream(e.stream):
        for t in (e.kc, e.vc, e.x_pre, e.hid_pre):
            t.zero_()
        e.conv_ring.fill_(5.0)  # stale state of an earlier utterance must go
        e.ssm.fill_(-2.0)
        for t in (e.attn_pre, e.yb_pre):
            t.fill_(SENTINEL)
        e.scan_ws.fill_(0xA5)


def _state(e, slot, off, s_len):
    e.stream.synchronize()
    e.check_errors()
    r = slice(2 * slot, 2 * slot + 2)
    return (e.x_pre[off: off + 2 * s_len].clone(), e.hid_pre[off: off + 2 * s_len].clone(), e.kc[:, r].clone(),
            e.vc[:, r].clone(), e.conv_ring[:, r].clone(), e.ssm[:, r].clone(), e.delayed[slot].clone())


def _count_passes(e):
    """Wrap e._prefill_layers on the instance -> the list its calls' (m, sequences) are appended to."""
    calls, inner = [], e._prefill_layers

    def counted(m, max_pos, seqs):
        seqs = list(seqs)
        calls.append((m, seqs))
        return inner(m, max_pos, seqs)
    e._prefill_layers = counted
    return calls


@pytest.fixture(scope="module")
def engine():
    return _model(tiny_hybrid(), max_slots=3, max_seqlen=96, max_prefill=64).engine


@pytest.fixture(scope="module")
def alone(engine):
    """Each of the three slots prefilled alone, under either attention: {mode: [state per slot]}."""
    from zonos_vibes_amd.engine import SamplingParams
    e = engine
    items = _items(SamplingParams(temperature=0.0))
    out = {}
    for mode in ("tiles", "rows"):
        e.prefill_attn = mode
        out[mode] = []
        for it, n in zip(items, LENS):
            _wipe(e)
            assert e.prefill(*it) == n
            out[mode].append(_state(e, it[0], 0, n))
            e.release(it[0])
    e.prefill_attn = "tiles"
    assert not torch.equal(out["tiles"][0][5], out["tiles"][2][5]) and out["tiles"][1][4].any()
    return out


@pytest.mark.parametrize("mode", ["tiles", "rows"])
def test_prefill_many_equals_slots_alone(engine, alone, mode):
    """3 slots of different lengths in one pass, one with an audio prefix."""
    from zonos_vibes_amd.engine import SamplingParams
    e = engine
    items = _items(SamplingParams(temperature=0.0))
    e.prefill_attn = mode
    try:
        _wipe(e)
        assert e.prefill_many(items) == LENS
        for it, off, n, want in zip(items, OFFS, LENS, alone[mode]):
            for name, a, b in zip(NAMES, _state(e, it[0], off, n), want):
                assert torch.equal(a, b), (mode, it[0], name)
    finally:
        e.prefill_attn = "tiles"
        for s in range(3):
            e.release(s)


def test_prefill_many_is_one_pass(engine):
    from zonos_vibes_amd.engine import SamplingParams
    e = engine
    assert type(e).prefill_batch is True
    calls = _count_passes(e)
    try:
        assert e.prefill_many(_items(SamplingParams(temperature=0.0))) == LENS
        e.stream.synchronize()
        e.check_errors()
    finally:
        del e._prefill_layers
        for s in range(3):
            e.release(s)
    assert len(calls) == 1
    m, seqs = calls[0]
    assert m == 2 * sum(LENS) and len(seqs) == 6
    assert [tuple(s) for s in seqs] == [(0, 10, 0, 0), (10, 10, 1, 0), (20, 36, 2, 0), (56, 36, 3, 0), (92, 6, 4, 0),
                                        (98, 6, 5, 0)]


def test_pass_boundary(engine, alone):
    """pre_rows too small for the third slot: two passes (the third slot's rows start at row 0 again), the same bits."""
    from zonos_vibes_amd.engine import SamplingParams
    e = engine
    items = _items(SamplingParams(temperature=0.0))
    calls = _count_passes(e)
    old = e.pre_rows
    e.pre_rows = 100  # 20 + 72 rows fit, 12 more do not
    try:
        _wipe(e)
        assert e.prefill_many(items) == LENS
        e.stream.synchronize()
        assert [(m, len(s)) for m, s in calls] == [(92, 4), (12, 2)]
        # the second pass reuses rows 0 .. 11, so only its own rows can be read back; caches and frames of all three
        for it, off, n, want, rows in zip(items, [0, 20, 0], LENS, alone["tiles"], [False, True, True]):
            got = _state(e, it[0], off, n)
            for k, (name, a, b) in enumerate(zip(NAMES, got, want)):
                if k >= 2 or rows:
                    assert torch.equal(a, b), (it[0], name)
    finally:
        e.pre_rows = old
        del e._prefill_layers
        for s in range(3):
            e.release(s)


def test_mixed_scan_forms_in_one_pass():
    """A 270-row sequence (past the SSD form's 256 positions: the 4-workgroup scan) beside a 10-row one (SSD)."""
    from zonos_vibes_amd.engine import SamplingParams
    e = _model(tiny_hybrid(), max_slots=2, max_seqlen=320, max_prefill=300).engine
    sp = SamplingParams(temperature=0.0)
    items = [(0, _cond(40, 9, 512), random_codes(260, seed=9).to(DEV), 8, sp), (1, _cond(41, 9, 512), None, 8, sp)]
    lens, offs = [270, 10], [0, 540]
    want = []
    for it, n in zip(items, lens):
        _wipe(e)
        assert e.prefill(*it) == n
        want.append(_state(e, it[0], 0, n))
        e.release(it[0])
    calls = _count_passes(e)
    _wipe(e)
    assert e.prefill_many(items) == lens
    assert [(m, len(s)) for m, s in calls] == [(560, 4)]
    for it, off, n, w in zip(items, offs, lens, want):
        for name, a, b in zip(NAMES, _state(e, it[0], off, n), w):
            assert torch.equal(a, b), (it[0], name)


# ------------------------------------------------------------------ API level
MNT = (30, 11, 22, 17)
SP = dict(min_p=0.1)


@pytest.fixture(scope="module")
def api():
    """(model, conds, seeds, generate()'s codes per utterance); generate() draws its seed from torch's generator."""
    from tests.test_gpu_stream_batch import _build, _requests
    from zonos_vibes_amd.model import _draw_seed
    model = _build(tiny_hybrid(), zero_eos=True)
    conds = _requests()[0][:4]
    seeds, want = [], []
    for i, (c, m) in enumerate(zip(conds, MNT)):
        torch.manual_seed(900 + i)
        seeds.append(_draw_seed())
        torch.manual_seed(900 + i)
        want.append(model.generate(c, max_new_tokens=m, sampling_params=SP, progress_bar=False))
    assert [w.shape[-1] for w in want] == list(MNT)
    return model, conds, seeds, want


def test_generate_batch_equals_generate(api):
    """Four utterances over two slots: the first fill and the refills go through prefill_many."""
    model, conds, seeds, want = api
    got = model.generate_batch(conds, None, max_new_tokens=list(MNT), sampling_params=SP, seeds=seeds, max_slots=2)
    assert type(model.engine).prefill_batch is True and model.engine.S == 2
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), i


def test_serve_equals_generate(api):
    """Three requests up front over three slots (one prefill_many pass), one more after the first round."""
    from tests.test_gpu_serve import SERVE, Req, check, drain
    model, conds, seeds, want = api
    reqs = []
    for c, m, s, w in zip(conds, MNT, seeds, want):
        r = Req(c, None, m, SP, 2.0, s)
        r.want = model.autoencoder.decode(w)
        reqs.append(r)
    with model.serve(3, **SERVE) as session:
        tickets = {reqs[i].submit(session): reqs[i] for i in (0, 1, 2)}
        items = session.run_round()
        tickets[reqs[3].submit(session)] = reqs[3]
        drain(session, items)
    check(tickets, items)
