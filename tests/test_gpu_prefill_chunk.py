"""Chunked prefill (prefill_chunk = C): a prompt of s_len rows goes through the layers as chunks [k C, (k + 1) C).

Transformer: bit for bit the unchunked engine (every per-row kernel is tile- and batch-invariant, and a later chunk's
attention reads the KV rows the earlier ones wrote): codes, prefill logits and the KV rows of the prompt.
Hybrid: the Mamba2 state is rounded to bf16 at a chunk boundary, so the result is held to the CPU oracle under the
criterion of tests/test_gpu_hybrid.py (logits within 24 bf16 ulps of the step's largest, no decision flipped whose
margin exceeds twice that), next to the unchunked engine's error against the same oracle; generate_batch == generate
under the same C and prompts of at most C rows == prefill_chunk None are exact.
serve(prefill_chunk=32): a prompt longer than max_prefill is admitted and runs one chunk in front of each round, the
running ticket speaks in every one of those rounds, every ticket's audio is decode(generate_batch(prefill_chunk=32)) of
it alone, and a ticket cancelled mid-prompt frees its slot without an item.

Measured on an MI355X: test_hybrid_chunked_against_the_oracle's docstring.
"""
import math

import pytest
import torch

from oracle.hybrid_cpu import OracleHybrid
from tests.helpers import synthetic_weights
from tests.stream_cases import random_codes
from tests.test_gpu_hybrid import _bf, _ulp
from tests.test_gpu_stream_batch import _cond
from zonos_vibes_amd.config import tiny_hybrid, tiny_transformer

pytestmark = pytest.mark.gpu
DEV = "cuda"
LC, P, MNT = 20, 150, 24
S_LEN = LC + P + 1  # 171


def _synth(cfg, **kw):
    from zonos_vibes_amd.model import Zonos
    return Zonos.synthetic(cfg, DEV, zero_eos=True, **kw)


# ---------------------------------------------------------------------------------------------- transformer: exact
def _gen(m, cond, prefix, chunk, sp, cfg_scale=2.0, seed=1234):
    torch.manual_seed(seed)
    codes = m.generate(cond, prefix, max_new_tokens=MNT, cfg_scale=cfg_scale, sampling_params=sp, progress_bar=False,
                       prefill_chunk=chunk)
    e = m.engine
    rps = e.rps
    return (codes.cpu(), e.logits_pre[:rps].clone().cpu(), e.kc[:, :rps, :, :S_LEN].clone().cpu(),
            e.vc[:, :rps, :, :, :S_LEN].clone().cpu())


def _exact_case(model_kw, cfg_scale):
    cfg = tiny_transformer(2)
    cond, prefix = _cond(71, LC), random_codes(P, seed=9).to(DEV)
    ref = _synth(cfg, max_seqlen=256, max_prefill=176, **model_kw)
    m = _synth(cfg, max_seqlen=256, max_prefill=64, **model_kw)
    for sp in (dict(temperature=0.0), dict(min_p=0.1)):
        want = _gen(ref, cond, prefix, None, sp, cfg_scale)
        assert want[0].shape == (1, 9, P + MNT)
        for chunk in (64, 37):
            got = _gen(m, cond, prefix, chunk, sp, cfg_scale)
            assert m.engine.max_prefill == 64  # the long prompt did not rebuild the engine
            for name, a, b in zip(("codes", "logits_pre", "K rows", "V rows"), got, want):
                assert torch.equal(a, b), (name, chunk, sp)
    return m


def test_transformer_chunked_equals_unchunked():
    m = _exact_case({}, 2.0)
    # prefill_chunk None: the engine still refuses a prompt past max_prefill, and a bad chunk is refused
    from zonos_vibes_amd.engine import SamplingParams
    cond, prefix = _cond(71, LC), random_codes(P, seed=9).to(DEV)
    with pytest.raises(ValueError, match="max_prefill"):
        m.engine.prefill(0, cond, prefix, MNT, SamplingParams(temperature=0.0))
    for bad in (0, 65):
        with pytest.raises(ValueError, match="prefill_chunk"):
            m.engine.prefill(0, cond, prefix, MNT, SamplingParams(temperature=0.0), prefill_chunk=bad)


def test_transformer_chunked_equals_unchunked_guidance_free():
    _exact_case({}, 1)


def test_transformer_chunked_equals_unchunked_fp8():
    _exact_case(dict(weights="fp8"), 2.0)


def test_stream_and_stream_batch_take_prefill_chunk():
    """stream(prefill_chunk=C) and stream_batch(prefill_chunk=C) are decode(generate(prefill_chunk=C)), chunk by chunk."""
    cfg = tiny_transformer(2)
    m = _synth(cfg, max_slots=2, max_seqlen=256, max_prefill=64)
    cond, prefix, sp = _cond(71, LC), random_codes(P, seed=9).to(DEV), dict(temperature=0.0)
    want = m.autoencoder.decode(m.generate(cond, prefix, max_new_tokens=MNT, sampling_params=sp, progress_bar=False,
                                           prefill_chunk=37))
    got = torch.cat(list(m.stream(cond, prefix, max_new_tokens=MNT, sampling_params=sp, chunk_frames=8,
                                  prefill_chunk=37)), dim=-1)
    assert got.shape == want.shape and torch.equal(got, want)
    items = list(m.stream_batch([_cond(72, 9), cond], [None, prefix], max_new_tokens=[12, MNT], sampling_params=sp,
                                seeds=[1, 2], chunk_frames=8, prefill_chunk=37))
    got = torch.cat([w for i, w, _ in items if i == 1], dim=-1)
    assert got.shape == want.shape and torch.equal(got, want)
    assert m.engine.max_prefill == 64


# ---------------------------------------------------------------------------------------------- hybrid: the oracle
N_STEPS = 8
BOUND = 24  # bf16 ulps of the step's largest logit: tests/test_gpu_hybrid.py's criterion for this model
_ORACLE = {}


def _oracle(s_len):
    """The CPU oracle's greedy trajectory over a prompt of s_len rows (20 conditioning rows + an audio prefix)."""
    if s_len not in _ORACLE:
        cfg = tiny_hybrid()
        o = OracleHybrid(cfg, synthetic_weights(cfg, seed=0))
        cond = _bf(2, LC, cfg.backbone.d_model, seed=31)
        prefix = random_codes(s_len - LC - 1, seed=s_len)
        raw = []
        o.generate(cond, prefix, max_new_tokens=N_STEPS,
                   sampling_params=dict(temperature=0.0, repetition_penalty=1.0), raw_trace=raw)
        _ORACLE[s_len] = (cond, prefix, raw, o.last_delayed[0])
    return _ORACLE[s_len]


def _against_oracle(s_len, chunk):
    """(per-step error in ulps of the step's largest logit, decisions flipped beyond twice BOUND) of the engine's
    prefill (in chunks of `chunk`; None: one pass) and the teacher-forced steps along the oracle's trajectory (N_STEPS
    new frames and the 8 steps that flush the delay pattern: 16 steps)."""
    from zonos_vibes_amd.engine import SamplingParams
    cond, prefix, raw, dl = _oracle(s_len)
    from zonos_vibes_amd.model import Zonos
    m = Zonos.synthetic(tiny_hybrid(), DEV, seed=0, max_seqlen=s_len + N_STEPS + 32,  # (the oracle's EOS row: not zeroed)
                        max_prefill=s_len if chunk is None else max(chunk, 32))
    e = m.engine
    e.prefill(0, cond.to(DEV), prefix.to(DEV), N_STEPS, SamplingParams(temperature=0.0, repetition_penalty=1.0),
              prefill_chunk=chunk)
    e.stream.synchronize()

    def cfg_logits(rows):
        c, u = rows[0].float().cpu(), rows[1].float().cpu()
        lg = u + (c - u) * 2.0
        lg[..., 1025:] = -torch.inf
        return lg

    got = [cfg_logits(e.logits_pre)]
    for _ in range(len(raw) - 1):
        with torch.cuda.stream(e.stream):
            e.delayed[0, :, : dl.shape[-1]] = dl.to(DEV, torch.int32)
            for k, v in (("active", 1), ("stopping", 0), ("remaining", 1000)):
                e.st[k][0] = v
            e.refresh_inputs()
        e.step(1, use_graph=False, slots=1)
        e.stream.synchronize()
        lg = cfg_logits(e.logits[0:2])
        lg[1:, 1024] = -torch.inf
        got.append(lg)
    e.check_errors()
    errs, flips = [], 0
    for g, r in zip(got, raw):
        r = r[0]
        fin = torch.isfinite(r)
        scale = _ulp(r[fin].abs().max())
        errs.append(((g - r).abs()[fin].max() / scale).item())
        top2 = r[:, :1025].topk(2, dim=-1)
        det = (top2.values[:, 0] - top2.values[:, 1]) / scale > 2 * BOUND
        flips += int((g[:, :1025].argmax(-1) != top2.indices[:, 0])[det].sum())
    return errs, flips


@pytest.mark.parametrize("s_len,chunk", [(100, 32), (300, 256)])
def test_hybrid_chunked_against_the_oracle(s_len, chunk):
    """The chunked engine and the unchunked one against the same oracle trajectory. Measured on an MI355X, max over the
    prefill and 16 steps in bf16 ulps of the step's largest logit (the bound is 24), chunked / unchunked:
        s_len 100, C 32     4.00 / 3.00   (prefill logits 3.00 / 3.00)
        s_len 300, C 256    3.00 / 3.00   (prefill logits 1.50 / 1.50)
    and no flipped decision in any of the four runs."""
    errs, flips = _against_oracle(s_len, chunk)
    errs0, flips0 = _against_oracle(s_len, None)
    print(f"hybrid s_len {s_len}: chunked (C = {chunk}) prefill {errs[0]:.2f} max {max(errs):.2f} ulps, flips {flips}; "
          f"unchunked prefill {errs0[0]:.2f} max {max(errs0):.2f} ulps, flips {flips0}")
    assert max(errs0) <= BOUND and flips0 == 0, ("unchunked", errs0, flips0)
    assert max(errs) <= BOUND and flips == 0, ("chunked", errs, flips)


def test_hybrid_batch_equals_single_and_short_prompts_keep_their_bits():
    cfg = tiny_hybrid()
    m = _synth(cfg, seed=3, max_slots=3, max_seqlen=192, max_prefill=64)
    d = cfg.backbone.d_model
    conds = [_bf(2, lc, d, seed=40 + lc).to(DEV) for lc in (20, 9, 14)]
    prefixes = [random_codes(79, seed=1).to(DEV), None, random_codes(50, seed=2).to(DEV)]  # s_len 100, 10, 65
    n, sp, C = [20, 14, 30], dict(temperature=0.0), 32
    batch = m.generate_batch(conds, prefixes, max_new_tokens=n, sampling_params=sp, seeds=[1, 2, 3], max_slots=3,
                             prefill_chunk=C)
    for c, p, k, b in zip(conds, prefixes, n, batch):
        single = m.generate(c, p, max_new_tokens=k, sampling_params=sp, progress_bar=False, prefill_chunk=C)
        assert torch.equal(single.cpu(), b.cpu())
    assert m.engine.max_prefill == 64
    # a prompt of at most C rows is one chunk from position 0: today's bits
    for c, p, k in ((conds[1], None, 14), (conds[0], random_codes(11, seed=3).to(DEV), 12)):  # s_len 10 and 32
        a = m.generate(c, p, max_new_tokens=k, sampling_params=sp, progress_bar=False, prefill_chunk=C)
        b = m.generate(c, p, max_new_tokens=k, sampling_params=sp, progress_bar=False)
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- serve
SERVE = dict(max_seqlen=256, max_prefill=64, chunk_frames=4, prefill_chunk=32)


class Req:
    def __init__(self, model, cond, prefix, mnt, seed):
        self.cond, self.prefix, self.mnt, self.seed = cond, prefix, mnt, seed
        codes = model.generate_batch([cond], [prefix], max_new_tokens=[mnt], sampling_params=dict(min_p=0.1),
                                     seeds=[seed], max_slots=1, prefill_chunk=32)[0]
        self.want = model.autoencoder.decode(codes)

    def submit(self, session):
        return session.submit(self.cond, self.prefix, max_new_tokens=self.mnt, sampling_params=dict(min_p=0.1),
                              seed=self.seed)


@pytest.fixture(scope="module", params=["transformer", "hybrid"])
def served(request):
    cfg = tiny_transformer(2) if request.param == "transformer" else tiny_hybrid()
    m = _synth(cfg, max_slots=2, max_seqlen=256, max_prefill=64)
    d = cfg.backbone.d_model
    a = Req(m, _cond(81, 10, d), None, 90, 5)
    b = Req(m, _cond(82, LC, d), random_codes(P, seed=7).to(DEV), MNT, 6)
    c = Req(m, _cond(83, 12, d), random_codes(8, seed=8).to(DEV), 16, 7)
    return m, a, b, c


def _audio(items, ticket):
    mine = [(w, last) for t, w, last in items if t == ticket]
    assert [last for _, last in mine].count(True) == 1 and mine[-1][1]
    return torch.cat([w for w, _ in mine], dim=-1)


def test_serve_long_prompt_arrives_mid_stream(served):
    m, a, b, _ = served
    with pytest.raises(ValueError, match="max_prefill"):  # without prefill_chunk the request is refused
        with m.serve(2, max_seqlen=256, max_prefill=64, chunk_frames=4) as plain:
            b.submit(plain)
    rounds = []
    with m.serve(2, **SERVE) as session:
        ta = a.submit(session)
        for _ in range(7):
            rounds.append(session.run_round())
        tb = b.submit(session)
        admitted = len(rounds)  # B is admitted (its first chunk runs) in the next round
        passes0 = session.passes_run
        while not session.idle:
            rounds.append(session.run_round())
            if len(rounds) == admitted + 2:
                assert list(session.mid) == [1] and session.passes_run == passes0 + 2  # one pass a round
        assert m.engine.max_prefill == 64
    items = [it for r in rounds for it in r]
    first_b = next(k for k, r in enumerate(rounds) if any(t == tb for t, _, _ in r))
    between = rounds[admitted: first_b + 1]
    n_chunks = math.ceil(S_LEN / 32)
    assert len(between) >= n_chunks, (admitted, first_b)
    for k, r in enumerate(between):  # A speaks in every round while B's prompt runs chunk by chunk
        assert any(t == ta and w.shape[-1] > 0 for t, w, _ in r), k
    for t, r in ((ta, a), (tb, b)):
        got = _audio(items, t)
        assert got.shape == r.want.shape and torch.equal(got, r.want), t


def test_serve_cancel_mid_prompt_frees_the_slot(served):
    m, a, b, c = served
    items = []
    with m.serve(2, **SERVE) as session:
        ta = a.submit(session)
        for _ in range(3):
            items += session.run_round()
        tb = b.submit(session)
        for _ in range(2):
            items += session.run_round()
        assert list(session.mid) == [1] and session.planner.pending
        assert session.cancel(tb)
        items += session.run_round()
        assert not session.mid and not session.planner.pending
        tc = c.submit(session)  # takes the slot B left with a third of its prompt in the caches
        while not session.idle:
            items += session.run_round()
    assert not any(t == tb for t, _, _ in items)
    for t, r in ((ta, a), (tc, c)):
        got = _audio(items, t)
        assert got.shape == r.want.shape and torch.equal(got, r.want), t
