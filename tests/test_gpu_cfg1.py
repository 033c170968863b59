"""Guidance-free generation (cfg_scale = 1: the engine's single layout, one activation / KV row per utterance)
through the engine and the public API.

The main oracle needs no tolerance. Every kernel's per-row arithmetic is independent of the rows beside it (pinned
elsewhere in the suite), so a paired run whose two conditioning rows are identical has u == c bit for bit and
u + (c - u) * cfg == c: generate(cat([c, c]), cfg_scale=2.0) on the paired layout and generate(c, cfg_scale=1) on
the single layout give equal codes and equal per-row logits (single row s against paired row 2s), greedy or
stochastic with the same seed. Then: generate_batch / stream / stream_batch / serve(guidance=False) against
generate(cfg_scale=1) of each utterance alone, layout switching on one model, and the single layout's logits against
the CPU oracle's cfg_scale = 1 branch, teacher-forced."""
import pytest
import torch

from tests.cfg1_cases import cond_single, oracle_run, random_prefix
from tests.helpers import load_golden, synthetic_weights
from zonos_vibes_amd.config import ZonosConfig, hybrid_config, tiny_hybrid, tiny_transformer, transformer_config
from zonos_vibes_amd.engine import SamplingParams

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_NEW = 24
GREEDY, MINP = dict(temperature=0.0), dict(min_p=0.1)


def _synth(cfg, **kw):
    from zonos_vibes_amd.model import Zonos
    return Zonos.synthetic(cfg, DEV, zero_eos=True, **kw)


# name -> (config, constructor keywords, Lc): "wide" gives the real instantiations (d 2048: the fused attention block,
# at one row in the single layout), "hybrid2048" the hybrid's (zmi_mamba_block and the ADDLN attention block)
MODELS = {
    "tiny": (lambda: tiny_transformer(2), dict(max_seqlen=128, max_prefill=64), 11),
    "wide": (lambda: transformer_config(2048, 2, 16, 4, 8192), dict(max_seqlen=64, max_prefill=32), 8),
    "fp8": (lambda: tiny_transformer(2), dict(max_seqlen=128, max_prefill=64, weights="fp8"), 11),
    "hybrid": (lambda: tiny_hybrid(), dict(max_seqlen=96, max_prefill=32), 9),
    "hybrid2048": (lambda: hybrid_config(2048, 3, [1], 16, 4), dict(max_seqlen=96, max_prefill=32), 9),
}
_BUILT: dict = {}


def _model(name):
    if name not in _BUILT:
        cfg, kw, _ = MODELS[name]
        _BUILT[name] = _synth(cfg(), **kw)
    return _BUILT[name]


def _cond(name, seed=1):
    m = _model(name)
    return cond_single(MODELS[name][2], m.config.backbone.d_model, seed).to(DEV)


def _generate(m, cond, prefix, cfg_scale, sp, seed=77, logits=None, n=N_NEW):
    """generate(); with `logits` (a list) through the per-step callback path, appending the slot's logits rows of
    every decode step (after the prefill's)."""
    torch.manual_seed(seed)
    cb = None
    if logits is not None:
        rows = 1 if cfg_scale == 1 else 2

        def cb(frame, step, max_steps):
            logits.append(m.engine.logits[:rows].clone())
            return True
    out = m.generate(cond, prefix, max_new_tokens=n, cfg_scale=cfg_scale, sampling_params=sp, progress_bar=False,
                     callback=cb)
    if logits is not None:
        logits.insert(0, m.engine.logits_pre[:rows].clone())
    return out


# ---------------------------------------------------------------------- the duplicate-conditioning equivalence
@pytest.mark.parametrize("sp", [GREEDY, MINP], ids=["greedy", "min_p"])
@pytest.mark.parametrize("plen", [0, 12], ids=["noprefix", "prefix12"])
@pytest.mark.parametrize("name", list(MODELS))
def test_single_layout_equals_paired_with_duplicate_conditioning(name, plen, sp):
    m, c = _model(name), _cond(name)
    prefix = random_prefix(plen, 5).to(DEV) if plen else None
    lg2, lg1 = [], []
    two = _generate(m, torch.cat([c, c]), prefix, 2.0, sp, logits=lg2)
    assert m.engine.rps == 2
    one = _generate(m, c, prefix, 1, sp, logits=lg1)
    assert m.engine.rps == 1 and m.engine.slots.rows_per_slot == 1
    assert one.shape == (1, 9, plen + N_NEW) and torch.equal(one, two)
    assert len(lg1) == len(lg2) == N_NEW + 9
    for step, (a, b) in enumerate(zip(lg1, lg2)):
        assert torch.equal(b[0], b[1]), ("paired rows of one slot", step)
        assert torch.equal(a[0], b[0]), ("single row 0 against paired row 0", step)
    # the chunked path (runs of hipGraph replays) gives the codes of the per-step callback path, in either layout
    assert torch.equal(_generate(m, c, prefix, 1, sp), one)
    assert torch.equal(_generate(m, torch.cat([c, c]), prefix, 2.0, sp), one)
    # [2, Lc, d] as prepare_conditioning hands it out: row 0 alone is used
    other = _cond(name, seed=9)
    assert torch.equal(_generate(m, torch.cat([c, other]), prefix, 1, sp), one)
    if name == "wide":  # the decode step ran the fused attention block at one row
        e = m.engine
        assert e._rows(1) == 1 and any(kind == "attnblk" for kind, _ in e._plan(1, e._segments(1, 1)[0][1]))


def _engine_run(m, conds, n, sp, rps, use_graph, chunk=7):
    """prefill_many + step() on the engine itself over len(conds) slots -> (codes per slot, last logits rows)."""
    m._ensure_capacity(len(conds), 64, 32)  # (slots; the model's own max_seqlen / max_prefill are larger)
    e = m.engine
    e.set_layout(rps)
    items = [(s, c if rps == 1 else torch.cat([c, c]), None, n, SamplingParams.from_dict(dict(sp), 2.0, 100 + s))
             for s, c in enumerate(conds)]
    e.prefill_many(items)
    left = n + 8
    while left:
        k = min(chunk, left)
        e.step(k, use_graph=use_graph, slots=len(conds))
        left -= k
    e.stream.synchronize()
    e.check_errors()
    rows = e.logits[: rps * len(conds)].clone()
    codes = [e.read_codes(s) for s in range(len(conds))]
    for s in range(len(conds)):
        e.release(s)
    return codes, rows


@pytest.mark.parametrize("name,slots", [("tiny", 1), ("tiny", 3), ("wide", 1), ("wide", 3), ("wide", 5), ("hybrid", 3),
                                        ("hybrid2048", 1), ("hybrid2048", 3), ("hybrid2048", 5)])
@pytest.mark.parametrize("sp", [GREEDY, MINP], ids=["greedy", "min_p"])
def test_engine_rows_single_s_equals_paired_2s_with_and_without_graphs(name, slots, sp):
    """Several slots (odd busy counts: 3 and 5 rows through the fused block on the wide config): single row s against
    paired row 2s, and the same run enqueued launch by launch (use_graph=False) against the hipGraph replays."""
    m = _model(name)
    conds = [_cond(name, seed=20 + s) for s in range(slots)]
    codes2, rows2 = _engine_run(m, conds, 12, sp, 2, True)
    codes1, rows1 = _engine_run(m, conds, 12, sp, 1, True)
    codes0, rows0 = _engine_run(m, conds, 12, sp, 1, False)
    for s in range(slots):
        assert torch.equal(codes1[s], codes2[s]) and torch.equal(codes1[s], codes0[s]), s
        assert torch.equal(rows1[s], rows2[2 * s]) and torch.equal(rows2[2 * s], rows2[2 * s + 1]), s
        assert torch.equal(rows1[s], rows0[s]), s
    assert not torch.equal(codes1[0], codes1[-1]) or slots == 1


# ---------------------------------------------------------------------- the batch and streaming entry points
@pytest.fixture(scope="module")
def utterances():
    """Five utterances: conditioning [1, Lc, d] (two with an audio prefix) and max_new_tokens."""
    conds = [cond_single(lc, 512, 40 + i).to(DEV) for i, lc in enumerate((11, 7, 14, 9, 12))]
    prefixes = [None, random_prefix(6, 61).to(DEV), None, random_prefix(12, 63).to(DEV), None]
    mnt = [24, 17, 30, 9, 21]
    return conds, prefixes, mnt


def _alone(m, utterances, sp, seeds):
    conds, prefixes, mnt = utterances
    return [m.generate_batch([c], [p], max_new_tokens=[n], cfg_scale=1, sampling_params=sp, seeds=[sd],
                             max_slots=1)[0] for c, p, n, sd in zip(conds, prefixes, mnt, seeds)]


@pytest.mark.parametrize("count,max_slots", [(3, 2), (5, 3)])
def test_generate_batch_guidance_free_equals_generate_alone(utterances, count, max_slots):
    m = _model("tiny")
    conds, prefixes, mnt = (u[:count] for u in utterances)
    single = [_generate(m, c, p, 1, GREEDY, n=n) for c, p, n in zip(conds, prefixes, mnt)]
    batch = m.generate_batch(conds, prefixes, max_new_tokens=mnt, cfg_scale=1, sampling_params=GREEDY,
                             max_slots=max_slots)
    e = m.engine
    assert e.rps == 1 and e.prefill_batch and e.S >= max_slots
    for a, b in zip(single, batch):
        assert torch.equal(a, b)
    seeds = list(range(200, 200 + count))
    want = _alone(m, (conds, prefixes, mnt), MINP, seeds)
    got = m.generate_batch(conds, prefixes, max_new_tokens=mnt, cfg_scale=1, sampling_params=MINP, seeds=seeds,
                           max_slots=max_slots)
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    # the same utterances guided, on duplicated rows: the same codes (the stepped row counts differ: k against 2 k)
    dup = m.generate_batch([torch.cat([c, c]) for c in conds], prefixes, max_new_tokens=mnt, cfg_scale=3.0,
                           sampling_params=MINP, seeds=seeds, max_slots=max_slots)
    for a, b in zip(want, dup):
        assert torch.equal(a, b)


def test_prefill_many_packs_one_sequence_per_utterance(utterances):
    """A pass holds s_len rows per utterance in the single layout (2 s_len in the paired one): its sequence table."""
    m = _model("tiny")
    m._ensure_capacity(3, 128, 64)
    e = m.engine
    seen = []
    orig = e._prefill_layers
    e._prefill_layers = lambda rows, max_pos, seqs: (seen.append((rows, list(seqs))), orig(rows, max_pos, seqs))[1]
    try:
        conds, prefixes, mnt = (u[:3] for u in utterances)
        for rps in (1, 2):
            e.set_layout(rps)
            e.prefill_many([(s, c if rps == 1 else torch.cat([c, c]), p, n, SamplingParams(temperature=0.0))
                            for s, (c, p, n) in enumerate(zip(conds, prefixes, mnt))])
            e.stream.synchronize()
            for s in range(3):
                e.release(s)
    finally:
        del e._prefill_layers
    lens = [c.shape[1] + (0 if p is None else p.shape[2]) + 1 for c, p in zip(conds, prefixes)]
    (rows1, seqs1), (rows2, seqs2) = seen
    assert rows1 == sum(lens) and rows2 == 2 * sum(lens)
    assert seqs1 == [(sum(lens[:s]), lens[s], s, 0) for s in range(3)]
    assert [q[2] for q in seqs2] == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("sp", [GREEDY, MINP], ids=["greedy", "min_p"])
def test_stream_guidance_free_equals_generate_then_decode(utterances, sp):
    m = _model("tiny")
    conds, prefixes, mnt = utterances
    for i in (0, 3):
        want = m.autoencoder.decode(_generate(m, conds[i], prefixes[i], 1, sp, seed=9, n=mnt[i]))
        torch.manual_seed(9)
        chunks = list(m.stream(conds[i], prefixes[i], max_new_tokens=mnt[i], cfg_scale=1, sampling_params=sp,
                               chunk_frames=4))
        assert len(chunks) > 1 and torch.equal(torch.cat(chunks, dim=-1), want)


@pytest.mark.parametrize("decoder", ["window", "carry"])
def test_stream_batch_guidance_free_equals_generate_then_decode(utterances, decoder):
    m = _model("tiny")
    conds, prefixes, mnt = utterances
    seeds = list(range(300, 305))
    want = [m.autoencoder.decode(c) for c in _alone(m, utterances, MINP, seeds)]
    got = {i: [] for i in range(5)}
    lasts = []
    for i, w, last in m.stream_batch(conds, prefixes, max_new_tokens=mnt, cfg_scale=1, sampling_params=MINP,
                                     seeds=seeds, max_slots=3, chunk_frames=4, decoder=decoder):
        got[i].append(w)
        if last:
            lasts.append(i)
    assert sorted(lasts) == list(range(5))
    for i in range(5):
        assert torch.equal(torch.cat(got[i], dim=-1), want[i]), i


def test_serve_guidance_free_session(utterances):
    m = _model("tiny")
    conds, prefixes, mnt = utterances
    seeds = list(range(400, 405))
    sps = [GREEDY, MINP, dict(top_k=50), GREEDY, MINP]
    want = [m.autoencoder.decode(m.generate_batch([c], [p], max_new_tokens=[n], cfg_scale=1, sampling_params=sp,
                                                  seeds=[sd], max_slots=1)[0])
            for c, p, n, sp, sd in zip(conds, prefixes, mnt, sps, seeds)]
    other = cond_single(conds[1].shape[1], 512, 99).to(DEV)
    with m.serve(2, max_seqlen=128, max_prefill=64, chunk_frames=4, guidance=False) as session:
        assert m.engine.rps == 1

        def submit(i):  # request 1 as [2, Lc, d] (row 0 is used), the others as [1, Lc, d]
            c = torch.cat([conds[i], other]) if i == 1 else conds[i]
            return session.submit(c, prefixes[i], max_new_tokens=mnt[i], cfg_scale=1, sampling_params=sps[i],
                                  seed=seeds[i])
        with pytest.raises(ValueError):
            session.submit(conds[0], max_new_tokens=4, cfg_scale=2.0)
        with pytest.raises(ValueError):
            session.submit(conds[0], max_new_tokens=200, cfg_scale=1)  # the capacity arithmetic holds
        tickets, items = {}, []
        for i in (0, 1):
            tickets[submit(i)] = i
        for rnd in range(1, 6):  # requests 2, 3, 4 are admitted while others are being spoken
            items += session.run_round()
            if rnd == 2:
                tickets[submit(2)] = 2
        for i in (3, 4):
            tickets[submit(i)] = i
        while not session.idle:
            items += session.run_round()
        with pytest.raises(RuntimeError):
            m.generate(conds[0], max_new_tokens=4, cfg_scale=1, progress_bar=False)
    assert list(tickets) == [0, 1, 2, 3, 4]
    for t, i in tickets.items():
        mine = [(w, last) for tk, w, last in items if tk == t]
        assert [last for _, last in mine].count(True) == 1 and mine[-1][1], t
        assert torch.equal(torch.cat([w for w, _ in mine], dim=-1), want[i]), t
    # a guided session still refuses cfg_scale = 1 and the one-row shape
    with m.serve(2, max_seqlen=128, max_prefill=64, chunk_frames=4) as session:
        assert m.engine.rps == 2
        with pytest.raises(AssertionError):
            session.submit(torch.cat([conds[0], conds[0]]), max_new_tokens=4, cfg_scale=1)
        with pytest.raises(ValueError):
            session.submit(conds[0], max_new_tokens=4)


# ---------------------------------------------------------------------- one model, both layouts
@pytest.mark.parametrize("name", ["wide", "hybrid"])
def test_layout_switching_leaves_nothing_stale(name):
    """Guided, guidance-free, guided, guidance-free on one model (different conditioning rows, so the results
    differ): each equals what a fresh model gives."""
    cfg, kw, lc = MODELS[name]
    d = cfg().backbone.d_model
    c0, c1 = cond_single(lc, d, 70).to(DEV), cond_single(lc, d, 71).to(DEV)
    guided_cond = torch.cat([c0, c1])
    prefix = random_prefix(5, 72).to(DEV)
    fresh_guided = _generate(_synth(cfg(), **kw), guided_cond, prefix, 2.0, MINP)
    fresh_free = _generate(_synth(cfg(), **kw), c0, None, 1, MINP)
    assert not torch.equal(fresh_guided[..., 5:], fresh_free[..., : N_NEW])
    m = _synth(cfg(), **kw)
    for rnd in range(2):
        assert torch.equal(_generate(m, guided_cond, prefix, 2.0, MINP), fresh_guided), rnd
        assert m.engine.rps == 2
        assert torch.equal(_generate(m, c0, None, 1, MINP), fresh_free), rnd
        assert m.engine.rps == 1
    batch = m.generate_batch([guided_cond, guided_cond], [prefix, prefix], max_new_tokens=N_NEW, cfg_scale=2.0,
                             sampling_params=GREEDY)
    assert m.engine.rps == 2 and torch.equal(batch[0], batch[1])
    free = m.generate_batch([c0, c1, c0], max_new_tokens=N_NEW, cfg_scale=1, sampling_params=GREEDY)
    assert torch.equal(free[0], free[2]) and torch.equal(free[0], _generate(m, c0, None, 1, GREEDY))


def test_set_layout_only_while_no_slot_is_active():
    m = _model("tiny")
    m._ensure_capacity(1, 128, 64)
    e = m.engine
    e.set_layout(2)
    c = _cond("tiny")
    e.prefill(0, torch.cat([c, c]), None, 8, SamplingParams(temperature=0.0))
    with pytest.raises(RuntimeError):
        e.set_layout(1)
    with pytest.raises(ValueError):
        e.set_layout(3)
    e.set_layout(2)  # no change: allowed
    e.release(0)
    e.set_layout(1)
    with pytest.raises(ValueError):
        e.prefill(0, torch.cat([c, c, c]), None, 8, SamplingParams(temperature=0.0))
    e.set_layout(2)
    with pytest.raises(ValueError):
        e.prefill(0, c, None, 8, SamplingParams(temperature=0.0))  # the paired layout takes [2, Lc, d] only
    with pytest.raises(ValueError):
        m.generate(c, max_new_tokens=4, progress_bar=False)  # cfg_scale 2.0 with one conditioning row


# ---------------------------------------------------------------------- against the CPU oracle
def test_single_layout_logits_match_the_oracle_teacher_forced():
    """Teacher-forced along the reference's greedy_maxlen trajectory (fixture), the single layout's logits against
    OracleZonos.prefill / compute_logits at cfg_scale = 1.0 on a one-row cache (tests/cfg1_cases.oracle_run), by the
    rule and the number of test_gpu_generate.test_teacher_forced_decisions_match_reference (the guided path's tiny-
    model logit test): per decision and codebook, the GPU's score of the oracle's top token is within NOISE_FACTOR x
    the case's exact-GEMM noise + 0.5 bf16 ulps of the oracle's top score, and the GPU picks the same token wherever
    the oracle's top-1 / top-2 margin exceeds twice that bound."""
    from oracle.zonos_cpu import OracleZonos
    from tests.test_gpu_generate import NOISE_FACTOR, _ulp
    t, meta = load_golden("tiny_trajectories")
    case = next(c for c in meta["cases"] if c["tag"] == "greedy_maxlen")
    bound = NOISE_FACTOR * case["exact_gemm_noise"]["max_ulps"] + 0.5
    cfg = ZonosConfig.from_dict(meta["cfg"])
    cond = t["greedy_maxlen/cond"][:1]
    dl = t["greedy_maxlen/delayed"].long()  # [1, 9, N + 9]
    n, n_dec = case["n"], 12
    om = OracleZonos(cfg, synthetic_weights(cfg, **case["model_kw"]))
    _, ref, _ = oracle_run(om, cond, None, n, 1, GREEDY, teacher=dl, max_decisions=n_dec)

    m = _synth(cfg, max_seqlen=128, max_prefill=64)
    m._select_layout(1)
    e = m.engine
    e.prefill(0, cond.to(DEV), None, n, SamplingParams(temperature=0.0))
    e.stream.synchronize()
    got = [e.logits_pre[0].float().cpu()]
    for _ in range(n_dec - 1):
        with torch.cuda.stream(e.stream):  # the reference's frames, whatever the GPU sampler chose
            e.delayed[0, :, : dl.shape[-1]] = dl[0].to(DEV, torch.int32)
            for k, v in (("active", 1), ("stopping", 0), ("remaining", 1000)):
                e.st[k][0] = v
            e.refresh_inputs()
        e.step(1, use_graph=False, slots=1)
        e.stream.synchronize()
        got.append(e.logits[0].float().cpu())
    e.check_errors()
    e.release(0)
    worst, rows, determined = 0.0, 0, 0
    for i, (g, r) in enumerate(zip(got, ref)):
        g, r = g.clone(), r[0].clone()
        g[:, 1025:] = -torch.inf
        if i:  # decode steps: the EOS bias on codebooks 1..8 (model.py:266-267), on both
            g[1:, 1024] = r[1:, 1024] = -torch.inf
        top2 = r.topk(2, dim=-1)
        for k in range(9):
            tok, top = int(top2.indices[k, 0]), top2.values[k, 0]
            u = float(_ulp(top))
            err = abs(float(g[k, tok]) - float(top)) / u
            margin = float(top - top2.values[k, 1]) / u
            worst, rows = max(worst, err), rows + 1
            if margin > 2 * bound:
                determined += 1
                assert int(g[k].argmax()) == tok, dict(decision=i, codebook=k, margin_ulps=margin)
    print(f"cfg1 oracle: {rows} decisions, {determined} determined, max err {worst:.2f} ulps (bound {bound})")
    assert rows == 9 * n_dec and determined > 0
    assert worst <= bound, dict(max_err_ulps=worst, bound_ulps=bound)
