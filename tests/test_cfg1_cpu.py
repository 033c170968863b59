"""CPU checks around guidance-free generation (cfg_scale = 1): the oracle loop the GPU tests compare against
(tests/cfg1_cases.oracle_run) reproduces OracleZonos.generate() exactly in its guided mode; SlotScheduler under
guidance=False; the eleven-field Slots keeps the paired layout."""
import pytest
import torch

from tests.cfg1_cases import cond_single, oracle_run, random_prefix
from tests.helpers import synthetic_weights
from zonos_vibes_amd.config import tiny_transformer
from zonos_vibes_amd.serving import SlotScheduler


@pytest.fixture(scope="module")
def oracle():
    from oracle.zonos_cpu import OracleZonos
    cfg = tiny_transformer(2)
    return cfg, OracleZonos(cfg, synthetic_weights(cfg, zero_eos=True))


@pytest.mark.parametrize("params,p", [(dict(temperature=0.0), 0), (dict(temperature=0.0), 5), (dict(min_p=0.1), 0)])
def test_helper_loop_reproduces_oracle_generate_in_guided_mode(oracle, params, p):
    cfg, om = oracle
    d = cfg.backbone.d_model
    cond = torch.cat([cond_single(7, d, 1), cond_single(7, d, 2)])
    prefix = random_prefix(p, 3) if p else None
    torch.manual_seed(5)
    raw = []
    ref = om.generate(cond, prefix, 6, 2.0, params, raw_trace=raw)
    torch.manual_seed(5)
    got, trace, delayed = oracle_run(om, cond, prefix, 6, 2.0, params)
    assert torch.equal(got, ref)
    assert torch.equal(delayed, om.last_delayed)
    assert len(trace) == len(raw) == 6 + 9
    assert torch.equal(trace[0], raw[0])  # (the later raw_trace entries carry the EOS bias)
    for a, b in zip(trace[1:], raw[1:]):
        assert torch.equal(a[..., :1024], b[..., :1024])


def test_helper_loop_single_mode_runs_one_row(oracle):
    """cfg_scale = 1: one cache row, [1, Lc, d] or row 0 of [2, Lc, d]; with identical conditioning rows the guided
    logits u + (c - u) * cfg are the single row's logits exactly, so the codes agree."""
    cfg, om = oracle
    d = cfg.backbone.d_model
    c = cond_single(7, d, 1)
    one, trace1, _ = oracle_run(om, c, None, 6, 1, dict(temperature=0.0))
    two, _, _ = oracle_run(om, torch.cat([c, cond_single(7, d, 9)]), None, 6, 1, dict(temperature=0.0))
    dup, trace2, _ = oracle_run(om, torch.cat([c, c]), None, 6, 2.0, dict(temperature=0.0))
    assert trace1[0].shape == (1, 9, 1026)
    assert torch.equal(one, two)
    assert torch.equal(one, dup)
    for a, b in zip(trace1, trace2):
        assert torch.equal(a, b)


def test_scheduler_guidance_free_accepts_one_row_and_keeps_the_capacity_arithmetic():
    free = SlotScheduler(2, max_seqlen=64, max_prefill=32, d_model=512, guidance=False)
    guided = SlotScheduler(2, max_seqlen=64, max_prefill=32, d_model=512)
    assert free.fit((1, 10, 512), None, 20) == (10, 0)
    assert free.fit((2, 10, 512), (1, 9, 4), 20) == (10, 4)
    with pytest.raises(ValueError):
        guided.fit((1, 10, 512), None, 20)
    assert guided.fit((2, 10, 512), None, 20) == (10, 0)
    for sched, rows in ((free, 1), (guided, 2)):
        assert sched.fit((rows, 10, 512), None, 45) == (10, 0)          # 10 + 45 + 9 = 64
        with pytest.raises(ValueError):
            sched.fit((rows, 10, 512), None, 46)                        # Lc + n + 9 > max_seqlen
        assert sched.fit((rows, 31, 512), None, 4) == (31, 0)           # 31 + 1 = 32
        with pytest.raises(ValueError):
            sched.fit((rows, 32, 512), None, 4)                         # Lc + 1 > max_prefill
        with pytest.raises(ValueError):
            sched.fit((rows, 20, 512), (1, 9, 12), 4)                   # Lc + P + 1 > max_prefill
        with pytest.raises(ValueError):
            sched.fit((rows, 10, 256), None, 4)                         # d_model
        with pytest.raises(ValueError):
            sched.fit((3, 10, 512), None, 4)
    t = free.submit((1, 10, 512), None, 8)
    assert free.begin_round()[1][0][1].ticket == t


def test_slots_with_eleven_positional_fields_is_the_paired_layout():
    from zonos_vibes_amd import _lib as L
    sl = L.Slots(*range(1, 10), 96, 4)
    assert (sl.tcap, sl.n_slots, sl.rows_per_slot) == (96, 4, 0)
    assert L.Slots._fields_[-1][0] == "rows_per_slot" and len(L.Slots._fields_) == 12
    assert L.ABI_VERSION == 10
