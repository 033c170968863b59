"""The single row layout of the sampler kernels (ZmiSlots.rows_per_slot = 1: guidance-free generation, one logits /
activation / KV row per slot) through the C ABI, against the paired layout on the same logits duplicated into rows
2s and 2s + 1. There u == c bit for bit, so the paired score u + (c - u) * cfg is c exactly, whatever cfg: every
output must be identical, with no tolerance: tokens, the delayed frame write, every slot-state array, the next
step's (kv row, position) and the fused embedding of the next input frame (x1[s] == x2[2s]). The single layout
touches nothing of rows S .. 2S - 1. Covers zmi_sample_step (decode and prefill mode, hashed noise and a caller's
noise buffer, greedy / min_p / top_k / top_p slots side by side), zmi_sample_step_greedy and zmi_embed_step; an
inactive slot, an EOS pick on codebook 0, exact ties, a slot whose frame is past total_len, three penalties."""
import ctypes

import pytest
import torch

from zonos_vibes_amd.engine import SamplingParams

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, D, TCAP = 4, 64, 96
ST_KEYS = ("active", "pos", "offset", "remaining", "stopping", "step", "total_len")
SENTINEL = -3
PENS = [(3.0, 2), (2.0, -5), (1.0, 2)]


def _state(seed):
    """Slot state, history, logits [S, 9, 1026] and embeddings (the shapes and cases of test_gpu_sampler_greedy)."""
    g = torch.Generator().manual_seed(seed)
    st = {k: torch.zeros(S, dtype=torch.int32) for k in ST_KEYS}
    delayed = torch.randint(0, 1026, (S, 9, TCAP), generator=g, dtype=torch.int32)
    for s in range(S):
        off = int(torch.randint(12, 60, (1,), generator=g))
        st["offset"][s] = off
        st["pos"][s] = off + 20
        st["remaining"][s] = [30, 9, 3, 1][s]
        st["stopping"][s] = s == 2
        st["step"][s] = off
        st["total_len"][s] = [TCAP - 4, TCAP - 4, TCAP - 4, off + 1][s]  # slot 3: frame past the total length
        st["active"][s] = s != 1 or seed % 2 == 0                        # odd seeds: slot 1 inactive
        delayed[s, :, off + 1:] = -1  # the frame being written and later ones are unknown
        delayed[s, 5:, off + 1] = 7   # ... except the delay pattern's already-known cells
    logits = torch.randn(S, 9, 1026, generator=g) * 3
    logits[:, :, 100] = logits[:, :, 101] = 50.0  # exact ties: the first index wins
    logits[0, 0, 1024] = 80.0                     # slot 0 codebook 0 picks EOS
    emb = (torch.randn(9, 1026, D, generator=g) * 0.1).to(torch.bfloat16)
    noise = torch.empty(S, 9, 1026).exponential_(1.0, generator=g)
    return st, delayed, logits, emb, noise


def _run(state, params, rps, call, mode=0, use_noise=False, layout_field=None):
    """One launch in the layout `rps` (1: logits as given; 2: each row duplicated into rows 2s, 2s + 1)."""
    from zonos_vibes_amd import _lib as L
    st0, delayed0, logits, emb, noise = state
    lib, sp = L.lib(), torch.cuda.current_stream().cuda_stream
    st = {k: v.clone().to(DEV) for k, v in st0.items()}
    delayed = delayed0.clone().to(DEV)
    prm = torch.tensor(bytearray(b"".join(bytes(bytearray(p.to_c())) for p in params)), dtype=torch.uint8).to(DEV)
    sl = L.Slots(*(st[k].data_ptr() for k in ("active", "pos", "offset", "remaining", "stopping", "step")),
                 delayed.data_ptr(), prm.data_ptr(), st["total_len"].data_ptr(), TCAP, S)
    assert sl.rows_per_slot == 0  # eleven positional fields: the paired layout
    sl.rows_per_slot = rps if layout_field is None else layout_field
    lg = (logits if rps == 1 else logits.repeat_interleave(2, dim=0)).contiguous().to(DEV)
    e = emb.to(DEV)
    nz = noise.to(DEV) if use_noise else None
    nxt = torch.full((S, 9), -7, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(S, dtype=torch.int32, device=DEV)
    x = torch.full((2 * S, D), 7.0, dtype=torch.bfloat16, device=DEV)
    row_kv = torch.full((2 * S,), SENTINEL, dtype=torch.int32, device=DEV)
    row_pos = torch.full((2 * S,), SENTINEL, dtype=torch.int32, device=DEV)
    if call == "greedy":
        rc = lib.zmi_sample_step_greedy(ctypes.byref(sl), lg.data_ptr(), nxt.data_ptr(), 0, S, e.data_ptr(), D,
                                        x.data_ptr(), row_kv.data_ptr(), row_pos.data_ptr(), sp)
    elif call == "embed":
        rc = lib.zmi_embed_step(ctypes.byref(sl), e.data_ptr(), D, x.data_ptr(), row_kv.data_ptr(),
                                row_pos.data_ptr(), sp)
    else:
        rc = lib.zmi_sample_step(ctypes.byref(sl), lg.data_ptr(), None if nz is None else nz.data_ptr(),
                                 nxt.data_ptr(), cnt.data_ptr(), mode, 0, S, e.data_ptr(), D, x.data_ptr(),
                                 row_kv.data_ptr(), row_pos.data_ptr(), sp)
    torch.cuda.synchronize()
    out = dict(next=nxt.cpu(), delayed=delayed.cpu(), x=x.cpu(), row_kv=row_kv.cpu(), row_pos=row_pos.cpu(),
               **{k: v.cpu() for k, v in st.items()})
    return rc, out


def _compare(single, paired, active, sampled=True):
    if sampled:
        assert torch.equal(single["next"][active], paired["next"][active]), "tokens"
        assert (single["next"][~active] == -7).all(), "an inactive slot's tokens are untouched"
    for k in ("delayed",) + ST_KEYS:
        assert torch.equal(single[k], paired[k]), k
    x1, x2 = single["x"], paired["x"]
    assert torch.equal(x1[:S], x2[0::2]), "x1[s] == x2[2s]"
    assert torch.equal(x2[0::2], x2[1::2])
    assert torch.equal(single["row_pos"][:S], paired["row_pos"][0::2]), "row_pos"
    # rows S .. 2S - 1 are not the single layout's: sentinels untouched
    assert (x1[S:] == 7.0).all() and (single["row_kv"][S:] == SENTINEL).all() and \
        (single["row_pos"][S:] == SENTINEL).all(), "rows >= n_slots were written"
    return x1


def _mixed(pen):
    """Greedy, min_p, top_k and top_p + unified slots side by side; the paired side runs a guidance scale != 1."""
    kw = dict(repetition_penalty=pen[0], repetition_penalty_window=pen[1])
    mk = lambda cfg: [SamplingParams(temperature=0.0, cfg_scale=cfg, seed=11, **kw),  # noqa: E731
                      SamplingParams(min_p=0.1, cfg_scale=cfg, seed=12, **kw),
                      SamplingParams(top_k=5, temperature=0.8, cfg_scale=cfg, seed=13, **kw),
                      SamplingParams(top_p=0.9, linear=0.5, conf=0.4, quad=0.1, cfg_scale=cfg, seed=14, **kw)]
    return mk(1.0), mk(2.0)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("pen", PENS)
@pytest.mark.parametrize("mode,use_noise", [(0, False), (0, True), (1, False), (1, True)])
def test_sample_step_single_equals_paired_on_duplicated_rows(seed, pen, mode, use_noise):
    state = _state(seed)
    p1, p2 = _mixed(pen)
    rc2, paired = _run(state, p2, 2, "step", mode, use_noise)
    rc1, single = _run(state, p1, 1, "step", mode, use_noise)
    assert rc1 == 0 and rc2 == 0
    active = state[0]["active"].bool()
    _compare(single, paired, active)
    live = paired["active"].bool()  # still running after the step: their rows are tabled
    assert torch.equal(single["row_kv"][:S][active], torch.arange(S, dtype=torch.int32)[active])
    assert (single["row_pos"][:S][active & ~live] == -1).all()
    if mode == 0 and seed == 0:  # the EOS pick on codebook 0 went through the state machine
        assert int(single["next"][0, 0]) == 1024 and int(single["stopping"][0]) == 1


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("pen", PENS)
def test_greedy_sampler_single_equals_paired_and_the_codebook_workgroups(seed, pen):
    state = _state(seed)
    mk = lambda cfgs: [SamplingParams(temperature=0.0, repetition_penalty=pen[0],  # noqa: E731
                                      repetition_penalty_window=pen[1], cfg_scale=c) for c in cfgs]
    rc2, paired = _run(state, mk((2.0, 1.0, 3.0, 2.0)), 2, "greedy")
    rc1, single = _run(state, mk((1.0,) * 4), 1, "greedy")
    rc0, step = _run(state, mk((7.0,) * 4), 1, "step")  # cfg_scale is ignored in the single layout
    assert rc0 == 0 and rc1 == 0 and rc2 == 0
    active = state[0]["active"].bool()
    _compare(single, paired, active)
    for k in single:
        if k == "next":
            assert torch.equal(single[k][active], step[k][active]), k
        else:
            assert torch.equal(single[k], step[k]), k
    assert torch.equal(single["row_kv"][:S][active], torch.arange(S, dtype=torch.int32)[active])
    assert int(single["next"][2, 1]) == 100 or pen[0] != 1.0  # the exact tie: first index (no penalty in the way)


@pytest.mark.parametrize("seed", [0, 1])
def test_embed_step_single_equals_paired(seed):
    state = _state(seed)
    prm = [SamplingParams(temperature=0.0)] * S
    rc2, paired = _run(state, prm, 2, "embed")
    rc1, single = _run(state, prm, 1, "embed")
    assert rc1 == 0 and rc2 == 0
    active = state[0]["active"].bool()
    x1 = _compare(single, paired, active, sampled=False)
    assert torch.equal(single["row_kv"][:S], torch.arange(S, dtype=torch.int32))  # written for every slot
    assert (single["row_pos"][:S][~active] == -1).all()
    assert (x1[:S][~active] == 7.0).all(), "an inactive slot's row is not embedded"


@pytest.mark.parametrize("call", ["step", "greedy", "embed"])
def test_rows_per_slot_3_is_refused_with_nothing_written(call):
    from zonos_vibes_amd import _lib as L
    state = _state(0)
    rc, out = _run(state, [SamplingParams(temperature=0.0)] * S, 1, call, layout_field=3)
    assert rc != 0 and b"rows_per_slot" in L.lib().zmi_last_error()
    assert (out["next"] == -7).all() and (out["x"] == 7.0).all()
    assert (out["row_kv"] == SENTINEL).all() and (out["row_pos"] == SENTINEL).all()
    assert torch.equal(out["delayed"], state[1])
    for k in ST_KEYS:
        assert torch.equal(out[k], state[0][k]), k
