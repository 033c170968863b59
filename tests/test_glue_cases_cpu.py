"""tests/glue_cases.py judged on the CPU: the sequential bf16 embedding sum against an independent restatement, the
`cancel` table telling it from an fp32 sum rounded once and from the reversed order on most elements (both mutants
miss), the token and slot builders, and the delay-pattern references against their definition. No GPU."""
import pytest
import torch

from tests import glue_cases as gc

D = 264  # the tables of the CPU test: a width of its own, the builders are the same at every width


@pytest.fixture(scope="module")
def tables():
    return {k: gc.table(D, k) for k in ("seeded", "cancel")}


def _bfround(x):
    return x.to(torch.bfloat16).float()


def test_embed_ref_is_the_sequential_bf16_sum(tables):
    """Restated with explicit roundings: acc = bf16(fp32(acc) + fp32(e_k)), k = 1 .. 8."""
    toks = gc.code_columns(3)
    for tab in tables.values():
        t = gc.clamp_tokens(toks)
        acc = tab[0, t[0]].float()
        for k in range(1, gc.NCB):
            acc = _bfround(acc + tab[k, t[k]].float())
        assert torch.equal(gc.embed_ref(tab, toks).float(), acc)


def test_tokens_cover_the_edges_and_are_clamped(tables):
    for n in (1, 3):
        c = gc.code_columns(n)
        for col in range(n):
            assert set(gc.EDGE_TOKENS) <= set(c[:, col].tolist())
        p = gc.padded_codes(c)
        assert p.shape[1] > n and torch.equal(p[:, :n], c) and bool((p[:, n:] == 7).all())
    lo = torch.full((gc.NCB, 1), -1, dtype=torch.int32)
    hi = torch.full((gc.NCB, 1), 1026, dtype=torch.int32)
    tab = tables["seeded"]
    assert torch.equal(gc.embed_ref(tab, lo), gc.embed_ref(tab, torch.zeros_like(lo)))
    assert torch.equal(gc.embed_ref(tab, hi), gc.embed_ref(tab, torch.full_like(hi, 1025)))
    # a codebook read from another codebook's table, or a neighbouring token, gives another row
    c = gc.code_columns(1)
    ref = gc.embed_ref(tab, c)
    assert not torch.equal(gc.embed_ref(tab.roll(1, 0), c), ref)
    assert not torch.equal(gc.embed_ref(tab, (c + 1)), ref)


@pytest.mark.parametrize("mutant", [gc.embed_fp32_once, gc.embed_reversed], ids=["fp32_once", "reversed"])
def test_cancel_table_tells_the_mutants_apart(tables, mutant):
    toks = gc.code_columns(3)
    ref = gc.embed_ref(tables["cancel"], toks)
    differ = (mutant(tables["cancel"], toks) != ref).float().mean().item()
    seeded = (mutant(tables["seeded"], toks) != gc.embed_ref(tables["seeded"], toks)).float().mean().item()
    print(f"{mutant.__name__}: differs on {differ:.3f} of the cancel elements, {seeded:.3f} of the seeded ones")
    assert differ > 0.5
    assert bool(torch.isfinite(ref.float()).all()) and float(ref.float().abs().max()) < 8


def test_step_state(tables):
    for tcap in (16, 300):
        st = gc.step_state(tcap)
        assert st["active"].tolist() == [1, 0, 1, 1]
        assert st["offset"][0] == 0 and st["offset"][2] == tcap - 1
        fr = gc.step_frames(st)
        assert fr.shape == (gc.NCB, 4)
        for s in range(4):
            assert set(gc.EDGE_TOKENS) <= set(fr[:, s].tolist())
        assert int(st["delayed"].min()) == -1 and int(st["delayed"].max()) == 1026


def test_delay_references():
    # the definition: codebook k is delayed by k + 1 columns, MASK elsewhere
    for T in gc.APPLY_T:
        codes = gc.audio_codes(3, T)
        out = gc.apply_delay_pattern(codes, 777)
        assert out.shape == (3, gc.NCB, T + gc.NCB)
        for k in range(gc.NCB):
            assert torch.equal(out[:, k, k + 1:k + 1 + T], codes[:, k])
            assert bool((out[:, k, :k + 1] == 777).all()) and bool((out[:, k, k + 1 + T:] == 777).all())
        assert torch.equal(gc.revert_delay_pattern(out), codes)


def test_init_reference():
    cases = gc.init_cases()
    assert len(cases) == 3 * (1 + 2 + 3)
    for tcap, p, total in cases:
        prefix = gc.audio_codes(1, p, tcap)[0]
        ref = gc.init_ref(tcap, prefix, total)
        assert ref.shape == (gc.NCB, tcap) and bool((ref[:, total:] == gc.MASK).all())
        for k in range(gc.NCB):
            assert torch.equal(ref[k, k + 1:k + 1 + p].long(), prefix[k])
            assert bool((ref[k, k + 1 + p:total - gc.NCB + k + 1] == -1).all())
            assert bool((ref[k, :k + 1] == gc.MASK).all()) and bool((ref[k, total - gc.NCB + k + 1:] == gc.MASK).all())


def test_revert_reference():
    buf = gc.revert_buffer(3, 64)
    assert set(buf.unique().tolist()) == set(gc.REVERT_VALUES)
    assert not torch.equal(buf[0], buf[2])
    out = gc.revert_ref(buf[2], 55)
    assert out.shape == (gc.NCB, 55) and set(out.unique().tolist()) == {-1, 0, 1023}
    for k in range(gc.NCB):
        raw = buf[2, k, k + 1:k + 56].long()
        assert torch.equal(out[k], torch.where(raw >= 1024, 0, raw))
