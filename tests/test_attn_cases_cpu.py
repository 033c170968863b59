"""tests/attn_cases.py judged on the CPU: every case does what its name says and meets its input conditions, the
restatement of the reference implementation's attention (oracle/attention_cpu.py) and a float32 emulation of the
kernels' chunk order meet the criterion on every case, head geometry and position, and each mutant of that arithmetic
misses it on the case named for it. No GPU."""
import math

import pytest
import torch

from oracle.attention_cpu import attend
from tests import attn_cases as ac
from tests.attn_cases import CASES, GAP, HD, HEADS, LONG_CASES, ONEHOT_PICK, ROWS

HKVS = sorted({hkv for _, hkv in HEADS}, reverse=True)
CASE_HKV = [(c, h) for c in CASES for h in HKVS]


def _ids(v):
    return f"{v[0]}-hkv{v[1]}"


def _scores32(bd, r):
    """fp32 scores [hkv, 4, p + 1] of row r, as the oracle takes them."""
    p = bd.pos[r]
    s = torch.einsum("hgd,hnd->hgn", bd.q[r].double(), bd.k[r, :, :p + 1].double()).float()
    return s * torch.tensor(ac.SCALE, dtype=torch.float32)


def _oracle(bd, kv_rows=None, pos=None, q=None):
    """oracle.attention_cpu.attend on every row (four heads per KV head) -> [R, hkv, 4, 128] bf16."""
    pos = bd.pos if pos is None else pos
    q = bd.q if q is None else q
    out = torch.zeros(len(pos), bd.hkv, 4, HD, dtype=torch.bfloat16)
    for r, p in enumerate(pos):
        if p >= 0:
            kr = r if kv_rows is None else kv_rows[r]
            out[r] = attend(q[r].reshape(bd.hkv * 4, HD), bd.k[kr], bd.v[kr], p).view(bd.hkv, 4, HD)
    return out


# ------------------------------------------------------------------------------------------ the criterion's parts
def test_ulp_and_ratio():
    v = torch.tensor([1.0, 1.5, 2.0, 255.0, 0.0, 2.0 ** -130], dtype=torch.float64)
    assert ac.ulp_bf16(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 1.0, 2.0 ** -133, 2.0 ** -133]
    bd = ac.build_rows("rand1_cancel", 1, (5, -1))
    ref = ac.ref_of(bd)
    got = ref.o64.clone()
    got[0, 0, 0, 0], got[0, 0, 1, 1], got[1] = math.nan, math.inf, 7.0
    r = ac.ratio(got, ref)
    assert r[0, 0, 0, 0] == math.inf and r[0, 0, 1, 1] == math.inf and r[0, 0, 2].max() == 0 and r[1].max() == 0
    assert ac.onehot_candidates(1279) == [0, 1279, 1278, 1272, 1271, 1264, 1263, 1248, 1247, 1152, 1151, 1024, 1023]
    assert (ac.E_of(ref)[0] >= 2.0 ** -8).all() and (ac.E_of(ref)[0] < 1.1 * 2.0 ** -8).all()


def test_every_profile_and_value_kind_appears():
    assert {p for p, _ in CASES.values()} == set(ac.COEF)
    assert {v for _, v in CASES.values()} == {"normal", "tails", "count", "cancel"}
    assert set(LONG_CASES) <= set(CASES)


# ------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("case_hkv", CASE_HKV, ids=_ids)
def test_case_does_what_its_name_says(case_hkv):
    case, hkv = case_hkv
    bd, ref = ac.build(case, hkv), ac.reference(case, hkv)
    prof = bd.profile
    R, S = len(bd.pos), bd.smax
    live = torch.arange(S)[None, :] <= torch.tensor(bd.pos)[:, None]
    vf, lm = bd.v.float(), live[:, None, :, None]
    assert (~lm | (vf.abs() <= ac.VMAX)).all()  # live V is finite and small
    assert (lm | ~torch.isfinite(vf) | (vf.abs() == 2.0 ** 120)).all() and torch.isnan(vf).any()  # stale V is not
    assert torch.isfinite(bd.k.float()).all()
    assert ac.clear_of_underflow(ref)
    seen = set()
    for r, p in enumerate(bd.pos):
        if p < 0:
            continue
        s = _scores32(bd, r)  # [hkv, 4, n]
        if prof == "flat":
            assert (s == 0).all() and (bd.q[r] == 0).all()
            continue
        # one admitted stale key would take >= 1 - e^-60 of the weight
        if p + 1 < S:
            st = ac.scores64(bd.q[r], bd.k[r, :, p + 1:p + 2])[..., 0]
            assert (torch.logsumexp(s.double(), -1) - st <= -60.0).all(), (case, p)
        if p >= 8:  # the heads of a group differ, and so do the KV heads
            for a in range(4):
                for b in range(a + 1, 4):
                    assert not torch.equal(s[:, a], s[:, b]), (case, p, a, b)
            for a in range(hkv):
                for b in range(a + 1, hkv):
                    assert not torch.equal(bd.v[r, a, :p + 1], bd.v[r, b, :p + 1])
                    # (spike0_tail is one K for all; where onehot's candidates coincide, so can two KV heads' peaks)
                    same_k = torch.equal(bd.k[r, a, :p + 1], bd.k[r, b, :p + 1])
                    few = prof == "onehot" and len(set(ac.onehot_candidates(p))) < 13
                    assert not same_k or prof == "spike0_tail" or few
        if prof == "onehot":
            for h in range(hkv):
                for g in range(4):
                    t = int(bd.t[r, h, ONEHOT_PICK[g]])
                    if len(set(ac.onehot_candidates(p))) == 13:
                        seen.add(ac.onehot_candidates(p).index(t))
                    rest = torch.cat([s[h, g, :t], s[h, g, t + 1:]])
                    assert p == 0 or (s[h, g, t] - rest.max() >= GAP), (case, p, h, g)
                    assert ref.wmax[r, h, g] > 1 - 2.0 ** -20
                    other, quarter = ac.onehot_margin(bd, r, h, g)
                    assert other < quarter, (case, p, h, g, other, quarter)
        if prof == "two_peaks":
            for h in range(hkv):
                a, b = (int(x) for x in bd.t[r, h])
                assert (s[h, :, a] == s[h, :, b]).all() and (s[h, :, a] == s[h].amax(-1)).all()
                assert p < 128 or a // 128 != b // 128
                assert p < 512 or a // 512 != b // 512
        if prof in ("steps_up", "steps_down") and p >= 512:
            m = torch.stack([s[..., j * 512:(j + 1) * 512].amax(-1) for j in range(p // 512 + 1)], -1)
            d = m[..., 1:] - m[..., :-1]
            assert (d > 20).all() if prof == "steps_up" else (d < -20).all(), (case, p)
        if prof in ("ramp_up", "ramp_down") and p >= 127:  # head 0: 0.25 per key, up to K's bf16 rounding
            rise = (s[:, 0, -1] - s[:, 0, 0]) / p
            assert ((rise - (0.25 if prof == "ramp_up" else -0.25)).abs() < 0.005).all(), (case, p)
        if prof.startswith("rand") and p >= 1023:
            sd = s[:, :2].double().std(-1) / float(prof[4:])
            assert (sd > 0.9).all() and (sd < 1.1).all(), (case, p)
        if prof in ("offset_pos", "offset_neg"):
            assert (s.abs() > 280).all()
        if prof == "spike0_tail" and p > 0:
            assert (s[..., 0] >= 5).all() and (s[..., 1:] == 0).all()
    if prof == "onehot" and hkv == 4:  # where the 13 candidates are 13 keys, each of them is some head's peak
        assert seen == set(range(13))


# ------------------------------------------------------------------------------------------ correct implementations
def _judge(tag, case, got, ref):
    r = ac.ratio(got, ref)
    worst = r.amax((1, 2, 3))
    print(f"{tag} {case}: max(error / bound) {worst.max():.3f}")
    return worst.max().item()


@pytest.mark.parametrize("case_hkv", CASE_HKV, ids=_ids)
def test_oracle_and_emulation_meet_the_criterion(case_hkv):
    """oracle.attention_cpu.attend and the float32 emulation of the chunk order, on every row of the single-query
    launch (the four heads per KV head cover every group size), and the exact checks on both."""
    case, hkv = case_hkv
    bd, ref = ac.build(case, hkv), ac.reference(case, hkv)
    got = {"oracle": _oracle(bd), "emulation": ac.emu_rows(bd).to(torch.bfloat16)}
    for tag, o in got.items():
        assert _judge(tag, f"{case} hkv={hkv}", o, ref) <= 1.0
        assert torch.equal(o[0], bd.v[0, :, 0][:, None].expand(hkv, 4, HD)), "position 0 is V_0"
        if bd.profile == "onehot":
            for r, p in enumerate(bd.pos):
                for g in range(4):
                    if p >= 0:
                        want = bd.v[r, torch.arange(hkv), bd.t[r, :, ONEHOT_PICK[g]]]
                        assert torch.equal(o[r, :, g], want), (tag, p, g)
    if case == "flat_count":
        assert torch.equal(got["emulation"], got["oracle"])  # exact integers: the same bits in any order


@pytest.mark.parametrize("case", LONG_CASES)
def test_long_row_meets_the_criterion(case):
    bd, ref = ac.build_long(case), ac.reference_long(case)
    assert bd.pos[0] == 8320 and ac.clear_of_underflow(ref)
    assert _judge("oracle", f"{case} long", _oracle(bd), ref) <= 1.0
    few = [0, 14, 19, 26]  # (the emulation on the long row, positions 129, 1023, 2048: the other rows are the oracle's)
    assert _judge("emulation", f"{case} long", ac.emu_rows(bd, rows=few)[few], ac.take(ref, few)) <= 1.0


PREFILL_CASE_HKV = [(c, h) for c, h in CASE_HKV if h == 1 or c in LONG_CASES or "onehot" in c]


@pytest.mark.parametrize("case_hkv", PREFILL_CASE_HKV, ids=_ids)
def test_prefill_rows_meet_the_criterion(case_hkv):
    """The causal rows of the prefill sequences: the oracle on every (sequence, position), with one KV head for every
    case and with four for a few (a row's arithmetic does not depend on the head count)."""
    case, hkv = case_hkv
    bd, ref = ac.build_prefill(case, hkv), ac.reference_prefill(case, hkv)
    seqs, n_rows, kv, pos = ac.prefill_rows()
    assert sorted(s[0] for s in seqs) != [s[0] for s in seqs]  # q rows in another order than the KV rows
    assert sum(p >= 0 for p in pos) == sum(n for _, n in ac.PREFILL_SEQS)
    assert ac.clear_of_underflow(ref)
    q = bd.q[[max(s, 0) for s in kv]]
    got = _oracle(bd, kv, pos, q)
    assert _judge("oracle", f"{case} hkv={hkv} prefill", got, ref) <= 1.0
    if bd.profile == "onehot":  # the peaks lie at or below pos0: every row of a sequence is V_t
        for q0, n, s, p0 in seqs:
            assert (bd.t[s] <= p0).all()
            for g in range(4):
                want = bd.v[s, torch.arange(hkv), bd.t[s, :, ONEHOT_PICK[g]]]
                assert all(torch.equal(got[q0 + i, :, g], want) for i in range(n))


# ------------------------------------------------------------------------------------------ mutants
PROBE_ROWS = [ROWS.index(p) for p in (129, 513, 1279, 2048)]
MUTANTS = {  # mutant -> (the case that must reject it, hkv, switches of emu_rows)
    "the last key dropped": ("ramp_up_count", 1, dict(drop_last=True)),
    "one key past the position admitted": ("rand1_cancel", 1, dict(admit_extra=True)),
    "acc not rescaled by exp(M_{j-1} - M_j)": ("steps_up_normal", 1, dict(no_acc_rescale=True)),
    "l not rescaled": ("steps_up_normal", 1, dict(no_l_rescale=True)),
    "a key at a chunk edge counted twice": ("flat_count", 1, dict(dup_edge=True)),
    "a query head reading the neighbouring KV head": ("rand4_count", 4, dict(kv_shift=1)),
    "two heads of a group swapped": ("rand12_tails", 1, dict(swap_heads=True)),
    "the scale omitted": ("rand1_cancel", 1, dict(no_scale=True)),
    "exp before the maximum is subtracted (+300)": ("offset_pos_cancel", 1, dict(exp_first=True)),
    "exp before the maximum is subtracted (-300)": ("offset_neg_normal", 1, dict(exp_first=True)),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_is_rejected_by_its_case(mutant):
    case, hkv, sw = MUTANTS[mutant]
    bd, ref = ac.build(case, hkv), ac.reference(case, hkv)
    good = ac.ratio(ac.emu_rows(bd, rows=PROBE_ROWS), ref)[PROBE_ROWS]
    bad = ac.ratio(ac.emu_rows(bd, rows=PROBE_ROWS, **sw), ref)[PROBE_ROWS]
    per_row = bad.amax((1, 2, 3))
    print(f"{mutant} on {case}: max(error / bound) per row {[f'{x:.3g}' for x in per_row.tolist()]}")
    assert good.max() <= 1.0
    assert bad.max() > 1.0, f"{case} does not reject: {mutant}"
    if "rescaled" not in mutant:  # (a rescaling needs a second block: the rows from position 513 on)
        assert (per_row > 1.0).all(), f"{case} does not reject at every probed position: {mutant}"
    else:
        assert (per_row[1:] > 1.0).all(), f"{case} does not reject past one block: {mutant}"
