"""Every Mamba2 step and scan form against the fp64 reference of tests/mamba_cases.py, on crafted regimes.

Forms: zmi_mamba2_scan (one workgroup per sequence and head), zmi_mamba2_scan_ws under ZMI_OPT_SCAN_PQ = 1, 2, 4
(mamba2_scan2_kernel<1 / 2 / 4>) and 0 (the SSD form up to 256 positions, the 4-workgroup scan past it),
zmi_mamba2_scan_seqs with every length in one launch under PQ 0 and 2, and zmi_mamba2_step. Geometry, regimes, the
reference, the input conditions and the criterion

    |got - ref64| <= E S_abs + 0.5 ulp_bf16(|ref64| + E S_abs),  E = 2^-14, elementwise, for y and for the state,

are those of tests/mamba_cases.py (derived there; tests/test_mamba_cases_cpu.py holds float32 emulations and mutants
to it). Ring slots must match bit for bit; in the conv case y must equal the conv output bit for bit. Every test
prints max(error / bound) per head regime.

Measured on an MI355X, max(error / bound) of y / of the state over every launch of this module (lengths 1, 4, 17, 32,
33, 256, 257, strided, permuted, handover); 1.0 is the criterion, ~0.98 is a result that differs from fp64 by its own
bf16 rounding alone:

                          scan        ws_pq1        ws_pq2        ws_pq4        ws_ssd      seqs_pq0      seqs_pq2          step
ordinary           0.979/0.984   0.979/0.984   0.979/0.984   0.979/0.984   0.979/0.984   0.979/0.984   0.979/0.984   0.979/0.984
slow               0.983/0.981   0.983/0.981   0.983/0.981   0.983/0.981   0.983/0.981   0.983/0.981   0.983/0.981   0.968/0.984
fast               0.969/0.983   0.969/0.983   0.969/0.983   0.969/0.983   0.969/0.983   0.969/0.983   0.969/0.983   0.948/0.984
threshold          0.968/0.984   0.968/0.984   0.968/0.984   0.968/0.984   0.968/0.984   0.968/0.984   0.968/0.984   0.966/0.984
reset              0.977/0.984   0.977/0.984   0.977/0.984   0.977/0.984   0.977/0.984   0.977/0.984   0.977/0.984   0.947/0.984
reset130           0.974/0.983   0.974/0.983   0.974/0.983   0.974/0.983   0.974/0.983   0.974/0.982   0.974/0.982   0.964/0.984
tails_ordinary     0.983/0.982   0.983/0.982   0.983/0.982   0.983/0.982   0.984/0.982   0.984/0.982   0.983/0.982   0.981/0.984
tails_slow         0.983/0.984   0.983/0.984   0.983/0.984   0.983/0.984   0.983/0.985   0.983/0.985   0.983/0.984   0.977/0.984
tails_reset        0.982/0.983   0.982/0.983   0.982/0.983   0.982/0.983   0.982/0.983   0.982/0.983   0.982/0.983   0.975/0.984
cancel_a           0.908/0.982   0.908/0.982   0.908/0.982   0.908/0.982   0.908/0.982   0.908/0.982   0.908/0.982   0.973/0.984
cancel_b           0.906/0.982   0.906/0.982   0.906/0.982   0.906/0.982   0.906/0.982   0.906/0.982   0.906/0.982   0.977/0.984
cancel_c           0.732/0.983   0.732/0.983   0.732/0.983   0.732/0.983   0.732/0.983   0.732/0.983   0.732/0.983   0.969/0.983
conv_*             0.000/0.000 in every form: y is the conv output bit for bit, the state stays 0

What the probe found. The SSD form (ws_ssd, and seqs_pq0 up to 256 positions) took exp(cum[t] - cum[s]) from one fp32
running sum of A dt. The CPU emulation (a sequential fp32 sum; tests/test_mamba_cases_cpu.py) predicted a miss wherever a
head forgets (A dt = -480 per position) and then decays slowly, and the kernel, whose shuffle scan adds in a tree, showed
it: max(error / bound) of y / state over the lengths, before the fix,

                 emulation, T = 256    MI355X, ws_ssd = seqs_pq0
    threshold      1.013 / 0.989         1.013 / 0.991
    reset          1.943 / 1.788         1.106 / 2.129
    reset130      32.765 / 29.991       10.832 / 15.524
    tails_reset         -                1.151 / 3.592

with every other form, regime, stride, state-row permutation and step within the criterion. mamba2_ssd_kernel now keeps
cum in fp64 and takes the differences in fp64 before expf; the table above is the kernel after that change.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import mamba_cases as mc
from tests.mamba_cases import CASES, CD, D_SSM, DS, HD, LENS, MD, NH
from tests.test_gpu_hybrid import _args

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -77.0  # exact in bf16
STALE_RING, STALE_SSM = mc.STALE_RING, 3.0
BF = torch.bfloat16

UNIFORM = {"scan": None, "ws_pq1": 1, "ws_pq2": 2, "ws_pq4": 4, "ws_ssd": 0}  # form -> ZMI_OPT_SCAN_PQ
RAGGED = {"seqs_pq0": 0, "seqs_pq2": 2}
FORMS = list(UNIFORM) + list(RAGGED)
TABLE = {}  # (form, regime) -> [max y ratio, max state ratio]


def _L():
    from zonos_vibes_amd import _lib
    return _lib, _lib.lib()


@pytest.fixture(scope="module", autouse=True)
def results_table():
    """After the module's tests: max(error / bound) over everything they ran, per form and head regime (y / state)."""
    yield
    regs = [h for heads, _ in CASES.values() for h in heads]
    forms = [f for f in FORMS + ["step"] if any((f, h) in TABLE for h in regs)]
    print("\n" + " " * 16 + "".join(f"{f:>14}" for f in forms))
    for h in regs:
        cells = [TABLE.get((f, h)) for f in forms]
        print(f"{h:<16}" + "".join(f"{'-':>14}" if c is None else f"{c[0]:>8.3f}/{c[1]:<5.3f}" for c in cells))


def _with_option(pq, fn):
    if pq is None:
        return fn()
    L, lib = _L()
    old = lib.zmi_get_option(L.OPT_SCAN_PQ)
    lib.zmi_set_option(L.OPT_SCAN_PQ, pq)
    try:
        return fn()
    finally:
        lib.zmi_set_option(L.OPT_SCAN_PQ, old)


class Launch:
    """Buffers of one call: sentinels in y, in the padding of the strided buffers and in gz, stale state rows, a stale
    workspace, so that only what the call must write may change."""

    def __init__(self, params, rows, n_kv, ld_zx=MD["d_in_proj"], ldy=D_SSM, row_pos=None, row_kv=None, ssm0=None,
                 ring0=None, gz=False, gz_g=0):
        L, lib = _L()
        m = rows.shape[0]
        self.m, self.ldy = m, ldy
        self.pd = [t.to(DEV) for t in params]
        zx = torch.full((m, ld_zx), SENT, dtype=BF)
        zx[:, :MD["d_in_proj"]] = rows
        self.zx0, self.zx = zx, zx.to(DEV)
        self.ring = (torch.full((n_kv, 4, CD), STALE_RING, dtype=BF) if ring0 is None else ring0.clone()).to(DEV)
        self.ssm = (torch.full((n_kv, NH, HD, DS), STALE_SSM, dtype=BF) if ssm0 is None else ssm0.clone()).to(DEV)
        self.y = torch.full((m, ldy), SENT, dtype=BF, device=DEV)
        self.gz = torch.full((m, ldy), SENT, dtype=torch.float32, device=DEV) if gz else None
        self.rp = (torch.zeros(m, dtype=torch.int32) if row_pos is None
                   else torch.tensor(row_pos, dtype=torch.int32)).to(DEV)
        self.rk = None if row_kv is None else torch.tensor(row_kv, dtype=torch.int32, device=DEV)
        self.nb = int(lib.zmi_mamba2_scan_ws_bytes(m, D_SSM, NH))
        self.ws = torch.full((max(self.nb, 1),), 0xA5, dtype=torch.uint8, device=DEV)
        self.a = _args(L, MD, self.zx, *self.pd, self.ring, self.ssm, self.y, m, self.rp, self.rk)
        self.a.ld_zx, self.a.ldy = ld_zx, ldy
        if gz:
            self.a.gz, self.a.gz_g = self.gz.data_ptr(), gz_g

    def uniform(self, form, T):
        L, lib = _L()

        def go():
            if form == "scan":
                return lib.zmi_mamba2_scan(ctypes.byref(self.a), T, 0)
            return lib.zmi_mamba2_scan_ws(ctypes.byref(self.a), T, self.ws.data_ptr(), self.nb, 0)
        L.check(_with_option(UNIFORM[form], go), form)
        torch.cuda.synchronize()

    def ragged(self, form, seqs):
        L, lib = _L()
        sa = np.ascontiguousarray(np.asarray(seqs, dtype=np.int32).reshape(-1, 4))
        dev = torch.from_numpy(sa.ravel().copy()).to(DEV)
        L.check(_with_option(RAGGED[form], lambda: lib.zmi_mamba2_scan_seqs(
            ctypes.byref(self.a), dev.data_ptr(), len(sa), sa.ctypes.data, self.ws.data_ptr(), self.nb, 0)), form)
        torch.cuda.synchronize()

    def step(self):
        L, lib = _L()
        L.check(lib.zmi_mamba2_step(ctypes.byref(self.a), 0), "step")
        torch.cuda.synchronize()

    def padding_kept(self):
        """The strided buffers' padding columns and the input rows keep their bits."""
        ok = torch.equal(self.zx.cpu(), self.zx0) and bool((self.y[:, D_SSM:] == SENT).all())
        return ok and (self.gz is None or bool((self.gz[:, D_SSM:] == SENT).all()))


def _judge(form, case, tag, y, state, ring, ref):
    """One sequence's y [T, d_ssm], state and ring against its reference: prints and records max(error / bound) per
    head regime, returns the failures."""
    wy = mc.head_max(mc.ratio(y.cpu(), ref.y64, ref.y_abs))
    ws = mc.head_max(mc.ratio(state.cpu(), ref.state64, ref.state_abs))
    heads = CASES[case][0]
    print(f"{form} {case} {tag}: " + ", ".join(f"{h} y {a:.3f} state {b:.3f}" for h, a, b in zip(heads, wy, ws)))
    bad = []
    for h, a, b in zip(heads, wy, ws):
        t = TABLE.setdefault((form, h), [0.0, 0.0])
        t[0], t[1] = max(t[0], a), max(t[1], b)
        if not (a <= 1.0 and b <= 1.0):
            bad.append((form, case, tag, h, a, b))
    if not torch.equal(ring.cpu(), ref.ring):
        bad.append((form, case, tag, "ring"))
    if case == "conv" and not torch.equal(y.cpu(), ref.xc[:, :D_SSM]):
        bad.append((form, case, tag, "y is not the conv output bit for bit"))
    return bad


def _layout(lens):
    """Sequences of these lengths in one buffer, not in table order, with sentinel rows between: -> (q_row0 per
    sequence, rows in all, rows no sequence owns)."""
    order = sorted(range(len(lens)), key=lambda s: (s * 5) % len(lens))
    q0, row, free = [0] * len(lens), 0, []
    for k, s in enumerate(order):
        gap = 2 if k in (0, 3) else 0
        free += list(range(row, row + gap))
        q0[s] = row + gap
        row += gap + lens[s]
    return q0, row + 1, free + [row]


def _rows_of(m, parts):
    rows = torch.full((m, MD["d_in_proj"]), SENT, dtype=BF)
    for q, zx in parts:
        rows[q:q + zx.shape[0]] = zx
    return rows


# ---------------------------------------------------------------------------------------------- forms x lengths x regimes
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("form", list(UNIFORM))
def test_uniform_forms(form, case):
    """One sequence per launch, every length of LENS."""
    bad = []
    for T in LENS:
        i, ref = mc.build(case, T), mc.reference(case, T)
        ln = Launch(i.params, i.zx, 1)
        ln.uniform(form, T)
        bad += _judge(form, case, f"T={T}", ln.y, ln.ssm[0], ln.ring[0], ref)
    assert not bad, bad


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("form", list(RAGGED))
def test_ragged_forms(form, case):
    """Every length of LENS in one zmi_mamba2_scan_seqs launch (PQ 0: SSD up to 256 positions and the 4-workgroup scan
    for 257 in one pass); rows and state rows of no sequence keep their bits."""
    kv = [5, 0, 8, 2, 7, 3, 1]
    q0, m, free = _layout(LENS)
    ins = [mc.build(case, T) for T in LENS]
    ln = Launch(ins[0].params, _rows_of(m, [(q0[s], ins[s].zx) for s in range(len(LENS))]), 9)
    ln.ragged(form, [(q0[s], LENS[s], kv[s], 0) for s in range(len(LENS))])
    bad = []
    for s, T in enumerate(LENS):
        bad += _judge(form, case, f"T={T}", ln.y[q0[s]:q0[s] + T], ln.ssm[kv[s]], ln.ring[kv[s]], mc.reference(case, T))
    assert not bad, bad
    assert (ln.y[free] == SENT).all()
    for k in (4, 6):
        assert (ln.ssm[k] == STALE_SSM).all() and (ln.ring[k] == STALE_RING).all()


# ---------------------------------------------------------------------------------------------- strides, state rows
@pytest.mark.parametrize("form", FORMS)
def test_padded_strides(form):
    """ld_zx = d_in_proj + 5, ldy = d_ssm + 8: the padding holds a sentinel and keeps it; results as with tight rows."""
    lens = [33, 17]
    ins = [mc.build("mix", T) for T in lens]
    q0 = [0, 33] if form in UNIFORM else [18, 0]
    bad = []
    if form in UNIFORM:
        for s, T in enumerate(lens):
            ln = Launch(ins[s].params, ins[s].zx, 1, ld_zx=MD["d_in_proj"] + 5, ldy=D_SSM + 8)
            ln.uniform(form, T)
            bad += _judge(form, "mix", f"strided T={T}", ln.y[:, :D_SSM], ln.ssm[0], ln.ring[0], mc.reference("mix", T))
            assert ln.padding_kept()
    else:
        ln = Launch(ins[0].params, _rows_of(52, [(q0[s], ins[s].zx) for s in range(2)]), 2,
                    ld_zx=MD["d_in_proj"] + 5, ldy=D_SSM + 8)
        ln.ragged(form, [(q0[s], lens[s], 1 - s, 0) for s in range(2)])
        for s, T in enumerate(lens):
            bad += _judge(form, "mix", f"strided T={T}", ln.y[q0[s]:q0[s] + T, :D_SSM], ln.ssm[1 - s], ln.ring[1 - s],
                          mc.reference("mix", T))
        assert ln.padding_kept() and (ln.y[[17, 51]] == SENT).all()
    assert not bad, bad


@pytest.mark.parametrize("form", list(UNIFORM))
def test_permuted_state_rows(form):
    """Three sequences of 33 positions in one uniform launch, their state rows a permutation with holes of five: each
    lands in its own row, the unlisted rows keep their stale bits."""
    T, kv = 33, [3, 0, 4]
    ins = [mc.build("dt", T, 0, seed) for seed in range(3)]
    row_kv = [kv[s] for s in range(3) for _ in range(T)]
    ln = Launch(ins[0].params, torch.cat([i.zx for i in ins]), 5, row_kv=row_kv)
    ln.uniform(form, T)
    bad = []
    for s in range(3):
        bad += _judge(form, "dt", f"state row {kv[s]}", ln.y[s * T:(s + 1) * T], ln.ssm[kv[s]], ln.ring[kv[s]],
                      mc.reference("dt", T, 0, s))
    assert not bad, bad
    for k in (1, 2):
        assert (ln.ssm[k] == STALE_SSM).all() and (ln.ring[k] == STALE_RING).all()


# ---------------------------------------------------------------------------------------------- steps
STEP_POS = list(mc.STEP_POS)
GATE_REL = 2.0 ** -21  # expf within 2 ulp (2^-22 of e, at most that of 1 + e), then 1 + e, 1 / (.), z * (.): one
GATE_ABS = 2.0 ** -126  # rounding of 2^-24 each -> 2^-22 + 3 2^-24 < 2^-21; below 2^-126 the gate may underflow


def _step_rows(case):
    return [mc.step_probe(case, pos) for pos in STEP_POS]


@pytest.mark.parametrize("gz", ["no_gz", "gate", "gated_y"])
@pytest.mark.parametrize("case", list(CASES))
def test_steps_from_crafted_states(case, gz):
    """zmi_mamba2_step at positions 0, 1, 3, 4, 530 (slots below position 0 hold stale values that must read as zero)
    from states of mixed huge and tiny magnitudes, one inactive row, state rows permuted; without gz, with gz = gate
    and with gz = y * gate: gate against fp64 z sigmoid(z) within GATE_REL (+ GATE_ABS), the product one rounding more.
    Rows are strided (ld_zx = d_in_proj + 5, ldy = d_ssm + 8, gz with ldy) and the padding keeps its sentinel."""
    rows = _step_rows(case)
    kv = [4, 2, 0, 5, 1, 3]
    ssm0, ring0 = torch.empty(6, NH, HD, DS, dtype=BF), torch.empty(6, 4, CD, dtype=BF)
    for r, (i, n, st, rg) in enumerate(rows):
        ssm0[kv[r]], ring0[kv[r]] = st, rg
    ln = Launch(rows[0][0].params, torch.stack([i.zx[n] for i, n, _, _ in rows]), 6, ld_zx=MD["d_in_proj"] + 5,
                ldy=D_SSM + 8, row_pos=STEP_POS, row_kv=kv, ssm0=ssm0, ring0=ring0, gz=gz != "no_gz", gz_g=int(gz == "gated_y"))
    ln.step()
    bad = []
    for r, pos in enumerate(STEP_POS):
        i, n, st, rg = rows[r]
        if pos < 0:
            assert (ln.y[r] == SENT).all() and torch.equal(ln.ssm[kv[r]].cpu(), st) and torch.equal(ln.ring[kv[r]].cpu(), rg)
            assert ln.gz is None or (ln.gz[r] == SENT).all()
            continue
        ref = mc.ref64(i.zx[n:], *i.params, MD, state0=st, ring0=rg, pos0=pos)
        bad += _judge("step", case, f"pos={pos}", ln.y[r:r + 1, :D_SSM], ln.ssm[kv[r]], ln.ring[kv[r]], ref)
        if ln.gz is not None:
            z = i.zx[n, :D_SSM].double()
            want = z * torch.sigmoid(z)
            tol = GATE_REL * want.abs() + GATE_ABS
            if gz == "gated_y":
                yb = ln.y[r, :D_SSM].cpu().double()
                want, tol = yb * want, yb.abs() * tol + 2.0 ** -24 * (yb * want).abs() + GATE_ABS
            got = ln.gz[r, :D_SSM].cpu().double()
            worst = ((got - want).abs() / tol).max().item()
            print(f"step {case} pos={pos} {gz}: max(error / bound) {worst:.3f}")
            if not worst <= 1.0:
                bad.append(("step", case, pos, gz, worst))
    assert not bad, bad
    assert ln.padding_kept()


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("form", ["ws_ssd", "ws_pq4"])
def test_handover_from_prefill_to_steps(form, case):
    """A prefill of 33 positions, then 5 steps on the cache it left. Each link is held to ref64 under the criterion; the
    reference of a step starts from the bf16 state the library stored (the criterion's half ulp of a stored state is
    2^-9 of it, far above E of the next y, so a reference carried on roundings of its own could not be compared), and
    from the ring, which must be the reference's bits."""
    T, n = mc.HANDOVER
    i = mc.build(case, T + n)
    ln = Launch(i.params, i.zx[:T], 1)
    ln.uniform(form, T)
    bad = _judge(form, case, "handover prefill", ln.y, ln.ssm[0], ln.ring[0], mc.ref64(i.zx[:T], *i.params, MD))
    ssm, ring = ln.ssm.cpu(), ln.ring.cpu()
    for pos in range(T, T + n):
        st = Launch(i.params, i.zx[pos:pos + 1], 1, row_pos=[pos], ssm0=ssm, ring0=ring)
        st.step()
        ref = mc.ref64(i.zx[pos:pos + 1], *i.params, MD, state0=ssm[0], ring0=ring[0], pos0=pos)
        bad += _judge("step", case, f"after {form}, pos={pos}", st.y, st.ssm[0], st.ring[0], ref)
        ssm, ring = st.ssm.cpu(), st.ring.cpu()
    assert not bad, bad
