"""Cases, the fp64 reference and the criterion shared by the CPU and GPU probes of the attention forms
(zmi_attention_variant 0 / 1 / 2 / 3 / 5 / 4 / 8 and zmi_attention_prefill). Imports no GPU.

GEOMETRY. hd = 128; (hq, hkv) in (16, 4), (8, 4), (4, 1), (4, 4): GQA groups G = 4, 2, 4, 1. Every query row has a
KV row of its own. A build holds the q of four heads per KV head; a geometry of group G takes the first G of them, so
the caches of one hkv serve every G and the reference is computed once.

SCORE CONTROL. u1 = 1 on the even dims, u2 = 1 on the odd dims (every 32-dim MFMA fragment holds 16 of each). Key k of
a KV head is b_k u1 + c_k u2, query head g is alpha_g u1 + beta_g u2, so the scaled score is
(64 / sqrt(128)) (alpha_g b_k + beta_g c_k): two base profiles B1, B2 per (row, KV head), chosen key by key, and four
(alpha, beta) per profile, so that the heads of a group see different profiles over the same K bytes. All values are
rounded to bf16 and the reference works on what bf16 holds; the properties a case is named for are asserted on those
values by tests/test_attn_cases_cpu.py.

  profile       B1, B2 (scaled scores)                                   heads (alpha, beta)
  flat          K ~ N(0, 4) in both, q = 0: every score is 0             (0, 0) four times: the one profile whose
                                                                         heads cannot differ
  onehot        68 at key t1 / at key t2, 0 elsewhere                    (1,0) (0,1) (2,1) (1,2): peak t1, t2, t1, t2,
                                                                         at least 64 above every other key
  two_peaks     N(0,1) clipped to +-3, 12 at keys a and b (equal rows)   (1,0) (0,1) (1,.5) (.5,1)
  ramp_up/down  +-0.25 k', +-0.125 k', k' = k + 8 (KV head)              (1,0) (0,1) (1,1) (.5,.5)
  steps_up/down +-30 per 512-key block + N(0,1); N(0,1)                  (1,1) (1,.5) (1,-.5) (1,.25)
  offset_pos/neg +-300 + N(0,1); N(0,1)                                  the same
  rand1/4/12    N(0, sigma^2), independent                               (1,0) (0,1) (cos, sin)(30 deg) (60 deg)
  spike0_tail   7 at key 0, 0 elsewhere, in both                         (1,0) (0,1.25) (.5,.25) (1,1)

onehot's t1 rotates per row and KV head through {0, p, p - 1, the largest multiples of 8 / 16 / 32 / 128 / 512 that
are <= p, and those minus 1}, t2 is the next of them that is another key; two_peaks puts a and b into different
128-key chunks, and into different 512-key blocks from p = 512 on.

V KINDS. normal: N(0,1). tails: N(0,1), an eighth of the values x 256, an eighth x 2^-20. count: key k holds 1 or 2 in
dim k mod 128 and 0 elsewhere (each dim counts its own keys: a dropped or doubled key moves a dim by ~ 10 %). cancel:
(-1)^k (1 + 2^-6 N(0,1)), so |o| << sum p |V|.

STALE REGION. Past the row's position K is S (u1 + u2) with S so large that every head with alpha + beta > 0 scores
it at least 72 above its maximum over the live keys, so that one admitted stale key takes >= 1 - e^-60 of the
weight (flat has no such S: its scores are 0 whatever K is), and V alternates four bf16 NaN bit patterns with +-2^120.
A form that admits one key too many is off by everything.

THE REFERENCE. ref_rows evaluates softmax(q K^T / sqrt(128)) V over keys 0 .. p of the bf16 inputs in fp64: no
blocking, no internal rounding. Besides o64 it returns A_d = sum_k p_k |V_kd|, sabs = scale max_k sum_i |q_i K_ki| and
smag = max_k |s_k|.

THE CRITERION, elementwise, for every element:

    |got - o64| <= E A_d + 0.5 ulp_bf16(|o64| + E A_d)
    E = 2^-8 + 2 2^-24 ((hd + 2) sabs + smag) + 2^-21 + (n + 16) 2^-24,    n = p + 1

E is derived, not measured. 2^-8: every probability is rounded to bf16 before P.V (the reference implementation's
rounding point, oracle/attention_cpu.py); bf16 keeps 8 significant bits, so half an ulp is up to 2^-8 of the value.
2 2^-24 ((hd + 2) sabs + smag): an fp32 dot product of hd terms errs by at most (hd + 2) 2^-24 of its absolute sum
(the accumulation and the scaling), the subtraction of the maximum by 2^-24 smag; exp carries an absolute error of the
score into a relative one of the weight, once in the numerator and once in the normaliser. 2^-21: expf (2 ulp), the
reciprocal and the product. (n + 16) 2^-24: an fp32 sum of n terms in any order, and the rescaling per block. E = 2^-9
would be wrong: the bf16 rounding alone reaches 2^-8.

UNDERFLOW. The criterion is fp32's relative-error model; it has no term for a weight lost below 2^-126 (flushed or
subnormal in exp(s - M), in its bf16 rounding or in the rescaling of a block). Such a weight is below 2^-126 of the
largest one, live |V| is at most 2^16 (asserted), and a row has fewer than 2^14 keys, so everything lost is below
2^-96 in absolute terms. The cases keep every A_d that is not exactly 0 (a count dim without a key: got is exactly 0
too) above n 2^-100, where E A_d >= 2^-8 n 2^-100 exceeds what was lost by 2^-12 (clear_of_underflow, asserted on the
CPU).

EXACT CHECKS. onehot: every other key's weight is below e^-64, so the output row is V_t bit for bit (condition:
n e^-64 max|V| is below a quarter of the smallest half-ulp in V_t; asserted on the CPU). flat with count: every sum
is an exact integer and acc (1 / l) the same two roundings, so the row equals oracle.attention_cpu.attend_row bit for
bit. Position 0: the row is V_0.
"""
from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass

import numpy as np
import torch

HD = 128
SCALE = 1.0 / math.sqrt(HD)
KSCALE = 64.0 * SCALE  # scaled score per unit of alpha b + beta c
HEADS = ((16, 4), (8, 4), (4, 1), (4, 4))
POS_ALL = (0, 1, 7, 8, 15, 16, 31, 32, 33, 63, 64, 127, 128, 129, 255, 511, 512, 513, 1023, 1024, 1279)
POS_FAR = (1280, 1535, 1536, 2047, 2048)  # past the whole-query forms' reach, across the 8 / 16-chunk merge groups
ROWS = POS_ALL + POS_FAR + (-1,)          # one launch: every position and one inactive row
LONG_POS = 8320                           # 66 chunks
LONG_ROWS = (LONG_POS,) + ROWS            # the long row's launch: smax = 8328 for every row of it
LONG_CASES = ("rand4_count", "steps_up_normal")
PREFILL_SEQS = ((0, 40), (120, 16), (505, 16), (1016, 16), (1272, 16), (2040, 16))  # (pos0, len)
BF, F64 = torch.bfloat16, torch.float64
PEAK, GAP = 68.0, 64.0
STALE_GAP = 72.0  # 64 and ln(2^14) on top: ONE admitted stale key outweighs all live keys by e^60
VMAX = 2.0 ** 16

CASES = {  # name -> (profile, V kind)
    "flat_count": ("flat", "count"),
    "onehot_normal": ("onehot", "normal"),
    "onehot_tails": ("onehot", "tails"),
    "two_peaks_count": ("two_peaks", "count"),
    "ramp_up_count": ("ramp_up", "count"),
    "ramp_down_cancel": ("ramp_down", "cancel"),
    "steps_up_normal": ("steps_up", "normal"),
    "steps_down_tails": ("steps_down", "tails"),
    "offset_pos_cancel": ("offset_pos", "cancel"),
    "offset_neg_normal": ("offset_neg", "normal"),
    "rand1_cancel": ("rand1", "cancel"),
    "rand4_count": ("rand4", "count"),
    "rand12_tails": ("rand12", "tails"),
    "spike0_tail_normal": ("spike0_tail", "normal"),
}
_C30, _S30 = math.cos(math.pi / 6), math.sin(math.pi / 6)
_STEP_COEF = ((1, 1), (1, .5), (1, -.5), (1, .25))
COEF = {
    "flat": ((0, 0),) * 4,
    "onehot": ((1, 0), (0, 1), (2, 1), (1, 2)),
    "two_peaks": ((1, 0), (0, 1), (1, .5), (.5, 1)),
    "ramp_up": ((1, 0), (0, 1), (1, 1), (.5, .5)), "ramp_down": ((1, 0), (0, 1), (1, 1), (.5, .5)),
    "steps_up": _STEP_COEF, "steps_down": _STEP_COEF, "offset_pos": _STEP_COEF, "offset_neg": _STEP_COEF,
    "rand1": ((1, 0), (0, 1), (_C30, _S30), (_S30, _C30)),
    "spike0_tail": ((1, 0), (0, 1.25), (.5, .25), (1, 1)),
}
COEF["rand4"] = COEF["rand12"] = COEF["rand1"]
ONEHOT_PICK = (0, 1, 0, 1)  # which of t1, t2 head g peaks at
# stale V: four bf16 NaN bit patterns alternating with +-2^120
STALE_V = (0x7FC0, 0x7B80, 0xFFFF, 0xFB80, 0x7F81, 0x7B80, 0xFFC0, 0xFB80)


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def ulp_bf16(v):
    """Spacing of bf16 at |v| (fp64 tensor): 2^(floor(log2 |v|) - 7), the subnormal spacing 2^-133 below 2^-126."""
    v = v.abs()
    e = torch.frexp(v)[1].to(torch.int64) - 1
    e = torch.where(v > 0, e, torch.full_like(e, -126)).clamp_min(-126)
    return torch.ldexp(torch.ones_like(v), (e - 7).to(torch.int32))


def onehot_candidates(p):
    """The keys an onehot peak rotates through at position p."""
    out = [0, p, p - 1]
    for m in (8, 16, 32, 128, 512):
        out += [p // m * m, p // m * m - 1]
    return [min(max(t, 0), p) for t in out]


# ---------------------------------------------------------------------------------------------- builders
@dataclass
class Build:
    case: str
    hkv: int
    pos: tuple            # the position each KV row is live up to (-1: nothing is live)
    smax: int
    q: torch.Tensor       # [R, hkv, 4, 128] bf16: four query heads per KV head
    k: torch.Tensor       # [R, hkv, smax, 128] bf16
    v: torch.Tensor       # [R, hkv, smax, 128] bf16 (position-major; the kernels take its transpose)
    t: torch.Tensor       # [R, hkv, 2] onehot peaks t1, t2 / two_peaks a, b (None otherwise)

    @property
    def profile(self):
        return CASES[self.case][0]

    @property
    def vkind(self):
        return CASES[self.case][1]

    def q_rows(self, G):
        """q of a geometry with group G: [R, hkv * G * 128]."""
        return self.q[:, :, :G].reshape(len(self.pos), -1).contiguous()


def _base_profiles(profile, pos, anchor, hkv, S, g):
    """-> (B1, B2 [R, hkv, S] fp64 scaled scores, t [R, hkv, 2] or None)."""
    R = len(pos)
    k = torch.arange(S)[None, None, :].expand(R, hkv, S)
    n01 = lambda: torch.randn(R, hkv, S, generator=g, dtype=F64)
    zero = torch.zeros(R, hkv, S, dtype=F64)
    t = None
    if profile == "flat":
        return 2 * n01(), 2 * n01(), None
    if profile == "onehot":
        t = torch.zeros(R, hkv, 2, dtype=torch.int64)
        for r, a in enumerate(anchor):
            cand = onehot_candidates(max(a, 0))
            for h in range(hkv):
                i = (3 * r + 2 * h) % 13
                other = [cand[(i + j) % 13] for j in range(1, 13) if cand[(i + j) % 13] != cand[i]]
                t[r, h, 0], t[r, h, 1] = cand[i], other[0] if other else cand[i]  # t2: the next one that is another key
        return PEAK * (k == t[..., 0:1]), PEAK * (k == t[..., 1:2]), t
    if profile == "two_peaks":
        t = torch.zeros(R, hkv, 2, dtype=torch.int64)
        for r, p in enumerate(pos):
            for h in range(hkv):
                edge = 512 if p >= 512 else 128 if p >= 128 else 0
                a = (7 * r + 31 * h) % edge if edge else 0
                b = max(edge, p - (r + h) % 3) if edge else max(p, 0)
                t[r, h, 0], t[r, h, 1] = a, b
        peak = (k == t[..., 0:1]) | (k == t[..., 1:2])
        B1, B2 = n01().clamp(-3, 3), n01().clamp(-3, 3)
        return torch.where(peak, 12.0, B1), torch.where(peak, 12.0, B2), t
    if profile in ("ramp_up", "ramp_down"):
        sg = 1.0 if profile == "ramp_up" else -1.0
        kk = (k + 8 * torch.arange(hkv)[None, :, None]).to(F64)  # shifted per KV head: the same ramp from other bytes
        return sg * 0.25 * kk, sg * 0.125 * kk, None
    if profile in ("steps_up", "steps_down"):
        sg = 30.0 if profile == "steps_up" else -30.0
        return sg * (k // 512).to(F64) + n01(), n01(), None
    if profile in ("offset_pos", "offset_neg"):
        return (300.0 if profile == "offset_pos" else -300.0) + n01(), n01(), None
    if profile.startswith("rand"):
        sigma = float(profile[4:])
        return sigma * n01(), sigma * n01(), None
    if profile == "spike0_tail":
        sp = 7.0 * (k == 0)
        return sp + zero, sp + zero, None
    raise KeyError(profile)


def _values(kind, R, hkv, S, g):
    """Live V [R, hkv, S, 128] (fp32, rounded to bf16 by the caller)."""
    shape = (R, hkv, S, HD)
    if kind == "normal":
        return torch.randn(shape, generator=g)
    if kind == "tails":
        u = torch.rand(shape, generator=g)
        mul = torch.where(u < 0.125, 256.0, torch.where(u < 0.25, 2.0 ** -20, 1.0))
        return torch.randn(shape, generator=g) * mul
    if kind == "count":
        v = torch.zeros(shape)
        val = 1.0 + torch.randint(0, 2, (R, hkv, S, 1), generator=g).float()
        return v.scatter_(3, (torch.arange(S) % HD)[None, None, :, None].expand(R, hkv, S, 1), val)
    if kind == "cancel":
        sign = (1.0 - 2.0 * (torch.arange(S) % 2))[None, None, :, None]
        return sign * (1.0 + 2.0 ** -6 * torch.randn(shape, generator=g))
    raise KeyError(kind)


def scores64(q, k):
    """Scaled scores in fp64 of q [.., hkv, G, 128] on k [.., hkv, n, 128] -> [.., hkv, G, n]."""
    return torch.einsum("...gd,...nd->...gn", q.double(), k.double()) * SCALE


def build_rows(case, hkv, pos, anchor=None, smax=None):
    """KV rows live up to `pos` (one per entry) and the four query heads of every KV head; onehot peaks are chosen
    among the candidates of `anchor` (default pos)."""
    profile, vkind = CASES[case]
    pos = tuple(pos)
    anchor = pos if anchor is None else tuple(anchor)
    R = len(pos)
    S = (max(pos) + 1 + 7) // 8 * 8 if smax is None else smax
    g = torch.Generator().manual_seed(_seed("attn", case, hkv, pos, anchor))
    B1, B2, t = _base_profiles(profile, pos, anchor, hkv, S, g)
    b, c = (B1 / KSCALE).to(BF), (B2 / KSCALE).to(BF)
    coef = torch.tensor(COEF[profile], dtype=torch.float32).to(BF)  # [4, 2]
    q = torch.empty(R, hkv, 4, HD, dtype=BF)
    q[..., 0::2], q[..., 1::2] = coef[None, None, :, 0:1], coef[None, None, :, 1:2]
    live = torch.arange(S)[None, :] <= torch.tensor(pos)[:, None]  # [R, S]
    # stale K: S (u1 + u2), at least STALE_GAP (+ margin for its own bf16 rounding) above every head's live maximum
    s = KSCALE * (coef[:, 0].double()[None, None, :, None] * b.double()[:, :, None, :]
                  + coef[:, 1].double()[None, None, :, None] * c.double()[:, :, None, :])  # [R, hkv, 4, S]
    mx = s.masked_fill(~live[:, None, None, :], -math.inf).amax(-1)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    den = KSCALE * (coef[:, 0] + coef[:, 1]).double()[None, None, :]
    need = (mx + STALE_GAP + 2.0 + 0.02 * mx.abs()) / den.clamp_min(1e-9)
    need = torch.where(den > 0, need, torch.full_like(mx, 8.0))
    stale_k = need.amax(-1)
    stale_k = (stale_k + stale_k.abs() * 2.0 ** -6).to(BF)  # [R, hkv]
    lv = live[:, None, :]
    b = torch.where(lv, b, stale_k[..., None])
    c = torch.where(lv, c, stale_k[..., None])
    k = torch.empty(R, hkv, S, HD, dtype=BF)
    k[..., 0::2], k[..., 1::2] = b[..., None], c[..., None]
    v = _values(vkind, R, hkv, S, g).to(BF)
    pat = torch.tensor(STALE_V, dtype=torch.int32).to(torch.int16)
    idx = (torch.arange(S)[:, None] + 3 * torch.arange(HD)[None, :]) % 8
    v = torch.where(live[:, None, :, None], v, pat[idx].view(BF)[None, None])
    return Build(case, hkv, pos, S, q, k, v, t)


@functools.lru_cache(maxsize=2)
def build(case, hkv):
    """The single-query launch's rows: every position of ROWS."""
    return build_rows(case, hkv, ROWS)


@functools.lru_cache(maxsize=2)
def build_long(case, hkv=4):
    return build_rows(case, hkv, LONG_ROWS)


@functools.lru_cache(maxsize=2)
def build_prefill(case, hkv):
    """One KV row per sequence of PREFILL_SEQS, live up to the sequence's last position; onehot peaks lie at or
    below pos0, so every query of the sequence sees them."""
    last = [p0 + n - 1 for p0, n in PREFILL_SEQS]
    return build_rows(case, hkv, last, anchor=[p0 for p0, _ in PREFILL_SEQS])


def prefill_rows():
    """-> (seqs [(q_row0, len, kv_row, pos0)], n q rows, kv row and position of every q row (-1: a gap row)):
    q rows handed out in another order than the KV rows, one unowned gap row after each sequence."""
    order = [3, 0, 5, 1, 4, 2]
    seqs, row = [None] * len(PREFILL_SEQS), 0
    for s in order:
        p0, n = PREFILL_SEQS[s]
        seqs[s] = (row, n, s, p0)
        row += n + 1
    kv, pos = [0] * row, [-1] * row
    for q0, n, s, p0 in seqs:
        for i in range(n):
            kv[q0 + i], pos[q0 + i] = s, p0 + i
    return seqs, row, kv, pos


# ---------------------------------------------------------------------------------------------- the fp64 reference
@dataclass
class Ref:
    o64: torch.Tensor    # [R, hkv, G, 128]
    A: torch.Tensor      # [R, hkv, G, 128]: sum_k p_k |V_kd|
    sabs: torch.Tensor   # [R, hkv, G]
    smag: torch.Tensor   # [R, hkv, G]
    n: torch.Tensor      # [R] keys (0: inactive row)
    wmax: torch.Tensor   # [R, hkv, G] the largest probability


def ref_rows(q, k, v, kv_rows, pos):
    """q [R, hkv, G, 128]; query row r attends keys 0 .. pos[r] of KV row kv_rows[r] (pos < 0: skipped, zeros)."""
    R, hkv, G, _ = q.shape
    o, A = torch.zeros(R, hkv, G, HD, dtype=F64), torch.zeros(R, hkv, G, HD, dtype=F64)
    sabs, smag, wmax = (torch.zeros(R, hkv, G, dtype=F64) for _ in range(3))
    for r, p in enumerate(pos):
        if p < 0:
            continue
        K, V = k[kv_rows[r], :, :p + 1].double(), v[kv_rows[r], :, :p + 1].double()
        s = scores64(q[r], K)
        sabs[r] = torch.einsum("hgd,hnd->hgn", q[r].double().abs(), K.abs()).amax(-1) * SCALE
        smag[r] = s.abs().amax(-1)
        e = torch.exp(s - s.amax(-1, keepdim=True))
        pr = e / e.sum(-1, keepdim=True)
        wmax[r] = pr.amax(-1)
        o[r], A[r] = pr @ V, pr @ V.abs()
    return Ref(o, A, sabs, smag, torch.tensor([max(p, -1) + 1 for p in pos]), wmax)


def take(ref, rows):
    """The reference of a launch that holds these rows of it (in this order, repeats allowed)."""
    return Ref(*(getattr(ref, f)[list(rows)] for f in ("o64", "A", "sabs", "smag", "n", "wmax")))


def ref_of(bd):
    return ref_rows(bd.q, bd.k, bd.v, list(range(len(bd.pos))), bd.pos)


@functools.lru_cache(maxsize=2)
def reference(case, hkv):
    return ref_of(build(case, hkv))


@functools.lru_cache(maxsize=2)
def reference_long(case, hkv=4):
    return ref_of(build_long(case, hkv))


@functools.lru_cache(maxsize=2)
def reference_prefill(case, hkv):
    bd = build_prefill(case, hkv)
    _, _, kv, pos = prefill_rows()
    q = bd.q[[max(s, 0) for s in kv]]  # a q row carries its sequence's heads
    return ref_rows(q, bd.k, bd.v, kv, pos)


def E_of(ref):
    """[R, hkv, G, 1]: the criterion's relative term."""
    n = ref.n.to(F64)[:, None, None]
    e = 2.0 ** -8 + 2 * 2.0 ** -24 * ((HD + 2) * ref.sabs + ref.smag) + 2.0 ** -21 + (n + 16) * 2.0 ** -24
    return e[..., None]


def bound(ref):
    ea = E_of(ref) * ref.A
    return ea + 0.5 * ulp_bf16(ref.o64.abs() + ea)


def ratio(got, ref, G=None):
    """|got - o64| / bound of got [R, hkv * G * 128] (or [R, hkv, G, 128]) -> [R, hkv, G, 128]; inf where got is not
    finite; 0 on inactive rows (whose output is not the reference's to judge)."""
    R, hkv = ref.o64.shape[:2]
    got = got.to(F64).reshape(R, hkv, -1, HD)
    G = got.shape[2]
    r = (got - ref.o64[:, :, :G]).abs() / bound(ref)[:, :, :G]
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))
    return torch.where((ref.n > 0)[:, None, None, None], r, torch.zeros_like(r))


def clear_of_underflow(ref):
    """The UNDERFLOW condition of the module docstring."""
    n = ref.n.to(F64)[:, None, None, None]
    return bool(((ref.A == 0) | (ref.A >= n * 2.0 ** -100)).all())


def onehot_margin(bd, r, h, g):
    """(everything the other keys can add, a quarter of the smallest half-ulp in V_t) of row r, KV head h, head g."""
    p = bd.pos[r]
    t = int(bd.t[r, h, ONEHOT_PICK[g]])
    live = bd.v[r, h, :p + 1].double().abs()
    return (p + 1) * math.exp(-GAP) * live.max().item(), 0.25 * 0.5 * ulp_bf16(bd.v[r, h, t].double()).min().item()


# ---------------------------------------------------------------------------------------------- fp32 emulation
f32 = np.float32


def _bf_np(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(BF).to(torch.float32).numpy()


def emu_row(q, k, v, n, drop_last=False, admit_extra=False, no_acc_rescale=False, no_l_rescale=False, dup_edge=False,
            no_scale=False, exp_first=False):
    """The chunk order of zmi_attn_merge.h in float32 for one KV head: q [G, 128], k / v [>= n + 1, 128] bf16, n keys.
    Scores as oracle/attention_cpu.py takes them (the dot product in fp64, rounded to fp32, times the fp32 scale);
    per 512-key block M_j, e = exp(s - M_j), P = bf16(e); l per 128-key chunk (lanes L and L + 64, then a butterfly);
    P.V per 32-key tile (products of bf16 operands summed in fp64 and rounded to fp32 once: the MFMA's own order is
    not modelled), the tiles in order, the chunks in order, then fold_block. -> [G, 128] bf16 as fp64.
    Mutants: the last key dropped; one key past the position admitted; acc / l not rescaled by exp(M_{j-1} - M_j);
    the first key of chunk 1 counted twice; the scale omitted; exp taken before the maximum is subtracted."""
    n = n - 1 if drop_last else n + 1 if admit_extra else n
    G = q.shape[0]
    nb = (n + 511) // 512
    s = (k[:n].double() @ q.double().T).float().T.numpy()  # [G, n]
    if not no_scale:
        s = s * f32(SCALE)
    sp = np.full((G, nb * 512), -np.inf, f32)
    sp[:, :n] = s
    sp = sp.reshape(G, nb, 512)
    vp = np.zeros((nb * 512, HD), np.float64)
    vp[:n] = v[:n].double().numpy()
    vp = vp.reshape(nb, 16, 32, HD)
    acc, l, mprev = np.zeros((G, HD), f32), np.zeros(G, f32), np.zeros(G, f32)
    with np.errstate(all="ignore"):
        for j in range(nb):
            mb = sp[:, j].max(-1) if j == 0 else np.maximum(mprev, sp[:, j].max(-1))
            e = np.exp(sp[:, j]) / np.exp(mb)[:, None] if exp_first else np.exp(sp[:, j] - mb[:, None])
            e = np.where(np.isneginf(sp[:, j]), f32(0), e).astype(f32)
            if dup_edge and j == 0 and n > 128:
                e[:, 128] = e[:, 128] * f32(2)
            x = e.reshape(G, 4, 128)
            x = x[..., :64] + x[..., 64:]
            w = 64
            while w > 1:
                w //= 2
                x = x[..., :w] + x[..., w:2 * w]
            lch = x[..., 0]  # [G, 4]
            P = _bf_np(e).astype(np.float64).reshape(G, 16, 32)
            tiles = np.einsum("gtk,tkd->gtd", P, vp[j]).astype(f32).reshape(G, 4, 4, HD)
            ob, lb = None, None
            for cc in range(4):
                o = tiles[:, cc, 0]
                for w in range(1, 4):
                    o = o + tiles[:, cc, w]
                ob = o if cc == 0 else ob + o
                lb = lch[:, 0] if cc == 0 else lb + lch[:, cc]
            if j == 0:
                acc, l = ob, lb
            else:
                et = np.exp(mprev - mb).astype(f32)
                l = lb + (l if no_l_rescale else et * l)
                acc = (acc if no_acc_rescale else acc * et[:, None]) + ob
            mprev = mb
        out = acc * (f32(1) / l)[:, None]
    return torch.from_numpy(_bf_np(out)).to(F64)


def emu_rows(bd, G=4, rows=None, kv_shift=0, swap_heads=False, **mut):
    """emu_row over the rows of a build -> [R, hkv, G, 128] fp64 (inactive rows: zeros). Mutants: a query head reading
    the neighbouring KV head (kv_shift = 1); heads 0 and 1 of a group swapped on the way out."""
    R = len(bd.pos)
    out = torch.zeros(R, bd.hkv, G, HD, dtype=F64)
    for r in (range(R) if rows is None else rows):
        p = bd.pos[r]
        if p < 0:
            continue
        for h in range(bd.hkv):
            hk = (h + kv_shift) % bd.hkv
            o = emu_row(bd.q[r, h, :G], bd.k[r, hk], bd.v[r, hk], p + 1, **mut)
            out[r, h] = o[[1, 0] + list(range(2, G))] if swap_heads and G > 1 else o
    return out
