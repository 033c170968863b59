"""Cases, references and criteria shared by the CPU and GPU tests of the weight-streaming GEMV (zmi_gemv_impl.h):
every launch form, prologue and epilogue that zmi_gemv_launch builds.

Inputs are seeded and exactly representable in bf16, so the fp64 reference and the kernel start from the same numbers.
A case names the launch form it is for; the tests ask zmi_gemv_form (host only) and require exactly that form.

Two layers, so that a failure says which half is wrong:

  sums       ZMI_EPI_F32 against X64 @ W64^T on EVERY element, |out - ref| <= SUM_BOUND (|X| @ |W|^T): the bound of
             test_gemv_f32_sums_match_fp64, not re-tuned. For a prologue case the rows fed to that launch are those of
             the standalone kernel (zmi_layernorm_rows / zmi_add_layernorm / zmi_gated_rmsnorm) and the fused prologue
             must give the same bits through ZMI_EPI_F32 or ZMI_EPI_STORE, whichever is built for it.
  epilogues  from the kernel's OWN fp32 sums v (the F32 launch of the same packed weight and prologue). The library is
             compiled with -ffp-contract=off and rounds to bf16 to nearest-even, so a float32 CPU emulation is exact
             for everything except expf: STORE, RESIDUAL, LOGITS and QKV must match bit for bit, every element the
             epilogue does not own keeping its sentinel. SWIGLU: y = bf16(v_y), g = bf16(v_g), sg = bf16(silu(g)) with
             silu in fp64, out = bf16(y sg). Where silu64(g) lies within 2^-16 |value| of a bf16 rounding boundary
             (256x below bf16 rounding, far above any fp32 expf / divide error) sg may be either neighbour; out must
             equal bf16(y sg) for an allowed sg, and at most SWIGLU_SECOND_CAP of a case's elements may need the
             second neighbour (a condition, not a measurement: under 1 % of the reference's elements sit that close to a
             boundary, tests/test_gemv_cases_cpu.py).

zmi_layernorm_rows against an fp64 LayerNorm: every element within 1 bf16 ulp of the fp64 value, no share (fp32 two-pass
statistics can only flip a rounding; measured 0.50 ulp). The same rule holds zmi_add_layernorm and zmi_gated_rmsnorm to
addln_ref and grms_ref (tests/test_gpu_rownorm.py).
"""
from __future__ import annotations

import contextlib
import ctypes
import functools
import os
import re
import zlib
from dataclasses import dataclass

import torch

SUM_BOUND = 2e-6               # tests/test_gpu_kernels.py test_gemv_f32_sums_match_fp64
SWIGLU_NEAR = 2.0 ** -16       # relative distance of silu64(g) to a bf16 rounding boundary that allows either neighbour
SWIGLU_SECOND_CAP = 0.02       # share of a case's elements that may need the second neighbour
SWIGLU_REF_SHARE_MAX = 0.01    # the reference's own boundary share over the committed seeds (CPU test)
SENT16, SENT32 = 0x4B4B, 0x4B4B4B4B  # sentinel bits of bf16 / f32 buffers (finite values no case produces)
EPS = 1e-5

EPI = {"store": 0, "residual": 1, "qkv": 2, "swiglu": 3, "logits": 4, "f32": 5}
PRO = {"plain": 0, "ln": 1, "addln": 2, "grms": 3, "grms_g": 4}
BODY, ROWS, ROWS_DENSE = 0, 1, 2
SHAPE_OF_K = {512: (2, 4, 16), 1024: (4, 4, 16), 2048: (4, 8, 16), 4096: (4, 16, 16), 8192: (8, 16, 8)}  # W, NL, RT
OPT_GEMM_ROWS = 1
HEADS = ((16, 4, 32), (4, 1, 128), (8, 4, 64))  # (hq, hkv, hd) of the QKV cases
SMAX = 12                                        # KV-cache capacity of the QKV cases


def body(K, G, ntw, pro="plain"):
    """The gemv_body form (kind, G, W, NL, RT, ntw, pro) of a K."""
    W, NL, RT = SHAPE_OF_K[K]
    return (BODY, G, W, NL, RT, int(ntw), PRO[pro])


def rows(dense):
    """The K = 2048 many-row form (gemm_rows_kernel), on M8 or dense-pair MFMAs."""
    return (ROWS_DENSE if dense else ROWS, 8, 4, 8, 16, 0, 0)


@dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int                      # packed columns
    K: int
    form: tuple                 # the form this case is for
    pro: str = "plain"
    groups: int = 0
    rows_opt: int = 3           # ZMI_OPT_GEMM_ROWS during the launch (3 = the library's default)
    epis: tuple = ()            # epilogues checked against the emulations: store / residual / swiglu / logits
    heads: tuple = ()           # QKV: (hq, hkv, hd)
    n_valid: int | None = None  # default: N - 3
    rpw_gt1: bool = False       # the form query must report more than one row tile per workgroup

    @property
    def nv(self):
        return self.N - 3 if self.n_valid is None else self.n_valid

    @property
    def ldo(self):
        return self.N + 8

    @property
    def seed(self):
        return zlib.crc32(self.name.encode()) & 0x7FFFFFFF


def _cases():
    out = []
    three = ("store", "residual", "swiglu")
    # A-G: the single-group / two-group bodies. N = 72: 9 groups, so the G = 2 forms end on a half-empty block
    fams = {"A": (512, 1), "B": (1024, 1), "C": (2048, 1), "D": (2048, 2), "E": (4096, 1), "F": (8192, 1), "G": (8192, 2)}
    for fam, (K, G) in fams.items():
        RT = SHAPE_OF_K[K][2]
        g = 2 if G == 2 else 0
        for M in (1, RT - 1, RT, RT + 1, 2 * RT + 1):
            out.append(Case(f"{fam}-m{M}", M, 72, K, body(K, G, M <= RT), groups=g,
                            epis=three if M in (RT - 1, RT + 1) else ()))
        if K != 8192:  # zmi_layernorm_rows is built for K <= 4096 (no LayerNorm'd K = 8192 projection exists)
            for M in (3, RT + 1):
                out.append(Case(f"{fam}-ln-m{M}", M, 72, K, body(K, G, M <= RT, "ln"), pro="ln", groups=g))
        if K in (512, 2048):
            for M in (3, RT + 1):
                out.append(Case(f"{fam}-addln-m{M}", M, 72, K, body(K, G, M <= RT, "addln"), pro="addln", groups=g))
        if K in (1024, 4096):
            for M in (1, 2, 3, 4):
                for pro in ("grms", "grms_g"):
                    out.append(Case(f"{fam}-{pro}-m{M}", M, 72, K, body(K, G, True, pro), pro=pro))
    # H: the 4-group tile loop. 257 groups: the last block holds one
    for M in (17, 33, 64):
        out.append(Case(f"H-m{M}", M, 2056, 2048, body(2048, 4, False), epis=three if M == 33 else ()))
    # R / RD: the many-row form, M8 (ZMI_OPT_GEMM_ROWS 1) and dense pairs (3)
    for fam, opt in (("R", 1), ("RD", 3)):
        f = rows(opt == 3)
        out.append(Case(f"{fam}-65x72", 65, 72, 2048, f, rows_opt=opt, epis=three))              # rpw 1, partial column block
        out.append(Case(f"{fam}-81x8264", 81, 8264, 2048, f, rows_opt=opt, epis=three, rpw_gt1=True))  # six tiles, the last one row
        out.append(Case(f"{fam}-33x3072", 33, 3072, 2048, f, rows_opt=opt))                      # rows_form's boundary ...
        out.append(Case(f"{fam}-32x3072", 32, 3072, 2048, body(2048, 4, False), rows_opt=opt))    # ... and its other side
    # a tile loop with rpw > 1 in gemv_body
    out.append(Case("D-ln-33x9248", 33, 9248, 2048, body(2048, 2, False, "ln"), pro="ln", epis=three, rpw_gt1=True))
    # LOGITS: two heads, and the real nine; LayerNorm'd, single tile and tile loop
    for K in (512, 2048):
        for N, nv in ((2056, 2052), (9248, 9234)):
            G = 2 if (K == 2048 and N == 9248) else 1
            for M in (2, 17):
                out.append(Case(f"L-k{K}-n{N}-m{M}", M, N, K, body(K, G, M <= 16, "ln"), pro="ln", epis=("logits",),
                                n_valid=nv))
    # QKV on forms A, C, D and R / RD
    for hq, hkv, hd in HEADS:
        N = (hq + 2 * hkv) * hd
        for fam, K, G in (("A", 512, 1), ("C", 2048, 1), ("D", 2048, 2)):
            for M in (5, 17):
                out.append(Case(f"Q{fam}-{hq}x{hkv}-m{M}", M, N, K, body(K, G, M <= 16), groups=2 if G == 2 else 0,
                                heads=(hq, hkv, hd)))
        for fam, opt in (("R", 1), ("RD", 3)):
            out.append(Case(f"Q{fam}-{hq}x{hkv}-m65", 65, N, 2048, rows(opt == 3), rows_opt=opt, heads=(hq, hkv, hd)))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
SUMS_CASES = tuple(c for c in CASES if c.pro in ("plain", "ln") and not c.heads and "logits" not in c.epis)
ADDLN_CASES = tuple(c for c in CASES if c.pro == "addln")
GRMS_CASES = tuple(c for c in CASES if c.pro == "grms")  # each runs with its grms_g twin
EPILOGUE_CASES = tuple((c, e) for c in CASES for e in c.epis if e != "logits")
LOGITS_CASES = tuple(c for c in CASES if "logits" in c.epis)
QKV_CASES = tuple(c for c in CASES if c.heads)
# refused: GRMS_G past one tile (and past its 4 rows), LayerNorm'd K = 8192 rows past the LDS image
REFUSED = (("grms_g", 17, 72, 1024, 0), ("grms_g", 5, 72, 4096, 0), ("ln", 8, 72, 8192, 0), ("plain", 3, 72, 1024, 2))


def built_forms():
    """Every (kind, G, W, NL, RT, ntw) zmi_gemv_launch builds, read from the list the dispatch itself expands
    (ZMI_GEMV_SHAPES in zmi_gemv_impl.h) x single tile / tile loop, the 4-group plain tile loop and the two many-row
    kernels: a form added there without a case here fails the coverage test."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zonos_vibes_amd", "csrc",
                            "zmi_gemv_impl.h")).read()
    line = re.search(r"#define ZMI_GEMV_SHAPES\(X\)(.*)", src).group(1)
    shapes = [tuple(int(v) for v in m) for m in re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", line)]
    assert len(shapes) >= 7
    forms = {(BODY, *s, ntw) for s in shapes for ntw in (0, 1)}
    return forms | {(BODY, 4, 4, 8, 16, 0), (ROWS, 8, 4, 8, 16, 0), (ROWS_DENSE, 8, 4, 8, 16, 0)}


# ------------------------------------------------------------------------------------------------ the form query
@contextlib.contextmanager
def _rows_opt(value):
    from tests.helpers import zmi_option
    with zmi_option(OPT_GEMM_ROWS, value):
        yield


def make_args(L, M, N, K, pro="plain", groups=0, ldo=None, n_valid=None, heads=(), ptr=None):
    """ZmiGemvArgs of a launch; `ptr` maps field names to device pointers (a dummy non-null value where the argument
    checks want a pointer: enough for zmi_gemv_form, which reads no pointer's target)."""
    ptr = dict(ptr or {})
    a = L.GemvArgs()
    a.W, a.X = ptr.get("W", 64), ptr.get("X", 64)
    a.M, a.N, a.K, a.ldx, a.groups, a.eps = M, N, K, K, groups, EPS
    a.out, a.ldo, a.n_valid = ptr.get("out", 64), N if ldo is None else ldo, N if n_valid is None else n_valid
    if pro != "plain":
        a.ln_w = ptr.get("ln_w", 64)
    if pro in ("ln", "addln"):
        a.ln_b = ptr.get("ln_b", 64)
    if pro in ("addln", "grms", "grms_g"):
        a.pro, a.aux, a.ld_aux = PRO[pro], ptr.get("aux", 64), ptr.get("ld_aux", K)
        a.res_out = ptr.get("res_out")
    if heads:
        a.hq, a.hkv, a.hd = heads
        a.smax = SMAX
        for k in ("row_kv", "row_pos", "k_cache", "v_cache", "rope"):
            setattr(a, k, ptr.get(k, 64))
    return a


def query_form(L, a, epi, rows_opt=3):
    """(kind, G, W, NL, RT, ntw, pro), rpw as zmi_gemv_form reports them, or None where the library refuses."""
    f = L.GemvForm()
    with _rows_opt(rows_opt):
        rc = L.lib().zmi_gemv_form(ctypes.byref(a), EPI[epi], ctypes.byref(f))
    if rc != 0:
        return None
    return (f.kind, f.G, f.W, f.NL, f.RT, f.ntw, f.pro), f.rpw


def case_epis(c):
    """The epilogues a case launches through its form (what the form query is asked about)."""
    if c.heads:
        return ("qkv",)
    if c.pro in ("addln", "grms", "grms_g"):
        return ("store",)
    return ("f32",) + c.epis


def case_args(L, c, epi, ptr=None):
    ldo = c.N // 2 + 8 if epi == "swiglu" else c.ldo
    return make_args(L, c.M, c.N, c.K, c.pro, c.groups, ldo, c.nv, c.heads, ptr)


# ------------------------------------------------------------------------------------------------ inputs
def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1).mul(scale).to(torch.bfloat16)


@functools.lru_cache(maxsize=8)
def _weight(N, K, swiglu, unit_rows):
    # SWIGLU: sums of std ~2 (uniform rows of variance 1 / 3, or LayerNorm'd rows of variance ~1): the gates of a case's
    # few hundred to few hundred thousand elements then span about +-8
    scale = 6.0 / (K ** 0.5) / (3 ** 0.5 if unit_rows else 1.0) if swiglu else 0.05
    return rnd(N, K, scale=scale, seed=(zlib.crc32(f"w{N}x{K}".encode()) & 0x7FFFFFFF) + (7 if swiglu else 1))


def weight(c, swiglu=False):
    """[N][K] bf16, shared by the cases of a shape (read only). SWIGLU: fc1 = value rows then gate rows, scaled so the
    gates span about +-8."""
    return _weight(c.N, c.K, bool(swiglu), bool(swiglu) and c.pro == "ln")


def swiglu_rows(N):
    """ZMI_PACK_SWIGLU: the fc1 row behind each packed column: group g holds value rows 4g .. 4g + 3, then their gates
    F + 4g .. F + 4g + 3 (F = N / 2)."""
    n = torch.arange(N)
    g, c_ = n // 8, n % 8
    return torch.where(c_ < 4, 4 * g + c_, N // 2 + 4 * g + c_ - 4)


def rows_in(c, scale=1.0):
    return rnd(c.M, c.K, scale=scale, seed=c.seed + 2)


def ln_params(c):
    return (rnd(c.K, scale=0.2, seed=c.seed + 3) + 1).contiguous(), rnd(c.K, scale=0.05, seed=c.seed + 4)


def residual_in(c):
    """Non-zero, several times the linear term (std sqrt(K) 0.05 / 3)."""
    return rnd(c.M, c.ldo, scale=4.0 * max(1.0, c.K ** 0.5 * 0.05 / 3), seed=c.seed + 5)


def sentinel16(*shape, device="cpu"):
    return torch.full(shape, SENT16, dtype=torch.int16, device=device).view(torch.bfloat16)


def sentinel32(*shape, device="cpu"):
    return torch.full(shape, SENT32, dtype=torch.int32, device=device).view(torch.float32)


def same_bits(a, b):
    iv = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def qkv_inputs(c):
    """row_pos with 0, SMAX - 1 and one inactive row; row_kv a non-identity permutation; the rope table of SMAX
    positions [SMAX][hd / 2][2] (cos, sin) fp32."""
    hq, hkv, hd = c.heads
    g = torch.Generator().manual_seed(c.seed + 6)
    pos = torch.randint(0, SMAX, (c.M,), generator=g, dtype=torch.int32)
    pos[0], pos[1], pos[2] = 0, SMAX - 1, -1
    if c.M > 16:
        pos[16] = SMAX - 1  # the second tile's first row
    kv = torch.roll(torch.arange(c.M, dtype=torch.int32), 3)
    kv[[0, 1]] = kv[[1, 0]]
    assert sorted(kv.tolist()) == list(range(c.M)) and (kv != torch.arange(c.M)).any()
    ang = torch.arange(SMAX, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(hd // 2, dtype=torch.float64) * 2 / hd))
    rope = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).float().contiguous()
    return pos, kv, rope


# ------------------------------------------------------------------------------------------------ sums
def sums_ref(X, W):
    """fp64 reference and bound of the fp32 sums (on the tensors' device)."""
    X64, W64 = X.double(), W.double()
    return X64 @ W64.t(), (X64.abs() @ W64.abs().t()) * SUM_BOUND + 1e-30


def sums_bad(out, X, W):
    """Elements of the F32 output outside the bound (out [M][>= N], compared on [:, :N])."""
    ref, bound = sums_ref(X, W)
    return ((out[:, : ref.shape[1]].double() - ref).abs() > bound).nonzero()


def bf16_ulp(x64):
    """The bf16 ulp (8 significant bits) at an fp64 value."""
    e = torch.frexp(x64.abs().clamp_min(2.0 ** -120))[1]
    return torch.ldexp(torch.ones_like(x64), e - 8)


def layernorm_ref(X, w, b):
    """fp64 LayerNorm of bf16 rows and its tolerance: 1 bf16 ulp of each value."""
    x, w64, b64 = X.double(), w.double(), b.double()
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    ref = (x - mean) / torch.sqrt(var + EPS) * w64 + b64
    return ref, bf16_ulp(ref)


def addln_ref(X, R, w, b):
    """fp64 add + LayerNorm (layer_norm_fn, prenorm): layernorm_ref on the fp64 sum of the two bf16 inputs."""
    return layernorm_ref(X.double() + R.double(), w, b)


def grms_ref(Y, Z, w):
    """fp64 RMSNormGated (norm_before_gate=False): g = y z sigmoid(z), out = g / sqrt(mean(g^2) + eps) w, and its
    tolerance: 1 bf16 ulp of each value."""
    z = Z.double()
    g = Y.double() * z * torch.sigmoid(z)
    ref = g / torch.sqrt((g * g).mean(dim=-1, keepdim=True) + EPS) * w.double()
    return ref, bf16_ulp(ref)


# ------------------------------------------------------------------------------------------------ epilogue emulations
def bfround(x32):
    return x32.to(torch.bfloat16).to(torch.float32)


def emulate_store(v):
    return v.to(torch.bfloat16)


def emulate_residual(v, res, round_linear=True):
    """bf16(f32(res) + f32(bf16(v))); round_linear=False is the deliberately wrong form (the linear term not rounded)."""
    lin = bfround(v) if round_linear else v
    return (res.float() + lin).to(torch.bfloat16)


def expect_rows(init, val, n_valid):
    """A [M][ldo] buffer after an epilogue that owns columns < n_valid of every row."""
    out = init.clone()
    out[:, :n_valid] = val[:, :n_valid]
    return out


def emulate_logits(v, n_valid, init, stride=1026):
    """f32(bf16(v)) at [(m 9 + n / 1026) 1026 + n % 1026] of a flat sentinel buffer; stride != 1026 is wrong on purpose."""
    out = init.clone()
    M = v.shape[0]
    n = torch.arange(n_valid)
    for m in range(M):
        out[(m * 9 + n // stride) * stride + n % stride] = bfround(v[m, :n_valid])
    return out


def emulate_qkv(v, heads, pos, kv, rope, q0, k0, vt0, rope_v=False, k_shift=0):
    """q [M][ldo], K cache [R][hkv][SMAX][hd] and transposed V cache [R][hkv][hd][SMAX] after the QKV epilogue, from
    their initial (sentinel) contents: bf16(v) pairs rotated in fp32 on q and k only (two products, one add / sub).
    rope_v / k_shift are the deliberately wrong forms."""
    hq, hkv, hd = heads
    qc, kc = hq * hd, hkv * hd
    x = bfround(v)
    q, kk, vt = q0.clone(), k0.clone(), vt0.clone()
    smax = kk.shape[2]

    def rot(seg, cs):
        x0, x1, co, si = seg[..., 0::2], seg[..., 1::2], cs[:, 0], cs[:, 1]
        a, b, c_, d = x0 * co, x1 * si, x1 * co, x0 * si
        return torch.stack([a - b, c_ + d], dim=-1).flatten(-2)

    for m in range(v.shape[0]):
        p = int(pos[m])
        if p < 0 or p >= smax:
            continue
        cs = rope[p]
        vv = x[m, qc + kc: qc + 2 * kc].view(hkv, hd)
        q[m, :qc] = rot(x[m, :qc].view(hq, hd), cs).flatten().to(torch.bfloat16)
        kk[int(kv[m]), :, (p + k_shift) % smax] = rot(x[m, qc: qc + kc].view(hkv, hd), cs).to(torch.bfloat16)
        vt[int(kv[m]), :, :, p] = (rot(vv, cs) if rope_v else vv).to(torch.bfloat16)
    return q, kk, vt


def swiglu_split(v):
    """The value / gate sums of a ZMI_PACK_SWIGLU weight's F32 launch: packed group g holds value columns 4g .. 4g + 3
    then their gates."""
    M, N = v.shape
    vg = v.reshape(M, N // 8, 8)
    return vg[..., :4].reshape(M, N // 2), vg[..., 4:].reshape(M, N // 2)


def bf16_neighbours(s):
    """Of fp64 values: their bf16 rounding (nearest-even), the other bf16 neighbour, and whether the value lies within
    SWIGLU_NEAR |value| of the boundary between the two."""
    ulp = bf16_ulp(s)
    q = s / ulp
    lo, hi, r = torch.floor(q), torch.ceil(q), torch.round(q)
    near = (lo != hi) & (((q - lo) - 0.5).abs() * ulp <= SWIGLU_NEAR * s.abs())
    return r * ulp, (lo + hi - r) * ulp, near


def swiglu_check(out, v, swap=False):
    """(ok, second, near) masks [M][F] of a SWIGLU output against the criterion of the module docstring. swap: read the
    halves the wrong way round (discrimination test only)."""
    vy, vgate = swiglu_split(v)
    if swap:
        vy, vgate = vgate, vy
    y, g = bfround(vy), bfround(vgate).double()
    sg0, sg1, near = bf16_neighbours(g / (1.0 + torch.exp(-g)))
    o0, o1 = (y * sg0.float()).to(torch.bfloat16), (y * sg1.float()).to(torch.bfloat16)
    ob = out.view(torch.int16)
    first = ob == o0.view(torch.int16)
    second = near & ~first & (ob == o1.view(torch.int16))
    return first | second, second, near


def emulate_swiglu(v, swap=False):
    """A float32 restatement of the kernel's SWIGLU epilogue (expf in float32); swap = value / gate halves swapped."""
    vy, vgate = swiglu_split(v)
    if swap:
        vy, vgate = vgate, vy
    y, g = bfround(vy), bfround(vgate)
    return (y * bfround(g / (1.0 + torch.exp(-g)))).to(torch.bfloat16)
