"""Every DAC kernel of zmi_dac.hip, called through the C ABI on its own, against a float64 reference at the tile
and signal edges (tests/dac_cases.py: cases, references, the derived error bound and the packed-layout emulation
that tests/test_dac_kernels_cpu.py checks on the CPU).

Every output buffer sits between canary rows; strided outputs also keep the canary in the phases they do not own.
Every launch form (ZMI_OPT_DAC_WIDE / _STAGE / _STAGE_MIN) must give the first form's bits in the whole buffer,
canaries included; the first form is the one compared with float64."""
import math

import pytest
import torch

from tests import dac_cases as dc
from zonos_vibes_amd.autoencoder import pack_conv, pack_conv_out, pack_conv_transpose

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = {torch.float16: (torch.int16, 0x5A5A), torch.float32: (torch.int32, 0x5A5A5A5A)}


class Buf:
    """An output [rows][cols] with canary rows before and after it."""

    def __init__(self, rows, cols, dtype):
        self.itype, self.pat = CANARY[dtype]
        self.rows, self.guard = rows, max(8, 64 // cols)
        self.full = torch.full((rows + 2 * self.guard, cols), self.pat, dtype=self.itype, device=DEV)
        self.mid = self.full[self.guard: self.guard + rows].view(dtype)

    def ptr(self):
        return self.full[self.guard:].data_ptr()  # valid for rows == 0 too

    def guards_intact(self):
        g = self.guard
        return bool((self.full[:g] == self.pat).all()) and bool((self.full[g + self.rows:] == self.pat).all())

    def rows_intact(self, rows):
        """The canary is still in these rows of the buffer proper (the phases a strided launch does not own)."""
        return bool((self.full[self.guard: self.guard + self.rows][rows] == self.pat).all())

    def untouched(self):
        return bool((self.full == self.pat).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(c, packed):
    return dict(x=c["x"].half().to(DEV), w=packed.to(DEV), bias=c["bias"].float().to(DEV),
                alpha=c["alpha"].float().to(DEV), skip=c["skip"].half().to(DEV) if "skip" in c else None)


class forms:
    """Run a launch under every form of dc.FORMS (or the given ones); the options are restored on exit."""

    def __init__(self, lib):
        from zonos_vibes_amd import _lib
        self.lib, self._lib = lib, _lib
        self.knobs = (_lib.OPT_DAC_WIDE, _lib.OPT_DAC_STAGE, _lib.OPT_DAC_STAGE_MIN)

    def __enter__(self):
        self.old = [self.lib.zmi_get_option(k) for k in self.knobs]
        return self

    def __exit__(self, *exc):
        for k, v in zip(self.knobs, self.old):
            self.lib.zmi_set_option(k, v)

    def run(self, launch, which=dc.FORMS):
        """launch() -> dict of Bufs. Returns the first form's; every other form must match it bit for bit."""
        first = None
        for form in which:
            for k, v in zip(self.knobs, self.old if form is None else form):
                self._lib.check(self.lib.zmi_set_option(k, v))
            outs = launch()
            if first is None:
                first = outs
            else:
                for name, b in outs.items():
                    assert torch.equal(b.full, first[name].full), (form, name)
        torch.cuda.synchronize()
        return first


def launch_conv(lib, d, t_in, c_in, c_out, taps, tap_step, in_off, n_out, out_stride, out_phase, t_out, epi, rc=0):
    """One zmi_dac_conv launch into fresh canaried buffers; epi: subset of skip / raw / snake / f32."""
    outs = {}
    for name, dtype in (("raw", torch.float16), ("snake", torch.float16), ("f32", torch.float32)):
        if name in epi:
            outs[name] = Buf(t_out, c_out, dtype)
    p = lambda n: outs[n].ptr() if n in outs else None  # noqa: E731
    got = lib.zmi_dac_conv(d["x"].data_ptr(), t_in, c_in, d["w"].data_ptr(), d["bias"].data_ptr(), c_out, taps,
                           tap_step, in_off, n_out, out_stride, out_phase, t_out,
                           d["skip"].data_ptr() if "skip" in epi else None, p("raw"), p("snake"),
                           d["alpha"].data_ptr(), p("f32"), _stream())
    assert (got != 0) == (rc != 0), (got, lib.zmi_last_error())
    return outs


def conv_failures(outs, rows, ref, M, K, alpha, label):
    """Compare the rows `rows` of each output with the float64 reference `ref` [len(rows)][c_out] (skip included
    where the launch adds it) under dc.bound; canaries everywhere else. Returns the list of failed checks (empty:
    the case passes) and the case's measured delta_sin (None without snake + f32)."""
    fails, dsin = [], None
    got = {}
    for name, b in outs.items():
        if not b.guards_intact():
            fails.append(f"{label}: {name} canary rows overwritten")
        other = torch.ones(b.rows, dtype=torch.bool)
        other[rows] = False
        if other.any() and not b.rows_intact(other.to(DEV)):
            fails.append(f"{label}: {name} rows of another phase overwritten")
        got[name] = b.mid.cpu()[rows]
    if "f32" in got:
        r = dc.worst_ratio(got["f32"], ref, dc.bound("f32", ref, M, K))
        if r > 1:
            fails.append(f"{label}: out_f32 at {r:.3g} x its bound")
    if "raw" in got:
        r = dc.worst_ratio(got["raw"], ref, dc.bound("raw", ref, M, K))
        if r > 1:
            fails.append(f"{label}: out_raw at {r:.3g} x its bound")
        if "f32" in got:
            bad, small = dc.raw_matches_f32(got["raw"], got["f32"])
            if bad or small > 1e-3:
                fails.append(f"{label}: out_raw != out_f32.half() in {bad} elements ({small:.2e} below 2^-14)")
    if "snake" in got:
        z = dc.snake64(ref, alpha)
        r = dc.worst_ratio(got["snake"], z, dc.bound("snake", z, M, K, alpha[None, :]))
        if r > 1:
            fails.append(f"{label}: out_snake at {r:.3g} x its bound")
        if "f32" in got and got["f32"].numel():
            dsin = dc.delta_sin_of(got["snake"], got["f32"], alpha)
            if dsin > dc.DELTA_SIN:
                fails.append(f"{label}: delta_sin {dsin:.3g} above the constant {dc.DELTA_SIN:.3g}")
    return fails, dsin


def _same_case(shape, T, *key):
    c_in, c_out, taps, dil = shape
    c = dc.conv_inputs(c_in, c_out, taps, T, T, dil, *key)
    ref = dc.ref_conv_same(c["x"], c["w"], c["bias"], dil)
    M = dc.ref_conv_same(c["x"].abs(), c["w"].abs(), c["bias"].abs(), dil)
    return c, ref, M


# ------------------------------------------------------------------------------------------------ zmi_dac_conv
@pytest.mark.parametrize("shape", dc.SAME_SHAPES, ids=str)
def test_conv_same(gpu_lib, shape):
    c_in, c_out, taps, dil = shape
    in_off = -dil * (taps - 1) // 2
    fails, dsin = [], -math.inf
    with forms(gpu_lib) as f:
        for T in dc.lengths_of(shape):
            c, ref, M = _same_case(shape, T)
            d = _dev(c, pack_conv(c["w"]))
            for epi in dc.epilogues_of(shape):
                outs = f.run(lambda: launch_conv(gpu_lib, d, T, c_in, c_out, taps, dil, in_off, T, 1, 0, T, epi))
                sk = "skip" in epi
                fl, ds = conv_failures(outs, torch.arange(T), ref + c["skip"] if sk else ref,
                                       M + c["skip"].abs() if sk else M, taps * c_in, c["alpha"], f"T={T} {epi}")
                fails += fl
                dsin = max(dsin, -math.inf if ds is None else ds)
    print(f"\nconv_same {shape}: delta_sin {dsin:.4g}")
    assert not fails, fails[:8]


GENERAL_SHAPES = ((64, 96, 7, 3), (32, 64, 7, 11), (64, 64, 1, 0))  # halo / staged, the tap-major ring, 1x1


@pytest.mark.parametrize("shape", GENERAL_SHAPES, ids=str)
def test_conv_general_indexing(gpu_lib, shape):
    """in_off past either end (rows outside the input read as zero), n_out != t_in, strided outputs."""
    c_in, c_out, taps, dil = shape
    t_in, n_out, K = 100, 130, taps * c_in
    fails = []
    with forms(gpu_lib) as f:
        for in_off in (5, -40):
            for out_stride, out_phase, t_out in ((1, 0, n_out), (3, 2, 3 * n_out), (3, 2, 3 * n_out + 7)):
                c = dc.conv_inputs(c_in, c_out, taps, t_in, t_out, dil, in_off)
                d = _dev(c, pack_conv(c["w"]))
                rows = torch.arange(n_out) * out_stride + out_phase
                ref = dc.ref_conv(c["x"], c["w"], c["bias"], dil, in_off, n_out) + c["skip"][rows]
                M = dc.ref_conv(c["x"].abs(), c["w"].abs(), c["bias"].abs(), dil, in_off, n_out) + c["skip"][rows].abs()
                epi = ("skip", "raw", "snake", "f32")
                outs = f.run(lambda: launch_conv(gpu_lib, d, t_in, c_in, c_out, taps, dil, in_off, n_out, out_stride,
                                                 out_phase, t_out, epi))
                fails += conv_failures(outs, rows, ref, M, K, c["alpha"],
                                       f"in_off={in_off} stride={out_stride} t_out={t_out}")[0]
    assert not fails, fails[:8]


def test_conv_rejected_arguments(gpu_lib):
    """n_out = 0 is a no-op; c_in % 32, c_out % 32 and an output row past t_out are errors with a message; none of
    them writes anything."""
    c = dc.conv_inputs(64, 64, 7, 100, 100, 1)
    d = _dev(c, pack_conv(c["w"]))
    epi = ("raw", "snake", "f32")
    outs = launch_conv(gpu_lib, d, 100, 64, 64, 7, 1, -3, 0, 1, 0, 100, epi)
    torch.cuda.synchronize()
    assert all(b.untouched() for b in outs.values())
    for kw, msg in ((dict(c_in=48), "c_in % 32"), (dict(c_out=40), "c_out must be a multiple of 32"),
                    (dict(n_out=34, out_stride=3, out_phase=1), "output bounds")):  # 33 * 3 + 1 = 100 = t_out
        a = dict(c_in=64, c_out=64, n_out=100, out_stride=1, out_phase=0)
        a.update(kw)
        outs = launch_conv(gpu_lib, d, 100, a["c_in"], a["c_out"], 7, 1, -3, a["n_out"], a["out_stride"],
                           a["out_phase"], 100, epi, rc=1)
        assert gpu_lib.zmi_last_error().decode() == "dac_conv: " + msg, (kw, gpu_lib.zmi_last_error())
        torch.cuda.synchronize()
        assert all(b.untouched() for b in outs.values()), kw


# ------------------------------------------------------------------------------------------------ zmi_dac_conv_t
def launch_conv_t(lib, d, t_in, c_in, c_out, stride, pad, epi):
    outs = {n: Buf(stride * t_in, c_out, torch.float16) for n in epi}
    p = lambda n: outs[n].ptr() if n in outs else None  # noqa: E731
    rc = lib.zmi_dac_conv_t(d["x"].data_ptr(), t_in, c_in, d["w"].data_ptr(), d["bias"].data_ptr(), c_out, stride,
                            pad, p("raw"), p("snake"), d["alpha"].data_ptr(), _stream())
    assert rc == 0, lib.zmi_last_error()
    return outs


@pytest.mark.parametrize("shape", dc.CONV_T_SHAPES, ids=str)
def test_conv_t(gpu_lib, shape):
    c_in, c_out, stride, pad = shape
    fails = []
    with forms(gpu_lib) as f:
        for t_in in dc.CONV_T_LENGTHS:
            c = dc.conv_t_inputs(c_in, c_out, stride, t_in, pad)
            d = _dev(c, pack_conv_transpose(c["w"], stride, pad))
            ref = dc.ref_conv_t(c["x"], c["w"], c["bias"], stride, pad)
            M = dc.ref_conv_t(c["x"].abs(), c["w"].abs(), c["bias"].abs(), stride, pad)
            for epi in (("raw",), ("snake",), ("raw", "snake")):
                outs = f.run(lambda: launch_conv_t(gpu_lib, d, t_in, c_in, c_out, stride, pad, epi))
                fails += conv_failures(outs, torch.arange(stride * t_in), ref, M, 2 * c_in, c["alpha"],
                                       f"t_in={t_in} {epi}")[0]
    assert not fails, fails[:8]


# ------------------------------------------------------------------------------------------------ negative control
def test_wrong_packing_is_reported(gpu_lib):
    """The comparison is sensitive on the real kernels: the same launches with wrong weight VALUES (same shapes,
    sizes and addresses) must fail it. k7: taps reversed; conv_t: phases built with (rho + pad + 1) % stride."""
    shape, T = (64, 96, 7, 3), 129
    c, ref, M = _same_case(shape, T)
    for w, should_fail in ((c["w"], False), (c["w"].flip(2), True)):
        packed = pack_conv(w)
        assert packed.shape == pack_conv(c["w"]).shape
        outs = launch_conv(gpu_lib, _dev(c, packed), T, 64, 96, 7, 3, -9, T, 1, 0, T, dc.DEFAULT_EPILOGUE)
        fails = conv_failures(outs, torch.arange(T), ref, M, 7 * 64, c["alpha"], "k7")[0]
        assert bool(fails) == should_fail, fails[:4]
        if should_fail:  # only values are wrong: every canary holds and all three outputs are off
            assert all("bound" in m or "delta_sin" in m for m in fails) and len(fails) >= 3, fails

    c_in, c_out, stride, pad, t_in = 64, 64, 8, 4, 33
    c = dc.conv_t_inputs(c_in, c_out, stride, t_in, pad)
    ref = dc.ref_conv_t(c["x"], c["w"], c["bias"], stride, pad)
    M = dc.ref_conv_t(c["x"].abs(), c["w"].abs(), c["bias"].abs(), stride, pad)
    right = pack_conv_transpose(c["w"], stride, pad)
    wrong = pack_conv_transpose(c["w"], stride, pad + 1)  # k0 = (rho + pad + 1) % stride
    assert wrong.shape == right.shape
    for packed, should_fail in ((right, False), (wrong, True)):
        outs = launch_conv_t(gpu_lib, _dev(c, packed), t_in, c_in, c_out, stride, pad, ("raw", "snake"))
        fails = conv_failures(outs, torch.arange(stride * t_in), ref, M, 2 * c_in, c["alpha"], "conv_t")[0]
        assert bool(fails) == should_fail, fails[:4]


# ------------------------------------------------------------------------------------------------ zmi_dac_conv_out
def _conv_out_case(c_in, t):
    c = dc.conv_inputs(c_in, 1, 7, t, 1, 2)
    w, b = pack_conv_out(c["w"], c["bias"])
    d = dict(x=c["x"].half().to(DEV), w=w.to(DEV), bias=b.to(DEV), alpha=torch.ones(32, device=DEV), skip=None)
    ref = dc.ref_conv_same(c["x"], c["w"], c["bias"], 1)[:, 0]
    M = dc.ref_conv_same(c["x"].abs(), c["w"].abs(), c["bias"].abs(), 1)[:, 0]
    return d, ref, M


def _conv_out(lib, d, t, c_in, q0=None, n=None, rc=0):
    whole = q0 is None
    out = Buf(t if whole else max(n, 0), 1, torch.float32)
    if whole:
        got = lib.zmi_dac_conv_out(d["x"].data_ptr(), t, c_in, d["w"].data_ptr(), d["bias"].data_ptr(), out.ptr(),
                                   _stream())
    else:
        got = lib.zmi_dac_conv_out_range(d["x"].data_ptr(), t, c_in, d["w"].data_ptr(), d["bias"].data_ptr(), q0, n,
                                         out.ptr(), _stream())
    assert (got != 0) == (rc != 0), (got, lib.zmi_last_error())
    return out


@pytest.mark.parametrize("c_in", (32, 96))
def test_conv_out_and_range(gpu_lib, c_in):
    dtanh = 0.0
    with forms(gpu_lib) as f:
        for t in (1, 3, 7, 129, 513):
            d, ref, M = _conv_out_case(c_in, t)
            whole = f.run(lambda: dict(out=_conv_out(gpu_lib, d, t, c_in)))["out"]
            assert whole.guards_intact(), t
            got = whole.mid.cpu()[:, 0]
            r = dc.worst_ratio(got, dc.tanh64(ref), dc.bound("tanh", ref, M, 7 * c_in))
            assert r <= 1, (t, r)
            # tanh's own error: against tanh64 of the fp32 value the same weights give through zmi_dac_conv
            y = launch_conv(gpu_lib, d, t, c_in, 32, 7, 1, -3, t, 1, 0, t, ("f32",))["f32"].mid.cpu()
            assert y[:, 1:].abs().max() == 0
            dtanh = max(dtanh, float((got.double() - dc.tanh64(y[:, 0])).abs().max()))
            for q0, n in ((0, t), (0, 1), (t - 1, 1), (1, t - 2), (127, 130), (5, 0)):
                if n < 0 or q0 + n > t:
                    continue  # not a range of this length (the ABI's precondition, checked below)
                part = f.run(lambda: dict(out=_conv_out(gpu_lib, d, t, c_in, q0, n)))["out"]
                assert part.guards_intact(), (t, q0, n)
                assert torch.equal(part.mid[:, 0], whole.mid[q0: q0 + n, 0]), (t, q0, n)
        for q0, n in ((-1, 2), (3, -1), (500, 14)):
            out = _conv_out(gpu_lib, d, 513, c_in, q0, n, rc=1)
            assert gpu_lib.zmi_last_error().decode() == "dac_conv_out_range: bounds", gpu_lib.zmi_last_error()
            torch.cuda.synchronize()
            assert out.untouched(), (q0, n)
    print(f"\nconv_out c_in={c_in}: delta_tanh {dtanh:.4g}")
    assert dtanh <= dc.DELTA_TANH, dtanh


# ------------------------------------------------------------------------------------------------ from_codes, im2col7
@pytest.mark.parametrize("T", (1, 2, 300))
def test_from_codes(gpu_lib, T):
    g = torch.Generator().manual_seed(T)
    cb = dc.f16_values((9, 1024, 8), g)
    pw = dc.f16_values((9, 1024, 8), g, 1 / math.sqrt(8))
    pb = dc.f16_values((9, 1024), g, 0.1)
    codes = torch.randint(0, 1024, (9, T), generator=g)
    if T == 1:  # one frame cannot hold both ends of a codebook: they alternate over the codebooks
        codes[:, 0] = torch.tensor([0, 1023] * 5)[:9]
    else:
        codes[:, 0], codes[:, -1] = 0, 1023
    lat = torch.stack([cb[i][codes[i]] for i in range(9)])                    # [9][T][8]
    ref = (torch.einsum("itj,icj->tc", lat, pw) + pb.sum(0)[None])            # [T][1024]
    M = torch.einsum("itj,icj->tc", lat.abs(), pw.abs()) + pb.abs().sum(0)[None]
    z = Buf(T, 1024, torch.float16)
    dv = [codes.to(DEV), cb.float().to(DEV), pw.float().to(DEV), pb.float().to(DEV)]
    rc = gpu_lib.zmi_dac_from_codes(dv[0].data_ptr(), T, dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), z.ptr(),
                                    _stream())
    assert rc == 0, gpu_lib.zmi_last_error()
    torch.cuda.synchronize()
    assert z.guards_intact()
    r = dc.worst_ratio(z.mid.cpu(), ref, dc.bound("raw", ref, M, 81))
    assert r <= 1, r


@pytest.mark.parametrize("T", (1, 2, 3, 4, 6, 7, 8, 255, 256, 257))
def test_im2col7(gpu_lib, T):
    wav = torch.randn(T, generator=torch.Generator().manual_seed(T))
    want = torch.zeros(T, 32, dtype=torch.float16)
    want[:, :7] = torch.nn.functional.pad(wav, (3, 3)).unfold(0, 7, 1).half()
    col = Buf(T, 32, torch.float16)
    wav_d = wav.to(DEV)
    rc = gpu_lib.zmi_dac_im2col7(wav_d.data_ptr(), T, col.ptr(), _stream())
    assert rc == 0, gpu_lib.zmi_last_error()
    torch.cuda.synchronize()
    assert col.guards_intact()
    got = col.mid.cpu()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert got[:, 7:].abs().max() == 0


# ------------------------------------------------------------------------------------------------ VQ ties
@pytest.mark.parametrize("P", (1, 3, 64, 256))
def test_vq_ties_go_to_the_lowest_index(gpu_lib, P):
    """Codebooks whose rows repeat with period P (raw rows, normalised rows and norms alike): every code is below P,
    and equals the oracle's on the P distinct rows wherever the oracle's margin between them is >= 1e-5."""
    from oracle.dac_cpu import OracleDAC
    T = 64
    g = torch.Generator().manual_seed(100 + P)
    w, j = {}, torch.arange(1024) % P
    for i in range(9):
        p = f"quantizer.quantizers.{i}."
        w[p + "in_proj.weight"] = torch.randn(8, 1024, 1, generator=g) / 32
        w[p + "in_proj.bias"] = 0.1 * torch.randn(8, generator=g)
        w[p + "codebook.weight"] = torch.randn(P, 8, generator=g)
        w[p + "out_proj.weight"] = torch.randn(1024, 8, 1, generator=g) / math.sqrt(8)
        w[p + "out_proj.bias"] = 0.1 * torch.randn(1024, generator=g)
    lat = torch.randn(T, 1024, generator=g)
    q = "quantizer.quantizers."
    stack = lambda name, f: torch.stack([f(w[f"{q}{i}.{name}"]) for i in range(9)]).contiguous().to(DEV)  # noqa: E731
    cb = stack("codebook.weight", lambda t: t[j])
    cbn = torch.nn.functional.normalize(cb, dim=-1).contiguous()
    cbn2 = cbn.pow(2).sum(-1).contiguous()
    assert torch.equal(cb[:, P:], cb[:, :-P]) and torch.equal(cbn[:, P:], cbn[:, :-P]) and \
        torch.equal(cbn2[:, P:], cbn2[:, :-P])
    codes = torch.full((9 + 2, T), -7, dtype=torch.int64, device=DEV)  # int64 [9][T] between two canary rows
    dv = [lat.to(DEV), stack("in_proj.weight", lambda t: t.reshape(8, -1)), stack("in_proj.bias", lambda t: t),
          stack("out_proj.weight", lambda t: t.reshape(-1, 8)), stack("out_proj.bias", lambda t: t)]
    rc = gpu_lib.zmi_dac_vq(dv[0].data_ptr(), T, dv[1].data_ptr(), dv[2].data_ptr(), cb.data_ptr(), cbn.data_ptr(),
                            cbn2.data_ptr(), dv[3].data_ptr(), dv[4].data_ptr(), codes[1:].data_ptr(), _stream())
    assert rc == 0, gpu_lib.zmi_last_error()
    torch.cuda.synchronize()
    codes = codes.cpu()
    assert (codes[0] == -7).all() and (codes[-1] == -7).all()
    got = codes[1:-1]
    assert got.min() >= 0 and got.max() < P, (int(got.min()), int(got.max()))
    if P > 1:
        ref, margins = OracleDAC(w).quantize(lat.t()[None])
        bad = dc.near_tie_violations(got, ref[0], margins[0], 1e-5)
        assert not bad, bad[:5]
        assert (margins >= 1e-5).float().mean() > 0.9  # the rule leaves most decisions constrained
