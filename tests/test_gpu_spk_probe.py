"""The speaker encoder's kernels against the fp64 references of tests/spk_cases.py, at the model's widths and on
crafted regimes: zmi_spk_conv2d (spk_conv_kernel<2 | 4>, up to 512 -> 512: 16 K steps, 8 column blocks, the 71 KiB LDS
form), zmi_spk_stem and zmi_spk_simam (C = 8 .. 2048, own sums and the conv's tile sums, 1 .. 257 chunks), and the
ragged-lane forms at C = 256.

Cases, references and the derived bounds are those of tests/spk_cases.py; tests/test_spk_cases_cpu.py holds float32
emulations that meet them and mutants that do not. Every output and the workspace start as NaNs of a known payload
between guard zones of the same payload; every test requires status 0, every element within its bound (bit equality
where the regime is exact), the guard zones untouched, the inputs unchanged and a second launch with the same bits, and
prints max(error / bound) per shape and regime. The module prints the maximum per kernel family at its end.
"""
import math

import pytest
import torch

from tests import spk_cases as sc
from tests.spk_cases import F64, REGIMES
from tests.test_gpu_speaker_lanes import F32, H16, _bits, _check_lanes, _nan16, _nan32, _pack, _sent16, _sent32
from zonos_vibes_amd import _lib
from zonos_vibes_amd.autoencoder import _blocked

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 512   # elements of sentinel on either side of a buffer a kernel writes
TABLE = {}    # (family, regime) -> max(error / bound) over the module


def _ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module", autouse=True)
def results_table():
    yield
    print()
    for (family, regime), v in sorted(TABLE.items()):
        print(f"{family:<16}{regime:<16}{v:.3f}")


def _note(family, regime, v):
    TABLE[(family, regime)] = max(TABLE.get((family, regime), 0.0), v)


class Guarded:
    """n elements of fp16 / fp32 sentinel between two guard zones of it."""

    def __init__(self, n, half):
        self.n, self.sent = n, H16 if half else F32
        self.buf = (_sent16 if half else _sent32)(n + 2 * GUARD)
        self.view = self.buf[GUARD:GUARD + n]

    def ptr(self):
        return self.view.data_ptr()

    def guards_intact(self):
        b = _bits(self.buf)
        return bool((b[:GUARD] == self.sent).all()) and bool((b[GUARD + self.n:] == self.sent).all())

    def all_written(self):
        return bool((_bits(self.view) != self.sent).all())


# ---------------------------------------------------------------------------------------------- conv
class ConvOnDevice:
    """A case's operands on the device, in the layouts the kernel reads."""

    def __init__(self, c):
        (self.H, self.W, self.ci), (self.co, _, self.k, _) = c.x.shape, c.w.shape
        self.stride, self.relu = c.stride, int(c.relu)
        self.ho, self.wo = sc.out_dim(self.H, self.k, c.stride), sc.out_dim(self.W, self.k, c.stride)
        self.x = c.x.half().to(DEV).contiguous()
        self.x0 = self.x.clone()
        self.w = _blocked(c.w.float().to(DEV).permute(2, 3, 0, 1).reshape(self.k * self.k, self.co, self.ci))
        self.scale, self.shift = c.scale.float().to(DEV), c.shift.float().to(DEV)

    def launch(self, lib, want_psum=True):
        """-> (stored [Ho][Wo][Co] fp16, psum [tiles][Co] fp32 or None), on the CPU; guards and inputs checked."""
        tiles = lib.zmi_spk_conv2d_tiles(self.H, self.W, self.k, self.stride)
        assert tiles == sc.n_tiles(self.H, self.W, self.k, self.stride)
        y = Guarded(self.ho * self.wo * self.co, True)
        ps = Guarded(tiles * self.co, False) if want_psum else None
        rc = lib.zmi_spk_conv2d(self.x.data_ptr(), self.H, self.W, self.ci, self.w.data_ptr(), self.scale.data_ptr(),
                                self.shift.data_ptr(), self.co, self.k, self.stride, self.relu, y.ptr(),
                                ps.ptr() if ps else None, 0)
        assert rc == 0, lib.zmi_last_error().decode()
        torch.cuda.synchronize()
        assert y.guards_intact() and (ps is None or ps.guards_intact()), "written outside the output"
        assert ps is None or ps.all_written(), "a psum row keeps its canary"
        assert torch.equal(self.x, self.x0)
        self.y_dev, self.ps_dev = y.view, ps.view if ps else None
        return (y.view.reshape(self.ho, self.wo, self.co).cpu(),
                ps.view.reshape(tiles, self.co).cpu() if ps else None)


def _judge_conv(c, stored, psum):
    worst = sc.worst_ratio(stored, c.ref.y, c.ref.bound)
    if c.exact and not torch.equal(stored, c.ref.y.half()):  # as values: no NaN, and a zero of either sign is zero
        worst = math.inf
    st = stored.to(F64)
    want = sc.tile_sums(st)
    wp = sc.worst_ratio(psum, want, sc.psum_bound(st).clamp_min(1e-300))
    if c.exact and not torch.equal(psum.to(F64), want):
        wp = math.inf
    return worst, wp


@pytest.mark.parametrize("shape_regime", [(s, r) for s in sc.CONV_SHAPES for r in sc.conv_regimes_of(s)],
                         ids=lambda v: f"{_ids(v[0])}-{v[1]}")
def test_conv2d(gpu_lib, shape_regime):
    """Every H x W of the shape: the stored values within the bound (the reference's own fp16 values on integers and
    border), psum within 128 U32 sum |stored| of the sums of the values that launch stored (exactly them on integer
    data), the same bits from a second launch, and the same stored bits without psum."""
    shape, regime = shape_regime
    bad = []
    for hw in sc.conv_hw_of(shape):
        c = sc.conv_case(shape, hw, regime)
        d = ConvOnDevice(c)
        stored, psum = d.launch(gpu_lib)
        worst, wp = _judge_conv(c, stored, psum)
        print(f"conv {_ids(shape)} {_ids(hw)} {regime}: y {worst:.3f} psum {wp:.3f}")
        _note("conv", regime, worst)
        _note("conv psum", regime, wp)
        if not (worst <= 1.0 and wp <= 1.0):
            bad.append((hw, worst, wp))
        again, psum2 = d.launch(gpu_lib)
        alone, _ = d.launch(gpu_lib, want_psum=False)
        if not (torch.equal(_bits(stored), _bits(again)) and torch.equal(_bits(psum), _bits(psum2))):
            bad.append((hw, "a second launch gives other bits"))
        if not torch.equal(_bits(stored), _bits(alone)):
            bad.append((hw, "other bits without psum"))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("regime", sc.STEM_REGIMES)
@pytest.mark.parametrize("hw", sc.STEM_HW, ids=_ids)
def test_stem(gpu_lib, hw, regime):
    (H, W), co = hw, sc.STEM_CO
    c = sc.stem_case(hw, regime)
    x = c.x.half().reshape(H, W).to(DEV).contiguous()
    w = c.w.half().reshape(co, 9).t().contiguous().to(DEV)  # [9][Co]
    scale, shift = c.scale.float().to(DEV), c.shift.float().to(DEV)
    x0, outs = x.clone(), []
    for _ in range(2):
        y = Guarded(H * W * co, True)
        rc = gpu_lib.zmi_spk_stem(x.data_ptr(), H, W, w.data_ptr(), scale.data_ptr(), shift.data_ptr(), co, y.ptr(), 0)
        assert rc == 0, gpu_lib.zmi_last_error().decode()
        torch.cuda.synchronize()
        assert y.guards_intact() and torch.equal(x, x0)
        outs.append(y.view.reshape(H, W, co).cpu())
    worst = sc.worst_ratio(outs[0], c.ref.y, c.ref.bound)
    print(f"stem {_ids(hw)} {regime}: {worst:.3f}")
    _note("stem", regime, worst)
    assert worst <= 1.0
    assert not c.exact or torch.equal(outs[0], c.ref.y.half())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


# ---------------------------------------------------------------------------------------------- SimAM
def _simam(lib, x, res, H, W, C, psum, n_psum):
    """One zmi_spk_simam launch on device operands -> the stored [P][C] on the CPU; workspace and output guarded."""
    ws = Guarded(lib.zmi_spk_simam_ws_floats(H, W, C), False)
    y = Guarded(H * W * C, True)
    rc = lib.zmi_spk_simam(x.data_ptr(), res.data_ptr(), H, W, C, _lib.ptr(psum), n_psum, ws.ptr(), y.ptr(), 0)
    assert rc == 0, lib.zmi_last_error().decode()
    torch.cuda.synchronize()
    assert y.guards_intact() and ws.guards_intact(), "written outside the output / the workspace"
    return y.view.reshape(H * W, C).cpu()


def _simam_case(lib, shape, with_psum):
    H, W, C = shape
    if with_psum:  # x: what the library's conv stored; the reference starts from those values
        d = ConvOnDevice(sc.psum_conv(shape))
        stored, psum = d.launch(lib)
        x_dev, ps_dev, n_psum = d.y_dev.clone(), d.ps_dev.clone(), psum.shape[0]
        x = stored.to(F64).reshape(H * W, C)
        crafted = sc.simam_x(shape)
        for i, n in enumerate(REGIMES):
            if n in ("const", "offset64", "offset16"):
                assert torch.equal(x[:, i::6], crafted[:, i::6]), "the identity channels are the crafted ones"
    else:
        x = sc.simam_x(shape)
        x_dev, ps_dev, n_psum = x.half().to(DEV).contiguous(), None, 0
    x0, bad = x_dev.clone(), []
    n_s = sc.simam_n_s(H * W, C, n_psum)
    for kind in sc.RESIDUALS:
        res = sc.residual(kind, x, shape)
        r_dev = res.half().to(DEV).contiguous()
        got = _simam(lib, x_dev, r_dev, H, W, C, ps_dev, n_psum)
        worst = sc.regime_max(sc.simam_ratio(got, sc.simam_ref(x, res), n_s))
        tag = "psum" if with_psum else "own sums"
        print(f"simam {_ids(shape)} {tag} {kind}: " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))
        for n, v in worst.items():
            _note("simam " + tag, n, v)
        if not max(worst.values()) <= 1.0:
            bad.append((kind, worst))
        again = _simam(lib, x_dev, r_dev, H, W, C, ps_dev, n_psum)
        if not torch.equal(_bits(got), _bits(again)):
            bad.append((kind, "a second launch gives other bits"))
        assert torch.equal(x_dev, x0) and torch.equal(r_dev, res.half().to(DEV))
    return bad


@pytest.mark.parametrize("shape", sc.SIMAM_SHAPES, ids=_ids)
def test_simam(gpu_lib, shape):
    """SimAM from its own sums, both residual kinds, all six regimes in one launch."""
    bad = _simam_case(gpu_lib, shape, False)
    assert not bad, bad


@pytest.mark.parametrize("shape", sc.PSUM_SHAPES, ids=_ids)
def test_simam_with_conv_tile_sums(gpu_lib, shape):
    """The path the model takes: x and psum from one zmi_spk_conv2d launch (the diagonal conv of spk_cases.psum_conv),
    n_psum its tile count."""
    bad = _simam_case(gpu_lib, shape, True)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- lanes at C = 256
def test_lanes_equal_single_launches_at_256(gpu_lib):
    """Three lanes of widths 43, 17 and 2 through zmi_spk_conv2d_lanes (256 -> 256, 3 x 3) and zmi_spk_simam_lanes
    (with the conv's tile sums, and with its own): each lane has the bits of its single launch, and every gap between
    the lanes keeps its sentinel."""
    lib, H, C, widths = gpu_lib, 3, 256, (43, 17, 2)
    g = torch.Generator().manual_seed(51)
    w = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
    wb = _blocked(w.to(DEV).permute(2, 3, 0, 1).reshape(9, C, C))
    scale, shift = (0.8 + 0.4 * torch.rand(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    xs = [torch.randn(H, wd, C, generator=g).half().to(DEV) for wd in widths]
    rss = [torch.randn(H, wd, C, generator=g).half().to(DEV) for wd in widths]
    wmax, L = max(widths), _lib.SpkLanes.of(widths)

    ys, pss = [], []
    for x, wd in zip(xs, widths):
        y, ps = _sent16(H * wd * C), _sent32(lib.zmi_spk_conv2d_tiles(H, wd, 3, 1) * C)
        _lib.check(lib.zmi_spk_conv2d(x.data_ptr(), H, wd, C, wb.data_ptr(), scale.data_ptr(), shift.data_ptr(), C, 3,
                                      1, 0, y.data_ptr(), ps.data_ptr(), 0), "spk_conv2d")
        ys.append(y)
        pss.append(ps)
    ls_a, ls_p = H * wmax * C, lib.zmi_spk_conv2d_tiles(H, wmax, 3, 1) * C
    ybuf, pbuf = _sent16(len(widths) * ls_a), _sent32(len(widths) * ls_p)
    _lib.check(lib.zmi_spk_conv2d_lanes(_pack(xs, ls_a, _nan16).data_ptr(), H, L, C, wb.data_ptr(), scale.data_ptr(),
                                        shift.data_ptr(), C, 3, 1, 0, ybuf.data_ptr(), pbuf.data_ptr(), ls_a, ls_a,
                                        ls_p, 0), "spk_conv2d_lanes")
    torch.cuda.synchronize()
    _check_lanes(ybuf, ls_a, ys, H16)
    _check_lanes(pbuf, ls_p, pss, F32)
    assert all(torch.isfinite(y.float()).all() for y in ys)

    ls_w = lib.zmi_spk_simam_ws_floats(H, wmax, C)
    rbuf = _pack(rss, ls_a, _nan16)
    rows = (_lib.c_int * len(widths))(*[p.numel() // C for p in pss])
    for with_psum in (True, False):
        singles = []
        for y, ps, rs, wd in zip(ys, pss, rss, widths):
            out, ws = _sent16(y.numel()), _nan32(lib.zmi_spk_simam_ws_floats(H, wd, C))
            _lib.check(lib.zmi_spk_simam(y.data_ptr(), rs.data_ptr(), H, wd, C, ps.data_ptr() if with_psum else None,
                                         ps.numel() // C if with_psum else 0, ws.data_ptr(), out.data_ptr(), 0),
                       "spk_simam")
            singles.append(out)
        out, ws = _sent16(len(widths) * ls_a), _nan32(len(widths) * ls_w)
        _lib.check(lib.zmi_spk_simam_lanes(ybuf.data_ptr(), rbuf.data_ptr(), H, L, C,
                                           pbuf.data_ptr() if with_psum else None, rows if with_psum else None,
                                           ws.data_ptr(), out.data_ptr(), ls_a, ls_a, ls_p, ls_w, ls_a, 0),
                   "spk_simam_lanes")
        torch.cuda.synchronize()
        _check_lanes(out, ls_a, singles, H16)
        assert all(torch.isfinite(s.float()).all() for s in singles)
