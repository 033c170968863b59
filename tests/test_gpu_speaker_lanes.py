"""Speaker embeddings for a batch of clips: ragged lanes through the trunk (csrc/zmi_spk.hip *_lanes,
SpeakerEmbeddingLDA.embed_features_batch, Zonos.make_speaker_embeddings).

Every comparison is bit equality with the single-clip path, which tests/test_gpu_speaker.py ties to the reference. The
kernel tests lay the lanes out at a stride of exactly the widest lane's extent, fill the inputs with NaN outside each
lane's own [H][w_l][C] (a padding test against the widest W would read one) and the outputs with a NaN of a known
payload, and require that payload everywhere a lane's own extent does not reach. Buffers are compared as integers.
"""
import math

import pytest
import torch

from zonos_vibes_amd import _lib
from zonos_vibes_amd.autoencoder import _blocked
from zonos_vibes_amd.speaker import SpeakerEmbeddingLDA, SpeakerEncoderConfig, plan_lanes

pytestmark = pytest.mark.gpu
DEV = "cuda"
TINY = SpeakerEncoderConfig(in_planes=32, num_blocks=(2, 2, 2, 1), acoustic_dim=24)
H16, F32 = 0x7E2A, 0x7FC0BEEF  # sentinels: NaN bit patterns no kernel produces
WIDTHS = (37, 5, 21, 37)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _sent16(n):
    return torch.full((n,), H16, dtype=torch.int16, device=DEV).view(torch.float16)


def _sent32(n):
    return torch.full((n,), F32, dtype=torch.int32, device=DEV).view(torch.float32)


def _pack(parts, stride, fill):
    """Flat buffer of len(parts) lanes at `stride` elements, lane l holding parts[l] (flattened), `fill` elsewhere."""
    buf = fill(len(parts) * stride)
    for l, t in enumerate(parts):
        buf[l * stride: l * stride + t.numel()] = t.reshape(-1).to(DEV)
    return buf


def _nan16(n):
    return torch.full((n,), float("nan"), dtype=torch.float16, device=DEV)


def _nan32(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)


def _check_lanes(buf, stride, singles, sentinel):
    """Lane l of buf equals singles[l] bit for bit and everything else still holds the sentinel."""
    own = torch.zeros(buf.numel(), dtype=torch.bool, device=DEV)
    for l, t in enumerate(singles):
        own[l * stride: l * stride + t.numel()] = True
        assert torch.equal(_bits(buf[l * stride: l * stride + t.numel()]), _bits(t.reshape(-1))), f"lane {l}"
    assert bool((_bits(buf)[~own] == sentinel).all()), "written outside a lane's own extent"


def _out(n, k, stride):
    return (n + 2 * (k // 2) - k) // stride + 1


def _conv_single(lib, x, wb, scale, shift, co, k, stride, psum=True):
    H, W, ci = x.shape
    y = _sent16(_out(H, k, stride) * _out(W, k, stride) * co)
    ps = _sent32(lib.zmi_spk_conv2d_tiles(H, W, k, stride) * co) if psum else None
    _lib.check(lib.zmi_spk_conv2d(x.data_ptr(), H, W, ci, wb.data_ptr(), scale.data_ptr(), shift.data_ptr(), co, k,
                                  stride, 0, y.data_ptr(), _lib.ptr(ps), 0), "spk_conv2d")
    return y, ps


def test_max_lanes_matches_binding(gpu_lib):
    assert gpu_lib.zmi_spk_max_lanes() == _lib.SPK_MAX_LANES == 32


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cio", [(32, 32), (64, 32), (32, 64)], ids=lambda v: f"{v[0]}to{v[1]}")
def test_conv2d_lanes(gpu_lib, cio, stride, k):
    """Partial tiles in both directions, a lane narrower than one tile, lanes of one, two and three tile columns in one
    grid, two lanes of one width and different data, two K blocks, both N tiles."""
    (ci, co), H, lib = cio, 24, gpu_lib
    xs = [_ints((H, w, ci), -3, 3, 100 + l).half().to(DEV) for l, w in enumerate(WIDTHS)]
    assert not torch.equal(xs[0], xs[3])
    w = _ints((co, ci, k, k), -2, 2, 2)
    wb = _blocked(w.to(DEV).permute(2, 3, 0, 1).reshape(k * k, co, ci))
    one, zero = torch.ones(co, device=DEV), torch.zeros(co, device=DEV)
    singles = [_conv_single(lib, x, wb, one, zero, co, k, stride) for x in xs]
    wmax, ho = max(WIDTHS), _out(H, k, stride)
    ls_x, ls_y = H * wmax * ci, ho * _out(wmax, k, stride) * co
    ls_p = lib.zmi_spk_conv2d_tiles(H, wmax, k, stride) * co
    L = _lib.SpkLanes.of(WIDTHS)
    xbuf = _pack(xs, ls_x, _nan16)
    ys = []
    for with_psum in (True, False):
        y, ps = _sent16(len(WIDTHS) * ls_y), _sent32(len(WIDTHS) * ls_p) if with_psum else None
        _lib.check(lib.zmi_spk_conv2d_lanes(xbuf.data_ptr(), H, L, ci, wb.data_ptr(), one.data_ptr(), zero.data_ptr(),
                                            co, k, stride, 0, y.data_ptr(), _lib.ptr(ps), ls_x, ls_y, ls_p, 0),
                   "spk_conv2d_lanes")
        _check_lanes(y, ls_y, [s[0] for s in singles], H16)
        if with_psum:  # rows beyond a lane's own tile count are outside its extent: still the sentinel
            _check_lanes(ps, ls_p, [s[1] for s in singles], F32)
        ys.append(y)
    assert torch.equal(_bits(ys[0]), _bits(ys[1]))
    assert not torch.isnan(singles[1][0]).any()


def test_conv2d_lanes_output_width_one(gpu_lib):
    """A lane whose output is one column wide after stride 2 (w = 2 -> 1, w = 1 -> 1) beside a two-tile lane."""
    H, ci, co, widths, lib = 24, 32, 32, (37, 2, 1), gpu_lib
    xs = [_ints((H, w, ci), -3, 3, 200 + l).half().to(DEV) for l, w in enumerate(widths)]
    wb = _blocked(_ints((co, ci, 3, 3), -2, 2, 3).to(DEV).permute(2, 3, 0, 1).reshape(9, co, ci))
    one, zero = torch.ones(co, device=DEV), torch.zeros(co, device=DEV)
    singles = [_conv_single(lib, x, wb, one, zero, co, 3, 2) for x in xs]
    ls_x, ls_y, ls_p = H * 37 * ci, 12 * 19 * co, lib.zmi_spk_conv2d_tiles(H, 37, 3, 2) * co
    y, ps = _sent16(3 * ls_y), _sent32(3 * ls_p)
    _lib.check(lib.zmi_spk_conv2d_lanes(_pack(xs, ls_x, _nan16).data_ptr(), H, _lib.SpkLanes.of(widths), ci,
                                        wb.data_ptr(), one.data_ptr(), zero.data_ptr(), co, 3, 2, 0, y.data_ptr(),
                                        ps.data_ptr(), ls_x, ls_y, ls_p, 0), "spk_conv2d_lanes")
    _check_lanes(y, ls_y, [s[0] for s in singles], H16)
    _check_lanes(ps, ls_p, [s[1] for s in singles], F32)


def test_stem_lanes(gpu_lib):
    H, co, lib = 24, 32, gpu_lib
    xs = [_ints((H, w), -3, 3, 300 + l).half().to(DEV) for l, w in enumerate(WIDTHS)]
    wd = _ints((co, 1, 3, 3), -2, 2, 7).reshape(co, 9).t().contiguous().half().to(DEV)
    g = torch.Generator().manual_seed(8)
    scale, shift = (0.8 + 0.4 * torch.rand(co, generator=g)).to(DEV), torch.randn(co, generator=g).to(DEV)
    singles = []
    for x, w in zip(xs, WIDTHS):
        y = _sent16(H * w * co)
        _lib.check(lib.zmi_spk_stem(x.data_ptr(), H, w, wd.data_ptr(), scale.data_ptr(), shift.data_ptr(), co,
                                    y.data_ptr(), 0), "spk_stem")
        singles.append(y)
    ls_x, ls_y = H * max(WIDTHS), H * max(WIDTHS) * co
    y = _sent16(len(WIDTHS) * ls_y)
    _lib.check(lib.zmi_spk_stem_lanes(_pack(xs, ls_x, _nan16).data_ptr(), H, _lib.SpkLanes.of(WIDTHS), wd.data_ptr(),
                                      scale.data_ptr(), shift.data_ptr(), co, y.data_ptr(), ls_x, ls_y, 0),
               "spk_stem_lanes")
    _check_lanes(y, ls_y, singles, H16)
    assert not torch.isnan(singles[1]).any() and float(singles[1].float().abs().max()) > 0


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("with_psum", [True, False], ids=["conv_psum", "own_sums"])
@pytest.mark.parametrize("shape", [(3, (5, 2, 5), 32), (24, (37, 5, 21), 64)], ids=["3x5_2_5", "24x37_5_21"])
def test_simam_lanes(gpu_lib, shape, with_psum, in_place):
    """x is a conv's stored output and psum that conv's per-tile sums, per lane; residual random."""
    (H, widths, C), lib = shape, gpu_lib
    g = torch.Generator().manual_seed(31)
    w = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
    wb = _blocked(w.to(DEV).permute(2, 3, 0, 1).reshape(9, C, C))
    scale, shift = (0.8 + 0.4 * torch.rand(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    xs, pss, rss = [], [], []
    for w in widths:
        x0 = torch.randn(H, w, C, generator=g).half().to(DEV)
        y, ps = _conv_single(lib, x0, wb, scale, shift, C, 3, 1)
        xs.append(y)
        pss.append(ps)
        rss.append(torch.randn(H, w, C, generator=g).half().to(DEV))
    assert not torch.equal(xs[0], xs[2])
    wmax = max(widths)
    singles = []
    for x, ps, rs, w in zip(xs, pss, rss, widths):
        ws = _nan32(lib.zmi_spk_simam_ws_floats(H, w, C))
        xin = x.clone()
        y = xin if in_place else _sent16(x.numel())
        _lib.check(lib.zmi_spk_simam(xin.data_ptr(), rs.data_ptr(), H, w, C, ps.data_ptr() if with_psum else None,
                                     ps.numel() // C if with_psum else 0, ws.data_ptr(), y.data_ptr(), 0), "spk_simam")
        singles.append(y)
    ls_a, ls_p = H * wmax * C, max(p.numel() for p in pss)
    ls_w = lib.zmi_spk_simam_ws_floats(H, wmax, C)
    xbuf, rbuf, pbuf = _pack(xs, ls_a, _nan16), _pack(rss, ls_a, _nan16), _pack(pss, ls_p, _nan32)
    ws = _nan32(len(widths) * ls_w)
    ybuf = xbuf if in_place else _sent16(len(widths) * ls_a)
    rows = (_lib.c_int * len(widths))(*[p.numel() // C for p in pss])
    _lib.check(lib.zmi_spk_simam_lanes(xbuf.data_ptr(), rbuf.data_ptr(), H, _lib.SpkLanes.of(widths), C,
                                       pbuf.data_ptr() if with_psum else None, rows if with_psum else None,
                                       ws.data_ptr(), ybuf.data_ptr(), ls_a, ls_a, ls_p, ls_w, ls_a, 0),
               "spk_simam_lanes")
    if in_place:  # outside a lane's extent the input's NaN (0x7E00) stays
        _check_lanes(ybuf, ls_a, singles, 0x7E00)
    else:
        _check_lanes(ybuf, ls_a, singles, H16)
    assert all(torch.isfinite(s.float()).all() for s in singles)


# ------------------------------------------------------------------------------------- models
@pytest.fixture(scope="module")
def encoders():
    made = {}

    def get(tag):
        if tag not in made:
            made[tag] = SpeakerEmbeddingLDA(DEV, seed=0, config=TINY if tag == "tiny" else SpeakerEncoderConfig())
        return made[tag]
    return get


FRAMES = (37, 203, 5, 64, 37)


@pytest.fixture(scope="module")
def tiny_clips(encoders):
    """Features of FRAMES frames and each clip's single-path result, computed once and left unchanged."""
    g = torch.Generator().manual_seed(41)
    feats = [2 * torch.randn(24, w, generator=g) for w in FRAMES]
    assert not torch.equal(feats[0], feats[4])
    singles = [tuple(t.clone() for t in encoders("tiny").embed_features(f)) for f in feats]
    return feats, singles


def _same(batch, singles, order=None):
    emb, lda = batch
    order = range(len(singles)) if order is None else order
    assert emb.shape == (len(order), 256) and lda.shape == (len(order), 128)
    assert emb.dtype == lda.dtype == torch.float32
    for row, i in enumerate(order):
        assert torch.equal(emb[row:row + 1], singles[i][0]), f"emb of clip {i}"
        assert torch.equal(lda[row:row + 1], singles[i][1]), f"lda of clip {i}"


def test_model_batch_equals_single(encoders, tiny_clips):
    feats, singles = tiny_clips
    enc = encoders("tiny")
    assert plan_lanes(list(FRAMES)) == [[1, 3, 0, 4, 2]]                # one group
    _same(enc.embed_features_batch(feats), singles)
    assert not torch.equal(singles[0][1], singles[4][1])                # the two 37-frame clips differ, each its own
    perm = [3, 0, 4, 2, 1]
    _same(enc.embed_features_batch([feats[i] for i in perm]), singles, perm)
    _same(enc.embed_features_batch([feats[1]]), singles, [1])


def test_model_forced_groups_equal_one_group(encoders, tiny_clips):
    feats, singles = tiny_clips
    enc = encoders("tiny")
    assert plan_lanes(list(FRAMES), max_lanes=2) == [[1, 3], [0, 4], [2]]
    _same(enc.embed_features_batch(feats, max_lanes=2), singles)
    assert plan_lanes(list(FRAMES), max_lane_frames=150) == [[1], [3, 0], [4, 2]]
    _same(enc.embed_features_batch(feats, max_lane_frames=150), singles)


def test_model_full_config(encoders):
    enc = encoders("full")
    g = torch.Generator().manual_seed(42)
    feats = [2 * torch.randn(80, 40, generator=g), 2 * torch.randn(80, 23, generator=g)]
    singles = [tuple(t.clone() for t in enc.embed_features(f)) for f in feats]
    _same(enc.embed_features_batch(feats), singles)
    assert all(torch.isfinite(s[1]).all() for s in singles)


def test_workspace_batch_single_larger_batch(tiny_clips):
    """One instance: a batch, a single clip, a larger batch (the workspace grows twice); each as a fresh instance's."""
    feats, singles = tiny_clips
    used = SpeakerEmbeddingLDA(DEV, seed=0, config=TINY)
    _same(used.embed_features_batch([feats[0], feats[2]]), singles, [0, 2])
    a = used.embed_features(feats[3])
    assert torch.equal(a[0], singles[3][0]) and torch.equal(a[1], singles[3][1])
    _same(used.embed_features_batch(feats), singles)
    _same(used.embed_features_batch([feats[2], feats[0]]), singles, [2, 0])


def test_make_speaker_embeddings():
    from zonos_vibes_amd.conditioning import v01_transformer_conditioners
    from zonos_vibes_amd.config import PrefixConditionerConfig, tiny_transformer
    from zonos_vibes_amd.model import Zonos
    cfg = tiny_transformer(2)
    cfg.prefix_conditioner = PrefixConditionerConfig(v01_transformer_conditioners(), "none")
    m = Zonos.synthetic(cfg, DEV, zero_eos=True, max_seqlen=96, max_prefill=48)
    g = torch.Generator().manual_seed(43)
    wavs = [torch.rand(2, 22050, generator=g) * 1.8 - 0.9,             # stereo, 0.5 s at 44.1 kHz
            torch.rand(4800, generator=g) * 1.8 - 0.9,                 # mono, 0.3 s at 16 kHz
            torch.rand(1, 15435, generator=g) * 1.8 - 0.9]             # mono, 0.7 s at 22.05 kHz
    srs = [44100, 16000, 22050]
    got = m.make_speaker_embeddings(wavs, srs)
    assert isinstance(got, list) and len(got) == 3
    for spk, wav, sr in zip(got, wavs, srs):
        ref = m.make_speaker_embedding(wav, sr)
        assert spk.shape == ref.shape == (1, 1, 128) and spk.dtype == ref.dtype == torch.bfloat16
        assert spk.device == ref.device and spk.device.type == "cuda"
        assert torch.equal(spk, ref)
    assert not torch.equal(got[0], got[1])
    same_rate = m.make_speaker_embeddings([wavs[1], wavs[1]], 16000)      # one int for every clip
    assert torch.equal(same_rate[0], got[1]) and torch.equal(same_rate[1], got[1])
    bare = Zonos(cfg, DEV, max_seqlen=96, max_prefill=48)
    with pytest.raises(RuntimeError):
        bare.make_speaker_embeddings(wavs, srs)


# ------------------------------------------------------------------------------------- rejections
def _lanes(n, widths):
    L = _lib.SpkLanes()
    L.n = n
    for i, w in enumerate(widths):
        L.w[i] = w
    return L


def test_lanes_reject_bad_arguments(gpu_lib):
    """Each error returns nonzero with a message and launches nothing: the sentinel-filled outputs are untouched."""
    lib, H, C = gpu_lib, 8, 32
    ext = H * 20 * C
    x = torch.zeros(4 * ext, dtype=torch.float16, device=DEV)
    res = torch.zeros(4 * ext, dtype=torch.float16, device=DEV)
    wt = torch.zeros(9 * 64 * 64, dtype=torch.float16, device=DEV)
    f = torch.zeros(4096, dtype=torch.float32, device=DEV)
    y, ps, ws = _sent16(4 * ext), _sent32(4096), _sent32(8192)
    ok, ok2 = _lanes(2, (20, 7)), _lanes(1, (20,))
    big = ws.numel() // 2  # a ws stride with room for both lanes
    p = lambda t: t.data_ptr()  # noqa: E731

    def conv(L, ci=C, co=C, k=3, s=1, ls=(ext, ext, 2 * C)):
        return lib.zmi_spk_conv2d_lanes(p(x), H, L, ci, p(wt), p(f), p(f), co, k, s, 0, p(y), p(ps), *ls, 0)

    def stem(L, co=C, ls=(H * 20, ext)):
        return lib.zmi_spk_stem_lanes(p(x), H, L, p(wt), p(f), p(f), co, p(y), *ls, 0)

    def simam(L, h=H, c=C, ls=(ext, ext, 2 * C, big, ext), rows=(2, 1)):
        return lib.zmi_spk_simam_lanes(p(x), p(res), h, L, c, p(ps), (_lib.c_int * 32)(*rows), p(ws), p(y), *ls, 0)

    bad = {
        "conv: no lanes": lambda: conv(_lanes(0, ())),
        "conv: 33 lanes": lambda: conv(_lanes(33, (20,) * 32)),
        "conv: width 0": lambda: conv(_lanes(2, (20, 0))),
        "conv: x stride": lambda: conv(ok, ls=(ext - 8, ext, 2 * C)),
        "conv: y stride": lambda: conv(ok, ls=(ext, ext - 8, 2 * C)),
        "conv: psum stride": lambda: conv(ok, ls=(ext, ext, 2 * C - 1)),
        "conv: unaligned stride": lambda: conv(ok, ls=(ext + 4, ext, 2 * C)),
        "conv: Ci": lambda: conv(ok, ci=16),
        "conv: Co": lambda: conv(ok, co=48),
        "conv: k": lambda: conv(ok, k=5),
        "conv: stride": lambda: conv(ok2, s=3),
        "stem: no lanes": lambda: stem(_lanes(0, ())),
        "stem: 33 lanes": lambda: stem(_lanes(33, (20,) * 32)),
        "stem: width -1": lambda: stem(_lanes(2, (20, -1))),
        "stem: x stride": lambda: stem(ok, ls=(H * 20 - 1, ext)),
        "stem: y stride": lambda: stem(ok, ls=(H * 20, ext - 8)),
        "stem: Co": lambda: stem(ok2, co=12),
        "simam: no lanes": lambda: simam(_lanes(0, ())),
        "simam: 33 lanes": lambda: simam(_lanes(33, (20,) * 32)),
        "simam: width 0": lambda: simam(_lanes(2, (0, 20))),
        "simam: H w < 2": lambda: simam(_lanes(2, (20, 1)), h=1),
        "simam: x stride": lambda: simam(ok, ls=(ext - 8, ext, 2 * C, big, ext)),
        "simam: residual stride": lambda: simam(ok, ls=(ext, ext - 8, 2 * C, big, ext)),
        "simam: psum stride": lambda: simam(ok, ls=(ext, ext, 2 * C - 1, big, ext)),
        "simam: ws stride": lambda: simam(ok, ls=(ext, ext, 2 * C, lib.zmi_spk_simam_ws_floats(H, 20, C) - 1, ext)),
        "simam: y stride": lambda: simam(ok, ls=(ext, ext, 2 * C, big, ext - 8)),
        "simam: C": lambda: simam(ok2, c=24),
        "simam: psum rows": lambda: simam(ok, rows=(2, 0)),
    }
    for name, call in bad.items():
        assert call() != 0, name
        assert lib.zmi_last_error().decode().startswith("spk_"), name
    torch.cuda.synchronize()
    assert bool((_bits(y) == H16).all()) and bool((_bits(ps) == F32).all()) and bool((_bits(ws) == F32).all())
    # the same calls with good arguments launch (the table above fails on its own terms, not on these buffers)
    big_ws = _sent32(2 * lib.zmi_spk_simam_ws_floats(H, 20, C))
    assert conv(ok) == 0 and stem(ok) == 0
    assert lib.zmi_spk_simam_lanes(p(x), p(res), H, ok, C, p(ps), (_lib.c_int * 2)(2, 1), p(big_ws), p(y), ext, ext,
                                   2 * C, big_ws.numel() // 2, ext, 0) == 0
    torch.cuda.synchronize()
