"""Speaker encoder on the GPU (csrc/zmi_spk.hip, zonos_vibes_amd/speaker.py).

Kernels: the implicit-GEMM conv is exact on small-integer data (fp32 sums of integers), SimAM is compared with the
CPU restatement to one fp16 ulp of the output, and both are bit-reproducible. Models: every stage the reference
recorded (tests/golden/speaker.safetensors, made by make_golden_spk.py) within

    max |hip - golden| <= 2 E_emul + thread noise

E_emul being the error of the fp16-emulating CPU restatement (tests/spk_cpu.py, which rounds where the kernels round)
and thread noise the reference's own 1-vs-8-thread difference, both stored beside the fixture
(tests/test_speaker_cpu.py checks E_emul is what the restatement gives). The kernels differ from the emulation only in
fp32 summation order, the fp32 form of the BatchNorm and the order of the SimAM statistics: the factor 2 is the room
given to those.
"""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F
from safetensors import safe_open

import spk_cpu
from zonos_vibes_amd import _lib
from zonos_vibes_amd.autoencoder import _blocked
from zonos_vibes_amd.speaker import SpeakerEmbeddingLDA, SpeakerEncoderConfig

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speaker.safetensors")
TINY = SpeakerEncoderConfig(in_planes=32, num_blocks=(2, 2, 2, 1), acoustic_dim=24)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def _conv(lib, x_hwc, w, scale, shift, stride, relu, want_psum=True):
    """x [H][W][Ci] fp16 (device), w [Co][Ci][k][k] fp32 -> y [Ho][Wo][Co] fp16 and the per-tile sums."""
    H, W, ci = x_hwc.shape
    co, _, k, _ = w.shape
    ho, wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    wb = _blocked(w.to(DEV).permute(2, 3, 0, 1).reshape(k * k, co, ci))
    y = torch.full((ho, wo, co), float("nan"), dtype=torch.float16, device=DEV)
    tiles = lib.zmi_spk_conv2d_tiles(H, W, k, stride)
    assert tiles == math.ceil(ho / 8) * math.ceil(wo / 16)
    psum = torch.full((tiles, co), float("nan"), dtype=torch.float32, device=DEV) if want_psum else None
    _lib.check(lib.zmi_spk_conv2d(x_hwc.data_ptr(), H, W, ci, wb.data_ptr(), scale.data_ptr(), shift.data_ptr(), co, k,
                                  stride, int(relu), y.data_ptr(), _lib.ptr(psum), 0), "spk_conv2d")
    torch.cuda.synchronize()
    return y, psum


@pytest.mark.parametrize("hw", [(3, 5), (24, 37), (12, 19)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cio", [(32, 32), (64, 32), (32, 64)], ids=lambda v: f"{v[0]}to{v[1]}")
def test_conv2d_exact(gpu_lib, cio, stride, k, hw):
    """Small-integer inputs and asymmetric small-integer weights: every fp32 sum is exact, so the kernel equals
    F.conv2d bit for bit (all four padding edges, partial tiles, one and two K blocks, odd sizes under stride 2)."""
    (ci, co), (H, W) = cio, hw
    x = _ints((H, W, ci), -3, 3, 1)
    w = _ints((co, ci, k, k), -2, 2, 2)
    assert not torch.equal(w, w.flip(2, 3)) or k == 1
    ref = F.conv2d(x.permute(2, 0, 1)[None], w, None, stride, k // 2)[0].permute(1, 2, 0)
    one, zero = torch.ones(co, device=DEV), torch.zeros(co, device=DEV)
    y, psum = _conv(gpu_lib, x.half().to(DEV), w, one, zero, stride, False)
    assert torch.equal(y.float().cpu(), ref.half().float())
    assert torch.equal(psum.sum(0).cpu(), ref.half().float().sum((0, 1)))  # integer sums: exact in any order
    y2, psum2 = _conv(gpu_lib, x.half().to(DEV), w, one, zero, stride, False)
    assert torch.equal(y, y2) and torch.equal(psum, psum2)


def test_conv2d_batchnorm_relu_epilogue(gpu_lib):
    """y = relu(acc * scale + shift) in fp32 (two roundings, no fused multiply-add), then fp16."""
    x, w = _ints((12, 19, 64), -3, 3, 3), _ints((64, 64, 3, 3), -2, 2, 4)
    g = torch.Generator().manual_seed(5)
    scale, shift = 0.8 + 0.4 * torch.rand(64, generator=g), torch.randn(64, generator=g)
    acc = F.conv2d(x.permute(2, 0, 1)[None], w, None, 1, 1)[0].permute(1, 2, 0)
    ref = torch.relu(acc * scale + shift).half()
    y, _ = _conv(gpu_lib, x.half().to(DEV), w, scale.to(DEV), shift.to(DEV), 1, True, want_psum=False)
    assert torch.equal(y.cpu(), ref)


def test_conv2d_rejects_bad_arguments(gpu_lib):
    t = torch.zeros(64, device=DEV)
    for (ci, co, k, s) in [(16, 32, 3, 1), (32, 48, 3, 1), (32, 32, 5, 1), (32, 32, 3, 3)]:
        assert gpu_lib.zmi_spk_conv2d(t.data_ptr(), 4, 4, ci, t.data_ptr(), t.data_ptr(), t.data_ptr(), co, k, s, 0,
                                      t.data_ptr(), None, 0) != 0


def test_stem_exact(gpu_lib):
    H, W, co = 24, 37, 32
    x, w = _ints((H, W), -3, 3, 6), _ints((co, 1, 3, 3), -2, 2, 7)
    ref = torch.relu(F.conv2d(x[None, None], w, None, 1, 1))[0].permute(1, 2, 0)
    xd = x.half().to(DEV)
    wd = w.reshape(co, 9).t().contiguous().half().to(DEV)
    y = torch.full((H, W, co), float("nan"), dtype=torch.float16, device=DEV)
    one, zero = torch.ones(co, device=DEV), torch.zeros(co, device=DEV)
    _lib.check(gpu_lib.zmi_spk_stem(xd.data_ptr(), H, W, wd.data_ptr(), one.data_ptr(), zero.data_ptr(), co,
                                    y.data_ptr(), 0), "spk_stem")
    assert torch.equal(y.float().cpu(), ref)


def _fp16_ulp(v):
    """One fp16 ulp at |v| (2^-24 below the smallest normal)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


@pytest.mark.parametrize("hw", [(3, 5), (24, 37)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_simam(gpu_lib, hw):
    """SimAM + residual + ReLU against the restatement: the statistics are fp32 on both sides, so the outputs agree
    to the fp16 rounding of the result (1 ulp at its magnitude); two launches give the same bits."""
    (H, W), C = hw, 32
    g = torch.Generator().manual_seed(11)
    x, res = torch.randn(H, W, C, generator=g).half(), torch.randn(H, W, C, generator=g).half()
    cpu = spk_cpu.SpeakerCPU({}, {}, C, (1, 1, 1, 1), torch.float16)
    ref = cpu.simam_tail(x.float().permute(2, 0, 1)[None], res.float().permute(2, 0, 1)[None])[0].permute(1, 2, 0)
    ws = torch.empty(gpu_lib.zmi_spk_simam_ws_floats(H, W, C), dtype=torch.float32, device=DEV)
    xd, rd = x.to(DEV), res.to(DEV)
    outs = []
    for _ in range(2):
        y = torch.full((H, W, C), float("nan"), dtype=torch.float16, device=DEV)
        _lib.check(gpu_lib.zmi_spk_simam(xd.data_ptr(), rd.data_ptr(), H, W, C, None, 0, ws.data_ptr(), y.data_ptr(), 0),
                   "spk_simam")
        outs.append(y.cpu())
    err = (outs[0].float() - ref).abs()
    print(f"simam {H}x{W}: max err {float(err.max()):.3e}, in ulps {float((err / _fp16_ulp(ref)).max()):.2f}")
    assert (err <= _fp16_ulp(ref)).all()
    assert torch.equal(outs[0], outs[1])


def test_simam_with_conv_tile_sums(gpu_lib):
    """The path the model takes: the producing conv writes its per-tile channel sums and SimAM takes its mean from
    them (n_psum = tiles). Same 1-ulp comparison, on the conv's own stored output; two tiles wide, three high, with
    partial tiles on both edges."""
    H, W, C = 20, 27, 32
    g = torch.Generator().manual_seed(12)
    x = torch.randn(H, W, C, generator=g).half()
    w = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
    res = torch.randn(H, W, C, generator=g).half()
    scale, shift = (0.8 + 0.4 * torch.rand(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    y, psum = _conv(gpu_lib, x.to(DEV), w.half().float(), scale, shift, 1, False)
    assert psum.shape[0] == 6 and torch.isfinite(psum).all()
    tot = y.float().sum((0, 1))
    assert (psum.sum(0) - tot).abs().max() <= 1e-5 * y.float().abs().sum((0, 1)).max()
    cpu = spk_cpu.SpeakerCPU({}, {}, C, (1, 1, 1, 1), torch.float16)
    ref = cpu.simam_tail(y.float().cpu().permute(2, 0, 1)[None], res.float().permute(2, 0, 1)[None])[0].permute(1, 2, 0)
    ws = torch.empty(gpu_lib.zmi_spk_simam_ws_floats(H, W, C), dtype=torch.float32, device=DEV)
    rd, outs = res.to(DEV), []
    for _ in range(2):
        out = torch.full((H, W, C), float("nan"), dtype=torch.float16, device=DEV)
        _lib.check(gpu_lib.zmi_spk_simam(y.data_ptr(), rd.data_ptr(), H, W, C, psum.data_ptr(), psum.shape[0],
                                         ws.data_ptr(), out.data_ptr(), 0), "spk_simam")
        outs.append(out.cpu())
    err = (outs[0].float() - ref).abs()
    print(f"simam after conv: max err {float(err.max()):.3e}, in ulps {float((err / _fp16_ulp(ref)).max()):.2f}")
    assert (err <= _fp16_ulp(ref)).all()
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------- models against the golden
@pytest.fixture(scope="module")
def golden():
    with safe_open(GOLDEN, "pt") as f:
        return {k: f.get_tensor(k) for k in f.keys()}, json.loads(f.metadata()["json"])


@pytest.fixture(scope="module")
def encoders():
    made = {}

    def get(tag):
        if tag not in made:
            made[tag] = SpeakerEmbeddingLDA(DEV, seed=0, config=TINY if tag == "tiny" else SpeakerEncoderConfig())
        return made[tag]
    return get


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_model_matches_reference(golden, encoders, tag):
    t, meta = golden
    m = meta[tag]
    rec = {}
    emb, lda = encoders(tag).embed_features(t[tag + "/input"], rec)
    rec.update(emb=emb, lda=lda)
    bad = []
    for k in m["e_emul"]:
        got, ref = rec[k].float().cpu(), t[f"{tag}/{k}"]
        assert got.shape == ref.shape, k
        err, bound = float((got - ref).abs().max()), 2 * m["e_emul"][k] + m["thread_noise"][k]
        print(f"{tag}/{k}: max |hip - golden| {err:.3e}, bound {bound:.3e} (E_emul {m['e_emul'][k]:.3e})")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


def test_pipeline_is_deterministic(encoders):
    enc = encoders("tiny")
    g = torch.Generator().manual_seed(21)
    wav = torch.rand(2, 9000, generator=g) * 1.8 - 0.9
    a, b = enc(wav, 22050), enc(wav, 22050)
    assert a[0].shape == (1, 256) and a[1].shape == (1, 128) and a[0].dtype == a[1].dtype == torch.float32
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert math.isfinite(float(a[1].abs().max())) and float(a[1].abs().max()) > 0


def test_workspace_growth_leaves_no_trace(encoders):
    """A fresh instance at 203 frames equals one that ran 37 frames first (its workspace grows in between)."""
    g = torch.Generator().manual_seed(22)
    short, long_ = 2 * torch.randn(24, 37, generator=g), 2 * torch.randn(24, 203, generator=g)
    used = SpeakerEmbeddingLDA(DEV, seed=0, config=TINY)
    used.embed_features(short)
    a = used.embed_features(long_)
    b = SpeakerEmbeddingLDA(DEV, seed=0, config=TINY).embed_features(long_)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = used.embed_features(short)
    d = encoders("tiny").embed_features(short)
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])


# ------------------------------------------------------------------------------------- API
def test_front_end_matches_restatement(encoders):
    """Mono mean + resampling + log filterbank on the device against tests/spk_cpu.py: fp32 sums of at most 512
    terms on |x| <= 0.9 input, 1e-4 absolute."""
    g = torch.Generator().manual_seed(23)
    wav = torch.rand(2, 22050, generator=g) * 1.8 - 0.9
    got = encoders("full").features(wav, 44100).cpu()
    ref = spk_cpu.log_fbank(spk_cpu.resample(wav.mean(0, keepdim=True), 44100, 16000))
    assert got.shape == ref.shape == (80, 51)
    err = float((got - ref).abs().max())
    print(f"front end max abs err {err:.3e}")
    assert err <= 1e-4


def test_make_speaker_embedding():
    from zonos_vibes_amd.conditioning import make_cond_dict, v01_transformer_conditioners
    from zonos_vibes_amd.config import PrefixConditionerConfig, tiny_transformer
    from zonos_vibes_amd.model import Zonos
    cfg = tiny_transformer(2)
    cfg.prefix_conditioner = PrefixConditionerConfig(v01_transformer_conditioners(), "none")
    m = Zonos.synthetic(cfg, DEV, zero_eos=True, max_seqlen=96, max_prefill=48)
    g = torch.Generator().manual_seed(24)
    wav = torch.rand(2, 22050, generator=g) * 1.8 - 0.9                # stereo, 0.5 s at 44.1 kHz
    assert m.spk_clone_model is None
    spk = m.make_speaker_embedding(wav, 44100)
    assert spk.shape == (1, 1, 128) and spk.dtype == torch.bfloat16 and spk.device.type == "cuda"
    assert isinstance(m.spk_clone_model, SpeakerEmbeddingLDA)
    _, lda = m.spk_clone_model(wav.mean(0, keepdim=True), 44100)
    assert torch.equal(spk, lda.unsqueeze(0).bfloat16())
    cond = m.prepare_conditioning(make_cond_dict(phonemes="həloʊ", speaker=spk, device=DEV))
    assert cond.shape[0] == 2 and cond.dtype == torch.bfloat16 and torch.isfinite(cond.float()).all()
    bare = Zonos(cfg, DEV, max_seqlen=96, max_prefill=48)
    with pytest.raises(RuntimeError):
        bare.make_speaker_embedding(wav, 44100)
