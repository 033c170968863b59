"""Speaker encoder, CPU side: the restatement (tests/spk_cpu.py) against the reference's recorded tensors
(tests/golden/speaker.safetensors), the fp16 emulation error the GPU bound is built from, the loader table, and the
front end's properties (filterbank, resampler)."""
import json
import math
import os

import pytest
import torch
from safetensors import safe_open

import spk_cpu
from zonos_vibes_amd import synthetic as syn
from zonos_vibes_amd import speaker as spk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speaker.safetensors")
# fp32 floor under "10 x thread noise" where the recorded noise is exactly 0 (stem .. layer2.0 of the tiny model):
# one fp32 ulp at the tensor's magnitude
ULP32 = 2.0 ** -23


def load_golden():
    with safe_open(GOLDEN, "pt") as f:
        return {k: f.get_tensor(k) for k in f.keys()}, json.loads(f.metadata()["json"])


def config_of(meta):
    c = meta["config"]
    return spk.SpeakerEncoderConfig(c["in_planes"], tuple(c["num_blocks"]), c["acoustic_dim"], c["embd_dim"], c["lda_dim"])


_weights = {}


def weights(tag, meta):
    if tag not in _weights:
        w = dict(syn.iter_torch_cpu(syn.speaker_specs(config_of(meta[tag])), 0))
        lda = {k[4:]: w.pop(k) for k in list(w) if k.startswith("lda.")}
        _weights[tag] = (w, lda)
    return _weights[tag]


def run(tag, dtype):
    t, meta = load_golden()
    cfg = config_of(meta[tag])
    w, lda = weights(tag, meta)
    rec = {}
    spk_cpu.SpeakerCPU(w, lda, cfg.in_planes, cfg.num_blocks, dtype)(t[tag + "/input"], rec)
    keys = [k[len(tag) + 1:] for k in t if k.startswith(tag + "/") and k != tag + "/input"]
    return {k: float((rec[k] - t[f"{tag}/{k}"]).abs().max()) for k in keys}, meta[tag]


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_fp32_restatement_matches_reference(tag):
    err, meta = run(tag, torch.float32)
    for k, e in err.items():
        bound = 10 * max(meta["thread_noise"][k], ULP32 * meta["max_abs"][k])
        print(f"{tag}/{k}: max abs err {e:.3e} (bound {bound:.3e})")
        assert e <= bound, (k, e, bound)


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_fp16_emulation_error_is_the_recorded_one(tag):
    """E_emul per recorded tensor, the quantity tests/test_gpu_speaker.py bounds the kernels with (2 E_emul + thread
    noise; it reads the STORED values, so that bound cannot drift). Which fp16 roundings flip depends on the host conv
    library's summation order (the fixture also records the 8-thread values, `e_emul_8_threads`, up to 6 % away on the
    tiny model's emb / lda), so the emulation runs with 1 thread, as when it was recorded, and must then reproduce the
    stored value: equal to 1e-6 relative."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        err, meta = run(tag, torch.float16)
    finally:
        torch.set_num_threads(n)
    for k, e in err.items():
        print(f"{tag}/{k}: E_emul {e:.4e} (stored {meta['e_emul'][k]:.4e})")
        assert e == pytest.approx(meta["e_emul"][k], rel=1e-6), k
        assert e > 10 * meta["thread_noise"][k]  # the emulation does round


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_loader_table_accepts_the_reference_state_dict(tag):
    _, meta = load_golden()
    cfg = config_of(meta[tag])
    table = spk.expected_shapes(cfg)
    ref = {k: tuple(v) for k, v in meta[tag]["state_dict"].items()}
    assert table == ref
    assert spk.lda_shapes(cfg) == {k: tuple(v) for k, v in meta[tag]["lda_state_dict"].items()}
    sd = {k: torch.empty(v, device="meta") for k, v in ref.items()}
    spk.check_state_dict(sd, table, "t")
    spk.check_state_dict({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}, table, "t")
    with pytest.raises(KeyError):
        spk.check_state_dict({**sd, "front.conv9.weight": torch.empty(1, device="meta")}, table, "t")
    with pytest.raises(KeyError):
        spk.check_state_dict({k: v for k, v in sd.items() if k != "front.layer2.0.downsample.0.weight"}, table, "t")
    with pytest.raises(ValueError):
        spk.check_state_dict({**sd, "bottleneck.bias": torch.empty(3, device="meta")}, table, "t")


def test_full_table_names():
    table = spk.expected_shapes(spk.SpeakerEncoderConfig())
    assert table["front.conv1.weight"] == (64, 1, 3, 3)
    assert table["front.layer3.17.bn2.running_var"] == (256,)
    assert table["front.layer2.0.downsample.0.weight"] == (128, 64, 1, 1)
    assert table["pooling.attention.0.weight"] == (128, 5120, 1) and table["pooling.attention.3.bias"] == (5120,)
    assert table["bottleneck.weight"] == (256, 10240)
    assert "front.layer1.0.downsample.0.weight" not in table
    n = sum(math.prod(s) for k, s in table.items() if not k.endswith("num_batches_tracked"))
    assert 98.5e6 < n < 99.5e6  # the 98.9 M parameters of ResNet293_SimAM_ASP_base


def test_weight_files(tmp_path):
    from safetensors.torch import save_file
    sd = {"weight": torch.randn(4, 3), "bias": torch.randn(4)}
    save_file(sd, str(tmp_path / "a.safetensors"))
    torch.save(sd, str(tmp_path / "a.pt"))
    for name in ("a.safetensors", "a.pt"):
        got = spk.load_weights_file(str(tmp_path / name))
        assert all(torch.equal(got[k], v) for k, v in sd.items())
    import pathlib
    torch.save({"weight": pathlib.PurePosixPath("x")}, str(tmp_path / "bad.pt"))  # a pickle of more than plain tensors
    with pytest.raises(Exception):
        spk.load_weights_file(str(tmp_path / "bad.pt"))


# ------------------------------------------------------------------------------------- front end
@pytest.mark.parametrize("mod", [spk, spk_cpu], ids=["package", "restatement"])
def test_filterbank(mod):
    fb = mod.mel_filterbank(257, 80, 16000)
    fb = fb[0] if isinstance(fb, tuple) else fb
    assert fb.shape == (257, 80) and (fb >= 0).all()
    # the triangles' peak frequencies (the module's own corner points 1 .. n_mels) rise strictly; below ~500 Hz a
    # triangle is narrower than the 31.25 Hz DFT bin spacing, so the peak BIN (the bank sampled at the DFT
    # frequencies) may repeat but never falls, and it lies within one bin of the triangle's peak frequency
    f_pts = mod.mel_points(80, 16000) if mod is spk else mod.mel_filterbank(257, 80, 16000)[1]
    assert f_pts.shape == (82,) and float(f_pts[0]) == 0.0 and abs(float(f_pts[-1]) - 8000.0) < 1e-2
    assert (f_pts[1:] > f_pts[:-1]).all()
    peak = fb.argmax(0)
    assert (peak[1:] >= peak[:-1]).all() and (peak[20:][1:] > peak[20:][:-1]).all()
    assert ((peak * 31.25 - f_pts[1:-1]).abs() <= 31.25).all()
    assert torch.equal(fb, spk_cpu.mel_filterbank(257, 80, 16000)[0])


def test_sine_peaks_in_its_mel_bin():
    """A 1 kHz sine at 16 kHz: the mel power (before the log and the mean subtraction, which flattens a stationary
    tone) peaks in a bin whose triangle contains 1 kHz."""
    wav = 0.5 * torch.sin(2 * math.pi * 1000.0 * torch.arange(16000) / 16000.0)[None]
    fb, f_pts = spk_cpu.mel_filterbank(257, 80, 16000)
    for power in (spk_cpu.mel_power(wav), spk.mel_power(wav, spk.dft_basis(), spk.mel_filterbank())):
        assert power.shape == (80, 101)
        got = int(power[:, 50].argmax())
        assert float(f_pts[got]) < 1000.0 < float(f_pts[got + 2])
        assert torch.equal(power[:, 10:90].argmax(0), torch.full((80,), got))


def test_log_fbank_package_matches_restatement():
    g = torch.Generator().manual_seed(3)
    wav = (torch.rand(1, 8000, generator=g) * 1.8 - 0.9)
    a = spk.log_fbank(wav, spk.dft_basis(), spk.mel_filterbank())
    b = spk_cpu.log_fbank(wav)
    assert a.shape == b.shape == (80, 51)
    assert (a - b).abs().max() <= 1e-4


@pytest.mark.parametrize("fn", [spk.resample, spk_cpu.resample], ids=["package", "restatement"])
def test_resample_lengths_and_identity(fn):
    x = torch.randn(1, 4411)
    assert fn(x, 16000, 16000) is x or torch.equal(fn(x, 16000, 16000), x)
    assert fn(x, 44100, 16000).shape == (1, math.ceil(160 * 4411 / 441))
    assert fn(torch.randn(2, 3000), 48000, 16000).shape == (2, 1000)


# max |resampled - analytic| of a 440 Hz sine 44.1 k -> 16 k, 64 samples in from each edge, measured once with the
# float64 restatement (spk_cpu.resample(dtype=torch.float64)): the windowed-sinc filter's own error
RESAMPLE_ERR64 = 2.239e-4


def _sine_err(fn, **kw):
    n = 22050
    x = torch.sin(2 * math.pi * 440.0 * torch.arange(n, dtype=torch.float64) / 44100.0)[None]
    y = fn(x if kw else x.float(), 44100, 16000, **kw)
    ref = torch.sin(2 * math.pi * 440.0 * torch.arange(y.shape[-1], dtype=torch.float64) / 16000.0)
    return float((y[0].double() - ref)[64:-64].abs().max())


def test_resample_sine():
    e64 = _sine_err(spk_cpu.resample, dtype=torch.float64)
    print(f"float64 restatement: {e64:.3e} (recorded {RESAMPLE_ERR64:.3e})")
    assert e64 == pytest.approx(RESAMPLE_ERR64, rel=1e-3)
    for fn in (spk.resample, spk_cpu.resample):
        e = _sine_err(fn)
        print(f"{fn.__module__}: {e:.3e}")
        assert e <= 2 * RESAMPLE_ERR64
