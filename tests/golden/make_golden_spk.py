"""Golden fixture of the speaker encoder, from the REFERENCE's own modules. It needs the reference tree and runs on
the CPU only; no test and no GPU run imports it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_spk.py

The reference's `ResNet293_based` (zonos/speaker_cloning.py:199-224) is built with `featCal` replaced by identity and
loaded with the counter-based synthetic weights of `zonos_vibes_amd.synthetic.speaker_specs`, plus the LDA Linear.
Two models are recorded on a `2 randn` input of 37 frames:
  tiny/  in_planes 32, blocks (2, 2, 2, 1), acoustic_dim 24 (the reference's ResNet293 factory pointed at those
         block counts): input, stem, layer1.0, layer2.0, front, pooled, emb, lda
  full/  ResNet293, acoustic_dim 80: input, front, emb, lda
Metadata: every state-dict key with its shape, the reference's own 1-thread vs 8-thread max-abs difference per
recorded tensor (`thread_noise`), and `e_emul`: the error of the fp16-emulating CPU restatement (tests/spk_cpu.py)
against the recorded tensors, from which the GPU tests' bound is derived (tests/test_gpu_speaker.py).
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402
from spk_cpu import SpeakerCPU  # noqa: E402

from zonos_vibes_amd import synthetic as syn  # noqa: E402
from zonos_vibes_amd.speaker import SpeakerEncoderConfig  # noqa: E402

TINY = SpeakerEncoderConfig(in_planes=32, num_blocks=(2, 2, 2, 1), acoustic_dim=24)
FULL = SpeakerEncoderConfig()
FRAMES = 37


def build_reference(sc, cfg):
    sc.ResNet293 = lambda in_planes, **kw: sc.ResNet(in_planes, sc.SimAMBasicBlock, list(cfg.num_blocks), **kw)
    model = sc.ResNet293_based(in_planes=cfg.in_planes, embd_dim=cfg.embd_dim, acoustic_dim=cfg.acoustic_dim,
                               featCal=torch.nn.Identity())
    w = dict(syn.iter_torch_cpu(syn.speaker_specs(cfg), 0))
    lda_w = {k[4:]: w.pop(k) for k in list(w) if k.startswith("lda.")}
    sd = model.state_dict()
    shapes = {k: list(v.shape) for k, v in sd.items()}
    assert set(w) == {k for k in sd if not k.endswith("num_batches_tracked")}, "spec names differ from the reference's"
    for k, v in w.items():
        assert sd[k].shape == v.shape, (k, sd[k].shape, v.shape)
        sd[k].copy_(v)
    model.load_state_dict(sd)
    lda = torch.nn.Linear(cfg.embd_dim, cfg.lda_dim, bias=True, dtype=torch.float32)
    lda.load_state_dict(lda_w)
    return model.eval().requires_grad_(False), lda.eval().requires_grad_(False), w, lda_w, shapes


def run_reference(model, lda, x, stages, threads):
    torch.set_num_threads(threads)
    got, hooks = {}, []

    def grab(name):
        return lambda _m, _i, o: got.__setitem__(name, o.detach().clone())

    hooks.append(model.front.register_forward_hook(grab("front")))
    hooks.append(model.pooling.register_forward_hook(grab("pooled")))
    if stages:
        hooks.append(model.front.relu.register_forward_hook(grab("stem")))
        hooks.append(model.front.layer1[0].register_forward_hook(grab("layer1.0")))
        hooks.append(model.front.layer2[0].register_forward_hook(grab("layer2.0")))
    with torch.inference_mode():
        got["emb"] = model(x[None])
        got["lda"] = lda(got["emb"])
    for h in hooks:
        h.remove()
    return got


def main():
    mg.import_reference()
    import zonos.speaker_cloning as sc
    tensors, meta = {}, {}
    for tag, cfg, stages in (("tiny", TINY, True), ("full", FULL, False)):
        model, lda, w, lda_w, shapes = build_reference(sc, cfg)
        x = 2 * torch.randn(cfg.acoustic_dim, FRAMES, generator=torch.Generator().manual_seed(7 if stages else 8))
        g8 = run_reference(model, lda, x, stages, 8)
        g1 = run_reference(model, lda, x, stages, 1)
        keep = list(g8) if stages else ["front", "emb", "lda"]
        noise = {k: float((g8[k] - g1[k]).abs().max()) for k in keep}
        e = {}
        for threads in (1, 8):
            torch.set_num_threads(threads)
            rec = {}
            SpeakerCPU(w, lda_w, cfg.in_planes, cfg.num_blocks, torch.float16)(x, rec)
            e[threads] = {k: float((rec[k] - g8[k]).abs().max()) for k in keep}
        tensors[tag + "/input"] = x
        for k in keep:
            tensors[f"{tag}/{k}"] = g8[k]
        meta[tag] = dict(config=dict(in_planes=cfg.in_planes, num_blocks=list(cfg.num_blocks),
                                     acoustic_dim=cfg.acoustic_dim, embd_dim=cfg.embd_dim, lda_dim=cfg.lda_dim),
                         state_dict=shapes, lda_state_dict={k: list(v.shape) for k, v in lda_w.items()},
                         thread_noise=noise, e_emul=e[1], e_emul_8_threads=e[8],
                         max_abs={k: float(g8[k].abs().max()) for k in keep})
        print(tag, "noise", noise, "\n  e_emul", e[1], "\n  e_emul(8 threads)", e[8], "\n  max_abs", meta[tag]["max_abs"])
    torch.set_num_threads(8)
    mg.save("speaker", tensors, meta)


if __name__ == "__main__":
    main()
