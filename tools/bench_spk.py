"""Speaker-encoder benchmark: embed a 10 s synthetic clip at full depth (ResNet293) and print one JSON line.

    python tools/bench_spk.py [--seconds 10] [--iters 5] [--warmup 2] [--no-cpu]

Fields: ms per clip (front end + trunk + tail, median of --iters), the trunk's achieved TFLOP/s over its analytic
FLOP count (2 Ho Wo Co Ci k^2 per conv), that as a fraction of the 2.5 PFLOP/s fp16 MFMA peak, the per-kernel split
(one extra pass with an event pair around every launch) and the time of the fp32 CPU restatement (tests/spk_cpu.py) of
the same clip on 16 threads.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from zonos_vibes_amd import synthetic as syn  # noqa: E402
from zonos_vibes_amd.speaker import SpeakerEmbeddingLDA, SpeakerEncoderConfig  # noqa: E402

PEAK_FP16 = 2.5e15


def trunk_flops(cfg: SpeakerEncoderConfig, frames: int) -> float:
    h, w = cfg.acoustic_dim, frames
    total = 2.0 * h * w * cfg.in_planes * 9
    for _, ci, co, s in syn.speaker_block_plan(cfg):
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        total += 2.0 * ho * wo * co * (ci * 9 + co * 9 + (ci if (s != 1 or ci != co) else 0))
        h, w = ho, wo
    return total


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


class Split:
    """Event pairs around the library's speaker entry points for one pass."""

    def __init__(self, lib):
        self.lib, self.events = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in ("zmi_spk_conv2d", "zmi_spk_simam", "zmi_spk_stem"):
            return fn

        def call(*a):
            key = name[len("zmi_spk_"):]
            if key == "conv2d":
                key = f"conv{a[8]}x{a[8]}_s{a[9]}"
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            self.events.append((key, e0, e1))
            return rc
        return call

    def totals(self):
        torch.cuda.synchronize()
        out = {}
        for key, e0, e1 in self.events:
            t = out.setdefault(key, dict(ms=0.0, launches=0))
            t["ms"] += e0.elapsed_time(e1)
            t["launches"] += 1
        return {k: dict(ms=round(v["ms"], 3), launches=v["launches"]) for k, v in sorted(out.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    cfg = SpeakerEncoderConfig()
    enc = SpeakerEmbeddingLDA("cuda", seed=0, config=cfg)
    n = int(args.seconds * 44100)
    wav = torch.rand(2, n, generator=torch.Generator().manual_seed(0)) * 1.8 - 0.9
    wav_d = wav.cuda()
    feat = enc.features(wav_d, 44100)
    frames = feat.shape[1]
    flops = trunk_flops(cfg, frames)
    clip_ms = timed(lambda: enc(wav_d, 44100), args.iters, args.warmup)
    trunk_ms = timed(lambda: enc.front(feat), args.iters, 1)
    front_end_ms = timed(lambda: enc.features(wav_d, 44100), args.iters, 1)
    real, enc.lib = enc.lib, Split(enc.lib)
    enc.front(feat)
    split = enc.lib.totals()
    enc.lib = real
    emb, lda = enc(wav_d, 44100)
    res = dict(workload=f"speaker embedding, {args.seconds:g} s stereo 44.1 kHz clip, ResNet293", frames=frames,
               ms_per_clip=round(clip_ms, 3), trunk_ms=round(trunk_ms, 3), front_end_ms=round(front_end_ms, 3),
               trunk_gflop=round(flops / 1e9, 1), tflops=round(flops / trunk_ms / 1e9, 2),
               frac_fp16_peak=round(flops / (trunk_ms * 1e-3) / PEAK_FP16, 4), kernels=split,
               lda_abs_max=round(float(lda.abs().max()), 4))
    if not args.no_cpu:
        import spk_cpu
        torch.set_num_threads(16)
        w = dict(syn.iter_torch_cpu(syn.speaker_specs(cfg), 0))
        lda_w = {k[4:]: w.pop(k) for k in list(w) if k.startswith("lda.")}
        cpu = spk_cpu.SpeakerCPU(w, lda_w, cfg.in_planes, cfg.num_blocks)
        t0 = time.perf_counter()
        f_cpu = spk_cpu.log_fbank(spk_cpu.resample(wav.mean(0, keepdim=True), 44100, 16000))
        e_cpu, l_cpu = cpu(f_cpu)
        res["cpu_restatement_s_16_threads"] = round(time.perf_counter() - t0, 2)
        res["cpu_threads"] = torch.get_num_threads()  # the limit in force while it ran
        res["cpu_model"] = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo")
                                 if ln.startswith("model name")), "unknown")
        res["lda_max_abs_diff_vs_cpu_fp32"] = float((lda.cpu() - l_cpu).abs().max())
        res["lda_cosine_vs_cpu_fp32"] = float(torch.nn.functional.cosine_similarity(lda.cpu(), l_cpu).item())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
