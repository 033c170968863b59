"""weights="fp8" against bf16 at the C2 configuration, in one process, one JSON line.

    python tools/bench_fp8.py [--iters 5] [--warmup 1] [--agree-frames 200] [--out profiles/fp8_bench.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_fp8.py --steps-only --iters 1 --agree-frames 0
        (a run of its own for the per-kernel times of fc1 / fc2 in both formats: decode steps only, a short trace)

Two Zonos.synthetic(zonos_v01_transformer()) models with the same seed, bf16 and fp8 MLP weights, bench.py's
conditioning (Lc 160, 861 new frames, greedy, EOS suppressed). After the warm-up the two arms are ALTERNATED (arms
closer than about 1 % must share their thermal and clock state). Fields, per arm:

  step_us            decode step of a live utterance at position 591 (bench.py's time_decode_step: 64 hipGraph replays
                     between device events), median of --iters; step_us_all the repeats, step_spread_us max - min
  step_bytes         algorithmic HBM bytes of that step: every weight once at its stored width (fp8: one byte per MLP
                     weight + one exponent per MLP column) + the KV cache up to the position
  step_hbm_frac      step_bytes / step time / 8 TB/s: a whole-step rate over the peak, not a kernel's share of it
  utterance_ms       generate() + decode(), call to device idle, median; utterance_ms_all, utterance_spread_ms
and: step_ratio / utterance_ratio / bytes_ratio (fp8 / bf16), faster_than_spread (bf16 - fp8 step time exceeds both arms'
spread), greedy_agreement: over the first --agree-frames frames, the fp8 model fed the bf16 model's frames (teacher
forcing), the fraction of its greedy decisions (frame, codebook) equal to the bf16 model's; synthetic weights only.
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

from bench import HBM_PEAK_GBS, LC, N_NEW, cond_tensor, step_bytes, time_decode_step  # noqa: E402
from zonos_vibes_amd.config import zonos_v01_transformer  # noqa: E402
from zonos_vibes_amd.engine import SamplingParams  # noqa: E402
from zonos_vibes_amd.model import Zonos  # noqa: E402

ARMS = ("bf16", "fp8")


def stored_step_bytes(model, pos: int) -> int:
    """bench.py's step_bytes with the MLP weights at their stored width."""
    e = model.engine
    b = step_bytes(model, pos)
    if e.weights == "fp8":
        mlp = e.L * (2 * e.F * e.d + e.d * e.F)
        b += -2 * mlp + sum(lw[k].numel() for lw in e.w["layers"] for k in ("fc1", "fc2"))
    return b


def greedy_agreement(mb, m8, cond, frames: int) -> dict:
    params = SamplingParams(temperature=0.0, cfg_scale=2.0)
    eb, e8 = mb.engine, m8.engine
    eb.prefill(0, cond, None, N_NEW, params)
    eb.step(frames, slots=1)
    eb.stream.synchronize()
    ref = eb.delayed[0].clone()
    eb.release(0)
    e8.prefill(0, cond, None, N_NEW, params)
    same = total = 0
    first = None
    for i in range(frames):
        with torch.cuda.stream(e8.stream):  # the bf16 model's frames, whatever the fp8 model chose so far
            e8.delayed[0] = ref
            e8.refresh_inputs()
        e8.step(1, use_graph=False, slots=1)
        e8.stream.synchronize()
        o = int(e8.st["offset"][0].item())
        want, got = ref[:, o], e8.delayed[0, :, o]
        real = want != 1025  # (codebooks still masked by the delay pattern are not decisions)
        eq = int((got[real] == want[real]).sum().item())
        same, total = same + eq, total + int(real.sum().item())
        if first is None and eq != int(real.sum().item()):
            first = i
    e8.check_errors()
    e8.release(0)
    return dict(frames=frames, decisions=total, equal=same, fraction=round(same / max(total, 1), 4),
                first_differing_frame=first, mode="teacher-forced on the bf16 model's frames, greedy",
                weights="synthetic (not measured on real weights)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--agree-frames", type=int, default=200)
    ap.add_argument("--steps-only", action="store_true", help="time the decode step only (kernel-trace runs)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = zonos_v01_transformer()
    models = {a: Zonos.synthetic(cfg, dev, seed=0, zero_eos=True, max_seqlen=LC + N_NEW + 9, max_prefill=LC + 1,
                                 weights=a) for a in ARMS}
    cond = cond_tensor(1, cfg.backbone.d_model, dev)
    params = dict(temperature=0.0)

    def utterance(m):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codes = m.generate(cond, max_new_tokens=N_NEW, sampling_params=params, progress_bar=False, chunk=128)
        wav = m.autoencoder.decode(codes)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, wav

    for _ in range(max(args.warmup, 1)):
        for a in ARMS:
            if not args.steps_only:
                utterance(models[a])
            time_decode_step(models[a], cond)
    step = {a: [] for a in ARMS}
    utt = {a: [] for a in ARMS}
    pos = None
    for _ in range(args.iters):
        for a in ARMS:
            us, pos = time_decode_step(models[a], cond)
            step[a].append(us)
        for a in ARMS:
            utt[a].append(0.0 if args.steps_only else utterance(models[a])[0])
    res = dict(workload=f"C2: zonos-v0.1-transformer synthetic, Lc {LC}, {N_NEW} new frames, greedy, batch 1",
               iters=args.iters, decode_step_pos=pos, hbm_peak_gbs=HBM_PEAK_GBS)
    for a in ARMS:
        us, b = statistics.median(step[a]), stored_step_bytes(models[a], pos)
        res[a] = dict(step_us=round(us, 1), step_us_all=[round(v, 1) for v in step[a]],
                      step_spread_us=round(max(step[a]) - min(step[a]), 1), step_bytes=b,
                      step_hbm_frac=round(b / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 3),
                      utterance_ms=round(statistics.median(utt[a]), 2), utterance_ms_all=[round(v, 2) for v in utt[a]],
                      utterance_spread_ms=round(max(utt[a]) - min(utt[a]), 2))
    res["step_ratio"] = round(res["fp8"]["step_us"] / res["bf16"]["step_us"], 4)
    res["utterance_ratio"] = None if args.steps_only else round(res["fp8"]["utterance_ms"] / res["bf16"]["utterance_ms"], 4)
    res["bytes_ratio"] = round(res["fp8"]["step_bytes"] / res["bf16"]["step_bytes"], 4)
    res["faster_than_spread"] = bool(res["bf16"]["step_us"] - res["fp8"]["step_us"] >
                                     max(res["bf16"]["step_spread_us"], res["fp8"]["step_spread_us"]))
    if args.agree_frames > 0:
        res["greedy_agreement"] = greedy_agreement(models["bf16"], models["fp8"], cond, args.agree_frames)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
