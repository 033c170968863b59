"""Resampling benchmark: the one-shot zmi_resample of a 10 s clip, and what sample_rate= costs a serving session.
One JSON line.

    python tools/bench_resample.py [--iters 3] [--utterances 64] [--slots 64] [--reps 50]
                                   [--out profiles/resample_bench.json]

one_shot: DACAutoencoder.resample of a 10 s mono clip, 48 kHz -> 44.1 kHz (480000 -> 441000 samples), device to
device, host-timed around a synchronize; median and spread (max - min) of --reps after a warm-up; bound_ok: the result
is within the fp32 chain bound of the fp64 evaluation of the same table.
serve: tools/bench_serve.py's up-front arm (utterances 0 .. n - 1 of the C3 set, all submitted before the first round,
`slots` slots, greedy, EOS suppressed, chunk_frames 16) with pcm16 = True, at sample_rate = 24000 against
sample_rate = None (the session as it was before the keyword) in one process, arms alternated after a warm-up of both:
  none / at_24k   wall_s (median), wall_s_all, spread_s (max - min of the arm's own repeats)
  delta_s, ratio  at_24k - none, at_24k / none (medians)
  samples         int16 samples handed out by each arm (24000 / 44100 of the other, up to one sample a ticket)
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

import bench  # noqa: E402
from zonos_vibes_amd.config import DAC_HOP, DAC_SAMPLE_RATE, zonos_v01_transformer  # noqa: E402
from zonos_vibes_amd.model import Zonos  # noqa: E402

CHUNK = 16
GREEDY = dict(temperature=0.0)
RATE = 24000


def spread(v):
    return max(v) - min(v)


def one_shot(ae, dev, reps) -> dict:
    from zonos_vibes_amd import resampling as rs
    from zonos_vibes_amd.speaker import resample_kernel
    orig, new, n = 48000, DAC_SAMPLE_RATE, 480000
    x = (torch.rand(1, 1, n, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    y = ae.resample(x, orig, new)  # warm-up: the table goes to the device
    o, m, W, T = rs.resample_plan(orig, new)
    kern = resample_kernel(o, m)[0].double()
    xp = torch.nn.functional.pad(x.cpu().double().view(-1), (W, W + o))
    fr = xp.unfold(-1, T, o)
    ref = (fr @ kern.t()).reshape(-1)[: y.shape[-1]]
    bound = (T + 2) * 2.0 ** -24 * (fr.abs() @ kern.abs().t()).reshape(-1)[: y.shape[-1]] + 1e-30
    ok = bool(((y.cpu().double().view(-1) - ref).abs() <= bound).all())
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ae.resample(x, orig, new)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(orig=orig, new=new, samples_in=n, samples_out=int(y.shape[-1]), reps=reps,
                ms=round(statistics.median(ms), 4), spread_ms=round(spread(ms), 4), min_ms=round(min(ms), 4),
                bound_ok=ok)


def serve(model, conds, n_new, slots, iters) -> dict:
    n = len(conds)
    order = sorted(range(n), key=lambda i: -n_new[i])
    cap = dict(max_seqlen=model.engine.smax, max_prefill=model.engine.max_prefill)

    def arm(rate):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        samples = lasts = 0
        with model.serve(slots, chunk_frames=CHUNK, pcm16=True, sample_rate=rate, **cap) as session:
            for i in order:
                session.submit(conds[i], max_new_tokens=n_new[i], sampling_params=GREEDY, seed=i)
            while not session.idle:
                for _, w, last in session.run_round():
                    samples += w.shape[-1]
                    lasts += bool(last)
            rounds = session.rounds_run
        torch.cuda.synchronize()
        return time.perf_counter() - t0, samples, lasts, rounds

    _, s0, l0, rounds = arm(None)  # warm-up of both arms
    _, s1, l1, _ = arm(RATE)
    a, b = [], []
    for _ in range(iters):
        a.append(arm(None)[0])
        b.append(arm(RATE)[0])
    ma, mb = statistics.median(a), statistics.median(b)
    return dict(iters=iters, rounds=rounds, sample_rate=RATE, pcm16=True,
                none=dict(wall_s=round(ma, 4), wall_s_all=[round(v, 4) for v in a], spread_s=round(spread(a), 4)),
                at_24k=dict(wall_s=round(mb, 4), wall_s_all=[round(v, 4) for v in b], spread_s=round(spread(b), 4)),
                delta_s=round(mb - ma, 4), ratio=round(mb / ma, 4),
                samples=dict(none=s0, at_24k=s1), last_items=dict(none=l0, at_24k=l1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", choices=["one_shot", "serve"], default=None)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, slots = args.utterances, args.slots
    res = dict(chunk_frames=CHUNK)
    cfg = zonos_v01_transformer()
    if args.only == "one_shot":
        from zonos_vibes_amd.autoencoder import DACAutoencoder
        res["one_shot"] = one_shot(DACAutoencoder(dev), dev, args.reps)
    else:
        model = Zonos.synthetic(cfg, dev, seed=0, zero_eos=True, max_seqlen=bench.LC + bench.N_NEW + 9,
                                max_prefill=bench.LC + 1)
        if args.only is None:
            res["one_shot"] = one_shot(model.autoencoder, dev, args.reps)
        lcs, n_new = (v[:n] for v in bench.c3_job())
        conds = [bench.cond_tensor(1000 + i, cfg.backbone.d_model, dev, lc) for i, lc in enumerate(lcs)]
        model._ensure_capacity(slots, max(lcs) + max(n_new) + 9, max(lcs) + 1)
        res["workload"] = (f"C3 share: utterances 0..{n - 1} of the 512-utterance C3 set, {slots} slots on one GPU, "
                           f"greedy, EOS suppressed, chunk_frames {CHUNK}, pcm16, all submitted before the first round")
        res["audio_s"] = round(sum(n_new) * DAC_HOP / DAC_SAMPLE_RATE, 1)
        model.generate_batch(conds, max_new_tokens=[4] * n, sampling_params=GREEDY, seeds=list(range(n)),
                             max_slots=slots)
        res["serve"] = serve(model, conds, list(n_new), slots, args.iters)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
