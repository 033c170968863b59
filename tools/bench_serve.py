"""Serving benchmark: Zonos.serve() against stream_batch() on the bench's C3 share, request arrivals replayed on the
wall clock, and the PCM16 egress against per-item copies + CPU conversion. One JSON line.

    python tools/bench_serve.py [--iters 2] [--utterances 64] [--slots 64] [--rate 16] [--egress-reps 20]
                                [--out profiles/serve_bench.json]

session_cost: utterances 0 .. n - 1 of the 512-utterance C3 set on `slots` slots, greedy, EOS suppressed, chunk_frames
16 (tools/bench_stream_batch.py's end_to_end workload). Everything is submitted before the first round in
stream_batch()'s longest-first order, so both arms run the same rounds; fp32 device chunks in both; arms alternated
in one process after a warm-up, median of --iters:
  stream_batch         wall_s, wall_s_all, spread_s (max - min of its own repeats)
  serve                the same of a session opened, drained with run_round() and closed
  delta_s              serve - stream_batch (medians); within_2x_spread: |delta_s| <= 2 spread_s of stream_batch
  bit_equal_utterances tickets whose chunks concatenated are torch.equal to stream_batch()'s for that utterance
arrivals: the same requests with seeded exponential inter-arrival gaps at --rate requests / s, in the set's order,
replayed on the wall clock from the driving thread (what has arrived is submitted before each round; wait_for_work
when idle), pcm16 = True:
  first_audio_ms       per request, arrival to its first audio complete on the host as int16: min / median / p90 / max
  rtf                  audio s / wall s from the first arrival to the last chunk; rounds; last_arrival_s
egress: one round's audio at `slots` lanes x chunk_frames frames, from "windows decoded" (fp32 on the device, device
idle) to "all chunks on the host as int16", arms alternated, median and spread (max - min) of --egress-reps:
  pcm16_pack           Pcm16Egress: one zmi_pcm16_pack launch, one copy, one event, then a host copy per chunk
  per_item_cpu         what a stream_batch() consumer does: .cpu() per item, then clamp, scale and cast on the CPU
                       (torch, 16 threads)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402
from zonos_vibes_amd.config import DAC_HOP, DAC_SAMPLE_RATE, zonos_v01_transformer  # noqa: E402
from zonos_vibes_amd.model import Zonos  # noqa: E402
from zonos_vibes_amd.serving import Pcm16Egress  # noqa: E402

CHUNK = 16
GREEDY = dict(temperature=0.0)


def spread(v):
    return max(v) - min(v)


def session_cost(model, conds, n_new, slots, iters) -> dict:
    n = len(conds)
    kw = dict(max_new_tokens=n_new, sampling_params=GREEDY, seeds=list(range(n)), max_slots=slots)
    order = sorted(range(n), key=lambda i: -n_new[i])  # stream_batch's queue
    cap = dict(max_seqlen=model.engine.smax, max_prefill=model.engine.max_prefill)

    def arm_stream(keep=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        items = list(model.stream_batch(conds, chunk_frames=CHUNK, **kw))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, items if keep else None

    def arm_serve(keep=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        items = []
        with model.serve(slots, chunk_frames=CHUNK, **cap) as session:
            owner = {session.submit(conds[i], max_new_tokens=n_new[i], sampling_params=GREEDY, seed=i): i
                     for i in order}
            while not session.idle:
                items += session.run_round()
            rounds = session.rounds_run
        torch.cuda.synchronize()
        return time.perf_counter() - t0, [(owner[t], w, last) for t, w, last in items] if keep else None, rounds

    _, ref = arm_stream(keep=True)  # warm-up of both arms, and the equality
    _, got, rounds = arm_serve(keep=True)
    equal = sum(bool(torch.equal(torch.cat([w for j, w, _ in got if j == i], dim=-1),
                                 torch.cat([w for j, w, _ in ref if j == i], dim=-1))) for i in range(n))
    lasts = sum(1 for _, _, last in got if last)
    del ref, got
    a, b = [], []
    for _ in range(iters):
        a.append(arm_stream()[0])
        b.append(arm_serve()[0])
    ma, mb = statistics.median(a), statistics.median(b)
    return dict(iters=iters, rounds=rounds,
                stream_batch=dict(wall_s=round(ma, 4), wall_s_all=[round(v, 4) for v in a], spread_s=round(spread(a), 4)),
                serve=dict(wall_s=round(mb, 4), wall_s_all=[round(v, 4) for v in b], spread_s=round(spread(b), 4)),
                delta_s=round(mb - ma, 4), ratio=round(mb / ma, 4),
                within_2x_spread=bool(abs(mb - ma) <= 2 * spread(a)),
                last_items=lasts, bit_equal_utterances=f"{equal}/{n}")


def arrivals(model, conds, n_new, slots, rate, seed=0) -> dict:
    n = len(conds)
    gaps = np.random.default_rng(seed).exponential(1.0 / rate, n)
    at = np.cumsum(gaps) - gaps[0]  # the first request arrives at 0
    cap = dict(max_seqlen=model.engine.smax, max_prefill=model.engine.max_prefill)
    audio_s = sum(n_new) * DAC_HOP / DAC_SAMPLE_RATE

    def replay():
        first, nxt, t_end = {}, 0, 0.0
        torch.cuda.synchronize()
        with model.serve(slots, chunk_frames=CHUNK, pcm16=True, **cap) as session:
            t0 = time.perf_counter()
            while nxt < n or not session.idle:
                now = time.perf_counter() - t0
                while nxt < n and at[nxt] <= now:
                    session.submit(conds[nxt], max_new_tokens=n_new[nxt], sampling_params=GREEDY, seed=nxt)
                    nxt += 1
                if session.idle:  # nothing has arrived: sleep until the next arrival is due (no other submitter)
                    session.wait_for_work(timeout=max(at[nxt] - (time.perf_counter() - t0), 0.0))
                    continue
                for t, w, _ in session.run_round():
                    t_end = time.perf_counter() - t0
                    if w.shape[-1] and t not in first:
                        first[t] = (t_end - at[t]) * 1e3  # tickets count up in submission = arrival order
            rounds = session.rounds_run
        return sorted(first.values()), t_end, rounds

    replay()  # warm-up: the decode graphs of the row counts and forms arrivals go through
    first, wall, rounds = replay()
    pct = lambda q: round(first[min(int(q * len(first)), len(first) - 1)], 1)  # noqa: E731
    return dict(rate_per_s=rate, seed=seed, last_arrival_s=round(float(at[-1]), 3), requests=n,
                first_audio_ms=dict(min=pct(0), median=pct(0.5), p90=pct(0.9), max=pct(1.0)),
                wall_s=round(wall, 3), rtf=round(audio_s / wall, 2), rounds=rounds)


def egress(dev, lanes, reps) -> dict:
    n = CHUNK * DAC_HOP
    g = torch.Generator().manual_seed(1)
    wavs = {s: (torch.rand(1, 1, n, generator=g) * 2.4 - 1.2).to(dev) for s in range(lanes)}
    eg = Pcm16Egress(dev, lanes, CHUNK)
    stream = torch.cuda.current_stream(dev)
    torch.set_num_threads(min(torch.get_num_threads(), 16))

    def arm_pack():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eg.enqueue(wavs, stream)
        out = eg.collect()
        return (time.perf_counter() - t0) * 1e3, out

    def arm_cpu():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = {s: (w.cpu().clamp(-1, 1) * 32767.0).to(torch.int16) for s, w in wavs.items()}
        return (time.perf_counter() - t0) * 1e3, out

    a, b, equal = [], [], True
    for i in range(reps + 2):
        ta, oa = arm_pack()
        tb, ob = arm_cpu()
        equal = equal and all(torch.equal(oa[s], ob[s]) for s in wavs)
        if i >= 2:
            a.append(ta)
            b.append(tb)
    ma, mb = statistics.median(a), statistics.median(b)
    return dict(lanes=lanes, samples_per_lane=n, reps=reps, cpu_threads=torch.get_num_threads(),
                pcm16_pack=dict(ms=round(ma, 3), spread_ms=round(spread(a), 3)),
                per_item_cpu=dict(ms=round(mb, 3), spread_ms=round(spread(b), 3)),
                ratio=round(ma / mb, 4), bit_equal=bool(equal))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--rate", type=float, default=16.0, help="arrivals: requests per second")
    ap.add_argument("--egress-reps", type=int, default=20)
    ap.add_argument("--only", choices=["session_cost", "arrivals", "egress"], default=None)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, slots = args.utterances, args.slots
    res = dict(chunk_frames=CHUNK,
               workload=f"C3 share: utterances 0..{n - 1} of the 512-utterance C3 set (2-30 s, Lc 8 + 15 s), {slots} "
                        f"slots on one GPU, greedy, EOS suppressed, chunk_frames {CHUNK}")
    if args.only in (None, "egress"):
        res["egress"] = egress(dev, slots, args.egress_reps)
    if args.only in (None, "session_cost", "arrivals"):
        cfg = zonos_v01_transformer()
        model = Zonos.synthetic(cfg, dev, seed=0, zero_eos=True, max_seqlen=bench.LC + bench.N_NEW + 9,
                                max_prefill=bench.LC + 1)
        lcs, n_new = (v[:n] for v in bench.c3_job())
        conds = [bench.cond_tensor(1000 + i, cfg.backbone.d_model, dev, lc) for i, lc in enumerate(lcs)]
        model._ensure_capacity(slots, max(lcs) + max(n_new) + 9, max(lcs) + 1)
        res["audio_s"] = round(sum(n_new) * DAC_HOP / DAC_SAMPLE_RATE, 1)
        model.generate_batch(conds, max_new_tokens=[4] * n, sampling_params=GREEDY, seeds=list(range(n)),
                             max_slots=slots)
        if args.only in (None, "session_cost"):
            res["session_cost"] = session_cost(model, conds, list(n_new), slots, args.iters)
        if args.only in (None, "arrivals"):
            res["arrivals"] = arrivals(model, conds, list(n_new), slots, args.rate)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
