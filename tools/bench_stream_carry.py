"""Carried-state streaming DAC decoder against the window decoder, both arms in one process, alternated. One JSON line.

    python tools/bench_stream_carry.py [--reps 20] [--iters 2] [--lanes 64] [--skip-batch] [--skip-stream]
                                       [--out profiles/stream_carry_bench.json]

steady_round_ms, per chunk_frames in (16, 8, 4, 1): `lanes` lanes of a stream_decoder_batch past their start, ONE
push of chunk_frames frames to every lane; wall time from the first enqueue to device idle; median, min and max of
--reps, the arms alternated; ratio = carry / window; bit_equal: every lane's samples of the timed pushes are
torch.equal between the arms.
memory: the carried state per lane and the scratch per lane-frame of a steady step (bytes).
stream_batch: utterances 0 .. n - 1 of the 512-utterance C3 set on `lanes` slots (tools/bench_stream_batch.py's
workload), greedy, EOS suppressed, chunk_frames 16, stream_batch(decoder=...) consumed without looking at the
chunks: wall_s, rtf = audio s / wall s.
stream: Zonos.stream() at the C2 configuration (tools/bench_stream.py's), chunk_frames 16, 8 and 4, per decoder:
total_ms (consumed without looking) and first_audio_ms (call to the first chunk complete on the device), medians.
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
from zonos_vibes_amd.autoencoder import DAC_LOOKAHEAD_FRAMES, DACAutoencoder  # noqa: E402
from zonos_vibes_amd.config import DAC_HOP, DAC_SAMPLE_RATE, zonos_v01_transformer  # noqa: E402
from zonos_vibes_amd.model import Zonos  # noqa: E402

ROUND_CHUNKS = (16, 8, 4, 1)
STREAM_CHUNKS = (16, 8, 4)
ARMS = ("window", "carry")


def spread(v, nd=3):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def steady_rounds(ae: DACAutoencoder, lanes: int, reps: int) -> dict:
    out = {}
    for chunk in ROUND_CHUNKS:
        total = 2 * DAC_LOOKAHEAD_FRAMES + chunk * (reps + 4)
        codes = torch.randint(0, 1024, (lanes, 9, total), generator=torch.Generator().manual_seed(chunk)).to(ae.dev)
        decs = {arm: ae.stream_decoder_batch(lanes, chunk, carry=arm == "carry") for arm in ARMS}
        at = 2 * DAC_LOOKAHEAD_FRAMES
        for dec in decs.values():  # past the start: every stage's frontier has left 0 and frames are being emitted
            dec.push({lane: codes[lane, :, :at] for lane in range(lanes)})
        ms = {arm: [] for arm in ARMS}
        equal = True
        for i in range(reps + 2):
            got = {}
            for arm, dec in decs.items():
                push = {lane: codes[lane, :, at: at + chunk] for lane in range(lanes)}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got[arm] = dec.push(push)
                torch.cuda.synchronize()
                if i >= 2:
                    ms[arm].append((time.perf_counter() - t0) * 1e3)
            equal = equal and all(torch.equal(got["window"][lane], got["carry"][lane]) and
                                  got["carry"][lane].shape[-1] == DAC_HOP * chunk for lane in range(lanes))
            at += chunk
        for dec in decs.values():
            for lane in range(lanes):
                dec.reset(lane)
        out[str(chunk)] = dict(window_ms=spread(ms["window"]), carry_ms=spread(ms["carry"]),
                               ratio=round(statistics.median(ms["carry"]) / statistics.median(ms["window"]), 3),
                               bit_equal=bool(equal))
        del decs
        torch.cuda.empty_cache()
    return out


def memory(ae: DACAutoencoder) -> dict:
    steps = ae.stream_decoder_batch(1, 16, carry=True).decode_steps
    lay = steps.state.layout
    res = dict(state_bytes_per_lane=steps.state.state_bytes_per_lane(), scratch_bytes_per_lane_frame={})
    for chunk in ROUND_CHUNKS:
        plan = lay.step_plan(4 * lay.R, chunk)
        res["scratch_bytes_per_lane_frame"][str(chunk)] = round(2 * steps.state.scratch_halfs(plan, 1)[1] / chunk)
    res["window_stage_bytes_per_lane"] = {str(c): 4 * 2 * 49152 * (2 * DAC_LOOKAHEAD_FRAMES + c) for c in ROUND_CHUNKS}
    return res


def stream_batch(model: Zonos, args, dev) -> dict:
    n, slots = args.utterances, args.lanes
    lcs, n_new = (v[:n] for v in bench.c3_job())
    d = model.config.backbone.d_model
    conds = [bench.cond_tensor(1000 + i, d, dev, lc) for i, lc in enumerate(lcs)]
    model._ensure_capacity(slots, max(lcs) + max(n_new) + 9, max(lcs) + 1)
    kw = dict(max_new_tokens=n_new, sampling_params=dict(temperature=0.0), seeds=list(range(n)), max_slots=slots)
    audio_s = sum(n_new) * DAC_HOP / DAC_SAMPLE_RATE

    def run(arm, keep=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        items = list(model.stream_batch(conds, chunk_frames=16, decoder=arm, **kw))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, items if keep else None

    model.generate_batch(conds, **dict(kw, max_new_tokens=[4] * n))
    ref = {arm: run(arm, keep=True)[1] for arm in ARMS}  # warm-up, and the items compared
    equal = len(ref["window"]) == len(ref["carry"]) and all(
        i == j and la == lb and torch.equal(a, b) for (i, a, la), (j, b, lb) in zip(ref["window"], ref["carry"]))
    del ref
    wall = {arm: [] for arm in ARMS}
    for _ in range(args.iters):
        for arm in ARMS:
            wall[arm].append(run(arm)[0])
    res = dict(workload=f"C3 share: utterances 0..{n - 1} of the 512-utterance C3 set, {slots} slots on one GPU, greedy, "
                        "EOS suppressed, chunk_frames 16", iters=args.iters, audio_s=round(audio_s, 1),
               items_equal=bool(equal))
    for arm in ARMS:
        res[arm] = dict(wall_s=spread(wall[arm]), rtf=round(audio_s / statistics.median(wall[arm]), 2))
    res["ratio"] = round(statistics.median(wall["carry"]) / statistics.median(wall["window"]), 4)
    return res


def stream(model: Zonos, args, dev) -> dict:
    n_new = bench.N_NEW
    cond = bench.cond_tensor(1, model.config.backbone.d_model, dev)
    params = dict(temperature=0.0)
    cur = torch.cuda.current_stream(dev)

    def total(chunk, arm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chunks = list(model.stream(cond, max_new_tokens=n_new, sampling_params=params, chunk_frames=chunk, decoder=arm))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, chunks

    def first_audio(chunk, arm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gen = model.stream(cond, max_new_tokens=n_new, sampling_params=params, chunk_frames=chunk, decoder=arm)
        next(gen)
        cur.synchronize()
        t = (time.perf_counter() - t0) * 1e3
        gen.close()
        torch.cuda.synchronize()
        return t

    out = dict(workload=f"C2: zonos-v0.1-transformer synthetic, Lc {bench.LC}, {n_new} new frames, greedy, batch 1",
               iters=args.stream_iters)
    for chunk in STREAM_CHUNKS:
        ref = {arm: torch.cat(total(chunk, arm)[1], dim=-1) for arm in ARMS}  # warm-up
        for arm in ARMS:
            first_audio(chunk, arm)
        tot, first = {a: [] for a in ARMS}, {a: [] for a in ARMS}
        for _ in range(args.stream_iters):
            for arm in ARMS:
                tot[arm].append(total(chunk, arm)[0])
                first[arm].append(first_audio(chunk, arm))
        out[str(chunk)] = {arm: dict(total_ms=spread(tot[arm], 2), first_audio_ms=spread(first[arm], 2)) for arm in ARMS}
        out[str(chunk)]["ratio_total"] = round(statistics.median(tot["carry"]) / statistics.median(tot["window"]), 4)
        out[str(chunk)]["bit_equal"] = bool(torch.equal(ref["window"], ref["carry"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--stream-iters", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=64)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--skip-batch", action="store_true")
    ap.add_argument("--skip-stream", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ae = DACAutoencoder(dev)
    res = dict(lookahead_frames=DAC_LOOKAHEAD_FRAMES, lanes=args.lanes, reps=args.reps, memory=memory(ae),
               steady_round_ms=steady_rounds(ae, args.lanes, args.reps))
    del ae
    if not (args.skip_batch and args.skip_stream):
        cfg = zonos_v01_transformer()
        model = Zonos.synthetic(cfg, dev, seed=0, zero_eos=True, max_seqlen=bench.LC + bench.N_NEW + 9,
                                max_prefill=bench.LC + 1)
        if not args.skip_stream:
            res["stream"] = stream(model, args, dev)
        if not args.skip_batch:
            res["stream_batch"] = stream_batch(model, args, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
