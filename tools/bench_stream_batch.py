"""Batched streaming benchmark: Zonos.stream_batch() against generate_batch() + decode() on the bench's C3 share, and
the batched DAC window against replays of the single-lane window graph. One JSON line.

    python tools/bench_stream_batch.py [--iters 2] [--warmup 1] [--utterances 64] [--slots 64] [--skip-e2e]
                                       [--out profiles/stream_batch_bench.json]

window_decode_ms, per lane count B (chunk_frames 16: 36-frame windows, B distinct code windows), wall time from the
first enqueue to device idle, median of --window-reps, the arms alternated:
  single_graph_x_B     B replays of the single-lane window graph (_WindowDecoder, what stream() runs)
  lanes                one _decode_lanes over B lanes, its 31 launches (B = 1: the single-lane graph, the route
                       DACBatchStreamDecoder gives a window alone in its shape)
  ratio = lanes / single_graph_x_B; bit_equal: every lane equals its single-lane window

end_to_end: utterances 0 .. n - 1 of the 512-utterance C3 set (bench.c3_job: 2-30 s, Lc 8 + 15 s) on `slots` slots,
greedy, EOS suppressed, the arms alternated after a warm-up:
  offline              generate_batch() + decode() of every utterance (bench.time_c3_sharded's work on one GPU)
  stream_batch         consumed without looking at the chunks: wall_s, rtf = audio s / wall s, ratio_vs_offline
  paced                every item waited for as a player would: first_audio_ms (call to an utterance's first samples
                       complete on the device: min / median / p90 / max over the utterances), max_gap_ms (largest time
                       between two consecutive chunks of one utterance, worst over utterances and runs) against
                       chunk_audio_ms
  bit_equal_utterances utterances whose concatenated chunks are torch.equal to decode(generate_batch()[i])
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
from zonos_vibes_amd.autoencoder import (DAC_LOOKAHEAD_FRAMES, DACAutoencoder, _BatchWindowDecoder,  # noqa: E402
                                         _WindowDecoder)
from zonos_vibes_amd.config import DAC_HOP, DAC_SAMPLE_RATE, zonos_v01_transformer  # noqa: E402
from zonos_vibes_amd.model import Zonos  # noqa: E402

LANES = (1, 8, 32, 64)
CHUNK = 16


def window_decode(ae: DACAutoencoder, reps: int) -> dict:
    R = DAC_LOOKAHEAD_FRAMES
    W = 2 * R + CHUNK
    codes = torch.randint(0, 1024, (max(LANES), 9, W), generator=torch.Generator().manual_seed(CHUNK)).to(ae.dev)
    single = _WindowDecoder(ae, CHUNK, True)
    dec = _BatchWindowDecoder(ae, max(LANES), CHUNK)
    out = {}
    for B in LANES:
        wins = [(codes[b], R, R + CHUNK) for b in range(B)]

        def run_single():
            return [single(*w) for w in wins]

        def run_lanes():
            return dec._group([w[0] for w in wins], W, R, R + CHUNK) if B > 1 else [dec.single(*wins[0])]

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(ae.stream):
                res = fn()
            ae.stream.synchronize()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, res

        ms = dict(single_graph_x_B=[], lanes=[])
        equal = True
        for i in range(reps + 2):
            t, ref = timed(run_single)
            if i >= 2:
                ms["single_graph_x_B"].append(t)
            t, got = timed(run_lanes)
            if i >= 2:
                ms["lanes"].append(t)
            equal = equal and all(torch.equal(g, r) for g, r in zip(got, ref))
        med = {k: statistics.median(v) for k, v in ms.items()}
        out[str(B)] = dict({k: round(v, 3) for k, v in med.items()},
                           ratio=round(med["lanes"] / med["single_graph_x_B"], 3), bit_equal=bool(equal))
    return out


def end_to_end(args, dev) -> dict:
    cfg = zonos_v01_transformer()
    model = Zonos.synthetic(cfg, dev, seed=0, zero_eos=True, max_seqlen=bench.LC + bench.N_NEW + 9,
                            max_prefill=bench.LC + 1)
    n, slots = args.utterances, args.slots
    lcs, n_new = (v[:n] for v in bench.c3_job())
    d = cfg.backbone.d_model
    conds = [bench.cond_tensor(1000 + i, d, dev, lc) for i, lc in enumerate(lcs)]
    model._ensure_capacity(slots, max(lcs) + max(n_new) + 9, max(lcs) + 1)
    kw = dict(max_new_tokens=n_new, sampling_params=dict(temperature=0.0), seeds=list(range(n)), max_slots=slots)
    audio_s = sum(n_new) * DAC_HOP / DAC_SAMPLE_RATE
    cur = torch.cuda.current_stream(dev)

    def offline(keep=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codes = model.generate_batch(conds, **kw)
        t1 = time.perf_counter()
        wavs = [model.autoencoder.decode(c) for c in codes]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return t2 - t0, t1 - t0, wavs if keep else None

    def stream_total(keep=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        items = list(model.stream_batch(conds, chunk_frames=CHUNK, **kw))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, items if keep else len(items)

    def stream_paced():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stamps = [[] for _ in range(n)]
        for i, wav, last in model.stream_batch(conds, chunk_frames=CHUNK, **kw):
            if wav.shape[-1]:
                cur.synchronize()
                stamps[i].append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        first = sorted(s[0] for s in stamps)
        gap = max((b - a for s in stamps for a, b in zip(s, s[1:])), default=0.0)
        return first, gap, sum(len(s) for s in stamps)

    # warm-up: the decode graphs of every step size, the stage buffers of the window decoder, and the reference
    short = dict(kw, max_new_tokens=[4] * n)
    model.generate_batch(conds, **short)
    _, _, ref = offline(keep=True)
    _, items = stream_total(keep=True)
    equal = 0
    for i in range(n):
        mine = [w for j, w, _ in items if j == i]
        equal += bool(torch.equal(torch.cat(mine, dim=-1), ref[i]))
    lasts = sum(1 for _, _, last in items if last)
    del items, ref
    for _ in range(max(args.warmup - 1, 0)):
        offline()
        stream_total()
    off, gen, tot, firsts, gaps, nitems = [], [], [], [], [], 0
    for _ in range(args.iters):
        t, g, _ = offline()
        off.append(t)
        gen.append(g)
        t, nitems = stream_total()
        tot.append(t)
        f, gp, _ = stream_paced()
        firsts.append(f)
        gaps.append(gp)
    off_s, tot_s = statistics.median(off), statistics.median(tot)
    first = firsts[len(firsts) // 2]
    pct = lambda q: round(first[min(int(q * len(first)), len(first) - 1)], 1)  # noqa: E731
    dec = model._stream_batch_decoders[(id(model.autoencoder), CHUNK, False)].decode_windows
    chunk_ms = CHUNK * DAC_HOP / DAC_SAMPLE_RATE * 1e3
    return dict(workload=f"C3 share: utterances 0..{n - 1} of the 512-utterance C3 set (2-30 s, Lc 8 + 15 s), {slots} "
                         f"slots on one GPU, greedy, EOS suppressed, chunk_frames {CHUNK}",
                iters=args.iters, audio_s=round(audio_s, 1),
                offline=dict(wall_s=round(off_s, 3), wall_s_all=[round(v, 3) for v in off],
                             generate_s=round(statistics.median(gen), 3), rtf=round(audio_s / off_s, 2)),
                stream_batch=dict(wall_s=round(tot_s, 3), wall_s_all=[round(v, 3) for v in tot],
                                  rtf=round(audio_s / tot_s, 2), ratio_vs_offline=round(tot_s / off_s, 4),
                                  items=nitems, last_items=lasts),
                paced=dict(first_audio_ms=dict(min=pct(0), median=pct(0.5), p90=pct(0.9), max=pct(1.0)),
                           max_gap_ms=round(max(gaps), 1), chunk_audio_ms=round(chunk_ms, 2),
                           underrun_margin_ms=round(chunk_ms - max(gaps), 1)),
                window_launch_sequences=dec.lane_launches, windows_in_them=dec.lanes_decoded,
                single_lane_windows=dec.single.graph_replays,
                bit_equal_utterances=f"{equal}/{n}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--window-reps", type=int, default=20)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = dict(lookahead_frames=DAC_LOOKAHEAD_FRAMES, chunk_frames=CHUNK,
               window_decode_ms=window_decode(DACAutoencoder(dev), args.window_reps))
    if not args.skip_e2e:
        res["end_to_end"] = end_to_end(args, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
