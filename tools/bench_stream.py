"""Streaming benchmark: Zonos.stream() against generate() + decode() at the C2 configuration, one JSON line.

    python tools/bench_stream.py [--iters 5] [--warmup 1] [--new-tokens 861] [--out profiles/stream_bench.json]

Zonos.synthetic(zonos_v01_transformer()), Lc 160, 861 new frames, bench.py's conditioning seed, greedy, EOS
suppressed. After the warm-up the arms are ALTERNATED in one process (offline, stream at chunk_frames 8 / 16 / 32,
again), because arms closer than about 1 % must share their thermal and clock state. Fields:

  offline_ms                 generate() + decode(), call to device idle, median of --iters
  per chunk_frames:
    total_ms                 stream() consumed without looking at the chunks, call to device idle, median
    ratio_vs_offline         total_ms / offline_ms (the acceptance figure: <= 1.03 at chunk_frames 16)
    first_audio_ms           call to the first chunk complete on the device (each chunk waited for), median
    max_gap_ms               largest time between two consecutive chunks' completion, worst over the runs
    chunk_audio_ms           audio duration of chunk_frames frames; underrun_margin_ms = chunk_audio_ms - max_gap_ms
    chunks                   chunks yielded
    bit_equal_runs           timed runs whose concatenated chunks are torch.equal to decode(generate()), of --iters
  stream_overlapped          the same fields with the DAC windows left to run beside the next decode steps
                             (Zonos._stream_overlap, off by default: the decode step's codes are then not reproducible)
  window_decode_us           one steady-state window (lookahead + chunk + lookahead frames), stream-ordered, as a
                             hipGraph replay (`captured`) and as its launches (`uncaptured`), alternated, median of 50
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

from bench import LC, N_NEW, cond_tensor  # noqa: E402
from zonos_vibes_amd.autoencoder import DAC_LOOKAHEAD_FRAMES, WINDOW_GRAPH  # noqa: E402
from zonos_vibes_amd.config import DAC_HOP, DAC_SAMPLE_RATE, zonos_v01_transformer  # noqa: E402
from zonos_vibes_amd.model import Zonos  # noqa: E402

CHUNKS = (8, 16, 32)


def window_decode_us(ae, chunk: int, reps: int = 50) -> dict:
    R = DAC_LOOKAHEAD_FRAMES
    W = 2 * R + chunk
    codes = torch.randint(0, 1024, (9, W), generator=torch.Generator().manual_seed(chunk)).to(ae.dev)
    wins = {name: ae.stream_decoder(chunk, capture=cap).decode_window
            for name, cap in (("captured", True), ("uncaptured", False))}
    out = {name: [] for name in wins}
    host = {name: [] for name in wins}
    ref = None
    for i in range(reps + 3):
        for name, win in wins.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            wav = win(codes, R, R + chunk)
            b.record()
            t1 = time.perf_counter()
            b.synchronize()
            if i >= 3:
                out[name].append(a.elapsed_time(b) * 1e3)
                host[name].append((t1 - t0) * 1e6)
            ref = wav.clone() if ref is None else ref
            assert torch.equal(wav, ref)
    return {name: dict(device_us=round(statistics.median(out[name]), 1),
                       host_enqueue_us=round(statistics.median(host[name]), 1)) for name in wins}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--new-tokens", type=int, default=N_NEW)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = zonos_v01_transformer()
    n_new = args.new_tokens
    model = Zonos.synthetic(cfg, dev, seed=0, zero_eos=True, max_seqlen=LC + n_new + 9, max_prefill=LC + 1)
    cond = cond_tensor(1, cfg.backbone.d_model, dev)
    params = dict(temperature=0.0)

    def offline():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codes = model.generate(cond, max_new_tokens=n_new, sampling_params=params, progress_bar=False, chunk=128)
        wav = model.autoencoder.decode(codes)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, wav

    def stream_total(arm):
        chunk, model._stream_overlap = arm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chunks = list(model.stream(cond, max_new_tokens=n_new, sampling_params=params, chunk_frames=chunk))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, chunks

    def stream_paced(arm):
        """Every chunk waited for as a player would: first-audio time and the gaps between completions."""
        chunk, model._stream_overlap = arm
        torch.cuda.synchronize()
        cur = torch.cuda.current_stream(dev)
        t0 = time.perf_counter()
        stamps = []
        for _ in model.stream(cond, max_new_tokens=n_new, sampling_params=params, chunk_frames=chunk):
            cur.synchronize()
            stamps.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        gaps = [b - a for a, b in zip(stamps, stamps[1:])]
        return stamps[0], max(gaps) if gaps else 0.0, len(stamps)

    arms = [(c, False) for c in CHUNKS] + [(16, True)]
    for _ in range(max(args.warmup, 1)):
        _, ref = offline()
        for arm in arms:
            stream_total(arm)
            stream_paced(arm)
    off, tot = [], {a: [] for a in arms}
    first, gap = {a: [] for a in arms}, {a: [] for a in arms}
    nchunks, equal = {}, {a: 0 for a in arms}
    for _ in range(args.iters):
        ms, wav = offline()
        off.append(ms)
        assert torch.equal(wav, ref)
        for arm in arms:
            ms, chunks = stream_total(arm)
            tot[arm].append(ms)
            equal[arm] += bool(torch.equal(torch.cat(chunks, dim=-1), ref))
            f, g, n = stream_paced(arm)
            first[arm].append(f)
            gap[arm].append(g)
            nchunks[arm] = n
    model._stream_overlap = False
    off_ms = statistics.median(off)
    res = dict(workload=f"C2: zonos-v0.1-transformer synthetic, Lc {LC}, {n_new} new frames, greedy, batch 1",
               iters=args.iters, lookahead_frames=DAC_LOOKAHEAD_FRAMES, window_graph_default=WINDOW_GRAPH,
               audio_s=round(n_new * DAC_HOP / DAC_SAMPLE_RATE, 3), offline_ms=round(off_ms, 2),
               offline_ms_all=[round(v, 2) for v in off], stream={}, stream_overlapped={}, window_decode_us={})
    for arm in arms:
        c, overlap = arm
        t = statistics.median(tot[arm])
        audio = c * DAC_HOP / DAC_SAMPLE_RATE * 1e3
        res["stream_overlapped" if overlap else "stream"][str(c)] = dict(
            total_ms=round(t, 2), total_ms_all=[round(v, 2) for v in tot[arm]], ratio_vs_offline=round(t / off_ms, 4),
            first_audio_ms=round(statistics.median(first[arm]), 2), max_gap_ms=round(max(gap[arm]), 2),
            chunk_audio_ms=round(audio, 2), underrun_margin_ms=round(audio - max(gap[arm]), 2), chunks=nchunks[arm],
            bit_equal_runs=f"{equal[arm]}/{args.iters}")
    for c in CHUNKS:
        res["window_decode_us"][str(c)] = window_decode_us(model.autoencoder, c)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
