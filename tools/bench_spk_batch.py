"""Speaker embeddings for a batch of clips against a loop of single calls, full depth (ResNet293); one JSON line.

    python tools/bench_spk_batch.py [--iters 7] [--warmup 2]

Workloads: B in {1, 4, 16} equal 10 s stereo 44.1 kHz clips, and one ragged set of 16 clips of 2 .. 30 s. Arms, in the
same process and alternated repeat by repeat: `loop` = B make_speaker_embedding calls (the single-clip path),
`batch` = one make_speaker_embeddings call. Each repeat is timed with a device event pair around at least 16 clips
(small B: the arm several times over); reported per workload are the per-clip ms of both arms (median, min, max of
--iters), the batch's split into front end / trunk / tail (each part timed on its own), the trunk's split by entry
point (one more pass with an event pair around every call, as tools/bench_spk.py's), the planner's groups and the
trunk's launches, counted at the library's entry points: calls (the 295 per clip of DESIGN.md §5f) and kernels (one
per conv and stem call, four per SimAM call that is handed the conv's sums). Checks (exit status 1 if one fails): the
batch's bits equal the loop's; a batch launches what one clip launches, per group; at B = 1 the two arms' medians
differ by no more than the loop arm's own min .. max spread.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from zonos_vibes_amd.config import tiny_transformer  # noqa: E402
from zonos_vibes_amd.model import Zonos  # noqa: E402
from zonos_vibes_amd.speaker import plan_lanes  # noqa: E402

SR = 44100


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms, clips):
    return dict(median=round(statistics.median(ms) / clips, 3), min=round(min(ms) / clips, 3),
                max=round(max(ms) / clips, 3))


class Launches:
    """Counts the trunk's kernel launches at the library's speaker entry points."""
    PER_CALL = {"zmi_spk_conv2d": 1, "zmi_spk_stem": 1, "zmi_spk_simam": 4,
                "zmi_spk_conv2d_lanes": 1, "zmi_spk_stem_lanes": 1, "zmi_spk_simam_lanes": 4}

    def __init__(self, lib, timed=False):
        self.lib, self.calls, self.kernels, self.timed, self.events = lib, 0, 0, timed, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in self.PER_CALL:
            return fn

        def call(*a):
            self.calls += 1
            self.kernels += self.PER_CALL[name]
            if not self.timed:
                return fn(*a)
            key = name[len("zmi_spk_"):].replace("_lanes", "")
            if key == "conv2d":  # k and stride sit at the same places in both forms
                key = f"conv{a[8]}x{a[8]}_s{a[9]}"
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            self.events.append((key, e0, e1))
            return rc
        return call

    def split_ms(self, clips):
        """Per entry point, the ms per clip between an event pair around every call (launch gaps included)."""
        torch.cuda.synchronize()
        out = {}
        for key, e0, e1 in self.events:
            out[key] = out.get(key, 0.0) + e0.elapsed_time(e1)
        return {k: round(v / clips, 3) for k, v in sorted(out.items())}


def count_launches(enc, fn, timed=False):
    """The wrapper after one run of fn: entry-point calls (DESIGN.md §5f's 295 per clip), kernels and, timed, events."""
    real, enc.lib = enc.lib, Launches(enc.lib, timed)
    try:
        fn()
        return enc.lib
    finally:
        enc.lib = real


def run(model, name, wavs, iters, warmup):
    enc = model.spk_clone_model
    B = len(wavs)
    inner = max(1, 16 // B)  # every timed window embeds at least 16 clips: 10 ms of work would time the clock
    loop = lambda: [[model.make_speaker_embedding(w, SR) for w in wavs] for _ in range(inner)][-1]  # noqa: E731
    batch = lambda: [model.make_speaker_embeddings(wavs, SR) for _ in range(inner)][-1]  # noqa: E731
    for _ in range(warmup):
        loop()
        batch()
    torch.cuda.synchronize()
    t_loop, t_batch = [], []
    for _ in range(iters):  # arms alternated
        ms, ref = event_ms(loop)
        t_loop.append(ms / inner)
        ms, got = event_ms(batch)
        t_batch.append(ms / inner)
    same = all(torch.equal(a, b) for a, b in zip(ref, got))
    feats = [enc.features(w, SR) for w in wavs]
    groups = plan_lanes([int(f.shape[1]) for f in feats])
    fronts = [[f.clone() for f in enc.front_lanes([feats[i] for i in g])] for g in groups]

    def tail():
        for fs in fronts:
            for fr in fs:
                e = enc.pool(fr) @ enc.bott_w.t() + enc.bott_b
                e @ enc.lda_w.t() + enc.lda_b

    parts = dict(front_end=lambda: [enc.features(w, SR) for w in wavs],
                 trunk=lambda: [enc.front_lanes([feats[i] for i in g]) for g in groups], tail=tail)
    split = {k: round(statistics.median(event_ms(fn)[0] for _ in range(iters)) / B, 3) for k, fn in parts.items()}
    one = count_launches(enc, lambda: enc.embed_features(feats[0]))
    n_batch = count_launches(enc, lambda: enc.embed_features_batch(feats))
    one, n_batch = (one.calls, one.kernels), (n_batch.calls, n_batch.kernels)
    trunk_split = count_launches(enc, parts["trunk"], timed=True).split_ms(B)
    lo, ba = stats(t_loop, B), stats(t_batch, B)
    frames = [int(f.shape[1]) for f in feats]
    return dict(workload=name, clips=B, frames=frames if name == "ragged" else frames[0],
                loop_ms_per_clip=lo, batch_ms_per_clip=ba, batch_over_loop=round(ba["median"] / lo["median"], 3),
                batch_split_ms_per_clip=split, batch_trunk_split_ms_per_clip=trunk_split,
                groups=[len(g) for g in groups], trunk_calls_one_clip=one[0],
                trunk_calls_batch=n_batch[0], kernels_one_clip=one[1], kernels_batch=n_batch[1],
                launches_ok=n_batch == tuple(n * len(groups) for n in one), bits_equal=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    model = Zonos.synthetic(tiny_transformer(2), "cuda", zero_eos=True, max_seqlen=96, max_prefill=48)
    g = torch.Generator().manual_seed(0)
    clip = lambda seconds: (torch.rand(2, int(seconds * SR), generator=g) * 1.8 - 0.9).cuda()  # noqa: E731
    model.make_speaker_embedding(clip(1.0), SR)  # creates the synthetic ResNet293
    rnd = random.Random(0)
    sets = [(f"equal_{b}", [clip(10.0) for _ in range(b)]) for b in (1, 4, 16)]
    sets.append(("ragged", [clip(rnd.uniform(2.0, 30.0)) for _ in range(16)]))
    rows = [run(model, name, wavs, args.iters, args.warmup) for name, wavs in sets]
    b1 = rows[0]
    spread = b1["loop_ms_per_clip"]["max"] - b1["loop_ms_per_clip"]["min"]
    b1_diff = abs(b1["batch_ms_per_clip"]["median"] - b1["loop_ms_per_clip"]["median"])
    recorded = json.load(open(os.path.join(REPO, "profiles", "spk_bench.json")))["ms_per_clip"]
    res = dict(benchmark="speaker embeddings, batch against a loop of single calls, ResNet293, stereo 44.1 kHz clips",
               iters=args.iters, warmup=args.warmup, workloads=rows,
               b1_loop_spread_ms=round(spread, 3),
               b1_batch_within_loop_spread=b1_diff <= spread,
               spk_bench_ms_per_clip=recorded,
               b1_loop_minus_spk_bench_ms=round(b1["loop_ms_per_clip"]["median"] - recorded, 3))
    print(json.dumps(res))
    ok = res["b1_batch_within_loop_spread"] and all(r["launches_ok"] and r["bits_equal"] for r in rows)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
