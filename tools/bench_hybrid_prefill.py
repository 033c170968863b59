"""The hybrid's batched admission: a loop of prefill() (one pass through the 46 layers per utterance: what
HybridEngine did before its scan took ragged sequences) against prefill_many (the utterances' rows packed into
passes of up to pre_rows rows, zmi_mamba2_scan_seqs over each pass's sequence table), in one process with the arms
alternated; one JSON document.

    python tools/bench_hybrid_prefill.py [--iters 5] [--out profiles/hybrid_prefill_batch_bench.json]

Zonos.synthetic(zonos_v01_hybrid()), one 64-slot engine, four shapes: 1, 2 and 6 C4 utterances (Lc 160, S 161) and
one serve()-style admission of the first 64 C3 requests (Lc 8 + 15 s, S 39 .. 459: the requests of
tools/bench_prefill.py). Per shape and arm:

  admission_event_ms    device-event time of engine.prefill_many over the shape's items (staging, the layers, heads,
                        first samples) on the engine's stream: median of --iters, all repeats, spread = max - min
  per_utterance_ms      the median / utterances
  passes                calls of _prefill_layers, counted

The "loop" arm is the same engine with prefill_batch = False on the instance, so prefill_many returns through
prefill() per item; with one utterance both arms take that path (the single-utterance check). Kernel times from a
profiler are not measured here, nor is the first-audio latency of a serve() session.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bench import LC, c3_job, cond_tensor  # noqa: E402
from zonos_vibes_amd.config import zonos_v01_hybrid  # noqa: E402
from zonos_vibes_amd.engine import SamplingParams  # noqa: E402
from zonos_vibes_amd.model import Zonos  # noqa: E402

ARMS = ("loop", "many")
N_NEW = 8


def event_ms(stream, run) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    a.record(stream)
    run()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def summary(v: list, nd: int) -> dict:
    return {"median": round(statistics.median(v), nd), "all": [round(x, nd) for x in v],
            "spread": round(max(v) - min(v), nd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = zonos_v01_hybrid()
    d = cfg.backbone.d_model
    e = Zonos.synthetic(cfg, dev, seed=0, zero_eos=True, max_slots=64, max_seqlen=512, max_prefill=512).engine
    assert type(e).prefill_batch is True
    sp = SamplingParams(temperature=0.0)
    lcs = c3_job(64)[0]
    c4 = [(i, cond_tensor(1 + i, d, dev), None, N_NEW, sp) for i in range(6)]
    shapes = [(f"C4_x{n}", c4[:n], f"{n} C4 utterance{'s' if n > 1 else ''} (Lc {LC}, S {LC + 1})") for n in (1, 2, 6)]
    shapes.append(("C3_admission_64", [(i, cond_tensor(100 + i, d, dev, lc=lc), None, N_NEW, sp)
                                       for i, lc in enumerate(lcs)],
                   f"64 C3 requests (Lc 8 + 15 s: S {min(lcs) + 1} .. {max(lcs) + 1}), max_prefill 512"))
    passes, inner = [0], e._prefill_layers

    def counted(m, max_pos, seqs):
        passes[0] += 1
        return inner(m, max_pos, seqs)
    e._prefill_layers = counted
    res = {"model": "zonos-v0.1-hybrid dims, synthetic weights, 46 layers (41 Mamba2 + MHA at 9/18/27/36/45)",
           "iters": args.iters, "pre_rows": e.pre_rows,
           "arms": {"loop": "prefill() per utterance (prefill_batch = False on the instance: one pass per utterance)",
                    "many": "prefill_many: the rows packed into passes, zmi_mamba2_scan_seqs over each pass's table"},
           "kernel_time": "not measured", "serve_first_audio_latency": "not measured", "shapes": {}}
    for name, items, what in shapes:
        lens = [it[1].shape[1] + 1 for it in items]
        t = {a: [] for a in ARMS}
        n_pass = {}
        for rep in range(args.iters + 1):  # the first round warms up
            for a in ARMS:
                e.prefill_batch = a == "many"
                passes[0] = 0

                def run():
                    assert e.prefill_many(items) == lens
                ms = event_ms(e.stream, run)
                e.stream.synchronize()
                e.check_errors()
                for it in items:
                    e.release(it[0])
                n_pass[a] = passes[0]
                if rep:
                    t[a].append(ms)
        ent = {"what": what, "utterances": len(items), "sequences": 2 * len(items), "n_rows": 2 * sum(lens)}
        for a in ARMS:
            s = summary(t[a], 3)
            ent[a] = {"admission_event_ms": s, "per_utterance_ms": round(s["median"] / len(items), 3),
                      "passes": n_pass[a]}
        ent["ratio_many_over_loop"] = round(ent["many"]["admission_event_ms"]["median"] /
                                            ent["loop"]["admission_event_ms"]["median"], 4)
        res["shapes"][name] = ent
        print(name, json.dumps(ent), flush=True)
    del e.prefill_batch
    doc = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(doc + "\n")
    else:
        print(doc)


if __name__ == "__main__":
    main()
