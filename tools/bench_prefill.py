"""The prefill's attention, prefill_attn="rows" (one query per row: the decode kernels) against "tiles"
(zmi_attention_prefill), in one process with the arms alternated; one JSON document.

    python tools/bench_prefill.py [--iters 5] [--out profiles/prefill_attn_bench.json]

Zonos.synthetic(zonos_v01_transformer()) at four prefill shapes: C2 (Lc 160, S 161), C5 (Lc 160 + a 430-frame
audio prefix, S 591), a 30 s prefix (2,584 frames, S 2,745, max_prefill raised) and one serve()-style admission of
the first 64 C3 requests (Lc 8 + 15 s, S 39 .. 459) through prefill_many. Per shape and arm:

  prefill_event_ms      device-event time of engine.prefill / prefill_many (staging, the 26 layers, heads, first
                        sample) on the engine's stream: median of --iters, all repeats, spread = max - min
  attn_event_us         device-event time of the 26 layers' attention launches alone, back to back over the same
                        row / sequence tables (the table copy of the "tiles" arm is outside the timed span)
  kv_bytes, mfma        per layer, COUNTED from the shapes (prefill_table.prefill_counts), not measured
Kernel times from a profiler are not measured here.
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
from zonos_vibes_amd.config import zonos_v01_transformer  # noqa: E402
from zonos_vibes_amd.engine import SamplingParams, make_engine  # noqa: E402
from zonos_vibes_amd.model import Zonos  # noqa: E402
from zonos_vibes_amd.prefill_table import PREFILL_ATTN, prefill_counts  # noqa: E402

ARMS = ("rows", "tiles")
N_NEW = 8


def event_ms(stream, run) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    a.record(stream)
    run()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def passes_of(e, lens) -> list:
    """The sequences of each pass prefill_many makes of utterances of `lens` rows (slot i = utterance i)."""
    out, cur, rows = [], [], 0
    for slot, n in enumerate(lens):
        if cur and rows + 2 * n > e.pre_rows:
            out.append(cur)
            cur, rows = [], 0
        cur += e._slot_seqs(slot, rows, n)
        rows += 2 * n
    return out + [cur]


def attention_alone(e, passes) -> float:
    """Event time (us) of every layer's prefill attention over the passes' tables, in the engine's current arm."""
    staged = []
    with torch.cuda.stream(e.stream):
        for seqs in passes:
            m = sum(n for _, n, _, _ in seqs)
            pos = torch.cat([torch.arange(p0, p0 + n, dtype=torch.int32) for _, n, _, p0 in seqs])
            kv = torch.cat([torch.full((n,), r, dtype=torch.int32) for _, n, r, _ in seqs])
            staged.append((m, max(p0 + n for _, n, _, p0 in seqs) - 1, pos.to(e.dev), kv.to(e.dev),
                           e._prefill_table(seqs)))

    def run():
        with torch.cuda.stream(e.stream):
            for m, max_pos, pos, kv, table in staged:
                e.row_pos_pre[:m] = pos
                e.row_kv_pre[:m] = kv
                for i in range(e.L):
                    e._prefill_attention(i, e.q_pre, m, e.row_kv_pre, e.row_pos_pre, max_pos, e.attn_pre, table)
    us = event_ms(e.stream, run) * 1e3
    e.check_errors()
    return us


def summary(v: list, nd: int) -> dict:
    return {"median": round(statistics.median(v), nd), "all": [round(x, nd) for x in v],
            "spread": round(max(v) - min(v), nd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert set(ARMS) == set(PREFILL_ATTN)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = zonos_v01_transformer()
    d = cfg.backbone.d_model
    long_p = 2584  # 30 s of 44.1 kHz audio at 512 samples per frame
    one = Zonos.synthetic(cfg, dev, seed=0, zero_eos=True, max_seqlen=LC + long_p + 1 + N_NEW + 16,
                          max_prefill=LC + long_p + 1).engine
    many = make_engine(cfg, dev, max_slots=64, max_seqlen=512, max_prefill=512)  # serve()'s shipped max_prefill
    many.w = one.w
    many._build_plan()
    sp = SamplingParams(temperature=0.0)
    g = torch.Generator().manual_seed(11)
    cond = cond_tensor(1, d, dev)

    def prefix(p):
        return torch.randint(0, 1024, (1, 9, p), generator=g).to(dev)

    lcs = c3_job(64)[0]
    c3_items = [(i, cond_tensor(100 + i, d, dev, lc=lc), None, N_NEW, sp) for i, lc in enumerate(lcs)]
    shapes = [
        ("C2", one, [(0, cond, None, N_NEW, sp)], f"Lc {LC}, no audio prefix, S {LC + 1}"),
        ("C5", one, [(0, cond, prefix(430), N_NEW, sp)], f"Lc {LC} + 430-frame prefix, S {LC + 431}"),
        ("prefix_30s", one, [(0, cond, prefix(long_p), N_NEW, sp)],
         f"Lc {LC} + {long_p}-frame (30 s) prefix, S {LC + long_p + 1}, max_prefill raised to {one.max_prefill}"),
        ("C3_admission_64", many, c3_items,
         f"64 C3 requests (Lc 8 + 15 s: S {min(lcs) + 1} .. {max(lcs) + 1}) through prefill_many, max_prefill 512"),
    ]
    res = {"model": "zonos-v0.1-transformer, synthetic weights, 26 layers, 16 / 4 heads x 128", "iters": args.iters,
           "arms": {"rows": "zmi_attention_pf, one query per row (the baseline: the parent commit's kernels)",
                    "tiles": "zmi_attention_prefill, 4 positions x 4 heads per MFMA tile"},
           "kernel_time": "not measured", "shapes": {}}
    for name, e, items, what in shapes:
        lens = [it[1].shape[1] + (0 if it[2] is None else it[2].shape[-1]) + 1 for it in items]
        passes = passes_of(e, lens)

        def prefill():
            got = e.prefill_many(items) if len(items) > 1 else [e.prefill(*items[0])]
            assert got == lens

        def done():
            e.stream.synchronize()
            e.check_errors()
            for it in items:
                e.release(it[0])

        t_pre = {a: [] for a in ARMS}
        t_att = {a: [] for a in ARMS}
        for rep in range(args.iters + 1):  # the first round warms up
            for a in ARMS:
                e.prefill_attn = a
                ms = event_ms(e.stream, prefill)
                done()
                us = attention_alone(e, passes)
                if rep:
                    t_pre[a].append(ms)
                    t_att[a].append(us)
        counts = [prefill_counts(seqs, 4, 4) for seqs in passes]
        ent = {"what": what, "sequences": 2 * len(items), "n_rows": 2 * sum(lens), "passes": len(passes)}
        for a in ARMS:
            ent[a] = {"prefill_event_ms": summary(t_pre[a], 3), "attn_event_us": summary(t_att[a], 1),
                      "kv_bytes_per_layer_counted": sum(c[a]["kv_bytes"] for c in counts),
                      "mfma_per_layer_counted": sum(c[a]["mfma"] for c in counts)}
        ent["attn_ratio_tiles_over_rows"] = round(ent["tiles"]["attn_event_us"]["median"] /
                                                  ent["rows"]["attn_event_us"]["median"], 4)
        ent["prefill_ratio_tiles_over_rows"] = round(ent["tiles"]["prefill_event_ms"]["median"] /
                                                     ent["rows"]["prefill_event_ms"]["median"], 4)
        res["shapes"][name] = ent
        print(name, json.dumps(ent), flush=True)
    doc = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(doc + "\n")
    else:
        print(doc)


if __name__ == "__main__":
    main()
