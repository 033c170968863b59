"""Chunked prefill (prefill_chunk = C) measured: what cutting a long prompt into chunks costs or gains in the prefill
itself, and what it does to a serving session that a long-prompt request joins. One JSON document.

    python tools/bench_prefill_chunk.py [--iters 5] [--serve-iters 2] [--only prefill|serve]
                                        [--out profiles/prefill_chunk_bench.json]

prefill: Zonos.synthetic at the full-size transformer and hybrid dims, one prompt of Lc 100 + P 860 + 1 = 961 rows (a
10 s audio prefix), one engine per model built with max_prefill 1024 (so the unchunked arm is today's path, not the
code under test refusing). Arms: unchunked (prefill_chunk None: one pass) and C in (128, 256, 512), alternated in one
process, --iters repeats after a warm-up round:
  prefill_event_ms   device-event time of engine.prefill (staging, the passes through the layers, heads, first sample)
                     on the engine's stream: median, all repeats, spread = max - min
  passes             calls of _prefill_layers, counted
  ratio_over_unchunked
The transformer pays one weight stream per pass; on the hybrid chunks of up to 256 positions stay on the SSD form of
the Mamba2 scan, where the unchunked 961-position prompt runs the 4-workgroup recurrence.

serve: the C3 share of tools/bench_serve.py (utterances 0 .. 62 of the C3 set on 64 slots, greedy, EOS suppressed,
chunk_frames 16, everything submitted before the first round) and ONE long-prompt request (the 961-row prompt, 64 new
frames) submitted after round 10. Arms, alternated, --serve-iters repeats after a warm-up:
  unchunked   serve(max_prefill 1024): the existing path, the whole prompt as one pass in front of a round
  chunk256    serve(max_prefill 512, prefill_chunk 256): at most one 256-row chunk in front of a round
Per arm: wall_s of the session (first submit to the last chunk, device synchronised after every round), and
largest_gap_ms, the largest time between two consecutive chunks of any ticket that was running when the long request
arrived (host clock after a device synchronise at the end of each round). bit_equal: the C3 tickets' audio is the same
in both arms (their prompts fit one chunk).

Not measured here: kernel times from a profiler; first-audio latency under arrivals on the wall clock; and, with no
checkpoint at hand, the quality of a continuation on real weights (chunked or not).
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
from zonos_vibes_amd.config import zonos_v01_hybrid, zonos_v01_transformer  # noqa: E402
from zonos_vibes_amd.engine import SamplingParams  # noqa: E402
from zonos_vibes_amd.model import Zonos  # noqa: E402

LC, P = 100, 860
S_LEN = LC + P + 1
CHUNKS = (128, 256, 512)
GREEDY = dict(temperature=0.0)
CHUNK_FRAMES = 16


def summary(v: list, nd: int = 3) -> dict:
    return {"median": round(statistics.median(v), nd), "all": [round(x, nd) for x in v],
            "spread": round(max(v) - min(v), nd)}


def long_prompt(d: int, dev):
    prefix = torch.randint(0, 1024, (1, 9, P), generator=torch.Generator().manual_seed(7), dtype=torch.int64)
    return bench.cond_tensor(77, d, dev, LC), prefix.to(dev)


def prefill_times(name: str, cfg, dev, iters: int) -> dict:
    model = Zonos.synthetic(cfg, dev, seed=0, zero_eos=True, max_seqlen=S_LEN + 64 + 9, max_prefill=1024)
    e = model.engine
    cond, prefix = long_prompt(cfg.backbone.d_model, dev)
    sp = SamplingParams(temperature=0.0)
    passes, inner = [0], e._prefill_layers

    def counted(m, max_pos, seqs):
        passes[0] += 1
        return inner(m, max_pos, seqs)
    e._prefill_layers = counted
    arms = (None,) + CHUNKS
    t, n_pass = {a: [] for a in arms}, {}
    for rep in range(iters + 1):  # the first round warms up
        for a in arms:
            passes[0] = 0
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e.stream.synchronize()
            t0.record(e.stream)
            assert e.prefill(0, cond, prefix, 8, sp, prefill_chunk=a) == S_LEN
            t1.record(e.stream)
            t1.synchronize()
            e.check_errors()
            e.release(0)
            n_pass[a] = passes[0]
            if rep:
                t[a].append(t0.elapsed_time(t1))
    out = {"model": name, "s_len": S_LEN, "rows": 2 * S_LEN, "iters": iters}
    base = statistics.median(t[None])
    for a in arms:
        s = summary(t[a])
        out["unchunked" if a is None else f"chunk{a}"] = {"prefill_event_ms": s, "passes": n_pass[a],
                                                          "ratio_over_unchunked": round(s["median"] / base, 4)}
    del model, e
    torch.cuda.empty_cache()
    return out


def serve_share(dev, iters: int, n: int = 63, slots: int = 64, after_round: int = 10) -> dict:
    cfg = zonos_v01_transformer()
    d = cfg.backbone.d_model
    lcs, n_new = (list(v[:n]) for v in bench.c3_job())
    conds = [bench.cond_tensor(1000 + i, d, dev, lc) for i, lc in enumerate(lcs)]
    cond_l, prefix_l = long_prompt(d, dev)
    seqlen = max(max(lcs) + max(n_new) + 9, S_LEN + 64 + 9)
    model = Zonos.synthetic(cfg, dev, seed=0, zero_eos=True, max_slots=slots, max_seqlen=seqlen, max_prefill=1024)
    order = sorted(range(n), key=lambda i: -n_new[i])
    arms = {"unchunked": dict(max_prefill=1024), "chunk256": dict(max_prefill=512, prefill_chunk=256)}

    def session(kw, keep=False):
        stamps, audio = {}, {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with model.serve(slots, max_seqlen=seqlen, chunk_frames=CHUNK_FRAMES, **kw) as s:
            owner = {s.submit(conds[i], max_new_tokens=n_new[i], sampling_params=GREEDY, seed=i): i for i in order}
            long_t, t_long, rounds = None, None, 0
            while not s.idle:
                items = s.run_round()
                torch.cuda.synchronize()
                now = time.perf_counter() - t0
                rounds += 1
                for t, w, _ in items:
                    if w.shape[-1]:
                        stamps.setdefault(t, []).append(now)
                        if keep and t in owner:
                            audio.setdefault(owner[t], []).append(w)
                if rounds == after_round:
                    long_t = s.submit(cond_l, prefix_l, max_new_tokens=64, sampling_params=GREEDY, seed=99)
                    t_long = now
            passes = s.passes_run
        wall = time.perf_counter() - t0
        # tickets that spoke before and after the long request arrived
        gaps = [b - a for t, v in stamps.items() if t != long_t for a, b in zip(v, v[1:]) if b > t_long]
        first_long = stamps[long_t][0] - t_long
        return wall, max(gaps) * 1e3, first_long * 1e3, rounds, passes, \
            {i: torch.cat(w, dim=-1) for i, w in audio.items()} if keep else None

    ref = {a: session(kw, keep=True) for a, kw in arms.items()}  # warm-up of both arms, and the equality
    au, ac = ref["unchunked"][5], ref["chunk256"][5]
    equal = sum(bool(au[i].shape == ac[i].shape and torch.equal(au[i], ac[i])) for i in range(n))
    del ref, au, ac
    res = {a: dict(wall_s=[], largest_gap_ms=[], long_first_audio_ms=[]) for a in arms}
    meta = {}
    for _ in range(iters):
        for a, kw in arms.items():
            wall, gap, first, rounds, passes, _ = session(kw)
            res[a]["wall_s"].append(wall)
            res[a]["largest_gap_ms"].append(gap)
            res[a]["long_first_audio_ms"].append(first)
            meta[a] = dict(rounds=rounds, chunk_passes=passes)
    out = {"workload": f"C3 share: utterances 0..{n - 1} on {slots} slots, greedy, EOS suppressed, chunk_frames "
                       f"{CHUNK_FRAMES}; a {S_LEN}-row prompt (Lc {LC} + P {P}, 64 new frames) submitted after round "
                       f"{after_round}", "iters": iters, "bit_equal_c3_tickets": f"{equal}/{n}"}
    for a in arms:
        out[a] = {k: summary(v, 4 if k == "wall_s" else 2) for k, v in res[a].items()}
        out[a].update(meta[a], serve=arms[a])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--serve-iters", type=int, default=2)
    ap.add_argument("--only", choices=["prefill", "serve"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefill_chunk: needs a GPU (no CPU fall-back: a CPU time says nothing here)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"prompt": f"Lc {LC} + P {P} + 1 = {S_LEN} rows", "kernel_time": "not measured",
           "continuation_quality_on_real_weights": "not measured (no checkpoint)"}
    with torch.inference_mode():
        if args.only in (None, "prefill"):
            res["prefill"] = {}
            for name, cfg in (("transformer", zonos_v01_transformer()), ("hybrid", zonos_v01_hybrid())):
                res["prefill"][name] = prefill_times(name, cfg, dev, args.iters)
                print(name, json.dumps(res["prefill"][name]), flush=True)
        if args.only in (None, "serve"):
            res["serve"] = serve_share(dev, args.serve_iters)
            print("serve", json.dumps(res["serve"]), flush=True)
    doc = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(doc + "\n")
    else:
        print(doc)


if __name__ == "__main__":
    main()
