"""Guidance-free generation (cfg_scale = 1, one row per utterance) against guided generation (cfg_scale = 2, two rows),
in one process, one JSON line.

    python tools/bench_cfg1.py [--iters 5] [--warmup 1] [--slots 64] [--out profiles/cfg1_bench.json]
    python tools/bench_cfg1.py --guided-unchanged PARENT_DIR [--out profiles/cfg1_bench.json]
        (PARENT_DIR: a built checkout of the parent commit; merges its result into --out if the file exists)

ONE Zonos.synthetic(zonos_v01_transformer()) model runs both arms (the layout is chosen per call), bench.py's
conditioning, greedy, EOS suppressed. After the warm-up the arms are ALTERNATED within every repeat (arms must share
their thermal and clock state). The guidance-free arm gets row 0 of the guided arm's conditioning. Fields:

  c2.<arm>.step_us        decode step of a live utterance at position 591 (64 hipGraph replays between device events),
                          median of --iters; step_us_all the repeats, step_spread_us max - min
  c2.<arm>.utterance_ms   generate() + decode() of the C2 utterance (Lc 160, 861 frames), call to device idle
  c2.step_ratio / utterance_ratio      guidance-free / guided
  c3.<arm>.batch_s        the C3 share (bench.py's: the first --slots utterances of the 512-utterance set, 2-30 s,
                          through --slots slots): generate_batch() + decode() of every utterance, wall seconds, median; its two
                          parts generate_s / dac_s (medians of their own), batch_rtf = audio s / batch_s
  c3.<arm>.stream_s       the same job through stream_batch(decoder="carry"), every chunk consumed
  c3.batch_ratio / generate_ratio / stream_ratio   guidance-free / guided; rows_ratio 0.5 is what the row counts alone
                          would give (the DAC decode and the per-launch floor are the same in both arms)
  c3.step_us_by_busy_slots / step_ratio_by_busy_slots / admission_ms   where a many-slot job's time goes: the decode
                          step with 1 .. --slots busy slots in either layout, and prefill_many of --slots utterances

--guided-unchanged: `python bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR` as child processes, in PARENT_DIR
and in this tree alternately, three times each: codes.npy and wav.npy compared byte for byte, ms_per_step of every run,
and whether this tree's median lies inside the parent's own repeat spread.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ARMS = ("guided", "free")
CFG = {"guided": 2.0, "free": 1}


def guided_unchanged(parent: str, rounds: int = 3) -> dict:
    """bench.py in the parent's tree and in this one, alternated; no GPU work in this process."""
    import numpy as np
    trees = {"parent": os.path.abspath(parent), "this": REPO}
    ms = {k: [] for k in trees}
    shas = {k: [] for k in trees}
    same = True
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(rounds):
            for name, tree in trees.items():
                out = os.path.join(tmp, f"{name}{r}")
                p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                                    "--dump-outputs", out], cwd=tree, capture_output=True, text=True, timeout=900)
                if p.returncode != 0:
                    raise SystemExit(f"bench.py failed in {tree}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
                line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
                ms[name].append(line["ms_per_step"])
                shas[name].append(line["codes_sha256_16"])
            for f in ("codes.npy", "wav.npy"):
                a, b = (np.load(os.path.join(tmp, f"{n}{r}", f)) for n in trees)
                same = same and a.shape == b.shape and a.tobytes() == b.tobytes()
    lo, hi = min(ms["parent"]), max(ms["parent"])
    med = statistics.median(ms["this"])
    return dict(rounds=rounds, outputs_identical=bool(same), codes_sha256_16=sorted(set(shas["parent"] + shas["this"])),
                ms_per_step_parent=ms["parent"], ms_per_step_this=ms["this"], parent_spread=[lo, hi],
                this_median=med, this_median_inside_parent_spread=bool(lo <= med <= hi),
                this_median_over_parent_median=round(med / statistics.median(ms["parent"]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--skip-c3", action="store_true")
    ap.add_argument("--guided-unchanged", metavar="PARENT_DIR", default=None)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    def emit(res):
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")

    if args.guided_unchanged:
        res = {}
        if args.out and os.path.exists(args.out):
            res = json.loads(open(args.out).read())
        res["guided_unchanged"] = guided_unchanged(args.guided_unchanged)
        return emit(res)

    import torch

    from bench import DAC_HOP, DAC_SAMPLE_RATE, LC, N_NEW, c3_job, cond_tensor
    from zonos_vibes_amd.config import zonos_v01_transformer
    from zonos_vibes_amd.engine import SamplingParams
    from zonos_vibes_amd.model import Zonos

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = zonos_v01_transformer()
    d = cfg.backbone.d_model
    model = Zonos.synthetic(cfg, dev, seed=0, zero_eos=True, max_seqlen=LC + N_NEW + 9, max_prefill=LC + 1)
    cond2 = cond_tensor(1, d, dev)
    sp = dict(temperature=0.0)

    def cond_of(arm, c):
        return c if arm == "guided" else c[:1].contiguous()

    def step_us(arm, steps=64):
        """bench.py's time_decode_step in the arm's layout: (us per step, mean position)."""
        model._select_layout(CFG[arm])
        e = model.engine
        s_len = e.prefill(0, cond_of(arm, cond2), None, N_NEW, SamplingParams(temperature=0.0, cfg_scale=CFG[arm]))
        lead = N_NEW // 2 - steps // 2
        e.step(lead, slots=1)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(e.stream):
            start.record(e.stream)
            e.step(steps, slots=1)
            end.record(e.stream)
        end.synchronize()
        assert e.slot_state(0)["active"]
        e.release(0)
        return start.elapsed_time(end) * 1000.0 / steps, s_len + lead + steps // 2

    def utterance(arm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codes = model.generate(cond_of(arm, cond2), max_new_tokens=N_NEW, cfg_scale=CFG[arm], sampling_params=sp,
                               progress_bar=False, chunk=128)
        model.autoencoder.decode(codes)
        torch.cuda.synchronize()
        assert codes.shape[-1] == N_NEW
        return (time.perf_counter() - t0) * 1e3

    def stats(vals, nd):
        return dict(median=round(statistics.median(vals), nd), all=[round(v, nd) for v in vals],
                    spread=round(max(vals) - min(vals), nd))

    for _ in range(max(args.warmup, 1)):
        for arm in ARMS:
            utterance(arm)
            step_us(arm)
    step = {a: [] for a in ARMS}
    utt = {a: [] for a in ARMS}
    pos = None
    for _ in range(args.iters):
        for arm in ARMS:
            us, pos = step_us(arm)
            step[arm].append(us)
        for arm in ARMS:
            utt[arm].append(utterance(arm))
    c2 = dict(workload=f"C2: zonos-v0.1-transformer synthetic, Lc {LC}, {N_NEW} new frames, greedy, batch 1",
              decode_step_pos=pos)
    for arm in ARMS:
        s, u = stats(step[arm], 1), stats(utt[arm], 2)
        c2[arm] = dict(rows_per_step=2 if arm == "guided" else 1, step_us=s["median"], step_us_all=s["all"],
                       step_spread_us=s["spread"], utterance_ms=u["median"], utterance_ms_all=u["all"],
                       utterance_spread_ms=u["spread"])
    c2["step_ratio"] = round(c2["free"]["step_us"] / c2["guided"]["step_us"], 4)
    c2["utterance_ratio"] = round(c2["free"]["utterance_ms"] / c2["guided"]["utterance_ms"], 4)
    res = dict(iters=args.iters, arms="guided: cfg_scale 2.0, rows 2s / 2s + 1; free: cfg_scale 1, row s", c2=c2)

    if not args.skip_c3:
        S = args.slots
        lcs, n_all = c3_job()
        lcs, n_new = lcs[:S], n_all[:S]
        conds2 = [cond_tensor(1000 + i, d, dev, lc) for i, lc in enumerate(lcs)]
        conds = {arm: [cond_of(arm, c) for c in conds2] for arm in ARMS}
        model._ensure_capacity(S, max(lcs) + max(n_new) + 9, max(lcs) + 1)
        seeds = list(range(S))
        audio = sum(n_new) * DAC_HOP / DAC_SAMPLE_RATE

        def batch(arm, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate_batch(conds[arm], max_new_tokens=n, cfg_scale=CFG[arm], sampling_params=sp,
                                       seeds=seeds, max_slots=S)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for c in out:
                model.autoencoder.decode(c)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert sum(int(c.shape[-1]) for c in out) == sum(n)
            return t2 - t0, t1 - t0, t2 - t1

        def stream(arm, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            samples = 0
            for _, w, _ in model.stream_batch(conds[arm], max_new_tokens=n, cfg_scale=CFG[arm], sampling_params=sp,
                                              seeds=seeds, max_slots=S, decoder="carry"):
                samples += w.shape[-1]
            torch.cuda.synchronize()
            assert samples == sum(n) * DAC_HOP
            return time.perf_counter() - t0

        for arm in ARMS:  # graphs of every busy-slot bucket, the DAC graphs and the carried decoder, outside the timing
            batch(arm, [4] * S)
            stream(arm, [20] * S)
            for _ in range(args.warmup):
                batch(arm, n_new)
                stream(arm, n_new)
        bt = {a: [] for a in ARMS}
        stt = {a: [] for a in ARMS}
        for _ in range(args.iters):
            for arm in ARMS:
                bt[arm].append(batch(arm, n_new))
            for arm in ARMS:
                stt[arm].append(stream(arm, n_new))
        c3 = dict(workload=f"C3 share: utterances 0..{S - 1} of the 512-utterance C3 set (2-30 s, Lc 8 + 15 s), {S} "
                           f"slots, greedy, EOS suppressed", audio_s=round(audio, 1), rows_ratio=0.5)
        for arm in ARMS:
            w, g, dc = (stats([t[i] for t in bt[arm]], 3) for i in range(3))  # whole, generate_batch, decode
            st_ = stats(stt[arm], 3)
            c3[arm] = dict(rows_at_full_load=(2 if arm == "guided" else 1) * S, batch_s=w["median"], batch_s_all=w["all"],
                           batch_spread_s=w["spread"], generate_s=g["median"], generate_spread_s=g["spread"],
                           dac_s=dc["median"], batch_rtf=round(audio / w["median"], 1), stream_s=st_["median"],
                           stream_s_all=st_["all"], stream_spread_s=st_["spread"],
                           stream_rtf=round(audio / st_["median"], 1))
        for k in ("batch_s", "generate_s", "stream_s"):
            c3[k.replace("_s", "_ratio")] = round(c3["free"][k] / c3["guided"][k], 4)

        # where a many-slot job's time goes: the step at each busy-slot count (the job's tail runs few slots, where a
        # step is the weight stream in either layout) and the admission (prefill_many of all the slots)
        def many_slot_step(arm, k, steps=32, lead=64):
            model._select_layout(CFG[arm])
            e = model.engine
            prm = SamplingParams(temperature=0.0, cfg_scale=CFG[arm])
            items = [(s_, conds[arm][s_], None, 400, prm) for s_ in range(k)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.prefill_many(items)
            torch.cuda.synchronize()
            pre_ms = (time.perf_counter() - t0) * 1e3
            e.step(lead, slots=k)
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(e.stream):
                start.record(e.stream)
                e.step(steps, slots=k)
                end.record(e.stream)
            end.synchronize()
            e.check_errors()
            for s_ in range(k):
                e.release(s_)
            return start.elapsed_time(end) * 1000.0 / steps, pre_ms

        buckets = [k for k in (1, 4, 8, 16, 32, 64) if k <= S]
        for arm in ARMS:
            for k in buckets:
                many_slot_step(arm, k)
        ms_ = {a: {k: [] for k in buckets} for a in ARMS}
        pm_ = {a: [] for a in ARMS}
        for _ in range(args.iters):
            for k in buckets:
                for arm in ARMS:
                    us, pre_ms = many_slot_step(arm, k)
                    ms_[arm][k].append(us)
                    if k == buckets[-1]:
                        pm_[arm].append(pre_ms)
        c3["step_us_by_busy_slots"] = {
            arm: {str(k): dict(zip(("median", "spread"), (stats(ms_[arm][k], 1)[f] for f in ("median", "spread"))))
                  for k in buckets} for arm in ARMS}
        c3["step_ratio_by_busy_slots"] = {str(k): round(statistics.median(ms_["free"][k]) /
                                                        statistics.median(ms_["guided"][k]), 4) for k in buckets}
        c3["admission_ms"] = {arm: dict(zip(("median", "spread"), (stats(pm_[arm], 2)[f] for f in ("median", "spread"))))
                              for arm in ARMS}
        c3["admission_note"] = (f"prefill_many of {buckets[-1]} utterances (the C3 share's conditioning), host clock "
                                "around a device synchronise; step: 32 graph replays between device events, positions "
                                "Lc + 64 .. Lc + 96")
        res["c3"] = c3
    emit(res)


if __name__ == "__main__":
    main()
