"""mixer_weights="fp8" against bf16 at the C4 configuration (Zonos-v0.1-hybrid dims), in one process, one JSON line.

    python tools/bench_fp8_hybrid.py [--iters 5] [--warmup 1] [--agree-frames 200] [--out profiles/fp8_hybrid_bench.json]

Two Zonos.synthetic(zonos_v01_hybrid()) models with the same seed, bf16 and fp8 Mamba2 projections, bench.py's
conditioning (Lc 160, 861 new frames, greedy, EOS suppressed). The method is tools/bench_fp8.py's: after the warm-up the
two arms are ALTERNATED (arms closer than about 1 % must share their thermal and clock state), 5 repeats,
medians with every repeat and the spread (max - min) next to them. Fields, per arm:

  step_us            decode step of a live utterance at its mean position (bench.py's time_decode_step: 64 hipGraph
                     replays between device events)
  step_bytes         algorithmic HBM bytes of that step (bench.py's hybrid_step_bytes) with the Mamba2 projections at
                     their stored width (fp8: one byte per weight + one exponent per column)
  step_hbm_frac      step_bytes / step time / 8 TB/s: a whole-step rate over the peak
  utterance_ms       generate() + decode(), call to device idle
  prefill_ms         the 161-position (322-row) prefill, call to device idle. The fp8 arm expands every Mamba2 layer's
                     two projections into bf16 scratch in front of its GEMMs: expand_ms is those 82 launches alone
                     (device events), the cost of the expansion inside prefill_ms
  mamba_block_us     one zmi_mamba_block launch (in_proj + Mamba2 step): the 41 layers' launches back to back, granules
                     zeroed before each run so every launch waits for its own in_proj (bench.py's _time_fused)
  out_proj_us        one GRMS_G out_proj launch: the 41 layers' launches back to back
  weight_bytes       device memory of the engine's weights; scratch_bytes: the prefill's expansion scratch
and: step_ratio / utterance_ratio / prefill_ratio / bytes_ratio / mamba_block_ratio / out_proj_ratio (fp8 / bf16),
faster_than_spread (bf16 - fp8 step time exceeds both arms' spread), greedy_agreement (tools/bench_fp8.py: the fp8 model
teacher-forced on the bf16 model's frames; reported, not asserted; synthetic weights only).
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
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench import HBM_PEAK_GBS, LC, N_NEW, _time_fused, cond_tensor, hybrid_step_bytes, time_decode_step  # noqa: E402
from bench_fp8 import greedy_agreement  # noqa: E402
from zonos_vibes_amd import _lib  # noqa: E402
from zonos_vibes_amd.config import zonos_v01_hybrid  # noqa: E402
from zonos_vibes_amd.engine import SamplingParams  # noqa: E402
from zonos_vibes_amd.model import Zonos  # noqa: E402

ARMS = ("bf16", "fp8")


def mamba_layers(e):
    return [lw for lw in e.w["layers"] if lw["kind"] == "mamba"]


def stored_step_bytes(e, pos: int) -> int:
    """bench.py's hybrid_step_bytes with the Mamba2 projections at their stored width."""
    b = hybrid_step_bytes(e, pos)
    if e.mixer_weights == "fp8":
        md = e.md
        proj = len(mamba_layers(e)) * (md["d_in_proj"] * e.d + e.d * md["d_ssm"])
        b += -2 * proj + sum(lw[k].numel() for lw in mamba_layers(e) for k in ("in_proj", "out"))
    return b


def weight_bytes(e) -> int:
    def walk(v):
        if isinstance(v, torch.Tensor):
            return v.numel() * v.element_size()
        if isinstance(v, dict):
            return sum(walk(x) for x in v.values())
        if isinstance(v, (list, tuple)):
            return sum(walk(x) for x in v)
        return 0
    return walk(e.w)


def time_prefill(e, cond) -> float:
    params = SamplingParams(temperature=0.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e.prefill(0, cond, None, N_NEW, params)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    e.release(0)
    return ms


def time_expand(e, reps: int = 5) -> float:
    """ms of the expansion launches of one prefill pass (every Mamba2 layer's in_proj and out_proj), device events."""
    if e.mixer_weights != "fp8":
        return 0.0
    md = e.md
    runs = [r for lw in mamba_layers(e) for r in (e._expand_mixer(lw["in_proj"], md["d_in_proj"], e.d, e.mix_scratch[0]),
                                                  e._expand_mixer(lw["out"], e.d, md["d_ssm"], e.mix_scratch[1]))]
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    with torch.cuda.stream(e.stream):
        for _ in range(reps + 1):
            st.record(e.stream)
            for r in runs:
                r()
            en.record(e.stream)
            en.synchronize()
            ms.append(st.elapsed_time(en))
    return statistics.median(ms[1:])


def time_launches(e, cond, reps: int = 20) -> tuple[float, float]:
    """(us per zmi_mamba_block launch, us per GRMS_G out_proj launch) of a live utterance's 2-row decode plan."""
    e.prefill(0, cond, None, N_NEW, SamplingParams(temperature=0.0))
    e.step(8, slots=1)
    e.stream.synchronize()
    plan = e._plan(e.rps, e._segments(1, 1)[0][1])
    blocks = [it for kind, it in plan if kind == "call" and hasattr(it, "args")]
    outs = [it for kind, it in plan if kind == "gemv" and it[0].pro == _lib.PRO_GRMS_G]
    n = len(mamba_layers(e))
    assert len(blocks) == n and len(outs) == n, (len(blocks), len(outs), n)
    blk = _time_fused(e, blocks, e.mgran, lambda it: it(), reps)
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tot = 0.0
    for r in range(reps + 1):  # (no hand-off: the launches read the step's g rows as they stand)
        st.record(e.stream)
        for it in outs:
            e._run_gemv(it)
        en.record(e.stream)
        en.synchronize()
        tot += st.elapsed_time(en) * 1000.0 if r else 0.0
    out = tot / (reps * n)
    e.check_errors()
    e.release(0)
    return blk, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--agree-frames", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = zonos_v01_hybrid()
    models = {a: Zonos.synthetic(cfg, dev, seed=0, zero_eos=True, max_seqlen=LC + N_NEW + 9, max_prefill=LC + 1,
                                 mixer_weights=a) for a in ARMS}
    cond = cond_tensor(1, cfg.backbone.d_model, dev)
    params = dict(temperature=0.0)

    def utterance(m):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codes = m.generate(cond, max_new_tokens=N_NEW, sampling_params=params, progress_bar=False, chunk=128)
        m.autoencoder.decode(codes)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(max(args.warmup, 1)):
        for a in ARMS:
            utterance(models[a])
            time_decode_step(models[a], cond)
            time_prefill(models[a].engine, cond)
            time_launches(models[a].engine, cond, 2)
    keys = ("step", "utt", "pre", "blk", "out", "exp")
    t = {a: {k: [] for k in keys} for a in ARMS}
    pos = None
    for _ in range(args.iters):
        for a in ARMS:
            us, pos = time_decode_step(models[a], cond)
            t[a]["step"].append(us)
        for a in ARMS:
            t[a]["utt"].append(utterance(models[a]))
        for a in ARMS:
            t[a]["pre"].append(time_prefill(models[a].engine, cond))
        for a in ARMS:
            blk, out = time_launches(models[a].engine, cond)
            t[a]["blk"].append(blk)
            t[a]["out"].append(out)
        for a in ARMS:
            t[a]["exp"].append(time_expand(models[a].engine))
    md = models["bf16"].engine.md
    res = dict(workload=f"C4: zonos-v0.1-hybrid dims synthetic (41 Mamba2 + 5 MHA layers), Lc {LC}, {N_NEW} new frames, "
                        "greedy, batch 1", iters=args.iters, decode_step_pos=pos, hbm_peak_gbs=HBM_PEAK_GBS,
               prefill_rows=2 * (LC + 1), d_in_proj=md["d_in_proj"], d_ssm=md["d_ssm"])

    # (samples, field, spread field, ratio field, digits)
    fields = (("step", "step_us", "step_spread_us", "step_ratio", 1),
              ("utt", "utterance_ms", "utterance_spread_ms", "utterance_ratio", 2),
              ("pre", "prefill_ms", "prefill_spread_ms", "prefill_ratio", 2),
              ("blk", "mamba_block_us", "mamba_block_spread_us", "mamba_block_ratio", 2),
              ("out", "out_proj_us", "out_proj_spread_us", "out_proj_ratio", 2),
              ("exp", "expand_ms", "expand_spread_ms", None, 3))
    for a in ARMS:
        e = models[a].engine
        ent = {}
        for key, name, spread, _, nd in fields:
            v = t[a][key]
            ent[name], ent[name + "_all"], ent[spread] = (round(statistics.median(v), nd), [round(x, nd) for x in v],
                                                          round(max(v) - min(v), nd))
        b = stored_step_bytes(e, pos)
        ent.update(step_bytes=b, step_hbm_frac=round(b / (ent["step_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 3),
                   weight_bytes=weight_bytes(e),
                   scratch_bytes=sum(s.numel() * s.element_size() for s in (e.mix_scratch or ())))
        res[a] = ent
    for _, name, _, ratio, _ in fields:
        if ratio:
            res[ratio] = round(res["fp8"][name] / res["bf16"][name], 4)
    res["bytes_ratio"] = round(res["fp8"]["step_bytes"] / res["bf16"]["step_bytes"], 4)
    res["weight_bytes_ratio"] = round(res["fp8"]["weight_bytes"] / res["bf16"]["weight_bytes"], 4)
    res["faster_than_spread"] = bool(res["bf16"]["step_us"] - res["fp8"]["step_us"] >
                                     max(res["bf16"]["step_spread_us"], res["fp8"]["step_spread_us"]))
    if args.agree_frames > 0:
        res["greedy_agreement"] = greedy_agreement(models["bf16"], models["fp8"], cond, args.agree_frames)
    res["unmeasured"] = ("speech quality on real weights (no checkpoint here): in particular the dt rows of in_proj are "
                         "quantised like the rest and feed softplus and exp(dt A)")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
