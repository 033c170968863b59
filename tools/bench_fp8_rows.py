"""fp8 MLP weights in the many-row GEMM forms against the fp8 tile loop and the bf16 forms, in one process.

    python tools/bench_fp8_rows.py [--iters 5] [--rows 24,32,48,64,128,322] [--slots 64] [--skip-e2e] [--skip-launch]
                                   [--out profiles/fp8_rows_bench.json]

per_launch: fc1 (N 16384, K 2048, SWIGLU) and fc2 (N 2048, K 8192, RESIDUAL, then the next LayerNorm) at M rows, three
arms, ALTERNATED inside every repeat (arms this close must share their thermal and clock state):
  loop   the fp8 tile loop: ZMI_OPT_FP8_ROWS 0 and zmi_gemv_launch (fc2: + zmi_layernorm_rows): what an fp8 engine ran
         before the many-row forms read fp8, the baseline
  rows   the fp8 many-row form (fc1: gemm_rows_kernel_f8; fc2: zmi_gemv_splitk_f8_ln)
  bf16   the bf16 many-row form (fc1: gemm_rows_kernel; fc2: zmi_gemv_splitk_ln)
A sample is a hipGraph of launches over --copies copies of the weight in turn (together larger than the Infinity Cache,
so every launch streams its weights from HBM as a layer of the model does), between device events; us per launch,
median of --iters, spread = max - min. faster_than_spread: loop - rows exceeds both arms' spread.

e2e: the C3 share (bench.py's: the first --slots utterances of the 512-utterance set on --slots slots, greedy, EOS
suppressed), generate_batch() + decode(), and one admission (prefill_many of all the slots), three arms: the fp8 engine
with fp8_rows False, a second fp8 engine on the same weight tensors with fp8_rows True, the bf16 engine.
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bench import DAC_HOP, DAC_SAMPLE_RATE, c3_job, cond_tensor  # noqa: E402
from zonos_vibes_amd import _lib, quant  # noqa: E402

ROWS = (24, 32, 48, 64, 128, 322)
ARMS = ("loop", "rows", "bf16")
EPS = 1e-5


def stats(v, nd):
    return dict(median=round(statistics.median(v), nd), all=[round(x, nd) for x in v], spread=round(max(v) - min(v), nd))


@contextlib.contextmanager
def option(which, value):
    lib = _lib.lib()
    old = lib.zmi_get_option(which)
    _lib.check(lib.zmi_set_option(which, value), "set_option")
    try:
        yield
    finally:
        _lib.check(lib.zmi_set_option(which, old), "set_option")


def rnd(*shape, scale=1.0, seed=0, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1).mul(scale).to(torch.bfloat16).to(dev)


def make_weights(n, k, mode, copies, dev):
    """`copies` x (fp8 bytes + exponents, the bf16 twin in layout M8) of random [n][k] weights."""
    lib, out = _lib.lib(), []
    s = torch.cuda.current_stream().cuda_stream
    for c in range(copies):
        q, e = quant.quantize_fp8(rnd(n, k, scale=0.05, seed=100 + c, dev=dev))
        packed, ep = quant.pack_m8f8(q, e, n, mode)
        deq = quant.dequantize_fp8(q, e).contiguous()
        twin = torch.empty(n * k, dtype=torch.bfloat16, device=dev)
        _lib.check(lib.zmi_pack_weight(deq.data_ptr(), twin.data_ptr(), n, k, n, mode, s), "pack")
        out.append((packed, ep, twin))
    torch.cuda.synchronize()
    return out


def per_launch(dev, iters, copies, reps, rows=ROWS):
    lib = _lib.lib()
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream
    d, F = 2048, 8192
    w1 = make_weights(2 * F, d, _lib.PACK_SWIGLU, copies, dev)
    w2 = make_weights(d, F, _lib.PACK_IDENTITY, copies, dev)
    lw, lb = (rnd(d, scale=0.1, seed=10) + 1).contiguous(), rnd(d, scale=0.02, seed=11)
    res = {"fc1": {}, "fc2": {}}
    for M in rows:
        x1, h1 = rnd(M, d, seed=1), torch.zeros(M, F, dtype=torch.bfloat16, device=dev)
        x2, o2 = rnd(M, F, scale=0.05, seed=2), torch.zeros(M, d, dtype=torch.bfloat16, device=dev)
        xn = torch.zeros(M, d, dtype=torch.bfloat16, device=dev)
        part = torch.zeros(lib.zmi_gemv_splitk_floats(M, d), dtype=torch.float32, device=dev)

        def args(w, f8, X, N, K, out, ldo):
            a = _lib.GemvArgs()
            a.W, a.X, a.M, a.N, a.K, a.ldx = (w[0] if f8 else w[2]).data_ptr(), X.data_ptr(), M, N, K, K
            a.out, a.ldo, a.n_valid, a.eps = out.data_ptr(), ldo, N, EPS
            if f8:
                a.w_fmt, a.w_exp = _lib.WFMT_FP8, w[1].data_ptr()
            return a

        def fc1(arm, w):
            a = args(w, arm != "bf16", x1, 2 * F, d, h1, F)
            with option(_lib.OPT_FP8_ROWS, 0 if arm == "loop" else 1):
                _lib.check(lib.zmi_gemv_launch(ctypes.byref(a), _lib.EPI_SWIGLU, sp), "fc1")

        def fc2(arm, w):
            a = args(w, arm != "bf16", x2, d, F, o2, d)
            pa = (part.data_ptr(), part.numel(), lw.data_ptr(), lb.data_ptr(), EPS, xn.data_ptr(), d, sp)
            if arm == "loop":
                _lib.check(lib.zmi_gemv_launch(ctypes.byref(a), _lib.EPI_RESIDUAL, sp), "fc2")
                _lib.check(lib.zmi_layernorm_rows(o2.data_ptr(), d, M, d, lw.data_ptr(), lb.data_ptr(), EPS, xn.data_ptr(),
                                                  d, sp), "ln")
            elif arm == "rows":
                _lib.check(lib.zmi_gemv_splitk_f8_ln(ctypes.byref(a), _lib.EPI_RESIDUAL, *pa), "fc2 splitk8")
            else:
                _lib.check(lib.zmi_gemv_splitk_ln(ctypes.byref(a), _lib.EPI_RESIDUAL, *pa), "fc2 splitk")

        for name, fn, ws in (("fc1", fc1, w1), ("fc2", fc2, w2)):
            graphs = {arm: _lib.capture(sp, lambda arm=arm: [fn(arm, w) for w in ws]) for arm in ARMS}
            us = {arm: [] for arm in ARMS}
            for it in range(iters + 1):  # the first round warms up
                for arm in ARMS:
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    _lib.check(lib.zmi_graph_launch(graphs[arm], 1, sp), "graph")
                    t0.record(stream)
                    _lib.check(lib.zmi_graph_launch(graphs[arm], reps, sp), "graph")
                    t1.record(stream)
                    t1.synchronize()
                    if it:
                        us[arm].append(t0.elapsed_time(t1) * 1000.0 / (reps * len(ws)))
            for g in graphs.values():
                _lib.check(lib.zmi_graph_destroy(g))
            r = {arm: stats(us[arm], 2) for arm in ARMS}
            r["rows_over_loop"] = round(r["rows"]["median"] / r["loop"]["median"], 4)
            r["rows_over_bf16"] = round(r["rows"]["median"] / r["bf16"]["median"], 4)
            r["faster_than_spread"] = bool(r["loop"]["median"] - r["rows"]["median"] >
                                           max(r["loop"]["spread"], r["rows"]["spread"]))
            res[name][str(M)] = r
    return res


def e2e(dev, iters, S):
    from zonos_vibes_amd.config import zonos_v01_transformer
    from zonos_vibes_amd.engine import SamplingParams
    from zonos_vibes_amd.model import Zonos
    cfg = zonos_v01_transformer()
    d = cfg.backbone.d_model
    lcs, n_all = c3_job()
    lcs, n_new = lcs[:S], n_all[:S]
    conds = [cond_tensor(1000 + i, d, dev, lc) for i, lc in enumerate(lcs)]
    cap = dict(max_slots=S, max_seqlen=max(lcs) + max(n_new) + 9, max_prefill=max(lcs) + 1)
    m_off = Zonos.synthetic(cfg, dev, seed=0, zero_eos=True, weights="fp8", **cap)
    m_on = Zonos(cfg, dev, autoencoder=m_off.autoencoder, weights="fp8", **cap)
    m_on.engine.w = m_off.engine.w  # the same weight tensors: the arms differ in the launch forms alone
    m_on.engine._build_plan()
    m_off.engine.fp8_rows = False
    m_off.engine._build_plan()
    models = {"fp8_loop": m_off, "fp8_rows": m_on,
              "bf16": Zonos.synthetic(cfg, dev, seed=0, zero_eos=True, **cap)}
    arms = tuple(models)
    seeds = list(range(S))
    audio = sum(n_new) * DAC_HOP / DAC_SAMPLE_RATE
    sp = dict(temperature=0.0)

    def batch(arm, n):
        m = models[arm]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.generate_batch(conds, max_new_tokens=n, sampling_params=sp, seeds=seeds, max_slots=S)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for c in out:
            m.autoencoder.decode(c)
        torch.cuda.synchronize()
        assert m.engine.S == S and sum(int(c.shape[-1]) for c in out) == sum(n)
        return time.perf_counter() - t0, t1 - t0, out

    def admission(arm):
        e = models[arm].engine
        prm = SamplingParams(temperature=0.0, cfg_scale=2.0)
        items = [(s, conds[s], None, 400, prm) for s in range(S)]
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(e.stream):
            t0.record(e.stream)
            e.prefill_many(items)
            t1.record(e.stream)
        t1.synchronize()
        e.check_errors()
        for s in range(S):
            e.release(s)
        return t0.elapsed_time(t1)

    codes = {}
    for arm in arms:  # the graphs of every busy-slot bucket and the DAC graphs, outside the timing
        batch(arm, [4] * S)
        codes[arm] = batch(arm, n_new)[2]
        admission(arm)
    same = {arm: all(torch.equal(a, b) for a, b in zip(codes[arm], codes["fp8_loop"])) for arm in ("fp8_rows",)}
    bt, gt, ad = ({a: [] for a in arms} for _ in range(3))
    for _ in range(iters):
        for arm in arms:
            w, g, _ = batch(arm, n_new)
            bt[arm].append(w)
            gt[arm].append(g)
        for arm in arms:
            ad[arm].append(admission(arm))
    res = dict(workload=f"C3 share: utterances 0..{S - 1} of the 512-utterance C3 set (2-30 s, Lc 8 + 15 s), {S} slots, "
                        "greedy, EOS suppressed, generate_batch() + decode() per utterance", audio_s=round(audio, 1),
               fp8_rows_codes_equal_fp8_loop=same["fp8_rows"])
    for arm in arms:
        w, g, a = stats(bt[arm], 3), stats(gt[arm], 3), stats(ad[arm], 2)
        res[arm] = dict(batch_s=w["median"], batch_s_all=w["all"], batch_spread_s=w["spread"], generate_s=g["median"],
                        generate_spread_s=g["spread"], rtf=round(audio / w["median"], 1), admission_ms=a["median"],
                        admission_ms_all=a["all"], admission_spread_ms=a["spread"])
    for k in ("batch_s", "generate_s", "admission_ms"):
        res[k.rsplit("_", 1)[0] + "_ratio_rows_over_loop"] = round(res["fp8_rows"][k] / res["fp8_loop"][k], 4)
        res[k.rsplit("_", 1)[0] + "_ratio_rows_over_bf16"] = round(res["fp8_rows"][k] / res["bf16"][k], 4)
    res["faster_than_spread"] = bool(res["fp8_loop"]["batch_s"] - res["fp8_rows"]["batch_s"] >
                                     max(res["fp8_loop"]["batch_spread_s"], res["fp8_rows"]["batch_spread_s"]))
    res["admission_faster_than_spread"] = bool(
        res["fp8_loop"]["admission_ms"] - res["fp8_rows"]["admission_ms"] >
        max(res["fp8_loop"]["admission_spread_ms"], res["fp8_rows"]["admission_spread_ms"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--copies", type=int, default=8, help="weight copies a sample cycles through")
    ap.add_argument("--reps", type=int, default=8, help="graph replays per sample")
    ap.add_argument("--rows", default=",".join(map(str, ROWS)), help="row counts of the per-launch samples")
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-launch", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = dict(iters=args.iters)
    if not args.skip_launch:
        res["per_launch_note"] = (f"us per launch over {args.copies} weight copies in turn, {args.reps} graph replays per "
                                  "sample; fc2 includes the next LayerNorm (loop: a zmi_layernorm_rows launch)")
        res["per_launch"] = per_launch(dev, args.iters, args.copies, args.reps,
                                       tuple(int(m) for m in args.rows.split(",")))
    if not args.skip_e2e:
        res["e2e"] = e2e(dev, args.iters, args.slots)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
