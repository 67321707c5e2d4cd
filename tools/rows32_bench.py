#!/usr/bin/env python3
"""float64 rows against float32 rows (itd_decompose_f32 / itd_decompose_rows32_f32) on the headline's signal, with bench.py's timing
discipline: device resident, an untimed warm-up by time, W warm-up steps, K back-to-back steps between two synchronisations; the
median and the spread (max - min) of `--runs` such regions.  Every 4th step of a further region carries the engine's own event pairs:
the per-kernel times (level 0, level 1, knot side, sample pass).  --batch B: the same pair for B signals of 2^log2n samples (the
summary is read inside the step, as bench.py does for batches).  --host: tools/host_api_bench.py's host form for both row types.
One JSON line per measurement.

usage: python tools/rows32_bench.py [--log2n 24] [--steps 20] [--warmup 3] [--runs 5] [--batch 0] [--host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import MAX_ITERATION, TIMING_STRIDE, batch_signals_device, sines_noise  # noqa: E402


def region(step, sync, steps):
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    return (time.perf_counter() - t0) / steps * 1e3


def measure(torch, eng, step, args, label, per_kernel):
    from pyitd_amd.engine import TIME_EXTRACT, TIME_EXTRACT_L0, TIME_KF_APPLY, TIME_KF_KNOTS
    sync = torch.cuda.synchronize
    step()
    sync()
    eng.summary(args.batch or 1)
    t_w = time.perf_counter()
    while (time.perf_counter() - t_w) * 1e3 < args.warm_ms:
        for _ in range(8 if not args.batch else 1):
            step()
        sync()
    runs = []
    for _ in range(args.runs):
        for _ in range(args.warmup):
            step()
        runs.append(region(step, sync, args.steps))
    out = {"what": label, "steps": args.steps, "runs_ms": [round(v, 4) for v in runs], "median_ms": round(float(np.median(runs)), 4),
           "spread_ms": round(max(runs) - min(runs), 4), "fuse_level": eng.last_fuse_level, "fuse_repeats": eng.fuse_repeats}
    if per_kernel:
        for _ in range(args.warmup):
            step()
        eng.set_timing(args.steps, stride=TIMING_STRIDE)
        region(step, sync, args.steps)
        k = {}
        for name, t in (("level0_us", TIME_EXTRACT_L0), ("levels_us", TIME_EXTRACT), ("knot_side_us", TIME_KF_KNOTS), ("sample_pass_us", TIME_KF_APPLY)):
            s = eng.kernel_timing_samples(t) * 1e3
            k[name] = round(float(np.median(s)), 2) if len(s) else None
        eng.set_timing(0)
        out["per_kernel_median"] = k
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=150.0)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    import torch
    import pyitd_amd
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    M, n = MAX_ITERATION, 1 << args.log2n
    R = M + 2
    if args.host:
        x = sines_noise(n, seed=0)
        eng = pyitd_amd.Engine(n, 1, 0)
        for dt in (np.float64, np.float32):
            out = np.empty((R, n), dt)
            eng.decompose_host(x, M, want_baselines=False, out=out, rows_dtype=dt)
            ts = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                eng.decompose_host(x, M, want_baselines=False, out=out, rows_dtype=dt)
                ts.append((time.perf_counter() - t0) * 1e3)
            print(json.dumps({"what": "host form, %s rows" % np.dtype(dt).name, "n": n, "runs_ms": [round(v, 3) for v in ts],
                              "median_ms": round(float(np.median(ts)), 3), "spread_ms": round(max(ts) - min(ts), 3)}), flush=True)
        return
    B = args.batch or 1
    if args.batch:
        x = batch_signals_device(torch, dev, 0, B, n)
    else:
        x = torch.from_numpy(sines_noise(n, seed=0)).to(dev)[None]
    stream = torch.cuda.Stream(device=dev)
    res = {}
    for dt, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        rows = torch.empty((B, R, n), dtype=tdt, device=dev)
        eng = pyitd_amd.Engine(n, B, 0)
        torch.cuda.synchronize()

        def step():
            eng.decompose_dev(x.data_ptr(), np.float32, n, B, x.stride(0), M, rows.data_ptr(), None, stream.cuda_stream, rows_dtype=dt)
            if args.batch:
                eng.summary(B)
        res[dt] = measure(torch, eng, step, args, "%s rows, %s" % (np.dtype(dt).name, ("batch %d x 2^%d" % (B, args.log2n)) if args.batch else "2^%d" % args.log2n),
                          per_kernel=not args.batch)
        eng.close()
        del rows
        torch.cuda.empty_cache()
    print(json.dumps({"what": "float32 rows / float64 rows", "ratio": round(res[np.float32]["median_ms"] / res[np.float64]["median_ms"], 4)}), flush=True)


if __name__ == "__main__":
    main()
