#!/usr/bin/env python3
"""Selected rows against all rows (itd_decompose_select_f32 / itd_decompose_f32) on the headline's signal, with bench.py's timing
discipline: device resident, an untimed warm-up by time, W warm-up steps, K back-to-back steps between two synchronisations.  The
variants ALTERNATE within one process — `--runs` rounds, every round one region of each variant — and the median and the spread
(max - min) of each variant's regions are reported:

  parent full      the parent commit's itd_decompose_f32, from --parent-lib (a libpyitd_hip.so built from the parent commit in a
                   scratch copy of the tree; loaded beside this tree's library, an engine of its own); left out without the option
  full             this tree's itd_decompose_f32
  residual         select = [-1]
  rot 2-4 + res    select = [2, 3, 4, -1]
  residual f32     select = [-1], float32 rows

Every 4th step of a further region per variant of this tree carries the engine's own event pairs: the per-kernel times of k_extract
(level 0, level 1), k_kf_knots and k_kf_apply.  One JSON line per variant, then the conditions of the comparison.

usage: python tools/rowsel_bench.py [--parent-lib PATH] [--log2n 24] [--steps 20] [--warmup 3] [--runs 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import MAX_ITERATION, TIMING_STRIDE, sines_noise  # noqa: E402


def parent_step(path, x, n, M, rows, stream):
    """The parent library's full call as a step function (its own engine, through the C ABI both commits share)."""
    L = ctypes.CDLL(path)
    P, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    L.itd_engine_create.argtypes = [ctypes.POINTER(P), ctypes.c_int, I64, I32]
    L.itd_decompose_f32.argtypes = [P, P, I64, I32, I64, I32, P, P, P]
    L.itd_engine_destroy.argtypes = [P]
    L.itd_engine_destroy.restype = None
    h = P()
    rc = L.itd_engine_create(ctypes.byref(h), 0, n, 1)
    assert rc == 0, "itd_engine_create of the parent library: %d" % rc

    xp, rp, sp = x.data_ptr(), rows.data_ptr(), stream.cuda_stream

    def step():
        rc = L.itd_decompose_f32(h, xp, n, 1, n, M, rp, None, sp)
        assert rc == 0, rc
    return step, lambda: L.itd_engine_destroy(h)


def region(step, sync, steps):
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=150.0)
    args = ap.parse_args()
    assert args.runs >= 5, "at least five regions per variant"
    import torch
    import pyitd_amd
    from pyitd_amd.engine import TIME_EXTRACT, TIME_EXTRACT_L0, TIME_KF_APPLY, TIME_KF_KNOTS, selection_of
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    M, n = MAX_ITERATION, 1 << args.log2n
    x = torch.from_numpy(sines_noise(n, seed=0)).to(dev)[None]
    stream = torch.cuda.Stream(device=dev)
    rows = torch.empty(((M + 2) * n,), dtype=torch.float64, device=dev)        # every variant writes into the head of the same buffer
    eng = pyitd_amd.Engine(n, 1, 0)

    # every variant's step is one call of a C entry with arguments prepared here, the parent's and this tree's alike: no Python
    # wrapper (select= parsing, row-type checks) inside a timed region
    xp, rp, sp, L, h = x.data_ptr(), rows.data_ptr(), stream.cuda_stream, eng._L, eng._h

    def ours(select, dt):
        if select is None:
            def step():
                rc = L.itd_decompose_f32(h, xp, n, 1, n, M, rp, None, sp)
                assert rc == 0, rc
            return step
        mask, want_res, _ = selection_of(select, M)
        r32 = 1 if dt == np.float32 else 0

        def step():
            rc = L.itd_decompose_select_f32(h, xp, n, 1, n, M, mask, want_res, rp, r32, sp)
            assert rc == 0, rc
        return step
    variants = [("full", ours(None, np.float64), M + 2, 8), ("residual", ours([-1], np.float64), 1, 8),
                ("rot 2-4 + res", ours([2, 3, 4, -1], np.float64), 4, 8), ("residual f32", ours([-1], np.float32), 1, 4)]
    close_parent = None
    if args.parent_lib:
        pstep, close_parent = parent_step(args.parent_lib, x, n, M, rows, stream)
        variants.insert(0, ("parent full", pstep, M + 2, 8))
    for _, step, _, _ in variants:      # first calls (workspaces, the policy's first decisions), then the warm-up by time
        step()
        sync()
    eng.summary(1)
    t_w = time.perf_counter()
    while (time.perf_counter() - t_w) * 1e3 < args.warm_ms * len(variants):
        for _, step, _, _ in variants:
            for _ in range(8):
                step()
        sync()
    runs = {name: [] for name, _, _, _ in variants}
    for _ in range(args.runs):
        for name, step, _, _ in variants:
            for _ in range(args.warmup):
                step()
            runs[name].append(region(step, sync, args.steps))
    res = {}
    for name, step, S, esz in variants:
        r = runs[name]
        out = {"what": name, "rows_stored": S, "result_bytes": S * n * esz, "steps": args.steps, "runs_ms": [round(v, 4) for v in r],
               "median_ms": round(float(np.median(r)), 4), "spread_ms": round(max(r) - min(r), 4), "min_ms": round(min(r), 4), "max_ms": round(max(r), 4)}
        if name != "parent full":
            for _ in range(args.warmup):
                step()
            eng.set_timing(args.steps, stride=TIMING_STRIDE)
            region(step, sync, args.steps)
            k = {}
            for key, t in (("k_extract_level0_us", TIME_EXTRACT_L0), ("k_extract_level1_us", TIME_EXTRACT), ("k_kf_knots_us", TIME_KF_KNOTS), ("k_kf_apply_us", TIME_KF_APPLY)):
                s = eng.kernel_timing_samples(t) * 1e3
                k[key] = round(float(np.median(s)), 2) if len(s) else None
            eng.set_timing(0)
            out["per_kernel_median"] = k
            out["fuse_level"], out["fuse_repeats"] = eng.last_fuse_level, eng.fuse_repeats
        res[name] = out
        print(json.dumps(out), flush=True)
    # the conditions: the parent is the yardstick (without it: this tree's full call, said so)
    ref = res.get("parent full", res["full"])
    verdict = {"what": "conditions", "yardstick": ref["what"], "yardstick_range_ms": [ref["min_ms"], ref["max_ms"]], "yardstick_spread_ms": ref["spread_ms"]}
    if "parent full" in res:
        verdict["full_median_within_parent_range"] = bool(ref["min_ms"] <= res["full"]["median_ms"] <= ref["max_ms"])
        verdict["full_runs_outside_parent_range"] = int(sum(not (ref["min_ms"] <= v <= ref["max_ms"]) for v in runs["full"]))
    for name, _, S, _ in variants:
        if name in ("parent full", "full"):
            continue
        gain = ref["median_ms"] - res[name]["median_ms"]
        verdict[name] = {"ratio_to_yardstick": round(res[name]["median_ms"] / ref["median_ms"], 4), "gain_ms": round(gain, 4),
                         "faster_by_more_than_the_spread": bool(gain > ref["spread_ms"]), "required": S <= 2}
    print(json.dumps(verdict), flush=True)
    eng.close()
    if close_parent:
        close_parent()


if __name__ == "__main__":
    main()
