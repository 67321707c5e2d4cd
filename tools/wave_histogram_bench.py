"""The half waves' joint amplitude-length histogram (pyitd_amd.wave_histogram) against what a caller has without it, over the same
device-resident float64 rows in the same process, the forms alternating:
    (a) pyitd_amd.wave_filter on the same rows, one set of bounds — the context figure: the same two front launches and the same
        8 + 8 B read per sample, but 8 B per sample written where the histogram writes a few KB per row;
    (b) the composition the call replaces: pyitd_amd.single_waves (the table, 20 B per half wave padded to the largest count), then
        torch.bucketize over both edge sets and index_add_ of ones and lengths into [R, T, Na, Nl] int32 tensors.
Rows: a real decomposition — pyitd_amd.itd_batch (8 levels: 8 rotations and the residual, 9 rows per signal) of the benchmark's
sum-of-sines-plus-noise signals (tests/helpers.sines_noise, draw b mod 16, f * (1 + b / 8192)): 1 signal of 2^24 samples (9 x 2^24)
and 1024 signals of 2^16 samples (9216 x 2^16).  32 x 32 log-spaced bins, one edge set for every row (amplitude: five decades up to
the rows' largest magnitude; length: 1 .. n + 1), hop None (one time bin) and hop 4096.

Before timing, the histogram is compared integer for integer with (b)'s.  Then --runs runs of --reps alternating repetitions ((b):
--comp-reps per run); per run and form the median and the range (host clock around the public call on CUDA tensors, which ends in a
synchronisation; output allocation included on every side).  One JSON line per shape and hop: the runs, each form's median over all
repetitions, the two comparisons the call is held to — its median no more than (a)'s and below (b)'s, no margin — and its byte
model (8 + 8 B read per sample, 80 B per tile written and read, the slots zeroed) as a share of the 8 TB/s HBM peak.
usage: python tools/wave_histogram_bench.py [--runs 3] [--reps 7] [--comp-reps 3] [--shapes 1x24,1024x16] [--hops 0,4096]
       [--only-histogram]
(a shape is SIGNALSxLOG2N; hop 0 is None; --only-histogram: the new call and wave_filter alone, no comparison: for a kernel trace)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyitd_amd  # noqa: E402
from helpers import sines_noise  # noqa: E402

PEAK = 8.0e12
LEVELS = 8
BINS = 32


def decomposition(B, n):
    """[B * 9, n] float64 on the GPU: the rows of itd_batch over B of the benchmark's signals (a signal that stops early leaves
    zero rows: one half wave each)."""
    x = torch.from_numpy(np.stack([sines_noise(n, seed=b % 16, fscale=1.0 + b / 8192.0) for b in range(B)])).cuda()
    d = pyitd_amd.itd_batch(x, max_iteration=LEVELS - 1)
    rows = d["rows"]
    assert rows.shape == (B, LEVELS + 1, n) and rows.dtype == torch.float64
    return rows.reshape(B * (LEVELS + 1), n), torch.as_tensor(d["n_rows"]).cpu().tolist()


def composition(x, ae, le, hop):
    """(count, samples, outside) from what exists without the call.  x[R, n] float64, ae / le float64, on the GPU."""
    R, n = x.shape
    Na, Nl, T = ae.numel() - 1, le.numel() - 1, -(-n // hop)
    w = pyitd_amd.single_waves(x)
    cap = w.start.shape[1]
    valid = torch.arange(cap, device=x.device)[None, :] < w.count[:, None]
    A, ln = w.value.abs(), w.length.to(torch.float64)
    inside = valid & (A >= ae[0]) & (A < ae[-1]) & (ln >= le[0]) & (ln < le[-1])
    i = torch.bucketize(A, ae, right=True) - 1
    j = torch.bucketize(ln, le, right=True) - 1
    t = torch.arange(R, device=x.device)[:, None] * T + w.peak.to(torch.int64) // hop
    cell = ((t * Na + i) * Nl + j)[inside]
    count = torch.zeros(R * T * Na * Nl, dtype=torch.int32, device=x.device)
    samples = torch.zeros_like(count)
    count.index_add_(0, cell, torch.ones(cell.numel(), dtype=torch.int32, device=x.device))
    samples.index_add_(0, cell, w.length[inside])
    outside = torch.zeros(R * T, dtype=torch.int32, device=x.device)
    rest = t[valid & ~inside]
    outside.index_add_(0, rest, torch.ones(rest.numel(), dtype=torch.int32, device=x.device))
    torch.cuda.synchronize()
    return count.reshape(R, T, Na, Nl), samples.reshape(R, T, Na, Nl), outside.reshape(R, T)


def clock(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(ts):
    return {"median_ms": round(statistics.median(ts) * 1e3, 4), "range_ms": [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--comp-reps", type=int, default=3)
    ap.add_argument("--shapes", default="1x24,1024x16")
    ap.add_argument("--hops", default="0,4096")
    ap.add_argument("--only-histogram", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()           # (torch's HIP runtime first, the library's behind it)
    for s in a.shapes.split(","):
        B, e = (int(v) for v in s.split("x"))
        n = 1 << e
        x, n_rows = decomposition(B, n)
        R = x.shape[0]
        top = float(x.abs().max())
        ae = np.geomspace(top * 1e-5, top * (1.0 + 1e-9), BINS + 1)
        le = np.geomspace(1.0, n + 1.0, BINS + 1)
        d_ae, d_le = torch.from_numpy(ae).cuda(), torch.from_numpy(le).cuda()
        bounds = dict(amplitude=(float(ae[8]), float(ae[-1])), length=(float(le[4]), float(le[-1])))
        for hop in (int(h) for h in a.hops.split(",")):
            hop_arg = hop or None
            hop_eff = hop or -(-n // 512) * 512
            T = -(-n // hop_eff)
            forms = {"histogram": lambda: pyitd_amd.wave_histogram(x, ae, le, hop=hop_arg),
                     "wave_filter": lambda: pyitd_amd.wave_filter(x, **bounds),
                     "composition": lambda: composition(x, d_ae, d_le, hop_eff)}
            line = {"rows": R, "n": n, "signals": B, "n_rows_min_max": [min(n_rows), max(n_rows)], "hop": hop_arg, "T": T, "bins": [BINS, BINS],
                    "dtype_in": "float64"}
            got = pyitd_amd.wave_histogram(x, ae, le, hop=hop_arg)        # warm-up of every form, and the comparison
            waves = int(got.count.sum()) + int(got.outside.sum())
            line.update({"half_waves": waves, "half_waves_per_sample": round(waves / (R * n), 4),
                         "half_waves_outside": int(got.outside.sum()), "cells_touched": int((got.count != 0).sum())})
            if a.only_histogram:
                del forms["composition"]
            else:
                want = composition(x, d_ae, d_le, hop_eff)
                line["integer_exact_against_the_composition"] = bool(all(torch.equal(g, w) for g, w in zip(got, want)))
                del want
            del got
            forms["wave_filter"]()
            torch.cuda.empty_cache()
            runs, every = [], {k: [] for k in forms}
            for _ in range(a.runs):
                ts = {k: [] for k in forms}
                for rep in range(a.reps):
                    for k, f in forms.items():
                        if k != "composition" or rep < a.comp_reps:
                            ts[k].append(clock(f))
                runs.append({k: stats(v) for k, v in ts.items()})
                for k, v in ts.items():
                    every[k] += v
                torch.cuda.empty_cache()
            med = {k: statistics.median(v) for k, v in every.items()}
            tiles = -(-n // 512)
            nbytes = R * n * 16 + R * tiles * 160 + 2 * R * T * BINS * BINS * 4
            line.update({"runs": runs, "reps_per_run": a.reps, "median_ms": {k: round(v * 1e3, 4) for k, v in med.items()},
                         "histogram_model_bytes": nbytes, "histogram_TBps": round(nbytes / med["histogram"] / 1e12, 3),
                         "histogram_frac_of_hbm_peak": round(nbytes / med["histogram"] / PEAK, 3),
                         "histogram_no_slower_than_wave_filter": bool(med["histogram"] <= med["wave_filter"])})
            if not a.only_histogram:
                line["histogram_faster_than_composition"] = bool(med["histogram"] < med["composition"])
            print(json.dumps(line), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
