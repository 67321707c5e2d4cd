"""The host cost of a many-row call where it is all there is: the five operators of pyitd_amd.batch on rows of shape (2, 3, 1030) —
six rows of three tiles; the kernels take a few microseconds —, each on numpy rows (staged through the C ABI's buffers) and on the
same rows as a torch CUDA tensor (used in place).  Host clock around the public call, which ends synchronised in both forms;
output allocation, upload and download included.  Per form: --runs runs of --calls calls after a warm-up, the forms alternating
run by run; the best and the median call of every run.  One JSON line per form.

To compare two trees, run the tool in a checkout of each, alternating, and take the spread of one tree's own runs as the noise.
usage: python tools/many_row_forms_bench.py [--runs 3] [--calls 300] [--warmup 30]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyitd_amd  # noqa: E402

EDGES = np.linspace(0.0, 0.5, 65)
AE, LE = np.geomspace(1e-3, 8.0, 33), np.geomspace(1.0, 1031.0, 33)
OPERATORS = {
    "instantaneous_batch": lambda r: pyitd_amd.instantaneous_batch(r),
    "tfe_spectrum": lambda r: pyitd_amd.tfe_spectrum(r, EDGES, 512),
    "single_waves": lambda r: pyitd_amd.single_waves(r),
    "single_waves_cap": lambda r: pyitd_amd.single_waves(r, cap=600),
    "wave_filter": lambda r: pyitd_amd.wave_filter(r, amplitude=(0.5, 2.0), length=(2, 40)),
    "wave_histogram": lambda r: pyitd_amd.wave_histogram(r, AE, LE, hop=512),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    torch.cuda.init()           # (torch's HIP runtime first, the library's behind it)
    rows = np.random.default_rng(1030).standard_normal((2, 3, 1030))
    forms = {}
    for name, f in OPERATORS.items():
        forms[name + " numpy"] = (f, rows)
        forms[name + " tensor"] = (f, torch.from_numpy(rows).cuda())
    for f, r in forms.values():
        for _ in range(a.warmup):
            f(r)
    best, med = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(a.runs):
        for k, (f, r) in forms.items():
            ts = []
            for _ in range(a.calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f(r)
                ts.append(time.perf_counter() - t0)
            best[k].append(round(min(ts) * 1e6, 1))
            med[k].append(round(statistics.median(ts) * 1e6, 1))
    for k in forms:
        print(json.dumps({"form": k, "rows_shape": [2, 3, 1030], "calls_per_run": a.calls, "best_us": best[k], "median_us": med[k]}), flush=True)


if __name__ == "__main__":
    main()
