"""The time-frequency-energy spectrum (pyitd_amd.tfe_spectrum, weight "energy") against what a caller has without it, over the same
device-resident float64 rows in the same process, the forms alternating:
    (a) pyitd_amd.instantaneous_batch(want=("amplitude", "frequency")) alone — the arithmetic the spectrum also does, with 16 B per
        sample written where the spectrum writes 8 F / hop;
    (b) the composition: (a), then torch.bucketize over the edges and index_add_ of A * A into a [R, T, F] tensor (float atomics:
        its sums change from run to run).
Shapes: 9 x 2^24 with hop 16384 (T = 1024) and F = 256; 9216 x 2^16 with hop 1024 and F = 64; edges uniform over [0, 0.5].

Before timing, the spectrum's first result is compared bit for bit with the definition's numpy statement (tests/spectrum_ref.py) fed
with (a)'s amplitude and frequency, on a sample of cells.  Then --runs runs of --reps alternating repetitions; per run and form the
median and the range (host clock around the public call on CUDA tensors, which ends in a synchronisation; output allocation
included on every side).  One JSON line per shape: the runs, each form's median over all repetitions, the two comparisons the
spectrum is held to — its median no more than (a)'s and below (b)'s, no margin — and its byte model (8 + 8 B read per sample,
8 F / hop B written) as a rate and as a share of the 8 TB/s HBM peak.
usage: python tools/tfe_spectrum_bench.py [--runs 3] [--reps 7] [--shapes 9x24:16384:256,9216x16:1024:64] [--only-spectrum]
(a shape is ROWSxN:HOP:F; an N of up to 31 is log2 of the row length; --only-spectrum: the new call alone, for a kernel trace)"""
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
import spectrum_ref  # noqa: E402
from instantaneous_batch_bench import PEAK, make_rows  # noqa: E402


def composition(x, edges, hop):
    """The energy spectrum from what exists without the call.  x[R, n] float64, edges[F + 1] float64, on the GPU."""
    R, n = x.shape
    F, T = edges.numel() - 1, -(-n // hop)
    amp, freq = pyitd_amd.instantaneous_batch(x, want=("amplitude", "frequency"))
    inside = (freq >= edges[0]) & (freq < edges[-1])
    k = torch.bucketize(freq, edges, right=True) - 1
    cell = (torch.arange(n, device=x.device) // hop * F)[None, :] + (torch.arange(R, device=x.device) * (T * F))[:, None]
    idx = torch.where(inside, cell + k, torch.zeros((), dtype=torch.int64, device=x.device))
    w = torch.where(inside, amp * amp, torch.zeros((), dtype=x.dtype, device=x.device))
    S = torch.zeros(R * T * F, dtype=torch.float64, device=x.device)
    S.index_add_(0, idx.reshape(-1), w.reshape(-1))
    torch.cuda.synchronize()
    return S.reshape(R, T, F)


def clock(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(ts):
    return {"median_ms": round(statistics.median(ts) * 1e3, 4), "range_ms": [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]}


def sample_check(x, edges, hop, got, cells=48):
    """The spectrum's cells against spectrum_ref on instantaneous_batch's outputs, on a sample of (row, time bin) pairs."""
    R, n = x.shape
    T = got.power.shape[1]
    amp, freq = pyitd_amd.instantaneous_batch(x, want=("amplitude", "frequency"))
    rng = np.random.default_rng(R + n)
    pairs = {(0, 0), (R - 1, T - 1)} | {(int(rng.integers(R)), int(rng.integers(T))) for _ in range(cells)}
    e = edges.cpu().numpy()
    same = True
    for r, t in sorted(pairs):
        lo, hi = t * hop, min(n, (t + 1) * hop)
        S, out = spectrum_ref.spectrum_ref(amp[r, lo:hi].cpu().numpy(), freq[r, lo:hi].cpu().numpy(), e, hop, "energy")
        same &= np.array_equal(got.power[r, t].cpu().numpy().view(np.uint64), S[0].view(np.uint64))
        same &= int(got.outside[r, t]) == int(out[0])
    return bool(same), len(pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="9x24:16384:256,9216x16:1024:64")
    ap.add_argument("--only-spectrum", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()           # (torch's HIP runtime first, the library's behind it)
    for s in a.shapes.split(","):
        shape, hop, F = s.split(":")
        r, e = shape.split("x")
        R, n, hop, F = int(r), (1 << int(e) if int(e) <= 31 else int(e)), int(hop), int(F)
        T = -(-n // hop)
        x = make_rows(R, n, seed=R + n)
        edges = torch.linspace(0.0, 0.5, F + 1, dtype=torch.float64, device="cuda")
        e_host = edges.cpu().numpy()
        forms = {"spectrum": lambda: pyitd_amd.tfe_spectrum(x, e_host, hop),
                 "instantaneous_a_f": lambda: pyitd_amd.instantaneous_batch(x, want=("amplitude", "frequency")),
                 "composition": lambda: composition(x, edges, hop)}
        if a.only_spectrum:
            forms = {"spectrum": forms["spectrum"]}
        # warm-up of every form, and the comparison
        got = pyitd_amd.tfe_spectrum(x, e_host, hop)
        same, cells = sample_check(x, edges, hop, got)
        inside = float(got.power.numel() and 1.0 - got.outside.sum().item() / (R * n))
        del got
        for f in forms.values():
            f()
        torch.cuda.empty_cache()
        runs, every = [], {k: [] for k in forms}
        for _ in range(a.runs):
            ts = {k: [] for k in forms}
            for _ in range(a.reps):
                for k, f in forms.items():
                    ts[k].append(clock(f))
            runs.append({k: stats(v) for k, v in ts.items()})
            for k, v in ts.items():
                every[k] += v
        med = {k: statistics.median(v) for k, v in every.items()}
        nbytes = R * n * 16 + R * T * F * 8
        line = {"rows": R, "n": n, "hop": hop, "T": T, "F": F, "weight": "energy", "dtype_in": "float64",
                "spectrum_bit_identical_to_reference_on_sample": same, "cells_compared": cells, "samples_inside_the_edges": round(inside, 4),
                "runs": runs, "reps_per_run": a.reps,
                "median_ms": {k: round(v * 1e3, 4) for k, v in med.items()},
                "spectrum_model_bytes": nbytes, "spectrum_TBps": round(nbytes / med["spectrum"] / 1e12, 3),
                "spectrum_frac_of_hbm_peak": round(nbytes / med["spectrum"] / PEAK, 3)}
        if not a.only_spectrum:
            line["spectrum_no_slower_than_instantaneous_a_f"] = bool(med["spectrum"] <= med["instantaneous_a_f"])
            line["spectrum_faster_than_composition"] = bool(med["spectrum"] < med["composition"])
        print(json.dumps(line), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
