"""The wave filter's bounds from histogram quantiles (pyitd_amd.wave_filter_bounds, streaming.WaveBoundsStream) against what a caller
has without them, over the same device-resident histograms in the same process, the forms alternating.  In every case the results are
compared bit for bit first.

  (a) the many-row call against its torch composition (sum over time and the other axis, cumsum, compare, gather) on the `count`
      histograms (tools/wave_histogram_bench.py's rows: itd_batch's 8-level decomposition of the benchmark's signals, 32 x 32
      log-spaced bins) at 9 x 2^24 with hop 4096 (T = 4096) and 9216 x 2^16 with one time bin.  Host clock around the public call
      on CUDA tensors, which ends in a synchronisation; --runs runs of --reps alternating repetitions.  One JSON line per shape with
      the byte model (4 B read per cell, 1 KB per row of workspace zeroed, added to and read) as a share of the 8 TB/s HBM peak.
  (b) the stream's push (device form, steady state) at 9 and 576 rows, 32 x 32 bins, 2 slices per push, a window of 8 pushes, against
      the same composition over a window tensor the caller keeps (one slice copy plus the composition per push) and against
      WaveHistogramStream.push_dev (L = 1024, hop 512, H = 1024) in the same run, by tools/wave_stream_bench.py's method: medians
      and ranges of --reps repetitions of --pushes pushes, microseconds per push.
usage: python tools/wave_bounds_bench.py [--runs 3] [--reps 7] [--pushes 200] [--shapes 1x24x4096,1024x16x0] > profiles/r28/wave_bounds.txt
(a shape is SIGNALSxLOG2NxHOP; hop 0 is one time bin)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyitd_amd  # noqa: E402
from pyitd_amd import streaming  # noqa: E402
from wave_histogram_bench import BINS, PEAK, clock, decomposition, stats  # noqa: E402
from wave_stream_bench import rows_signal, timed  # noqa: E402

Q = (0.1, 0.9, 0.05, 0.95, 1.0, 1.0, 1.0, 1.0)
L, HOP, H, WINDOW = 1024, 512, 1024, 8


def first(mask, none):
    """per row the first True of mask[R, B], `none` where there is none (argmax returns the first of equal maxima)"""
    return torch.where(mask.any(dim=1), mask.to(torch.int8).argmax(dim=1), none)


def composition(hist, ae, le, q=Q):
    """bounds[R, 4] float64 from what torch has: hist[R, T, Na, Nl] int32, ae / le float64 [N + 1], all on the GPU"""
    out = []
    for m, e, k in ((hist.sum(dim=(1, 3), dtype=torch.int64), ae, 0), (hist.sum(dim=(1, 2), dtype=torch.int64), le, 1)):
        B = m.shape[1]
        cum = m.cumsum(dim=1)
        N = cum[:, -1:]
        c, Nf = cum.to(torch.float64), N.to(torch.float64)
        last = torch.full((m.shape[0],), B - 1, dtype=torch.int64, device=m.device)
        iL = first(c > q[2 * k] * Nf, first(cum == N, last))
        iU = torch.maximum(iL, first(c >= q[2 * k + 1] * Nf, last))
        empty = N[:, 0] == 0
        iL, iU = torch.where(empty, torch.zeros_like(iL), iL), torch.where(empty, last, iU)
        out += [e[iL] * q[4 + 2 * k], e[iU + 1] * q[5 + 2 * k]]
    return torch.stack(out, dim=1)


def many_rows(a):
    for s in a.shapes.split(","):
        B, e, hop = (int(v) for v in s.split("x"))
        n = 1 << e
        x, _ = decomposition(B, n)
        R = x.shape[0]
        top = float(x.abs().max())
        ae, le = np.geomspace(top * 1e-5, top * (1.0 + 1e-9), BINS + 1), np.geomspace(1.0, n + 1.0, BINS + 1)
        d_ae, d_le = torch.from_numpy(ae).cuda(), torch.from_numpy(le).cuda()
        hist = pyitd_amd.wave_histogram(x, ae, le, hop=hop or None).count
        del x
        torch.cuda.empty_cache()
        T = hist.shape[1]
        forms = {"bounds": lambda: pyitd_amd.wave_filter_bounds(hist, ae, le, Q[0:2], Q[2:4]),
                 "composition": lambda: composition(hist, d_ae, d_le)}
        got, want = forms["bounds"](), forms["composition"]()
        torch.cuda.synchronize()
        line = {"rows": R, "n": n, "hop": hop or None, "T": T, "bins": [BINS, BINS], "half_waves": int(hist.sum()),
                "bit_exact_against_the_composition": bool(torch.equal(got.view(torch.int64), want.view(torch.int64)))}
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
        nbytes = hist.numel() * 4 + R * 1024 * 3
        line.update({"runs": runs, "reps_per_run": a.reps, "median_ms": {k: round(v * 1e3, 4) for k, v in med.items()},
                     "bounds_model_bytes": nbytes, "bounds_TBps": round(nbytes / med["bounds"] / 1e12, 3),
                     "bounds_frac_of_hbm_peak": round(nbytes / med["bounds"] / PEAK, 3),
                     "bounds_no_slower_than_composition": bool(med["bounds"] <= med["composition"])})
        print(json.dumps(line), flush=True)
        del hist
        torch.cuda.empty_cache()


def stream_pushes(a):
    rng = np.random.default_rng(0)
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    C = L // HOP
    print("# bounds stream, us per push (device form, steady state), %d x %d bins, %d slices per push, window %d pushes" % (BINS, BINS, C, WINDOW))
    print("# composition = one slice copy into a window tensor plus sum, cumsum, compare, gather in torch; histogram = WaveHistogramStream.push_dev,")
    print("# L = %d, hop %d, H = %d; median of %d repetitions of %d pushes (min .. max)" % (L, HOP, H, a.reps, a.pushes))
    for rows in (9, 9 * 64):
        nb = 16
        n = nb * L
        x = torch.from_numpy(rows_signal(rng, rows, n)).cuda()
        ae, le = np.geomspace(1e-4, float(x.abs().max()) * 1.001, BINS + 1), np.geomspace(1.0, H + 1.0, BINS + 1)
        d_ae, d_le, d_q = torch.from_numpy(ae).cuda(), torch.from_numpy(le).cuda(), torch.tensor(Q, dtype=torch.float64, device="cuda")
        # the slices the histogram stream emits for these rows, kept for the bounds forms
        hs = streaming.WaveHistogramStream(L, rows, H, ae, le, HOP)
        slices = []
        for k in range(nb):
            out = hs.push(x[:, k * L:(k + 1) * L].cpu().numpy())
            if out is not None:
                slices.append(torch.from_numpy(out.count).cuda())
        hs.close()
        F = C * BINS * BINS
        count, samples = (torch.empty(rows, C, BINS, BINS, dtype=torch.int32, device="cuda") for _ in range(2))
        bounds = torch.empty(rows, 4, dtype=torch.float64, device="cuda")
        win = torch.zeros(rows, WINDOW, C, BINS, BINS, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def bounds_step(st, k):
            st.push_dev(slices[k % len(slices)].data_ptr(), F, d_ae.data_ptr(), 0, d_le.data_ptr(), 0, d_q.data_ptr(), 0, bounds.data_ptr(), 4, None, s)

        def comp_step(k):
            win[:, k % WINDOW] = slices[k % len(slices)]
            return composition(win.view(rows, WINDOW * C, BINS, BINS), d_ae, d_le)

        # bit for bit first: WINDOW + 3 pushes through both
        st = streaming.WaveBoundsStream(rows, BINS, BINS, C, WINDOW)
        with torch.cuda.stream(ts):
            for k in range(WINDOW + 3):
                bounds_step(st, k)
                want = comp_step(k)
        ts.synchronize()
        st.close()
        exact = bool(torch.equal(bounds.view(torch.int64), want.view(torch.int64)))

        def bounds_form():
            st = streaming.WaveBoundsStream(rows, BINS, BINS, C, WINDOW)
            us = timed(lambda k: bounds_step(st, k), a.pushes, WINDOW + 2, ts)
            st.close()
            return us

        def comp_form():
            with torch.cuda.stream(ts):
                return timed(comp_step, a.pushes, WINDOW + 2, ts)

        def hist_form():
            st = streaming.WaveHistogramStream(L, rows, H, ae, le, HOP)
            us = timed(lambda k: st.push_dev(x[:, (k % nb) * L:].data_ptr(), n, d_ae.data_ptr(), 0, d_le.data_ptr(), 0, count.data_ptr(),
                                             samples.data_ptr(), F, None, None, 0, s), a.pushes, 8, ts)
            st.close()
            return us

        forms = (("bounds", bounds_form), ("composition", comp_form), ("histogram", hist_form))
        res = {name: [] for name, _ in forms}
        for _ in range(a.reps):
            for name, form in forms:
                res[name].append(form())

        def fmt(v):
            return "%8.1f (%.1f .. %.1f)" % (statistics.median(v), min(v), max(v))
        med = {k: statistics.median(v) for k, v in res.items()}
        print("rows=%4d  bit-exact: %s  %s  bounds < histogram: %s  bounds <= composition: %s" % (
            rows, "yes" if exact else "NO", "  ".join("%s %s" % (name, fmt(res[name])) for name, _ in forms),
            "yes" if med["bounds"] < med["histogram"] else "NO", "yes" if med["bounds"] <= med["composition"] else "NO"), flush=True)
        del x
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--shapes", default="1x24x4096,1024x16x0")
    ap.add_argument("--only", choices=("rows", "stream"), default=None)
    a = ap.parse_args()
    torch.cuda.init()           # (torch's HIP runtime first, the library's behind it)
    if a.only != "stream":
        many_rows(a)
    if a.only != "rows":
        stream_pushes(a)


if __name__ == "__main__":
    main()
