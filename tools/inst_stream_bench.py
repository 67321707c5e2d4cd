"""Microseconds per push of the instantaneous stream (pyitd_amd.streaming.InstantaneousStream, device form, all four outputs and
the counts), steady state, float64 rows on the device, L = 1024, rows in {9, 9 * 64}, H in {1024, 8192, 65536}, beside

  * what a caller had before the stream for the same job: on every push a contiguous device copy of the (2 D + 1) L window
    followed by itd_instantaneous_batch_f64 over it (three outputs; it has no length).  THIS COMPOSITION IS WRONG AT THE WINDOW'S
    EDGES (a half wave cut by the window looks shorter and smaller than it is); it stands here for its cost only;
  * LevelsStream.push_dev at L = 1024, 8 levels, rows / 9 channels: the stage whose rows the instantaneous stream consumes.

The three forms run in one process, alternating, `--reps` times each; every figure is the median of the repetitions' means, with
the spread (min .. max) behind it.  Rows: white noise, a random walk (long half waves: the searches run far) and a sine in noise,
in turn.  The byte model of a push is 8 L in and into the ring, 8 L read again, 28 L written per row: 44 L bytes; the last column
is that over the stream's median, as a fraction of the 8 TB/s HBM peak.
usage: python tools/inst_stream_bench.py [--pushes 200] [--reps 3] > profiles/r22/inst_stream.txt"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyitd_amd import Engine, streaming  # noqa: E402

L = 1024
LEVELS = 8
HBM_PEAK = 8.0e12


def rows_signal(rng, rows, n):
    t = np.arange(n) / n
    x = np.empty((rows, n))
    for r in range(rows):
        if r % 3 == 0:
            x[r] = rng.standard_normal(n)
        elif r % 3 == 1:
            x[r] = np.cumsum(rng.standard_normal(n))
        else:
            x[r] = np.sin(2 * np.pi * rng.uniform(5, 500) * t) + 0.1 * rng.standard_normal(n)
    return x


def timed(step, pushes, warm, ts):
    for k in range(warm):
        step(k)
    ts.synchronize()
    t0 = time.perf_counter()
    for k in range(pushes):
        step(warm + k)
    ts.synchronize()
    return (time.perf_counter() - t0) / pushes * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="rows,H: one shape, the stream's form alone (for a kernel trace)")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    print("# instantaneous stream, us per push (device form, steady state), L = %d, four outputs and counts, float64 rows on the device" % L)
    print("# composition = device copy of the (2D+1) L window + itd_instantaneous_batch_f64: wrong at the window's edges, here for its cost only")
    print("# levels = LevelsStream.push_dev, L = %d, %d levels, rows / 9 channels; median of %d repetitions of %d pushes (min .. max)"
          % (L, LEVELS, a.reps, a.pushes))
    print("# (the composition: %d pushes per repetition where its window exceeds 1224 blocks over all rows)" % max(20, a.pushes // 8))
    print("# model = 44 L bytes per row and push over the stream's median, as a fraction of the %.0f TB/s HBM peak" % (HBM_PEAK / 1e12))
    only = tuple(int(v) for v in a.only.split(",")) if a.only else None
    for rows in (9, 9 * 64):
        for H in (1024, 8192, 65536):
            D = -(-(H + 1) // L)
            W = 2 * D + 1
            nb = W + 8
            n = nb * L
            if only and only != (rows, H):
                continue
            x = torch.from_numpy(rows_signal(rng, rows, n)).cuda()
            C = rows // 9
            xl = x[:C]
            lrows = torch.empty(C, LEVELS + 1, L, dtype=torch.float64, device="cuda")
            out = torch.empty(3, rows, L, dtype=torch.float64, device="cuda")
            length = torch.empty(rows, L, dtype=torch.int32, device="cuda")
            counts = torch.empty(rows, 2, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def stream_form():
                st = streaming.InstantaneousStream(L, rows, H)
                us = timed(lambda k: st.push_dev(x[:, (k % nb) * L:].data_ptr(), n, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                 length.data_ptr(), L, counts.data_ptr(), 2, s), a.pushes, W + 8, ts)
                st.close()
                return us

            if only:
                print("rows=%4d H=%6d D=%3d  stream %9.1f" % (rows, H, D, stream_form()), flush=True)
                continue
            win = torch.empty(rows, W * L, dtype=torch.float64, device="cuda")
            wout = torch.empty(3, rows, W * L, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            eng = Engine(W * L, 1)
            pushes = a.pushes if rows * W <= 9 * 17 * 8 else max(20, a.pushes // 8)       # (the composition moves the whole window)

            def composition():
                def step(k):
                    with torch.cuda.stream(ts):
                        win.copy_(x[:, (k % 8) * L:(k % 8 + W) * L])
                    eng.instantaneous_batch_dev(win.data_ptr(), np.float64, W * L, rows, W * L, wout[0].data_ptr(), wout[1].data_ptr(),
                                                wout[2].data_ptr(), W * L, False, None, s)
                return timed(step, pushes, 5, ts)

            def levels_form():
                st = streaming.LevelsStream(L, LEVELS, C)
                us = timed(lambda k: st.push_dev(xl[:, (k % nb) * L:].data_ptr(), n, lrows.data_ptr(), L, (LEVELS + 1) * L, None, s),
                           a.pushes, LEVELS + 8, ts)
                st.close()
                return us

            res = {"stream": [], "composition": [], "levels": []}
            for _ in range(a.reps):
                res["stream"].append(stream_form())
                res["composition"].append(composition())
                res["levels"].append(levels_form())

            def fmt(v):
                return "%9.1f (%.1f .. %.1f)" % (statistics.median(v), min(v), max(v))
            frac = 44.0 * L * rows / (statistics.median(res["stream"]) * 1e-6) / HBM_PEAK
            print("rows=%4d H=%6d D=%3d  stream %s  composition %s  levels %s  model %.4f"
                  % (rows, H, D, fmt(res["stream"]), fmt(res["composition"]), fmt(res["levels"]), frac), flush=True)
            eng.close()
            del x, win, wout
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
