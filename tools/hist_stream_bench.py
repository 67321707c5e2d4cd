"""Microseconds per push of the histogram stream (pyitd_amd.streaming.WaveHistogramStream, device form), steady state, float64 rows on
the device, L = 1024, 32 x 32 log-spaced bins, hop in {512, 1024}, rows in {9, 9 * 64}, H in {1024, 8192, 65536}, beside

  * what a caller had before the stream for the same job: on every push a contiguous device copy of the (2 D + 1) L window
    followed by itd_wave_hist_batch_f64 over it.  THIS COMPOSITION IS WRONG AT THE WINDOW'S EDGES (a half wave cut by the window looks
    shorter and smaller than it is, and its peak may lie elsewhere); it stands here for its cost only;
  * LevelsStream.push_dev at L = 1024, 8 levels, rows / 9 channels: the stage whose rows the histogram stream consumes.

Before any timing the stream's concatenated slices are compared integer for integer with pyitd_amd.wave_histogram of the same rows,
at a horizon that holds every half wave.  The three forms run in one process, alternating, `--reps` times each; every figure is the
median of the repetitions' means, with the spread (min .. max) behind it.  Rows: white noise, a random walk (long half waves: the
searches run far) and a sine in noise, in turn.  usage: python tools/hist_stream_bench.py [--pushes 200] [--reps 3] > profiles/r24/hist_stream.txt"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyitd_amd  # noqa: E402
from pyitd_amd import Engine, streaming  # noqa: E402

L = 1024
NA = NL = 32
LEVELS = 8


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


def check(rng, ae, le):
    """the stream's slices against the whole-row call, at a horizon that holds every half wave"""
    x = rows_signal(rng, 9, 16 * L)
    H = int(pyitd_amd.single_waves(x).length.max())
    for hop in (512, 1024):
        got = streaming.blockwise_wave_histogram(x, L, H, ae, le, hop)
        want = pyitd_amd.wave_histogram(x, ae, le, hop)
        same = (np.array_equal(got.count, want.count) and np.array_equal(got.samples, want.samples)
                and np.array_equal(got.outside, want.outside) and not got.overlong.any())
        print("# check: 9 rows of %d samples, H = %d (the longest half wave), hop = %d: %d half waves in cells, %d outside: %s"
              % (16 * L, H, hop, int(want.count.sum()), int(want.outside.sum()), "the same integers" if same else "DIFFERENT"), flush=True)
        if not same:
            sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="rows,H,hop: one shape, the stream's form alone (for a kernel trace)")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    ae_h, le_h = np.geomspace(1e-3, 1e3, NA + 1), np.geomspace(1.0, 2.0 ** 18, NL + 1)
    only = tuple(int(v) for v in a.only.split(",")) if a.only else None
    print("# histogram stream, us per push (device form, steady state), L = %d, %d x %d log-spaced bins, float64 rows on the device" % (L, NA, NL))
    print("# composition = device copy of the (2D+1) L window + itd_wave_hist_batch_f64: wrong at the window's edges, here for its cost only")
    print("# levels = LevelsStream.push_dev, L = %d, %d levels, rows / 9 channels; median of %d repetitions of %d pushes (min .. max)"
          % (L, LEVELS, a.reps, a.pushes))
    print("# (the composition: %d pushes per repetition where its window exceeds 1224 blocks over all rows)" % max(20, a.pushes // 8))
    if not only:
        check(rng, ae_h, le_h)
    ae, le = torch.from_numpy(ae_h).cuda(), torch.from_numpy(le_h).cuda()
    for rows in (9, 9 * 64):
        for H in (1024, 8192, 65536):
            D = -(-H // L)
            W = 2 * D + 1
            nb = W + 8
            n = nb * L
            if only and only[:2] != (rows, H):
                continue
            x = torch.from_numpy(rows_signal(rng, rows, n)).cuda()
            win = torch.empty(rows, W * L, dtype=torch.float64, device="cuda")
            C = rows // 9
            xl = x[:C]
            lrows = torch.empty(C, LEVELS + 1, L, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            eng = Engine(W * L, 1)
            pushes = a.pushes if rows * W <= 9 * 17 * 8 else max(20, a.pushes // 8)       # (the composition moves the whole window)
            for hop in (512, 1024):
                if only and only[2] != hop:
                    continue
                cells = L // hop
                F = cells * NA * NL
                hist = torch.empty(2, rows, F, dtype=torch.int32, device="cuda")
                counts = torch.empty(2, rows, cells, dtype=torch.int32, device="cuda")
                T = W * L // hop
                whist = torch.empty(2, rows, T * NA * NL, dtype=torch.int32, device="cuda")
                wout = torch.empty(rows, T, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()

                def stream_form():
                    st = streaming.WaveHistogramStream(L, rows, H, ae_h, le_h, hop)
                    us = timed(lambda k: st.push_dev(x[:, (k % nb) * L:].data_ptr(), n, ae.data_ptr(), 0, le.data_ptr(), 0, hist[0].data_ptr(),
                                                     hist[1].data_ptr(), F, counts[0].data_ptr(), counts[1].data_ptr(), cells, s),
                               a.pushes, W + 8, ts)
                    st.close()
                    return us

                def composition():
                    def step(k):
                        with torch.cuda.stream(ts):
                            win.copy_(x[:, (k % 8) * L:(k % 8 + W) * L])
                        eng.wave_hist_batch_dev(win.data_ptr(), np.float64, W * L, rows, W * L, ae.data_ptr(), 0, NA, le.data_ptr(), 0, NL, hop,
                                                whist[0].data_ptr(), whist[1].data_ptr(), T * NA * NL, wout.data_ptr(), None, s)
                    return timed(step, pushes, 5, ts)

                def levels_form():
                    st = streaming.LevelsStream(L, LEVELS, C)
                    us = timed(lambda k: st.push_dev(xl[:, (k % nb) * L:].data_ptr(), n, lrows.data_ptr(), L, (LEVELS + 1) * L, None, s),
                               a.pushes, LEVELS + 8, ts)
                    st.close()
                    return us

                if only:
                    print("rows=%4d H=%6d hop=%4d D=%3d  stream %9.1f" % (rows, H, hop, D, stream_form()), flush=True)
                    continue
                res = {"stream": [], "composition": [], "levels": []}
                for _ in range(a.reps):
                    res["stream"].append(stream_form())
                    res["composition"].append(composition())
                    res["levels"].append(levels_form())

                def fmt(v):
                    return "%9.1f (%.1f .. %.1f)" % (statistics.median(v), min(v), max(v))
                print("rows=%4d H=%6d hop=%4d D=%3d  stream %s  composition %s  levels %s"
                      % (rows, H, hop, D, fmt(res["stream"]), fmt(res["composition"]), fmt(res["levels"])), flush=True)
                del hist, counts, whist, wout
            eng.close()
            del x, win
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
