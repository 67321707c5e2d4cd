"""Microseconds per push of the table stream (pyitd_amd.streaming.WaveTableStream, device form), steady state, float64 rows on the
device, L = 1024, rows in {9, 9 * 64}, beside, in the same run and by tools/wave_stream_bench.py's method,

  * WaveFilterStream.push_dev at H = 1024;
  * InstantaneousStream.push_dev at H = 1024 (amplitude, phase, frequency and length);
  * LevelsStream.push_dev at L = 1024, 8 levels, rows / 9 channels: the stage whose rows these streams consume;
  * itd_waves_batch_f64 over the arriving block alone.  THAT TABLE IS WRONG AT THE BLOCK'S EDGES (a half wave cut by the block looks
    shorter and smaller than it is); it stands here for its cost only.

The forms run in one process, alternating, `--reps` times each; every figure is the median of the repetitions' means, with the spread
(min .. max) behind it.  Rows: white noise, a random walk and a sine in noise, in turn.  The last column says whether a table push
costs no more than a wave-filter push at the same rows, the margin being the spread of the filter's own figure in this run.
usage: python tools/table_stream_bench.py [--pushes 200] [--reps 3] > profiles/r27/table_stream.txt"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyitd_amd import Engine, streaming  # noqa: E402
from wave_stream_bench import rows_signal, timed  # noqa: E402

L = 1024
H = 1024
LEVELS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    print("# table stream, us per push (device form, steady state), L = %d, float64 rows on the device" % L)
    print("# filter = WaveFilterStream.push_dev, instant = InstantaneousStream.push_dev (four outputs), both at H = %d" % H)
    print("# levels = LevelsStream.push_dev, %d levels, rows / 9 channels; batch = itd_waves_batch_f64 over the arriving block alone:" % LEVELS)
    print("# wrong at the block's edges, here for its cost only; median of %d repetitions of %d pushes (min .. max)" % (a.reps, a.pushes))
    for rows in (9, 9 * 64):
        nb = 16
        n = nb * L
        x = torch.from_numpy(rows_signal(rng, rows, n)).cuda()
        S1 = L + 1
        tabs = [torch.empty(rows, S1, dtype=torch.int64, device="cuda") for _ in range(3)]
        val = torch.empty(rows, S1, dtype=torch.float64, device="cuda")
        cnt = torch.empty(rows, dtype=torch.int32, device="cuda")
        tabs32 = [torch.empty(rows, S1, dtype=torch.int32, device="cuda") for _ in range(3)]
        bounds = torch.tensor([0.1, 10.0, 2.0, float(H)], dtype=torch.float64, device="cuda")
        out = [torch.empty(rows, L, dtype=torch.float64, device="cuda") for _ in range(3)]
        ilen = torch.empty(rows, L, dtype=torch.int32, device="cuda")
        icnt = torch.empty(rows, 2, dtype=torch.int32, device="cuda")
        C = rows // 9
        xl = x[:C]
        lrows = torch.empty(C, LEVELS + 1, L, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        eng = Engine(L, 1)

        def blk(k):
            return x[:, (k % nb) * L:].data_ptr()

        def table_form():
            st = streaming.WaveTableStream(L, rows)
            us = timed(lambda k: st.push_dev(blk(k), n, tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), val.data_ptr(), S1,
                                             cnt.data_ptr(), s), a.pushes, 8, ts)
            st.close()
            return us

        def filter_form():
            st = streaming.WaveFilterStream(L, rows, H)
            us = timed(lambda k: st.push_dev(blk(k), n, bounds.data_ptr(), 0, out[0].data_ptr(), L, s), a.pushes, 8, ts)
            st.close()
            return us

        def instant_form():
            st = streaming.InstantaneousStream(L, rows, H)
            us = timed(lambda k: st.push_dev(blk(k), n, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ilen.data_ptr(), L,
                                             icnt.data_ptr(), 2, s), a.pushes, 8, ts)
            st.close()
            return us

        def levels_form():
            st = streaming.LevelsStream(L, LEVELS, C)
            us = timed(lambda k: st.push_dev(xl[:, (k % nb) * L:].data_ptr(), n, lrows.data_ptr(), L, (LEVELS + 1) * L, None, s),
                       a.pushes, LEVELS + 8, ts)
            st.close()
            return us

        def batch_form():
            return timed(lambda k: eng.waves_batch_dev(blk(k), np.float64, L, rows, n, tabs32[0].data_ptr(), tabs32[1].data_ptr(),
                                                       tabs32[2].data_ptr(), val.data_ptr(), S1, S1, cnt.data_ptr(), None, s), a.pushes, 8, ts)

        forms = (("table", table_form), ("filter", filter_form), ("instant", instant_form), ("levels", levels_form), ("batch", batch_form))
        res = {name: [] for name, _ in forms}
        for _ in range(a.reps):
            for name, form in forms:
                res[name].append(form())
        eng.close()

        def fmt(v):
            return "%8.1f (%.1f .. %.1f)" % (statistics.median(v), min(v), max(v))
        margin = max(res["filter"]) - min(res["filter"])
        holds = statistics.median(res["table"]) <= statistics.median(res["filter"]) + margin
        print("rows=%4d  %s  table <= filter + %.1f: %s" % (rows, "  ".join("%s %s" % (name, fmt(res[name])) for name, _ in forms), margin,
                                                           "yes" if holds else "NO"), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
