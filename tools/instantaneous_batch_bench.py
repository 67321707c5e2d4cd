"""The batched instantaneous step (itd_instantaneous_batch_f64 / _f32: three launches, no host round trip) against the loop of
single-row calls it replaces (itd_instantaneous_f64: one synchronous call per row), over the same device-resident rows in the same
process, the two alternating.  Shapes: 9 x 2^24, 9216 x 2^16, 60 000 x 256; each with float64 rows in and out and with float32
rows in and out.  The single-row operator takes float64 rows only: beside the float32 case the loop runs over a float64 copy of
the rows and writes float64 — the widening and narrowing a caller would add are NOT in its time.

One JSON line per case: the median and the range of the timed repetitions (host clock around work that ends in a
synchronisation; a repetition of the batched form is --inner calls, each synchronised), the ratio loop / batch, and the batched call's share of the 8 TB/s HBM peak by its byte model — every sample
read twice and each of the three outputs written once.  Before timing, the batched float64 results are compared with the loop's
bit for bit.  usage: python tools/instantaneous_batch_bench.py [--reps 7] [--loop-reps 3] [--inner 10] [--shapes 9x24,9216x16,60000x256]
(a shape is ROWSxN; an N of up to 31 is log2 of the row length)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyitd_amd  # noqa: E402

PEAK = 8.0e12


def make_rows(R, n, seed):
    """Oscillations about zero like a decomposition's rotations: a tone per row (4 to 400 samples per half wave) plus noise."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64, device="cuda")
    x = torch.empty((R, n), dtype=torch.float64, device="cuda")
    step = max(1, (1 << 24) // n)
    for r0 in range(0, R, step):
        r1 = min(R, r0 + step)
        half = 4.0 * 100.0 ** torch.rand((r1 - r0, 1), generator=g, dtype=torch.float64, device="cuda")
        phase = 6.283185307179586 * torch.rand((r1 - r0, 1), generator=g, dtype=torch.float64, device="cuda")
        x[r0:r1] = torch.sin(3.141592653589793 / half * t + phase)
        x[r0:r1] += 0.05 * torch.randn((r1 - r0, n), generator=g, dtype=torch.float64, device="cuda")
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10, help="batched calls per timed repetition")
    ap.add_argument("--shapes", default="9x24,9216x16,60000x256")
    a = ap.parse_args()
    torch.cuda.init()           # (torch's HIP runtime first, the library's behind it)
    shapes = []
    for s in a.shapes.split(","):
        r, e = s.split("x")
        shapes.append((int(r), 1 << int(e) if int(e) <= 31 else int(e)))
    for R, n in shapes:
        eng = pyitd_amd.Engine(n, 1, 0)
        x64 = make_rows(R, n, seed=R + n)
        x32 = x64.float()
        xw = x32.double()                                        # what the loop beside the float32 case reads
        out64 = [torch.empty((R, n), dtype=torch.float64, device="cuda") for _ in range(3)]
        loop_out = [torch.empty((R, n), dtype=torch.float64, device="cuda") for _ in range(3)]
        out32 = [torch.empty((R, n), dtype=torch.float32, device="cuda") for _ in range(3)]
        info = torch.empty(R, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def batch(x, outs, f32):
            eng.instantaneous_batch_dev(x.data_ptr(), np.float32 if x.dtype == torch.float32 else np.float64, n, R, n,
                                        outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), n, f32, info.data_ptr())
            eng.copy(info.data_ptr(), info.data_ptr(), 0, 2, wait=True)     # the engine's stream has run dry

        def loop(x):
            fn, h = eng._L.itd_instantaneous_f64, eng._h
            px, pa, pp, pf = x.data_ptr(), loop_out[0].data_ptr(), loop_out[1].data_ptr(), loop_out[2].data_ptr()
            for r in range(R):
                o = 8 * r * n
                rc = fn(h, px + o, n, pa + o, pp + o, pf + o, None)          # synchronises by itself
                if rc:
                    raise RuntimeError("itd_instantaneous_f64: %d" % rc)

        def clock(f):
            t0 = time.perf_counter()
            f()
            return time.perf_counter() - t0

        # warm-up of every form, and the comparison: the batched float64 results are the loop's bit for bit
        batch(x64, out64, False)
        loop(x64)
        assert int(info.min()) >= 0, "a NaN row"
        same = all(torch.equal(b.view(torch.int64), s.view(torch.int64)) for b, s in zip(out64, loop_out))
        batch(x32, out32, True)
        for _ in range(2):
            batch(x64, out64, False)
            batch(x32, out32, True)
        for name, xin, xloop, outs, f32, bpe in (("float64", x64, x64, out64, False, 8), ("float32", x32, xw, out32, True, 4)):
            tb, tl = [], []
            for k in range(a.reps):
                tb.append(clock(lambda: [batch(xin, outs, f32) for _ in range(a.inner)]) / a.inner)
                if k < a.loop_reps:
                    tl.append(clock(lambda: loop(xloop)))
            mb, ml = statistics.median(tb), statistics.median(tl)
            nbytes = R * n * (2 * bpe + 3 * bpe)
            print(json.dumps({
                "rows": R, "n": n, "dtype_in_out": name, "batch_bit_identical_to_loop_f64": bool(same),
                "batch_ms": round(mb * 1e3, 4), "batch_ms_range": [round(min(tb) * 1e3, 4), round(max(tb) * 1e3, 4)], "batch_reps": len(tb), "batch_calls_per_rep": a.inner,
                "loop_ms": round(ml * 1e3, 3), "loop_ms_range": [round(min(tl) * 1e3, 3), round(max(tl) * 1e3, 3)], "loop_reps": len(tl),
                "loop_over_batch": round(ml / mb, 2), "batch_model_bytes": nbytes, "batch_TBps": round(nbytes / mb / 1e12, 3),
                "frac_of_hbm_peak_batch": round(nbytes / mb / PEAK, 3),
                "frac_of_hbm_peak_loop": round(R * n * 40 / ml / PEAK, 3)}), flush=True)
        del x64, x32, xw, out64, loop_out, out32
        eng.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
