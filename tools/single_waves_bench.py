"""Single-wave analysis (pyitd_amd.wave_filter, pyitd_amd.single_waves) against what a caller could do without it: the amplitude of
every sample's half wave from pyitd_amd.instantaneous_batch(want="amplitude"), the half waves' lengths by a torch composition
(crossing flags, cumsum, bincount, gather) and the mask — over the same device-resident float64 rows in the same process, the two
alternating.  Shapes: 9 x 2^24 and 9216 x 2^16.  Every row has its own bounds.  Also timed on the same rows: single_waves with
the capacity given, and instantaneous_batch with all three outputs (the filter moves 24 B per sample where that call moves 40 and
evaluates no arcsine: is it no slower?).

One JSON line per shape: the median and the range of the timed repetitions (host clock around the public call on CUDA tensors,
which ends in a synchronisation; output allocation included on both sides), the ratio composition / filter, and the filter's share
of the 8 TB/s HBM peak by its byte model — every sample read twice and written once.  Before timing, the filter's result is
compared with the composition's bit for bit.
usage: python tools/single_waves_bench.py [--reps 7] [--shapes 9x24,9216x16]   (a shape is ROWSxN; an N of up to 31 is log2 of the
row length)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pyitd_amd  # noqa: E402
from instantaneous_batch_bench import PEAK, make_rows  # noqa: E402


def composition(x, b):
    """The filter from what exists without it.  x[R, n] float64, b[R, 4] float64 (amp_lo, amp_hi, len_lo, len_hi), on the GPU."""
    R, n = x.shape
    (amp,) = pyitd_amd.instantaneous_batch(x, want="amplitude")
    mid, nxt = x[:, 1:-1], x[:, 2:]
    cross = ((mid > 0) & (nxt < 0)) | ((mid < 0) & (nxt > 0))       # crossing indices 1 .. n-2
    hw = torch.zeros((R, n), dtype=torch.int64, device=x.device)    # the half wave of every sample, numbered along the row
    hw[:, 2:] = torch.cumsum(cross, dim=1)
    hw += (torch.arange(R, device=x.device, dtype=torch.int64) * n)[:, None]
    length = torch.bincount(hw.reshape(-1), minlength=R * n)[hw].to(torch.float64)
    keep = (b[:, 0:1] <= amp) & (amp <= b[:, 1:2]) & (b[:, 2:3] <= length) & (length <= b[:, 3:4])
    out = torch.where(keep, x, torch.zeros((), dtype=x.dtype, device=x.device))
    torch.cuda.synchronize()
    return out


def clock(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(ts):
    return round(statistics.median(ts) * 1e3, 4), [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="9x24,9216x16")
    a = ap.parse_args()
    torch.cuda.init()           # (torch's HIP runtime first, the library's behind it)
    for s in a.shapes.split(","):
        r, e = s.split("x")
        R, n = int(r), (1 << int(e) if int(e) <= 31 else int(e))
        x = make_rows(R, n, seed=R + n)
        g = torch.Generator(device="cuda").manual_seed(R)
        u = torch.rand((R, 2), generator=g, dtype=torch.float64, device="cuda")
        amp = (0.3 + 0.5 * u[:, 0:1], torch.full((R, 1), float("inf"), dtype=torch.float64, device="cuda"))
        ln = (2.0 + torch.floor(6.0 * u[:, 1:2]), torch.full((R, 1), 500.0, dtype=torch.float64, device="cuda"))
        b = torch.cat((amp[0], amp[1], ln[0], ln[1]), dim=1).contiguous()
        bh = b.cpu().numpy()
        kw = dict(amplitude=(bh[:, 0], bh[:, 1]), length=(bh[:, 2], bh[:, 3]))
        # warm-up of every form, and the comparison
        got = pyitd_amd.wave_filter(x, **kw)
        want = composition(x, b)
        same = bool(torch.equal(got.view(torch.int64), want.view(torch.int64)))
        kept = float((got != 0).double().mean())
        del got, want
        cap = int(pyitd_amd.single_waves(x).count.max())
        pyitd_amd.single_waves(x, cap=cap)
        pyitd_amd.instantaneous_batch(x)
        torch.cuda.empty_cache()
        tf, tc, tw, ti = [], [], [], []
        for _ in range(a.reps):
            tc.append(clock(lambda: composition(x, b)))
            tf.append(clock(lambda: pyitd_amd.wave_filter(x, **kw)))
            ti.append(clock(lambda: pyitd_amd.instantaneous_batch(x)))
            tw.append(clock(lambda: pyitd_amd.single_waves(x, cap=cap)))
        (mf, rf), (mc, rc), (mw, rw), (mi, ri) = stats(tf), stats(tc), stats(tw), stats(ti)
        nbytes = R * n * 24
        print(json.dumps({
            "rows": R, "n": n, "dtype_in_out": "float64", "filter_bit_identical_to_composition": same, "samples_kept": round(kept, 4),
            "half_waves_per_row_max": cap, "reps": a.reps,
            "wave_filter_ms": mf, "wave_filter_ms_range": rf, "composition_ms": mc, "composition_ms_range": rc,
            "composition_over_filter": round(mc / mf, 2),
            "single_waves_ms": mw, "single_waves_ms_range": rw,
            "instantaneous_batch_all_ms": mi, "instantaneous_batch_all_ms_range": ri,
            "filter_no_slower_than_instantaneous_all": bool(mf <= mi),
            "filter_model_bytes": nbytes, "filter_TBps": round(nbytes / (mf * 1e-3) / 1e12, 3),
            "filter_frac_of_hbm_peak": round(nbytes / (mf * 1e-3) / PEAK, 3)}), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
