"""The engine's FFT against the long-double reference of tests/fft_cases.py over every listed length, input family and direction:
the worst measured ratio err / max(yard_fft, yard_seq) per tier and direction (rows whose yardstick is exactly 0 apart, by their
error in units), beside the bound's factor K = 4 — the open form of tests/test_gpu_fft_exact.py::test_fft_accuracy.
usage: python tools/fft_accuracy.py [--rows]     (--rows: one line per row as well)"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import fft_cases as fc
from pyitd_amd.fourier import debug_fft

if not fc.LONGDOUBLE_OK:
    sys.exit(fc.LONGDOUBLE_WHY)
per_row = "--rows" in sys.argv[1:]
worst = {}          # (tier, path, direction, kind of row) -> (ratio, n, family, err, yard)
zero_yard = {}      # (tier, path, direction) -> (err in units, n, family)
over = 0
for n in fc.LENGTHS:
    tier, path = fc.path_of(n)
    names, x, by_dir = fc.length_case(n)
    for inverse in (False, True):
        ref, u, y_fft, y_seq, idx = by_dir[inverse]
        err = fc.err_units(debug_fft(x, inverse), ref, u)
        yard = y_fft if y_seq is None else np.maximum(y_fft, y_seq)
        limit = fc.bound(y_fft, y_seq)
        d = "inverse" if inverse else "forward"
        for b, name in enumerate(names):
            over += int(not err[b] <= limit[b])
            if per_row:
                print("n %7d tier %d %-9s %s %-12s err %9.2f yard_fft %9.2f yard_seq %9s bound %9.2f%s" % (
                    n, tier, path, d, name, err[b], y_fft[b], "-" if y_seq is None else "%.2f" % y_seq[b], limit[b],
                    "" if err[b] <= limit[b] else "  EXCEEDS"))
            if yard[b] == 0:
                if err[b] >= zero_yard.get((tier, path, d), (-1,))[0]:
                    zero_yard[(tier, path, d)] = (err[b], n, name)
                continue
            key = (tier, path, d, "random" if fc.is_random(name) else "structured")
            if err[b] / yard[b] >= worst.get(key, (-1,))[0]:
                worst[key] = (err[b] / yard[b], n, name, err[b], yard[b])
print("worst err / max(yard_fft, yard_seq) per tier, path, direction and kind of row (bound: %g x yard + %g units)" % (fc.K, fc.F))
for key in sorted(worst):
    r, n, name, e, y = worst[key]
    print("tier %d %-9s %s %-10s ratio %5.2f  (n %d %s: err %.2f units, yard %.2f)" % (key + (r, n, name, e, y)))
print("rows whose yardstick is exactly 0: the largest error in units (bound: %g)" % fc.F)
for key in sorted(zero_yard):
    e, n, name = zero_yard[key]
    print("tier %d %-9s %s err %.2f  (n %d %s)" % (key + (e, n, name)))
print("rows over the bound: %d" % over)
