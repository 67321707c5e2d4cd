#!/usr/bin/env python3
"""Timing of the ITD-Fourier cascade on one GPU -> profiles/r07/fourier_cascade.txt.

  * the radio case (tests/golden/radio8000_input.npz at 842 Hz: a rate for which no band's last knot lies beyond the signal):
    ms per whole cascade and per round, non-lean and lean, host arrays in and out
  * the same for a batch of 256 such signals in one call (each a copy with its own small noise)
  * the same cascade as a composition of today's calls: pyitd_amd.itd_sine_wrapper (two engine round trips per band) plus the
    selector, the mode test and the sum in numpy on the host, the loop of itd_fourier_decomposition.py:212-255
  * the FFT alone (itd_debug_fft_f64 on device buffers, synchronous): n = 8000, 8192 and 2^20 (four-step)
Every figure is the median of several timed runs after one untimed run.
Usage: python tools/fourier_timing.py [--out profiles/r07/fourier_cascade.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts)


def host_selector_any(rotation):
    X = np.fft.fft(rotation)
    a = np.abs(X)
    half = len(a) // 2
    xn = np.zeros(len(a), dtype=np.complex64)
    pm = np.argmax(a[1:half]) + 1
    if pm == 1 or pm == half - 1:
        return np.zeros(rotation.size)
    fp = np.argmax(a[:pm])
    lp = np.argmax(a[pm + 1:half]) + pm + 1
    if fp == pm - 1 or lp == pm + 1:
        return np.zeros(rotation.size)
    mina = fp + np.argmin(a[fp:pm + 1])
    minb = pm + np.argmin(a[pm:lp + 1])
    xn[mina:minb] = X[mina:minb]
    xn[-minb:-mina] = X[-minb:-mina]
    return np.fft.ifft(xn).real


def composed_cascade(x, sr):
    import pyitd_amd
    current, rounds = x.copy(), 0
    while True:
        rotations = pyitd_amd.itd_sine_wrapper(current, sr)
        found = False
        for i, rot in enumerate(rotations[:-1]):
            mode = host_selector_any(rot)
            if not np.allclose(mode, 0):
                found = True
                rotations[i] = rot - mode
        if not found:
            return rounds
        current = np.sum(rotations, axis=0)
        rounds += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "fourier_cascade.txt"))
    args = ap.parse_args()
    import pyitd_amd
    from pyitd_amd.engine import DeviceBuffer
    from pyitd_amd.fourier import _engine_for
    lines = ["# tools/fourier_timing.py on one MI355X; medians, ms (wall clock, host arrays in and out unless stated)"]
    x = np.load(os.path.join(ROOT, "tests", "golden", "radio8000_input.npz"))["x"].astype(np.float64)
    sr = 842
    _, info = pyitd_amd.itd_fourier_decomposition(x, sr, return_info=True)
    rounds = info["rounds"] + 1          # the rounds run: the last one finds no mode
    for lean, name in ((False, "itd_fourier_decomposition"), (True, "itd_fourier_decomposition_lean")):
        fn = pyitd_amd.itd_fourier_decomposition_lean if lean else pyitd_amd.itd_fourier_decomposition
        ms = med(lambda: fn(x, sr), 7)
        lines.append("radio8000 @ %d Hz, %s: %.3f ms per cascade, %d rounds run (%d with modes): %.3f ms per round"
                     % (sr, name, ms, rounds, info["rounds"], ms / rounds))
    rng = np.random.default_rng(3)
    xs = x[None, :] + 1e-3 * np.std(x) * rng.standard_normal((256, x.shape[0]))
    outs, infos = pyitd_amd.itd_fourier_decomposition_batch(xs, sr, return_info=True)
    max_rounds = max(i["rounds"] for i in infos) + 1
    ms = med(lambda: pyitd_amd.itd_fourier_decomposition_batch(xs, sr), 3)
    lines.append("256 x radio8000 (own noise each) @ %d Hz, one batch call: %.3f ms per call, %.3f ms per signal; rounds run %d..%d: "
                 "%.3f ms per round of the longest" % (sr, ms, ms / 256, min(i["rounds"] for i in infos) + 1, max_rounds, ms / max_rounds))
    t0 = time.perf_counter()
    r = composed_cascade(x, sr)
    ms = 1e3 * (time.perf_counter() - t0)
    lines.append("radio8000 @ %d Hz as today's composition (pyitd_amd.itd_sine_wrapper + numpy selection on the host): %.3f ms per "
                 "cascade, %d rounds run: %.3f ms per round (one run)" % (sr, ms, r + 1, ms / (r + 1)))
    for n, batch in ((8000, 1), (8000, 256), (8192, 1), (8192, 256), (1 << 20, 1), (1 << 20, 8)):
        eng = _engine_for(n)
        z = (rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n))).astype(np.complex128)
        buf = DeviceBuffer(2 * z.nbytes)
        buf.upload(z)
        call = lambda: eng._check(eng._L.itd_debug_fft_f64(eng._h, ctypes.c_void_p(buf.ptr), ctypes.c_void_p(buf.ptr + z.nbytes), n, batch, 0))
        ms = med(call, 20)
        buf.free()
        form = "four-step %d x %d" % (1024, 1024) if n == 1 << 20 else "one workgroup in LDS"
        lines.append("FFT n = %d (%s), batch %d, device buffers, synchronous call: %.4f ms per call, %.4f ms per transform"
                     % (n, form, batch, ms, ms / batch))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
