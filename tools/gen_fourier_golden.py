#!/usr/bin/env python3
"""Golden vectors for the ITD-Fourier cascade (itd_fourier_decomposition.py:131-303), computed by the reference itself.

Runs on a CPU machine that holds a checkout of the reference (--ref).  The reference is imported through
oracle.gen_golden.load_cubic_reference (plain Python under a numba stand-in), with the smallest fix for each of two upstream defects:
  * fourier_mode_decomposition_any (:171-209) says `numpy.` although the file imports numpy as `np` only: `numpy` is injected into
    the module's namespace;
  * itd_fourier_decomposition_lean (:258-303) calls the undefined `itd_fourier_wrapper` (:269, :276): it is bound to
    itd_sine_wrapper, the file's only wrapper.
The reference's progress lines are counted (the iteration count) and swallowed.  A numpy restatement of each selector records the
decisions; the generator asserts that it reproduces the reference's returned mode bit for bit, that the sum of the rows in row order
is np.sum(rows, axis=0) bit for bit, and it keeps the smallest relative decision margin of a run: the gap between winner and
runner-up of every argmax / argmin over the range's largest value, and max|mode| against 1e-8.  A cascade case whose margin is
below 1e-6 is refused (two FFTs' rounding could flip a decision).  numpy 2 computes ifft of a complex64 array in float32, numpy 1 in
complex128: the version is recorded.

Outputs are data only: tests/golden/fourier/*.npz (floats of the cascades stored as float32: the tests hold them to 1e-6 of scale).
Usage: python tools/gen_fourier_golden.py [--ref DIR] [--out tests/golden/fourier]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _gap(seg, want_max):
    if seg.shape[0] < 2:
        return np.inf
    s = np.sort(seg)
    d = (s[-1] - s[-2]) if want_max else (s[1] - s[0])
    return d / s[-1] if s[-1] > 0 else np.inf


def select(x, rule):
    """The selector restated: (rec int32[6] = status, peak_max, first_peak, last_peak, mina, minb; -1 not reached),
    xn (complex64), margin."""
    X = np.fft.fft(x)
    a = np.abs(X)
    n = a.shape[0]
    half = n // 2
    m = [np.inf]
    pm = fp = lp = mina = minb = -1
    ok = False
    if rule == "any":
        pm = int(np.argmax(a[1:half])) + 1
        m.append(_gap(a[1:half], True))
        if pm != 1 and pm != half - 1:
            fp = int(np.argmax(a[:pm]))
            lp = int(np.argmax(a[pm + 1:half])) + pm + 1
            m += [_gap(a[:pm], True), _gap(a[pm + 1:half], True)]
            ok = not (fp == pm - 1 or lp == pm + 1)
    else:
        peaks = [i for i in range(1, half - 1) if a[i] > a[i - 1] and a[i] > a[i + 1]]
        for i in range(1, half - 1):
            for j in (i - 1, i + 1):
                if max(a[i], a[j]) > 0:
                    m.append(abs(a[i] - a[j]) / max(a[i], a[j]))
        if len(peaks) >= 3:
            order = sorted(peaks, key=lambda i: a[i], reverse=True)
            pm = order[0]
            m.append(_gap(a[np.asarray(peaks)], True))
            below = [i for i in peaks if i < pm - 1]
            above = [i for i in peaks if i > pm + 1]
            if below and above:
                fp, lp = max(below), min(above)
                ok = True
    if ok:
        mina = fp + int(np.argmin(a[fp:pm + 1]))
        minb = pm + int(np.argmin(a[pm:lp + 1]))
        m += [_gap(a[fp:pm + 1], False), _gap(a[pm:lp + 1], False)]
    xn = np.zeros(n, dtype=np.complex64)
    if ok:
        xn[mina:minb] = X[mina:minb]
        xn[-minb:-mina] = X[-minb:-mina]
    return np.array([int(ok), pm, fp, lp, mina, minb], np.int32), xn, min(m)


def load_reference(ref_dir):
    from oracle.gen_golden import load_cubic_reference
    ref = load_cubic_reference(ref_dir)
    ref.numpy = np                                  # :177-209 say `numpy.`
    ref.itd_fourier_wrapper = ref.itd_sine_wrapper  # :269, :276
    return ref


def selector_cases(ref):
    rng = np.random.default_rng(2024)
    cases = []

    def tone_noise(n, seed):
        r = np.random.default_rng(seed)
        t = np.arange(n)
        f1, f2 = r.uniform(0.05, 0.2), r.uniform(0.25, 0.45)
        x = np.sin(2 * np.pi * f1 * t) + 0.6 * np.sin(2 * np.pi * f2 * t + 1.0) + 0.3 * r.standard_normal(n)
        return np.round(x * 4096) / 4096          # exact in float32 and small to store
    for n in list(range(4, 65)) + [99, 127, 255, 1001, 8191, 8192, 8193, 10007, 12000, 44100]:
        cases.append(("n%d" % n, tone_noise(n, n)))
    cases.append(("delta64", np.eye(1, 64)[0]))            # |X| = 1 everywhere: every argmax a tie, no strict maximum
    t = np.arange(256)
    cases.append(("pure_tone256", np.round(np.cos(2 * np.pi * 37 * t / 256) * 4096) / 4096))
    cases.append(("edge_peak_any", np.round(np.cos(2 * np.pi * 1 * np.arange(40) / 40) * 4096) / 4096))
    cases.append(("dc_heavy100", np.round((5 + np.sin(2 * np.pi * 0.1 * np.arange(100)) + 0.2 * rng.standard_normal(100)) * 4096) / 4096))
    # exact ties: a zero-mean integer pattern repeated four times has a spectrum that is exactly zero off the multiples of 4 (both
    # numpy's FFT and a decimation of the first radix-4 stage give exact zeros), so a[0..3] tie at 0: first_peak = argmax(a[:4]) = 0,
    # mina = argmin(a[0:5]) = 0 (the second slice xn[-minb:-0] is empty) and minb = 4 + argmin over a run of zeros -- argmax and
    # argmin ties inside accepted selections, decided by the first index
    ties = []
    for n in (36, 60, 100, 140):
        r = np.random.default_rng(n)
        P = n // 4
        for _ in range(2000):
            pat = np.round(12 * np.cos(2 * np.pi * np.arange(P) / P) + r.integers(-3, 4, P))
            pat[-1] -= pat.sum()
            x = np.tile(pat, 4)
            rec, _, _ = select(x, "any")
            if rec[0] == 1 and rec[4] == 0:
                ties.append(("tie_mina0_n%d" % n, x))
                break
    assert len(ties) >= 3, "no exact-tie case with mina == 0 found"
    cases += ties
    out = []
    for name, x in cases:
        for rule, fn in (("any", ref.fourier_mode_decomposition_any), ("valid", ref.fourier_mode_decomposition_valid)):
            mode_ref = np.asarray(fn(x.copy()))
            rec, xn, margin = select(x, rule)
            mine = np.fft.ifft(xn).real
            assert np.array_equal(mine, mode_ref) and (not rec[0] or mine.dtype == mode_ref.dtype), (name, rule)
            exact_tie = name == "delta64" or name.startswith("tie_")
            if margin < 1e-6 and not exact_tie:
                continue
            out.append((name, rule, x, rec, mode_ref, margin))
    return out


class _Stop(Exception):
    pass


def run_cascade(ref, fn_name, x, sr, limit):
    """One cascade of the reference, instrumented: (outputs, iterations, records int32[m, 7], margin)."""
    state = {"iters": 0, "calls": 0, "records": [], "margin": np.inf}
    orig = ref.fourier_mode_decomposition_any
    K = np.arange(2, sr // 2 - 1, 96).size - 1

    def selector(rotation):
        mode = orig(rotation)
        rec, xn, margin = select(rotation, "any")
        mine = np.fft.ifft(xn).real
        assert np.array_equal(mine, mode)
        c = state["calls"]
        state["calls"] += 1
        mx = float(np.max(np.abs(mode)))
        state["margin"] = min(state["margin"], margin, abs(mx - 1e-8) / 1e-8)
        if not np.allclose(mode, 0):
            state["records"].append([c // K + 1, c % K] + list(rec[1:]))
        return mode

    def printer(*a, **k):
        if a and str(a[0]).startswith("Iteration"):
            state["iters"] += 1
            if state["iters"] > limit:
                raise _Stop()
    real_sum = np.sum

    def checked_sum(a, axis=None, **kw):
        r = real_sum(a, axis=axis, **kw)
        if axis == 0 and isinstance(a, list):
            acc = a[0].copy()
            for row in a[1:]:
                acc = acc + row
            assert np.array_equal(acc, r), "the row-order sum is not np.sum(rows, axis=0)"
        return r
    ref.fourier_mode_decomposition_any = selector
    ref.print = printer
    ref.np.sum = checked_sum
    try:
        out = getattr(ref, fn_name)(x.copy(), sr)
    finally:
        ref.fourier_mode_decomposition_any = orig
        ref.np.sum = real_sum
        del ref.print
    recs = np.asarray(state["records"], np.int32).reshape(-1, 7)
    return [np.asarray(o, np.float64) for o in out], state["iters"], recs, state["margin"]


def cascade_cases(out_dir):
    cases = []
    radio = np.load(os.path.join(ROOT, "tests", "golden", "radio8000_input.npz"))["x"].astype(np.float64)
    cases.append(("radio8000_sr842", radio, 842))
    # (n, sample_rate) pairs for which no band's extrapolated last knot lies beyond the signal (the reference raises there)
    rng = np.random.default_rng(7)
    for sr in (400, 421, 842):
        t = np.arange(8000) / sr
        cases.append(("two_tone_noise8000_sr%d" % sr, np.sin(2 * np.pi * 41 * t) + 0.5 * np.sin(2 * np.pi * 133 * t) + 0.2 * rng.standard_normal(t.size), sr))
    t = np.arange(2000) / 421.0
    cases.append(("am2000_sr421", (1 + 0.6 * np.sin(2 * np.pi * 3 * t)) * np.sin(2 * np.pi * 90 * t), 421))
    for sr in (450, 439, 507):
        t = np.arange(9000) / sr
        cases.append(("long9000_sr%d" % sr, np.sin(2 * np.pi * 31 * t) + 0.4 * np.sin(2 * np.pi * 170 * t) + 0.1 * np.random.default_rng(9).standard_normal(t.size), sr))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("PYITD_REFERENCE", "reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fourier"))
    ap.add_argument("--limit", type=int, default=40, help="refuse a cascade case that runs more iterations")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    ref = load_reference(args.ref)
    ver = np.array(np.__version__)
    sel = selector_cases(ref)
    # one file per group of cases: signals and modes back to back (float32: exact for the signals, the modes are float32 under
    # numpy 2), offs [m + 1] where each starts
    groups = {}
    for c in sel:
        groups.setdefault("small" if c[2].shape[0] <= 1001 else c[0], []).append(c)
    for g, cs in groups.items():
        offs = np.cumsum([0] + [c[2].shape[0] for c in cs])
        np.savez_compressed(os.path.join(args.out, "selectors_%s.npz" % g), names=np.array([c[0] for c in cs]),
                            rules=np.array([c[1] for c in cs]), offs=offs, x=np.concatenate([c[2] for c in cs]).astype(np.float32),
                            recs=np.stack([c[3] for c in cs]), modes=np.concatenate([c[4] for c in cs]).astype(np.float32),
                            margins=np.array([c[5] for c in cs]), numpy_version=ver)
    print("selector cases:", len(sel), "files:", len(groups))
    kept = set()
    for name, x, sr in cascade_cases(args.out):
        try:
            full, it_full, recs, m1 = run_cascade(ref, "itd_fourier_decomposition", x, sr, args.limit)
            lean, it_lean, recs_lean, m2 = run_cascade(ref, "itd_fourier_decomposition_lean", x, sr, args.limit)
        except (IndexError, _Stop) as ex:
            print("refused", name, type(ex).__name__)
            continue
        margin = min(m1, m2)
        if margin < 1e-6:
            print("refused", name, "margin", margin)
            continue
        assert it_full == it_lean and np.array_equal(recs, recs_lean)
        if not len(recs) or any(k.startswith(name.split("_sr")[0]) for k in kept):
            print("skipped", name, "modes", len(recs))
            continue
        kept.add(name)
        # the lean output is the non-lean rows with each row's modes summed in the order found: stored once
        K = len(lean) // 2
        rows_full, j = [], 0
        for i in range(K):
            m = recs[recs[:, 1] == i]
            accm = np.zeros_like(x)
            for _ in range(len(m)):
                accm = accm + full[j]
                j += 1
            rows_full.append(full[j])
            j += 1
            assert np.array_equal(rows_full[-1], lean[2 * i + 1]) and np.allclose(accm, lean[2 * i], rtol=0, atol=1e-12)
        np.savez_compressed(os.path.join(args.out, "cascade_%s.npz" % name), x=x, sample_rate=np.array(sr),
                            full=np.stack(full).astype(np.float32),
                            iterations=np.array(it_full), records=recs, margin=np.array(margin), numpy_version=ver)
        print("cascade", name, "iterations", it_full, "modes", len(recs), "margin %.3g" % margin)


if __name__ == "__main__":
    main()
