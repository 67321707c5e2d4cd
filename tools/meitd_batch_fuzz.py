"""MEITD_batch / XITD_batch (one launch, one workgroup per signal) against the single-signal calls on random batches built from the
six signal families of tools/meitd_fuzz.py, with the solver "auto" or "parallel" and lengths from 600 samples (below 1024, "auto"
loops over the single calls and "parallel" takes the launch): every signal's components bit for bit, the same errors (type and
ITDError status).
usage: python tools/meitd_batch_fuzz.py [batches] [seed]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyitd_amd import meitd


def family(rng, fam, n, k):
    """signal k of family fam (tools/meitd_fuzz.py's six)"""
    t = np.arange(n) / 1000.0
    if fam == 0:
        return np.sin(2 * np.pi * rng.uniform(1, 8) * t) + rng.uniform(0.05, 0.5) * rng.standard_normal(n)
    if fam == 1:
        return np.cumsum(rng.standard_normal(n))
    if fam == 2:
        return np.sin(2 * np.pi * rng.uniform(1, 5) * t) * (1 + 0.5 * np.sin(2 * np.pi * rng.uniform(0.1, 1) * t)) + 0.3 * np.sin(2 * np.pi * rng.uniform(20, 60) * t)
    if fam == 3:
        return rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7)
    if fam == 4:
        return np.round(np.sin(2 * np.pi * rng.uniform(1, 8) * t) * 50 + 5 * rng.standard_normal(n))      # plateaus, ties
    return np.exp(-((t - t.mean()) * rng.uniform(0.5, 3)) ** 2) + 1e-3 * rng.standard_normal(n) * (k % 12 == 5)


def _call(f, *a, **kw):
    try:
        return f(*a, **kw), None
    except Exception as ex:                             # (the batch must raise what the first raising single call raises)
        return None, (type(ex), getattr(ex, "status", None))


def _equal(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def run(batches, seed, log=print):
    """returns (mismatching signals or calls, signals compared)"""
    rng = np.random.default_rng(seed)
    bad = signals = 0
    for case in range(batches):
        n = int(rng.choice([600, 900, 1024, 1500, 2048, 3000, 4096, 4800, 5000, 8192]))
        solver = "parallel" if case % 3 == 1 else "auto"
        B = int(rng.integers(8, 41))
        x = np.stack([family(rng, int(rng.integers(0, 6)), n, k) for k in range(B)])
        wpemax = float(rng.uniform(0.3, 0.9))
        chunk = None if case % 2 == 0 else int(rng.integers(3, B + 1))
        with np.errstate(all="ignore"):
            got, err = _call(meitd.MEITD_batch, x, WPEMAX=wpemax, solver=solver, chunk=chunk)
            stats = dict(meitd.last_batch)
            ref, err2 = [], None
            for xi in x:
                r, err2 = _call(meitd.MEITD, xi.copy(), WPEMAX=wpemax, solver=solver)
                if err2:
                    break
                ref.append(r)
            gx, errx = _call(meitd.XITD_batch, x, solver=solver, chunk=chunk)
            rx, errx2 = [], None
            for xi in x:
                r, errx2 = _call(meitd.XITD, xi.copy(), solver=solver)
                if errx2:
                    break
                rx.append(r)
        ok = err == err2
        if ok and err is None:
            for i in range(B):
                signals += 1
                if not _equal(got[i], ref[i]):
                    bad += 1
                    log("batch %d (n %d, B %d, WPEMAX %.3f, solver %s, chunk %s): MEITD signal %d differs  %s" % (case, n, B, wpemax, solver, chunk, i, stats))
        elif not ok:
            bad += 1
            log("batch %d: MEITD errors differ: %s against %s" % (case, err, err2))
        okx = errx == errx2
        if okx and errx is None:
            for i in range(B):
                if not _equal(gx[i], rx[i]):
                    bad += 1
                    log("batch %d (n %d, B %d, solver %s, chunk %s): XITD signal %d differs" % (case, n, B, solver, chunk, i))
        elif not okx:
            bad += 1
            log("batch %d: XITD errors differ: %s against %s" % (case, errx, errx2))
    return bad, signals


if __name__ == "__main__":
    batches = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    t0 = time.time()
    bad, signals = run(batches, int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    print("%d batches, %d signals, %d mismatches, %.1f s" % (batches, signals, bad, time.time() - t0))
    sys.exit(1 if bad else 0)
