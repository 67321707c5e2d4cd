"""MEITD_batch (one launch, one workgroup per signal: itd_meitd_batch_f64) against the loop of single MEITD calls over the same
signals, B in {1, 16, 64, 256, 1024} x N in {3000, 4800, 8192}: wall time of each (batch: best of 3; loop: one pass) and every
signal's components compared bit for bit.  Both sides are timed the same way: best of 3 passes for B <= 64, one pass above,
each after a warm-up of both at that N.  usage: python tools/meitd_batch_bench.py [B,B,...] [N,N,...]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyitd_amd import meitd


def signals(n, count, seed):
    """two tones with an envelope and noise, as the golden meitd_two_tone_noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 1000.0
    f1, f2, fe = rng.uniform(1, 6, count), rng.uniform(20, 60, count), rng.uniform(0.1, 1, count)
    amp = rng.uniform(0.02, 0.3, count)
    return (np.sin(2 * np.pi * f1[:, None] * t) * (1.0 + 0.5 * np.sin(2 * np.pi * fe[:, None] * t))
            + 0.3 * np.sin(2 * np.pi * f2[:, None] * t + 1.0) + amp[:, None] * rng.standard_normal((count, n)))


def same(a, b):
    return all(p.shape == q.shape and np.array_equal(p, q) for p, q in zip(a, b))


def main():
    Bs = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [1, 16, 64, 256, 1024]
    Ns = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [3000, 4800, 8192]
    print("MEITD_batch against the loop of single MEITD calls (WPEMAX 0.6; both sides: best of 3 passes for B <= 64, one pass above)")
    print("%6s %6s %12s %12s %12s %9s %9s %s" % ("B", "N", "batch_ms", "loop_ms", "single_ms", "speedup", "mismatch", "status / handed back"))
    for n in Ns:
        x = signals(n, max(Bs), n)
        meitd.MEITD_batch(x[:2])                    # warm-up of both sides: library, engine, workspaces, kernel attributes
        for xi in x[:3]:
            meitd.MEITD(xi.copy())
        for B in Bs:
            xb = x[:B]
            reps = 3 if B <= 64 else 1
            t_batch = t_loop = 1e9
            for _ in range(reps):
                t0 = time.perf_counter(); got = meitd.MEITD_batch(xb); t_batch = min(t_batch, time.perf_counter() - t0)
            st = dict(meitd.last_batch)
            for _ in range(reps):
                t0 = time.perf_counter(); ref = [meitd.MEITD(xi.copy()) for xi in xb]; t_loop = min(t_loop, time.perf_counter() - t0)
            bad = sum(0 if same(g, r) else 1 for g, r in zip(got, ref))
            print("%6d %6d %12.2f %12.2f %12.3f %9.1f %9d %s / %d" % (B, n, t_batch * 1e3, t_loop * 1e3, t_loop * 1e3 / B, t_loop / t_batch, bad,
                                                                     st["status"], st["handed_back"]), flush=True)
    n, B = Ns[0], min(256, max(Bs))
    x = signals(n, B, 7)
    meitd.XITD_batch(x[:2])
    meitd.XITD(x[0].copy())
    t0 = time.perf_counter(); got = meitd.XITD_batch(x); t_batch = time.perf_counter() - t0
    t0 = time.perf_counter(); ref = [meitd.XITD(xi.copy()) for xi in x]; t_loop = time.perf_counter() - t0
    bad = sum(0 if g.shape == r.shape and np.array_equal(g, r) else 1 for g, r in zip(got, ref))
    print("XITD_batch %d x %d (one pass each): %.2f ms, loop of XITD %.2f ms (%.1fx), mismatches %d" % (B, n, t_batch * 1e3, t_loop * 1e3, t_loop / t_batch, bad))


if __name__ == "__main__":
    main()
