"""MEITD_batch / XITD_batch (pyitd_amd/meitd.py; itd_meitd_batch_f64, csrc/itd_meitd.hpp: k_meitd_batch): many short signals, one
workgroup per signal, one launch.  The contract is [MEITD(x) for x in data] / [XITD(x) for x in data] bit for bit — the same
components, the same errors — and the reference's goldens to the existing tolerance."""
import importlib.util
import os

import numpy as np
import pytest

from helpers import GOLDEN

pytestmark = pytest.mark.gpu
SPLINE = os.path.join(GOLDEN, "spline")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(f[:-4] for f in os.listdir(SPLINE) if f.startswith("meitd_"))


@pytest.fixture(scope="module")
def meitd():
    from pyitd_amd import meitd
    return meitd


def _close(got, ref, what, tol=1e-10):
    assert got.shape == ref.shape, what
    scale = max(1.0, float(np.max(np.abs(ref))))
    assert float(np.max(np.abs(got - ref))) <= tol * scale, what


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(a, b), what


def _same_meitd(got, ref, what):
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        for a, b, part in zip(g, r, ("high", "low", "residual")):
            _same(a, b, "%s: signal %d %s" % (what, i, part))


def _signals(n, count, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 1000.0
    out = np.empty((count, n))
    for i in range(count):
        out[i] = (np.sin(2 * np.pi * rng.uniform(1, 6) * t) * (1.0 + 0.5 * np.sin(2 * np.pi * rng.uniform(0.1, 1) * t))
                  + 0.3 * np.sin(2 * np.pi * rng.uniform(20, 60) * t + 1.0) + rng.uniform(0.02, 0.3) * rng.standard_normal(n))
    return out


def test_goldens_in_one_batch_and_inside_a_larger_one(meitd):
    g = [np.load(os.path.join(SPLINE, name + ".npz")) for name in NAMES]
    x = np.stack([gi["x"] for gi in g])
    assert x.shape[1] == 3000
    single = [meitd.MEITD(xi.copy()) for xi in x]
    single_x = [meitd.XITD(xi.copy()) for xi in x]
    got = meitd.MEITD_batch(x)
    got_x = meitd.XITD_batch(x)
    assert meitd.last_batch["launches"] == 1 and meitd.last_batch["handed_back"] == 0, meitd.last_batch
    for i, name in enumerate(NAMES):
        hi, lo, res = got[i]
        assert hi.shape == g[i]["high"].shape and lo.shape == g[i]["low"].shape, name
        if hi.size:
            _close(hi, g[i]["high"], name + " high")
        if lo.size:
            _close(lo, g[i]["low"], name + " low")
        _close(res, g[i]["residual"], name + " residual")
        _close(got_x[i], g[i]["xitd"], name + " XITD")
        _same(got_x[i], single_x[i], name + " XITD against the single call")
    _same_meitd(got, single, "goldens")
    # the three goldens repeated, at scattered places of a 64-signal batch
    big = _signals(3000, 64, 3)
    at = [0, 17, 63]
    big[at] = x
    got = meitd.MEITD_batch(big)
    got_x = meitd.XITD_batch(big)
    for k, i in enumerate(at):
        _same_meitd([got[i]], [single[k]], "golden %s at %d" % (NAMES[k], i))
        _same(got_x[i], single_x[k], "golden %s XITD at %d" % (NAMES[k], i))


@pytest.mark.parametrize("n, count, seed", [(1024, 48, 1), (3000, 64, 2), (4800, 32, 3), (5000, 32, 4), (8192, 32, 5)])
def test_random_batches_equal_the_single_calls(meitd, n, count, seed):
    """4800: the last length whose solver arrays fit LDS; 5000 and 8192: the global-memory form"""
    x = _signals(n, count, seed)
    got = meitd.MEITD_batch(x, WPEMAX=0.55)
    stats = dict(meitd.last_batch)
    words = []
    for i in range(count):
        ref = meitd.MEITD(x[i].copy(), WPEMAX=0.55)
        _same_meitd([got[i]], [ref], "n %d" % n)
        words.append(dict(meitd._work_for(n, 0).last))
    assert stats["launches"] == 1 and stats["looped"] == 0
    # the result words: the single calls' extractions and probes, signal by signal
    eng = meitd._eng(n, 0)
    per = 50 * n
    from pyitd_amd.engine import DeviceBuffer
    buf = DeviceBuffer(count * per * 8)
    try:
        res, _, _, _ = eng.meitd_batch_dev(buf.ptr, n, count, per, 0.55, x=x)
    finally:
        buf.free()
    for i, w in enumerate(words):
        if w.get("status") == 0:
            assert res[i, 0] == 0 and res[i, 5] == w["extractions"] and res[i, 4] == w["probes"] and res[i, 6] == w["turns"], (i, w)
    got_x = meitd.XITD_batch(x)
    for i in range(0, count, 4):
        _same(got_x[i], meitd.XITD(x[i].copy()), "XITD n %d signal %d" % (n, i))


def test_a_mixed_batch(meitd):
    from pyitd_amd._lib import ITDError
    x = _signals(2000, 8, 7)
    x[3] = np.linspace(-1.0, 2.0, 2000)                       # fewer than 4 extrema
    nan = x.copy()
    nan[5, 777] = np.nan
    with pytest.raises(ITDError) as ei:
        meitd.MEITD_batch(nan)
    with pytest.raises(ITDError) as ej:
        meitd.MEITD(nan[5].copy())
    assert ei.value.status == ej.value.status
    with pytest.raises(ITDError) as ek:
        meitd.XITD_batch(nan)
    assert ek.value.status == ej.value.status
    got = meitd.MEITD_batch(x)
    assert meitd.last_batch["status"].get(1) == 1, meitd.last_batch
    hi, lo, res = got[3]
    assert not hi.any() and not lo.any() and np.array_equal(res, x[3])
    _same_meitd(got, [meitd.MEITD(xi.copy()) for xi in x], "mixed")
    got_x = meitd.XITD_batch(x)
    for i in range(len(x)):
        _same(got_x[i], meitd.XITD(x[i].copy()), "mixed XITD %d" % i)


def test_chunks_do_not_change_the_results(meitd):
    x = _signals(3000, 23, 9)
    a = meitd.MEITD_batch(x, chunk=5)
    assert meitd.last_batch["launches"] == 5 and meitd.last_batch["chunks"] == 5
    b = meitd.MEITD_batch(x)
    assert meitd.last_batch["launches"] == 1
    _same_meitd(a, b, "chunk 5 against the default")
    xa, xb = meitd.XITD_batch(x, chunk=5), meitd.XITD_batch(x)
    for i in range(len(x)):
        _same(xa[i], xb[i], "XITD chunk 5, signal %d" % i)
    one = meitd.MEITD_batch(x[:1])
    _same_meitd(one, [meitd.MEITD(x[0].copy())], "a batch of one")
    _same(meitd.XITD_batch(x[:1])[0], meitd.XITD(x[0].copy()), "XITD of a batch of one")


def test_one_launch_and_no_host_driven_operator_for_delivered_signals(meitd, monkeypatch):
    calls = {"extract": 0, "probe": 0}
    for k in calls:
        orig = getattr(meitd._Work, k)
        monkeypatch.setattr(meitd._Work, k, (lambda o, kk: lambda self, *a, **kw: (calls.__setitem__(kk, calls[kk] + 1), o(self, *a, **kw))[1])(orig, k))
    x = _signals(3000, 64, 11)
    meitd.MEITD_batch(x)
    st = meitd.last_batch
    assert st["launches"] == 1 and st["chunks"] == 1 and st["looped"] == 0, st
    assert st["status"].get(0, 0) + st["status"].get(1, 0) == 64 and st["handed_back"] == 0, st
    assert calls == {"extract": 0, "probe": 0}, calls
    meitd.XITD_batch(x)
    assert meitd.last_batch["launches"] == 1 and meitd.last_batch["handed_back"] == 0
    assert calls == {"extract": 0, "probe": 0}, calls


@pytest.mark.parametrize("n, solver", [(600, "auto"), (9000, "auto"), (2000, "serial")])
def test_ineligible_lengths_loop_over_the_single_path(meitd, n, solver):
    x = _signals(n, 3, 13)
    got = meitd.MEITD_batch(x, solver=solver)
    assert meitd.last_batch["looped"] == 3 and meitd.last_batch["launches"] == 0
    _same_meitd(got, [meitd.MEITD(xi.copy(), solver=solver) for xi in x], "n %d" % n)
    got_x = meitd.XITD_batch(x, solver=solver)
    _same(got_x[0], meitd.XITD(x[0].copy(), solver=solver), "XITD n %d" % n)


def test_parallel_solver_below_1024_over_several_chunks(meitd):
    """solver="parallel" takes the launch below 1024 samples too.  A signal with fewer than 4 extrema in an early chunk sends XITD
    through the single-signal entropy, which sets the shared engine's solver to "auto": every later chunk must still launch under
    "parallel" (itd_meitd_batch_f64 refuses "auto" below 1024 samples), and the results stay the single calls'."""
    from pyitd_amd import spline
    x = _signals(600, 6, 17)
    x[0] = np.linspace(-1.0, 2.0, 600)                          # fewer than 4 extrema: status 1
    got_x = meitd.XITD_batch(x, solver="parallel", chunk=2)
    st = meitd.last_batch
    assert st["chunks"] == 3 and st["launches"] == 3 and st["looped"] == 0 and st["status"].get(1) == 1, st
    for i in range(len(x)):
        _same(got_x[i], meitd.XITD(x[i].copy(), solver="parallel"), "XITD parallel 600, signal %d" % i)
    spline._eng(600, 0)                                         # (another call leaves the engine at "auto")
    got = meitd.MEITD_batch(x, solver="parallel", chunk=2)
    assert meitd.last_batch["launches"] == 3 and meitd.last_batch["looped"] == 0
    _same_meitd(got, [meitd.MEITD(xi.copy(), solver="parallel") for xi in x], "MEITD parallel 600")


def test_batch_fuzz_slice(meitd):
    spec = importlib.util.spec_from_file_location("meitd_batch_fuzz", os.path.join(ROOT, "tools", "meitd_batch_fuzz.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    bad, signals = mod.run(4, 3, log=lines.append)
    assert signals > 0 and bad == 0, "\n".join(lines)
