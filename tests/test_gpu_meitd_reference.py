"""MEITD / XITD and their helpers on the GPU — the host-driven loop, the one-launch kernel (k_meitd_small), the batch kernel
(k_meitd_batch) under every solver — against the REFERENCE's own outputs on tests/golden/meitd/: cases chosen so that together they
take every branch of MEITD.py:344-534 (the dig loop, the three early exits, thresholds other than 0.6), each decided by the reference
with room to spare (oracle/gen_golden.py: make_meitd_branch_cases; tests/test_meitd_reference_cpu.py holds the port's control flow to
them bit for bit on the CPU).  Decisions — the numbers of high and low rows, the order of XITD's rows, `proper` — are exact; values lie
within the goldens' tolerance, 1e-10 max(1, max|ref|).  An eligible case the kernel hands back to the host fails: the fallback would
be what was compared.  The largest error of every form is printed (pytest -s) as a RATIO line: err / (1e-10 scale).

Also here: itd_gather_rows_f64 (k_gather_rows), through which MEITD_batch collects its components, against numpy's fancy indexing."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, DevArrays

pytestmark = pytest.mark.gpu
MEITD = os.path.join(GOLDEN, "meitd")
NAMES = [str(s) for s in np.load(os.path.join(MEITD, "index.npz"))["names"]]
CASES = {name: dict(np.load(os.path.join(MEITD, name + ".npz"))) for name in NAMES}
TOL = 1e-10
WORST = {}


@pytest.fixture(scope="module")
def meitd():
    from pyitd_amd import meitd
    yield meitd
    for form in sorted(WORST):
        print("RATIO %-44s gpu %9.3g  (1e-10 S)" % ("meitd reference/" + form, WORST[form]))


def _close(got, ref, what, form):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, "%s: shape %s, the reference's %s" % (what, got.shape, ref.shape)
    if not ref.size:
        return
    scale = max(1.0, float(np.max(np.abs(ref))))
    err = float(np.max(np.abs(got - ref)))
    print("RATIO %-44s gpu %9.3g  (1e-10 S)" % (form + "/" + what, err / (TOL * scale)))
    WORST[form] = max(WORST.get(form, 0.0), err / (TOL * scale))
    assert err <= TOL * scale, "%s: %.3g beyond %.3g" % (what, err, TOL * scale)


def _early(g):
    return g["high"].ndim == 1              # MEITD.py:414: zeros, zeros, the signal


def _check(got, g, name, form):
    for a, part in zip(got, ("high", "low", "residual")):
        _close(a, g[part], "%s %s" % (name, part), form)


def _xitd_ref(g):
    return np.vstack((np.vstack((g["high"], g["low"])), g["residual"]))[g["xitd_order"]]


def _eligible(n, solver="auto"):
    return 3 <= n <= 8192 and (solver == "parallel" or (solver == "auto" and n >= 1024))


def _counted(wk, calls):
    orig = {k: getattr(wk, k) for k in calls}

    def counted(k):
        def f(*a, **kw):
            calls[k] += 1
            return orig[k](*a, **kw)
        return f

    for k in calls:
        setattr(wk, k, counted(k))


@pytest.mark.parametrize("name", NAMES)
def test_meitd_auto_and_the_host_driven_loop(meitd, name):
    g = CASES[name]
    x, w = g["x"], float(g["wpemax"])
    n = len(x)
    extract, _, probe = g["port_calls"].tolist()
    got = meitd.MEITD(x.copy(), WPEMAX=w)
    _check(got, g, name, "auto")
    wk = meitd._work_for(n, 0)
    assert wk.one_launch == _eligible(n)
    if wk.one_launch:
        last = dict(wk.last)
        assert last.get("one_launch") and last["status"] == (1 if _early(g) else 0), last
        assert last["extractions"] == extract and last["probes"] == probe, (last, g["port_calls"])
    # the host-driven loop: one launch per operator
    calls = {"extract": 0, "probe": 0}
    _counted(wk, calls)
    was = wk.one_launch
    wk.one_launch = False
    try:
        got = meitd.MEITD(x.copy(), WPEMAX=w)
    finally:
        wk.one_launch = was
        for k in calls:
            delattr(wk, k)
    _check(got, g, name, "host loop")
    assert calls == {"extract": extract, "probe": probe}, (calls, g["port_calls"])


@pytest.mark.parametrize("solver", ["serial", "parallel"])
@pytest.mark.parametrize("name", NAMES)
def test_meitd_under_either_solver(meitd, name, solver):
    g = CASES[name]
    x, w = g["x"], float(g["wpemax"])
    got = meitd.MEITD(x.copy(), WPEMAX=w, solver=solver)
    _check(got, g, name, solver)
    wk = meitd._work_for(len(x), 0, solver)
    assert wk.one_launch == _eligible(len(x), solver)
    if wk.one_launch:
        extract, _, probe = g["port_calls"].tolist()
        assert wk.last.get("one_launch") and wk.last["status"] == (1 if _early(g) else 0), wk.last
        assert wk.last["extractions"] == extract and wk.last["probes"] == probe, (wk.last, g["port_calls"])


def _groups():
    keys = sorted({(len(g["x"]), float(g["wpemax"])) for g in CASES.values()})
    return [(n, w, [k for k in NAMES if len(CASES[k]["x"]) == n and float(CASES[k]["wpemax"]) == w]) for n, w in keys]


@pytest.mark.parametrize("n, w, names", _groups(), ids=lambda v: "-".join(v) if isinstance(v, list) else str(v))
def test_meitd_batch_of_the_cases_of_one_length_and_threshold(meitd, n, w, names):
    """(below 1024 samples the launch takes a batch under solver="parallel" only)"""
    solver = "auto" if n >= 1024 else "parallel"
    x = np.stack([CASES[k]["x"] for k in names])
    got = meitd.MEITD_batch(x, WPEMAX=w, solver=solver)
    st = dict(meitd.last_batch)
    for k, r in zip(names, got):
        _check(r, CASES[k], k, "batch")
    early = sum(1 for k in names if _early(CASES[k]))
    assert st["launches"] == 1 and st["looped"] == 0 and st["handed_back"] == 0, st
    assert st["status"].get(1, 0) == early and st["status"].get(0, 0) == len(names) - early, st


def _filler(n, count, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 1000.0
    return np.stack([np.sin(2 * np.pi * rng.uniform(1, 6) * t) * (1.0 + 0.5 * np.sin(2 * np.pi * rng.uniform(0.1, 1) * t))
                     + 0.3 * np.sin(2 * np.pi * rng.uniform(20, 60) * t + 1.0) + rng.uniform(0.02, 0.3) * rng.standard_normal(n) for _ in range(count)])


@pytest.mark.parametrize("w", sorted({float(g["wpemax"]) for g in CASES.values() if len(g["x"]) == 1024}))
def test_meitd_batch_with_the_cases_scattered_among_other_signals(meitd, w):
    names = [k for k in NAMES if len(CASES[k]["x"]) == 1024 and float(CASES[k]["wpemax"]) == w]
    big = _filler(1024, 32, 5)
    at = np.unique(np.round(np.linspace(0, 31, len(names))).astype(int)) if len(names) > 1 else np.array([17])
    assert len(at) == len(names)
    big[at] = np.stack([CASES[k]["x"] for k in names])
    got = meitd.MEITD_batch(big, WPEMAX=w)
    st = dict(meitd.last_batch)
    assert st["launches"] == 1 and st["looped"] == 0, st
    for k, i in zip(names, at):
        _check(got[i], CASES[k], "%s at %d" % (k, i), "batch scattered")
    if w == 0.6:
        got_x = meitd.XITD_batch(big)
        for k, i in zip(names, at):
            assert len(got_x[i]) == int(CASES[k]["xitd_rows"]), k
            _close(got_x[i], _xitd_ref(CASES[k]), "%s at %d XITD" % (k, i), "XITD_batch scattered")


XITD_NAMES = [k for k in NAMES if "xitd_order" in CASES[k]]


@pytest.mark.parametrize("name", XITD_NAMES)
def test_xitd_rows_in_the_reference_order(meitd, name):
    """the rows ordered by their entropies, the NaN entropies of the early return's all-zero rows last, as numpy sorts them"""
    g = CASES[name]
    with np.errstate(all="ignore"):
        got = meitd.XITD(g["x"].copy())
    assert len(got) == int(g["xitd_rows"])
    _close(got, _xitd_ref(g), name, "XITD")


@pytest.mark.parametrize("n", sorted({len(CASES[k]["x"]) for k in XITD_NAMES}))
def test_xitd_batch_rows_in_the_reference_order(meitd, n):
    names = [k for k in XITD_NAMES if len(CASES[k]["x"]) == n]
    solver = "auto" if n >= 1024 else "parallel"
    with np.errstate(all="ignore"):
        got = meitd.XITD_batch(np.stack([CASES[k]["x"] for k in names]), solver=solver)
    st = dict(meitd.last_batch)
    assert st["launches"] == 1 and st["looped"] == 0 and st["handed_back"] == 0, st
    for k, r in zip(names, got):
        assert len(r) == int(CASES[k]["xitd_rows"]), k
        _close(r, _xitd_ref(CASES[k]), k, "XITD_batch")


@pytest.mark.parametrize("name", NAMES)
def test_the_helpers(meitd, name):
    """determine_if_first_is_proper_rotation / retrieve_proper_rotation (MEITD.py:344-392): `proper` exact; the arrays (stored up to
    1024 samples) to the tolerance; retrieve hands back its input where it finds no proper rotation"""
    g = CASES[name]
    x, w = g["x"], float(g["wpemax"])
    r, b, proper = meitd.determine_if_first_is_proper_rotation(x.copy(), w)
    assert proper == int(g["determine_proper"])
    out, found = meitd.retrieve_proper_rotation(x.copy(), w)
    assert found == int(g["retrieve_proper"])
    if not found:
        assert np.array_equal(out, x)
    if "determine_rotation" in g:
        _close(r, g["determine_rotation"], name + " determine: rotation", "helpers")
        _close(b, g["determine_baseline"], name + " determine: baseline", "helpers")
        _close(out, g["retrieve_rotation"], name + " retrieve", "helpers")


# ---- itd_gather_rows_f64 ----------------------------------------------------------------------------------------------------------
SENTINEL = -7.25


def _gather(eng, src, offsets, n, with_host):
    rows = len(offsets)
    dev = DevArrays(eng, src=src, dst=np.full(rows * n + 64, SENTINEL))
    try:
        out = np.full((rows, n), SENTINEL) if with_host else None
        eng.gather_rows_dev(dev.ptr("src"), src.size, offsets, n, dev.ptr("dst"), out=out)
        return dev.get("dst"), out, dev.get("src")
    finally:
        dev.free()


@pytest.mark.parametrize("with_host", [False, True], ids=["device", "device+host"])
@pytest.mark.parametrize("rows, n", [(1, 1), (1, 257), (7, 1), (40, 255), (40, 256), (40, 257), (65537, 3), (3, 8192)])
def test_gather_rows_against_fancy_indexing(rows, n, with_host):
    """rows at element offsets that overlap and repeat, the last possible one (src_elems - n) and 0 among them; 65537 rows of 3: the
    grid-stride loop beyond 65536 workgroups; n around the 256 threads of a workgroup.  The device destination alone and with the host
    destination; a sentinel behind the destination stays; the source is left alone."""
    from pyitd_amd.spline import _eng
    eng = _eng(1024, 0)
    rng = np.random.default_rng(rows * 1000 + n)
    elems = max(2 * n + 5, min(rows * n // 3, 200000)) if rows > 1 else n + 9
    src = rng.standard_normal(elems)
    offsets = rng.integers(0, elems - n + 1, rows)
    offsets[-1] = elems - n                                         # the last row that fits
    if rows > 3:
        offsets[0], offsets[1], offsets[2] = 0, offsets[-1], max(0, offsets[-1] - n // 2)        # repeated, overlapping
    ref = src[offsets[:, None] + np.arange(n)[None, :]]
    dst, out, src_after = _gather(eng, src, offsets, n, with_host)
    assert np.array_equal(dst[:rows * n].reshape(rows, n), ref)
    assert np.array_equal(dst[rows * n:], np.full(64, SENTINEL))
    assert np.array_equal(src_after, src)
    if with_host:
        assert np.array_equal(out, ref)
