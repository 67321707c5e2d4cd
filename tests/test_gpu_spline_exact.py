"""The natural cubic operator (itd_cubic.hpp) and the parallel not-a-knot solver (itd_nak.hpp) against their EXACT results
(oracle/exact_spline.py) on layouts built for where their scans can go wrong: element counts at the sweep's workgroup geometry,
spacings at the bounds of the warm-up's damping argument, tiles at the evaluation's staging limit, extreme end ratios of the
folded not-a-knot rows, and every ABI path of the operators (caller's list, detected knots, shared and per-signal lists,
strides, I/Q, per-row failures).

Bound, with S = max(|x|, |exact|) and eps = 2^-52:  max err(GPU) <= 4 max err(fp64 oracle) + 64 eps S, where the fp64 oracle
is cpu_oracle.itd_baseline_extract_fast (serial loops) for the natural operator and scipy (spline_oracle.baseline) for the
not-a-knot one.  A 1e-11 error at a workgroup seam, or a warm-up that is too short, exceeds it; the 1e-9 / 1e-10 tolerances
of the older tests do not notice either.  Every measured err / (eps S) is printed (pytest -s) as RATIO lines.
"""
import numpy as np
import pytest

from oracle import cpu_oracle, exact_spline as ex
from test_oracle_exact_spline import (nak_exact, nak_layout, nak_layouts, natural_exact, natural_layout,
                                      natural_layouts)

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
C_REF, C_ABS = 4.0, 64.0
SENT = -7.25e300          # sentinel of the gaps between strided rows


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


# The parallel not-a-knot form at extreme spacing ratios.  It solves for the second derivatives M and recovers the end one as
# M_0 = (1 + r) M_1 - r M_2 (r = h_0 / h_1, mirrored at the other end), and the long segment next to a huge gap is evaluated from
# moments whose difference is multiplied by the ratio: rounding in M_1, M_2 reaches the result amplified by about r.  FITPACK's
# B-spline form (scipy, the serial solver) does not have this amplification.  Measured on the MI355X (err / (eps S)):
# ends_1_10000 8.8e3, ends_10000_1 7.2e3, ends_10000_0.0001 6.3e3, ends_0.0001_10000 2.5e3, ends_10000_10000 237,
# naks_gap2p20 4.9e3, against scipy's 5.6 .. 22.  Those layouts keep their cases with this absolute allowance instead of C_ABS.
NAK_RATIO_ABS = 2.0 ** 14
NAK_RATIO_LAYOUTS = ("ends_0.0001_10000", "ends_1_10000", "ends_10000_0.0001", "ends_10000_1", "ends_10000_10000",
                     "naks_gap2p20")


def _check(what, r, got, x, ref_fp64, c_abs=C_ABS):
    """The bound against the exact result r; prints the ratios."""
    S = r.scale(x)
    e_gpu = float(np.max(r.err(got)))
    e_ref = float(np.max(r.err(ref_fp64)))
    print("RATIO %-34s gpu %9.3g  fp64 %9.3g  (eps S)" % (what, e_gpu / (EPS * S), e_ref / (EPS * S)))
    assert np.all(np.isfinite(got)), what
    assert e_gpu <= C_REF * e_ref + c_abs * EPS * S, "%s: err %.3g eps S, fp64 oracle %.3g eps S" % (
        what, e_gpu / (EPS * S), e_ref / (EPS * S))
    return e_gpu / (EPS * S)


def _tight(name):
    """Layouts of order-1 values and small integer spacings: the kernels hold 1e-14 of the scale outright there."""
    return name.startswith(("count", "tile", "uniform1")) and not name.endswith("_off")


def _bits(a, b, what):
    """Bit equality, +0 == -0 (a scaled copy of the natural operator's zero knot value K[idx-1] is -0 after a negative factor)."""
    a, b = np.ascontiguousarray(a) + 0.0, np.ascontiguousarray(b) + 0.0
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


# ---- the natural cubic operator -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", natural_layouts())
def test_cubic_caller_list_and_detected_knots(P, name):
    L = natural_layout(name)
    x, lst, idx = L["x"], L["lst"], L["idx"]
    r = natural_exact(name, "list")
    got = P.itd_baseline_extract_fast(x, lst, idx)
    u = _check("fast/%s" % name, r, got, x, cpu_oracle.itd_baseline_extract_fast(x, lst, idx))
    if _tight(name):
        assert u * EPS <= 1e-14, (name, u)
    for k in (400, -400):                                   # every operation is homogeneous in x: power-of-two scaling is exact
        _bits(P.itd_baseline_extract_fast(np.ldexp(x, k), lst, idx), np.ldexp(got, k), "fast %s 2^%d" % (name, k))
    if name == "edges":                                     # a list that is not the signal's extrema: no detected form
        return
    rd = natural_exact(name, "detect")
    gd, kn = P.itd_baseline_extract_cubic(x, want_knots=True)
    np.testing.assert_array_equal(kn, L["knots"])
    e, ie = cpu_oracle.extrema_cpp(x)
    u = _check("detect/%s" % name, rd, gd, x, cpu_oracle.itd_baseline_extract_fast(x, e, ie))
    if _tight(name):
        assert u * EPS <= 1e-14, (name, u)
    for k in (400, -400):
        _bits(P.itd_baseline_extract_cubic(np.ldexp(x, k)), np.ldexp(gd, k), "detect %s 2^%d" % (name, k))


def _cubic_batch(P, X, lists, e_stride, idx, x_stride=None, b_stride=None):
    """engine.cubic_batch_dev on device buffers: X [B, n]; lists int32 [B or 1, e_stride or idx + 1 + pad] or None (detected).
    Returns (baseline rows with their stride gaps [B, b_stride], info int32[B])."""
    from pyitd_amd.engine import DeviceBuffer
    from pyitd_amd.itd import _engine_for
    B, n = X.shape
    xs, bs = x_stride or n, b_stride or n
    xh = np.full((B, xs), SENT)
    xh[:, :n] = X
    bh = np.full((B, bs), SENT)
    eh = np.zeros(1, np.int32) if lists is None else np.ascontiguousarray(lists, dtype=np.int32)
    info = np.full(B, 12345, np.int32)
    eng = _engine_for(n)
    buf = DeviceBuffer(xh.nbytes + bh.nbytes + eh.nbytes + info.nbytes)
    px = buf.ptr
    pb = px + xh.nbytes
    pe = pb + bh.nbytes
    pi = pe + eh.nbytes
    for p, a in ((px, xh), (pb, bh), (pe, eh), (pi, info)):
        eng.copy(p, a.ctypes.data, a.nbytes, 1, wait=True)
    eng.cubic_batch_dev(px, n, B, xs, None if lists is None else pe, e_stride, idx, pb, bs, pi)
    eng.copy(bh.ctypes.data, pb, bh.nbytes, 0, wait=True)
    eng.copy(info.ctypes.data, pi, info.nbytes, 0, wait=True)
    xback = np.empty_like(xh)
    eng.copy(xback.ctypes.data, px, xh.nbytes, 0, wait=True)
    buf.free()
    _bits(xback, xh, "the input rows are left alone")
    return bh, info


@pytest.mark.parametrize("name", natural_layouts())
def test_cubic_batch_shared_and_per_signal_lists(P, name):
    L = natural_layout(name)
    x, lst, idx = L["x"], L["lst"], L["idx"]
    n = x.size
    r = natural_exact(name, "list")
    single = P.itd_baseline_extract_fast(x, lst, idx)
    # one shared list for two rows (extrema_stride = 0): the second row is -x / 2, whose exact result is -r / 2 exactly
    X = np.stack((x, -0.5 * x))
    bh, info = _cubic_batch(P, X, lst[None, : idx + 1], 0, idx)
    assert list(info) == [idx, idx]
    _bits(bh[0], single, "shared list row 0 = the single-signal call")
    _check("batch shared/%s" % name, r, bh[0], x, cpu_oracle.itd_baseline_extract_fast(x, lst, idx))
    _bits(bh[1], -0.5 * bh[0], "shared list row 1")
    # per-signal lists (extrema_stride = idx + 1 + pad): identical lists give the shared call's rows bit for bit ...
    pad = 3
    E = np.full((2, idx + 1 + pad), -99, np.int32)
    E[:, : idx + 1] = lst[: idx + 1]
    bp, info = _cubic_batch(P, X, E, idx + 1 + pad, idx)
    assert list(info) == [idx, idx]
    _bits(bp, bh, "per-signal identical lists = shared list")
    # ... and a different list per row is each row's own operator
    lst2 = lst[: idx + 1] + 1
    if lst2[-1] < n:
        E[1, : idx + 1] = lst2
        bp, info = _cubic_batch(P, X, E, idx + 1 + pad, idx)
        assert list(info) == [idx, idx]
        _bits(bp[0], bh[0], "row 0 keeps its list")
        r2 = ex.natural(X[1], lst2, idx)
        _check("batch per-signal/%s" % name, r2, bp[1], X[1], cpu_oracle.itd_baseline_extract_fast(X[1], lst2, idx))


@pytest.mark.parametrize("name", ["count1025", "tile320", "hugegap", "count2"])
def test_cubic_batch_strides_and_per_row_failures(P, name):
    L = natural_layout(name)
    x, lst, idx = L["x"], L["lst"], L["idx"]
    n = x.size
    r = natural_exact(name, "list")
    rd = natural_exact(name, "detect")
    X = np.stack((x, x, -0.5 * x, x))
    xs, bs = n + 3, n + 5
    # per-signal lists: row 1 not strictly increasing -> info -1 and its row untouched; the others computed
    pad = 2
    E = np.zeros((4, idx + 1 + pad), np.int32)
    E[:, : idx + 1] = lst[: idx + 1]
    E[1, 1] = E[1, 0]
    bh, info = _cubic_batch(P, X, E, idx + 1 + pad, idx, xs, bs)
    assert list(info) == [idx, -1, idx, idx], info
    assert np.all(bh[:, n:] == SENT), "the stride gaps are written"
    assert np.all(bh[1] == SENT), "the invalid row is written"
    ref = cpu_oracle.itd_baseline_extract_fast(x, lst, idx)
    for row, f in ((0, 1.0), (2, -0.5), (3, 1.0)):
        _check("strided list row %d/%s" % (row, name), r, bh[row, :n] / f, x, ref)
    # detected knots: a NaN row gets -2 and stays untouched; the others are the detected operator
    X2 = X.copy()
    X2[2, n // 2] = np.nan
    bh, info = _cubic_batch(P, X2, None, 0, 0, xs, bs)
    assert list(info) == [len(L["knots"]), len(L["knots"]), -2, len(L["knots"])], info
    assert np.all(bh[:, n:] == SENT) and np.all(bh[2] == SENT)
    e, ie = cpu_oracle.extrema_cpp(x)
    refd = cpu_oracle.itd_baseline_extract_fast(x, e, ie)
    for row in (0, 1, 3):
        _check("strided detect row %d/%s" % (row, name), rd, bh[row, :n], x, refd)


@pytest.mark.parametrize("name", natural_layouts())
def test_iq_with_retained_knots(P, name):
    L = natural_layout(name)
    x, lst, idx = L["x"], L["lst"], L["idx"]
    rng = np.random.default_rng(len(name))
    Q = 0.5 * x + 0.25 * np.max(np.abs(x)) * rng.standard_normal(x.size)
    r = ex.iq(x, Q, lst, idx)
    got = P.itd_baseline_extract_iq(x + 1j * Q, lst, idx)
    avg = (x + Q) / 2.0
    _check("iq/%s" % name, r, got, np.maximum(np.abs(x), np.abs(Q)), cpu_oracle.itd_baseline_extract_fast(avg, lst, idx))


# ---- the not-a-knot (FITPACK) flavour -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spline():
    from pyitd_amd import spline
    from oracle import spline_oracle
    return spline, spline_oracle


@pytest.mark.parametrize("name", nak_layouts())
def test_nak_parallel_and_serial(spline, name):
    sp, so = spline
    L = nak_layout(name)
    x = L["x"]
    r = nak_exact(name)
    ref = so.baseline(x, 0)
    c_abs = NAK_RATIO_ABS if name in NAK_RATIO_LAYOUTS else C_ABS
    for solver in ("parallel", "serial"):
        got = sp.itd_baseline_extract_modified(x, solver=solver)
        _check("nak %s/%s" % (solver, name), r, got, x, ref, C_ABS if solver == "serial" else c_abs)
        if solver == "parallel":
            for k in (400, -400):
                _bits(sp.itd_baseline_extract_modified(np.ldexp(x, k), solver=solver), np.ldexp(got, k),
                      "nak %s 2^%d" % (name, k))
    rot, base = sp.itd_baseline_extract_spline(x, solver="parallel")        # MEITD's form
    _check("nak meitd/%s" % name, r, base, x, ref, c_abs)
    _bits(rot, x - base, "meitd rotation")
    # two rows: the per-row launches; row 1 = -x / 2 (same knots, exact result -r / 2)
    rows = sp.itd_baseline_extract_rows(np.stack((x, -0.5 * x)), 10, solver="parallel")
    _check("nak rows/%s" % name, r, rows[0], x, ref, c_abs)
    r1 = ex.Exact(r.samples, -0.5 * r.hi, -0.5 * r.lo)
    _check("nak rows 1/%s" % name, r1, rows[1], 0.5 * x, -0.5 * ref, c_abs)
