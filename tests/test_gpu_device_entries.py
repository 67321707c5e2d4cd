"""The single-signal device-pointer entries and the float32 entries of the C ABI (include/pyitd_hip.h) against references.

The suite reaches most single-signal operators through their host forms only; these tests call the device forms on buffers of
their own (sentinel-filled, with pads behind every output), on the caller's stream, with every optional output left out in turn:
  itd_baseline_extract_f64 / _f32     rows bit for bit against oracle.cpu_oracle.itd_baseline_extract, knots and count exact
  itd_detect_f64 / _f32               all five modes against the oracle's function for each mode
  itd_baseline_extract_cubic_f64/_f32 the caller's list and detected knots against oracle.exact_spline (the bound and layouts of
  itd_baseline_extract_iq_f64         test_gpu_spline_exact.py) and bit for bit against the host forms
  itd_baseline_extract_spline_f64     strided batches under both solvers, row by row bit for bit against the host form
  itd_crossways_f64                   against oracle.spline_oracle.crossways
  itd_engine_device
  itd_baseline_extract_batch_f64      here only with batch = 1 beside the single-signal entry's plain-rule form; held to references
  itd_detect_batch_f64                (the C oracle, and oracle.numpy_itd's plain rules for NaN rows) in test_gpu_batch_ops.py
Every _f32 entry gives exactly what its _f64 twin gives on the widened signal.  NaN input follows pyitd_hip.h's rules, and
arguments that are refused on the host are refused.
"""
import ctypes
import itertools

import numpy as np
import pytest

from helpers import DevArrays, assert_bits_equal
from oracle import cpu_oracle, exact_spline as ex
from test_gpu_spline_exact import _check
from test_oracle_exact_spline import natural_exact, natural_layout, natural_layouts

pytestmark = pytest.mark.gpu
SENT = -7.25e300
ISENT = -123456
PAD = 7
SHAPES = (3, 4, 5, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 3001 * 512 + 317)
MAX_N = 3001 * 512 + 317
OK, INVALID, NONFINITE = 0, 1, 6


@pytest.fixture(scope="module")
def eng():
    import pyitd_amd
    e = pyitd_amd.Engine(MAX_N, 1, 0)
    yield e
    e.close()


def _bits(a, b, what):
    """Bit equality (+0 and -0 differ), any NaN == any NaN."""
    assert_bits_equal(a, b, what)


def _i64(v=0):
    return ctypes.c_int64(v)


# ---- float32 signals that stress the predicates ---------------------------------------------------------------------------
def signal32(kind, n, seed=0):
    """int16: quantised to int16 steps (ties, plateaus); tiny: +-0.0 and float32 subnormals; thirds: values that are not exact
    halves.  Every kind has knots at sample 1 and at n-2 and on both sides of the tile seams."""
    rng = np.random.default_rng(seed + 7 * n + len(kind))
    if kind == "int16":
        x = (rng.integers(-3, 4, n) * 4096).astype(np.float32)
    elif kind == "tiny":
        v = np.array([0.0, -0.0, 1.4e-45, -1.4e-45, 2.8e-45, -5.9e-39, 1.1e-38], np.float32)
        x = v[rng.integers(0, v.size, n)]
    else:
        x = (rng.standard_normal(n) / 3.0).astype(np.float32)
    if n >= 4:
        hi = np.float32(np.max(np.abs(x)) * 2 + 1e-38)
        x[1], x[n - 2] = hi, -hi
    for t in range(512, n - 1, 512):
        x[t - 1], x[t] = hi, -hi
    return x


KINDS = ("int16", "tiny", "thirds")


# ---- itd_baseline_extract_f64 / _f32 ----------------------------------------------------------------------------------------
def _extract(eng, fn, x, want_knots=True, want_m=True, stream=None, d=None):
    n = x.size
    own = d is None
    if own:
        d = DevArrays(eng, x=x, rot=np.full(n + PAD, SENT), base=np.full(n + PAD, SENT), kn=np.full(n + PAD, ISENT, np.int32))
    m = _i64(-5)
    rc = fn(eng._h, d.ptr("x"), n, d.ptr("rot"), d.ptr("base"), d.ptr("kn") if want_knots else None,
            ctypes.byref(m) if want_m else None, stream)
    out = dict(rc=rc, m=m.value, rot=d.get("rot"), base=d.get("base"), kn=d.get("kn"), x=d.get("x"))
    if own:
        d.free()
    return out


@pytest.mark.parametrize("n", SHAPES)
def test_extract_f64_and_f32_against_the_oracle(eng, n):
    L = eng._L
    for kind in KINDS:
        x32 = signal32(kind, n)
        x = x32.astype(np.float64)
        rot, base, kn, _ = cpu_oracle.itd_baseline_extract(x, want_knots=True)
        g = _extract(eng, L.itd_baseline_extract_f64, x)
        assert g["rc"] == OK
        _bits(g["rot"][:n], rot, "%s n=%d rotation" % (kind, n))
        _bits(g["base"][:n], base, "%s n=%d baseline" % (kind, n))
        assert g["m"] == len(kn) and np.array_equal(g["kn"][: len(kn)], kn), (kind, n)
        assert np.all(g["kn"][len(kn):] == ISENT) and np.all(g["rot"][n:] == SENT) and np.all(g["base"][n:] == SENT)
        _bits(g["x"], x, "the input is left alone")
        h = _extract(eng, L.itd_baseline_extract_f32, x32)
        assert h["rc"] == OK
        for k in ("rot", "base", "kn"):
            _bits(h[k], g[k], "%s n=%d f32 %s = f64 of the widened signal" % (kind, n, k))
        assert h["m"] == g["m"]
        assert np.array_equal(h["x"].view(np.uint32), x32.view(np.uint32))


@pytest.mark.parametrize("n", (5, 1025, 5 * 512 + 3))
def test_extract_optional_outputs(eng, n):
    x = signal32("thirds", n).astype(np.float64)
    full = _extract(eng, eng._L.itd_baseline_extract_f64, x)
    for want_knots, want_m in itertools.product((False, True), repeat=2):
        for fn in (eng._L.itd_baseline_extract_f64, eng._L.itd_baseline_extract_f32):
            xx = x.astype(np.float32) if fn is eng._L.itd_baseline_extract_f32 else x
            ref = full if xx is x else _extract(eng, fn, xx)
            g = _extract(eng, fn, xx, want_knots, want_m)
            assert g["rc"] == OK
            _bits(g["rot"], ref["rot"], "rotation")
            _bits(g["base"], ref["base"], "baseline")
            if want_knots:
                assert np.array_equal(g["kn"], ref["kn"])
            else:
                assert np.all(g["kn"] == ISENT), "the knot buffer was not passed"
            assert g["m"] == (ref["m"] if want_m else -5)


# ---- itd_detect_f64 / _f32 --------------------------------------------------------------------------------------------------
def oracle_detect(x, mode):
    if mode == 0:
        return cpu_oracle.knots(x)
    if mode in (1, 2):
        return cpu_oracle.detect_peaks(x, matlab=mode == 2)
    if mode == 3:
        e, idx = cpu_oracle.extrema_cpp(x)
        return e[:idx]
    e, idx = cpu_oracle.find_extrema(x)          # [0, crossings, extrapolated]: the entry delivers the crossings alone
    return e[1: idx - 1]


def _detect(eng, fn, x, mode, stream=None, d=None):
    n = x.size
    own = d is None
    if own:
        d = DevArrays(eng, x=x, kn=np.full(n + PAD, ISENT, np.int32))
    m = _i64(-5)
    rc = fn(eng._h, d.ptr("x"), n, mode, d.ptr("kn"), ctypes.byref(m), stream)
    out = dict(rc=rc, m=m.value, kn=d.get("kn"), x=d.get("x"))
    if own:
        d.free()
    return out


@pytest.mark.parametrize("n", SHAPES)
def test_detect_f64_and_f32_all_modes(eng, n):
    for kind in KINDS:
        x32 = signal32(kind, n, seed=1)
        x = x32.astype(np.float64)
        for mode in range(5):
            want = oracle_detect(x, mode)
            for fn, xx in ((eng._L.itd_detect_f64, x), (eng._L.itd_detect_f32, x32)):
                g = _detect(eng, fn, xx, mode)
                what = "%s n=%d mode %d %s" % (kind, n, mode, xx.dtype)
                assert g["rc"] == OK, what
                assert g["m"] == len(want), (what, g["m"], len(want))
                assert np.array_equal(g["kn"][: len(want)], want), what
                assert np.all(g["kn"][len(want):] == ISENT), what
                assert np.array_equal(g["x"].view(np.uint8), xx.view(np.uint8)), what


# ---- the natural cubic operator and its I/Q form on device lists --------------------------------------------------------------
def _cubic(eng, fn, x, lst=None, idx=0, stream=None):
    n = x.size
    d = DevArrays(eng, x=x, base=np.full(n + PAD, SENT), e=np.zeros(1, np.int32) if lst is None else np.asarray(lst, np.int32))
    got = _i64(-5)
    rc = fn(eng._h, d.ptr("x"), n, None if lst is None else d.ptr("e"), idx, d.ptr("base"), ctypes.byref(got), stream)
    out = dict(rc=rc, idx=got.value, base=d.get("base"), x=d.get("x"))
    d.free()
    return out


@pytest.mark.parametrize("name", natural_layouts())
def test_cubic_device_list_and_detected_knots(name):
    import pyitd_amd as P
    from pyitd_amd.itd import _engine_for
    Lo = natural_layout(name)
    x, lst, idx = Lo["x"], Lo["lst"], Lo["idx"]
    n = x.size
    eng = _engine_for(n)                  # (the layouts reach 1.1e7 samples: the host forms' engine, grown to fit)
    g = _cubic(eng, eng._L.itd_baseline_extract_cubic_f64, x, lst[: idx + 1], idx)
    assert g["rc"] == OK and g["idx"] == idx
    assert np.all(g["base"][n:] == SENT)
    _bits(g["base"][:n], P.itd_baseline_extract_fast(x, lst, idx), "list %s = the host form" % name)
    _check("dev list/%s" % name, natural_exact(name, "list"), g["base"][:n], x, cpu_oracle.itd_baseline_extract_fast(x, lst, idx))
    if name != "edges":
        gd = _cubic(eng, eng._L.itd_baseline_extract_cubic_f64, x)
        assert gd["rc"] == OK and gd["idx"] == len(Lo["knots"])
        _bits(gd["base"][:n], P.itd_baseline_extract_cubic(x), "detected %s = the host form" % name)
        e, ie = cpu_oracle.extrema_cpp(x)
        _check("dev detect/%s" % name, natural_exact(name, "detect"), gd["base"][:n], x, cpu_oracle.itd_baseline_extract_fast(x, e, ie))
    # float32 = float64 of the widened signal
    x32 = x.astype(np.float32)
    for lst_, idx_ in ((lst[: idx + 1], idx), (None, 0)):
        a = _cubic(eng, eng._L.itd_baseline_extract_cubic_f32, x32, lst_, idx_)
        b = _cubic(eng, eng._L.itd_baseline_extract_cubic_f64, x32.astype(np.float64), lst_, idx_)
        assert a["rc"] == b["rc"] and a["idx"] == b["idx"]
        _bits(a["base"], b["base"], "%s f32 = f64 of the widened signal" % name)


def _iq(eng, I, Q, lst=None, idx=0, misalign=False):
    n = I.size
    iq = np.empty(2 * n + 2)
    iq[0:2 * n:2], iq[1:2 * n:2] = I, Q
    if misalign:
        iq = np.concatenate(([0.0], iq[:-1]))
    d = DevArrays(eng, iq=iq, base=np.full(n + PAD, SENT), e=np.zeros(1, np.int32) if lst is None else np.asarray(lst, np.int32))
    got = _i64(-5)
    rc = eng._L.itd_baseline_extract_iq_f64(eng._h, d.ptr("iq") + (8 if misalign else 0), n, None if lst is None else d.ptr("e"),
                                            idx, d.ptr("base"), ctypes.byref(got), None)
    out = dict(rc=rc, idx=got.value, base=d.get("base"))
    _bits(d.get("iq"), iq, "the I/Q input is left alone")
    d.free()
    return out


@pytest.mark.parametrize("name", ["count2", "count64", "count1025", "tile320", "hugegap", "geometric", "edges"])
def test_iq_device_list_and_detected_knots(name):
    import pyitd_amd as P
    from pyitd_amd.itd import _engine_for
    Lo = natural_layout(name)
    x, lst, idx = Lo["x"], Lo["lst"], Lo["idx"]
    n = x.size
    eng = _engine_for(n)
    rng = np.random.default_rng(len(name))
    Q = 0.5 * x + 0.25 * np.max(np.abs(x)) * rng.standard_normal(n)
    g = _iq(eng, x, Q, lst[: idx + 1], idx)
    assert g["rc"] == OK
    assert np.all(g["base"][n:] == SENT)
    _bits(g["base"][:n], P.itd_baseline_extract_iq(x + 1j * Q, lst, idx), "iq list %s = the host form" % name)
    _check("dev iq/%s" % name, ex.iq(x, Q, lst, idx), g["base"][:n], np.maximum(np.abs(x), np.abs(Q)),
           cpu_oracle.itd_baseline_extract_fast((x + Q) / 2.0, lst, idx))
    gd = _iq(eng, x, Q)
    hb, hk, hidx = P.itd_baseline_extract_iq(x + 1j * Q, want_knots=True)
    assert gd["rc"] == OK and gd["idx"] == hidx == len(hk)
    if hidx >= 2:
        _bits(gd["base"][:n], hb, "iq detected %s = the host form" % name)
    else:
        assert np.all(gd["base"] == SENT), "fewer than two knots leave the buffer alone"
    assert _iq(eng, x, Q, lst[: idx + 1], idx, misalign=True)["rc"] == INVALID      # not 16-byte aligned


# ---- the FITPACK flavour over strided batches -------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", (2, 300))
def test_spline_strided_batch_is_the_host_form_row_by_row(eng, batch):
    """batch 2 takes the parallel-in-knots solver under AUTO, batch 300 FITPACK's serial sweep; all three strides exceed n."""
    n = 1100
    rng = np.random.default_rng(batch)
    X = rng.integers(0, 256, (batch, n)).astype(np.float64)
    X[0] = np.round(100 * np.sin(np.arange(n) / 40.0))
    X[-1] = np.linspace(0.0, 1.0, n)                                      # no knots: returned unchanged
    xs, bs, rs = n + 3, n + 5, n + 9
    href, hrot, hkn = np.empty((batch, n)), np.empty((batch, n)), np.zeros(batch, np.int32)
    assert eng._L.itd_baseline_extract_spline_host_f64(eng._h, X.ctypes.data, n, batch, 10, href.ctypes.data, hrot.ctypes.data,
                                                       hkn.ctypes.data) == OK
    for with_rot, with_kn in ((True, True), (False, False), (True, False), (False, True)):
        xh = np.full((batch + 1, xs), SENT)
        xh[:batch, :n] = X
        d = DevArrays(eng, x=xh, base=np.full((batch + 1, bs), SENT), rot=np.full((batch + 1, rs), SENT))
        kn = np.full(batch, ISENT, np.int32)
        rc = eng._L.itd_baseline_extract_spline_f64(eng._h, d.ptr("x"), n, batch, xs, 10, d.ptr("base"), bs,
                                                    d.ptr("rot") if with_rot else None, rs,
                                                    kn.ctypes.data if with_kn else None, None)
        assert rc == OK
        base, rot = d.get("base"), d.get("rot")
        _bits(d.get("x"), xh, "the input rows are left alone")
        d.free()
        _bits(base[:batch, :n], href, "baseline rows")
        assert np.all(base[:batch, n:] == SENT) and np.all(base[batch] == SENT), "stride gaps / the row beyond the batch"
        if with_rot:
            _bits(rot[:batch, :n], hrot, "rotation rows")
            assert np.all(rot[:batch, n:] == SENT) and np.all(rot[batch] == SENT)
        else:
            assert np.all(rot == SENT)
        if with_kn:
            assert np.array_equal(kn, hkn)
        else:
            assert np.all(kn == ISENT)


def test_crossways_device_form_against_the_oracle(eng):
    from oracle import spline_oracle as so
    rng = np.random.default_rng(9)
    planes, rows, cols = 2, 40, 57
    img = rng.integers(0, 256, (planes, rows, cols)).astype(np.float64)
    img[1] = np.round(80 * np.sin(np.arange(rows)[:, None] / 5.0) * np.cos(np.arange(cols)[None, :] / 7.0))
    cnt = planes * rows * cols
    d = DevArrays(eng, img=img, out=np.full(cnt + PAD, SENT))
    assert eng._L.itd_crossways_f64(eng._h, d.ptr("img"), planes, rows, cols, 10, d.ptr("out"), None) == OK
    out = d.get("out")
    _bits(d.get("img"), img, "the image is left alone")
    d.free()
    assert np.all(out[cnt:] == SENT)
    got = out[:cnt].reshape(planes, rows, cols)
    _bits(got, eng.crossways_host(img, 10), "device form = host form")
    for p in range(planes):
        ref = so.crossways(img[p], 10)
        assert np.max(np.abs(got[p] - ref)) <= 1e-12 * max(1.0, float(np.max(np.abs(ref)))), "plane %d" % p


# ---- the caller's stream ----------------------------------------------------------------------------------------------------
def test_entries_run_on_the_callers_stream(eng):
    """The input is filled by a device copy queued on the caller's stream; the entry is called on that stream and read after
    that stream alone has been synchronised: the results are the new input's."""
    import torch
    n = 7 * 512 + 11
    s = torch.cuda.Stream()
    new = signal32("thirds", n, seed=3).astype(np.float64)
    old = signal32("int16", n, seed=4).astype(np.float64)
    rot, base, kn, _ = cpu_oracle.itd_baseline_extract(new, want_knots=True)

    def staged(**extra):
        d = DevArrays(eng, x=old, stage=new, **extra)
        eng.copy(d.ptr("x"), d.ptr("stage"), new.nbytes, 2, wait=False, stream=s.cuda_stream)
        return d

    d = staged(rot=np.full(n, SENT), base=np.full(n, SENT), kn=np.full(n, ISENT, np.int32))
    g = _extract(eng, eng._L.itd_baseline_extract_f64, new, stream=s.cuda_stream, d=d)
    s.synchronize()
    assert g["rc"] == OK and g["m"] == len(kn)
    _bits(g["rot"], rot, "extract on the caller's stream")
    _bits(g["base"], base, "extract on the caller's stream")
    d.free()
    d = staged(kn=np.full(n, ISENT, np.int32))
    g = _detect(eng, eng._L.itd_detect_f64, new, 3, stream=s.cuda_stream, d=d)
    want = oracle_detect(new, 3)
    assert g["rc"] == OK and g["m"] == len(want) and np.array_equal(g["kn"][: len(want)], want)
    d.free()
    d = staged(base=np.full(n, SENT))
    got = _i64()
    rc = eng._L.itd_baseline_extract_cubic_f64(eng._h, d.ptr("x"), n, None, 0, d.ptr("base"), ctypes.byref(got), s.cuda_stream)
    s.synchronize()
    import pyitd_amd as P
    assert rc == OK
    _bits(d.get("base"), P.itd_baseline_extract_cubic(new), "cubic on the caller's stream")
    d.free()


# ---- NaN input (pyitd_hip.h: itd_set_nan_input_mode) ----------------------------------------------------------------------
@pytest.fixture
def nan_eng():
    import pyitd_amd
    e = pyitd_amd.Engine(1 << 14, 1, 0)
    yield e
    e.close()


@pytest.mark.parametrize("n", (5, 1025, 4099))
def test_nan_input_of_the_device_entries(nan_eng, n):
    eng = nan_eng
    L = eng._L
    x32 = signal32("thirds", n, seed=5)
    x32[n // 2] = np.nan
    if n > 5:
        x32[[0, 700 % n, n - 1]] = np.nan
    x = x32.astype(np.float64)
    rot, base, kn, bk = cpu_oracle.itd_baseline_extract(x, want_knots=True)       # the reference's NaN branch
    # the host form: the knot values too (those of the mutated copy: the branch's infinities are among them)
    assert not np.all(np.isfinite(bk))
    keep = x.copy()
    h_rot, h_base, h_kn, h_bk = eng.baseline_extract_host(x, want_knots=True)
    _bits(h_rot, rot, "host form, NaN branch rotation")
    _bits(h_base, base, "host form, NaN branch baseline")
    assert h_kn.dtype == np.int64 and np.array_equal(h_kn, kn)
    assert h_bk.shape == (len(kn) + 2,)
    _bits(h_bk, bk, "host form, NaN branch knot values")
    _bits(x, keep, "the host form leaves the caller's array alone")
    for fn, xx in ((L.itd_baseline_extract_f64, x), (L.itd_baseline_extract_f32, x32)):
        for want_knots, want_m in ((True, True), (False, True), (True, False)):
            g = _extract(eng, fn, xx, want_knots, want_m)
            assert g["rc"] == OK
            _bits(g["rot"][:n], rot, "NaN branch rotation")
            _bits(g["base"][:n], base, "NaN branch baseline")
            if want_knots:
                assert np.array_equal(g["kn"][: len(kn)], kn)
            if want_m:
                assert g["m"] == len(kn)
            assert np.array_equal(g["x"].view(np.uint8), xx.view(np.uint8)), "the NaN re-run writes the input"
        # without m_host / knots_dev: the plain rules, = itd_baseline_extract_batch_f64 (info -1 - count)
        g = _extract(eng, fn, xx, False, False)
        assert g["rc"] == OK
        d = DevArrays(eng, x=x, rot=np.full(n, SENT), base=np.full(n, SENT), info=np.zeros(1, np.int32))
        assert L.itd_baseline_extract_batch_f64(eng._h, d.ptr("x"), n, 1, n, d.ptr("rot"), n, d.ptr("base"), n, d.ptr("info"), None) == OK
        _bits(g["rot"][:n], d.get("rot"), "plain rules rotation")
        _bits(g["base"][:n], d.get("base"), "plain rules baseline")
        assert d.get("info")[0] < 0
        d.free()
    for mode in range(5):
        for fn, xx in ((L.itd_detect_f64, x), (L.itd_detect_f32, x32)):
            g = _detect(eng, fn, xx, mode)
            if mode <= 2:
                want = oracle_detect(x, mode)
                assert g["rc"] == OK and g["m"] == len(want) and np.array_equal(g["kn"][: len(want)], want), (mode, xx.dtype)
            else:
                assert g["rc"] == NONFINITE, (mode, xx.dtype)
            assert np.array_equal(g["x"].view(np.uint8), xx.view(np.uint8))
    assert _cubic(eng, L.itd_baseline_extract_cubic_f64, x)["rc"] == NONFINITE
    assert _cubic(eng, L.itd_baseline_extract_cubic_f32, x32)["rc"] == NONFINITE
    assert _iq(eng, x, x)["rc"] == NONFINITE
    if n >= 1024:
        d = DevArrays(eng, x=x, base=np.full(n, SENT), a=np.full(n, SENT))
        assert L.itd_baseline_extract_spline_f64(eng._h, d.ptr("x"), n, 1, n, 0, d.ptr("base"), n, None, 0, None, None) == NONFINITE
        assert L.itd_instantaneous_f64(eng._h, d.ptr("x"), n, d.ptr("a"), None, None, None) == NONFINITE
        d.free()
    # ITD_NAN_INPUT_REJECT: the synchronising forms refuse
    assert L.itd_set_nan_input_mode(eng._h, 1) == OK
    for fn, xx in ((L.itd_baseline_extract_f64, x), (L.itd_baseline_extract_f32, x32)):
        assert _extract(eng, fn, xx)["rc"] == NONFINITE
    for mode in range(5):
        assert _detect(eng, L.itd_detect_f32, x32, mode)["rc"] == NONFINITE
    assert L.itd_set_nan_input_mode(eng._h, 0) == OK


# ---- arguments refused on the host --------------------------------------------------------------------------------------------
def test_rejected_arguments(nan_eng):
    eng = nan_eng
    L, h = eng._L, eng._h
    big = eng.max_n + 1
    n = 3000
    x = np.sin(np.arange(n) / 9.0)
    d = DevArrays(eng, x=x, x32=x.astype(np.float32), o1=np.full(n, SENT), o2=np.full(n, SENT), o3=np.full(n, SENT),
                  kn=np.full(n, ISENT, np.int32), iq=np.zeros(2 * n + 2))
    m = _i64()
    for bad_n in (2, big):
        assert L.itd_baseline_extract_f64(h, d.ptr("x"), bad_n, d.ptr("o1"), d.ptr("o2"), None, ctypes.byref(m), None) == INVALID
        assert L.itd_baseline_extract_f32(h, d.ptr("x32"), bad_n, d.ptr("o1"), d.ptr("o2"), None, ctypes.byref(m), None) == INVALID
        for fn in (L.itd_detect_f64, L.itd_detect_f32):
            assert fn(h, d.ptr("x"), bad_n, 0, d.ptr("kn"), ctypes.byref(m), None) == INVALID
        for fn in (L.itd_baseline_extract_cubic_f64, L.itd_baseline_extract_cubic_f32):
            assert fn(h, d.ptr("x"), bad_n, None, 0, d.ptr("o1"), ctypes.byref(m), None) == INVALID
        assert L.itd_baseline_extract_iq_f64(h, d.ptr("iq"), bad_n, None, 0, d.ptr("o1"), ctypes.byref(m), None) == INVALID
        assert L.itd_instantaneous_f64(h, d.ptr("x"), bad_n, d.ptr("o1"), None, None, None) == INVALID
    assert L.itd_baseline_extract_spline_f64(h, d.ptr("x"), 2, 1, 2, 0, d.ptr("o1"), 2, None, 0, None, None) == INVALID
    assert L.itd_crossways_f64(h, d.ptr("x"), 1, 2, 50, 10, d.ptr("o1"), None) == INVALID
    assert L.itd_baseline_extract_iq_f64(h, d.ptr("iq") + 8, 100, None, 0, d.ptr("o1"), ctypes.byref(m), None) == INVALID
    nb = 10                       # strides < n with batch > 1, each of the three
    for xs, bs, rs in ((nb - 1, nb, nb), (nb, nb - 1, nb), (nb, nb, nb - 1)):
        assert L.itd_baseline_extract_spline_f64(h, d.ptr("x"), nb, 2, xs, 0, d.ptr("o1"), bs, d.ptr("o2"), rs, None, None) == INVALID
    assert L.itd_instantaneous_f64(h, d.ptr("x"), n, None, None, None, None) == INVALID
    for fn in (L.itd_detect_f64, L.itd_detect_f32):
        assert fn(h, d.ptr("x"), n, 5, d.ptr("kn"), ctypes.byref(m), None) == INVALID
    # the bad knot lists of test_gpu_cubic.py::test_bad_knot_lists_are_rejected, as device lists (k_cubic_validate)
    for lst, idx in (([0, 10, 10, 50, 0], 4), ([0, 10, 20, 5000, 0], 4), ([0, 10, 20, -5, 0], 4), ([0, 0], 1)):
        g = _cubic(eng, L.itd_baseline_extract_cubic_f64, x, lst, idx)
        assert g["rc"] == INVALID and np.all(g["base"] == SENT), lst
        g = _cubic(eng, L.itd_baseline_extract_cubic_f32, x.astype(np.float32), lst, idx)
        assert g["rc"] == INVALID and np.all(g["base"] == SENT), lst
        assert _iq(eng, x, x, lst, idx)["rc"] == INVALID, lst
    for k in ("o1", "o2", "o3"):
        assert np.all(d.get(k) == SENT), "a refused call wrote %s" % k
    assert np.all(d.get("kn") == ISENT)
    d.free()


def test_rejected_knot_lists_of_the_cubic_host_forms():
    """A caller's list with idx outside [2, n - 1] or an entry outside [0, n): refused before anything is enqueued, the caller's
    baseline buffer untouched, and the next valid call on the same engine gives what a fresh engine gives."""
    import pyitd_amd
    n = 16
    x = signal32("thirds", n, seed=2).astype(np.float64)
    z = (x + 1j * signal32("thirds", n, seed=3)).view(np.float64)
    good = np.array([0, 3, 6, 9, 12, 15], np.int64)
    forms = (("itd_baseline_extract_cubic_host_f64", x), ("itd_baseline_extract_iq_host_f64", z))

    def call(e, name, arr, lst, idx):
        base = np.full(n + PAD, SENT)
        got = _i64(-5)
        rc = getattr(e._L, name)(e._h, arr.ctypes.data, n, lst.ctypes.data, idx, base.ctypes.data, ctypes.byref(got), None)
        return rc, base

    fresh = pyitd_amd.Engine(1 << 10, 1, 0)
    want = [call(fresh, name, arr, good, 5) for name, arr in forms]
    fresh.close()
    e = pyitd_amd.Engine(1 << 10, 1, 0)
    long_list = np.arange(n + 1, dtype=np.int64) % n
    for (name, arr), (want_rc, want_base) in zip(forms, want):
        assert want_rc == OK and np.all(want_base[:n] != SENT) and np.all(want_base[n:] == SENT)
        bad = [(good, 1), (long_list, n)]
        bad += [(np.array(lst, np.int64), 5) for lst in ([0, 3, 6, 9, n, 15], [0, 3, -1, 9, 12, 15], [0, 3, 6, 9, 12, n])]
        for lst, idx in bad:
            rc, base = call(e, name, arr, lst, idx)
            assert rc == INVALID, (name, lst, idx)
            assert np.all(base == SENT), "a refused call wrote the baseline (%s, idx %d)" % (name, idx)
            rc, base = call(e, name, arr, good, 5)
            assert rc == OK
            _bits(base, want_base, "%s after a refused call" % name)
    e.close()


def test_engine_device(eng):
    assert eng._L.itd_engine_device(eng._h) == 0
    assert eng._L.itd_engine_device(None) == -1
