"""Selected result rows (itd_decompose_select_*, select=): the arithmetic is the full entries', only the named rows are stored, densely
packed — the selected rotations in ascending order, the residual's slot last.  The expected value of every delivered slot is the CPU
oracle's float64 row (through numpy's astype for float32 rows), compared on bit patterns (any NaN equal to any NaN), with n_rows from the
summary: the slot of rotation r is checked where r <= n_rows - 2, the residual's slot always holds row n_rows - 1.  Every result
buffer is exactly B * S * n elements, pre-filled with a sentinel NaN and followed by a guard region that must come back untouched: a
row that was not selected has nowhere to go."""
import numpy as np
import pytest

from conftest import golden_cases
from helpers import DevArrays, coarse, fuzz_signal, load_golden, sha, sines_noise

pytestmark = pytest.mark.gpu

SENT32 = np.uint32(0x7FC5A5A5)      # NaNs no computation produces
SENT64 = np.uint64(0x7FF85A5A5A5A5A5A)
OK, INVALID_ARG = 0, 1


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


@pytest.fixture(scope="module")
def oracle():
    from oracle import cpu_oracle
    cpu_oracle.lib()
    return cpu_oracle


def canon(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))
    assert a.dtype == np.float64
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def as_type(rows64, dt):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(rows64, dtype=np.float64).astype(dt)


def assert_bits(got, want64, what):
    """got (float32 or float64) against the oracle's float64 values in got's type, bit for bit."""
    want = as_type(want64, got.dtype)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    g, w = canon(got), canon(want)
    if np.array_equal(g, w):
        return
    idx = np.argwhere(g != w)
    first = tuple(idx[0])
    raise AssertionError("%s: %d of %d values differ bitwise; first at %s: %r vs %r" % (what, len(idx), g.size, first, got[first], want[first]))


def selections(m):
    """The selections of every case: residual only, rotation 0 only, every second rotation plus the residual, everything."""
    return [[-1], [0], list(range(0, m + 1, 2)) + [-1], list(range(m + 1)) + [-1]]


def check_slots(got, select, n_rows, want64, what):
    """got[S, n]: every delivered slot of one signal against the full decomposition's rows want64[n_rows, n]."""
    assert n_rows == want64.shape[0], "%s: n_rows %d, the oracle has %d" % (what, n_rows, want64.shape[0])
    assert got.shape[0] == len(select)
    for k, r in enumerate(select):
        if r == -1:
            assert k == len(select) - 1
            assert_bits(got[k], want64[n_rows - 1], "%s, residual in slot %d" % (what, k))
        elif r <= n_rows - 2:
            assert_bits(got[k], want64[r], "%s, rotation %d in slot %d" % (what, r, k))


def run_sel(eng, x, m, select, rows_dtype=np.float64, x_stride=None, pre=None):
    """x[B, n] (or one signal) through the device entry with `select`.  The result buffer holds exactly B * S * n elements, pre-filled with
    the sentinel, and is followed by a guard region (at least one row) that must come back untouched.  Returns (rows[B, S, n], summary)."""
    x2 = np.atleast_2d(np.ascontiguousarray(x))
    B, n = x2.shape
    S = len(select)
    xs = n if x_stride is None else x_stride
    xin = np.zeros((B, xs), x2.dtype)
    xin[:, :n] = x2
    if xs > n:
        xin[:, n:] = 12345.0
    f32 = np.dtype(rows_dtype) == np.float32
    guard = max(2 * n, 64)
    sent = SENT32 if f32 else SENT64
    buf = np.full(B * S * n + guard, sent, np.uint32 if f32 else np.uint64)
    d = DevArrays(eng, x=xin, rows=buf)
    try:
        eng.decompose_dev(d.ptr("x"), x2.dtype, n, B, xs, m, d.ptr("rows"), None, None, rows_dtype=rows_dtype, select=select)
        if pre is not None:
            pre(d)
        s = eng.summary(B)
        out = d.get("rows")
    finally:
        d.free()
    assert (out[B * S * n:] == sent).all(), "the call wrote behind its result buffer of %d x %d rows (select=%s)" % (B, S, select)
    return out[: B * S * n].view(np.float32 if f32 else np.float64).reshape(B, S, n), s


def run_full(eng, x, m, rows_dtype=np.float64):
    x2 = np.atleast_2d(np.ascontiguousarray(x))
    B, n = x2.shape
    f32 = np.dtype(rows_dtype) == np.float32
    d = DevArrays(eng, x=x2, rows=np.full(B * (m + 2) * n, SENT32 if f32 else SENT64, np.uint32 if f32 else np.uint64))
    try:
        eng.decompose_dev(d.ptr("x"), x2.dtype, n, B, n, m, d.ptr("rows"), None, None, rows_dtype=rows_dtype)
        s = eng.summary(B)
        out = d.get("rows")
    finally:
        d.free()
    return out.view(np.float32 if f32 else np.float64).reshape(B, m + 2, n), s


def same_summary(a, b, what):
    for k in ("n_rows", "stop", "knot_counts", "nan_levels"):
        assert np.array_equal(a[k], b[k]), "%s: %s differs from the full call's" % (what, k)


def every_selection(eng, x, m, want64, what, dtypes=(np.float64, np.float32), sels=None, full_summary=None):
    for sel in (sels or selections(m)):
        for dt in dtypes:
            rows, s = run_sel(eng, x, m, sel, dt)
            w = "%s, select=%s, %s rows" % (what, sel, np.dtype(dt).name)
            check_slots(rows[0], sel, int(s["n_rows"][0]), want64, w)
            if full_summary is not None:
                same_summary(s, full_summary, w)


# ---- 0. the entries refuse a bad selection on a real engine ----------------------------------------------------------------------
def test_rejected_selections(P):
    eng = P.Engine(4096, 2, 0)
    L = eng._L
    x = sines_noise(1000, dtype=np.float64)
    d = DevArrays(eng, x=x, rows=np.full(4 * 1000, SENT64, np.uint64))
    for f, xx in ((L.itd_decompose_select_f64, d.ptr("x")), (L.itd_decompose_select_f32, d.ptr("x"))):
        assert f(eng._h, xx, 1000, 1, 1000, 3, 1 << 4, 1, d.ptr("rows"), 0, None) == INVALID_ARG      # a bit above max_iteration
        assert f(eng._h, xx, 1000, 1, 1000, 3, 1 << 31, 0, d.ptr("rows"), 0, None) == INVALID_ARG
        assert f(eng._h, xx, 1000, 1, 1000, 3, 0, 0, d.ptr("rows"), 0, None) == INVALID_ARG           # S = 0
        assert f(eng._h, xx, 1000, 1, 1000, 3, 1, 2, d.ptr("rows"), 0, None) == INVALID_ARG           # the flag is 0 or 1
        assert f(eng._h, xx, 1000, 1, 1000, 3, 1, 1, d.ptr("rows"), 2, None) == INVALID_ARG           # so is the row type
        assert f(eng._h, xx, 1000, 1, 1000, 3, 1, 1, None, 0, None) == INVALID_ARG
    nr, why = np.zeros(1, np.int32), np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data
    out = np.zeros((4, 1000))
    assert L.itd_decompose_select_host_f64(eng._h, p(x), 1000, 3, 1 << 4, 1, p(out), 0, p(nr), p(why), None) == INVALID_ARG
    assert L.itd_decompose_select_host_f64(eng._h, p(x), 1000, 3, 0, 0, p(out), 0, p(nr), p(why), None) == INVALID_ARG
    assert L.itd_decompose_select_host_f64(eng._h, p(x), 1000, 3, 1, 1, None, 0, p(nr), p(why), None) == INVALID_ARG
    assert (d.get("rows") == SENT64).all() and not out.any()
    # nothing of that has disturbed the engine
    rows, s = run_sel(eng, x, 3, [3, -1])
    assert rows.shape == (1, 2, 1000)
    d.free()
    eng.close()


# ---- 1. every top-level golden: device and host entry, both row types, the four selections ---------------------------------------
@pytest.mark.parametrize("name", golden_cases())
def test_goldens_bit_for_bit(P, oracle, name):
    from pyitd_amd.engine import NAN_INPUT_FOLLOW
    g = load_golden(name)
    x, m = np.asarray(g["x"]), int(g["max_iteration"])
    if "rows" in g.files:
        want = np.asarray(g["rows"], dtype=np.float64)
    else:
        want = oracle.itd(x, m)["rows"]
        assert sha(want) == str(g["rows_sha256"]), "the oracle's rows are not the golden's"
    nr = int(g["n_rows"])
    assert want.shape[0] == nr
    eng = P.Engine(max(len(x), 4096), 1, 0)
    eng.set_nan_input_mode(NAN_INPUT_FOLLOW)
    try:
        full, s_full = run_full(eng, x, m)
        assert_bits(full[0, :nr], want, name + ", full entry")
        for sel in selections(m):
            for dt in (np.float64, np.float32):
                what = "%s, select=%s, %s rows" % (name, sel, np.dtype(dt).name)
                rows, s = run_sel(eng, x, m, sel, dt)
                same_summary(s, s_full, what)
                assert ("natural", "timeout")[int(s["stop"][0])] == str(g["stop"]), what
                check_slots(rows[0], sel, int(s["n_rows"][0]), want, what + ", device entry")
                # the host entry: exactly S rows of a pre-filled array that is longer than that
                out = np.full((len(sel) + 1, len(x)), np.nan, dt)
                sent = canon(out[-1]).copy()
                h = eng.decompose_host(x, m, out=out, rows_dtype=dt, select=sel)
                assert "baselines" not in h and "fetch_baselines" not in h
                assert h["n_rows"] == nr and h["stop"] == int(s["stop"][0]) and np.array_equal(h["knot_counts"], s["knot_counts"][0]), what
                assert h["rows"].shape == (len(sel), len(x)) and h["rows"].dtype == dt
                check_slots(h["rows"], sel, nr, want, what + ", host entry")
                assert np.array_equal(canon(out[-1]), sent), what + ": the host entry wrote behind its S rows"
                for k, r in enumerate(sel):     # the Python wrapper's zero fill of rotations the decomposition did not reach
                    if r != -1 and r > nr - 2:
                        assert not h["rows"][k].any(), what
            if len(sel) == m + 2:           # the full selection against the full entry's own output, slot by slot
                rows, s = run_sel(eng, x, m, sel)
                check_slots(rows[0], sel, nr, full[0, :nr], name + ": full selection against the full entry")
    finally:
        eng.close()


# ---- 2. each form of the engine, pinned ---------------------------------------------------------------------------------------------
def test_resident_form(P, oracle):
    from pyitd_amd.engine import RESIDENT_ONLY
    for n, m, T in ((8192, 7, np.float32), (5000, 20, np.float64), (700, 3, np.float32), (64, 5, np.float64)):
        x = sines_noise(n, seed=n, dtype=T)
        eng = P.Engine(8192, 1, 0)
        eng.set_resident_mode(RESIDENT_ONLY)          # the one-workgroup form or an error: never a silent level-by-level call
        _, s_full = run_full(eng, x, m)
        every_selection(eng, x, m, oracle.itd(x, m)["rows"], "resident n=%d" % n, full_summary=s_full)
        assert eng.resident_repeats == 0 and eng.last_fuse_level == 0
        eng.close()


def test_level_by_level_forced(P, oracle):
    from pyitd_amd.engine import FUSE_OFF, LEVEL0_FUSED, LEVEL0_RECORDS, RESIDENT_OFF, TIME_EXTRACT, TIME_EXTRACT_FINAL, TIME_EXTRACT_L0, TIME_KF_APPLY
    n, m = 200000, 7
    for T, l0 in ((np.float32, LEVEL0_FUSED), (np.float64, LEVEL0_FUSED), (np.float32, LEVEL0_RECORDS), (np.float64, LEVEL0_RECORDS)):
        x = sines_noise(n, seed=3, dtype=T)
        want = oracle.itd(x, m)["rows"]
        eng = P.Engine(n, 1, 0)
        eng.set_fuse_mode(FUSE_OFF)
        eng.set_resident_mode(RESIDENT_OFF)
        eng.set_level0_mode(l0)
        what = "level by level, level-0 mode %d, %s" % (l0, np.dtype(T).name)
        _, s_full = run_full(eng, x, m)
        every_selection(eng, x, m, want, what, full_summary=s_full)
        eng.set_timing(1)
        run_sel(eng, x, m, [1, -1])
        assert eng.last_fuse_level == 0 and eng.fuse_repeats == 0, what
        assert eng.kernel_timing(TIME_KF_APPLY)[1] == 0, what
        assert eng.kernel_timing(TIME_EXTRACT_L0)[1] == 1 and eng.kernel_timing(TIME_EXTRACT)[1] == m and \
            eng.kernel_timing(TIME_EXTRACT_FINAL)[1] == 1, what
        eng.close()


def _fused_engine(P, n, cap, batch=1):
    from pyitd_amd.engine import FUSE_AUTO
    eng = P.Engine(n, batch, 0)
    eng.set_fuse_mode(FUSE_AUTO)
    eng.set_fuse_min_samples(65536)
    eng.set_fuse_level(0)
    eng.set_fuse_cap(cap)
    return eng


def test_fused_levels_on_a_noise_like_signal_of_2_22_samples(P, oracle):
    n, m = 1 << 22, 7
    x = sines_noise(n)
    want = oracle.itd_lean(x, m)["rows"]
    eng = _fused_engine(P, n, -1)
    _, s_full = run_full(eng, x, m)
    assert eng.last_fuse_level >= 2 and eng.fuse_repeats == 0 and eng.last_fuse_cap == 0
    every_selection(eng, x, m, want, "fused sparse levels", full_summary=s_full, sels=selections(m) + [[2, 3, 4, -1], [5], [7]])
    assert eng.last_fuse_level >= 2 and eng.fuse_repeats == 0 and eng.last_fuse_cap == 0
    # the partial form, pinned: levels up to 4 fused, 5 .. m + 1 one launch each behind them
    eng.set_fuse_cap(5)
    every_selection(eng, x, m, want, "fused sparse levels capped at 5", full_summary=s_full, sels=selections(m) + [[4], [5, -1], [3, 6]])
    assert eng.last_fuse_level >= 2 and eng.last_fuse_cap == 5 and eng.fuse_repeats == 0
    eng.close()


def test_fused_levels_refused_then_repeated_into_the_same_slots(P, oracle):
    n, m = 1 << 20, 7
    xc = coarse(sines_noise(n))
    want = oracle.itd_lean(xc, m)["rows"]
    eng = _fused_engine(P, n, -1)
    every_selection(eng, xc, m, want, "refused, then repeated", sels=[[-1], [1, 4, -1]])
    assert eng.fuse_repeats > 0
    eng.close()


def test_capped_form_on_the_periodic_radio_clip(P, oracle):
    """The reference's 8000-sample clip tiled: the first call is refused at one level and repeated; the calls behind it run the levels
    in front of that one fused and the rest level by level (tests/test_gpu_fused.py)."""
    n, m = 1 << 20, 9
    x = np.resize(load_golden("radio8000_input")["x"], n).astype(np.float32)
    want = oracle.itd_lean(x, m)["rows"]
    eng = _fused_engine(P, n, 0)
    every_selection(eng, x, m, want, "radio clip, first call", sels=[[0, 2, 4, 6, 8, -1]], dtypes=(np.float64,))
    assert eng.fuse_repeats == 1
    every_selection(eng, x, m, want, "radio clip, capped calls")
    assert eng.last_fuse_cap >= 0 and eng.last_fuse_cap >= eng.last_fuse_level + 2 and eng.fuse_repeats == 1
    eng.close()


def test_nan_in_the_input_is_followed(P, oracle):
    from pyitd_amd.engine import NAN_INPUT_FOLLOW
    rng = np.random.default_rng(3)
    for n in (5000, 70000):                     # the resident form's own NaN rules, and the NaN-input repeat of the level launches
        x = np.cumsum(rng.standard_normal(n)) * 0.05 + np.sin(np.arange(n) / 11.0)
        for at in (0, 1, 511, 512, 513, 4095, 4096, n // 2, n // 2 + 1, n - 2, n - 1):
            x[at] = np.nan
        m = 6
        want = oracle.itd(x.copy(), m)["rows"]
        eng = P.Engine(n, 1, 0)
        eng.set_nan_input_mode(NAN_INPUT_FOLLOW)
        _, s_full = run_full(eng, x, m)
        assert int(s_full["nan_levels"][0]) == -1
        every_selection(eng, x, m, want, "NaN input, n=%d" % n, full_summary=s_full)
        eng.close()


def test_leading_plateau_nan_golden(P, oracle):
    from pyitd_amd.engine import NAN_INPUT_FOLLOW, RESIDENT_OFF
    for name in ("edge_lead_plateau_nan", "edge_lead_plateau2_nan"):
        g = load_golden(name)
        x, m = np.asarray(g["x"]), int(g["max_iteration"])
        want = np.asarray(g["rows"], dtype=np.float64) if "rows" in g.files else oracle.itd(x, m)["rows"]
        for resident_off in (False, True):
            eng = P.Engine(max(len(x), 4096), 1, 0)
            eng.set_nan_input_mode(NAN_INPUT_FOLLOW)
            if resident_off:
                eng.set_resident_mode(RESIDENT_OFF)
            every_selection(eng, x, m, want, "%s (resident off: %s)" % (name, resident_off))
            eng.close()
    # the same on a signal long enough for the level launches and their NaN rules
    x = sines_noise(150000, seed=5, dtype=np.float64)
    x[:40] = x[40]
    want = oracle.itd(x, 5)["rows"]
    assert np.isnan(want).any() or np.isinf(want).any()
    eng = P.Engine(len(x), 1, 0)
    eng.set_fuse_min_samples(65536)
    every_selection(eng, x, 5, want, "leading plateau, 150000 samples")
    eng.close()


# ---- 3. stops ---------------------------------------------------------------------------------------------------------------------------
def _stopping_signal(n, T=np.float64):
    """Few knots: the decomposition stops naturally long before max_iteration."""
    t = np.arange(n) / n
    return (np.sin(2 * np.pi * 3 * t) + 0.3 * np.sin(2 * np.pi * 17 * t + 0.4)).astype(T)


@pytest.mark.parametrize("n", [3000, 100000, 1 << 20])
def test_natural_stop_in_front_of_selected_rotations(P, oracle, n):
    from pyitd_amd.engine import FUSE_OFF, RESIDENT_OFF
    x, m = _stopping_signal(n), 12
    ref = oracle.itd(x, m)
    want, nr = ref["rows"], ref["rows"].shape[0]
    assert ref["stop"] == "natural" and 3 <= nr <= m - 2, nr
    sels = [[-1], [nr - 2, -1], [nr - 1, -1], [0, nr - 1, nr, m, -1], [nr - 1, nr, m], list(range(m + 1)) + [-1]]
    for lbl in (False, True):
        eng = P.Engine(max(n, 4096), 1, 0)
        eng.set_fuse_min_samples(65536)
        if lbl:
            eng.set_fuse_mode(FUSE_OFF)
            eng.set_resident_mode(RESIDENT_OFF)
        _, s_full = run_full(eng, x, m)
        assert int(s_full["n_rows"][0]) == nr and int(s_full["stop"][0]) == 0
        every_selection(eng, x, m, want, "natural stop at %d rows, n=%d, level by level %s" % (nr, n, lbl), sels=sels, full_summary=s_full)
        eng.close()
    # the Python surface zero-fills the slots of the rotations that do not exist, and x is still the sum of what it returns
    dec = P.ITD()
    rows = dec.itd(x, m, select=list(range(m + 1)) + [-1])
    assert rows.shape == (m + 2, n) and dec.n_rows == nr and dec.stop_reason == "natural"
    assert not rows[nr - 1: m + 1].any()
    assert_bits(rows[: nr - 1], want[: nr - 1], "ITD.itd(select=all), rotations")
    assert_bits(rows[m + 1], want[nr - 1], "ITD.itd(select=all), residual")


def test_stop_at_c0_and_the_timeout_row(P, oracle):
    from pyitd_amd.engine import FUSE_OFF, RESIDENT_OFF
    for n in (2000, 120000):
        for lbl in (False, True):
            eng = P.Engine(max(n, 4096), 1, 0)
            eng.set_fuse_min_samples(65536)
            if lbl:
                eng.set_fuse_mode(FUSE_OFF)
                eng.set_resident_mode(RESIDENT_OFF)
            # constant input: the stop at c = 0, one all-zero row
            x = np.full(n, 2.5)
            want = oracle.itd(x, 5)["rows"]
            assert want.shape[0] == 1 and not want.any()
            for sel in ([-1], [0, -1], [0, 3], [0, 1, 2, 3, 4, 5, -1]):
                for dt in (np.float64, np.float32):
                    rows, s = run_sel(eng, x, 5, sel, dt)
                    assert int(s["n_rows"][0]) == 1 and int(s["stop"][0]) == 0
                    check_slots(rows[0], sel, 1, want, "constant input, select=%s" % sel)
                    if sel[-1] == -1:
                        assert canon(rows[0, -1]).max() == 0, "the residual slot of a stop at c = 0 is all zero (+0.0)"
            # "Out of time!": the residual is (x - b) + b of the last requested level
            x = sines_noise(n, seed=7, dtype=np.float64)
            for m in (0, 1, 4):
                ref = oracle.itd(x, m)
                assert ref["stop"] == "timeout" and ref["rows"].shape[0] == m + 2
                _, s_full = run_full(eng, x, m)
                every_selection(eng, x, m, ref["rows"], "timeout, m=%d n=%d level by level %s" % (m, n, lbl), full_summary=s_full,
                                sels=selections(m) + [[m], [m, -1]])
            eng.close()


# ---- 4. a mixed batch with the device-side repair and valid flags ----------------------------------------------------------------------
def test_mixed_batch_with_the_device_side_repair(P, oracle):
    from pyitd_amd.engine import FUSE_AUTO
    rng = np.random.default_rng(20240607)
    B, m = 32, 7
    n = int(rng.integers(70000, 300000))
    kinds = [b % 7 for b in range(B)]
    x = np.stack([fuzz_signal(rng, k, n) for k in kinds]).astype(np.float32)
    assert np.isfinite(x).all()
    refs = [oracle.itd(x[b], m) for b in range(B)]
    xs = n + 37
    eng = P.Engine(n, B, 0)
    eng.set_fuse_mode(FUSE_AUTO)
    eng.set_fuse_min_samples(65536)
    for sel, dt in (([2, 3, 4, -1], np.float64), ([-1], np.float32), ([0, 5], np.float64)):
        S = len(sel)
        # the host-side repairs of itd_get_summary first
        rows, s = run_sel(eng, x, m, sel, dt, x_stride=xs)
        assert eng.fuse_repeats + eng.fuse_signal_repairs > 0, "the batch was meant to hold signals the fused levels refuse"
        for b in range(B):
            check_slots(rows[b], sel, int(s["n_rows"][b]), refs[b]["rows"], "signal %d (family %d), select=%s" % (b, kinds[b], sel))
            assert ("natural", "timeout")[int(s["stop"][b])] == refs[b]["stop"]
        # the repair on the device: the rows leave by a stream-ordered copy before any summary is read
        valid = DevArrays(eng, valid=np.full(B, -1, np.int32))
        eng.set_valid_flags(valid.ptr("valid"))
        eng.set_device_repair(True)
        taken = {}

        def pre(d):
            taken["rows"] = d.get("rows")
            taken["valid"] = valid.get("valid")
        rows_b, s_b = run_sel(eng, x, m, sel, dt, x_stride=xs, pre=pre)          # (asserts the guard behind the buffer)
        eng.set_device_repair(False)
        eng.set_valid_flags(0)
        valid.free()
        early = taken["rows"][: B * S * n].view(dt).reshape(B, S, n)
        assert (taken["valid"] == 1).all(), "valid flags %s" % taken["valid"].tolist()
        for b in range(B):
            check_slots(early[b], sel, refs[b]["rows"].shape[0], refs[b]["rows"], "device-side repair, signal %d (family %d), select=%s" % (b, kinds[b], sel))
        same_summary(s_b, s, "device-side repair")
    eng.close()


def test_batch_chunks(P, oracle):
    rng = np.random.default_rng(5)
    B, n, m = 7, 90000, 6
    x = np.stack([sines_noise(n, seed=b) if b % 3 else _stopping_signal(n, np.float32) for b in range(B)])
    refs = [oracle.itd(x[b], m)["rows"] for b in range(B)]
    eng = P.Engine(n, B, 0)
    eng.set_fuse_min_samples(65536)
    eng.set_batch_chunk(3)
    for sel in ([-1], [1, 3, 5, -1], [6]):
        rows, s = run_sel(eng, x, m, sel, np.float32 if len(sel) == 1 else np.float64)
        for b in range(B):
            check_slots(rows[b], sel, int(s["n_rows"][b]), refs[b], "chunked batch, signal %d, select=%s" % (b, sel))
    eng.close()


# ---- 5. calls of every kind on one engine ------------------------------------------------------------------------------------------------
def test_interleaved_calls_on_one_engine(P, oracle):
    cases = [(sines_noise(6000, seed=1), 7), (sines_noise(150000, seed=2), 7), (coarse(sines_noise(150000, seed=4)), 5),
             (_stopping_signal(90000), 9)]
    eng = P.Engine(max(len(x) for x, _ in cases), 1, 0)
    eng.set_fuse_min_samples(65536)
    for x, m in cases:
        want = oracle.itd(x, m)["rows"]
        nr = want.shape[0]
        sel = [1, 2, -1]
        full, s0 = run_full(eng, x, m)                                              # full float64
        assert_bits(full[0, :nr], want, "full float64 call")
        r, s = run_sel(eng, x, m, sel, np.float64)                                  # selected float64
        check_slots(r[0], sel, int(s["n_rows"][0]), want, "selected float64 call")
        same_summary(s, s0, "selected float64")
        r, s = run_sel(eng, x, m, sel, np.float32)                                  # selected float32
        check_slots(r[0], sel, int(s["n_rows"][0]), want, "selected float32 call")
        same_summary(s, s0, "selected float32")
        r32, s = run_full(eng, x, m, np.float32)                                    # rows32
        assert_bits(r32[0, :nr], want, "rows32 call behind selected calls")
        same_summary(s, s0, "rows32")
        again, s = run_full(eng, x, m)                                              # full again
        assert_bits(again[0, :nr], want, "full float64 call behind selected calls")
        same_summary(s, s0, "full again")
        h = eng.decompose_host(x, m, want_baselines=True)                            # and the host form with its baselines
        assert_bits(h["rows"], want, "host form behind selected calls")
        assert_bits(h["baselines"], oracle.itd(x, m)["baselines"], "its baselines")
    eng.close()


# ---- 6. the Python surface ---------------------------------------------------------------------------------------------------------------
def test_python_surface(P, torch, oracle):
    x = sines_noise(50000, seed=9)
    ref = oracle.itd(x, 7)
    want = ref["rows"]
    dec = P.ITD()
    rows = dec.itd(x, 7, select=[2, 3, -1])
    assert rows.shape == (3, len(x)) and rows.dtype == np.float64 and dec.n_rows == want.shape[0]
    assert_bits(rows, want[[2, 3, want.shape[0] - 1]], "ITD().itd(select=[2, 3, -1])")
    assert dec.get_rotations() is rows and dec.stop_reason == ref["stop"]
    with pytest.raises(ValueError, match="baselines"):
        dec.get_baselines()
    r32 = dec.itd(x, 7, select=(-1,), out_dtype=np.float32)
    assert r32.shape == (1, len(x)) and r32.dtype == np.float32
    assert_bits(r32[0], want[-1], "select=[-1] with out_dtype=float32")
    buf = np.full((2, len(x)), np.nan)
    r2 = dec.itd(x, 7, out=buf, select=[0, 7])
    assert r2.base is buf or r2 is buf
    assert_bits(r2, want[[0, 7]], "out= with selected rows")
    with pytest.raises(ValueError):
        dec.itd(x, 7, out=np.empty((1, len(x))), select=[0, 7])
    r64 = dec.itd(x, 7)                                     # a full call on the same instance behaves as ever
    assert_bits(r64, want, "full call after selected calls")
    assert_bits(dec.get_baselines(), ref["baselines"], "its baselines")
    # batches: numpy in, numpy out; a torch device tensor in, a device-resident tensor out; a signal that stops early among them
    xb = np.stack([sines_noise(30000, seed=s) for s in range(4)] + [coarse(sines_noise(30000, seed=8)), _stopping_signal(30000, np.float32)])
    m = 9
    refs = [oracle.itd(xb[b], m)["rows"] for b in range(len(xb))]
    assert refs[-1].shape[0] < m
    sel = [0, 4, 8, -1]
    xt = torch.from_numpy(xb).cuda()
    for dt, tdt in ((None, torch.float64), (np.float32, torch.float32)):
        out = P.itd_batch(xb, m, select=sel, out_dtype=dt)
        ot = P.itd_batch(xt, m, select=sel, out_dtype=tdt if dt is not None else None)
        assert out["rows"].shape == (len(xb), 4, 30000) and out["rows"].dtype == (dt or np.float64) and "baselines" not in out
        assert ot["rows"].is_cuda and ot["rows"].dtype == tdt and tuple(ot["rows"].shape) == out["rows"].shape
        for b in range(len(xb)):
            nr = refs[b].shape[0]
            assert int(out["n_rows"][b]) == nr == int(ot["n_rows"][b])
            for got, what in ((out["rows"][b], "itd_batch(numpy)"), (ot["rows"][b].cpu().numpy(), "itd_batch(torch)")):
                check_slots(got, sel, nr, refs[b], "%s, signal %d" % (what, b))
                for k, r in enumerate(sel[:-1]):
                    if r > nr - 2:
                        assert canon(got[k]).max() == 0, "%s, signal %d: slot %d of a rotation that does not exist is not zero" % (what, b, k)
    # x is still the sum of all rotations and the residual
    allsel = list(range(m + 1)) + [-1]
    out = P.itd_batch(xb[-1:].astype(np.float64), m, select=allsel)
    full = P.itd_batch(xb[-1:].astype(np.float64), m)
    nr = int(full["n_rows"][0])
    assert np.array_equal(out["rows"][0].sum(axis=0), np.concatenate([full["rows"][0, :nr - 1], np.zeros((m + 2 - nr, 30000)), full["rows"][0, nr - 1: nr]]).sum(axis=0))
    with pytest.raises(ValueError):
        P.itd_batch(xt, m, select=sel, keep_baselines=True)
