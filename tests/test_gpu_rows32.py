"""float32 result rows (itd_decompose_rows32_*, out_dtype=float32): every element of a delivered row is the float64 entry's element
converted to float32, so the expected value of every case is the oracle's (or the golden's) float64 rows through numpy's astype, and the
comparison is on bit patterns (any NaN equal to any NaN).  The summary must be the float64 call's."""
import numpy as np
import pytest

from conftest import golden_cases
from helpers import DevArrays, coarse, fuzz_signal, load_golden, sha, sines_noise

pytestmark = pytest.mark.gpu

SENT32 = np.uint32(0x7FC5A5A5)      # a NaN no computation produces: the pre-fill of the float32 result buffers and of what lies behind them
SENT64 = np.uint64(0x7FF85A5A5A5A5A5A)


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


def to32(rows64):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(rows64, dtype=np.float64).astype(np.float32)


def canon32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def assert_bits32(got, want, what):
    assert got.dtype == np.float32, what
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    g, w = canon32(got), canon32(want)
    if np.array_equal(g, w):
        return
    idx = np.argwhere(g != w)
    first = tuple(idx[0])
    raise AssertionError("%s: %d of %d values differ bitwise; first at %s: %r vs %r" % (what, len(idx), g.size, first, got[first], want[first]))


def assert_bits64(got, want, what):
    g, w = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert g.shape == w.shape, what
    ok = (g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))
    assert ok.all(), "%s: %d float64 values differ" % (what, int((~ok).sum()))


def run_dev(eng, x, m, rows_dtype, x_stride=None, guard=None, pre=None, summary=True):
    """x[B, n] (or one signal) through the device entry of `rows_dtype`.  The result buffer is pre-filled with the sentinel and followed
    by a guard region of `guard` elements (at least one row) that must come back untouched.  Returns (rows[B, R, n], summary)."""
    x2 = np.atleast_2d(np.ascontiguousarray(x))
    B, n = x2.shape
    R = m + 2
    xs = n if x_stride is None else x_stride
    xin = np.zeros((B, xs), x2.dtype)
    xin[:, :n] = x2
    if xs > n:
        xin[:, n:] = 12345.0           # what lies between the signals is not part of them
    f32 = np.dtype(rows_dtype) == np.float32
    guard = max(n, 64) if guard is None else guard
    sent = SENT32 if f32 else SENT64
    buf = np.full(B * R * n + guard, sent, np.uint32 if f32 else np.uint64)
    d = DevArrays(eng, x=xin, rows=buf)
    try:
        eng.decompose_dev(d.ptr("x"), x2.dtype, n, B, xs, m, d.ptr("rows"), None, None, rows_dtype=rows_dtype)
        if pre is not None:
            pre(d)
        s = eng.summary(B) if summary else None
        out = d.get("rows")
    finally:
        d.free()
    assert (out[B * R * n:] == sent).all(), "the call wrote behind its %s result buffer" % np.dtype(rows_dtype).name
    return out[: B * R * n].view(np.float32 if f32 else np.float64).reshape(B, R, n), s


def same_summary(s32, s64, what):
    for k in ("n_rows", "stop", "knot_counts", "nan_levels"):
        assert np.array_equal(s32[k], s64[k]), "%s: %s differs between the float32 and the float64 call" % (what, k)


def check_against(rows32, s32, b, want64, what):
    nr = int(s32["n_rows"][b])
    assert nr == want64.shape[0], "%s: %d rows, expected %d" % (what, nr, want64.shape[0])
    assert_bits32(rows32[b, :nr], to32(want64), what)


# ---- 1. every top-level golden, device and host entry, both input types where the values allow -----------------------------------
def _input_types(x):
    x = np.asarray(x)
    types = [x.dtype.type]
    other = np.float64 if x.dtype == np.float32 else np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        y = x.astype(other)
    if np.array_equal(y.astype(np.float64), x.astype(np.float64), equal_nan=True):       # the same values in the other type
        types.append(other)
    return types


@pytest.mark.parametrize("name", golden_cases())
def test_goldens_bit_for_bit(P, oracle, name):
    from pyitd_amd.engine import NAN_INPUT_FOLLOW
    g = load_golden(name)
    x0, m = np.asarray(g["x"]), int(g["max_iteration"])
    if "rows" in g.files:
        want = np.asarray(g["rows"], dtype=np.float64)
    else:
        want = oracle.itd(x0, m)["rows"]
        assert sha(want) == str(g["rows_sha256"]), "the oracle's rows are not the golden's"
    assert want.shape[0] == int(g["n_rows"])
    eng = P.Engine(max(len(x0), 4096), 1, 0)
    eng.set_nan_input_mode(NAN_INPUT_FOLLOW)
    try:
        for T in _input_types(x0):
            x = x0.astype(T)
            what = "%s (%s input)" % (name, np.dtype(T).name)
            rows64, s64 = run_dev(eng, x, m, np.float64)
            rows32, s32 = run_dev(eng, x, m, np.float32)
            same_summary(s32, s64, what)
            assert ("natural", "timeout")[int(s32["stop"][0])] == str(g["stop"]), what
            check_against(rows32, s32, 0, want, what + ", device entry")
            assert_bits64(rows64[0, : want.shape[0]], want, what + ", float64 device entry")
            h64 = eng.decompose_host(x, m, want_baselines=False)
            h32 = eng.decompose_host(x, m, rows_dtype=np.float32)
            assert "baselines" not in h32 and "fetch_baselines" not in h32
            assert h32["stop"] == h64["stop"] and np.array_equal(h32["knot_counts"], h64["knot_counts"]), what
            assert h32["rows"].shape[0] == int(g["n_rows"])
            assert_bits32(h32["rows"], to32(want), what + ", host entry")
    finally:
        eng.close()


# ---- 2. every form of the engine, and the proof that it was the form that ran ----------------------------------------------------
def _both(eng, x, m, what, oracle_rows):
    rows32, s32 = run_dev(eng, x, m, np.float32)
    check_against(rows32, s32, 0, oracle_rows, what)
    return s32


def test_resident_form(P, oracle):
    from pyitd_amd.engine import RESIDENT_ONLY
    for n, m, T in ((8192, 7, np.float32), (5000, 20, np.float64), (700, 3, np.float32)):
        x = sines_noise(n, seed=n, dtype=T)
        eng = P.Engine(8192, 1, 0)
        eng.set_resident_mode(RESIDENT_ONLY)          # the one-workgroup form or an error: never a silent level-by-level call
        s32 = _both(eng, x, m, "resident n=%d" % n, oracle.itd(x, m)["rows"])
        assert eng.resident_repeats == 0 and eng.last_fuse_level == 0
        _, s64 = run_dev(eng, x, m, np.float64)
        same_summary(s32, s64, "resident n=%d" % n)
        eng.close()


def test_level_by_level_and_record_driven_level0(P, oracle):
    from pyitd_amd.engine import (FUSE_OFF, LEVEL0_FUSED, LEVEL0_RECORDS, RESIDENT_OFF, TIME_EXTRACT, TIME_EXTRACT_FINAL,
                                  TIME_EXTRACT_L0, TIME_KF_APPLY, TIME_SCAN0)
    n, m = 200000, 7
    for T in (np.float32, np.float64):
        x = sines_noise(n, seed=3, dtype=T)
        want = oracle.itd(x, m)["rows"]
        for l0 in (LEVEL0_FUSED, LEVEL0_RECORDS):
            eng = P.Engine(n, 1, 0)
            eng.set_fuse_mode(FUSE_OFF)
            eng.set_resident_mode(RESIDENT_OFF)
            eng.set_level0_mode(l0)
            eng.set_timing(1)
            what = "level by level, level-0 mode %d, %s" % (l0, np.dtype(T).name)
            _both(eng, x, m, what, want)
            assert eng.last_fuse_level == 0 and eng.fuse_repeats == 0, what
            assert eng.kernel_timing(TIME_KF_APPLY)[1] == 0, what
            assert eng.kernel_timing(TIME_EXTRACT_L0)[1] == 1 and eng.kernel_timing(TIME_EXTRACT)[1] == m and \
                eng.kernel_timing(TIME_EXTRACT_FINAL)[1] == 1, what
            assert eng.kernel_timing(TIME_SCAN0)[1] == (1 if l0 == LEVEL0_RECORDS else 0), what     # the record-driven level 0 scans first
            eng.close()


def _fused_engine(P, n, cap):
    from pyitd_amd.engine import FUSE_AUTO
    eng = P.Engine(n, 1, 0)
    eng.set_fuse_mode(FUSE_AUTO)
    eng.set_fuse_min_samples(65536)
    eng.set_fuse_level(0)
    eng.set_fuse_cap(cap)
    return eng


def test_fused_sparse_levels_delivered_refused_and_capped(P, oracle):
    n, m = 1 << 20, 7
    x = sines_noise(n)
    want = oracle.itd_lean(x, m)["rows"]
    eng = _fused_engine(P, n, -1)
    s32 = _both(eng, x, m, "fused sparse levels", want)
    assert eng.last_fuse_level >= 2 and eng.fuse_repeats == 0 and eng.last_fuse_cap == 0
    _, s64 = run_dev(eng, x, m, np.float64)
    same_summary(s32, s64, "fused sparse levels")
    # the partial form, pinned: levels up to 4 fused, 5 .. m + 1 one launch each behind them
    eng.set_fuse_cap(5)
    _both(eng, x, m, "fused sparse levels capped at 5", want)
    assert eng.last_fuse_level >= 2 and eng.last_fuse_cap == 5 and eng.fuse_repeats == 0
    eng.close()
    # refused (ties everywhere), then repeated level by level into the same float32 buffer
    xc = coarse(x)
    eng = _fused_engine(P, n, -1)
    _both(eng, xc, m, "refused, then repeated", oracle.itd_lean(xc, m)["rows"])
    assert eng.fuse_repeats > 0             # (the repeat ran level by level: that is the form the getters name afterwards)
    eng.close()


def test_capped_form_on_the_periodic_radio_clip(P, oracle):
    """Configuration 5's substitute: the reference's 8000-sample clip tiled.  The first call is refused at one level and repeated; the
    second runs the levels in front of that one fused and the rest level by level (tests/test_gpu_fused.py)."""
    n, m = 1 << 20, 9
    x = np.resize(load_golden("radio8000_input")["x"], n).astype(np.float32)
    want = oracle.itd_lean(x, m)["rows"]
    eng = _fused_engine(P, n, 0)
    _both(eng, x, m, "radio clip, first call", want)
    assert eng.fuse_repeats == 1
    _both(eng, x, m, "radio clip, second call", want)
    assert eng.last_fuse_cap >= 0 and eng.last_fuse_cap >= eng.last_fuse_level + 2 and eng.fuse_repeats == 1
    eng.close()


# ---- 3. a batch that mixes signals the fused levels deliver with signals they refuse ------------------------------------------------
def test_batch_of_64_with_repairs_and_the_device_side_repair(P, oracle):
    from pyitd_amd.engine import FUSE_AUTO
    rng = np.random.default_rng(20240607)
    B, m = 64, 7
    n = int(rng.integers(70000, 400000))
    kinds = [b % 7 for b in range(B)]
    x = np.stack([fuzz_signal(rng, k, n) for k in kinds]).astype(np.float32)
    assert np.isfinite(x).all()
    refs = [oracle.itd(x[b], m) for b in range(B)]
    xs = n + 37
    eng = P.Engine(n, B, 0)
    eng.set_fuse_mode(FUSE_AUTO)
    eng.set_fuse_min_samples(65536)
    rows32, s32 = run_dev(eng, x, m, np.float32, x_stride=xs)
    refused = eng.fuse_repeats + eng.fuse_signal_repairs
    assert refused > 0, "the batch was meant to hold signals the fused levels refuse"
    for b in range(B):
        check_against(rows32, s32, b, refs[b]["rows"], "signal %d (family %d)" % (b, kinds[b]))
        assert ("natural", "timeout")[int(s32["stop"][b])] == refs[b]["stop"]
    _, s64 = run_dev(eng, x, m, np.float64, x_stride=xs)
    same_summary(s32, s64, "batch")
    # once more with the repair on the device: the rows leave by a stream-ordered copy before any summary is read
    valid = DevArrays(eng, valid=np.full(B, -1, np.int32))
    eng.set_valid_flags(valid.ptr("valid"))
    eng.set_device_repair(True)
    taken = {}

    def pre(d):
        taken["rows"] = d.get("rows")              # itd_copy on the engine's stream, waited for: no summary has been read yet
        taken["valid"] = valid.get("valid")
    rows_b, s_b = run_dev(eng, x, m, np.float32, x_stride=xs, pre=pre)
    eng.set_device_repair(False)
    eng.set_valid_flags(0)
    valid.free()
    R = m + 2
    early = taken["rows"][: B * R * n].view(np.float32).reshape(B, R, n)
    assert (taken["valid"] == 1).all(), "valid flags %s" % taken["valid"].tolist()
    for b in range(B):
        nr = refs[b]["rows"].shape[0]
        assert_bits32(early[b, :nr], to32(refs[b]["rows"]), "device-side repair, signal %d (family %d)" % (b, kinds[b]))
    same_summary(s_b, s32, "device-side repair")
    eng.close()


# ---- 4. shapes: a store sized for float64 would run past the float32 buffer ---------------------------------------------------------
@pytest.mark.parametrize("n", [3, 5, 511, 513, 8191, 8193, 65537, (1 << 20) + 3])
def test_shapes_and_what_lies_behind_the_buffer(P, oracle, n):
    rng = np.random.default_rng(n)
    eng = P.Engine(max(n, 4096), 1, 0)
    for m in (0, 1, 7, 20):
        for T in (np.float32, np.float64):
            x = (np.sin(np.arange(n) * 0.37) + 0.3 * rng.standard_normal(n)).astype(T)
            want = oracle.itd(x, m)["rows"]
            rows32, s32 = run_dev(eng, x, m, np.float32)            # (asserts the guard region behind the buffer itself)
            check_against(rows32, s32, 0, want, "n=%d m=%d %s" % (n, m, np.dtype(T).name))
            h = eng.decompose_host(x, m, rows_dtype=np.float32)
            assert_bits32(h["rows"], to32(want), "n=%d m=%d %s host" % (n, m, np.dtype(T).name))
    eng.close()


# ---- 5. range: float32 subnormals and overflow to +-inf must be numpy's ---------------------------------------------------------------
def test_subnormal_and_overflowing_values_convert_like_numpy(P, oracle):
    cases = []
    for name in ("edge_denormal", "edge_large"):
        g = load_golden(name)
        cases.append((name, np.asarray(g["x"]), int(g["max_iteration"])))
    rng = np.random.default_rng(77)
    for k in range(12):
        x = fuzz_signal(rng, 7, int(rng.integers(100, 120000)))
        if np.isfinite(x).all():
            cases.append(("extreme magnitudes %d" % k, x, 5))
    # magnitudes placed on purpose around float32's limits: subnormal results, and results beyond 3.4e38
    base = rng.standard_normal(30000)
    for k, sc in enumerate((1e-39, 3e-42, 1e-45, 7e-46, 1e38, 3e38, 1e39)):
        cases.append(("scaled %g" % sc, base * sc, 5))
    sub = over = 0
    for name, x, m in cases:
        want = oracle.itd(x, m)["rows"]
        w32 = to32(want)
        tiny = np.finfo(np.float32).tiny
        sub += int(((np.abs(w32) < tiny) & (w32 != 0)).sum())
        over += int((np.isinf(w32) & np.isfinite(want)).sum())
        for n_max in (len(x),):
            eng = P.Engine(max(n_max, 4096), 1, 0)
            rows32, s32 = run_dev(eng, x, m, np.float32)
            check_against(rows32, s32, 0, want, name)
            h = eng.decompose_host(x, m, rows_dtype=np.float32)
            assert_bits32(h["rows"], w32, name + " host")
            eng.close()
    assert sub > 0 and over > 0, "the cases were meant to produce float32 subnormals (%d) and overflows (%d)" % (sub, over)


# ---- 6. both row types on one engine, in both orders -----------------------------------------------------------------------------------
def test_interleaved_row_types_on_one_engine(P, oracle):
    cases = [(sines_noise(6000, seed=1), 7), (sines_noise(150000, seed=2), 7), (coarse(sines_noise(150000, seed=4)), 5),
             (sines_noise(90000, seed=3, dtype=np.float64), 9)]
    n_max = max(len(x) for x, _ in cases)
    mixed, clean = P.Engine(n_max, 1, 0), P.Engine(n_max, 1, 0)
    for e in (mixed, clean):
        e.set_fuse_min_samples(65536)
    for order in (("f32", "f64"), ("f64", "f32"), ("f32", "f32", "f64", "f64", "f32")):
        for x, m in cases:
            want = oracle.itd(x, m)["rows"]
            r_clean, s_clean = run_dev(clean, x, m, np.float64)
            for kind in order:
                if kind == "f32":
                    rows, s = run_dev(mixed, x, m, np.float32)
                    check_against(rows, s, 0, want, "interleaved float32 call")
                else:
                    rows, s = run_dev(mixed, x, m, np.float64)
                    nr = int(s["n_rows"][0])
                    assert_bits64(rows[0, :nr], want, "interleaved float64 call")
                    assert_bits64(rows[0, :nr], r_clean[0, :nr], "float64 rows of an engine that saw float32 calls")
                same_summary(s, s_clean, "interleaved")
    mixed.close()
    clean.close()


# ---- 7. the Python surface ---------------------------------------------------------------------------------------------------------------
def test_python_round_trips(P, torch, oracle):
    x = sines_noise(50000, seed=9)
    ref = oracle.itd(x, 7)
    want = to32(ref["rows"])
    dec = P.ITD()
    rows = dec.itd(x, 7, out_dtype=np.float32)
    assert_bits32(rows, want, "ITD().itd(out_dtype=float32)")
    assert dec.get_rotations() is rows and dec.get_rotations().dtype == np.float32
    assert dec.stop_reason == ref["stop"]
    with pytest.raises(ValueError, match="baselines"):
        dec.get_baselines()
    buf = np.full((9, len(x)), np.nan, np.float32)
    r2 = dec.itd(x, 7, out=buf, out_dtype=np.float32)
    assert r2.base is buf or r2 is buf
    assert_bits32(r2, want, "out= with a float32 array")
    with pytest.raises(ValueError):
        dec.itd(x, 7, out=np.empty((9, len(x)), np.float64), out_dtype=np.float32)
    with pytest.raises(ValueError):
        dec.itd(x, 7, out=buf)                                  # a float32 array for float64 rows
    with pytest.raises(ValueError):
        dec.get_baselines()
    # a float64 call on the same instance behaves as ever
    r64 = dec.itd(x, 7)
    assert r64.dtype == np.float64
    assert_bits64(r64, ref["rows"], "float64 call after float32 calls")
    assert_bits64(dec.get_baselines(), ref["baselines"], "its baselines")
    # batches: numpy in, numpy out; a torch device tensor in, a device-resident float32 tensor out
    xb = np.stack([sines_noise(30000, seed=s) for s in range(5)] + [coarse(sines_noise(30000, seed=8))])
    refs = [oracle.itd(xb[b], 5) for b in range(len(xb))]
    out = P.itd_batch(xb, 5, out_dtype=np.float32)
    assert out["rows"].dtype == np.float32 and "baselines" not in out
    out64 = P.itd_batch(xb, 5)
    assert out64["rows"].dtype == np.float64
    xt = torch.from_numpy(xb).cuda()
    for dt in (torch.float32, np.float32):
        ot = P.itd_batch(xt, 5, out_dtype=dt)
        assert ot["rows"].is_cuda and ot["rows"].dtype == torch.float32
        for b in range(len(xb)):
            nr = int(ot["n_rows"][b])
            assert nr == refs[b]["rows"].shape[0] == int(out["n_rows"][b]) == int(out64["n_rows"][b])
            assert_bits32(ot["rows"][b, :nr].cpu().numpy(), to32(refs[b]["rows"]), "itd_batch(torch), signal %d" % b)
            assert_bits32(out["rows"][b, :nr], to32(refs[b]["rows"]), "itd_batch(numpy), signal %d" % b)
            assert_bits64(out64["rows"][b, :nr], refs[b]["rows"], "itd_batch float64, signal %d" % b)
    with pytest.raises(ValueError):
        P.itd_batch(xt, 5, out_dtype=torch.float16)
