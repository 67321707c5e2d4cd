"""The wave filter's bounds from histogram quantiles without a GPU: tests/wave_bounds_ref.py, the numpy statement of DESIGN.md
section 28, gives the answers worked out by hand, keeps its three invariants on tie-heavy marginals, chooses bounds under which the
reference filter keeps what the quantiles promise, and its windowed form is its range form; the Python surface refuses bad values
before any engine exists, and the library exports the new entries and refuses bad arguments before touching a device."""
import ctypes
import os

import numpy as np
import pytest

import wave_bounds_ref as wb
import wave_hist_ref as wh
import waves_ref
from test_oracle_exact_tfe import FAMILIES, family

ENTRIES = ("itd_bounds_create", "itd_wave_bounds_batch", "itd_bounds_stream_create", "itd_bounds_stream_push", "itd_bounds_stream_push_host")
INF = np.inf


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m, q, want", [
    ([1, 0, 0, 3], (0.25, 0.25), (3, 3)),        # tau = 1: cum = 1 is not above it; the next bin that holds anything is bin 3
    ([1, 0, 0, 3], (1.0, 1.0), (3, 3)),          # nothing above N: the last non-empty bin
    ([1, 0, 0, 3], (0.0, 1.0), (0, 3)),
    ([0, 2, 2, 0], (0.0, 0.0), (1, 1)),          # the empty first bin is skipped; iU = 0 is raised to iL
    ([0, 2, 2, 0], (0.5, 0.5), (2, 2)),          # a tie k / N exactly: the lower half ends in bin 1, the bounds begin behind it
    ([0, 2, 2, 0], (0.0, 1.0), (1, 2)),
    ([0, 0, 0, 0], (0.2, 0.3), (0, 3)),          # an all-zero histogram: the whole edge range
    ([7], (0.3, 0.6), (0, 0)),
    ([0], (0.0, 1.0), (0, 0)),
])
def test_known_indices(m, q, want):
    assert wb.axis_indices(m, *q)[:2] == want


def test_known_bounds_with_scales_and_an_infinite_edge():
    e = np.array([0.5, 1.0, 2.0, 4.0, INF])
    assert wb.axis_bounds([1, 0, 0, 3], e, 0.0, 1.0) == (0.5, INF, 4)
    assert wb.axis_bounds([1, 0, 0, 3], e, 0.25, 0.25) == (4.0, INF, 4)
    assert wb.axis_bounds([0, 2, 2, 0], e, 0.0, 1.0, 1.0, 1.0) == (1.0, 4.0, 4)
    assert wb.axis_bounds([0, 2, 2, 0], e, 0.0, 1.0, 2.5, 2.5) == (2.5, 10.0, 4)
    third = np.array([0.1, 1.0 / 3.0, 0.7])
    lo, hi, _ = wb.axis_bounds([1, 1], third, 0.0, 1.0)                   # a scale of 1.0: the edge's own bits
    assert wb.bits([lo, hi]).tolist() == wb.bits(third[[0, 2]]).tolist()
    lo, hi, _ = wb.axis_bounds([1, 1], third, 0.0, 1.0, 2.5, 2.5)
    assert wb.bits([lo, hi]).tolist() == wb.bits([third[0] * 2.5, third[2] * 2.5]).tolist()
    lo, hi, _ = wb.axis_bounds([1, 0, 0, 3], e, 0.0, 1.0, 1.0, 0.0)        # inf * 0: a NaN bound, with which the filter keeps nothing
    assert lo == 0.5 and np.isnan(hi)
    x = family("noise", 700)
    assert not waves_ref.ref_filter(x, (0.0, hi, 0.0, INF)).any()
    b, N = wb.ref_bounds(np.zeros((3, 4, 2), np.int32), e, [1.0, 2.0, 3.0], (0.2, 0.3, 0.4, 0.5, 1.0, 1.0, 1.0, 1.0))
    assert N == 0 and b.tolist() == [0.5, INF, 1.0, 3.0]


def test_whatever_the_parameters_hold_the_indices_stay_in_range():
    rng = np.random.default_rng(28)
    odd = (np.nan, -1.0, -0.0, 2.0, INF, -INF, 1e308, 0.5)
    for _ in range(400):
        B = int(rng.integers(1, 65))
        m = rng.integers(0, 4, B) * (rng.random(B) < 0.4)
        iL, iU, _ = wb.axis_indices(m, odd[rng.integers(len(odd))], odd[rng.integers(len(odd))])
        assert 0 <= iL <= iU < B


# ---- 2. the invariants ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", range(1, 65))
def test_the_three_invariants_on_tie_heavy_marginals(B):
    rng = np.random.default_rng(2800 + B)
    cases = 0
    for it in range(60):
        big = it % 5 == 4                                                  # cells near 2^31 - 1: sums beyond 2^32
        m = rng.integers(0, 4, B) * (rng.random(B) < 0.4) * (2 ** 31 - 1 if big else 1)
        N = int(m.sum())
        if N == 0:
            assert wb.axis_indices(m, 0.3, 0.4)[:2] == (0, B - 1)
            continue
        k = np.sort(rng.integers(0, N + 1, 2))
        if it % 3 == 0:
            k = np.sort(rng.choice(np.concatenate(([0], np.cumsum(m))), 2))   # exact ties: thresholds ON a prefix sum
        q = k / N
        iL, iU, N2 = wb.axis_indices(m, q[0], q[1])
        cases += 1
        assert N2 == N and 0 <= iL <= iU < B
        assert m[iL] > 0, "the lower bin is empty"
        if not big:                                                        # (k / N * N is k again only while the products are exact)
            assert int(m[iL:iU + 1].sum()) >= k[1] - k[0], (m, q, iL, iU)
    assert cases > 20 or B < 3


# ---- 3. the filter keeps what the quantiles promise -----------------------------------------------------------------------------------
def cover_edges(values, bins):
    """-inf, up to bins - 1 of the values themselves (edges ON values the row has), +inf: every half wave is in a bin"""
    v = np.unique(np.asarray(values, dtype=np.float64))
    v = v[np.isfinite(v)]
    inner = np.unique(v[(np.arange(bins - 1) * max(v.size - 1, 0)) // max(bins - 2, 1)]) if v.size else np.array([])
    return np.concatenate(([-INF], inner, [INF]))


@pytest.mark.parametrize("fam", FAMILIES)
def test_the_reference_filter_keeps_at_least_the_asked_share(fam):
    n = 3 * 512 + 77
    x = family(fam, n)
    start, length, peak, value = waves_ref.ref_table(x)
    A = np.abs(value)
    ae, le = cover_edges(A, 9), cover_edges(length, 7)
    count, samples, outside = wh.ref_hist(x, ae, le)
    assert outside.sum() == 0 and count.sum() == start.size
    wave_of = np.repeat(np.arange(start.size), length)
    for q in ((0.0, 1.0), (0.1, 0.9), (0.25, 0.5), (0.5, 0.5), (0.0, 0.0), (1.0, 1.0), (0.9, 1.0)):
        b, N = wb.ref_bounds(count, ae, le, (q[0], q[1], q[0], q[1], 1.0, 1.0, 1.0, 1.0))
        assert N == start.size
        for axis, bounds, feature in ((0, (b[0], b[1], -INF, INF), A), (1, (-INF, INF, b[2], b[3]), length.astype(np.float64))):
            keep = (bounds[2 * axis] <= feature) & (feature <= bounds[2 * axis + 1])
            assert keep.sum() >= (q[1] - q[0]) * N, (fam, q, axis)
            assert keep.sum() >= 1                                          # bin iL holds a half wave
            out = waves_ref.ref_filter(x, bounds)
            assert np.array_equal(wb.bits(out), wb.bits(np.where(keep[wave_of], x, 0.0))), (fam, q, axis)
        # by samples instead of by half waves: the same rule on the other histogram
        bs, Ns = wb.ref_bounds(samples, ae, le, (q[0], q[1], q[0], q[1], 1.0, 1.0, 1.0, 1.0))
        assert Ns == n
        keep = (bs[2] <= length) & (length <= bs[3])
        assert length[keep].sum() >= (q[1] - q[0]) * n


# ---- 4. the window form is the range form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", (1, 2, 5))
@pytest.mark.parametrize("C", (1, 4))
def test_the_window_form_equals_the_range_form(W, C):
    rng = np.random.default_rng(100 * W + C)
    Na, Nl, pushes = 5, 7, 13
    hist = (rng.integers(0, 5, (pushes * C, Na, Nl)) * (rng.random((pushes * C, Na, Nl)) < 0.3)).astype(np.int32)
    hist[3 * C:4 * C] = 0                                                  # an empty push: with W = 1 an empty window
    hist[7 * C] = 2 ** 31 - 1
    ae, le = np.linspace(0.0, 2.0, Na + 1), np.arange(1.0, Nl + 2)
    st = wb.RefBoundsStream(W)
    for p in range(pushes):
        q = (rng.integers(0, 3) / 4, rng.integers(2, 5) / 4, 0.0, rng.random(), 1.0, 1.5, 0.5, 1.0)
        got, N = st.push(hist[p * C:(p + 1) * C], ae, le, q)
        want, Nw = wb.ref_bounds(hist, ae, le, q, *wb.window_range(p, W, C))
        assert N == Nw and np.array_equal(wb.bits(got), wb.bits(want)), (p, got, want)
    assert wb.window_range(0, W, C) == (0, C) and wb.window_range(9, W, C) == ((10 - W) * C, 10 * C)
    st.reset()
    got, N = st.push(hist[:C], ae, le)
    assert N == int(hist[:C].astype(np.int64).sum())


# ---- 5. the Python surface and the library, without a device ----------------------------------------------------------------------------
def test_the_wrapper_refuses_bad_values_before_any_engine_exists():
    import pyitd_amd
    h = np.zeros((2, 3, 3, 2), np.int32)
    ae, le = [0.0, 1.0, 2.0, 3.0], [1.0, 2.0, 3.0]
    bad = [dict(amplitude_q=(-0.1, 1.0)), dict(amplitude_q=(0.0, 1.5)), dict(length_q=(0.6, 0.4)), dict(length_q=(np.nan, 1.0)),
           dict(amplitude_q=0.5), dict(amplitude_q=([0.1, 0.2, 0.3], 1.0)), dict(amplitude_scale=(np.nan, 1.0)), dict(length_scale=(1.0, np.nan)),
           dict(time_bins=(0, 0)), dict(time_bins=(2, 1)), dict(time_bins=(0, 4)), dict(time_bins=(-1, 2)), dict(time_bins=(0.5, 2)),
           dict(time_bins=3), dict(amplitude_edges=[0.0, 1.0, 1.0, 3.0]), dict(amplitude_edges=[0.0, 1.0, 2.0]),
           dict(length_edges=[1.0, np.nan, 3.0]), dict(length_edges=[1.0, 2.0, 3.0, 4.0]), dict(hist=h.astype(np.int64)),
           dict(hist=h.astype(np.float64)), dict(hist=np.zeros((3, 2), np.int32)), dict(hist=np.zeros((1, 65, 1), np.int32)),
           dict(hist=np.zeros((0, 3, 3, 2), np.int32))]
    for kw in bad:
        a = dict(dict(hist=h, amplitude_edges=ae, length_edges=le), **kw)
        with pytest.raises(ValueError):
            pyitd_amd.wave_filter_bounds(**a)
    from pyitd_amd import streaming
    for kw in (dict(rows=0), dict(rows=65536), dict(Na=0), dict(Na=65), dict(Nl=65), dict(Na=64, Nl=17), dict(slices=0), dict(slices=9),
               dict(window=0), dict(window=65537), dict(window=1.5), dict(rows=True)):
        with pytest.raises(ValueError):
            streaming.WaveBoundsStream(**dict(dict(rows=2, Na=32, Nl=32, slices=8, window=4), **kw))
    assert pyitd_amd.WaveBoundsStream is streaming.WaveBoundsStream and "wave_filter_bounds" in pyitd_amd.__all__
    assert "WaveBoundsStream" in pyitd_amd.__all__


@pytest.fixture(scope="module")
def lib():
    from pyitd_amd import _lib
    _lib.build()
    return _lib.load()


def test_header_abi_table_and_library_agree(lib):
    from pyitd_amd._lib import ABI
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pyitd_hip.h")).read()
    for name in ENTRIES:
        assert name in ABI and hasattr(lib, name), name
        assert "int %s(" % name in header, name
        proto = header[header.index("int %s(" % name):]
        proto = proto[:proto.index(";")]
        assert proto.count(",") + 1 == len(ABI[name][1]), name          # as many parameters as the table's argtypes
    for name, decl in (("itd_bounds_destroy", "void itd_bounds_destroy(itd_bounds *b);"),
                       ("itd_bounds_last_error", "const char *itd_bounds_last_error(const itd_bounds *b);")):
        assert name in ABI and hasattr(lib, name) and decl in header, name
    assert "#define ITD_STREAM_BOUNDS 8" in header and lib.itd_abi_version() == 12


def test_the_entries_refuse_null_and_bad_values_before_touching_a_device(lib):
    buf = ctypes.create_string_buffer(8 * 1024)
    good = dict(e=buf, hist=buf, rows=2, hs=64, T=4, t0=0, t1=4, na=4, nl=4, ae=buf, as_=0, le=buf, ls=0, q=buf, qs=0, b=buf, bs=4)

    def batch(**kw):
        a = dict(good, **kw)
        return lib.itd_wave_bounds_batch(a["e"], a["hist"], a["rows"], a["hs"], a["T"], a["t0"], a["t1"], a["na"], a["nl"], a["ae"], a["as_"],
                                         a["le"], a["ls"], a["q"], a["qs"], a["b"], a["bs"], None, None)
    # (the handle is no handle: every call below must return before it is looked at)
    for kw in (dict(e=None), dict(hist=None), dict(ae=None), dict(le=None), dict(q=None), dict(b=None), dict(rows=0), dict(na=0), dict(na=65),
               dict(nl=0), dict(nl=65), dict(na=64, nl=17, hs=64 * 17 * 4), dict(T=0), dict(t0=-1), dict(t0=2, t1=2), dict(t0=3, t1=2),
               dict(t1=5), dict(hs=63), dict(as_=4), dict(ls=4), dict(qs=7), dict(bs=3), dict(bs=0), dict(T=2 ** 31, hs=2 ** 40)):
        assert batch(**kw) == 1, kw
    assert lib.itd_bounds_create(None, 0) == 1 and lib.itd_bounds_last_error(None) == b"null handle"
    lib.itd_bounds_destroy(None)
    h = ctypes.c_void_p()
    assert lib.itd_bounds_stream_create(None, 0, 1, 4, 4, 1, 1) == 1
    for rows, na, nl, slices, window in ((0, 4, 4, 1, 1), (65536, 4, 4, 1, 1), (1, 0, 4, 1, 1), (1, 65, 1, 1, 1), (1, 4, 65, 1, 1),
                                         (1, 64, 17, 1, 1), (1, 32, 32, 9, 1), (1, 4, 4, 0, 1), (1, 4, 4, 1, 0), (1, 4, 4, 1, 65537)):
        assert lib.itd_bounds_stream_create(ctypes.byref(h), 0, rows, na, nl, slices, window) == 1 and not h.value
    assert lib.itd_bounds_stream_push(None, buf, 16, buf, 0, buf, 0, buf, 0, buf, 4, None, None) == 1
    assert lib.itd_bounds_stream_push_host(None, buf, buf, 0, buf, 0, buf, 0, buf, None) == 1


def test_a_valid_create_without_a_gpu_is_a_loud_failure(lib):
    import torch
    h = ctypes.c_void_p()
    rc = lib.itd_bounds_create(ctypes.byref(h), 0)
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        lib.itd_bounds_destroy(h)
    else:
        assert rc == 2 and not h.value
    for rows, na, nl, slices, window in ((1, 1, 1, 1, 1), (9, 32, 32, 8, 16), (3, 64, 16, 2, 5)):
        rc = lib.itd_bounds_stream_create(ctypes.byref(h), 0, rows, na, nl, slices, window)
        if torch.cuda.is_available():                                     # (with a GPU the same calls make streams)
            assert rc == 0 and h.value
            lib.itd_stream_destroy(h)
        else:
            assert rc == 2 and not h.value                                # ITD_ERR_NO_DEVICE
