"""The wave filter's bounds from histogram quantiles on the GPU (itd_wave_bounds_batch, pyitd_amd.wave_filter_bounds;
itd_wave_bounds.hpp) against wave_bounds_ref, the numpy statement of DESIGN.md section 28.  Every decision is an integer sum and a
comparison and every output a copy of an edge, multiplied once at most: everything is compared exactly, the float64 bits and the totals.

Where the kernels can go wrong: the split of the time range into parts and the ragged last part, time bins abreast where the cells
are fewer than the threads and cells per thread where they are more, sums beyond 2^32, a row's slot of the workspace across the
chunk seam, thresholds exactly on a prefix sum, the lanes beyond the axis's bins, strides and gaps, parameters no wrapper would pass,
the workspace after other calls, a captured call whose inputs change in place.
"""
import numpy as np
import pytest

import wave_bounds_ref as wb
import wave_hist_ref as wh
import waves_ref
from helpers import DevArrays
from test_oracle_exact_tfe import FAMILIES, family

pytestmark = pytest.mark.gpu
ISENT, DSENT, TSENT = -777, -7.77e77, -(2 ** 50)
SHAPES = ((1, 1), (64, 1), (1, 64), (64, 16), (16, 64), (5, 7), (32, 32))
PLAIN = (0.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


@pytest.fixture
def eng(P):
    from pyitd_amd.itd import _engine_for
    return _engine_for(8192)


def handle():
    """the many-row call's handle, the one pyitd_amd.wave_filter_bounds uses: a stream and a workspace of its own"""
    from pyitd_amd.itd import _wave_bounds_for
    return _wave_bounds_for(0)


def settled():
    """the handle's stream is not the engine's, whose copies read the results: wait for the device in between"""
    import torch
    torch.cuda.synchronize()


def synth(rng, kind, R, T, Na, Nl):
    """int32 histograms [R, T, Na, Nl]: random, many zero cells, cells near 2^31 - 1 (a row's sums pass 2^32)"""
    shape = (R, T, Na, Nl)
    if kind == "random":
        h = rng.integers(0, 1000, shape)
    elif kind == "sparse":
        h = rng.integers(1, 4, shape) * (rng.random(shape) < 0.03)
        h[0] = 0                                                           # an empty row: N == 0
    else:
        h = (2 ** 31 - 1 - rng.integers(0, 3, shape)) * (rng.random(shape) < 0.5)
    return h.astype(np.int32)


def edges_for(rng, R, N, per_row):
    e = np.cumsum(0.1 + rng.random((R if per_row else 1, N + 1)), axis=1)
    e[:, -1] = np.where(rng.random(e.shape[0]) < 0.3, np.inf, e[:, -1])
    return e if per_row else e[0]


def quantiles_for(rng, hist, per_row, t0=0, t1=None):
    """eight parameters per row (or one set): q of 0 and 1, equal pairs, exact ties k / N on the rows' own prefix sums, scales"""
    R = hist.shape[0]
    q = np.empty((R, 8))
    for r in range(R):
        ma, ml = wb.marginals(hist[r], t0, t1)
        N = int(ma.sum())
        for a, m in enumerate((ma, ml)):
            mode = (r + a) % 5
            if mode == 0 or N == 0:
                pair = (0.0, 1.0)
            elif mode == 1:
                pair = (1.0, 1.0) if r % 2 else (0.0, 0.0)
            else:
                k = np.sort(rng.choice(np.concatenate(([0], np.cumsum(m))), 2)) if mode < 4 else np.sort(rng.integers(0, N + 1, 2))
                pair = (k[0] / N, k[0 if mode == 2 else 1] / N)
            q[r, 2 * a:2 * a + 2] = pair
        q[r, 4:] = (1.0, 1.0, 1.0, 1.0) if r % 3 else (0.5, 2.5, 1.0, 1.0 / 3.0)
    return q if per_row else q[0]


def run_bounds(eng, hist, ae, le, q, t0=0, t1=None, gap=0, edge_gap=0, bounds_stride=4, want_total=True, stream=None, T=None):
    """itd_wave_bounds_batch on device buffers that hold sentinels; hist [R, T, Na, Nl]; ae / le / q: one set (stride 0) or one per row.
    Returns (bounds [R, 4], totals [R]) after checking that nothing else was written."""
    R, Th, Na, Nl = hist.shape
    T = Th if T is None else T
    slot = Th * Na * Nl
    hs = slot + gap
    hin = np.full((R, hs), ISENT, np.int32)
    hin[:, :slot] = hist.reshape(R, slot)

    def strided(v, gap_):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 1:
            return v, 0
        g = np.full((R, v.shape[1] + gap_), np.nan)
        g[:, :v.shape[1]] = v
        return g, g.shape[1]
    (da, sa), (dl, sl), (dq, sq) = strided(ae, edge_gap), strided(le, edge_gap), strided(q, edge_gap)
    d = DevArrays(eng, hist=hin, ae=da, le=dl, q=dq, b=np.full(R * bounds_stride + 3, DSENT), t=np.full(R + 3, TSENT, np.int64))
    try:
        handle().batch_dev(d.ptr("hist"), R, hs, T, t0, Th if t1 is None else t1, Na, Nl, d.ptr("ae"), sa, d.ptr("le"), sl, d.ptr("q"), sq,
                                  d.ptr("b"), bounds_stride, d.ptr("t") if want_total else None, stream)
        settled()
        b, t = d.get("b"), d.get("t")
        assert np.array_equal(d.get("hist"), hin), "the histogram or a gap behind it was written"
        assert np.array_equal(d.get("ae"), da, equal_nan=True) and np.array_equal(d.get("q"), dq, equal_nan=True)
        body = b[:R * bounds_stride].reshape(R, bounds_stride)
        assert np.all(b[R * bounds_stride:] == DSENT) and np.all(body[:, 4:] == DSENT), "bounds: a gap or the pad was written"
        assert np.all(t[R:] == TSENT) and (want_total or np.all(t == TSENT)), "total: the pad was written"
        return body[:, :4].copy(), t[:R].copy()
    finally:
        d.free()


def same(got, want, what):
    b, n = got
    wbnd, wn = want
    assert np.array_equal(n, wn), "%s: totals %s, expected %s" % (what, n[:8], wn[:8])
    bad = np.flatnonzero((wb.bits(b) != wb.bits(wbnd)).any(axis=1))
    assert bad.size == 0, "%s: %d rows differ, first row %d: %s, expected %s" % (what, bad.size, bad[0], b[bad[0]], wbnd[bad[0]])


# ---- 1. synthetic histograms at every shape ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("random", "sparse", "big"))
@pytest.mark.parametrize("Na, Nl", SHAPES)
def test_synthetic_histograms_against_the_definition(eng, Na, Nl, kind):
    rng = np.random.default_rng(1000 * Na + Nl + len(kind))
    for R, T, per_row in ((1, 1, False), (9, 2, True), (9, 37, False), (1, 37, True)):
        hist = synth(rng, kind, R, T, Na, Nl)
        ae, le = edges_for(rng, R, Na, per_row), edges_for(rng, R, Nl, not per_row)
        q = quantiles_for(rng, hist, True)
        got = run_bounds(eng, hist, ae, le, q, gap=0 if per_row else 5, edge_gap=3, bounds_stride=4 if per_row else 6)
        same(got, wb.ref_bounds_rows(hist, ae, le, q), "%dx%d %s R=%d T=%d" % (Na, Nl, kind, R, T))
        one = quantiles_for(rng, hist, False)                             # one parameter set for every row
        same(run_bounds(eng, hist, ae, le, one, want_total=False)[:1] + (wb.ref_bounds_rows(hist, ae, le, one)[1],),
             wb.ref_bounds_rows(hist, ae, le, one), "%dx%d %s R=%d T=%d, one set" % (Na, Nl, kind, R, T))
    if kind == "big":
        assert wb.ref_bounds_rows(hist, ae, le, q)[1].max() > 2 ** 32 or Na * Nl * T < 4


def test_700_rows_with_their_own_edges_and_parameters(eng):
    rng = np.random.default_rng(700)
    hist = synth(rng, "sparse", 700, 3, 5, 7)
    hist[1::7] = synth(rng, "big", 100, 3, 5, 7)
    ae, le = edges_for(rng, 700, 5, True), edges_for(rng, 700, 7, True)
    q = quantiles_for(rng, hist, True)
    same(run_bounds(eng, hist, ae, le, q, gap=11, edge_gap=1, bounds_stride=5), wb.ref_bounds_rows(hist, ae, le, q), "700 rows")


def test_a_time_range_over_many_parts(eng):
    """32 x 32 bins: a part is 16 time bins, 4099 of them are 257 parts, the last one ragged; 1 x 1 and 5 x 7: time bins abreast"""
    rng = np.random.default_rng(4099)
    for (Na, Nl), T, kind in (((32, 32), 4099, "random"), ((1, 1), 40000, "big"), ((5, 7), 2000, "big"), ((64, 16), 50, "sparse")):
        hist = synth(rng, kind, 2, T, Na, Nl)
        ae, le = edges_for(rng, 2, Na, False), edges_for(rng, 2, Nl, True)
        q = quantiles_for(rng, hist, True)
        same(run_bounds(eng, hist, ae, le, q), wb.ref_bounds_rows(hist, ae, le, q), "%dx%d T=%d" % (Na, Nl, T))
        for t0, t1 in ((1, T), (T // 2, T // 2 + 1), (0, T - 1), (17, 18 + T // 3)):
            q = quantiles_for(rng, hist, True, t0, t1)
            same(run_bounds(eng, hist, ae, le, q, t0, t1), wb.ref_bounds_rows(hist, ae, le, q, t0, t1), "%dx%d T=%d [%d, %d)" % (Na, Nl, T, t0, t1))


def test_sub_ranges_a_single_bin_and_an_empty_sum(eng):
    rng = np.random.default_rng(11)
    hist = synth(rng, "random", 4, 9, 5, 7)
    hist[:, 4] = 0                                                         # the range [4, 5) sums to nothing: the whole edge range
    ae, le = edges_for(rng, 4, 5, True), edges_for(rng, 4, 7, False)
    for t0, t1 in ((0, 9), (0, 1), (8, 9), (4, 5), (3, 6), (2, 9)):
        q = quantiles_for(rng, hist, True, t0, t1)
        got = run_bounds(eng, hist, ae, le, q, t0, t1, gap=2)
        same(got, wb.ref_bounds_rows(hist, ae, le, q, t0, t1), "[%d, %d)" % (t0, t1))
        if (t0, t1) == (4, 5):
            assert not got[1].any()
            assert np.array_equal(wb.bits(got[0][:, 0]), wb.bits(ae[:, 0] * q[:, 4])) and np.array_equal(wb.bits(got[0][:, 3]), wb.bits(le[-1] * q[:, 7]))
    # the histogram is longer than the T the call is told of: only [0, T) exists for it
    same(run_bounds(eng, hist, ae, le, PLAIN, 0, 3, T=3), wb.ref_bounds_rows(hist, ae, le, PLAIN, 0, 3), "T below the slot")


def test_parameters_no_wrapper_would_pass_write_nothing_else(eng):
    rng = np.random.default_rng(5)
    hist = synth(rng, "random", 6, 3, 64, 16)
    ae, le = edges_for(rng, 6, 64, False), edges_for(rng, 6, 16, False)
    odd = np.array([np.nan, -1.0, 2.0, np.inf, -np.inf, 1e308, -0.0, 0.5])
    q = odd[rng.integers(0, 8, (6, 8))]
    q[0, :4] = np.nan
    q[1, :4] = (2.0, -1.0, np.inf, -np.inf)
    same(run_bounds(eng, hist, ae, le, q, bounds_stride=7), wb.ref_bounds_rows(hist, ae, le, q), "odd parameters")


# ---- 2. more rows than one launch takes ------------------------------------------------------------------------------------------------
def test_more_rows_than_one_grid(P):
    R = 65535 + 37
    rng = np.random.default_rng(65)
    base = synth(rng, "sparse", 512, 2, 3, 4)
    idx = np.arange(R) % 512
    ae, le = edges_for(rng, 512, 3, True), edges_for(rng, 512, 4, False)
    q = quantiles_for(rng, base, True)
    want = wb.ref_bounds_rows(base, ae, le, q)
    b, n = P.wave_filter_bounds(base[idx], ae[idx], le, (q[idx, 0], q[idx, 1]), (q[idx, 2], q[idx, 3]), (q[idx, 4], q[idx, 5]),
                                (q[idx, 6], q[idx, 7]), want_total=True)
    assert b.shape == (R, 4) and n.shape == (R,) and n.dtype == np.int64
    same((b, n), (want[0][idx], want[1][idx]), "across the chunk seam")


# ---- 3. real histograms, numpy and tensors, and the filter behind them ---------------------------------------------------------------
@pytest.fixture(scope="module")
def real(P):
    n = 5 * 512 + 77
    rows = np.stack([family(fam, n) for fam in FAMILIES])
    ae = np.concatenate(([0.0], np.geomspace(1e-3, 1e3, 11), [np.inf]))
    le = np.concatenate((np.arange(1.0, 9.0), [16.0, 64.0, np.inf]))
    h = P.wave_histogram(rows, ae, le, hop=512)
    for r, x in enumerate(rows):
        ref = wh.ref_hist(x, ae, le, 512)
        assert np.array_equal(h.count[r], ref[0]) and np.array_equal(h.samples[r], ref[1])
    return rows, ae, le, h


@pytest.mark.parametrize("which", ("count", "samples"))
def test_real_histograms_and_the_filter_behind_them(P, real, which):
    rows, ae, le, h = real
    hist = getattr(h, which)
    R = rows.shape[0]
    aq, lq = (0.1, 0.9), (np.linspace(0.0, 0.5, R), 0.75)
    got = P.wave_filter_bounds(hist, ae, le, aq, lq, length_scale=(1.0, 2.0), want_total=True)
    q = np.stack([np.broadcast_to(np.float64(v), (R,)) for v in (aq[0], aq[1], lq[0], lq[1], 1.0, 1.0, 1.0, 2.0)], axis=1)
    want = wb.ref_bounds_rows(hist, ae, le, q)
    same(got, want, which)
    assert np.array_equal(got[1], hist.astype(np.int64).sum(axis=(1, 2, 3)))
    out = P.wave_filter(rows, amplitude=(got[0][:, 0], got[0][:, 1]), length=(got[0][:, 2], got[0][:, 3]))
    for r, x in enumerate(rows):
        assert np.array_equal(wb.bits(out[r]), wb.bits(waves_ref.ref_filter(x, want[0][r]))), "%s: filtered row %d" % (which, r)
    part = P.wave_filter_bounds(hist, ae, le, aq, time_bins=(2, 5))
    same((part, want[1]), (wb.ref_bounds_rows(hist, ae, le, np.array((0.1, 0.9) + PLAIN[2:]), 2, 5)[0], want[1]), "%s, time bins 2 .. 4" % which)
    one = P.wave_filter_bounds(hist[3], ae, le, (0.25, 0.5))               # one row, no leading axis
    assert one.shape == (4,) and np.array_equal(wb.bits(one), wb.bits(wb.ref_bounds(hist[3], ae, le, (0.25, 0.5) + PLAIN[2:])[0]))


def test_tensors_in_place_feed_the_filter_on_the_device(P, real, eng):
    import torch
    rows, ae, le, _ = real
    R, n = rows.shape
    t = torch.from_numpy(rows).cuda()
    h = P.wave_histogram(t.reshape(2, R // 2, n) if R % 2 == 0 else t, ae, le, hop=512)
    lead = tuple(h.count.shape[:-3])
    aq = (torch.linspace(0.0, 0.4, R).reshape(lead).numpy(), 0.8)
    b, N = P.wave_filter_bounds(h.samples, ae, le, aq, (0.05, 0.95), want_total=True)
    assert b.device == t.device and b.dtype == torch.float64 and tuple(b.shape) == lead + (4,) and N.dtype == torch.int64
    hist = h.samples.cpu().numpy().reshape((R,) + tuple(h.samples.shape[-3:]))
    q = np.stack([np.broadcast_to(np.float64(v), (R,)) for v in (aq[0].reshape(-1), 0.8, 0.05, 0.95, 1.0, 1.0, 1.0, 1.0)], axis=1)
    want = wb.ref_bounds_rows(hist, ae, le, q)
    same((b.cpu().numpy().reshape(R, 4), N.cpu().numpy().reshape(R)), want, "tensors")
    out = torch.empty_like(t)
    torch.cuda.synchronize()
    eng.wave_filter_batch_dev(t.data_ptr(), np.float64, n, R, n, b.data_ptr(), 4, out.data_ptr(), n)       # the bounds where they lie
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for r, x in enumerate(rows):
        assert np.array_equal(wb.bits(got[r]), wb.bits(waves_ref.ref_filter(x, want[0][r]))), "filtered row %d" % r
    view = h.count[..., 1:4, :, :]                                         # dense cells, a row stride beyond the slot
    part = P.wave_filter_bounds(view, ae, le, (0.2, 0.6))
    cnt = h.count.cpu().numpy().reshape((R,) + tuple(h.count.shape[-3:]))
    wantv = wb.ref_bounds_rows(cnt[:, 1:4], ae, le, np.array((0.2, 0.6) + PLAIN[2:]))
    assert np.array_equal(wb.bits(part.cpu().numpy().reshape(R, 4)), wb.bits(wantv[0]))
    for bad in (h.count[..., ::2], h.count.float(), h.count.cpu()):
        with pytest.raises(ValueError):
            P.wave_filter_bounds(bad, ae, le)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_the_entry_refuses_bad_arguments_before_any_launch(P, eng):
    hist = synth(np.random.default_rng(3), "random", 2, 4, 4, 4)
    d = DevArrays(eng, h=hist, e=np.arange(8.0), q=np.array(PLAIN), b=np.full(12, DSENT))
    good = dict(rows=2, hs=64, T=4, t0=0, t1=4, na=4, nl=4, ae=d.ptr("e"), sa=0, le=d.ptr("e"), sl=0, q=d.ptr("q"), sq=0, b=d.ptr("b"), sb=4)
    try:
        for kw in (dict(na=0), dict(na=65), dict(nl=65), dict(na=64, nl=17), dict(T=0), dict(t0=-1), dict(t0=4), dict(t0=2, t1=2), dict(t1=5),
                   dict(hs=63), dict(sa=4), dict(sl=3), dict(sq=7), dict(sb=3), dict(ae=None), dict(le=None), dict(q=None), dict(b=None),
                   dict(rows=0)):
            a = dict(good, **kw)
            with pytest.raises(P.ITDError):
                handle().batch_dev(d.ptr("h"), a["rows"], a["hs"], a["T"], a["t0"], a["t1"], a["na"], a["nl"], a["ae"], a["sa"], a["le"],
                                          a["sl"], a["q"], a["sq"], a["b"], a["sb"])
        with pytest.raises(P.ITDError):
            handle().batch_dev(None, 2, 64, 4, 0, 4, 4, 4, d.ptr("e"), 0, d.ptr("e"), 0, d.ptr("q"), 0, d.ptr("b"), 4)
        assert np.all(d.get("b") == DSENT)
    finally:
        d.free()


# ---- 5. a captured call follows the parameters and the histogram ----------------------------------------------------------------------
def test_on_a_callers_stream_and_in_a_graph(P, eng):
    import torch
    rng = np.random.default_rng(8)
    R, T, Na, Nl = 5, 40, 32, 32
    hist = synth(rng, "random", R, T, Na, Nl)
    ae, le, q = edges_for(rng, R, Na, True), edges_for(rng, R, Nl, False), quantiles_for(rng, hist, True, 3, 37)
    d = DevArrays(eng, h=hist, ae=ae, le=le, q=q, b=np.full((R, 4), DSENT), t=np.full(R, TSENT, np.int64))

    def enqueue(stream):
        handle().batch_dev(d.ptr("h"), R, T * Na * Nl, T, 3, 37, Na, Nl, d.ptr("ae"), Na + 1, d.ptr("le"), 0, d.ptr("q"), 8, d.ptr("b"), 4,
                                  d.ptr("t"), stream)
    s = torch.cuda.Stream()
    enqueue(s.cuda_stream)
    s.synchronize()
    same((d.get("b"), d.get("t")), wb.ref_bounds_rows(hist, ae, le, q, 3, 37), "on the caller's stream")
    # (the call above was the warm-up of this size: the workspace exists, the capture allocates nothing)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            enqueue(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for kind in ("sparse", "big", "random"):
        hist = synth(rng, kind, R, T, Na, Nl)
        ae, q = edges_for(rng, R, Na, True), quantiles_for(rng, hist, True, 3, 37)
        d.put("h", hist)                           # histogram, edges and parameters changed in place: the replay follows them
        d.put("ae", ae)
        d.put("q", q)
        g.replay()
        torch.cuda.synchronize()
        same((d.get("b"), d.get("t")), wb.ref_bounds_rows(hist, ae, le, q, 3, 37), "replayed, %s" % kind)
    d.free()


# ---- 6. whatever the engine ran before ---------------------------------------------------------------------------------------------------
def test_the_same_bits_as_a_fresh_engine_between_other_calls_and_in_any_batch_position(P, real):
    rows, ae, le, h = real
    args = (h.count, ae, le, (0.2, 0.7), (0.1, 1.0))
    P.release_engines()
    fresh = P.wave_filter_bounds(*args, want_total=True)
    P.wave_histogram(rows, ae, le, hop=1024)                               # behind a wave_histogram call ...
    behind = P.wave_filter_bounds(*args, want_total=True)
    out = P.wave_filter(rows, amplitude=(behind[0][:, 0], behind[0][:, 1]), length=(behind[0][:, 2], behind[0][:, 3]))
    again = P.wave_filter_bounds(*args, want_total=True)                   # ... and behind the wave_filter call it fed
    for got in (behind, again):
        assert got[0].tobytes() == fresh[0].tobytes() and got[1].tobytes() == fresh[1].tobytes()
    fed = P.wave_filter(rows, amplitude=(fresh[0][:, 0], fresh[0][:, 1]), length=(fresh[0][:, 2], fresh[0][:, 3]))
    assert out.tobytes() == fed.tobytes()
    moved = P.wave_filter_bounds(np.concatenate((h.count[1:], h.count[:1])), ae, le, (0.2, 0.7), (0.1, 1.0))
    assert moved[-1].tobytes() == fresh[0][0].tobytes() and moved[:-1].tobytes() == fresh[0][1:].tobytes()
