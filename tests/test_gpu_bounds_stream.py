"""The bounds stream on the GPU (itd_bounds_stream_*, streaming.WaveBoundsStream; k_bounds_stream in itd_wave_bounds.hpp): after
every push the bounds of the last min(W, pushes) pushes are, bit for bit, wave_bounds_ref's statement and the many-row call over the
concatenated slices with [t0, t1) = [max(0, p + 1 - W) C, (p + 1) C).

Where it can go wrong: the ring slot and what it replaces once the window is full, a window of one push, the running sums across a
reset (state that is not read in a stream's first push), sums beyond 2^32 that leave the window again, strides, the host form's
staging, the other kinds' entries, and the chain LevelsStream -> WaveHistogramStream -> WaveBoundsStream -> WaveFilterStream on one
HIP stream through device pointers.
"""
import ctypes

import numpy as np
import pytest

import wave_bounds_ref as wb
from helpers import DevArrays

pytestmark = pytest.mark.gpu
DSENT, TSENT, ISENT = -7.77e77, -(2 ** 50), -777


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


@pytest.fixture
def eng(P):
    from pyitd_amd.itd import _engine_for
    return _engine_for(8192)


def slices_for(rng, pushes, R, C, Na, Nl):
    """[pushes, R, C, Na, Nl] int32: sparse small counts, an empty push, and one push of cells near 2^31 - 1"""
    shape = (pushes, R, C, Na, Nl)
    h = rng.integers(0, 6, shape) * (rng.random(shape) < 0.3)
    h[3] = 0
    h[4] = (2 ** 31 - 1 - rng.integers(0, 3, shape[1:])) * (rng.random(shape[1:]) < 0.5)
    return h.astype(np.int32)


def params_for(rng, R):
    q = np.empty((R, 8))
    q[:, 0], q[:, 2] = rng.integers(0, 3, R) / 4, rng.integers(0, 2, R) / 2
    q[:, 1], q[:, 3] = rng.integers(2, 5, R) / 4, rng.integers(1, 3, R) / 2
    q[:, 4:] = (1.0, 1.0, 0.5, 2.5)
    return q


def edges(rng, R, N):
    e = np.cumsum(0.1 + rng.random((R, N + 1)), axis=1)
    e[::2, -1] = np.inf
    return e


def same(got, want, what):
    assert np.array_equal(np.asarray(got[1]), want[1]), "%s: totals %s, expected %s" % (what, got[1], want[1])
    assert np.array_equal(wb.bits(got[0]), wb.bits(want[0])), "%s: bounds\n%s\nexpected\n%s" % (what, got[0], want[0])


def want_after(hist, p0, p, W, ae, le, q):
    """the definition: the range form over the slices pushed since the stream began at push p0, concatenated along time"""
    C = hist.shape[2]
    cat = np.concatenate(list(hist[p0:p + 1]), axis=1)                    # [R, (p - p0 + 1) C, Na, Nl]
    t0, t1 = wb.window_range(p - p0, W, C)
    return wb.ref_bounds_rows(cat, ae, le, q, t0, t1), cat, (t0, t1)


@pytest.mark.parametrize("W", (1, 2, 5))
@pytest.mark.parametrize("C", (1, 4))
def test_every_push_is_the_many_row_call_over_the_window(P, eng, W, C):
    rng = np.random.default_rng(10 * W + C)
    R, Na, Nl, pushes, gap = 9, 5, 7, 12, 3
    hist = slices_for(rng, pushes, R, C, Na, Nl)
    ae, le = edges(rng, R, Na), edges(rng, R, Nl)
    F = C * Na * Nl
    hin = np.full((R, F + gap), ISENT, np.int32)
    d = DevArrays(eng, h=hin, ae=ae, le=le[0], q=np.zeros((R, 8)), b=np.full((R, 6), DSENT), t=np.full(R + 2, TSENT, np.int64))
    bs = P.WaveBoundsStream(R, Na, Nl, C, W)
    try:
        p0 = 0
        for p in range(pushes):
            if p == 7:                                                     # a reset in the middle: the window is empty again
                bs.reset()
                assert bs.blocks_held == 0
                p0 = p
            q = params_for(rng, R)
            hin[:, :F] = hist[p].reshape(R, F)
            d.put("h", hin)
            d.put("q", q)
            bs.push_dev(d.ptr("h"), F + gap, d.ptr("ae"), Na + 1, d.ptr("le"), 0, d.ptr("q"), 8, d.ptr("b"), 6, d.ptr("t"))
            assert bs.status() == 0 and bs.blocks_held == p - p0 + 1      # (status synchronises the device)
            b, t = d.get("b"), d.get("t")
            assert np.all(b[:, 4:] == DSENT) and np.all(t[R:] == TSENT) and np.array_equal(d.get("h"), hin)
            want, cat, (t0, t1) = want_after(hist, p0, p, W, ae, le[0], q)
            same((b[:, :4], t[:R]), want, "W=%d C=%d push %d" % (W, C, p))
            # ... and the many-row call itself over the concatenated slices
            pairs = [(q[:, 2 * k], q[:, 2 * k + 1]) for k in range(4)]
            same(P.wave_filter_bounds(cat, ae, le[0], *pairs, time_bins=(t0, t1), want_total=True), want, "many-row call, push %d" % p)
    finally:
        bs.close()
        d.free()


@pytest.mark.parametrize("Na, Nl, C", ((1, 1, 1), (64, 16, 8), (16, 64, 1), (32, 32, 8), (64, 1, 128)))
def test_the_shapes_at_the_limits_through_the_host_form(P, Na, Nl, C):
    rng = np.random.default_rng(Na + Nl + C)
    R, W, pushes = 3, 3, 8
    hist = slices_for(rng, pushes, R, C, Na, Nl)
    ae, le = edges(rng, R, Na), edges(rng, R, Nl)[1]
    bs = P.WaveBoundsStream(R, Na, Nl, C, W)
    ref = [wb.RefBoundsStream(W) for _ in range(R)]
    try:
        for p in range(pushes):
            q = params_for(rng, R)
            pairs = [(q[:, 2 * k], q[:, 2 * k + 1]) for k in range(4)]
            got = bs.push(hist[p], ae, le, *pairs, want_total=True)
            assert got[0].shape == (R, 4) and got[1].dtype == np.int64
            want = want_after(hist, 0, p, W, ae, le, q)[0]
            same(got, want, "%dx%d C=%d push %d" % (Na, Nl, C, p))
            kept = [ref[r].push(hist[p, r], ae[r], le, q[r]) for r in range(R)]     # the windowed statement, as the stream keeps it
            same(got, (np.stack([b for b, _ in kept]), np.array([n for _, n in kept])), "windowed statement, push %d" % p)
        one = bs.push(hist[0], ae[0], le, (0.25, 0.75))                    # one set of edges and parameters, no totals
        assert one.shape == (R, 4)
        for bad in (hist[0][:, :, :, :-1] if Nl > 1 else hist[0][:-1], hist[0].astype(np.int64)):
            with pytest.raises(ValueError):
                bs.push(bad, ae, le)
        assert bs.blocks_held == pushes + 1
    finally:
        bs.close()


def test_kind_refusals_both_ways_and_bad_strides(P, eng):
    L = P.streaming._lib.load()
    bs = P.WaveBoundsStream(2, 4, 4, 2, 3)
    tb = P.WaveTableStream(64, rows=2)
    hsm = P.WaveHistogramStream(64, rows=2, horizon=64, amplitude_edges=np.arange(5.0), length_edges=np.arange(1.0, 6.0))
    d = DevArrays(eng, h=np.zeros((2, 32), np.int32), e=np.arange(5.0), q=np.array([0.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0]),
                  b=np.full((2, 4), DSENT), x=np.zeros((2, 4096)))
    em = ctypes.c_int32(0)
    p = {k: ctypes.c_void_p(d.ptr(k)) for k in ("h", "e", "q", "b", "x")}
    try:
        for other in (tb, hsm):                                            # the bounds entries refuse every other kind
            assert L.itd_bounds_stream_push(other._h, p["h"], 32, p["e"], 0, p["e"], 0, p["q"], 0, p["b"], 4, None, None) == 1
            assert L.itd_bounds_stream_push_host(other._h, p["h"], p["e"], 0, p["e"], 0, p["q"], 0, p["b"], None) == 1
        h = bs._h                                                          # ... and every other kind's entries refuse a bounds stream
        assert L.itd_stream_push_f64(h, p["x"], 64, p["x"], 64, None, 0, ctypes.byref(em), None) == 1
        assert L.itd_stream_flush_f64(h, p["x"], 64, None, 0, ctypes.byref(em), None) == 1
        assert L.itd_levels_stream_push_f64(h, p["x"], 64, p["x"], 64, 64, None, ctypes.byref(em), None) == 1
        assert L.itd_wave_stream_push_f64(h, p["x"], 64, p["b"], 4, p["x"], 64, ctypes.byref(em), None) == 1
        assert L.itd_wave_stream_flush_f64(h, p["b"], 4, p["x"], 64, ctypes.byref(em), None) == 1
        assert L.itd_hist_stream_push_f64(h, p["x"], 64, p["e"], 0, p["e"], 0, p["h"], p["h"], 16, None, None, 0, ctypes.byref(em), None) == 1
        assert L.itd_table_stream_push_f64(h, p["x"], 64, None, None, None, None, 65, p["h"], ctypes.byref(em), None) == 1
        assert L.itd_table_stream_flush_f64(h, None, None, None, None, 65, p["h"], ctypes.byref(em), None) == 1
        assert L.itd_wave_stream_latency(h) == -1 and L.itd_hist_stream_latency(h) == -1
        # strides and pointers out of range: refused before any launch, the stream as it was
        good = dict(h=d.ptr("h"), hs=32, ae=d.ptr("e"), sa=0, le=d.ptr("e"), sl=0, q=d.ptr("q"), sq=0, b=d.ptr("b"), sb=4)
        for kw in (dict(hs=31), dict(sa=4), dict(sl=1), dict(sq=7), dict(sb=3), dict(sb=0), dict(h=None), dict(ae=None), dict(le=None),
                   dict(q=None), dict(b=None)):
            a = dict(good, **kw)
            with pytest.raises(P.ITDError):
                bs.push_dev(a["h"], a["hs"], a["ae"], a["sa"], a["le"], a["sl"], a["q"], a["sq"], a["b"], a["sb"])
        assert bs.blocks_held == 0 and bs.status() == 0 and np.all(d.get("b") == DSENT)
        bs.push_dev(*[good[k] for k in ("h", "hs", "ae", "sa", "le", "sl", "q", "sq", "b", "sb")])
        assert bs.status() == 0 and bs.blocks_held == 1
        assert d.get("b").tolist() == [[0.0, 4.0, 0.0, 4.0]] * 2          # an empty window: the whole edge range
    finally:
        for s in (bs, tb, hsm):
            s.close()
        d.free()


def test_the_chain_from_samples_to_filtered_rows_on_one_stream(P):
    """LevelsStream -> WaveHistogramStream -> WaveBoundsStream -> WaveFilterStream through device pointers on one HIP stream equals,
    bit for bit, the same chain through the host forms with the reference's bounds handed to WaveFilterStream.push(bounds=...)."""
    import torch
    L, M, H, hop, Na, Nl, W, pushes = 256, 3, 512, 128, 8, 8, 3, 14
    C, R = L // hop, M + 1
    rng = np.random.default_rng(2028)
    t = np.arange(pushes * L)
    x = np.sin(2 * np.pi * t / 37.0) * (1.0 + 0.5 * np.sin(2 * np.pi * t / 900.0)) + 0.3 * rng.standard_normal(t.size) + 0.8 * np.sin(2 * np.pi * t / 301.0)
    ae = np.concatenate(([0.0], np.geomspace(0.05, 3.0, Na - 1), [np.inf]))
    le = np.concatenate(([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0], [np.inf]))
    q = np.array([0.2, 0.9, 0.1, 1.0, 1.0, 1.0, 1.0, 1.0])
    start = np.array([0.0, np.inf, 0.0, np.inf])

    def streams():
        return (P.streaming.LevelsStream(L, M), P.streaming.WaveHistogramStream(L, rows=R, horizon=H, amplitude_edges=ae, length_edges=le, hop=hop),
                P.streaming.WaveFilterStream(L, rows=R, horizon=H))
    # the host forms, the reference's bounds in between
    lv, hs, wf = streams()
    ref = [wb.RefBoundsStream(W) for _ in range(R)]
    bounds, host_out, host_bounds = np.tile(start, (R, 1)), [], []
    for p in range(pushes):
        got = lv.push(x[p * L:(p + 1) * L])
        if got is None:
            continue
        rows = got[0]
        hist = hs.push(rows)
        if hist is not None:
            bounds = np.stack([ref[r].push(hist.count[r], ae, le, q)[0] for r in range(R)])
            host_bounds.append(bounds)
        out = wf.push(rows, bounds=bounds)
        if out is not None:
            host_out.append(out)
    for s in (lv, hs, wf):
        s.close()
    assert len(host_out) == pushes - (M + 1) - 2 and len(host_bounds) == len(host_out)
    assert len({b.tobytes() for b in host_bounds}) > 3                    # the bounds move with the signal

    # device pointers, one HIP stream
    lv, hs, wf = streams()
    bs = P.WaveBoundsStream(R, Na, Nl, C, W)
    dev = torch.device("cuda")
    x_d = torch.from_numpy(x.reshape(pushes, L)).to(dev)
    rows_d, out_d = torch.zeros((R, L), dtype=torch.float64, device=dev), torch.zeros((R, L), dtype=torch.float64, device=dev)
    ae_d, le_d, q_d = (torch.from_numpy(v).to(dev) for v in (ae, le, q))
    count_d, samples_d = (torch.zeros((R, C, Na, Nl), dtype=torch.int32, device=dev) for _ in range(2))
    bounds_d = torch.from_numpy(np.tile(start, (R, 1))).to(dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    dev_out, dev_bounds = [], []
    with torch.cuda.stream(s):
        for p in range(pushes):
            if not lv.push_dev(x_d[p].data_ptr(), L, rows_d.data_ptr(), L, R * L, None, s.cuda_stream):
                continue
            if hs.push_dev(rows_d.data_ptr(), L, ae_d.data_ptr(), 0, le_d.data_ptr(), 0, count_d.data_ptr(), samples_d.data_ptr(), C * Na * Nl,
                           None, None, 0, s.cuda_stream):
                bs.push_dev(count_d.data_ptr(), C * Na * Nl, ae_d.data_ptr(), 0, le_d.data_ptr(), 0, q_d.data_ptr(), 0, bounds_d.data_ptr(), 4,
                            None, s.cuda_stream)
                dev_bounds.append(bounds_d.clone())
            if wf.push_dev(rows_d.data_ptr(), L, bounds_d.data_ptr(), 4, out_d.data_ptr(), L, s.cuda_stream):
                dev_out.append(out_d.clone())
    s.synchronize()
    assert len(dev_out) == len(host_out) and len(dev_bounds) == len(host_bounds)
    for k, (g, w) in enumerate(zip(dev_bounds, host_bounds)):
        assert np.array_equal(wb.bits(g.cpu().numpy()), wb.bits(w)), "bounds of emitted block %d" % k
    for k, (g, w) in enumerate(zip(dev_out, host_out)):
        assert np.array_equal(wb.bits(g.cpu().numpy()), wb.bits(w)), "filtered block %d" % k
    assert any((o == 0.0).any() and (o != 0.0).any() for o in host_out)   # the filter removes some half waves and keeps others
    for st in (lv, hs, wf, bs):
        st.close()
