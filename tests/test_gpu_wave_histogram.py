"""The half waves' joint amplitude-length histogram on the GPU (itd_wave_hist_batch_f64 / _f32, pyitd_amd.wave_histogram;
itd_wave_hist.hpp) against wave_hist_ref, the numpy statement of the definition: every output is an integer, so everything is
compared exactly.

Where the kernel can go wrong: a value exactly on an edge, the time bin of a half wave whose peak lies in another tile than its
end (k_wave_hist bins a half wave in the tile it ends in), equal maxima on both sides of a time seam, the per-tile LDS histogram
and its hand-over under contention (every sample its own half wave, all in one cell), the zeroing of the rows' slots and only of
them, NULL outputs, NaN rows, per-row edges across the chunk seam of more rows than one grid, a caller's stream, a captured graph
whose edges change in place, and the order of the integer atomics (which must not show).
"""
import numpy as np
import pytest

import wave_hist_ref as wh
import waves_ref
from helpers import DevArrays
from oracle import exact_tfe as et
from test_oracle_exact_tfe import FAMILIES, family, with_crossings
from test_single_waves_cpu import LENGTHS, tied_row

pytestmark = pytest.mark.gpu
ISENT = -777
CARRY_K = 2048                  # records per pass of k_wave_carry<256> (kInstCarryChunk)
FIELDS = ("count", "samples", "outside")


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


@pytest.fixture
def eng(P):
    from pyitd_amd.itd import _engine_for
    return _engine_for(8192)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.int32 and got.shape == want.shape, "%s: %s %s, expected %s" % (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at %s: %d, expected %d" % (
        what, bad.size, got.size, np.unravel_index(bad[0], got.shape), got.ravel()[bad[0]], want.ravel()[bad[0]])


def own_edges(values, N, pad):
    """N + 1 strictly increasing edges that stand ON values the row has (its quantiles), padded below with pad - 1, pad - 2, ..."""
    v = np.unique(np.asarray(values, dtype=np.float64))
    v = v[np.isfinite(v)]
    e = np.unique(v[(np.arange(N + 1) * max(v.size - 1, 0)) // N]).tolist() if v.size else []
    while len(e) < N + 1:
        e.insert(0, (min(e[0], pad) if e else pad) - 1.0)
    return np.array(e)


def tables_of(rows):
    return [waves_ref.ref_table(x) for x in np.asarray(rows, dtype=np.float64)]


def check(P, rows, ae, le, hop, what, tables=None):
    """wave_histogram of rows[R, n] against the reference row by row; ae / le: one set or one per row."""
    tables = tables_of(rows) if tables is None else tables
    ae, le = np.asarray(ae, dtype=np.float64), np.asarray(le, dtype=np.float64)
    h = P.wave_histogram(rows, ae, le, hop=hop)
    assert isinstance(h, P.WaveHistogram)
    for r, x in enumerate(np.asarray(rows, dtype=np.float64)):
        want = wh.ref_hist(x, ae[r] if ae.ndim == 2 else ae, le[r] if le.ndim == 2 else le, hop, tables[r])
        for name, got, w in zip(FIELDS, h, want):
            same(got[r], w, "%s row %d %s" % (what, r, name))
        assert int(h.count[r].sum()) + int(h.outside[r].sum()) == tables[r][0].size
    return h


# ---- 1. the signal families at every seam length ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("n", LENGTHS)
def test_signal_families_against_the_definition(P, n, dtype):
    with np.errstate(over="ignore", under="ignore"):     # float32: "huge" becomes +-inf, "subnormal" zeros — rows like any other
        rows = np.stack([family(fam, n) for fam in FAMILIES] + [tied_row(n)]).astype(dtype)
    tables = tables_of(rows)
    shared_a = np.array([0.0, 0.3, 0.75, 1.0, 2.5, 4.0, 1e299, np.inf])
    shared_l = np.array([1.0, 2.0, 3.0, 4.0, 8.0, 19.0, 600.0, 3000.0])
    own_a = np.stack([own_edges(np.abs(t[3]), 5, 0.0) for t in tables])
    own_l = np.stack([own_edges(t[1], 4, 1.0) for t in tables])
    for hop in (None, 512, 1024):
        check(P, rows, shared_a, shared_l, hop, "n=%d hop=%s, one edge set" % (n, hop), tables)
        check(P, rows, own_a, own_l, hop, "n=%d hop=%s, edges per row" % (n, hop), tables)
    check(P, rows, own_a, shared_l, 512, "n=%d, amplitude edges per row only" % n, tables)


# ---- 2. amplitudes and lengths exactly on the edges ---------------------------------------------------------------------------------
def test_values_on_an_edge_open_the_upper_bin(P):
    n = 3 * 512 + 77
    x = family("noise", n)
    table = waves_ref.ref_table(x)
    _, length, peak, value = table
    k = int(np.argmax(length))                                      # one half wave to watch
    A, ln, t = abs(value[k]), float(length[k]), int(peak[k]) // 512
    up, down, inf = np.nextafter(A, np.inf), np.nextafter(A, 0.0), np.inf
    wide_l, wide_a = [0.0, 1.5, inf], [0.0, A / 2, inf]
    #        amplitude edges       length edges                         where wave k must be counted: (i, j) or None = outside
    cases = [([0.0, A, inf], wide_l, (1, 1)),                           # on an edge: the upper bin
             ([0.0, up, inf], wide_l, (0, 1)),                          # nextafter below the edge: the lower bin
             ([down, A, up], wide_l, (1, 1)),
             ([0.0, A / 2, A], wide_l, None),                           # on the last edge: outside
             ([A, up, inf], wide_l, (0, 1)),                            # on the first edge: inside
             ([up, 2 * up, inf], wide_l, None),
             (wide_a, [0.0, ln, inf], (1, 1)),
             (wide_a, [0.0, np.nextafter(ln, inf), inf], (1, 0)),
             (wide_a, [0.0, 1.0, ln], None),
             (wide_a, [ln, ln + 1.0, inf], (1, 0)),
             (wide_a, [1.0, 2.0, 1e300], (1, 1)),
             ([-inf, A, inf], [-inf, ln, inf], (1, 1))]                 # infinite end edges: nothing is outside
    rows = np.stack([x] * len(cases))
    ae, le = np.array([c[0] for c in cases]), np.array([c[1] for c in cases])
    for hop in (None, 512):
        h = check(P, rows, ae, le, hop, "edge cases hop=%s" % hop, [table] * len(cases))
        tk = t if hop else 0
        for r, (_, _, cell) in enumerate(cases):
            # the same call with wave k's own samples zeroed out of the reference would differ exactly here: check the cell directly
            others = np.delete(np.arange(length.size), k)
            want = wh.hist_of_table(n, length[others], peak[others], value[others], ae[r], le[r], hop or wh.default_hop(n))
            if cell is None:
                assert h.outside[r, tk] == want[2][tk] + 1 and np.array_equal(h.count[r], want[0]), cases[r]
            else:
                assert h.count[r, tk][cell] == want[0][tk][cell] + 1 and h.samples[r, tk][cell] == want[1][tk][cell] + length[k], cases[r]
                assert np.array_equal(h.outside[r], want[2]), cases[r]
    assert h.outside[-1].sum() == 0


# ---- 3. time seams ------------------------------------------------------------------------------------------------------------------
def test_the_peak_decides_the_time_bin_at_a_seam(P):
    n, hop = 3 * 512 + 1, 512
    rng = np.random.default_rng(41)

    def quiet():
        return with_crossings(n, [400, 600, n - 2], rng, mag=0.1 + 0.5 * rng.random(n))
    rows = [quiet() for _ in range(4)]
    for x, at in zip(rows, ((511,), (512,), (511, 512), (512, 599))):   # the half wave 401 .. 600 lies across the seam at 512
        for p in at:
            x[p] = np.sign(x[p]) * 0.75
    rows = np.stack(rows)
    ae, le = [0.0, 0.7, 0.8], [1.0, 2.0, 250.0, 2000.0]
    h = check(P, rows, ae, le, hop, "seam")
    assert h.count.shape == (4, 4, 2, 3)
    for r, t in enumerate((0, 1, 0, 1)):                            # row 2: equal maxima on both sides, the earliest index decides
        assert h.count[r, :, 1, 1].tolist() == [1 - t, t, 0, 0] and h.samples[r, t, 1, 1] == 200, (r, h.count[r, :, 1, 1])
    # the last time bin is one sample, and that sample is a half wave of its own
    assert h.count[:, 3].sum(axis=(1, 2)).tolist() == [1] * 4 and h.samples[:, 3].sum(axis=(1, 2)).tolist() == [1] * 4
    assert np.all(h.count[:, 3, 0, 0] == 1)
    # tied_row: the first half wave's maximum stands in two tiles 600 samples apart and is binned where it stands first
    n2 = 20011
    t = tied_row(n2)[None, :]
    h = check(P, t, [0.7, 0.8], [1.0, 1e5], 512, "tied")
    assert np.flatnonzero(h.count[0, :, 0, 0]).tolist() == [(n2 // 8) // 512, (n2 // 2 + 2) // 512]
    assert (n2 // 8 + 600) // 512 != (n2 // 8) // 512
    check(P, t, [0.7, 0.8], [1.0, 1e5], 1024, "tied, hop 1024")


# ---- 4. a half wave over many tiles -----------------------------------------------------------------------------------------------
def test_a_half_wave_of_513_tiles_lands_where_its_peak_is(P):
    n = (1 << 18) + 3
    first, last, mid = (family("positive", n) for _ in range(3))
    first[5] = 3.0                                                  # the peak in the first tile: time bin 0, not bin 512 where it ends
    last[n - 1] = 3.0
    mid[200 * 512 + 511] = 3.0
    mid[300 * 512] = 3.0                                            # an equal maximum 100 tiles later
    rows = np.stack([first, last, mid])
    h = check(P, rows, [0.0, 2.0, 4.0], [1.0, 1000.0, 1e6], 512, "513 tiles")
    assert h.count.shape == (3, 513, 2, 2)
    for r, t in enumerate((0, 512, 200)):
        assert np.flatnonzero(h.count[r].sum(axis=(1, 2))).tolist() == [t] and h.count[r, t, 1, 1] == 1 and h.samples[r, t, 1, 1] == n
    assert not h.outside.any()


def test_half_waves_across_the_carry_chunks(P):
    """test_gpu_single_waves' rows of (2 K + 1) * 512 + 5 samples with a single crossing: the first half wave's maximum is the
    row's second sample, the second one's the row's last, so each peak crosses chunk seams of the forward or the backward pass on
    its way to the tile that bins the half wave."""
    n = (2 * CARRY_K + 1) * 512 + 5
    rng = np.random.default_rng(17)
    rows, cuts = [], []
    for tile in (100, 2 * CARRY_K - 90):
        x = with_crossings(n, [tile * 512 + 300], rng, mag=0.1 + 0.5 * rng.random(n))
        x[1] = 0.9375
        x[-1] = np.sign(x[-1]) * 0.96875
        rows.append(x)
        cuts.append(tile * 512 + 300)
    rows = np.stack(rows)
    h = check(P, rows, [0.9, 0.95, 1.0], [1.0, 1e7], 512, "carry chunks")
    T = 2 * CARRY_K + 2
    assert h.count.shape == (2, T, 2, 1)
    for r in range(2):
        assert np.flatnonzero(h.count[r].sum(axis=(1, 2))).tolist() == [0, T - 1]
        assert h.samples[r, 0, 0, 0] == cuts[r] + 1 and h.samples[r, T - 1, 1, 0] == n - 1 - cuts[r]


# ---- 5. contention: every sample its own half wave, all in one cell ---------------------------------------------------------------
def test_one_cell_takes_every_half_wave(P):
    n = 20011
    zig = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)               # crossings at 1 .. n-2: half waves (0, 1), (2), (3), ..., (n-1)
    ae, le = [0.5, 2.0], [1.0, 2.0]                                # the first half wave (2 samples) is outside
    h = check(P, zig[None, :], ae, le, None, "zigzag")
    assert h.count.shape == (1, 1, 1, 1) and h.outside[0, 0] == 1
    assert h.count[0, 0, 0, 0] == n - 1 - h.outside[0, 0] == n - 2 and h.samples[0, 0, 0, 0] == n - 2
    table = tables_of(zig[None, :]) * 64
    h = check(P, np.stack([zig] * 64), ae, le, None, "zigzag x 64", table)
    assert np.all(h.count == n - 2) and np.all(h.samples == n - 2) and np.all(h.outside == 1)
    h = check(P, np.stack([zig, -zig]), [0.5, 1.0, 2.0], [1.0, 2.0, 3.0], 1024, "zigzag over time", table[:2])
    assert h.count[0, :, 1, 0].tolist() == [1022] + [1024] * 18 + [20011 - 19 * 1024] and h.count[0, 0, 1, 1] == 1


# ---- 6. buffers: sentinels, gaps, NULL outputs, NaN rows (the C entries on device arrays) ----------------------------------------
def run_hist(eng, rows, ae, le, hop, hist_stride=None, want=(1, 1, 1), row_stride=None, edge_gap=0, pad=5, stream=None):
    """itd_wave_hist_batch_* on device buffers that hold ISENT.  ae / le: [N + 1] (stride 0) or [R, N + 1].  Returns (count, samples
    as [R, hist_stride], the pad behind each, outside [R, T], info, the edges as left behind)."""
    R, n = rows.shape
    ae, le = np.asarray(ae, dtype=np.float64), np.asarray(le, dtype=np.float64)
    Na, Nl, T = ae.shape[-1] - 1, le.shape[-1] - 1, -(-n // hop) if hop > 0 else 1        # (a hop the entry refuses: any size)
    slot = T * Na * Nl
    hs = slot if hist_stride is None else hist_stride
    rs = n if row_stride is None else row_stride
    xin = np.full((R, rs), np.finfo(rows.dtype).max, rows.dtype)
    xin[:, :n] = rows

    def edges(e):
        if e.ndim == 1:
            return e, 0
        g = np.full((R, e.shape[1] + edge_gap), np.nan)
        g[:, :e.shape[1]] = e
        return g, g.shape[1]
    (da, sa), (dl, sl) = edges(ae), edges(le)
    sent = np.full(max(R * hs, (R - 1) * hs + slot) + pad, ISENT, np.int32)
    d = DevArrays(eng, x=xin, ae=da, le=dl, count=sent, samples=sent, outside=np.full(R * T + pad, ISENT, np.int32), info=np.full(R, ISENT, np.int32))
    try:
        eng.wave_hist_batch_dev(d.ptr("x"), rows.dtype, n, R, rs, d.ptr("ae"), sa, Na, d.ptr("le"), sl, Nl, hop,
                                d.ptr("count") if want[0] else None, d.ptr("samples") if want[1] else None, hs,
                                d.ptr("outside") if want[2] else None, d.ptr("info"), stream)
        out = {k: d.get(k) for k in FIELDS}
        assert np.array_equal(d.get("x").view(np.uint64 if rows.dtype == np.float64 else np.uint32), xin.view(np.uint64 if rows.dtype == np.float64 else np.uint32))
        assert np.array_equal(d.get("ae"), da, equal_nan=True) and np.array_equal(d.get("le"), dl, equal_nan=True)
        return out, d.get("info")
    finally:
        d.free()


def check_buffers(out, rows, ae, le, hop, hs, want, skip=(), pad=5):
    """Every cell of every slot is the reference's; the gaps between the slots and the pads hold the sentinel."""
    R, n = rows.shape
    ae, le = np.asarray(ae, dtype=np.float64), np.asarray(le, dtype=np.float64)
    T = -(-n // hop)
    slot = T * (ae.shape[-1] - 1) * (le.shape[-1] - 1)
    refs = [None if r in skip else wh.ref_hist(rows[r], ae[r] if ae.ndim == 2 else ae, le[r] if le.ndim == 2 else le, hop) for r in range(R)]
    for i, name in enumerate(FIELDS[:2]):
        body, tail = out[name][:R * hs].reshape(R, hs), out[name][R * hs:]
        assert tail.size == pad and np.all(tail == ISENT), "%s: the pad behind the last row is written" % name
        if not want[i]:
            assert np.all(body == ISENT), "%s was not asked for" % name
            continue
        assert np.all(body[:, slot:] == ISENT), "%s: a gap between the rows' slots is written" % name
        for r in range(R):
            if refs[r] is not None:
                same(body[r, :slot], refs[r][i].ravel(), "%s row %d" % (name, r))
    body, tail = out["outside"][:R * T].reshape(R, T), out["outside"][R * T:]
    assert np.all(tail == ISENT)
    if not want[2]:
        assert np.all(body == ISENT)
    else:
        for r in range(R):
            if refs[r] is not None:
                same(body[r], refs[r][2], "outside row %d" % r)


@pytest.mark.parametrize("n", (5 * 512 + 77, 515))
def test_every_cell_is_written_and_nothing_else(eng, n):
    rows = np.stack([family(fam, n) for fam in ("noise", "seams", "quantised", "slow", "zeros")])
    crossings = [int(np.count_nonzero(et.structure(x)[0])) for x in rows]
    tables = tables_of(rows)
    ae = np.stack([own_edges(np.abs(t[3]), 3, 0.0) for t in tables])
    le = np.array([1.0, 2.0, 5.0, 50.0])
    for hop, gap, rs, want in ((512, 0, n, (1, 1, 1)), (512, 7, n + 13, (1, 1, 1)), (1024, 3, n + 1, (1, 0, 1)), (1024, 3, n, (0, 1, 0)),
                               (3072, 1, n, (1, 1, 0))):
        T = -(-n // hop)
        hs = T * 9 + gap
        out, info = run_hist(eng, rows, ae, le, hop, hs, want, rs, edge_gap=2)
        assert info.tolist() == crossings
        check_buffers(out, rows, ae, le, hop, hs, want)
    out, info = run_hist(eng, rows.astype(np.float32), ae[0], le, 512, -(-n // 512) * 9 + 4, row_stride=n + 3)     # one set, float32 rows
    check_buffers(out, rows.astype(np.float32).astype(np.float64), ae[0], le, 512, -(-n // 512) * 9 + 4, (1, 1, 1))
    # a single row: its stride and the histograms' stride are not looked at
    out, _ = run_hist(eng, rows[:1], ae[0], le, 512, 0)
    same(out["count"][:-5], wh.ref_hist(rows[0], ae[0], le, 512)[0].ravel(), "one row")


def test_the_entries_refuse_bad_arguments(P, eng):
    n = 700
    rows = np.stack([family("noise", n)] * 2)
    ae, le = np.linspace(0.0, 4.0, 5), np.array([1.0, 3.0, 9.0])
    bad = [dict(hop=0), dict(hop=256), dict(hop=768), dict(hop=-512), dict(hist_stride=15), dict(want=(0, 0, 1))]
    for kw in bad:
        with pytest.raises(P.ITDError):
            run_hist(eng, rows, ae, le, **{"hop": 512, **kw})
    for a, l in ((np.linspace(0.0, 1.0, 66), le), (ae, np.linspace(1.0, 9.0, 66)), (np.linspace(0.0, 1.0, 34), np.linspace(1.0, 9.0, 33))):
        with pytest.raises(P.ITDError):
            run_hist(eng, rows, a, l, 512)
    d = DevArrays(eng, x=rows, e=np.zeros(8), h=np.full(64, ISENT, np.int32))
    try:
        for args in ((d.ptr("e"), 4, 4, d.ptr("e"), 0, 2), (d.ptr("e"), 0, 4, d.ptr("e"), 2, 2), (None, 0, 4, d.ptr("e"), 0, 2),
                     (d.ptr("e"), 0, 4, None, 0, 2), (d.ptr("e"), 0, 0, d.ptr("e"), 0, 2), (d.ptr("e"), 0, 4, d.ptr("e"), 0, 0)):
            with pytest.raises(P.ITDError):
                eng.wave_hist_batch_dev(d.ptr("x"), np.float64, n, 2, n, *args, 1024, d.ptr("h"), None, 8)
        for nn, rs in ((2, n), (n, n - 1)):                              # n < 3; rows that overlap
            with pytest.raises(P.ITDError):
                eng.wave_hist_batch_dev(d.ptr("x"), np.float64, nn, 2, rs, d.ptr("e"), 0, 4, d.ptr("e"), 0, 2, 1024, d.ptr("h"), None, 8)
        assert np.all(d.get("h") == ISENT)
    finally:
        d.free()


@pytest.mark.parametrize("where", ("first", "seam", "last"))
def test_rows_with_a_nan(P, eng, where):
    n = 3 * 512 + 5
    rows = np.stack([family(fam, n) for fam in ("noise", "seams", "quantised", "noise", "slow")])
    rows[3] = rows[3][::-1]
    bad = rows.copy()
    at = {"first": 0, "seam": 512, "last": n - 1}[where]
    bad[1, at] = np.nan
    bad[3, at - 1 if where == "seam" else at] = np.nan
    with np.errstate(invalid="ignore"):
        crossings = [int(np.count_nonzero(et.structure(x)[0])) for x in bad]
    ae = np.stack([own_edges(np.abs(waves_ref.ref_table(x)[3]), 4, 0.0) for x in rows])
    le = np.array([1.0, 2.0, 4.0, 9.0, 1000.0])
    hs = 4 * 16 + 6
    out, info = run_hist(eng, bad, ae, le, 512, hs, row_stride=n + 13)
    assert info.tolist() == [crossings[0], -1 - crossings[1], crossings[2], -1 - crossings[3], crossings[4]]
    check_buffers(out, rows, ae, le, 512, hs, (1, 1, 1), skip=(1, 3))     # the neighbours are exact, the gaps and pads untouched
    with pytest.raises(P.ITDError, match=r"NaN in rows \[1, 3\]"):
        P.wave_histogram(bad, ae, le)


# ---- 7. more rows than one launch takes --------------------------------------------------------------------------------------------
def test_more_rows_than_one_grid(P):
    """65 535 + 37 rows of 24 samples: 1024 different ones, repeated (row r is base row r % 1024, so the rows on both sides of the
    chunk seam at 65 535 differ), every row with its own amplitude edges."""
    R, n = 65535 + 37, 24
    base = np.random.default_rng(5).standard_normal((1024, n))
    idx = np.arange(R) % 1024
    tables = tables_of(base)
    ae = np.stack([own_edges(np.abs(t[3]), 3, 0.0) for t in tables])
    le = np.array([1.0, 2.0, 4.0])
    h = P.wave_histogram(base[idx], ae[idx], le)
    want = [wh.ref_hist(x, a, le, None, t) for x, a, t in zip(base, ae, tables)]
    for i, (name, got) in enumerate(zip(FIELDS, h)):
        same(got, np.stack([w[i] for w in want])[idx], name)


# ---- 8. the caller's stream and a captured graph whose edges change in place ---------------------------------------------------------
def test_on_a_callers_stream_and_in_a_graph(P, eng):
    import torch
    n, R, hop = 5 * 512 + 77, 4, 1024
    fams = ("noise", "seams", "quantised", "slow")
    x = np.stack([family(f, n) for f in fams])
    tables = tables_of(x)
    T = -(-n // hop)
    slot = T * 3 * 2
    ae_new = np.stack([own_edges(np.abs(t[3]), 3, 0.0) for t in tables])
    le_new = np.array([1.0, 3.0, 40.0])
    sent = np.full(R * slot, ISENT, np.int32)
    d = DevArrays(eng, x=x, ae=np.zeros((R, 4)), le=np.zeros(3), count=sent, samples=sent, outside=np.full(R * T, ISENT, np.int32),
                  info=np.zeros(R, np.int32))

    def enqueue(stream):
        eng.wave_hist_batch_dev(d.ptr("x"), np.float64, n, R, n, d.ptr("ae"), 4, 3, d.ptr("le"), 0, 2, hop, d.ptr("count"), d.ptr("samples"),
                                slot, d.ptr("outside"), d.ptr("info"), stream)

    def check_now(rows, ae, le, what):
        out = {k: d.get(k) for k in FIELDS}
        for r in range(R):
            want = wh.ref_hist(rows[r], ae[r], le, hop)
            same(out["count"].reshape(R, -1)[r], want[0].ravel(), "%s: count row %d" % (what, r))
            same(out["samples"].reshape(R, -1)[r], want[1].ravel(), "%s: samples row %d" % (what, r))
            same(out["outside"].reshape(R, T)[r], want[2], "%s: outside row %d" % (what, r))
    d.put("ae", ae_new)
    d.put("le", le_new)
    s = torch.cuda.Stream()
    enqueue(s.cuda_stream)
    s.synchronize()
    check_now(x, ae_new, le_new, "on the caller's stream")
    # (the call above was the warm-up of this size: the workspace exists, the capture allocates nothing)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            enqueue(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    y = x[::-1].copy()
    for rows, ae, le in ((x, ae_new * 0.5, np.array([2.0, 5.0, 41.0])), (y, ae_new[::-1].copy(), le_new),
                         (y, np.stack([[0.0, 0.5, 1.0, np.inf]] * R), np.array([1.0, 2.0, np.inf]))):
        d.put("x", rows)
        d.put("ae", ae)                             # the edges changed in place: the replay bins with the new ones
        d.put("le", le)
        g.replay()                                  # (the outputs still hold the last result: the replay clears them itself)
        torch.cuda.synchronize()
        check_now(rows, ae, le, "replayed")
    d.free()


# ---- 9. determinism ------------------------------------------------------------------------------------------------------------------
def test_the_same_bytes_from_run_to_run_and_in_any_batch_position(P):
    n = 9 * 512 + 300
    rows = np.stack([family(f, n) for f in ("noise", "quantised", "seams", "slow", "huge", "noise")])
    rows[5] = rows[5][::-1]
    ae, le = np.array([0.0, 0.5, 1.0, 1.5, 2.5, np.inf]), np.array([1.0, 2.0, 3.0, 5.0, 9.0, 17.0, np.inf])
    a = P.wave_histogram(rows, ae, le, hop=1024)
    b = P.wave_histogram(rows, ae, le, hop=1024)
    for name, u, v in zip(FIELDS, a, b):
        assert u.tobytes() == v.tobytes(), name
    moved = P.wave_histogram(np.concatenate((rows[1:], rows[:1])), ae, le, hop=1024)      # row 0 now stands last
    for name, u, v in zip(FIELDS, a, moved):
        assert u[0].tobytes() == v[-1].tobytes() and u[1:].tobytes() == v[:-1].tobytes(), name


# ---- 10. the torch-tensor path -----------------------------------------------------------------------------------------------------
def test_tensors_in_place(P):
    import torch
    n = 4099
    rows = np.stack([family(fam, n) for fam in ("noise", "slow", "quantised", "seams", "positive", "negzero")]).reshape(2, 3, n)
    t = torch.from_numpy(rows).cuda()
    ae = np.array([[0.0, 0.5, 1.0, 9.0], [0.0, 1.0, 2.0, 3.0], [0.25, 0.5, 2.0, 4.0]])          # one set per level (the second axis)
    le = np.array([1.0, 2.0, 10.0, 5000.0])
    h = P.wave_histogram(t, ae, le, hop=2048)
    assert all(v.device == t.device and v.dtype == torch.int32 for v in h)
    assert tuple(h.count.shape) == tuple(h.samples.shape) == (2, 3, 3, 3, 3) and tuple(h.outside.shape) == (2, 3, 3)
    for i in range(2):
        for j in range(3):
            want = wh.ref_hist(rows[i, j], ae[j], le, 2048)
            for name, got, w in zip(FIELDS, h, want):
                same(got[i, j].cpu().numpy(), w, "tensor %d %d %s" % (i, j, name))
    view = P.wave_histogram(t[:, 2:3, :].float(), torch.tensor([0.0, 1.5, 3.5], dtype=torch.float64), le)     # row stride 3 n, float32
    assert tuple(view.count.shape) == (2, 1, 1, 2, 3)
    for i in range(2):
        want = wh.ref_hist(rows[i, 2].astype(np.float32), [0.0, 1.5, 3.5], le)
        same(view.count[i, 0].cpu().numpy(), want[0], "view %d" % i)
        same(view.samples[i, 0].cpu().numpy(), want[1], "view %d" % i)
    strided = P.wave_histogram(t[:, 2:3, :], ae[2], le, hop=512)         # float64 in place: a non-contiguous leading axis
    same(strided.count[1, 0].cpu().numpy(), wh.ref_hist(rows[1, 2], ae[2], le, 512)[0], "a strided view")
    for bad in (t[:, 1:3, :], t[:, :, ::2]):                             # no one row stride; a strided last axis
        with pytest.raises(ValueError):
            P.wave_histogram(bad, ae[0], le)
