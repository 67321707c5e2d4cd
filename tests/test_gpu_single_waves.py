"""Single-wave analysis on the GPU (itd_waves_batch_f64 / _f32, itd_wave_filter_batch_f64 / _f32, pyitd_amd.single_waves,
pyitd_amd.wave_filter; itd_waves.hpp) against waves_ref, the numpy statement of the definitions: every output is an integer, a copy
of an input sample or a zero, so everything is compared bit for bit (the value of an all-zero half wave with == 0.0: the sign of
that zero is not pinned).

Where the kernels can go wrong: a half wave inside one 64-sample step, across steps of a tile, across tiles (the tile records and
their two scans along the row), across the scans' chunks — k_wave_carry takes K = 2048 records per pass on rows of more than 512
tiles, forward from the row's first tile and backward from its last — equal maxima (the earliest index is the peak) inside a
tile, across tiles and across chunks, the filter's inclusive bounds, strides and gaps, the table's capacity, pointer subsets, NaN
rows, more rows than one launch's grid takes, a caller's stream and a captured graph whose input and bounds change in place.
The file also passes with PYITD_POISON=1.
"""
import numpy as np
import pytest

import waves_ref
from helpers import DevArrays
from oracle import exact_tfe as et
from test_oracle_exact_tfe import FAMILIES, family, with_crossings
from test_single_waves_cpu import LENGTHS, some_bounds, tied_row

pytestmark = pytest.mark.gpu
SENT = -7.25e300
SENT32 = np.float32(-7.25e30)
ISENT = -777
CARRY_K = 2048                  # records per pass of k_wave_carry<256> (kInstCarryChunk)
COPY = (0.0, np.inf, 0.0, np.inf)


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


@pytest.fixture
def eng(P):
    from pyitd_amd.itd import _engine_for
    return _engine_for(8192)


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    bad = np.flatnonzero(a.view(u).ravel() != b.view(u).ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at %d: %r vs %r" % (what, bad.size, a.size, bad[0], a.ravel()[bad[0]], b.ravel()[bad[0]])


def _values(got, want, what):
    """Bit for bit, but an all-zero half wave's value with == 0.0."""
    zero = want == 0.0
    assert np.all(got[zero] == 0.0), what
    _bits(got[~zero], want[~zero], what)


def check_table(x, w, r, what, ref=None):
    """Row r of a Waves (numpy) against the reference of x: the entries in front of count, and the wrapper's fill behind."""
    rs, rl, rp, rv = waves_ref.ref_table(x) if ref is None else ref
    k = rs.size
    assert int(w.count[r]) == k, "%s: count %d, expected %d" % (what, w.count[r], k)
    assert w.start.dtype == w.length.dtype == w.peak.dtype == w.count.dtype == np.int32 and w.value.dtype == np.float64
    for got, want, name in ((w.start, rs, "start"), (w.length, rl, "length"), (w.peak, rp, "peak")):
        bad = np.flatnonzero(got[r, :k] != want)
        assert bad.size == 0, "%s: %s of half wave %d is %d, expected %d" % (what, name, bad[0], got[r, bad[0]], want[bad[0]])
        assert np.all(got[r, k:] == -1), "%s: %s behind the count" % (what, name)
    _values(w.value[r, :k], rv, what + ": value")
    assert np.all(np.isnan(w.value[r, k:])), what + ": value behind the count"


def check_rows(P, rows, what, bounds=None):
    """single_waves and wave_filter (every row its own bounds) of float64 or float32 rows against the reference."""
    wide = rows.astype(np.float64)
    w = P.single_waves(rows)
    assert w.start.shape == rows.shape[:1] + (int(w.count.max()),)
    b = np.array([some_bounds(x) for x in wide]) if bounds is None else bounds
    out = P.wave_filter(rows, amplitude=(b[:, 0], b[:, 1]), length=(b[:, 2], b[:, 3]))
    assert out.dtype == np.float64 and out.shape == rows.shape
    for r, x in enumerate(wide):
        check_table(x, w, r, "%s row %d" % (what, r))
        _bits(out[r], waves_ref.ref_filter(x, b[r]), "%s row %d filtered" % (what, r))
    return w, out


# ---- 1. the signal families at every seam length ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("n", LENGTHS)
def test_signal_families_against_the_definitions(P, n, dtype):
    with np.errstate(over="ignore", under="ignore"):     # float32: "huge" becomes +-inf, "subnormal" zeros — rows like any other
        rows = np.stack([family(fam, n) for fam in FAMILIES] + [tied_row(n)]).astype(dtype)
    check_rows(P, rows, "n=%d %s" % (n, np.dtype(dtype).name))


# ---- 2. half waves across many tiles and across the carry's chunk seams -------------------------------------------------------
def test_half_waves_over_hundreds_of_tiles(P):
    n = (1 << 18) + 3
    pos = family("positive", n)
    one = pos.copy()
    one[n // 2:] *= -1.0
    seams = sorted(512 * k + d for k in (1, 2, 200, 511, 512) for d in (-1, 0, 1))
    at_seams = with_crossings(n, seams, np.random.default_rng(3))
    assert np.flatnonzero(et.structure(at_seams)[0]).tolist() == seams
    rows = np.stack([pos, one, at_seams])
    w, _ = check_rows(P, rows, "513 tiles")
    assert w.count.tolist() == [1, 2, len(seams) + 1]
    assert w.length[0, 0] == n and w.length[1].tolist()[:2] == [n // 2, n - n // 2]


def test_half_waves_across_the_carry_chunks(P):
    """Rows of (2 K + 1) * 512 + 5 samples with a single crossing: the first half wave's maximum is the row's second sample, the
    second one's the row's last, so each pair (maximum, index) crosses chunk seams of the forward or the backward pass on its way to
    the tile that writes or filters by it, and so do the begin of the second half wave and the end of the first."""
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
    # keep the first half wave only, by its amplitude in row 0 and by its length in row 1
    b = np.array([(0.9375, 0.9375, 0.0, np.inf), (0.0, np.inf, cuts[1] + 1.0, cuts[1] + 1.0)])
    w, out = check_rows(P, rows, "carry chunks", b)
    for r in range(2):
        assert w.count[r] == 2 and w.start[r].tolist() == [0, cuts[r] + 1] and w.length[r].tolist() == [cuts[r] + 1, n - 1 - cuts[r]]
        assert w.peak[r].tolist() == [1, n - 1] and np.abs(w.value[r]).tolist() == [0.9375, 0.96875]
        assert np.all(out[r, :cuts[r] + 1] == rows[r, :cuts[r] + 1]) and not out[r, cuts[r] + 1:].any()


def test_the_last_sample_in_a_tile_of_its_own(P):
    rng = np.random.default_rng(23)
    for n in (513, 3 * 512 + 1):
        rows = np.stack([with_crossings(n, [n - 2], rng), with_crossings(n, [n - 3], rng), with_crossings(n, [5, 511], rng),
                         with_crossings(n, [], rng)])
        w, _ = check_rows(P, rows, "n=%d" % n)
        assert w.length[0, 1] == 1 and w.start[0, 1] == n - 1 and w.length[1, 1] == 2


# ---- 3. peak ties ---------------------------------------------------------------------------------------------------------------
def _plant(x, at, mag=0.75):
    for p in at:
        x[p] = np.sign(x[p]) * mag


def test_equal_maxima_give_the_earliest_index(P):
    rng = np.random.default_rng(31)
    n = 8 * 512 + 77

    def quiet(cross):
        return with_crossings(n, cross, rng, mag=0.1 + 0.5 * rng.random(n))
    rows, peaks = [], []
    x = quiet([])                                   # two steps of one tile, then other tiles: one half wave
    _plant(x, (512 + 70, 512 + 70 + 3 * 64, 512 + 300, 3 * 512 + 9, 7 * 512 + 70))
    rows.append(x); peaks.append([512 + 70])
    x = quiet([1000, 2900])                         # head, tail and whole tiles of one half wave, and its neighbours
    _plant(x, (3, 600, 1000, 1001, 1100, 1600, 2500, 2900, 2901, n - 1))
    rows.append(x); peaks.append([3, 1001, 2901])
    x = quiet([520, 530, 700, 1000])                # half waves inside a tile: the same lane of two steps, neighbouring lanes
    _plant(x, (521, 525, 530, 540, 540 + 64, 540 + 128, 698, 699, 701, 999, 1000))
    rows.append(x); peaks.append([0, 521, 540, 701, 1001])
    _plant(rows[-1], (0, 519, 1001, 4000))
    x = quiet([])                                   # 1, 0, -1 is one half wave: samples of both signs with the same magnitude
    x[200:205] = (0.9, 0.0, -0.9, 0.0, 0.3)
    x[2000:2003] = (-0.9, -0.0, 0.9)
    rows.append(x); peaks.append([200])
    rows.append(-x); peaks.append([200])
    rows = np.stack(rows)
    w, _ = check_rows(P, rows, "ties")
    for r, pk in enumerate(peaks):
        assert w.peak[r, :len(pk)].tolist() == pk, (r, w.peak[r, :len(pk)].tolist(), pk)
    assert w.value[3, 0] == 0.9 and w.value[4, 0] == -0.9


def test_equal_maxima_across_the_carry_chunks(P):
    n = (2 * CARRY_K + 1) * 512 + 5
    rng = np.random.default_rng(37)
    cut = (CARRY_K + 3) * 512 + 17
    rows = np.stack([with_crossings(n, c, rng, mag=0.1 + 0.5 * rng.random(n)) for c in ([], [cut])])
    far = (5 * 512 + 7, (CARRY_K + 7) * 512 + 1, (2 * CARRY_K - 6) * 512 + 500, n - 1)
    _plant(rows[0], far)
    _plant(rows[1], far)
    w, _ = check_rows(P, rows, "ties across chunks", np.array([COPY, (0.75, 0.75, cut + 1.0, n)]))
    assert w.peak[0, 0] == far[0] and w.peak[1].tolist() == [far[0], far[1]]


# ---- 4. the filter's edges ----------------------------------------------------------------------------------------------------
def test_bounds_are_inclusive_and_nextafter_drops_the_wave(P):
    n = 3 * 512 + 77
    x = family("noise", n)
    start, length, peak, value = waves_ref.ref_table(x)
    k = int(np.argmax(length))                                      # a half wave of a length no other has with this amplitude
    A, ln = abs(value[k]), float(length[k])
    sl = slice(start[k], start[k] + length[k])
    up, down = np.nextafter(A, np.inf), np.nextafter(A, 0.0)
    cases = [((A, A, ln, ln), True), ((A, A, 0, np.inf), True), ((0, np.inf, ln, ln), True),
             ((up, np.inf, 0, np.inf), False), ((0, down, 0, np.inf), False),
             ((0, np.inf, np.nextafter(ln, np.inf), np.inf), False), ((0, np.inf, 0, np.nextafter(ln, 0.0)), False)]
    rows = np.stack([x] * len(cases))
    b = np.array([c[0] for c in cases], dtype=np.float64)
    out = P.wave_filter(rows, amplitude=(b[:, 0], b[:, 1]), length=(b[:, 2], b[:, 3]))
    for r, (bounds, kept) in enumerate(cases):
        _bits(out[r], waves_ref.ref_filter(x, bounds), "bounds %s" % (bounds,))
        assert np.array_equal(out[r, sl], x[sl]) if kept else not out[r, sl].any(), bounds
    assert not out[0, :start[k]].any() and not out[0, start[k] + length[k]:].any()      # only that one wave passes case 0


def test_default_bounds_copy_and_one_set_serves_every_row(P):
    n = 2 * 512 + 514
    rows = np.stack([family(fam, n) for fam in FAMILIES])
    _bits(P.wave_filter(rows), rows, "default bounds")              # "negzero": -0.0 stays -0.0
    b = some_bounds(rows[0])
    shared = P.wave_filter(rows, amplitude=b[:2], length=b[2:])      # bounds_stride 0
    R = rows.shape[0]
    per_row = P.wave_filter(rows, amplitude=(np.full(R, b[0]), b[1]), length=(b[2], np.full(R, b[3])))   # bounds_stride 4
    _bits(shared, per_row, "one set against the same set per row")
    for r in range(R):
        _bits(shared[r], waves_ref.ref_filter(rows[r], b), "row %d" % r)
    cube = rows[:8].reshape(2, 4, n)                                 # leading axes, bounds that broadcast over them
    lo = np.array([[0.0], [0.5]])
    got = P.wave_filter(cube, amplitude=(lo, np.inf), length=(0, np.array([5.0, 9.0, 40.0, np.inf])))
    for i in range(2):
        for j in range(4):
            _bits(got[i, j], waves_ref.ref_filter(cube[i, j], (lo[i, 0], np.inf, 0, (5.0, 9.0, 40.0, np.inf)[j])), "cube %d %d" % (i, j))


def test_float32_out_is_the_reference_rounded_once(P):
    n = 2 * 512 + 514
    rows = np.stack([family(fam, n) for fam in FAMILIES])          # "subnormal" and "huge" among them
    b = np.array([some_bounds(x) for x in rows])
    got = P.wave_filter(rows, amplitude=(b[:, 0], b[:, 1]), length=(b[:, 2], b[:, 3]), out_dtype=np.float32)
    assert got.dtype == np.float32
    with np.errstate(over="ignore", under="ignore"):
        want = np.stack([waves_ref.ref_filter(x, bb) for x, bb in zip(rows, b)]).astype(np.float32)
    assert np.any(np.isinf(want[FAMILIES.index("huge")]))
    _bits(got, want, "float32 out")
    rows32 = rows[[0, 4, 8]].astype(np.float32)
    both = P.wave_filter(rows32, amplitude=(0.5, 2.0), out_dtype=np.float32)
    want = np.stack([waves_ref.ref_filter(x, (0.5, 2.0, 0, np.inf)) for x in rows32.astype(np.float64)]).astype(np.float32)
    _bits(both, want, "float32 in and out")


# ---- 5. buffers: strides, gaps, capacity, pointer subsets, NaN rows (the C entries on device arrays with sentinels) ----------------
TABLE = ("start", "length", "peak", "value")


def run_table(eng, rows, cap, mask=(1, 1, 1, 1), row_stride=None, wave_stride=None, count=True):
    """itd_waves_batch_* on device buffers: the input's gaps hold 1e308, the four tables (all exist) ISENT / SENT.  Returns ({name:
    [R, wave_stride] as left behind}, count, info, the input as left behind)."""
    R, n = rows.shape
    rs = n if row_stride is None else row_stride
    ws = max(cap, 1) if wave_stride is None else wave_stride
    xin = np.full((R, rs), 1e308, rows.dtype)
    xin[:, :n] = rows
    isent = np.full((R, ws), ISENT, np.int32)
    d = DevArrays(eng, x=xin, start=isent, length=isent, peak=isent, value=np.full((R, ws), SENT), count=np.full(R, ISENT, np.int32),
                  info=np.full(R, ISENT, np.int32))
    try:
        ptrs = [d.ptr(k) if on else None for k, on in zip(TABLE, mask)]
        eng.waves_batch_dev(d.ptr("x"), rows.dtype, n, R, rs, *ptrs, ws, cap, d.ptr("count") if count else None, d.ptr("info"))
        return {k: d.get(k) for k in TABLE}, d.get("count"), d.get("info"), d.get("x")
    finally:
        d.free()


def run_filter(eng, rows, bounds, row_stride=None, out_stride=None, bounds_stride=4, out_f32=False):
    R, n = rows.shape
    rs = n if row_stride is None else row_stride
    os_ = n if out_stride is None else out_stride
    xin = np.full((R, rs), 1e308, rows.dtype)
    xin[:, :n] = rows
    bin_ = np.full((R if bounds_stride else 1, max(bounds_stride, 4)), np.nan)
    bin_[:, :4] = bounds
    sent = np.full((R, os_), SENT32, np.float32) if out_f32 else np.full((R, os_), SENT)
    d = DevArrays(eng, x=xin, b=bin_, out=sent, info=np.full(R, ISENT, np.int32))
    try:
        eng.wave_filter_batch_dev(d.ptr("x"), rows.dtype, n, R, rs, d.ptr("b"), bounds_stride, d.ptr("out"), os_, out_f32, d.ptr("info"))
        return d.get("out"), d.get("info"), d.get("x"), d.get("b")
    finally:
        d.free()


@pytest.mark.parametrize("n", (5 * 512 + 77, 515))
def test_strides_gaps_capacity_and_pointer_subsets(eng, n):
    rows = np.stack([family(fam, n) for fam in ("noise", "seams", "quantised", "slow")])
    refs = [waves_ref.ref_table(x) for x in rows]
    counts = [r[0].size for r in refs]
    crossings = [int(np.count_nonzero(et.structure(x)[0])) for x in rows]
    assert counts == [c + 1 for c in crossings]
    big = max(counts)
    for cap, ws, rs in ((big, big, n), (big + 3, big + 11, n + 13), (counts[3] + 2, counts[3] + 5, n + 1), (1, 1, n)):
        got, count, info, xin = run_table(eng, rows, cap, row_stride=rs, wave_stride=ws)
        assert count.tolist() == counts and info.tolist() == crossings           # the true count, also where count > cap
        _bits(xin[:, :n], rows, "the input is left alone")
        assert np.all(xin[:, n:] == 1e308)
        for r, ref in enumerate(refs):
            k = min(counts[r], cap)
            for name, want in zip(TABLE[:3], ref):
                assert np.array_equal(got[name][r, :k], want[:k]), (cap, r, name)
                assert np.all(got[name][r, k:] == ISENT), "%s: entries from min(count, cap) on are written" % name
            _values(got["value"][r, :k], ref[3][:k], "value")
            assert np.all(got["value"][r, k:] == SENT)
    dense, _, _, _ = run_table(eng, rows, big)
    for mask in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 1, 0), (0, 1, 0, 1)):
        got, count, info, _ = run_table(eng, rows, big, mask, n + 13, big + 11, count=mask[0] == 1)
        assert count.tolist() == (counts if mask[0] else [ISENT] * 4) and info.tolist() == crossings
        for name, on in zip(TABLE, mask):
            if on:
                _bits(got[name][:, :big], dense[name], "%s: %s = the dense call's" % (mask, name))
                assert np.all(got[name][:, big:] == (SENT if name == "value" else ISENT))
            else:
                assert np.all(got[name] == (SENT if name == "value" else ISENT)), "%s: %s was not asked for" % (mask, name)
    got, count, info, _ = run_table(eng, rows, 0, (0, 0, 0, 0), n + 13, 3)       # the counting form: cap and stride are ignored
    assert count.tolist() == counts and info.tolist() == crossings
    for name in TABLE:
        assert np.all(got[name] == (SENT if name == "value" else ISENT))
    # the filter: row, out and bounds strides with gaps
    b = np.array([some_bounds(x) for x in rows])
    for rs, os_, bs in ((n, n, 4), (n + 13, n + 7, 6), (n + 1, n, 0)):
        bb = b if bs else b[:1]
        out, info, xin, bback = run_filter(eng, rows, bb, rs, os_, bs)
        assert info.tolist() == crossings
        assert np.all(xin[:, n:] == 1e308) and np.all(out[:, n:] == SENT) and np.all(np.isnan(bback[:, 4:]))
        for r, x in enumerate(rows):
            _bits(out[r, :n], waves_ref.ref_filter(x, bb[r if bs else 0]), "filter, strides %s row %d" % ((rs, os_, bs), r))
    out32, _, _, _ = run_filter(eng, rows, b, n + 13, n + 7, 4, out_f32=True)
    assert np.all(out32[:, n:] == SENT32)
    _bits(out32[:, :n], np.stack([waves_ref.ref_filter(x, bb) for x, bb in zip(rows, b)]).astype(np.float32), "float32 with strides")


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
    want_info = [crossings[0], -1 - crossings[1], crossings[2], -1 - crossings[3], crossings[4]]
    cap = max(crossings) + 1
    got, count, info, _ = run_table(eng, bad, cap, row_stride=n + 13, wave_stride=cap + 9)
    assert info.tolist() == want_info and count.tolist() == [c + 1 for c in crossings]
    b = np.array([some_bounds(x) for x in rows])
    out, finfo, _, _ = run_filter(eng, bad, b, n + 13, n + 7, 4)
    assert finfo.tolist() == want_info
    assert np.all(out[:, n:] == SENT)
    for name in TABLE:
        assert np.all(got[name][:, cap:] == (SENT if name == "value" else ISENT)), "the gap behind %s is written" % name
    for r in (0, 2, 4):                                              # the rows either side of the NaN rows are exact
        ref = waves_ref.ref_table(rows[r])
        k = ref[0].size
        for name, want in zip(TABLE[:3], ref):
            assert np.array_equal(got[name][r, :k], want) and np.all(got[name][r, k:] == ISENT)
        _values(got["value"][r, :k], ref[3], "value")
        _bits(out[r, :n], waves_ref.ref_filter(rows[r], b[r]), "filter row %d" % r)
    with pytest.raises(P.ITDError, match=r"NaN in rows \[1, 3\]"):
        P.single_waves(bad)
    with pytest.raises(P.ITDError, match=r"NaN in rows \[1, 3\]"):
        P.single_waves(bad, cap=cap)
    with pytest.raises(P.ITDError, match=r"NaN in rows \[1, 3\]"):
        P.wave_filter(bad)


def test_an_explicit_cap(P):
    n = 1025
    rows = np.stack([family(fam, n) for fam in ("slow", "positive", "quantised")])
    counts = [waves_ref.ref_table(x)[0].size for x in rows]
    w = P.single_waves(rows, cap=counts[2] + 4)
    assert w.start.shape == (3, counts[2] + 4) and w.count.tolist() == counts
    for r in range(3):
        check_table(rows[r], w, r, "cap row %d" % r)
    with pytest.raises(ValueError, match=r"rows \[2\]"):
        P.single_waves(rows, cap=counts[2] - 1)


# ---- 6. more rows than one launch takes -----------------------------------------------------------------------------------------
def test_more_rows_than_one_grid(P):
    """65 537 rows of 5 samples: 1024 different ones, repeated (row r is base row r % 1024, so the rows on both sides of the chunk
    seam at 65 535 differ), every row with its own bounds."""
    R, n = 65537, 5
    base = np.random.default_rng(5).standard_normal((1024, n))
    idx = np.arange(R) % 1024
    w = P.single_waves(base[idx], cap=n - 1)
    lens = np.where(np.arange(1024) % 3 == 0, 1.0, 2.0)              # keep the half waves of at least 1 or 2 samples
    out = P.wave_filter(base[idx], amplitude=(0.0, np.inf), length=(lens[idx], np.inf))
    ref = [waves_ref.ref_table(x) for x in base]
    want = [np.full((1024, n - 1), -1, np.int32) for _ in range(3)] + [np.full((1024, n - 1), np.nan)]
    for r, t in enumerate(ref):
        for dst, src in zip(want, t):
            dst[r, :src.size] = src
    assert w.count.tolist() == [ref[i][0].size for i in idx]
    for got, wnt in zip((w.start, w.length, w.peak), want):
        assert np.array_equal(got, wnt[idx])
    assert np.array_equal(w.value, want[3][idx], equal_nan=True)
    fref = np.stack([waves_ref.ref_filter(x, (0.0, np.inf, l, np.inf)) for x, l in zip(base, lens)])
    _bits(out, fref[idx], "filter")


# ---- 7. the caller's stream and a captured graph: the real-time use -------------------------------------------------------------------
def test_on_a_callers_stream_and_in_a_graph(P, eng):
    import torch
    n, R = 5 * 512 + 77, 4
    fams = ("noise", "seams", "quantised", "slow")
    x_old = np.stack([family(f, n)[::-1] for f in fams])
    x_new = np.stack([family(f, n) for f in fams])
    b_new = np.array([some_bounds(x) for x in x_new])
    cap = max(waves_ref.ref_table(x)[0].size for x in np.concatenate((x_old, x_new))) + 3
    isent = np.full((R, cap), ISENT, np.int32)
    d = DevArrays(eng, x=x_old, stage=x_new, b=np.zeros((R, 4)), out=np.full((R, n), SENT), start=isent, length=isent, peak=isent,
                  value=np.full((R, cap), SENT), count=np.zeros(R, np.int32), info=np.zeros(R, np.int32))

    def enqueue(stream):
        eng.wave_filter_batch_dev(d.ptr("x"), np.float64, n, R, n, d.ptr("b"), 4, d.ptr("out"), n, False, d.ptr("info"), stream)
        eng.waves_batch_dev(d.ptr("x"), np.float64, n, R, n, d.ptr("start"), d.ptr("length"), d.ptr("peak"), d.ptr("value"), cap, cap,
                            d.ptr("count"), None, stream)

    def check(x, b, what):
        out = d.get("out")
        got = P.Waves(d.get("count"), *[d.get(k) for k in TABLE])
        for r in range(R):
            _bits(out[r], waves_ref.ref_filter(x[r], b[r]), "%s: filter row %d" % (what, r))
            ref = waves_ref.ref_table(x[r])
            k = ref[0].size
            assert got.count[r] == k
            for name, want in zip(TABLE[:3], ref):
                assert np.array_equal(getattr(got, name)[r, :k], want), (what, r, name)
                assert np.all(getattr(got, name)[r, k:] == ISENT)
            _values(got.value[r, :k], ref[3], what)
        assert d.get("info").tolist() == [int(np.count_nonzero(et.structure(r)[0])) for r in x]
    d.put("b", b_new)
    s = torch.cuda.Stream()
    eng.copy(d.ptr("x"), d.ptr("stage"), x_new.nbytes, 2, wait=False, stream=s.cuda_stream)
    enqueue(s.cuda_stream)
    s.synchronize()
    check(x_new, b_new, "on the caller's stream")
    # (the calls above were the warm-up of this size: the workspace exists, the capture allocates nothing)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            enqueue(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    y = np.stack([family(f, n) for f in ("quantised", "noise", "slow", "seams")])
    for x, b in ((x_old, np.array([some_bounds(r) for r in x_old])), (y, np.array([some_bounds(r) for r in y])), (y, np.array([COPY] * R))):
        d.put("x", x)
        d.put("b", b)                               # the bounds changed in place: the replay filters with the new ones
        d.put("out", np.full((R, n), SENT))
        for k in TABLE[:3]:
            d.put(k, isent)
        d.put("value", np.full((R, cap), SENT))
        g.replay()
        torch.cuda.synchronize()
        check(x, b, "replayed")
    d.free()


# ---- 8. consistency with the instantaneous amplitude, and the torch-tensor path ---------------------------------------------------
def test_the_amplitude_of_every_wave_is_the_instantaneous_one(P):
    n = 2 * 512 + 514
    rows = np.stack([family(fam, n) for fam in ("noise", "slow", "quantised")])
    (amp,) = P.instantaneous_batch(rows, want="amplitude")
    w = P.single_waves(rows)
    for r in range(3):
        k = int(w.count[r])
        _bits(amp[r][w.start[r, :k]], np.abs(w.value[r, :k]), "row %d" % r)
        _bits(amp[r][w.start[r, :k] + w.length[r, :k] - 1], np.abs(w.value[r, :k]), "row %d, the waves' last samples" % r)
        assert np.array_equal(np.abs(rows[r][w.peak[r, :k]]), np.abs(w.value[r, :k]))


def test_tensors_in_place(P):
    import torch
    n = 4099
    rows = np.stack([family(fam, n) for fam in ("noise", "slow", "quantised", "seams", "positive", "negzero")]).reshape(2, 3, n)
    t = torch.from_numpy(rows).cuda()
    w = P.single_waves(t)
    assert w.count.device == t.device and tuple(w.count.shape) == (2, 3) and tuple(w.start.shape) == (2, 3, int(w.count.max()))
    host = P.Waves(*[v.cpu().numpy().reshape((6,) + tuple(v.shape[2:])) for v in w])
    for r in range(6):
        check_table(rows.reshape(6, n)[r], host, r, "tensor row %d" % r)
    lo = torch.tensor([[0.0], [0.4]])
    out = P.wave_filter(t[:, 1:2, :].float(), amplitude=(lo.numpy(), np.inf), length=(3, 50), out_dtype=torch.float32)
    assert out.dtype == torch.float32 and out.device == t.device and tuple(out.shape) == (2, 1, n)
    for i in range(2):
        x = rows[i, 1].astype(np.float32).astype(np.float64)
        _bits(out[i, 0].cpu().numpy(), waves_ref.ref_filter(x, (float(lo[i, 0]), np.inf, 3, 50)).astype(np.float32), "tensor filter %d" % i)
    view = P.wave_filter(t[:, 2:3, :], length=(2, np.inf))           # row stride 3 n
    _bits(view[1, 0].cpu().numpy(), waves_ref.ref_filter(rows[1, 2], (0, np.inf, 2, np.inf)), "a strided view")
    for bad in (t[:, 1:3, :], t[:, :, ::2]):                         # no one row stride; a strided last axis
        with pytest.raises(ValueError):
            P.single_waves(bad)
        with pytest.raises(ValueError):
            P.wave_filter(bad)
