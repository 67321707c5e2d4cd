"""What tests/test_gpu_batch_ops.py stands on, checked without a GPU and without the code under test:
  * the plain rules (oracle/numpy_itd.py: baseline_extract(plain_nan=True), valley_flags / peak_flags / knot_flags) equal the C oracle
    bit for bit on every finite signal family at every length the GPU file uses — so on rows that hold a NaN they are the same
    expressions with nothing but the NaN treatment taken away;
  * every generator of tests/batch_cases.py delivers what its GPU test relies on (conditions on the inputs);
  * the comparisons of tests/batch_cases.py pass a correct result set built from the oracle and raise on the same set with one
    defect at a time.
"""
import numpy as np
import pytest

import batch_cases as bc
from helpers import assert_bits_equal, fuzz_signal
from oracle import cpu_oracle, numpy_itd

LENGTHS = sorted(set(bc.EXTRACT_N + bc.DETECT_N + bc.NAN_N + (bc.ASYNC_N,) + tuple(n for n, _ in bc.CHUNK_CASES)))


def _many_groups_rows():
    return np.concatenate((bc.family_rows("thirds", bc.MANY_GROUPS_N), bc.family_rows("sparse_mid", bc.MANY_GROUPS_N, knot_tile=bc.MANY_GROUPS_TILE)))


def _tile_counts(flags):
    n = flags.size
    tiles = (n + bc.TILE - 1) // bc.TILE
    return np.bincount(np.flatnonzero(flags) // bc.TILE, minlength=tiles)


# ---- the plain rules = the C oracle on finite input -----------------------------------------------------------------------------
def _plain_equals_oracle(x, what):
    rot, base, kn, _ = cpu_oracle.itd_baseline_extract(x, want_knots=True)
    p_rot, p_base, m, p_kn = numpy_itd.baseline_extract(x, plain_nan=True)
    assert m == len(kn) and np.array_equal(p_kn, kn), what
    assert_bits_equal(p_rot, rot, what + " rotation")
    assert_bits_equal(p_base, base, what + " baseline")
    valleys, peaks = np.flatnonzero(numpy_itd.valley_flags(x)), np.flatnonzero(numpy_itd.peak_flags(x))
    assert np.array_equal(valleys, cpu_oracle.detect_peaks(x)), what
    assert np.array_equal(peaks, cpu_oracle.detect_peaks(x, matlab=True)), what
    assert np.array_equal(np.union1d(valleys, peaks), cpu_oracle.knots(x)), what
    for mode in range(5):
        assert np.array_equal(bc.plain_detect(x, mode), bc.oracle_detect(x, mode))


@pytest.mark.parametrize("n", LENGTHS)
def test_plain_rules_are_the_c_oracle_on_finite_rows(n):
    x, names = bc.mixed_batch(n, len(bc.FAMILIES), seed=n)
    assert np.all(np.isfinite(x))
    for b, name in enumerate(names):
        _plain_equals_oracle(x[b], "%s n=%d" % (name, n))
    for row in bc.zero_cross_rows(n, 2):
        _plain_equals_oracle(row, "zero crossings n=%d" % n)


def test_plain_rules_are_the_c_oracle_on_the_many_group_rows():
    for b, row in enumerate(_many_groups_rows()):
        _plain_equals_oracle(row, "many groups row %d" % b)


def test_default_restatement_still_refuses_nan():
    x = bc.nan_batch(513)
    with pytest.raises(ValueError):
        numpy_itd.baseline_extract(x[bc.NAN_ROWS[0]])
    assert len(numpy_itd.baseline_extract(x[0])) == 3


# ---- conditions on the inputs ---------------------------------------------------------------------------------------------------
def test_family_order_puts_a_dense_row_on_both_sides_of_every_sparse_row():
    dense = ("int16", "zigzag", "thirds")
    for k, name in enumerate(bc.FAMILIES):
        if name in bc.SPARSE:
            assert bc.FAMILIES[k - 1] in dense and bc.FAMILIES[k + 1] in dense
    x, names = bc.mixed_batch(1025, 30)
    assert names[:11] == list(bc.FAMILIES) and names[11] == bc.FAMILIES[0]
    assert len({row.tobytes() for row in x}) == 30, "every row is its own draw"


@pytest.mark.parametrize("n", LENGTHS + [bc.MANY_GROUPS_N])
def test_zigzag_rows(n):
    if n == bc.MANY_GROUPS_N:
        n = 3 * bc.GROUP + 7
    x = bc.family_rows("zigzag", n, 2, seed=1)
    rng = np.random.default_rng([1, n, bc.FAMILIES.index("zigzag")])
    assert np.array_equal(x[0], fuzz_signal(rng, 6, n)), "helpers.fuzz_signal kind 6"
    for row in x:
        f = numpy_itd.knot_flags(row)
        assert f.sum() == n - 2
        full = _tile_counts(f)[:n // bc.TILE]                # (sample 0 and sample n - 1 are never knots)
        assert np.all(full >= bc.TILE - 2) and bc.TILE - 2 > bc.RANK_CAP0


@pytest.mark.parametrize("n", LENGTHS)
def test_knot_free_and_plateau_rows(n):
    for name in ("const", "linspace"):
        for row in bc.family_rows(name, n, 3):
            assert not numpy_itd.knot_flags(row).any(), name
    lead = bc.family_rows("lead_plateau", n, 3)
    trail = bc.family_rows("trail_plateau", n, 3)
    for row in lead:
        assert row[0] == row[1] and np.all(np.isfinite(row))
        rot, base = cpu_oracle.itd_baseline_extract(row)
        assert np.isnan(base[0]), "the first segment's slope is 0 / 0: a NaN baseline from finite input"
    for row in trail:
        assert row[-1] == row[-2] and np.all(np.isfinite(row))
    ex = bc.family_rows("extreme", n, 40)
    assert np.all(np.isfinite(ex)) and np.abs(ex).max() > 1e50 and (np.abs(ex).max(axis=1) < 1e-50).any()


@pytest.mark.parametrize("n", LENGTHS)
def test_sparse_rows(n):
    tiles = (n + bc.TILE - 1) // bc.TILE
    a, b = bc.sparse_mid_window(n)
    for row in bc.family_rows("sparse_mid", n, 3):
        k = np.flatnonzero(numpy_itd.knot_flags(row))
        assert k.size >= 1 and k[0] >= a - 1 and k[-1] <= b
        assert k.size >= b - a - 1, "every sample of the window is a knot"
        if tiles >= 3:
            c = _tile_counts(numpy_itd.knot_flags(row))
            assert np.count_nonzero(c) == 1 and c[tiles // 2] > 0 and c[0] == 0 and c[-1] == 0
    (a0, b0), (a1, b1) = bc.sparse_ends_windows(n)
    for row in bc.family_rows("sparse_ends", n, 3):
        k = np.flatnonzero(numpy_itd.knot_flags(row))
        assert k.size >= 1 and k[0] <= a0 and k[-1] >= b1 - 1
        assert np.all((k <= b0) | (k >= a1 - 1))
        if tiles >= 4:
            c = _tile_counts(numpy_itd.knot_flags(row))
            assert c[0] > 0 and np.all(c[1:-2] == 0) and c[-2] + c[-1] > 0


def test_many_group_rows():
    dense, sparse = _many_groups_rows()
    n = bc.MANY_GROUPS_N
    assert (n + bc.GROUP - 1) // bc.GROUP == 67 > 64, "the group-sum loops take their second trip"
    c = _tile_counts(numpy_itd.knot_flags(sparse))
    t = bc.MANY_GROUPS_TILE
    assert t // 64 == 65 and np.flatnonzero(c).tolist() == [t] and c[t] >= 479
    assert c[:t].size >= 64 and c[t + 1:].size >= 64 and not c[:t].any() and not c[t + 1:].any()
    cd = _tile_counts(numpy_itd.knot_flags(dense))
    assert np.all(cd > 0) and len(set(cd.tolist())) > 20, "a dense row whose tiles differ in their counts"


@pytest.mark.parametrize("n", bc.NAN_N)
def test_nan_rows(n):
    x = bc.nan_batch(n)
    assert x.shape == (bc.NAN_BATCH, n)
    pos = bc.nan_positions(n)
    for b in range(bc.NAN_BATCH):
        assert np.flatnonzero(np.isnan(x[b])).tolist() == sorted(pos.get(b, []))
    for b in bc.NAN_ROWS:
        assert 0 < b < bc.NAN_BATCH - 1 and b - 1 not in bc.NAN_ROWS and b + 1 not in bc.NAN_ROWS
    ends, inner = pos[bc.NAN_ROWS[0]], pos[bc.NAN_ROWS[1]]
    assert 0 in ends and n - 1 in ends and n // 2 in inner
    if n > bc.TILE:
        assert bc.TILE - 1 in ends and bc.TILE in ends
    if n >= 16:
        q = n // 4
        assert {q, q + 1, q + 2} <= set(inner) and q + 3 < n // 2
    plain = [len(bc.plain_detect(x[b], 0)) for b in bc.NAN_ROWS]
    branch = [len(cpu_oracle.knots(x[b])) for b in bc.NAN_ROWS]
    assert plain != branch, "the two rule sets must differ on a NaN row, or no test can tell them apart"
    for b in bc.NAN_ROWS:                                   # a NaN sample and both its neighbours are never knots
        k = bc.plain_detect(x[b], 0)
        for p in pos[b]:
            assert not np.isin([p - 1, p, p + 1], k).any()
        _, _, m, kn = numpy_itd.baseline_extract(x[b], plain_nan=True)
        assert m == len(k) and np.array_equal(kn, k)


@pytest.mark.parametrize("n", [n for n in LENGTHS if n > bc.TILE + 2])
def test_zero_cross_rows(n):
    for row in bc.zero_cross_rows(n, 3):
        assert np.any((row == 0) & ~np.signbit(row)) and np.any((row == 0) & np.signbit(row))
        k = bc.oracle_detect(row, 4)
        for t in range(bc.TILE, n - 2, bc.TILE):
            assert {t - 2, t - 1, t} <= set(k.tolist()), "crossings before, across and behind the seam at %d" % t


def test_rows_to_check_at_the_chunk_boundary():
    for n, batch in bc.CHUNK_CASES:
        assert batch > bc.CHUNK
        rows = bc.chunk_rows_to_check(batch)
        assert set(range(bc.CHUNK - 64, batch)) <= set(rows.tolist())
        assert np.count_nonzero(rows < bc.CHUNK - 64) >= 1900 and rows.max() == batch - 1 and np.all(np.diff(rows) > 0)


# ---- the comparisons are sensitive ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def result_set():
    """A correct result set of the first chunk-boundary case: what the entries must leave in the buffers, built from the oracle."""
    n, batch = bc.CHUNK_CASES[0]
    x, _ = bc.mixed_batch(n, batch)
    ref = bc.extract_reference(x)
    strides = (n, n + 1, n)
    info = np.full(batch + bc.PAD, bc.ISENT, np.int32)
    info[:batch] = ref[2]
    got = dict(x=bc.layout(x, strides[0]), rot=bc.layout(ref[0], strides[1]), base=bc.layout(ref[1], strides[2]), info=info)
    return n, batch, x, ref, strides, got


def _row(buf, b, stride, n):
    return buf[b * stride:b * stride + n]


def _defects(n, batch, strides, r0):
    """name -> a function that plants the defect in a copy of the result set; r0: a row of the last chunk"""
    def swap(g):
        a, b = _row(g["rot"], r0, strides[1], n), _row(g["rot"], r0 + 1, strides[1], n)
        assert not np.array_equal(a, b)
        t = a.copy(); a[:] = b; b[:] = t

    def count(g):
        g["info"][r0] += 1

    def gap(g):
        g["rot"][r0 * strides[1] + n] = 0.0

    def behind(g):
        g["base"][batch * strides[2]] = 0.0

    def chunk_row(g):
        a, b = _row(g["base"], r0, strides[2], n), _row(g["base"], r0 - bc.CHUNK, strides[2], n)
        assert r0 - bc.CHUNK >= 0 and not np.array_equal(a, b)
        a[:] = b

    def ulp(g):
        a = _row(g["base"], r0, strides[2], n)
        a[n // 2] = np.nextafter(a[n // 2], np.inf)

    def zero_sign(g):
        a = _row(g["rot"], r0, strides[1], n)
        a[3] = -a[3] if a[3] == 0.0 else np.nextafter(a[3], -np.inf)

    def input_written(g):
        g["x"][r0 * strides[0] + 1] += 1.0

    return dict(swap=swap, count=count, gap=gap, behind=behind, chunk_row=chunk_row, ulp=ulp, zero_sign=zero_sign, input_written=input_written)


def test_extraction_comparison_passes_the_oracle_and_raises_on_every_defect(result_set):
    n, batch, x, ref, strides, got = result_set
    some = bc.chunk_rows_to_check(batch)
    part = tuple(r[some] for r in ref)
    bc.check_extract(got, x, ref, strides, "correct set")
    bc.check_extract(got, x, part, strides, "correct set, some rows", rows=some)
    r0 = next(b for b in range(bc.CHUNK + 2, batch) if b % len(bc.FAMILIES) == bc.FAMILIES.index("zigzag"))   # of the last chunk
    for name, plant in _defects(n, batch, strides, r0).items():
        bad = {k: v.copy() for k, v in got.items()}
        plant(bad)
        with pytest.raises(AssertionError):
            bc.check_extract(bad, x, ref, strides, name)
        with pytest.raises(AssertionError):
            bc.check_extract(bad, x, part, strides, name, rows=some)
    without_info = dict(got, info=None)
    bc.check_extract(without_info, x, ref, strides, "info not passed")


@pytest.mark.parametrize("stride_extra", (0, 7))
def test_detection_comparison_passes_the_oracle_and_raises_on_every_defect(stride_extra):
    n = 513
    x, names = bc.mixed_batch(n, len(bc.FAMILIES))
    stride = n - 2 + stride_extra
    zig = names.index("zigzag")
    for mode in range(5):
        lists, info = ref = bc.detect_reference(x, mode)
        idx = bc.blank(len(lists), n - 2, stride, bc.ISENT, dtype=np.int32)
        for b, k in enumerate(lists):
            idx[b * stride:b * stride + len(k)] = k
        inf = np.full(len(lists) + bc.PAD, bc.ISENT, np.int32)
        inf[:len(lists)] = info
        got = dict(idx=idx, info=inf)
        bc.check_detect(got, ref, n, stride, "correct set")
        bc.check_detect(dict(idx=idx, info=None), ref, n, stride, "lists only")
        bc.check_detect(dict(idx=None, info=inf), ref, n, stride, "info only")
        junk = idx.copy()                                   # entries [count, n - 2) of a slot are unspecified
        for b, k in enumerate(lists):
            junk[b * stride + len(k):b * stride + n - 2] = 77
        bc.check_detect(dict(idx=junk, info=inf), ref, n, stride, "unspecified tail")
        b = zig if mode != 4 else 0
        m = len(lists[b])
        assert m >= 2

        def shifted(g):
            g["idx"][b * stride:b * stride + m] = np.roll(g["idx"][b * stride:b * stride + m], 1)

        def swapped(g):
            c = b + 2
            assert not np.array_equal(lists[b], lists[c])
            s0, s1 = g["idx"][b * stride:(b + 1) * stride].copy(), g["idx"][c * stride:(c + 1) * stride].copy()
            g["idx"][b * stride:(b + 1) * stride], g["idx"][c * stride:(c + 1) * stride] = s1, s0

        def count(g):
            g["info"][b] -= 1

        def behind(g):
            g["idx"][len(lists) * stride] = 0

        def info_behind(g):
            g["info"][len(lists)] = 0

        plants = [shifted, swapped, count, behind, info_behind]
        if stride_extra:
            plants.append(lambda g: g["idx"].__setitem__(b * stride + n - 2, 5))
        for plant in plants:
            bad = dict(idx=idx.copy(), info=inf.copy())
            plant(bad)
            with pytest.raises(AssertionError):
                bc.check_detect(bad, ref, n, stride, "defect")
    # the zigzag row fills its slot to the last entry at idx_stride = n - 2
    assert len(bc.detect_reference(x[zig], 0)[0][0]) == n - 2


def test_nan_equals_nan_but_nothing_else():
    a = np.array([[1.0, np.nan, 0.0]])
    buf = bc.layout(a, 3)
    bc.assert_rows(buf, np.array([[1.0, -np.nan, 0.0]]), 3, "any NaN = any NaN")
    for other in ([1.0, np.inf, 0.0], [1.0, np.nan, -0.0]):
        with pytest.raises(AssertionError):
            bc.assert_rows(buf, np.array([other]), 3, "defect")
