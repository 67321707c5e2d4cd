"""The batched single-level entries of the C ABI (include/pyitd_hip.h) and their wrappers (pyitd_amd/batch.py) against references,
called directly on device buffers of the tests' own: sentinel-filled outputs with a pad behind them, every comparison bit for bit
(any NaN = any NaN) or integer-exact, the input read back and compared byte for byte.  Which reference each entry is held to:
  itd_baseline_extract_batch_f64   finite rows: oracle.cpu_oracle.itd_baseline_extract, info = its knot count;
                                   rows that hold a NaN: the plain rules, oracle.numpy_itd.baseline_extract(plain_nan=True),
                                   info = -1 - its count
  itd_detect_batch_f64             finite rows: test_gpu_device_entries.oracle_detect (modes 0-2 cpu_oracle.knots / .detect_peaks,
                                   mode 3 cpu_oracle.extrema_cpp, mode 4 the crossings of cpu_oracle.find_extrema);
                                   rows that hold a NaN: modes 0-2 the flags of oracle.numpy_itd (knot_flags / valley_flags /
                                   peak_flags), modes 3 and 4 the same C loops (plain IEEE comparisons), info = -1 - count
  pyitd_amd.itd_baseline_extract_batch          every row, NaN rows too: cpu_oracle.itd_baseline_extract (the reference's NaN branch)
  pyitd_amd.count_knots_batch / detect_knots_batch   every row: oracle_detect (NaN branch in modes 0-2, plain in modes 3 and 4)
tests/test_batch_ops_cpu.py holds the plain rules to the C oracle on finite input, the generators to what is relied on here, and
the comparisons (tests/batch_cases.py) to raising on one defect at a time.

The gaps these tests close (each named again at its test):
  1. the chunk loop of extract_batch above 65535 signals           test_extraction_across_the_chunk_boundary
  2. per-signal indexing beyond one tile and one group, a sparse    test_extraction_lengths_and_strides, test_many_groups
     signal next to a dense one
  3. strides: odd, unequal, padded; the gaps between rows           test_extraction_lengths_and_strides, test_detection_all_modes
  4. modes 1, 2 and 4, the lists of modes 3 and 4, the exact fit    test_detection_all_modes
  5. rows that hold a NaN against a statement of the plain rules    test_nan_rows_follow_the_plain_rules, test_wrappers_on_nan_rows
  6. the caller's stream, a captured graph, beside a decomposition  test_batched_entries_on_the_callers_stream,
                                                                    test_batched_entries_are_graph_capturable,
                                                                    test_batched_entries_beside_a_decomposition
"""
import numpy as np
import pytest

import batch_cases as bc
from batch_cases import ISENT, PAD, SENT
from helpers import DevArrays, assert_bits_equal, sines_noise
from oracle import cpu_oracle

pytestmark = pytest.mark.gpu
OK, INVALID = 0, 1
STRIDE_SETS = {"tight": (0, 0, 0), "odd": (1, 3, 2), "padded": (37, 37, 37)}      # added to n: (x, rot, base)


@pytest.fixture(scope="module")
def eng():
    import pyitd_amd
    e = pyitd_amd.Engine(bc.MANY_GROUPS_N, 1, 0)
    yield e
    e.close()


def _info_blank(B):
    return np.full(B + PAD, ISENT, np.int32)


def _extract_bufs(eng, x, strides, **extra):
    B, n = x.shape
    return DevArrays(eng, x=bc.layout(x, strides[0]), rot=bc.blank(B, n, strides[1]), base=bc.blank(B, n, strides[2]),
                     info=_info_blank(B), **extra)


def _extract_call(eng, d, B, n, strides, with_info=True, stream=None):
    return eng._L.itd_baseline_extract_batch_f64(eng._h, d.ptr("x"), n, B, strides[0], d.ptr("rot"), strides[1], d.ptr("base"),
                                                 strides[2], d.ptr("info") if with_info else None, stream)


def _read_extract(d, with_info=True):
    got = dict(x=d.get("x"), rot=d.get("rot"), base=d.get("base"), info=d.get("info"))
    if not with_info:
        assert np.all(got["info"] == ISENT), "info_dev was not passed"
        got["info"] = None
    return got


def _extract(eng, x, strides, with_info=True):
    d = _extract_bufs(eng, x, strides)
    rc = _extract_call(eng, d, x.shape[0], x.shape[1], strides, with_info)
    got = _read_extract(d, with_info)
    d.free()
    assert rc == OK
    return got


def _detect_bufs(eng, x, x_stride, idx_stride, **extra):
    B, n = x.shape
    return DevArrays(eng, x=bc.layout(x, x_stride), idx=bc.blank(B, n - 2, idx_stride, ISENT, dtype=np.int32), info=_info_blank(B), **extra)


def _detect_call(eng, d, B, n, x_stride, mode, idx_stride, lists=True, info=True, stream=None, idx="idx", inf="info"):
    return eng._L.itd_detect_batch_f64(eng._h, d.ptr("x"), n, B, x_stride, mode, d.ptr(idx) if lists else None, idx_stride,
                                       d.ptr(inf) if info else None, stream)


def _read_detect(d, lists=True, info=True, idx="idx", inf="info"):
    got = dict(idx=d.get(idx), info=d.get(inf))
    if not lists:
        assert np.all(got["idx"] == ISENT), "idx_dev was not passed"
        got["idx"] = None
    if not info:
        assert np.all(got["info"] == ISENT), "info_dev was not passed"
        got["info"] = None
    return got


# ---- a. extraction: lengths x strides (gaps 2 and 3) -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", bc.EXTRACT_N)
def test_extraction_lengths_and_strides(eng, n):
    """Every family in one batch (a dense row on both sides of every sparse one) at one, two, 64, 65 and 66 tiles per signal: one
    and two groups.  An odd x_stride flips the 16-byte alignment from row to row; the three strides differ; every sentinel between
    and behind the rows stays."""
    x, names = bc.mixed_batch(n, len(bc.FAMILIES), seed=n)
    B = x.shape[0]
    ref = bc.extract_reference(x)
    for key, add in STRIDE_SETS.items():
        strides = tuple(n + a for a in add)
        for with_info in (True, False):
            got = _extract(eng, x, strides, with_info)
            bc.check_extract(got, x, ref, strides, "n=%d %s strides%s" % (n, key, "" if with_info else ", no info"))
    # batch = 1: the strides are not used and may be anything
    for b in (names.index("zigzag"), names.index("sparse_mid")):
        one = tuple(r[b:b + 1] for r in ref)
        got = _extract(eng, x[b:b + 1], (n - 1, 1, 0))
        bc.check_extract(got, x[b:b + 1], one, (n - 1, 1, 0), "n=%d batch 1, strides below n" % n)


# ---- b. many groups (gap 2) ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_groups():
    n = bc.MANY_GROUPS_N
    rows = {"dense": bc.family_rows("thirds", n)[0], "sparse": bc.family_rows("sparse_mid", n, knot_tile=bc.MANY_GROUPS_TILE)[0]}
    ref = {k: dict(extract=bc.extract_reference(r), m0=bc.detect_reference(r, 0), m3=bc.detect_reference(r, 3)) for k, r in rows.items()}
    return rows, ref


@pytest.mark.parametrize("order", (("dense", "sparse"), ("sparse", "dense")))
def test_many_groups(eng, many_groups, order):
    """Two signals of 67 groups (66 * 64 * 512 + 5 samples) in one call: the group-sum loops of k_compact and k_batch_totals take
    their second trip, and the sparse signal's only knots sit in group 65 with 4160 empty tiles before them and 64 behind, its
    dense neighbour directly before (after) it in memory: a neighbour search that left the signal would find the neighbour's knots."""
    rows, ref = many_groups
    n = bc.MANY_GROUPS_N
    x = np.stack([rows[k] for k in order])
    want = tuple(np.concatenate([ref[k]["extract"][j] for k in order]) for j in range(3))
    strides = (n, n, n)
    bc.check_extract(_extract(eng, x, strides), x, want, strides, "many groups %s" % (order,))
    d = _detect_bufs(eng, x, n, n - 2, cnt=_info_blank(2))
    for mode, key in ((0, "m0"), (3, "m3")):
        dref = ([ref[k][key][0][0] for k in order], np.concatenate([ref[k][key][1] for k in order]))
        d.put("idx", d.host["idx"]); d.put("info", d.host["info"]); d.put("cnt", d.host["cnt"])
        assert _detect_call(eng, d, 2, n, n, mode, n - 2) == OK
        assert _detect_call(eng, d, 2, n, n, mode, 0, lists=False, inf="cnt") == OK
        bc.check_detect(_read_detect(d), dref, n, n - 2, "many groups %s mode %d lists" % (order, mode))
        bc.check_detect(dict(idx=None, info=d.get("cnt")), dref, n, n - 2, "many groups %s mode %d counts" % (order, mode))
    assert_bits_equal(d.get("x"), d.host["x"], "the input is left alone")
    d.free()


# ---- c. the chunk boundary (gap 1) -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunk24():
    n, batch = bc.CHUNK_CASES[0]
    x, _ = bc.mixed_batch(n, batch)
    return n, batch, x, bc.extract_reference(x)


def test_extraction_across_the_chunk_boundary_one_tile(eng, chunk24):
    """65535 + 37 signals run as two chunks in a workspace carved for the first chunk's size, the last chunk's pointers offset by
    65535 rows: every row against the oracle.  Then 40 signals of the same length on the same engine: a later, smaller call in
    the arena grown for the larger one."""
    n, batch, x, ref = chunk24
    strides = (n, n + 1, n)
    bc.check_extract(_extract(eng, x, strides), x, ref, strides, "%d signals of %d" % (batch, n))
    small = tuple(r[:40] for r in ref)
    bc.check_extract(_extract(eng, x[:40], strides), x[:40], small, strides, "40 signals of %d after the large call" % n)


def test_extraction_across_the_chunk_boundary_two_tiles(eng):
    """The same with two tiles per signal (515 samples, 65535 + 3 signals): every row of the last chunk, every row within 64 of the
    chunk boundary and 2000 seeded others against the oracle; every stride gap of the whole buffer."""
    n, batch = bc.CHUNK_CASES[1]
    x, _ = bc.mixed_batch(n, batch)
    rows = bc.chunk_rows_to_check(batch)
    ref = bc.extract_reference(x[rows])
    strides = (n, n + 1, n)
    bc.check_extract(_extract(eng, x, strides), x, ref, strides, "%d signals of %d" % (batch, n), rows=rows)
    small = bc.extract_reference(x[:40])
    bc.check_extract(_extract(eng, x[:40], strides), x[:40], small, strides, "40 signals of %d after the large call" % n)


def test_detection_takes_65535_signals_and_refuses_65536(eng, chunk24):
    n, _, x, ref = chunk24
    d = DevArrays(eng, x=bc.layout(x[:bc.CHUNK + 1], n), info=_info_blank(bc.CHUNK + 1))
    assert _detect_call(eng, d, bc.CHUNK + 1, n, n, 0, 0, lists=False) == INVALID
    assert np.all(d.get("info") == ISENT), "a refused call wrote info"
    assert _detect_call(eng, d, bc.CHUNK, n, n, 0, 0, lists=False) == OK
    info = d.get("info")
    d.free()
    assert info[bc.CHUNK] == ISENT
    bc.assert_info(np.concatenate((info[:bc.CHUNK], _info_blank(0))), ref[2][:bc.CHUNK], "counts of 65535 signals")


# ---- d. detection, all five modes (gaps 3 and 4) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", bc.DETECT_N)
def test_detection_all_modes(eng, n):
    """Lists + info, lists only and info only (the count-only kernels) under every predicate.  idx_stride = n - 2 is the exact fit:
    the zigzag rows (one of them the last of the batch) fill their slots to the last entry, so the next row's first entry and the
    sentinel behind the last row tell an overrun.  Modes 3 and 4 build lists with another kernel pair than they count with."""
    x = np.concatenate((bc.mixed_batch(n, len(bc.FAMILIES), seed=n + 1)[0], bc.zero_cross_rows(n, 2), bc.family_rows("zigzag", n, 1, seed=3)))
    B = x.shape[0]
    xs = n + 1
    refs = [bc.detect_reference(x, mode) for mode in range(5)]
    assert len(refs[0][0][-1]) == n - 2
    for idx_stride in (n - 2, n + 5):
        d = _detect_bufs(eng, x, xs, idx_stride)
        for mode in range(5):
            for lists, info in ((True, True), (True, False), (False, True)):
                d.put("idx", d.host["idx"]); d.put("info", d.host["info"])
                assert _detect_call(eng, d, B, n, xs, mode, idx_stride if lists else 0, lists, info) == OK
                bc.check_detect(_read_detect(d, lists, info), refs[mode], n, idx_stride,
                                "n=%d mode %d idx_stride %d lists=%s info=%s" % (n, mode, idx_stride, lists, info))
        assert_bits_equal(d.get("x"), d.host["x"], "the input is left alone")
        d.free()


# ---- e. rows that hold a NaN (gap 5) -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", bc.NAN_N)
def test_nan_rows_follow_the_plain_rules(eng, n):
    """NaNs at sample 0, at n - 1, on both sides of a tile seam, at one interior sample and as a run of three, in rows between finite
    rows: info = -1 - count and the rows of the plain rules — the same expressions, a comparison with a NaN false, nothing
    overwritten with +inf — for the NaN rows, the C oracle for the others."""
    x = bc.nan_batch(n)
    B = x.shape[0]
    ref = bc.extract_reference(x)
    assert np.all((ref[2] < 0) == np.isin(np.arange(B), bc.NAN_ROWS))
    strides = (n + 1, n + 3, n + 2)
    bc.check_extract(_extract(eng, x, strides), x, ref, strides, "NaN rows n=%d" % n)
    d = _detect_bufs(eng, x, n + 1, n - 2)
    for mode in range(5):
        dref = bc.detect_reference(x, mode)
        for lists in (True, False):
            d.put("idx", d.host["idx"]); d.put("info", d.host["info"])
            assert _detect_call(eng, d, B, n, n + 1, mode, n - 2 if lists else 0, lists) == OK
            bc.check_detect(_read_detect(d, lists), dref, n, n - 2, "NaN rows n=%d mode %d lists=%s" % (n, mode, lists))
    assert_bits_equal(d.get("x"), d.host["x"], "the input is left alone")
    d.free()


@pytest.mark.parametrize("n", bc.NAN_N)
def test_wrappers_on_nan_rows(n):
    """pyitd_amd.batch: NaN rows come back under the reference's NaN branch for the extraction and for modes 0-2 (the wrappers run
    them again through the single-signal operators), under the plain rules for modes 3 and 4; finite rows as ever."""
    from pyitd_amd.batch import count_knots_batch, detect_knots_batch, itd_baseline_extract_batch
    x = bc.nan_batch(n)
    keep = x.copy()
    rot, base, counts = itd_baseline_extract_batch(x, want_counts=True)
    for b in range(x.shape[0]):
        r, bs, kn, _ = cpu_oracle.itd_baseline_extract(x[b], want_knots=True)
        assert_bits_equal(rot[b], r, "wrapper n=%d row %d rotation" % (n, b))
        assert_bits_equal(base[b], bs, "wrapper n=%d row %d baseline" % (n, b))
        assert counts[b] == len(kn)
    for mode in range(5):
        cnt = count_knots_batch(x, mode)
        lists = detect_knots_batch(x, mode)
        for b in range(x.shape[0]):
            want = bc.oracle_detect(x[b], mode)
            if mode >= 3:
                assert np.array_equal(want, bc.plain_detect(x[b], mode))
            assert cnt[b] == len(want), (n, mode, b)
            assert lists[b].dtype == np.int64 and np.array_equal(lists[b], want), (n, mode, b)
    assert_bits_equal(x, keep, "the caller's array is not written")


# ---- f. order and asynchrony (gap 6) -----------------------------------------------------------------------------------------------
ASYNC_B = 5


def _async_bufs(eng, x, **extra):
    n = x.shape[1]
    return _extract_bufs(eng, x, (n + 37,) * 3, idx=bc.blank(ASYNC_B, n - 2, n + 5, ISENT, dtype=np.int32), kinfo=_info_blank(ASYNC_B),
                         cinfo=_info_blank(ASYNC_B), **extra)


def _async_calls(eng, d, n, stream):
    """extraction, mode 0 lists and mode 3 counts back to back on one stream, nothing synchronised in between"""
    xs = n + 37
    assert _extract_call(eng, d, ASYNC_B, n, (xs,) * 3, stream=stream) == OK
    assert _detect_call(eng, d, ASYNC_B, n, xs, 0, n + 5, stream=stream, inf="kinfo") == OK
    assert _detect_call(eng, d, ASYNC_B, n, xs, 3, 0, lists=False, stream=stream, inf="cinfo") == OK


def _async_check(d, x, what):
    n = x.shape[1]
    bc.check_extract(_read_extract(d), x, bc.extract_reference(x), (n + 37,) * 3, what)
    bc.check_detect(_read_detect(d, inf="kinfo"), bc.detect_reference(x, 0), n, n + 5, what + " mode 0 lists")
    bc.check_detect(dict(idx=None, info=d.get("cinfo")), bc.detect_reference(x, 3), n, n + 5, what + " mode 3 counts")


def test_batched_entries_on_the_callers_stream(eng):
    """The input is filled by a device copy queued on a side stream, the three calls follow on that stream (extraction and detection
    work in different arenas) and the results are read after that stream alone has been synchronised: they are the new data's."""
    import torch
    n = bc.ASYNC_N
    new, old = bc.mixed_batch(n, ASYNC_B, seed=1)[0], bc.mixed_batch(n, ASYNC_B, seed=2)[0]
    s = torch.cuda.Stream()
    d = _async_bufs(eng, old, stage=bc.layout(new, n + 37))
    eng.copy(d.ptr("x"), d.ptr("stage"), d.host["stage"].nbytes, 2, wait=False, stream=s.cuda_stream)
    _async_calls(eng, d, n, s.cuda_stream)
    s.synchronize()
    _async_check(d, new, "on the caller's stream")
    d.free()


def test_batched_entries_are_graph_capturable():
    """After one warm call of each entry at the same (n, batch) — the arenas allocate at the first call of a size — extraction and
    detection are captured into one graph and replayed on two fresh data sets.  (No larger call of either kind may follow on the
    engine while the graph is in use: pyitd_hip.h.)"""
    import pyitd_amd
    import torch
    n = bc.ASYNC_N
    e = pyitd_amd.Engine(1 << 12, 1, 0)
    x0 = bc.mixed_batch(n, ASYNC_B, seed=3)[0]
    d = _async_bufs(e, x0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _async_calls(e, d, n, side.cuda_stream)                              # warm-up
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            _async_calls(e, d, n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for seed in (4, 5):
        x = bc.mixed_batch(n, ASYNC_B, seed=seed)[0]
        d.put("x", bc.layout(x, n + 37))
        for k in ("rot", "base", "info", "idx", "kinfo", "cinfo"):
            d.put(k, d.host[k])
        g.replay()
        torch.cuda.synchronize()
        _async_check(d, x, "graph replay seed %d" % seed)
    del g
    d.free()
    e.close()


def test_batched_entries_beside_a_decomposition(eng):
    """On one stream: a decomposition, the batched extraction and detection of other data, then itd_get_summary: the batched
    entries work in arenas of their own, the decomposition's rows are the oracle's and so are theirs."""
    import torch
    n, m = 70000, 5
    sig = sines_noise(n, seed=9, dtype=np.float64)
    x = bc.mixed_batch(bc.ASYNC_N, ASYNC_B, seed=6)[0]
    d = _async_bufs(eng, x, sig=sig, rows=np.zeros((m + 2, n)))
    s = torch.cuda.Stream()
    eng.decompose_dev(d.ptr("sig"), np.float64, n, 1, n, m, d.ptr("rows"), None, s.cuda_stream)
    _async_calls(eng, d, bc.ASYNC_N, s.cuda_stream)
    summary = eng.summary(1)
    s.synchronize()
    ref = cpu_oracle.itd(sig, m)
    nr = int(summary["n_rows"][0])
    assert nr == ref["rows"].shape[0] and ("natural", "timeout")[int(summary["stop"][0])] == ref["stop"]
    assert_bits_equal(d.get("rows")[:nr], ref["rows"], "the decomposition's rows")
    _async_check(d, x, "beside a decomposition")
    d.free()


# ---- g. refused arguments ------------------------------------------------------------------------------------------------------------
def test_refused_arguments(eng):
    n, B = 100, 2
    x = bc.mixed_batch(n, B)[0]
    d = _extract_bufs(eng, x, (n, n, n), idx=bc.blank(B, n - 2, n - 2, ISENT, dtype=np.int32))
    L, h = eng._L, eng._h
    px, pr, pb, pi, pk = (d.ptr(k) for k in ("x", "rot", "base", "info", "idx"))

    def ext(e=h, x=px, n=n, batch=B, xs=n, rot=pr, rs=n, base=pb, bs=n):
        return L.itd_baseline_extract_batch_f64(e, x, n, batch, xs, rot, rs, base, bs, pi, None)

    def det(e=h, x=px, n=n, batch=B, xs=n, mode=0, idx=pk, stride=n - 2, info=pi):
        return L.itd_detect_batch_f64(e, x, n, batch, xs, mode, idx, stride, info, None)

    for bad in (dict(e=None), dict(x=None), dict(rot=None), dict(base=None), dict(n=2), dict(batch=0), dict(xs=n - 1), dict(rs=n - 1),
                dict(bs=n - 1)):
        assert ext(**bad) == INVALID, bad
    for bad in (dict(e=None), dict(x=None), dict(idx=None, info=None), dict(n=2), dict(batch=0), dict(xs=n - 1), dict(stride=n - 3),
                dict(mode=-1), dict(mode=5)):
        assert det(**bad) == INVALID, bad
    assert np.all(d.get("rot") == SENT) and np.all(d.get("base") == SENT), "a refused call wrote a row"
    assert np.all(d.get("info") == ISENT) and np.all(d.get("idx") == ISENT), "a refused call wrote info or a list"
    assert ext() == OK and det() == OK and det(idx=None) == OK and det(info=None) == OK      # the same calls, valid
    d.free()
