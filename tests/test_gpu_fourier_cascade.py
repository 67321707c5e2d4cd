"""The ITD-Fourier cascade (fourier_cascade in itd_fourier.inc; k_band_step, k_fourier_apply, k_fourier_sum, k_copy_rows) against
the composition of the GPU's own single calls (tests/cascade_ref.py): cubic = itd_baseline_extract_fast, select = one row through
fourier_mode_batch(.., "any"), find_extrema = pyitd_amd.find_extrema.  Every operator is held on its own
(tests/test_gpu_spline_exact.py, tests/test_gpu_fft_exact.py, tests/test_gpu_fourier_selectors.py) and runs deterministically, so
everything here is compared bit for bit: rows, every mode in order, the lean accumulators, records, rounds, the cap, mode counts.
No tolerances.

  a  single signals over every small pair of the table, full and lean; the case set is asserted from the composition's results
  b  the goldens' own x at 9000 / 450 (four-step FFT) and 2000 / 421
  c  a batch whose signals leave at different rounds (slot compaction)
  d  max_rounds = 1, 2, single and inside a batch where only some signals reach the cap
  e  the mode test at a power-of-two scale on either side of 1e-8
  f  the device entry: strides, sentinels, pads, itd_fourier_modes_f64, refusals
  g  the per-engine plan cache with the caller's own lists
  h  workspaces that grow and shrink between calls; the mode arena growing with live modes in it
"""
import ctypes

import numpy as np
import pytest

import cascade_ref as cr
from helpers import DevArrays, assert_bits_equal
from test_fourier_cpu import FOURIER

pytestmark = pytest.mark.gpu

SENT = -7.25e300
PAD = 7
OK, INVALID, NONFINITE = 0, 1, 6
# The cascade loops until a round finds no mode.  A composition here ends by itself (cascade_ref raises after 64 rounds), in fewer
# than SAFE rounds; the cascade is then called with max_rounds = SAFE, which such a signal never reaches: were the cascade to take
# another turn than its composition, the call would still end, and the comparison fail.
SAFE = 40
BATCH_PAIR = (632, 421)
# The pairs whose last band has idx = 2: no sign change of its sine, so find_extrema's list is 0, the extrapolation of 0, 0 = 0, and a
# zero.  The float64 oracle of the cubic operator takes two knots at sample 0; the GPU operator's contract does not.
REFUSED = tuple(pair for pair, idx in sorted(cr.VALID_PAIRS.items()) if 2 in idx)
BATCH_POOL = range(1, 16)


def _cubic(problem, knots, idx):
    import pyitd_amd
    return pyitd_amd.itd_baseline_extract_fast(problem, knots, idx)


def _select(row):
    from pyitd_amd.fourier import fourier_mode_batch
    modes, recs = fourier_mode_batch(row[None, :], "any")
    return modes[0], recs[0]


def _find_extrema(s):
    import pyitd_amd
    return pyitd_amd.find_extrema(s)


_plans, _refs = {}, {}


def _plan(n, sr):
    if (n, sr) not in _plans:
        _plans[(n, sr)] = cr.plan(n, sr, _find_extrema)
    return _plans[(n, sr)]


def _compose(x, sr, **kw):
    return cr.compose(x, sr, _cubic, _select, bands=kw.pop("bands", None) or _plan(x.shape[0], sr), **kw)


def _ref(pair, seed):
    """The uncapped full composition of one signal of the family, computed once and left unchanged."""
    if (pair, seed) not in _refs:
        _refs[(pair, seed)] = _free(cr.signal(pair[0], pair[1], seed), pair[1])
    return _refs[(pair, seed)]


def _free(x, sr, **kw):
    res = _compose(x, sr, **kw)
    assert res["rounds"] < SAFE - 1 and not res["capped"]
    return res


def _bits(a, b, what):
    assert_bits_equal(np.asarray(a), np.asarray(b), what)


def _same(out, info, res, lean, what):
    """One signal's result of the Python entries against its composition."""
    want = cr.outputs(res, lean)
    assert len(out) == len(want), (what, len(out), len(want))
    assert info["rounds"] == res["rounds"] and info["capped"] == res["capped"], (what, info["rounds"], res["rounds"], info["capped"])
    assert np.array_equal(info["records"], res["records"]), what
    for i, (o, w) in enumerate(zip(out, want)):
        _bits(o, w, "%s: output %d" % (what, i))


# ---- a -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(cr.VALID_PAIRS))
def test_single_signals_are_their_composition(pair):
    import pyitd_amd
    from pyitd_amd._lib import ITDError
    n, sr = pair
    lists, idxs = _plan(n, sr)
    assert tuple(idxs) == cr.VALID_PAIRS[pair]
    for seed in cr.SEEDS[pair]:
        x = cr.signal(n, sr, seed)
        if pair in REFUSED:
            # the last band's list is 0, 0, 0: the GPU's cubic operator refuses it (itd_cubic.hpp: e[0 .. idx - 1] strictly
            # increasing), so the composition has no value here, and the cascade must refuse alike, writing nothing
            assert list(lists[-1]) == [0, 0, 0]
            for call in (lambda: _cubic(x, lists[-1], idxs[-1]), lambda: pyitd_amd.itd_fourier_decomposition(x, sr, max_rounds=SAFE),
                         lambda: pyitd_amd.itd_fourier_decomposition_lean(x, sr, max_rounds=SAFE)):
                with pytest.raises(ITDError) as err:
                    call()
                assert err.value.status == INVALID, err.value.args
            continue
        res = _ref(pair, seed)
        for lean, fn in ((False, pyitd_amd.itd_fourier_decomposition), (True, pyitd_amd.itd_fourier_decomposition_lean)):
            out, info = fn(x, sr, max_rounds=SAFE, return_info=True)
            _same(out, info, res, lean, "%s seed %d lean %d" % (pair, seed, lean))


def test_the_single_signals_hold_the_cases():
    zero = deep = two = last_row = 0
    for pair, idx in sorted(cr.VALID_PAIRS.items()):
        for seed in () if pair in REFUSED else cr.SEEDS[pair]:
            res = _ref(pair, seed)
            rec = res["records"]
            zero += res["rounds"] == 0
            deep += res["rounds"] >= 3
            two += any((rec[:, 0] == r).sum() >= 2 for r in range(1, res["rounds"] + 1))
            last_row += bool((rec[:, 1] == len(idx) - 1).any())
    print("0 rounds: %d, >= 3 rounds: %d, a round with >= 2 modes: %d, a hit on the last row: %d" % (zero, deep, two, last_row))
    assert zero >= 1 and deep >= 1 and two >= 1 and last_row >= 1


# ---- b -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("long9000_sr450", "am2000_sr421"))
def test_golden_lengths_are_their_composition(name):
    import pyitd_amd
    z = np.load("%s/cascade_%s.npz" % (FOURIER, name))
    x, sr = z["x"].astype(np.float64), int(z["sample_rate"])
    res = _free(x, sr)
    assert res["rounds"] >= 2
    for lean, fn in ((False, pyitd_amd.itd_fourier_decomposition), (True, pyitd_amd.itd_fourier_decomposition_lean)):
        out, info = fn(x, sr, max_rounds=SAFE, return_info=True)
        _same(out, info, res, lean, "%s lean %d" % (name, lean))


# ---- c, d ------------------------------------------------------------------------------------------------------------------------
def _batch():
    """12 to 16 signals of one pair ordered by the round counts of their compositions: signal 0 leaves first, the last one in the
    middle, a signal leaves while a later one stays, at least three leaving rounds.  Returns (x[B, n], sample_rate, seeds)."""
    n, sr = BATCH_PAIR
    by_rounds = sorted(BATCH_POOL, key=lambda s: (_ref(BATCH_PAIR, s)["rounds"], s))
    levels = sorted({_ref(BATCH_PAIR, s)["rounds"] for s in by_rounds})
    assert len(levels) >= 3, levels
    mid = next(s for s in by_rounds if _ref(BATCH_PAIR, s)["rounds"] == levels[len(levels) // 2])
    rest = [s for s in by_rounds[1:] if s != mid]
    order = [by_rounds[0]] + rest[1::2] + rest[0::2][::-1] + [mid]          # (mixed, neither ascending nor descending)
    r = [_ref(BATCH_PAIR, s)["rounds"] for s in order]
    assert 12 <= len(order) <= 16
    assert r[0] == min(r) and min(r) < r[-1] < max(r) and len(set(r)) >= 3, r
    assert any(r[i] < r[j] for i in range(1, len(r)) for j in range(i + 1, len(r))), r          # a later slot moves down
    return np.stack([cr.signal(n, sr, s) for s in order]), sr, order


def test_batch_whose_signals_leave_at_different_rounds():
    import pyitd_amd
    xs, sr, seeds = _batch()
    for lean in (False, True):
        outs, infos = pyitd_amd.itd_fourier_decomposition_batch(xs, sr, lean=lean, max_rounds=SAFE, return_info=True)
        for b, s in enumerate(seeds):
            _same(outs[b], infos[b], _ref(BATCH_PAIR, s), lean, "signal %d (seed %d) lean %d" % (b, s, lean))


@pytest.mark.parametrize("cap", (1, 2))
def test_the_cap_single_and_inside_a_batch(cap):
    import pyitd_amd
    xs, sr, seeds = _batch()
    want = [_compose(x, sr, max_rounds=cap) for x in xs]
    capped = [w["capped"] for w in want]
    assert any(capped) and not all(capped), capped          # only some signals reach the cap
    for w, s in zip(want, seeds):
        assert w["capped"] == (_ref(BATCH_PAIR, s)["rounds"] >= cap) and (not w["capped"] or w["rounds"] == cap)
    for lean in (False, True):
        outs, infos = pyitd_amd.itd_fourier_decomposition_batch(xs, sr, lean=lean, max_rounds=cap, return_info=True)
        for b in range(len(seeds)):
            _same(outs[b], infos[b], want[b], lean, "cap %d signal %d lean %d" % (cap, b, lean))
    b = capped.index(True)
    for lean, fn in ((False, pyitd_amd.itd_fourier_decomposition), (True, pyitd_amd.itd_fourier_decomposition_lean)):
        out, info = fn(xs[b], sr, max_rounds=cap, return_info=True)
        assert info["capped"] and info["rounds"] == cap
        _same(out, info, want[b], lean, "cap %d single lean %d" % (cap, lean))


# ---- e -------------------------------------------------------------------------------------------------------------------------
def test_the_mode_test_at_a_power_of_two_on_either_side_of_1e_8():
    import pyitd_amd
    pair = (230, 230)
    seed = next(s for s in range(16) if _ref(pair, s)["rounds"] >= 1)
    x, res = cr.signal(pair[0], pair[1], seed), _ref(pair, seed)
    assert res["records"][0, 0] == 1
    A = float(np.max(np.abs(res["modes"][0])))
    c = 2.0 ** np.floor(np.log2(2e-8 / A))
    assert 1e-8 < c * A <= 2e-8, (c, A)
    hit, miss = _free(c * x, pair[1]), _free(c / 2 * x, pair[1])
    assert hit["rounds"] >= 1 and np.array_equal(hit["records"][0], res["records"][0])          # that hit, in the first run
    assert 1e-8 < float(np.max(np.abs(hit["modes"][0]))) <= 2e-8
    assert miss["rounds"] == 0 and not miss["modes"]                                            # and not in the second
    for xs, want, what in ((c * x, hit, "above"), (c / 2 * x, miss, "below")):
        for lean, fn in ((False, pyitd_amd.itd_fourier_decomposition), (True, pyitd_amd.itd_fourier_decomposition_lean)):
            out, info = fn(xs, pair[1], max_rounds=SAFE, return_info=True)
            _same(out, info, want, lean, "%s the threshold, lean %d" % (what, lean))


# ---- the C entries -------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def eng():
    import pyitd_amd
    e = pyitd_amd.Engine(4096, 1, 0)
    yield e
    e.close()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _flat(lists, idxs):
    return np.ascontiguousarray(np.concatenate(lists), dtype=np.int64), np.asarray(idxs, dtype=np.int64)


def _modes(eng, n, count, with_modes=True):
    recs = np.full((count, 8), -1, np.int32)
    modes = np.full((count, n), SENT) if with_modes else None
    rc = eng._L.itd_fourier_modes_f64(eng._h, _p(modes), count, _p(recs), 1)
    return rc, modes, recs


def _host_call(eng, xs, sr, bands, lean=False, cap=SAFE):
    """itd_fourier_cascade_host_f64 with the caller's lists: a dict of rows, acc, rounds, capped, counts, recs, modes."""
    B, n = xs.shape
    knots, idx = _flat(*bands)
    K = idx.shape[0]
    rows, acc = np.full((B, K + 1, n), SENT), (np.full((B, K, n), SENT) if lean else None)
    rounds, capped, counts = np.full(B, -1, np.int32), np.full(B, -1, np.int32), np.full(B, -1, np.int64)
    rc = eng._L.itd_fourier_cascade_host_f64(eng._h, _p(np.ascontiguousarray(xs)), n, B, float(sr), K, _p(knots), _p(idx), int(lean), cap,
                                             _p(rows), _p(acc), _p(rounds), _p(capped), _p(counts))
    assert rc == OK, rc
    rc, modes, recs = _modes(eng, n, int(counts.sum()), not lean)
    assert rc == OK, rc
    return dict(rows=rows, acc=acc, rounds=rounds, capped=capped, counts=counts, recs=recs, modes=modes)


def _same_call(got, wants, lean, what):
    """A C call's result over B signals against their compositions; the records' order is round, then signal, then row."""
    recs = got["recs"]
    key = [tuple(r[[1, 0, 2]]) for r in recs]
    assert key == sorted(key), "%s: the modes are not in the order round, signal, row" % what
    for b, w in enumerate(wants):
        sel = np.flatnonzero(recs[:, 0] == b)
        assert got["rounds"][b] == w["rounds"] and bool(got["capped"][b]) == w["capped"] and got["counts"][b] == len(w["modes"]) == sel.size, \
            (what, b, got["rounds"][b], w["rounds"], got["counts"][b], len(w["modes"]))
        assert np.array_equal(recs[sel, 1:], w["records"]), (what, b)
        _bits(got["rows"][b], w["rows"], "%s: rows of signal %d" % (what, b))
        if lean:
            _bits(got["acc"][b], w["acc"] if w["acc"] is not None else cr.lean_acc(w), "%s: acc of signal %d" % (what, b))
        else:
            for j, m in zip(sel, w["modes"]):
                _bits(got["modes"][j], m, "%s: mode %d" % (what, j))


def _same_bits(a, b, what):
    for k in ("rows", "acc", "modes"):
        if a[k] is not None or b[k] is not None:
            _bits(a[k], b[k], "%s: %s" % (what, k))
    for k in ("rounds", "capped", "counts", "recs"):
        assert np.array_equal(a[k], b[k]), (what, k)


# ---- f -------------------------------------------------------------------------------------------------------------------------
DEV_PAIR = (211, 421)


def _dev_signals():
    seeds = sorted(cr.SEEDS[DEV_PAIR], key=lambda s: -_ref(DEV_PAIR, s)["rounds"])[:3]
    assert _ref(DEV_PAIR, seeds[0])["rounds"] >= 1
    return np.stack([cr.signal(DEV_PAIR[0], DEV_PAIR[1], s) for s in seeds]), [_ref(DEV_PAIR, s) for s in seeds]


def _dev_call(eng, xs, sr, bands, lean, cap=SAFE, stride=None, with_acc=True, batch=None):
    """itd_fourier_cascade_f64 on x laid out with `stride`, sentinels in the gaps and a pad behind every buffer.  The input and
    every pad must come back untouched."""
    B, n = xs.shape
    stride = n + PAD if stride is None else stride
    knots, idx = _flat(*bands)
    K = idx.shape[0]
    x = np.full(B * max(stride, n) + PAD, SENT)
    for b in range(B):
        x[b * stride:b * stride + n] = xs[b]
    arrays = dict(x=x, rows=np.full(B * (K + 1) * n + PAD, SENT), acc=np.full(B * K * n + PAD, SENT))
    d = DevArrays(eng, **arrays)
    try:
        rounds, capped, counts = np.full(B, -1, np.int32), np.full(B, -1, np.int32), np.full(B, -1, np.int64)
        rc = eng._L.itd_fourier_cascade_f64(eng._h, d.ptr("x"), n, B if batch is None else batch, stride, float(sr), K, _p(knots), _p(idx),
                                            int(lean), cap, d.ptr("rows"), d.ptr("acc") if (lean and with_acc) else None,
                                            _p(rounds), _p(capped), _p(counts))
        rows, acc = d.get("rows"), d.get("acc")
        _bits(d.get("x"), x, "the input was changed")
        assert (rows[B * (K + 1) * n:] == SENT).all() and (acc[B * K * n:] == SENT).all(), "written past the rows or the accumulators"
        if rc != OK:
            assert (rows == SENT).all() and (acc == SENT).all(), "a refused call wrote its outputs"
            return rc, None
        if not lean:
            assert (acc == SENT).all(), "a full call wrote the accumulators"
        got = dict(rows=rows[:B * (K + 1) * n].reshape(B, K + 1, n), acc=acc[:B * K * n].reshape(B, K, n) if lean else None,
                   rounds=rounds, capped=capped, counts=counts)
        rc2, got["modes"], got["recs"] = _modes(eng, n, int(counts.sum()), not lean)
        assert rc2 == OK
        return rc, got
    finally:
        d.free()


def test_device_entry_with_strides_sentinels_and_pads(eng):
    xs, wants = _dev_signals()
    sr, bands = DEV_PAIR[1], _plan(*DEV_PAIR)
    for lean in (False, True):
        rc, got = _dev_call(eng, xs, sr, bands, lean)
        assert rc == OK
        _same_call(got, wants, lean, "device entry, lean %d" % lean)
        _same_bits(got, _host_call(eng, xs, sr, bands, lean), "device against host entry, lean %d" % lean)


def test_modes_entry_to_device_partial_counts_and_after_a_lean_call(eng):
    xs, wants = _dev_signals()
    n, sr, bands = DEV_PAIR[0], DEV_PAIR[1], _plan(*DEV_PAIR)
    rc, got = _dev_call(eng, xs, sr, bands, False)
    assert rc == OK
    total = int(got["counts"].sum())
    assert total >= 2
    d = DevArrays(eng, modes=np.full(total * n + PAD, SENT))
    try:
        recs = np.full((total, 8), -1, np.int32)
        assert eng._L.itd_fourier_modes_f64(eng._h, d.ptr("modes"), total, _p(recs), 0) == OK
        m = d.get("modes")
        assert (m[total * n:] == SENT).all()
        _bits(m[:total * n].reshape(total, n), got["modes"], "to_host = 0 against to_host = 1")
        assert np.array_equal(recs, got["recs"])
    finally:
        d.free()
    part = total - 1
    modes, recs = np.full((total, n), SENT), np.full((total, 8), -1, np.int32)
    assert eng._L.itd_fourier_modes_f64(eng._h, _p(modes), part, _p(recs), 1) == OK
    _bits(modes[:part], got["modes"][:part], "the first `count` modes")
    assert (modes[part:] == SENT).all() and np.array_equal(recs[:part], got["recs"][:part]) and (recs[part:] == -1).all()
    assert eng._L.itd_fourier_modes_f64(eng._h, _p(modes), total + 1, _p(recs), 1) == INVALID
    rc, lean = _dev_call(eng, xs, sr, bands, True)
    assert rc == OK and int(lean["counts"].sum()) == total
    modes = np.full((total, n), SENT)
    assert eng._L.itd_fourier_modes_f64(eng._h, _p(modes), total, _p(recs), 1) == INVALID
    assert (modes == SENT).all()
    assert np.array_equal(lean["recs"], got["recs"])          # records alone


def test_device_entry_refusals(eng):
    xs, _ = _dev_signals()
    n, sr, bands = DEV_PAIR[0], DEV_PAIR[1], _plan(*DEV_PAIR)
    bad = xs.copy()
    bad[1, n // 2] = np.nan
    assert _dev_call(eng, bad, sr, bands, False)[0] == NONFINITE
    assert _dev_call(eng, xs, sr, bands, False, stride=n - 1)[0] == INVALID
    assert _dev_call(eng, xs, sr, bands, True, with_acc=False)[0] == INVALID
    assert _dev_call(eng, xs, sr, bands, False, cap=0)[0] == INVALID
    assert _dev_call(eng, xs, sr, bands, False)[0] == OK


# ---- g -------------------------------------------------------------------------------------------------------------------------
def _moved(lists, idxs):
    """Every interior knot (the sine's sign changes) moved up by one where the list stays increasing (from the right, so a
    neighbour's move is seen); the extrapolated index and the zero behind it stay."""
    out, moved = [], 0
    for kn, idx in zip(lists, idxs):
        kn = kn.copy()
        for j in range(idx - 2, 0, -1):
            if kn[j] + 1 < kn[j + 1]:
                kn[j] += 1
                moved += 1
        assert (np.diff(kn[:idx]) > 0).all()
        out.append(kn)
    assert moved >= len(idxs)
    return out, list(idxs)


def test_the_plan_cache_with_the_callers_own_lists(eng):
    n, sr = 422, 842
    x = cr.signal(n, sr, next(s for s in cr.SEEDS[(n, sr)] if _ref((n, sr), s)["rounds"] >= 1))[None, :]
    first, second = _plan(n, sr), _moved(*_plan(n, sr))
    wants = [_free(x[0], sr, bands=first), _free(x[0], sr, bands=second)]
    assert not np.array_equal(wants[0]["rows"], wants[1]["rows"])
    a = _host_call(eng, x, sr, first)
    b = _host_call(eng, x, sr, second)
    c = _host_call(eng, x, sr + 1.0, first)
    again = _host_call(eng, x, sr, first)
    _same_call(a, wants[:1], False, "the band_plan lists")
    _same_call(b, wants[1:], False, "same n, sample rate, idx and lengths, other knots")
    _same_call(c, wants[:1], False, "the first lists under another sample rate")
    _same_bits(again, a, "the first call repeated")


# ---- h -------------------------------------------------------------------------------------------------------------------------
def test_workspaces_between_a_large_batch_and_a_longer_signal(eng):
    xs, sr, seeds = _batch()
    z = np.load("%s/cascade_am2000_sr421.npz" % FOURIER)
    long_x, long_sr = z["x"].astype(np.float64)[None, :], int(z["sample_rate"])
    bands, long_bands = _plan(*BATCH_PAIR), _plan(long_x.shape[1], long_sr)
    for lean in (False, True):
        a = _host_call(eng, xs, sr, bands, lean)
        _host_call(eng, long_x, long_sr, long_bands, lean)
        b = _host_call(eng, xs, sr, bands, lean)
        _same_bits(a, b, "a batch of 16, one longer signal, the batch again; lean %d" % lean)
        _same_call(a, [_ref(BATCH_PAIR, s) for s in seeds], lean, "the batch, lean %d" % lean)


def test_the_mode_arena_grows_with_live_modes_in_it():
    import pyitd_amd
    xs, sr, seeds = _batch()
    wants = [_ref(BATCH_PAIR, s) for s in seeds]
    per_round = [sum(int((w["records"][:, 0] == r).sum()) for w in wants) for r in range(1, max(w["rounds"] for w in wants) + 1)]
    assert sum(per_round) >= 12 and len(per_round) >= 3, per_round          # the arena is reserved round by round
    fresh = pyitd_amd.Engine(4096, 1, 0)          # its arena starts empty
    try:
        _host_call(fresh, xs[:2], sr, _plan(*BATCH_PAIR), lean=True)
        _same_call(_host_call(fresh, xs, sr, _plan(*BATCH_PAIR)), wants, False, "a full call after a lean one")
    finally:
        fresh.close()
