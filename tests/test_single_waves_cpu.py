"""Single-wave analysis (itd_waves_batch_*, itd_wave_filter_batch_*, pyitd_amd.single_waves, pyitd_amd.wave_filter) as far as it goes
without a GPU: the entries refuse a NULL engine, the wrappers refuse bad arguments before any engine exists, and the algebra the
kernels implement (itd_waves.hpp: one record per 512-sample tile, a forward and a backward scan of maps along the row with the
earlier index winning a tie, the table and the filter assembled tile by tile) is written out here in numpy and equals waves_ref,
the statement of the definitions that knows of no tiles.
"""
import numpy as np
import pytest

import waves_ref
from oracle import exact_tfe as et
from test_oracle_exact_tfe import FAMILIES, family, with_crossings

TILE = 512
NONE = 2 ** 31 - 1
LENGTHS = (3, 5, 64, 65, 511, 512, 513, 514, 1024, 1025, 1537, 1538, 20011)


def tied_row(n):
    """Two half waves (one for n < 5); the first one's maximum 0.75 stands at two samples 600 apart — in two different tiles once
    the row is long enough — and again behind the crossing with the other sign; everything else is below 0.6."""
    rng = np.random.default_rng(n)
    x = with_crossings(n, [n // 2] if n >= 5 else [], rng, mag=0.1 + 0.5 * rng.random(n))
    for p in (n // 8, n // 8 + 600, n // 8 + 1100, n // 2 + 2, n // 2 + 602):
        if p < n:
            x[p] = np.sign(x[p]) * 0.75
    return x


def rows_of(n):
    return [(fam, family(fam, n)) for fam in FAMILIES] + [("tied", tied_row(n))]


def test_entries_refuse_a_null_engine():
    from pyitd_amd import _lib
    L = _lib.load()
    for fn in (L.itd_waves_batch_f64, L.itd_waves_batch_f32):
        assert fn(None, None, 5, 1, 5, None, None, None, None, 4, 4, None, None, None) == 1       # ITD_ERR_INVALID_ARG
    for fn in (L.itd_wave_filter_batch_f64, L.itd_wave_filter_batch_f32):
        assert fn(None, None, 5, 1, 5, None, 0, None, 5, 0, None, None) == 1


def test_wrappers_refuse_bad_arguments_before_any_engine(monkeypatch):
    import pyitd_amd
    from pyitd_amd import _place, batch

    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(batch, "_engine_for", no_engine)
    monkeypatch.setattr(_place, "DeviceBuffer", no_engine)
    good = np.zeros((2, 5))
    for bad, kw in ((np.zeros(5), {}), (np.zeros((2, 2)), {}), (np.zeros((2, 5), np.int32), {}), (good, {"cap": 0}), (good, {"cap": -3}),
                    (good, {"cap": 2.5})):
        with pytest.raises(ValueError):
            pyitd_amd.single_waves(bad, **kw)
    nan = float("nan")
    for bad, kw in ((np.zeros(5), {}), (np.zeros((2, 2)), {}), (np.zeros((2, 5), np.int32), {}), (good, {"amplitude": (2.0, 1.0)}),
                    (good, {"length": (7, 3)}), (good, {"amplitude": (nan, 1.0)}), (good, {"length": (0, nan)}),
                    (good, {"amplitude": (np.array([0.0, 2.0]), np.array([1.0, 1.0]))}),            # lo > hi in one row
                    (good, {"amplitude": (np.zeros(3), np.ones(3))}),                               # 3 bounds, 2 rows
                    (np.zeros((2, 3, 5)), {"length": (np.zeros((3, 2)), 9.0)}),
                    (good, {"amplitude": 1.0}), (good, {"out_dtype": np.int16})):
        with pytest.raises(ValueError):
            pyitd_amd.wave_filter(bad, **kw)


def test_the_bounds_broadcast_to_the_leading_axes():
    from pyitd_amd.batch import _wave_bounds
    b = _wave_bounds((0, np.inf), (0, np.inf), (2, 3))
    assert b.shape == (4,) and b.tolist() == [0.0, np.inf, 0.0, np.inf]
    b = _wave_bounds((np.array([[0.0], [1.0]]), 5.0), (2, np.array([7, 8, 9])), (2, 3))
    assert b.shape == (6, 4) and b.dtype == np.float64
    assert b[:, 0].tolist() == [0, 0, 0, 1, 1, 1] and b[:, 3].tolist() == [7, 8, 9, 7, 8, 9]
    assert np.all(b[:, 1] == 5.0) and np.all(b[:, 2] == 2.0)


# ---- the numpy model of k_wave_records, k_wave_carry, k_wave_table and k_wave_filter ----------------------------------------
def pick(a, b):
    """The larger magnitude; on equal magnitudes the smaller index (a pair is (m, i); the identity (0, NONE))."""
    return a if (a[0] > b[0] or (a[0] == b[0] and a[1] <= b[1])) else b


IDENT = (0, (0.0, NONE), 0, 0)


def then(f, g):
    """Maps (reset, pair, pos, cnt): f, then g."""
    return (f[0] | g[0], g[1] if g[0] else pick(f[1], g[1]), g[2] if g[0] else f[2], f[3] + g[3])


def app(f, s):
    """A map on a state (pair, pos, cnt)."""
    return (f[1] if f[0] else pick(s[0], f[1]), f[2] if f[0] else s[1], s[2] + f[3])


def arg_first_max(a, s):
    """(max, the absolute index of its first occurrence) of the magnitudes a that start at sample s; empty: the identity."""
    if a.size == 0:
        return (0.0, NONE)
    k = int(np.argmax(a))                                            # numpy's argmax is the first one
    return (float(a[k]), s + k)


def records(x):
    n = x.size
    cross = et.structure(x)[0]
    out = []
    for s in range(0, n, TILE):
        a = np.abs(x[s:s + TILE])
        k = np.flatnonzero(cross[s:s + TILE])
        if k.size == 0:
            out.append(dict(c=0, head=arg_first_max(a, s), tail=(0.0, NONE), first=None, last=None))
        else:
            out.append(dict(c=k.size, head=arg_first_max(a[:k[0] + 1], s), tail=arg_first_max(a[k[-1] + 1:], s + k[-1] + 1),
                            first=s + int(k[0]), last=s + int(k[-1])))
    return cross, out


def scan(maps, state, chunk):
    """in[] of every position: the maps composed chunk by chunk the way the workgroup does (a tree inside a chunk, the running
    state from chunk to chunk) — any bracketing gives the same if the operator is associative."""
    ins = []
    for b in range(0, len(maps), chunk):
        part = maps[b:b + chunk]
        pre = [IDENT]
        for f in part:
            pre.append(then(pre[-1], f))
        # the chunk's total once more as a balanced tree: another bracketing of the same product
        level = list(part)
        while len(level) > 1:
            level = [then(level[i], level[i + 1]) if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
        assert level[0] == pre[-1]
        ins += [app(p, state) for p in pre[:-1]]
        state = app(pre[-1], state)
    return ins, state


def carry(rec, n, chunk=4):
    fmaps = [(1, r["tail"], r["last"] + 1, r["c"]) if r["c"] else (0, r["head"], 0, 0) for r in rec]
    bmaps = [(1, r["head"], r["first"], 0) if r["c"] else (0, r["head"], 0, 0) for r in rec][::-1]
    fin, total = scan(fmaps, ((0.0, NONE), 0, 0), chunk)
    bout, _ = scan(bmaps, ((0.0, NONE), n - 1, 0), chunk)
    bout = bout[::-1]
    fwd = [dict(pair=pick(v[0], r["head"]), start=v[1], prefix=v[2]) for v, r in zip(fin, rec)]
    bwd = [dict(pair=pick(r["tail"], v[0]), end=v[1]) for v, r in zip(bout, rec)]
    return fwd, bwd, total[2] + 1


def tile_waves(x, cross, t, rec, fwd, bwd):
    """The half waves 0 .. c of tile t as (start, end, pair): 0 and c from the carries, the others from the tile alone."""
    s = t * TILE
    k = s + np.flatnonzero(cross[s:s + TILE])
    c = rec["c"]
    if c == 0:
        return [(fwd["start"], bwd["end"], pick(fwd["pair"], bwd["pair"]))]
    waves = [(fwd["start"], int(k[0]), fwd["pair"])]
    for r in range(1, c):
        lo, hi = int(k[r - 1]) + 1, int(k[r])
        waves.append((lo, hi, arg_first_max(np.abs(x[lo:hi + 1]), lo)))
    waves.append((int(k[-1]) + 1, bwd["end"], bwd["pair"]))
    return waves


def model(x, bounds):
    n = x.size
    cross, rec = records(x)
    fwd, bwd, count = carry(rec, n)
    start, length, peak = (np.full(count, -1, np.int32) for _ in range(3))
    out = np.empty(n)
    for t, r in enumerate(rec):
        waves = tile_waves(x, cross, t, r, fwd[t], bwd[t])
        ends_here = waves[:-1] if t < len(rec) - 1 else waves         # the row's last tile writes the row's last half wave
        for rank, (lo, hi, (m, i)) in enumerate(ends_here):
            k = fwd[t]["prefix"] + rank
            assert start[k] == -1, "half wave %d written twice" % k
            start[k], length[k], peak[k] = lo, hi - lo + 1, i
        s = t * TILE
        hw = np.zeros(min(TILE, n - s), np.int64)
        hw[1:] = np.cumsum(cross[s:s + TILE])[:-1]
        A = np.array([w[2][0] for w in waves])[hw]
        ln = np.array([float(w[1] - w[0] + 1) for w in waves])[hw]
        with np.errstate(invalid="ignore"):
            keep = (bounds[0] <= A) & (A <= bounds[1]) & (bounds[2] <= ln) & (ln <= bounds[3])
        out[s:s + TILE] = np.where(keep, x[s:s + TILE], 0.0)
    assert np.all(start >= 0)
    return start, length, peak, x[peak], out


def some_bounds(x):
    """Bounds that cut through the row's own amplitudes and lengths (both sides inclusive at existing values)."""
    _, length, _, value = waves_ref.ref_table(x)
    a = np.sort(np.abs(value))
    ln = np.sort(length)
    return (a[a.size // 3], a[-1 - a.size // 4], float(ln[ln.size // 4]), float(ln[-1 - ln.size // 5]))


@pytest.mark.parametrize("n", LENGTHS)
def test_the_tile_algebra_equals_the_definitions(n):
    for fam, x in rows_of(n):
        rs, rl, rp, rv = waves_ref.ref_table(x)
        b = some_bounds(x)
        start, length, peak, value, out = model(x, b)
        for got, want, what in ((start, rs, "start"), (length, rl, "length"), (peak, rp, "peak")):
            assert np.array_equal(got, want), (fam, n, what)
        assert np.array_equal(value.view(np.uint64), rv.view(np.uint64)), (fam, n, "value")
        assert np.array_equal(out.view(np.uint64), waves_ref.ref_filter(x, b).view(np.uint64)), (fam, n, "filter")
        assert np.array_equal(model(x, (0.0, np.inf, 0.0, np.inf))[4].view(np.uint64), x.view(np.uint64)), (fam, n, "copy")


def test_the_reference_on_a_known_row():
    x = np.array([-0.5, 0.25, 1.0, 1.0, -2.0, -0.5, 3.0, 0.0, 0.0, -1.0, -1.0])    # (0 -> 1 is no crossing; 3, 0, 0, -1 is one half wave)
    start, length, peak, value = waves_ref.ref_table(x)
    assert start.tolist() == [0, 4, 6] and length.tolist() == [4, 2, 5] and peak.tolist() == [2, 4, 6]
    assert value.tolist() == [1.0, -2.0, 3.0]
    assert waves_ref.ref_filter(x, (2.0, 2.5, 0, np.inf)).tolist() == [0, 0, 0, 0, -2.0, -0.5, 0, 0, 0, 0, 0]
    assert waves_ref.ref_filter(x, (0, np.inf, 4, 4)).tolist() == [-0.5, 0.25, 1.0, 1.0, 0, 0, 0, 0, 0, 0, 0]
    assert [v.tolist() for v in waves_ref.ref_table(np.array([1.0, 1.0, -1.0]))] == [[0, 2], [2, 1], [0, 2], [1.0, -1.0]]   # n-2 -> n-1 is one
    assert not np.signbit(waves_ref.ref_filter(x, (5.0, 9.0, 0, np.inf))).any()     # +0.0 everywhere
    assert np.all(waves_ref.ref_filter(x, (np.nan, np.inf, 0, np.inf)) == 0)
    z = waves_ref.ref_table(np.zeros(7))
    assert [v.tolist() for v in z] == [[0], [7], [0], [0.0]]
    t = tied_row(20011)
    _, _, peak, value = waves_ref.ref_table(t)
    assert peak.tolist() == [20011 // 8, 20011 // 2 + 2] and np.abs(value).tolist() == [0.75, 0.75]
    assert peak[0] // TILE != (peak[0] + 600) // TILE


def test_the_scan_operator_is_associative_with_the_earlier_index_winning():
    """k_wave_carry scans the maps in parallel: composition is associative, IDENT its identity, and among equal magnitudes the
    smaller index survives whichever operand holds it."""
    rng = np.random.default_rng(5)

    def draw():
        reset = int(rng.integers(0, 2))
        pair = (float(rng.integers(0, 4)), int(rng.integers(0, 6)))
        return (reset, pair, int(rng.integers(0, 9)) if reset else 0, int(rng.integers(0, 3)))
    for _ in range(3000):
        f, g, h = draw(), draw(), draw()
        assert then(then(f, g), h) == then(f, then(g, h))
        s = ((float(rng.integers(0, 4)), int(rng.integers(0, 6))), int(rng.integers(0, 9)), int(rng.integers(0, 3)))
        assert app(then(f, g), s) == app(g, app(f, s))
        assert then(IDENT, f) == f and then(f, IDENT) == f
    assert pick((1.0, 7), (1.0, 3)) == (1.0, 3) and pick((1.0, 3), (1.0, 7)) == (1.0, 3)
    assert pick((0.0, 5), (0.0, NONE)) == (0.0, 5) and pick((0.0, NONE), (0.0, 5)) == (0.0, 5)
