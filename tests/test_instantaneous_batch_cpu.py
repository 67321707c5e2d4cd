"""The batched instantaneous step (itd_instantaneous_batch_*, pyitd_amd.instantaneous_batch) as far as it goes without a GPU:
the entries refuse a NULL engine, the wrapper refuses bad arguments before any engine exists, and the amplitude algebra the
kernels implement (itd_tfe_batch.hpp: one record per 512-sample tile, a scan along the row, the tile's own segmented maxima) is
written out here in numpy and equals oracle.exact_tfe.structure's amplitudes and crossing totals.
"""
import numpy as np
import pytest

from oracle import exact_tfe as et
from test_oracle_exact_tfe import FAMILIES, family

TILE = 512
LENGTHS = (3, 5, 64, 65, 511, 512, 513, 514, 1024, 1025, 1537, 1538, 20011, 60000)


def test_entries_refuse_a_null_engine():
    from pyitd_amd import _lib
    L = _lib.load()
    for fn in (L.itd_instantaneous_batch_f64, L.itd_instantaneous_batch_f32):
        assert fn(None, None, 5, 1, 5, None, None, None, 5, 0, None, None) == 1          # ITD_ERR_INVALID_ARG


def test_wrapper_refuses_bad_arguments_before_any_engine(monkeypatch):
    import pyitd_amd
    from pyitd_amd import _place, batch

    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(batch, "_engine_for", no_engine)
    monkeypatch.setattr(_place, "DeviceBuffer", no_engine)
    good = np.zeros((2, 5))
    for bad, kw in ((np.zeros(5), {}), (np.zeros((2, 2)), {}), (np.zeros((2, 5), np.int32), {}), (good, {"want": ("amplitude", "energy")}),
                    (good, {"want": ()}), (good, {"out_dtype": np.int16})):
        with pytest.raises(ValueError):
            pyitd_amd.instantaneous_batch(bad, **kw)


def test_leading_axes_collapse_to_one_row_stride_or_not():
    from pyitd_amd._place import _row_stride
    assert _row_stride((3, 4, 10), (40, 10, 1)) == 10
    assert _row_stride((3, 4, 10), (52, 13, 1)) == 13            # padded rows, still one stride
    assert _row_stride((3, 4, 10), (100, 13, 1)) is None         # padded planes
    assert _row_stride((3, 1, 10), (13, 999, 1)) == 13           # an axis of one element has no stride
    assert _row_stride((1, 10), (7, 1)) == 10
    assert _row_stride((3, 10), (9, 1)) is None                  # overlapping rows
    assert _row_stride((3, 10), (20, 2)) is None                 # a strided last axis


# ---- the numpy model of k_inst_records, k_inst_carry and k_inst_apply's amplitudes ---------------------------------------
def records(x):
    """Per tile: c, head, tail (itd_tfe_batch.hpp)."""
    n = x.size
    cross = np.zeros(n, bool)
    cross[1:n - 1] = ((x[1:-1] > 0) & (x[2:] < 0)) | ((x[1:-1] < 0) & (x[2:] > 0))
    tiles = (n + TILE - 1) // TILE
    c, head, tail = np.zeros(tiles, np.int64), np.zeros(tiles), np.zeros(tiles)
    for t in range(tiles):
        s = t * TILE
        a = np.abs(x[s:s + TILE])
        k = np.flatnonzero(cross[s:s + TILE])
        c[t] = k.size
        if k.size == 0:
            head[t] = a.max()
        else:
            head[t] = a[:k[0] + 1].max()
            tail[t] = a[k[-1] + 1:].max() if k[-1] + 1 < a.size else 0.0
    return cross, c, head, tail


def carry(c, head, tail):
    tiles = c.size
    inn, out = np.zeros(tiles), np.zeros(tiles)
    for t in range(1, tiles):
        inn[t] = tail[t - 1] if c[t - 1] > 0 else max(inn[t - 1], head[t - 1])
    for t in range(tiles - 2, -1, -1):
        out[t] = head[t + 1] if c[t + 1] > 0 else max(head[t + 1], out[t + 1])
    a_head = np.maximum(np.maximum(inn, head), np.where(c == 0, out, 0.0))
    a_tail = np.maximum(tail, out)
    return a_head, a_tail


def apply_amplitudes(x, cross, c, a_head, a_tail):
    n = x.size
    amp = np.empty(n)
    for t in range(c.size):
        s = t * TILE
        xs = x[s:s + TILE]
        hw = np.zeros(xs.size, np.int64)                             # the half wave's number inside the tile
        hw[1:] = np.cumsum(cross[s:s + TILE])[:-1]
        seg = np.zeros(TILE + 1)
        np.maximum.at(seg, hw, np.abs(xs))
        amp[s:s + TILE] = np.where(hw == 0, a_head[t], np.where(hw == c[t], a_tail[t], seg[hw]))
    return amp


def model(x):
    cross, c, head, tail = records(x)
    a_head, a_tail = carry(c, head, tail)
    return apply_amplitudes(x, cross, c, a_head, a_tail), int(c.sum())


@pytest.mark.parametrize("fam", FAMILIES)
def test_the_amplitude_algebra_equals_the_exact_structure(fam):
    for n in LENGTHS:
        x = family(fam, n)
        cross, _, amp, _, _, _ = et.structure(x)
        got, total = model(x)
        assert total == np.count_nonzero(cross), (fam, n)
        assert np.array_equal(got.view(np.uint64), amp.view(np.uint64)), (fam, n)


def test_the_scan_operator_is_associative():
    """k_inst_carry scans maps s -> (reset ? m : max(s, m)) in parallel: composition is associative, {0, 0} its identity."""
    rng = np.random.default_rng(5)

    def then(f, g):
        return (f[0] | g[0], g[1] if g[0] else max(f[1], g[1]))

    def app(f, s):
        return f[1] if f[0] else max(s, f[1])
    for _ in range(2000):
        f, g, h = ((int(rng.integers(0, 2)), float(rng.integers(0, 6))) for _ in range(3))
        assert then(then(f, g), h) == then(f, then(g, h))
        s = float(rng.integers(0, 6))
        assert app(then(f, g), s) == app(g, app(f, s))
        assert then((0, 0.0), f) == f and then(f, (0, 0.0)) == f
