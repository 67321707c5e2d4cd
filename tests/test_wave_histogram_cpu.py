"""The half waves' joint amplitude-length histogram (itd_wave_hist_batch_*, pyitd_amd.wave_histogram) as far as it goes without a
GPU: the numpy statement of the definition (wave_hist_ref) on a row whose cells are known by hand and its two invariants on random
rows, the wrapper's refusals before any engine exists, how the edges broadcast, and the entries refusing a NULL engine.
"""
import numpy as np
import pytest

import wave_hist_ref as wh
import waves_ref
from test_oracle_exact_tfe import FAMILIES, family
from test_single_waves_cpu import tied_row


def test_entries_refuse_a_null_engine():
    from pyitd_amd import _lib
    L = _lib.load()
    for fn in (L.itd_wave_hist_batch_f64, L.itd_wave_hist_batch_f32):
        assert fn(None, None, 5, 1, 5, None, 0, 4, None, 0, 4, 512, None, None, 16, None, None, None) == 1      # ITD_ERR_INVALID_ARG


def test_the_reference_on_a_known_row():
    # half waves: [0, 4) A 1.0 peak 2; [4, 6) A 2.0 peak 4; [6, 11) A 3.0 peak 6 (test_single_waves_cpu's known row)
    x = np.array([-0.5, 0.25, 1.0, 1.0, -2.0, -0.5, 3.0, 0.0, 0.0, -1.0, -1.0])
    count, samples, outside = wh.ref_hist(x, [0.0, 1.0, 2.0, 3.0], [1.0, 4.0, 5.0])
    assert count.shape == samples.shape == (1, 3, 2) and outside.shape == (1,) and count.dtype == samples.dtype == outside.dtype == np.int32
    # A = 1.0 opens bin 1 and length 4 opens bin 1; A = 2.0 opens bin 2, length 2 in bin 0; A = 3.0 is the last edge, length 5 too: outside
    assert count[0].tolist() == [[0, 0], [0, 1], [1, 0]] and samples[0].tolist() == [[0, 0], [0, 4], [2, 0]] and outside.tolist() == [1]
    count, samples, outside = wh.ref_hist(x, [0.0, np.inf], [0.0, np.inf])
    assert count.tolist() == [[[3]]] and samples.tolist() == [[[11]]] and outside.tolist() == [0]
    count, _, outside = wh.ref_hist(x, [np.nextafter(1.0, 2.0), 2.0, np.nextafter(3.0, 4.0)], [2.0, np.nextafter(5.0, 0.0), 6.0])
    assert count[0].tolist() == [[0, 0], [1, 1]] and outside.tolist() == [1]       # 1.0 is below the first edge now, 3.0 inside
    # the time bin is the peak's: a row of two half waves whose first peak stands at sample 2501 and whose second one at 10007
    t = tied_row(20011)
    _, length, peak, _ = waves_ref.ref_table(t)
    assert peak.tolist() == [2501, 10007] and length.tolist() == [10006, 10005]
    count, samples, outside = wh.ref_hist(t, [0.0, 1.0], [0.0, 1e6], hop=512)
    assert count.shape == (40, 1, 1) and np.flatnonzero(count).tolist() == [2501 // 512, 10007 // 512]
    assert samples[2501 // 512, 0, 0] == 10006 and samples[10007 // 512, 0, 0] == 10005 and not outside.any()
    assert wh.default_hop(3) == 512 and wh.default_hop(512) == 512 and wh.default_hop(513) == 1024


@pytest.mark.parametrize("fam", FAMILIES + ("tied",))
def test_the_reference_keeps_the_two_invariants(fam):
    rng = np.random.default_rng(11)
    for n in (3, 65, 513, 1537, 5000):
        x = tied_row(n) if fam == "tied" else family(fam, n)
        _, length, _, value = waves_ref.ref_table(x)
        A = np.abs(value)
        top = max(float(A.max()), 1e-300)
        for hop in (None, 512, 1024):
            for ae, le in (([0.0, np.inf], [1.0, np.inf]),
                           (np.sort(rng.random(6)) * top, [1.0, 2.0, 3.0, 5.0, 9.0, 600.0]),
                           ([0.25 * top, 0.5 * top], [2.0, 4.0])):
                count, samples, outside = wh.ref_hist(x, ae, le, hop)
                T = -(-n // (hop or wh.default_hop(n)))
                assert count.shape == (T, len(ae) - 1, len(le) - 1) and outside.shape == (T,)
                assert int(count.sum()) + int(outside.sum()) == length.size, (fam, n, hop)
                ok = wh.bin_of(A, ae)[1] & wh.bin_of(length.astype(np.float64), le)[1]
                assert int(samples.sum()) + int(length[~ok].sum()) == n, (fam, n, hop)
                assert np.all((count == 0) == (samples == 0))
                if hop is not None:                                      # the time bins only split what one bin holds
                    one = wh.ref_hist(x, ae, le, None)
                    assert np.array_equal(count.sum(axis=0), one[0][0]) and np.array_equal(samples.sum(axis=0), one[1][0])
                    assert outside.sum() == one[2][0]


def test_wrapper_refuses_bad_arguments_before_any_engine(monkeypatch):
    import pyitd_amd
    from pyitd_amd import _place, batch

    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(batch, "_engine_for", no_engine)
    monkeypatch.setattr(_place, "DeviceBuffer", no_engine)
    good, ae, le = np.zeros((2, 700)), [0.0, 0.5, 1.0], [1.0, 10.0, np.inf]
    nan = float("nan")
    bad_edges = (0.25, [0.1], [0.0, nan, 1.0], [nan, 1.0], [0.0, 0.2, 0.2], [0.0, 0.3, 0.2], [0.0, np.inf, np.inf], [-np.inf, -np.inf, 0.0],
                 np.linspace(0.0, 1.0, 66),                             # 65 bins
                 np.zeros((3, 3)) + [0.0, 1.0, 2.0],                    # 3 sets of edges, 2 rows
                 np.array([[0.0, 1.0, 2.0], [0.0, 2.0, 1.0]]))          # the second row's edges decrease
    for e in bad_edges:
        with pytest.raises(ValueError):
            pyitd_amd.wave_histogram(good, e, le)
        with pytest.raises(ValueError):
            pyitd_amd.wave_histogram(good, ae, e)
    with pytest.raises(ValueError, match="cells"):
        pyitd_amd.wave_histogram(good, np.arange(34.0), np.arange(33.0))           # 33 x 32 = 1056 cells
    with pytest.raises(ValueError):
        pyitd_amd.wave_histogram(np.zeros((2, 3, 700)), np.zeros((3, 2, 3)) + [0.0, 1.0, 2.0], le)
    for hop in (0, -512, 64, 256, 511, 513, 768, 1000, 512.5, "512", True):
        with pytest.raises((ValueError, TypeError)):
            pyitd_amd.wave_histogram(good, ae, le, hop=hop)
    for rows in (np.zeros(700), np.zeros((2, 2)), np.zeros((2, 700), np.int32), np.zeros((0, 700))):
        with pytest.raises(ValueError):
            pyitd_amd.wave_histogram(rows, ae, le)
    assert pyitd_amd.WaveHistogram._fields == ("count", "samples", "outside")


def test_the_edges_broadcast_to_the_leading_axes():
    from pyitd_amd.batch import _hist_edges, _hist_hop
    e = _hist_edges([0, 1, np.inf], "amplitude_edges", (2, 3))
    assert e.shape == (3,) and e.dtype == np.float64 and e.tolist() == [0.0, 1.0, np.inf]          # one set: stride 0
    per_level = np.array([[0.0, 1.0, 2.0], [0.0, 10.0, 20.0], [-np.inf, 0.5, np.inf]])
    e = _hist_edges(per_level, "length_edges", (2, 3))                  # [3, 3] over the leading axes (2, 3): every level its own
    assert e.shape == (6, 3) and e.flags.c_contiguous and np.array_equal(e, np.concatenate((per_level, per_level)))
    e = _hist_edges(per_level[:2, None, :], "length_edges", (2, 3))     # [2, 1, 3]: one set per first axis
    assert e.shape == (6, 3) and np.array_equal(e[:, 1], [1.0, 1.0, 1.0, 10.0, 10.0, 10.0])
    e = _hist_edges(per_level[:1], "amplitude_edges", (4,))             # [1, 3] is "per row", broadcast
    assert e.shape == (4, 3)
    assert _hist_hop(None, 3) == 512 and _hist_hop(None, 512) == 512 and _hist_hop(None, 513) == 1024 and _hist_hop(1024.0, 7) == 1024
