"""The time-frequency-energy spectrum (itd_tfe_spectrum_*, pyitd_amd.tfe_spectrum) as far as it goes without a GPU: the wrapper
refuses bad arguments before any engine exists, the entries refuse a NULL engine, and the numpy statement of the definition
(spectrum_ref) has the properties the definition promises: it conserves the count, its count-weighted cells are a plain
two-dimensional histogram, hop >= n gives one time bin, an empty cell is +0.0.
"""
import numpy as np
import pytest

import spectrum_ref as sr
from test_gpu_tfe import numpy_tfe
from test_oracle_exact_tfe import FAMILIES, family


def test_entries_refuse_a_null_engine():
    from pyitd_amd import _lib
    L = _lib.load()
    for fn in (L.itd_tfe_spectrum_f64, L.itd_tfe_spectrum_f32):
        assert fn(None, None, 5, 1, 5, None, 4, 64, 2, None, 4, None, None, None) == 1      # ITD_ERR_INVALID_ARG


def test_wrapper_refuses_bad_arguments_before_any_engine(monkeypatch):
    import pyitd_amd
    from pyitd_amd import _place, batch

    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(batch, "_engine_for", no_engine)
    monkeypatch.setattr(_place, "DeviceBuffer", no_engine)
    good, edges = np.zeros((2, 700)), np.linspace(0.0, 0.5, 5)
    bad_edges = (0.25, [0.1], np.zeros((2, 3)), [0.0, 0.2, 0.2], [0.0, 0.3, 0.2], [0.0, np.nan, 0.5], [0.0, 0.1, np.inf],
                 np.linspace(0.0, 0.5, 515))
    for e in bad_edges:
        with pytest.raises(ValueError):
            pyitd_amd.tfe_spectrum(good, e, 64)
    for hop in (0, -64, 32, 100, 192, 320, 384, 448, 513, 64.5, "64"):
        with pytest.raises((ValueError, TypeError)):
            pyitd_amd.tfe_spectrum(good, edges, hop)
    for w in ("power", "", None, 2):
        with pytest.raises(ValueError):
            pyitd_amd.tfe_spectrum(good, edges, 64, weight=w)
    for rows in (np.zeros(700), np.zeros((2, 2)), np.zeros((2, 700), np.int32), np.zeros((0, 700))):
        with pytest.raises(ValueError):
            pyitd_amd.tfe_spectrum(rows, edges, 64)
    assert pyitd_amd.Spectrum._fields == ("power", "outside")


@pytest.mark.parametrize("fam", FAMILIES)
def test_the_reference_conserves_the_count_and_is_a_histogram(fam):
    for n, hop, F in ((3, 64, 1), (65, 64, 3), (1027, 128, 16), (1027, 576, 3), (3 * 512 + 514, 512, 16), (5000, 1088, 512)):
        x = family(fam, n)
        with np.errstate(all="ignore"):
            A, _, f = numpy_tfe(x)
        for edges in (sr.uniform_edges(F), sr.log_edges(F), sr.pi_edges(F), sr.uniform_edges(F, 0.1, 0.3)):
            S, out = sr.spectrum_ref(A, f, edges, hop, "count")
            T = -(-n // hop)
            assert S.shape == (T, F) and out.shape == (T,) and out.dtype == np.int32
            assert S.sum() + out.sum() == n, (fam, n, hop, F)
            j = np.arange(n)
            H, _, _ = np.histogram2d(j // hop, f, bins=(np.arange(T + 1), edges))
            if np.any(f == edges[-1]):                                  # numpy's last bin is closed on the right, ours is not
                H[:, -1] -= np.bincount((j // hop)[f == edges[-1]], minlength=T)
            assert np.array_equal(S, H), (fam, n, hop, F)
            for weight in ("amplitude", "energy"):
                Sw, outw = sr.spectrum_ref(A, f, edges, hop, weight)
                assert np.array_equal(outw, out)
                assert not np.isnan(Sw).any() and not np.signbit(Sw).any()
                assert np.all(Sw[S == 0] == 0.0)                         # a cell with no sample is +0.0


def test_the_sums_follow_the_definitions_order():
    """A row of 130 samples in one bin, weights chosen so that the order of the additions shows in the last bits: the step sum is
    the adjacent-pair tree, the cell the step sums added in order."""
    rng = np.random.default_rng(3)
    A = 1.0 + rng.random(130)
    f = np.full(130, 0.2)
    S, out = sr.spectrum_ref(A, f, np.array([0.1, 0.3]), 8192, "amplitude")

    def tree(v):
        v = list(v) + [0.0] * (64 - len(v))
        while len(v) > 1:
            v = [v[i] + v[i + 1] for i in range(0, len(v), 2)]
        return v[0]
    want = 0.0
    for s in range(3):
        want = want + tree(A[64 * s:64 * s + 64])
    assert S.shape == (1, 1) and S[0, 0] == want and out.tolist() == [0]


def test_a_hop_of_the_rows_length_or_more_gives_one_time_bin():
    x = family("noise", 1000)
    A, _, f = numpy_tfe(x)
    edges = sr.uniform_edges(8)
    for hop in (1024, 8192):
        S, out = sr.spectrum_ref(A, f, edges, hop, "energy")
        assert S.shape == (1, 8) and out.shape == (1,)
    many, out_many = sr.spectrum_ref(A, f, edges, 64, "count")
    assert np.array_equal(many.sum(axis=0), sr.spectrum_ref(A, f, edges, 1024, "count")[0][0])
    assert out_many.sum() == out.sum()


def test_samples_on_an_edge_and_outside():
    f = np.array([0.0, 0.1, 0.2, 0.3, np.nan, 0.05, 0.25, -0.0, 1.0])
    A = np.arange(1.0, 10.0)
    S, out = sr.spectrum_ref(A, f, np.array([0.1, 0.2, 0.3]), 64, "amplitude")
    assert S.tolist() == [[2.0, 3.0 + 7.0]] and out.tolist() == [6]     # 0.1 and 0.2 open their bins, 0.3 is outside
