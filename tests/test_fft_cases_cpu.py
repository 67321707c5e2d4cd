"""tests/fft_cases.py on its own, without a GPU: the reference's precision, the yardsticks' ranges, where every listed length
lands, and the selector cases' decided shares and intended records.

The yardstick fences are a sanity check on the helper, not a bound on the kernel.  On the seeded Gaussian rows float64 numpy.fft
stays below 64 units and the sequential direct DFT below 256 units up to 8192 points; a sequential sum's error grows with the
square root of its length, so beyond that the fence is 256 sqrt(n / 8192) (measured: 390 units at 240240 points).  An impulse, a tone
or a constant puts the whole row into one output of sqrt(n) ||x||2, whose half ulp alone is sqrt(n) units: those rows are fenced at
16 sqrt(n) units more (measured: 2055 units = 8 sqrt(n) for numpy.fft on a tone of 65537 points).
"""
import numpy as np
import pytest

import fft_cases as fc


def test_long_double_is_wider_than_double_here():
    assert fc.LONGDOUBLE_OK, fc.LONGDOUBLE_WHY
    assert ref_dtype() == np.clongdouble


def ref_dtype():
    return fc.ref_fft(np.ones(4, np.complex128)).dtype


@pytest.mark.parametrize("n", (97, 128, 360))
def test_reference_against_mpmath(n):
    mp = pytest.importorskip("mpmath")
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    R = fc.ref_fft(x)
    with mp.workprec(200):
        def tomp(v):
            hi = float(v)
            return mp.mpf(hi) + mp.mpf(float(v - np.longdouble(hi)))
        xs = [mp.mpc(v.real, v.imag) for v in x]
        w = [mp.expjpi(mp.mpf(-2 * e) / n) for e in range(n)]
        worst = mp.mpf(0)
        for k in range(n):
            X = mp.fsum(xs[j] * w[(j * k) % n] for j in range(n))
            worst = max(worst, abs(X - mp.mpc(tomp(R[k].real), tomp(R[k].imag))))
        err = float(worst) / float(fc.unit(x)[0])
    assert err < 0.01, (n, err)


@pytest.mark.parametrize("n", (97, 128, 360, 8209))
def test_reference_round_trip(n):
    rng = np.random.default_rng(n + 1)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    back = fc.ref_fft(fc.ref_fft(x), True)
    assert float(np.max(np.abs(back - x))) <= 2.0 ** -58 * float(np.max(np.abs(x)))


@pytest.mark.parametrize("n", fc.LENGTHS)
def test_yardstick_ranges(n):
    names, x, by_dir = fc.length_case(n)
    for inverse in (False, True):
        ref, u, y_fft, y_seq, idx = by_dir[inverse]
        assert (y_seq is not None) == fc.takes_generic(n)
        for b, name in enumerate(names):
            extra = 0.0 if fc.is_random(name) else 16.0 * np.sqrt(n)
            assert 0.0 <= y_fft[b] <= 64.0 + extra, (n, name, inverse, y_fft[b])
            if y_seq is not None:
                assert 0.0 <= y_seq[b] < 256.0 * max(1.0, np.sqrt(n / 8192.0)) + extra, (n, name, inverse, y_seq[b])
        if idx is not None:
            assert 8 <= idx.shape[0] <= 512 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n


def test_families_hold_what_they_name():
    names, x = fc.family_rows(1001)
    assert names == ["complex0", "complex1", "real0", "real1", "impulse0", "impulse1", "impulse500", "impulse1000", "tone1", "tone1000",
                     "constant"]
    assert (x[2:4].imag == 0).all() and (x[0:2].imag != 0).any()
    for b, j0 in ((4, 0), (5, 1), (6, 500), (7, 1000)):
        assert x[b, j0] == 1.0 and np.count_nonzero(x[b]) == 1
    for b, k0 in ((8, 1), (9, 1000)):
        X = fc.ref_fft(x[b])
        assert abs(X[k0] - 1001) < 1e-10 and np.max(np.abs(np.delete(X, k0))) < 1e-10
    assert fc.family_rows(1)[1].shape == (7, 1) and fc.family_rows(2)[0] == ["complex0", "complex1", "real0", "real1", "impulse0",
                                                                              "impulse1", "tone1", "constant"]
    assert len(fc.family_rows(1 << 20)[0]) == 5          # the longest transform: one row per family


def test_every_listed_length_lands_where_the_list_says():
    for n in fc.TIER1_UNROLLED:
        assert fc.path_of(n) == (1, "unrolled"), n
        assert set(fc.radices(n)) <= {2, 3, 4, 5, 7, 8}
    for n in fc.TIER1_GENERIC:
        assert fc.path_of(n) == (1, "generic"), n
        assert max(fc.radices(n)) >= 11
    assert fc.radices(8186) == [2, 4093] and fc.radices(8191) == [8191] and fc.radices(88) == [8, 11] and fc.radices(2310) == [2, 3, 5, 7, 11]
    assert fc.radices(6720) == [8, 8, 3, 5, 7] and fc.radices(4096) == [8, 8, 8, 8] and fc.radices(2) == [2] and fc.radices(1) == []
    # the thread seams; the 256-thread instance of k_fft_lds ends at 2048 points
    assert [fc.fft_threads(n) for n in fc.TIER1_SEAMS] == [64, 128, 128, 256, 256, 512, 512, 1024]
    assert all(fc.path_of(n)[0] == 1 for n in fc.TIER1_SEAMS)
    assert all(8 * fc.fft_threads(n) >= n for n in range(1, fc.LDS_MAX + 1))
    splits = {8193: 3, 8194: 34, 16382: 2, 16384: 128, 24576: 128, 240240: 462, 1 << 20: 1024}
    for n in fc.TIER2:
        n1 = fc.four_step_split(n)
        assert fc.path_of(n)[0] == 2 and n1 == splits[n] and n % n1 == 0 and n1 <= n // n1 <= fc.LDS_MAX, n
    assert [fc.path_of(n)[1] for n in fc.TIER2] == ["generic", "generic", "generic", "unrolled", "unrolled", "generic", "unrolled"]
    for n in fc.TIER3:
        assert fc.path_of(n) == (3, "bluestein") and fc.four_step_split(n) == 0, n
    assert 24627 == 3 * 8209 and 16418 == 2 * 8209            # composite, and still no admissible split
    # the plumbing cases of tests/test_gpu_fft_exact.py: one workspace chunk holds 1024 / 512 transforms; one chirp buffer
    assert fc.CHUNK_BYTES // (16384 * 16) == 1024 and fc.CHUNK_BYTES // (fc.bluestein_m(8209) * 16) == 512
    assert fc.bluestein_m(8209) == fc.bluestein_m(10007) == 32768
    assert len(fc.LENGTHS) == len(set(fc.LENGTHS)) == 37


@pytest.mark.parametrize("rule", ("any", "valid"))
def test_selector_cases_are_decided_and_mean_what_they_say(rule):
    decided, left_out = fc.selector_cases(rule)
    assert left_out <= 0.05, left_out
    by_name = {c[0]: c for c in decided}
    designed = [c for c in fc.designed_cases() if c[1] == rule]
    assert {int(c[0].split("_n")[-1].split("_")[0]) for c in designed} == set(fc.SELECTOR_NS)
    for name, _, x, intended in designed:
        assert name in by_name, "%s is not decided" % name
        assert np.array_equal(by_name[name][3], intended), (name, by_name[name][3], intended)
        a = np.abs(fc.ref_fft(x))
        assert fc.decide(a, rule)[1] >= 0.01, (name, fc.decide(a, rule)[1])          # every gap the rule compares: 1 per cent
    noisy = np.stack([c[3] for c in decided if c[0].startswith("noisy")])
    assert len(noisy) >= 0.95 * fc.NOISY_ROWS
    assert 20 <= int(noisy[:, 0].sum()) <= len(noisy) - (20 if rule == "any" else 1)          # modes and rejections
    recs = np.stack([c[3] for c in decided])
    assert ((recs[:, 0] == 0) == (recs[:, 4] == -1)).all() and ((recs[:, 4] == -1) == (recs[:, 5] == -1)).all()
    for c in decided:
        if not c[3][0]:
            assert not c[4].any(), c[0]          # a rejection's mode is all zero
        else:
            assert np.max(np.abs(c[4])) > 0, c[0]


def test_designed_cases_reach_every_branch():
    names = {c[0] for c in fc.designed_cases()}
    for n in (64, 65, 1000, 1001, 8192, 8193, 10007):
        for must in ("pm1", "pm2", "pmhalf2", "pmhalf1", "fp_adjacent", "lp_adjacent", "fp0", "narrow", "wide"):
            assert "%s_n%d_any" % (must, n) in names
        for must in ("two_peaks", "three_peaks", "three_peaks_shifted", "none_below", "none_above", "below_at_pm_minus_2"):
            assert "%s_n%d_valid" % (must, n) in names
    for n in (4, 5, 6, 7):
        assert "pm1_n%d_any" % n in names and "nopeaks_n%d_valid" % n in names
