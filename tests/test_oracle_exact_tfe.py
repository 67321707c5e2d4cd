"""The exact reference of the instantaneous operator (oracle/exact_tfe.py) and the signal families the GPU test
(test_gpu_instantaneous_exact.py) runs it on.

1. The exact reference agrees with test_gpu_tfe.numpy_tfe, an independent fp64 statement of the same definitions, to 1e-13 on
   that test's three signals and on every family: it is the same operation, not a transcription of the kernel.
2. The families have the structure they are built for: crossings at the step and tile seams, half waves longer than a tile,
   no crossing at the first sample pair, exact zeros that do not cut a wave, plateaus at the maximum.
"""
import numpy as np
import pytest

from oracle import exact_tfe as et
from test_gpu_tfe import numpy_tfe

TOL = 1e-13


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31)


def seam_crossings(n):
    """Crossing indices at lanes 62 / 63 / 0 of 64-sample steps, at samples 511 / 512 / 513 of tiles, at 0 -> 1 (not a crossing
    by the definition) and at (n-2) -> (n-1)."""
    c = {0, n - 2}
    for s in range(0, n, 64):
        c.update((s - 2, s - 1, s))
    for t in range(512, n + 512, 512):
        c.update((t - 1, t, t + 1))
    return np.array(sorted(i for i in c if 0 <= i <= n - 2), np.int64)


def with_crossings(n, cross, rng, mag=None):
    """A signal whose strict sign changes x[i] -> x[i+1] are exactly at `cross` (random magnitudes in [0.1, 1.1))."""
    flips = np.zeros(n, np.int64)
    flips[np.asarray(cross, np.int64) + 1] = 1
    sign = np.where(np.cumsum(flips) % 2 == 0, 1.0, -1.0)
    m = 0.1 + rng.random(n) if mag is None else mag
    return sign * m


def family(name, n):
    rng = np.random.default_rng(_seed(name) + n)
    t = np.arange(n, dtype=np.float64)
    if name == "seams":
        return with_crossings(n, seam_crossings(n), rng)
    if name == "slow":          # half waves of 3 .. 20 tiles: the period sweeps from 3072 to 20480 samples
        period = 3072.0 * (20480.0 / 3072.0) ** (t / n)
        return np.sin(2 * np.pi * np.cumsum(1.0 / period) + 0.3)
    if name == "positive":      # one half wave, m = 0
        return 0.5 + rng.random(n)
    if name == "zeros":
        return np.zeros(n)
    if name == "quantised":     # int-valued: exact zeros inside waves (1, 0, -1), plateaus at the maximum, ties
        return np.round(3.4 * np.sin(2 * np.pi * t / 37.0) + 0.7 * rng.standard_normal(n))
    if name == "negzero":       # the quantised signal with every zero a -0.0 or +0.0 at random
        x = family("quantised", n)
        return np.where(x == 0, np.where(rng.random(n) < 0.5, -0.0, 0.0), x)
    if name == "subnormal":     # the quantised signal in units of 2^-1074: every value subnormal
        return family("quantised", n) * 2.0 ** -1074
    if name == "huge":          # values near +-1e300
        return 1e300 * (np.sin(2 * np.pi * t / 23.0) + 0.8 * rng.standard_normal(n))
    if name == "noise":
        return rng.standard_normal(n)
    raise KeyError(name)


FAMILIES = ("seams", "slow", "positive", "zeros", "quantised", "negzero", "subnormal", "huge", "noise")


def _agree(x, samples=None):
    ex = et.exact_tfe(x, samples)
    a, p, f = numpy_tfe(x)
    s = ex.samples
    assert np.array_equal(a[s], ex.amp), "amplitude"
    pe = float(np.max(ex.phase_err(p))) if s.size else 0.0
    fe = float(np.max(ex.freq_err(f))) if s.size else 0.0
    assert pe <= TOL and fe <= TOL, (pe, fe)
    return pe, fe


def test_agrees_with_the_numpy_statement_on_its_signals():
    rng = np.random.default_rng(11)
    n = 100003
    t = np.arange(n)
    for x in (np.sin(2 * np.pi * 0.013 * t + 0.3) * (1 + 0.5 * np.sin(2 * np.pi * 0.0004 * t)),
              np.sin(2 * np.pi * (0.002 * t + 4e-8 * t * t)),
              rng.standard_normal(n)):
        _agree(x, et.sample_subset(n, x))


@pytest.mark.parametrize("name", FAMILIES)
def test_agrees_with_the_numpy_statement_on_the_families(name):
    for n in (3, 4, 65, 1027, 3 * 512 + 514):
        _agree(family(name, n))
    n = 60000                                                       # every 5th sample and the last ones
    _agree(family(name, n), np.concatenate((np.arange(0, n, 5), np.arange(n - 100, n))))


def test_families_have_their_structure():
    n = 2051
    cross, hw, amp, _, _, _ = et.structure(family("seams", n))
    got = np.flatnonzero(cross)
    want = seam_crossings(n)
    assert np.array_equal(got, want[want >= 1])                     # 0 -> 1 is a sign change but no crossing
    assert {62, 63, 64, 511, 512, 513, n - 2} <= set(got.tolist())
    x = family("slow", 60000)
    c = np.flatnonzero(et.structure(x)[0])
    gaps = np.diff(c)
    assert gaps.min() >= 3 * 512 and gaps.max() <= 20 * 512 and gaps.max() >= 8 * 512, (gaps.min(), gaps.max())
    _, hw, amp, _, _, _ = et.structure(family("positive", 999))
    assert hw.max() == 0
    q = family("quantised", 4000)
    assert np.any((q[:-2] > 0) & (q[1:-1] == 0) & (q[2:] < 0))    # 1, 0, -1: no crossing there
    _, _, amp, _, _, _ = et.structure(q)
    assert np.any((np.abs(q[:-1]) == amp[:-1]) & (q[:-1] == q[1:]))  # a plateau at the maximum
    z = family("negzero", 4000)
    assert np.any((z == 0) & np.signbit(z))
    s = family("subnormal", 4000)
    assert np.all(np.abs(s) < 2.0 ** -1022) and np.any(s != 0)


def test_exact_values_of_a_known_wave():
    """One half wave 0.5, 1, 0.5 then its mirror: phases pi/6, pi/2, 5pi/6, then 7pi/6, 3pi/2, 11pi/6 (the last sample rises
    by its backward difference); frequencies 1/6 everywhere."""
    x = np.array([0.5, 1.0, 0.5, -0.5, -1.0, -0.5])
    ex = et.exact_tfe(x)
    want = np.array([1, 3, 5, 7, 9, 11]) * np.pi / 6
    assert np.max(np.abs(ex.phase_hi - want)) < 1e-15
    assert np.array_equal(ex.amp, np.ones(6))
    assert np.max(np.abs(ex.freq_hi - 1.0 / 6)) < 1e-15
    z = et.exact_tfe(np.zeros(5))
    assert np.all(z.phase_hi == 0) and np.all(z.freq_hi == 0) and np.all(z.zero_amp)
