"""Exact reference of the instantaneous amplitude / phase / frequency operator (pyitd_amd/csrc/itd_tfe.hpp) — TEST
INFRASTRUCTURE ONLY (never imported by pyitd_amd).

The operator's definitions, with every decision taken exactly on the fp64 input:
  crossing i       1 <= i <= n-2 and a strict sign change x[i] -> x[i+1] ((x[i] > 0 and x[i+1] < 0) or the mirror); an
                   exact zero (of either sign) is no crossing, so 1, 0, -1 keeps one half wave
  half wave of j   the number of crossings i < j (a prefix count)
  amplitude        A = max |x| over the half wave, exact (a maximum of fp64 values)
  slope            rising where x[j+1] >= x[j] (the last sample: x[n-1] >= x[n-2]), an exact comparison
  phase            0 where A = 0; else with r = fl(x / A) and a = asin(r):
                       x >= 0, rising: a          x >= 0, falling: pi - a
                       x <  0, falling: pi - a    x <  0, rising:  2 pi + a
  frequency        dp = phase[j+1] - phase[j] (the last sample: phase[n-1] - phase[n-2]); dp + 2 pi where dp < 0;
                   divided by 2 pi
The one rounded step is the kernel's own quotient r = fl(x / A): the library is built without fast-math, so that division
is correctly rounded on the GPU as in numpy here.  asin, the quadrant placement, the difference, the wrap and the division
by 2 pi are taken in mpmath at PREC bits and returned as double-doubles (hi, lo).
"""
from collections import namedtuple

import mpmath
import numpy as np

PREC = 212                     # bits (64 decimal digits)
ULP_2PI = 2.0 ** -50           # ulp(2 pi): 2 pi lies in [4, 8)


def structure(x):
    """(crossing flags bool[n], half-wave index int64[n], amplitude float64[n], rising bool[n], quadrant int8[n], r float64[n])."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = x.size
    if n < 3:
        raise ValueError("needs at least 3 samples")
    cross = np.zeros(n, bool)
    cross[1:n - 1] = ((x[1:-1] > 0) & (x[2:] < 0)) | ((x[1:-1] < 0) & (x[2:] > 0))
    hw = np.zeros(n, np.int64)
    hw[1:] = np.cumsum(cross)[:-1]
    A = np.zeros(int(hw[-1]) + 1)
    np.maximum.at(A, hw, np.abs(x))
    amp = A[hw]
    rising = np.empty(n, bool)
    rising[:-1] = x[1:] >= x[:-1]
    rising[-1] = x[-1] >= x[-2]
    quad = np.where(x >= 0, np.where(rising, 0, 1), np.where(rising, 3, 2)).astype(np.int8)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(amp > 0, x / np.where(amp > 0, amp, 1.0), 0.0)
    return cross, hw, amp, rising, quad, r


class ExactTFE(namedtuple("ExactTFE", "samples amp phase_hi phase_lo freq_hi freq_lo dp quad zero_amp")):
    """At `samples`: amp (exact), phase and frequency as double-doubles, dp = the exact phase difference before the wrap
    (rounded to fp64: its sign and size decide the wrap), quad = the sample's quadrant (0..3), zero_amp = A == 0."""

    def phase_err(self, g):
        g = np.asarray(g, dtype=np.float64)[self.samples]
        return np.abs((g - self.phase_hi) - self.phase_lo)

    def freq_err(self, g, circular=True):
        """|g - exact| in cycles per sample; circular: the distance mod 1 (a wrap decided the other way at dp ~ 0 is one cycle)."""
        d = (np.asarray(g, dtype=np.float64)[self.samples] - self.freq_hi) - self.freq_lo
        return np.abs(d - np.round(d)) if circular else np.abs(d)


def exact_tfe(x, samples=None):
    """The exact results of the operator on x at `samples` (default: every sample)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = x.size
    _, _, amp, _, quad, r = structure(x)
    samples = np.arange(n, dtype=np.int64) if samples is None else np.unique(np.asarray(samples, dtype=np.int64))
    need = np.unique(np.concatenate((samples, np.minimum(samples + 1, n - 1), [n - 2])))
    cache = {}
    ph = {}
    with mpmath.workprec(PREC):
        pi = mpmath.pi
        two_pi = 2 * pi
        for j in need.tolist():
            if not amp[j] > 0:
                ph[j] = mpmath.mpf(0)
                continue
            rj = float(r[j])
            a = cache.get(rj)
            if a is None:
                a = cache[rj] = mpmath.asin(mpmath.mpf(rj))
            q = int(quad[j])
            ph[j] = a if q == 0 else (pi - a if q in (1, 2) else two_pi + a)
        k = samples.size
        p_hi, p_lo, f_hi, f_lo, dps = (np.empty(k) for _ in range(5))
        for t, j in enumerate(samples.tolist()):
            p = ph[j]
            dp = ph[j + 1] - p if j + 1 < n else p - ph[n - 2]
            f = (dp + two_pi if dp < 0 else dp) / two_pi
            p_hi[t] = float(p)
            p_lo[t] = float(p - p_hi[t])
            f_hi[t] = float(f)
            f_lo[t] = float(f - f_hi[t])
            dps[t] = float(dp)
    return ExactTFE(samples, amp[samples], p_hi, p_lo, f_hi, f_lo, dps, quad[samples], ~(amp[samples] > 0))


def quadrant_bounds(quad):
    """The closed phase interval of each quadrant (fp64 bounds): [0, pi/2], [pi/2, 3pi/2] (both falling), [3pi/2, 2pi]."""
    lo = np.array([0.0, np.pi / 2, np.pi / 2, 1.5 * np.pi])[quad]
    hi = np.array([np.pi / 2, 1.5 * np.pi, 1.5 * np.pi, 2 * np.pi])[quad]
    return lo, hi


def sample_subset(n, x):
    """Every sample for short signals; else every crossing +-1, every 64-sample step edge +-1 of the first and last tiles, every
    tile edge +-1, the first and last 600 samples and a stride (oracle.exact_spline.sample_subset's pattern on the crossings)."""
    from oracle.exact_spline import sample_subset as ss
    cross = np.flatnonzero(structure(x)[0])
    s = ss(n, np.concatenate((cross, cross + 1)))
    if n <= 65536:
        return s
    tiles = np.arange(0, n, 512, dtype=np.int64)
    steps = np.concatenate((np.arange(0, 1024, 64), np.arange((n - 1024) // 64 * 64, n, 64)))
    out = np.unique(np.concatenate((s, tiles - 1, tiles + 1, steps - 1, steps, steps + 1, [n - 2, n - 1])))
    return out[(out >= 0) & (out < n)]
