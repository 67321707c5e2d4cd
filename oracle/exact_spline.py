"""Exact references of the two spline baselines — TEST INFRASTRUCTURE ONLY (never imported by pyitd_amd).

  natural(x, e, idx)      itd_baseline_extract_fast (itd_fourier_decomposition.py:49-122), every quirk as written
  iq(I, Q, e, idx)        the same operator on avg = (I + Q) / 2 (itd.cpp:96-108), avg taken exactly
  nak(x, min_extrema)     the FITPACK flavour (numba_accelerated_itd.py:182-211): the interpolating not-a-knot cubic
                          through the knot values at the sites [0, knots, n-1], solved exactly

The fp64 inputs are taken as exact values.  Knot values and the knot recurrences run in mpmath at PREC bits; the
per-sample evaluation is exact integer arithmetic on those values (fixed point, about 2^-300 of the signal's scale)
and ends in one correctly rounded division.  The result of every evaluated sample is a double-double (hi, lo): the
error of an fp64 result g there is |(g - hi) - lo| (Exact.err).

zigzag() builds test signals: a piecewise-linear signal whose strict alternating extrema lie exactly at the designed
knots, so that both knot detectors (cpu_oracle.extrema_cpp, cpu_oracle.knots) find exactly those knots.
"""
from collections import namedtuple

import mpmath
import numpy as np

PREC = 256
FULL_N = 65536          # above this many samples only a subset is evaluated (sample_subset)
TILE = 512              # the GPU evaluation's tile: its edges are always in the subset


class Exact(namedtuple("Exact", "samples hi lo")):
    """samples int64[k], hi/lo float64[k]: the exact result at samples is hi + lo (|lo| <= ulp(hi) / 2)."""

    def err(self, g):
        g = np.asarray(g, dtype=np.float64)[self.samples]
        return np.abs((g - self.hi) - self.lo)

    def scale(self, x):
        """S = max(|x|, |exact|) over the signal."""
        return max(float(np.max(np.abs(x))), float(np.max(np.abs(self.hi))))

    def ulps(self, g, x):
        """max err / (eps * S), eps = 2^-52."""
        return float(np.max(self.err(g))) / (2.0 ** -52 * self.scale(x))


def sample_subset(n, sites):
    """Every sample for n <= FULL_N; else every site +-1, every tile edge, the segment midpoints, the first and last
    600 samples and a stride."""
    if n <= FULL_N:
        return np.arange(n, dtype=np.int64)
    s = np.asarray(sites, dtype=np.int64)
    tiles = np.arange(0, n, TILE, dtype=np.int64)
    parts = [s - 1, s, s + 1, tiles, tiles + TILE - 1, (s[:-1] + s[1:]) // 2,
             np.arange(600), np.arange(n - 600, n), np.arange(0, n, max(1, n // 20000))]
    out = np.unique(np.concatenate(parts))
    return out[(out >= 0) & (out < n)]


def _evaluate(n, sites, Y, M, seg, linear_seg=None, samples=None):
    """The cubic with second derivatives M at sites through the values Y, segment j = seg(i) for every sample i:
        ((h - a) Y_j + a Y_{j+1}) / h  -  a (h - a) ((2h - a) M_j + (h + a) M_{j+1}) / (6h),   a = i - s_j, h = s_{j+1} - s_j
    (= (1-t) Y_j + t Y_{j+1} + h^2/6 ((1-t)^3 - (1-t)) M_j + h^2/6 (t^3 - t) M_{j+1} with t = a / h, for any integer a);
    segment linear_seg without its M terms.  Exact integers, one rounding per sample at the end."""
    if samples is None:
        samples = sample_subset(n, sites)
    samples = np.asarray(samples, dtype=np.int64)
    sites = [int(v) for v in sites]
    with mpmath.workprec(PREC):
        big = max([abs(y) for y in Y] + [abs(M[j]) * (sites[j + 1] - sites[j]) ** 2 for j in range(len(sites) - 1)]
                  + [mpmath.mpf(2) ** -1000])
        F = PREC + 64 - int(mpmath.mag(big))         # fixed point: granularity 2^-(PREC+64) of the largest term
        Yi = np.array([int(mpmath.nint(mpmath.ldexp(y, F))) for y in Y] + [0], dtype=object)
        Mi = np.array([int(mpmath.nint(mpmath.ldexp(m, F))) for m in M] + [0], dtype=object)
    j = seg(samples)
    s_arr = np.array(sites + [0], dtype=object)
    sj, sn = s_arr[j], s_arr[j + 1]
    h = sn - sj
    a = samples.astype(object) - sj
    hb = h - a
    mj, mn = Mi[j], Mi[j + 1]
    if linear_seg is not None:
        lin = j == linear_seg
        mj = np.where(lin, 0, mj)
        mn = np.where(lin, 0, mn)
    num = 6 * (hb * Yi[j] + a * Yi[j + 1]) - a * hb * ((h + hb) * mj + (h + a) * mn)
    den = 6 * h
    if F >= 0:
        den = den * (1 << F)
    else:
        num = num * (1 << -F)
    hi = np.array([float(v) for v in num / den], dtype=np.float64) if len(samples) else np.zeros(0)

    def _lo(nm, dn, hv):
        p, q = hv.as_integer_ratio()
        return (nm * q - p * dn) / (dn * q)

    lo = np.array([_lo(nm, dn, hv) for nm, dn, hv in zip(num, den, hi.tolist())], dtype=np.float64)
    return Exact(samples, hi, lo)


def _mp(v):
    return mpmath.mpf(float(v))


def _natural_from_values(n, at, e, idx, samples=None):
    """The operator of itd_fourier_decomposition.py:49-122 on the signal whose value at sample p is at(p) (mpf)."""
    e = [int(v) for v in np.asarray(e)[: idx + 1]]
    if idx < 2 or any(not 0 <= v < n for v in e):
        raise ValueError("idx >= 2 and every e[0..idx] inside the signal")
    with mpmath.workprec(PREC):
        half = mpmath.mpf(0.5)
        K = [mpmath.mpf(0)] * (idx + 1)
        for k in range(1, idx - 1):                 # :61-80 (stops at idx-2: K[idx-1] stays 0)
            w = mpmath.mpf(e[k] - e[k - 1]) / (e[k + 1] - e[k - 1])
            K[k] = half * (at(e[k - 1]) + w * (at(e[k + 1]) - at(e[k - 1]))) + half * at(e[k])
        K[0], K[idx] = at(e[0]), at(e[idx])         # :83
        h = [mpmath.mpf(e[i + 1] - e[i]) for i in range(idx)]
        u = [mpmath.mpf(0)] * (idx + 1)
        v = [mpmath.mpf(0)] * (idx + 1)
        b = [mpmath.mpf(0)] * (idx + 1)
        for i in range(1, idx):                     # :88-91
            u[i] = h[i - 1] / (h[i - 1] + h[i])
            v[i] = 1 - u[i]
            b[i] = 6 * ((K[i + 1] - K[i]) / h[i] - (K[i] - K[i - 1]) / h[i - 1]) / (h[i - 1] + h[i])
        for i in range(1, idx):                     # :93-98: the original u and v; the normalised u is never read
            d = 2 - u[i] * v[i - 1]
            b[i] = (b[i] - u[i] * b[i - 1]) / d
        for i in range(idx - 2, -1, -1):            # :100-101: back substitution with v
            b[i] = b[i] - v[i] * b[i + 1]
        b[0] = mpmath.mpf(0)                        # :104-105; b[idx] is numpy.zeros' 0
        b[idx - 1] = mpmath.mpf(0)
        b[idx] = mpmath.mpf(0)
    inner = np.asarray(e[1:idx], dtype=np.int64)

    def seg(i):                                     # j_lookup (:107-111): clamps at idx-1
        return np.searchsorted(inner, i, side="right")

    return _evaluate(n, e, K, b, seg, linear_seg=idx - 2, samples=samples)


def natural(x, e, idx, samples=None):
    """itd_baseline_extract_fast(x, e, idx) exactly; e needs idx + 1 entries (detect mode: the knots, then 0)."""
    x = np.asarray(x, dtype=np.float64)
    return _natural_from_values(x.shape[0], lambda p: _mp(x[p]), e, idx, samples)


def iq(I, Q, e, idx, samples=None):
    """The I/Q form: the natural operator on avg = (I + Q) / 2, avg exact."""
    I = np.asarray(I, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    return _natural_from_values(I.shape[0], lambda p: (_mp(I[p]) + _mp(Q[p])) / 2, e, idx, samples)


def nak(x, min_extrema=10, knots=None, samples=None):
    """itd_baseline_extract_modified (min_extrema = 10) / MEITD's itd_baseline_extract (min_extrema = 0) exactly.
    knots: the interior knots (default: cpu_oracle.knots(x)).  Fewer than min_extrema knots: x itself."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    if knots is None:
        from . import cpu_oracle
        knots = cpu_oracle.knots(x)
    knots = [int(v) for v in knots]
    if len(knots) < min_extrema:
        s = np.arange(n, dtype=np.int64) if samples is None else np.asarray(samples, dtype=np.int64)
        return Exact(s, x[s].copy(), np.zeros(len(s)))
    if len(knots) < 2:
        raise ValueError("the not-a-knot cubic needs at least 4 sites")
    s = [0] + knots + [n - 1]
    m = len(s) - 1                                  # sites s_0 .. s_m
    with mpmath.workprec(PREC):
        half = mpmath.mpf(0.5)
        X = lambda p: _mp(x[p])                     # noqa: E731
        Y = [mpmath.mpf(0)] * (m + 1)
        Y[0] = (2 * X(0) - X(1) + X(0)) / 2         # numpy.pad(x, 1, 'reflect', reflect_type='odd'), mean of the first two
        Y[m] = (X(n - 1) + 2 * X(n - 1) - X(n - 2)) / 2
        for k in range(1, m):                       # baseline_knot_estimation (:167-178)
            w = mpmath.mpf(s[k] - s[k - 1]) / (s[k + 1] - s[k - 1])
            Y[k] = half * (X(s[k - 1]) + w * (X(s[k + 1]) - X(s[k - 1]))) + half * X(s[k])
        h = [mpmath.mpf(s[i + 1] - s[i]) for i in range(m)]
        # rows i = 1 .. m-1:  mu_i M_{i-1} + 2 M_i + lam_i M_{i+1} = 6 f[s_{i-1}, s_i, s_{i+1}]
        lo_, di, up, rhs = [], [], [], []
        for i in range(1, m):
            mu = h[i - 1] / (h[i - 1] + h[i])
            lo_.append(mu)
            di.append(mpmath.mpf(2))
            up.append(1 - mu)
            rhs.append(6 * ((Y[i + 1] - Y[i]) / h[i] - (Y[i] - Y[i - 1]) / h[i - 1]) / (h[i - 1] + h[i]))
        # not-a-knot: the third derivative is continuous at s_1 and s_{m-1}, i.e. (M_1 - M_0) / h_0 = (M_2 - M_1) / h_1:
        # M_0 = (1 + r) M_1 - r M_2 with r = h_0 / h_1 (mirrored at the right end), substituted into the first / last row
        r0 = h[0] / h[1]
        rm = h[m - 1] / h[m - 2]
        di[0] += lo_[0] * (1 + r0)
        up[0] -= lo_[0] * r0
        di[-1] += up[-1] * (1 + rm)
        lo_[-1] -= up[-1] * rm
        # Thomas on the m-1 unknowns M_1 .. M_{m-1}
        cnt = m - 1
        cp = [mpmath.mpf(0)] * cnt
        dp = [mpmath.mpf(0)] * cnt
        for i in range(cnt):
            piv = di[i] - (lo_[i] * cp[i - 1] if i else 0)
            cp[i] = up[i] / piv
            dp[i] = (rhs[i] - (lo_[i] * dp[i - 1] if i else 0)) / piv
        M = [mpmath.mpf(0)] * (m + 1)
        M[m - 1] = dp[cnt - 1]
        for i in range(cnt - 2, -1, -1):
            M[i + 1] = dp[i] - cp[i] * M[i + 2]
        M[0] = (1 + r0) * M[1] - r0 * M[2]
        M[m] = (1 + rm) * M[m - 1] - rm * M[m - 2]
    inner = np.asarray(s[1:m], dtype=np.int64)

    def seg(i):                                     # numba_splev's interval: s_j <= i < s_{j+1}, the last one closed
        return np.searchsorted(inner, i, side="right")

    return _evaluate(n, s, Y, M, seg, samples=samples)


# ---- layouts ------------------------------------------------------------------------------------------------------------
def alternating_values(m, rng, amp=1.0, offset=0.0, jitter=0.5):
    """m knot values that alternate strictly around offset: offset + (-1)^k amp (1 + jitter u_k), u_k in [0, 1)."""
    sign = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
    return offset + sign * amp * (1.0 + jitter * rng.random(m))


def zigzag(n, knots, values):
    """float64[n], linear between consecutive knots and strictly monotone on every segment, so that the knots are
    exactly its strict alternating extrema.  knots: strictly increasing in [1, n-2]; values: strictly alternating.
    The ends run towards the neighbouring knot's value (x[0] = values[1], x[n-1] = values[-2])."""
    kn = np.asarray(knots, dtype=np.int64)
    v = np.asarray(values, dtype=np.float64)
    if kn.size < 2 or kn[0] < 1 or kn[-1] > n - 2 or np.any(np.diff(kn) <= 0):
        raise ValueError("knots: at least 2, strictly increasing, inside [1, n-2]")
    d = np.diff(v)
    if np.any(d == 0) or np.any(d[1:] * d[:-1] >= 0):
        raise ValueError("values must alternate strictly")
    pos = np.concatenate(([0], kn, [n - 1]))
    val = np.concatenate(([v[1]], v, [v[-2]]))
    i = np.arange(n, dtype=np.int64)
    j = np.clip(np.searchsorted(pos, i, side="right") - 1, 0, pos.size - 2)
    p0, p1 = pos[j], pos[j + 1]
    t = (i - p0).astype(np.float64) / (p1 - p0).astype(np.float64)
    x = val[j] + (val[j + 1] - val[j]) * t
    x[kn] = v                                       # exact at the knots
    x[n - 1] = val[-1]
    seg_d = np.diff(x)
    want = np.sign(val[j + 1] - val[j])[:-1]
    if np.any(np.sign(seg_d) != want):
        raise ValueError("the zigzag is not strictly monotone between knots (spacing too long for the value step)")
    return x


def knots_from_spacings(first, h):
    """Knot positions first, first + h_0, first + h_0 + h_1, ..."""
    return np.concatenate(([first], first + np.cumsum(np.asarray(h, dtype=np.int64)))).astype(np.int64)
