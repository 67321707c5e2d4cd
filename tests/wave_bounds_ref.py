"""The numpy statement of the wave filter's bounds from histogram quantiles (pyitd_amd.wave_filter_bounds, itd_wave_bounds_batch,
streaming.WaveBoundsStream) — a plain helper of the tests.

A row has a histogram h[T][Na][Nl] of non-negative int32 cells, a range of time bins [t0, t1), edges ae[0..Na], le[0..Nl] and eight
float64 parameters q = (aq_lo, aq_hi, lq_lo, lq_hi, as_lo, as_hi, ls_lo, ls_hi).  In int64: ma[i] = sum over t and j, ml[j] = sum
over t and i, N = sum ma = sum ml.  One axis with marginal m[0..B), edges e[0..B] and inclusive prefix sums cum:
    N == 0      iL = 0, iU = B - 1
    otherwise   tau_lo = q_lo * (double)N, tau_hi = q_hi * (double)N (one IEEE multiply each);
                iL = the smallest i with (double)cum[i] > tau_lo; none: the smallest i with cum[i] == N
                iU = max(iL, the smallest i with (double)cum[i] >= tau_hi; none: B - 1)
    lo = e[iL] * s_lo, hi = e[iU + 1] * s_hi (one IEEE multiply each)
Nothing here knows of parts, workspaces, rings or wavefronts.
"""
import numpy as np


def axis_indices(m, q_lo, q_hi):
    """(iL, iU, N) of one axis's marginal m[B] (integers)."""
    m = np.asarray(m, dtype=np.int64)
    B = m.size
    cum = np.cumsum(m)
    N = int(cum[-1])
    if N == 0:
        return 0, B - 1, 0
    c = cum.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        tau_lo, tau_hi = np.float64(q_lo) * np.float64(N), np.float64(q_hi) * np.float64(N)
        above, reach = np.flatnonzero(c > tau_lo), np.flatnonzero(c >= tau_hi)
    iL = int(above[0]) if above.size else int(np.flatnonzero(cum == N)[0])
    iU = max(iL, int(reach[0]) if reach.size else B - 1)
    return iL, iU, N


def axis_bounds(m, e, q_lo, q_hi, s_lo=1.0, s_hi=1.0):
    """(lo, hi, N) of one axis: its marginal m[B], its edges e[B + 1]."""
    e = np.asarray(e, dtype=np.float64)
    iL, iU, N = axis_indices(m, q_lo, q_hi)
    with np.errstate(invalid="ignore", over="ignore"):
        return e[iL] * np.float64(s_lo), e[iU + 1] * np.float64(s_hi), N


def marginals(h, t0=0, t1=None):
    """(ma[Na], ml[Nl]) in int64 of the time bins [t0, t1) of h[T][Na][Nl]."""
    h = np.asarray(h)
    part = h[t0:h.shape[0] if t1 is None else t1].astype(np.int64)
    return part.sum(axis=(0, 2)), part.sum(axis=(0, 1))


def ref_bounds(h, ae, le, q=(0.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0), t0=0, t1=None):
    """(bounds float64[4] = (amp_lo, amp_hi, len_lo, len_hi), N) of one row's histogram h[T][Na][Nl]."""
    ma, ml = marginals(h, t0, t1)
    alo, ahi, N = axis_bounds(ma, ae, q[0], q[1], q[4], q[5])
    llo, lhi, N2 = axis_bounds(ml, le, q[2], q[3], q[6], q[7])
    assert N == N2
    return np.array([alo, ahi, llo, lhi], dtype=np.float64), N


def ref_bounds_rows(hist, ae, le, q, t0=0, t1=None):
    """ref_bounds of every row of hist[R][T][Na][Nl]; ae, le, q: one set ([N + 1] / [8]) or one per row.  (bounds[R, 4], N int64[R])."""
    ae, le, q = (np.asarray(v, dtype=np.float64) for v in (ae, le, q))
    out = [ref_bounds(h, ae[r] if ae.ndim == 2 else ae, le[r] if le.ndim == 2 else le, q[r] if q.ndim == 2 else q, t0, t1)
           for r, h in enumerate(hist)]
    return np.stack([b for b, _ in out]), np.array([n for _, n in out], dtype=np.int64)


class RefBoundsStream:
    """The windowed form as the stream keeps it: the marginals of the last W pushes and their running sums, nothing else."""

    def __init__(self, window):
        self.W, self.ring, self.run = int(window), [], None

    def reset(self):
        self.ring, self.run = [], None

    def push(self, slices, ae, le, q=(0.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0)):
        """slices[C][Na][Nl] of one row: (bounds[4], N) of the last min(W, pushes) pushes."""
        ma, ml = marginals(slices)
        if self.run is None:
            self.run = [np.zeros_like(ma), np.zeros_like(ml)]
        if len(self.ring) == self.W:
            old = self.ring.pop(0)
            self.run = [self.run[0] - old[0], self.run[1] - old[1]]
        self.ring.append((ma, ml))
        self.run = [self.run[0] + ma, self.run[1] + ml]
        alo, ahi, N = axis_bounds(self.run[0], ae, q[0], q[1], q[4], q[5])
        llo, lhi, _ = axis_bounds(self.run[1], le, q[2], q[3], q[6], q[7])
        return np.array([alo, ahi, llo, lhi], dtype=np.float64), N


def window_range(p, W, C):
    """[t0, t1) of the concatenated slices that push p (counted from 0) of a stream with window W and C slices per push answers for."""
    return max(0, p + 1 - W) * C, (p + 1) * C


def bits(a):
    """The float64 bit patterns, every NaN as one pattern: which NaN inf * 0 gives (its sign) is the processor's choice, not IEEE's."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))
