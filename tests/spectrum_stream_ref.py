"""The numpy statement of the spectrum stream's rule (include/pyitd_hip.h, itd_spectrum_stream_*), block by
block — a plain helper of the tests.  Block b of a row x[0 .. P L) is decided from x[b L - H, (b+1) L + H] clipped to what exists and
from nothing else; nothing here knows of rings, slots or LDS.

For the samples j of block b and for sample (b+1) L where it exists, on absolute indices (i is a crossing index iff i >= 1, x[i+1]
lies inside the range read and the sign changes strictly between x[i] and x[i+1]):
    backward   the last crossing index c with b L - H <= c < j: the half wave begins at c + 1.  None: it begins at 0 if the range
               begins at the stream's start, else it is longer than H
    forward    the first crossing index c with j <= c and c + 1 <= (b+1) L + H: the half wave ends at c.  None: it ends at the last
               sample if the range ends at the (flushed) stream's end, else it is longer than H
    A          max |x| over the half wave; phase by phase_np (the case split of phase_in, numpy's arcsin), from the forward
               difference x[j+1] - x[j] (the stream's last sample: the backward one)
    f          (phase[j+1] - phase[j], + 2 pi where negative) / (2 pi); the stream's last sample: phase[j] - phase[j-1]
    overlong   the half wave of j is longer than H, or j + 1 exists and its half wave is; the stream's last sample (it has no
               successor, its frequency needs A of its predecessor): or its predecessor's half wave is
and then spectrum_ref.spectrum_from_bins on the block's L samples with the overlong samples forced outside.

whole_row_* is the same statement without locality: the half waves of tests/waves_ref.py on the whole row.
"""
import numpy as np

import spectrum_ref as sr
from waves_ref import ref_table


def phase_np(x, slope, A):
    """phase_in of itd_halfwave.hpp elementwise: 0 where A is not > 0, else the three cases on asin(clip(x / A))."""
    x, slope, A = (np.asarray(v, dtype=np.float64) for v in (x, slope, A))
    ok = A > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(ok, x / np.where(ok, A, 1.0), 0.0)
    a = np.arcsin(np.clip(r, -1.0, 1.0))
    ph = np.where(x >= 0, np.where(slope >= 0, a, np.pi - a), np.where(slope < 0, np.pi - a, 2.0 * np.pi + a))
    return np.where(ok, ph, 0.0)


def freq_np(dp):
    dp = np.where(dp < 0, dp + 2.0 * np.pi, dp)
    return dp / (2.0 * np.pi)


def overlong_of(lengths_per_sample, H):
    """sample j is overlong: its half wave is longer than H, or its successor's is; the row's last sample, whose frequency is the
    backward difference: or its predecessor's is"""
    long_ = lengths_per_sample > H
    out = long_.copy()
    out[:-1] |= long_[1:]
    out[-1] |= long_[-2]
    return out


def whole_row_inst(x):
    """(A, f, length of every sample's half wave) of the whole row: the instantaneous step in numpy."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    start, length, _, value = ref_table(x)
    A = np.repeat(np.abs(value), length)
    ln = np.repeat(length.astype(np.int64), length)
    slope = np.empty_like(x)
    slope[:-1] = x[1:] - x[:-1]
    slope[-1] = x[-1] - x[-2]
    ph = phase_np(x, slope, A)
    dp = np.empty_like(x)
    dp[:-1] = ph[1:] - ph[:-1]
    dp[-1] = ph[-1] - ph[-2]
    return A, freq_np(dp), ln


def masked_spectrum(A, f, overlong, edges, hop, weight):
    """(power[T, F], outside[T], overlong[T]) of section 19's definition with the overlong samples forced outside."""
    edges = np.asarray(edges, dtype=np.float64)
    k, inside = sr.bins_of(f, edges)
    inside = inside & ~overlong
    S, outside = sr.spectrum_from_bins(sr.weights_of(A, weight), k, inside, edges.size - 1, hop)
    T = S.shape[0]
    ovl = np.bincount(np.flatnonzero(overlong) // hop, minlength=T).astype(np.int32)
    return S, outside, ovl


def whole_row_spectrum(x, H, edges, hop, weight):
    A, f, ln = whole_row_inst(x)
    return masked_spectrum(A, f, overlong_of(ln, H), edges, hop, weight)


def block_inst(x, L, H, b):
    """(A[L], f[L], overlong bool[L]) of block b of the flushed row x (P L samples), from x[b L - H, (b+1) L + H] alone."""
    n = x.size
    lo, hi = max(b * L - H, 0), min((b + 1) * L + H + 1, n)
    at_start, at_end = lo == 0, hi == n
    w = np.array(x[lo:hi], dtype=np.float64)                  # everything below reads w only
    m = w.size
    cross = np.zeros(m, bool)
    with np.errstate(invalid="ignore"):
        cross[:m - 1] = ((w[:-1] > 0) & (w[1:] < 0)) | ((w[:-1] < 0) & (w[1:] > 0))
    if lo == 0:
        cross[0] = False                                      # index 0 of the stream is never a crossing index
    cidx = np.flatnonzero(cross)
    k0 = b * L - lo                                           # the block's first sample in w
    cnt = L + 1 if k0 + L < m else L                          # with sample (b+1) L where it exists
    A = np.zeros(cnt)
    long_ = np.zeros(cnt, bool)
    known = {}
    for i in range(cnt):
        k = k0 + i
        p = int(np.searchsorted(cidx, k, "left"))             # crossings in front of k
        s = int(cidx[p - 1]) + 1 if p > 0 else (0 if at_start else None)
        e = int(cidx[p]) if p < cidx.size else (m - 1 if at_end else None)
        if s is None or e is None or e - s + 1 > H:
            long_[i] = True                                   # (its amplitude is never used: the sample and the one before are outside)
            continue
        if (s, e) not in known:
            known[(s, e)] = np.abs(w[s:e + 1]).max()
        A[i] = known[(s, e)]
    xs = w[k0:k0 + cnt]
    slope = np.empty(cnt)
    last = k0 + cnt == m and at_end                           # the row's last sample is the last one taken here
    nxt = w[k0 + 1:k0 + cnt + 1]
    slope[:nxt.size] = nxt - xs[:nxt.size]
    if last:
        slope[-1] = xs[-1] - xs[-2]
    ph = phase_np(xs, slope, A)
    dp = np.empty(L)
    dp[:cnt - 1] = ph[1:] - ph[:-1]
    if cnt == L:
        dp[-1] = ph[-1] - ph[-2]
    overlong = long_[:L].copy()
    overlong[:cnt - 1] |= long_[1:]
    if last:
        overlong[-1] |= long_[-2]
    return A[:L], freq_np(dp), overlong


def ref_stream_block(x, L, H, b, edges, hop, weight):
    """(power[C, F], outside[C], overlong[C]) of block b, C = L / hop."""
    A, f, overlong = block_inst(np.ascontiguousarray(x, dtype=np.float64), L, H, b)
    return masked_spectrum(A, f, overlong, edges, hop, weight)


def envelope(n, rng):
    """a smooth positive envelope: the run-length signals' frequencies spread under it"""
    t = np.arange(n)
    return 1.0 + 0.6 * np.sin(2 * np.pi * t / rng.uniform(9.0, 40.0) + rng.uniform(0, 6.0)) + 0.3 * np.cos(2 * np.pi * t / rng.uniform(3.0, 7.0))
