"""The numpy statement of the instantaneous stream's rule (include/pyitd_hip.h, itd_inst_stream_*) — a plain
helper of the tests; nothing here knows of rings, slots or LDS.

Per sample j of the flushed row x (P L samples), on absolute indices (i is a crossing index iff i >= 1, x[i+1] exists and the sign
changes strictly between x[i] and x[i+1]; a crossing index is the last sample of its half wave):
    len[j]       the samples of j's half wave
    A[j]         max |x| over it
    phase[j]     phase_np (spectrum_stream_ref: the case split of phase_in) of x[j], the forward difference x[j+1] - x[j] (the row's
                 last sample: the backward one) and A[j]
    f[j]         (phase[j+1] - phase[j], + 2 pi where negative) / (2 pi); the row's last sample: phase[j] - phase[j-1]
    long[j]      len[j] > H
    overlong[j]  spectrum_stream_ref.overlong_of: long[j], or long[j+1] where j + 1 exists, or for the row's last sample long[j-1]
and what is delivered:
    amplitude, phase   A, phase where not long, else NONE        frequency   f where not overlong, else NONE
    length             len (int32) where not long, else 0        NONE        the one pattern 0x7FF8000000000000

whole_row_features(x, H) states this on the whole row, from the half waves of tests/waves_ref.py.  block_features(x, L, H, b) states
block b from x[b L - H, (b+1) L + H] clipped to what exists and from nothing else: a half wave whose begin (end) is not found inside
that range is long, unless the range begins at the row's start (ends at the row's end).
Both return (amplitude, phase, frequency, length, long, overlong): float64 x 3, int32, bool x 2, one value per sample.
"""
import numpy as np

from spectrum_stream_ref import freq_np, overlong_of, phase_np
from waves_ref import ref_table

NONE_BITS = np.uint64(0x7FF8000000000000)
NONE = np.array([NONE_BITS]).view(np.float64)[0]


def deliver(A, ph, f, ln, long_, overlong):
    """what leaves the stream, from the full per-sample quantities and the two masks"""
    return (np.where(long_, NONE, A), np.where(long_, NONE, ph), np.where(overlong, NONE, f), np.where(long_, 0, ln).astype(np.int32),
            long_.copy(), overlong.copy())


def whole_row_features(x, H):
    x = np.ascontiguousarray(x, dtype=np.float64)
    _, length, _, value = ref_table(x)
    ln = np.repeat(length.astype(np.int64), length)
    A = np.repeat(np.abs(value), length)
    slope = np.append(x[1:] - x[:-1], x[-1] - x[-2])
    ph = phase_np(x, slope, A)
    f = freq_np(np.append(ph[1:] - ph[:-1], ph[-1] - ph[-2]))
    return deliver(A, ph, f, ln, ln > H, overlong_of(ln, H))


def block_features(x, L, H, b):
    n = x.size
    lo, hi = max(b * L - H, 0), min((b + 1) * L + H + 1, n)
    w = np.array(x[lo:hi], dtype=np.float64)                  # everything below reads w only
    from_start, to_end = lo == 0, hi == n
    m = w.size
    with np.errstate(invalid="ignore"):
        cross = np.append(((w[:-1] > 0) & (w[1:] < 0)) | ((w[:-1] < 0) & (w[1:] > 0)), False)
    if from_start:
        cross[0] = False                                      # index 0 of the row is never a crossing index
    cidx = np.flatnonzero(cross)
    k0 = b * L - lo                                           # the block's first sample in w
    ext = k0 + L < m                                          # sample (b+1) L exists: its phase gives the last sample's frequency
    cnt = L + 1 if ext else L
    A, ln, long_ = np.zeros(cnt), np.zeros(cnt, np.int64), np.zeros(cnt, bool)
    for i in range(cnt):
        k = k0 + i
        p = int(np.searchsorted(cidx, k, "left"))             # the crossing indices in front of k
        first = int(cidx[p - 1]) + 1 if p > 0 else (0 if from_start else None)
        end = int(cidx[p]) if p < cidx.size else (m - 1 if to_end else None)
        if first is None or end is None or end - first + 1 > H:
            long_[i] = True
        else:
            ln[i] = end - first + 1
            A[i] = np.abs(w[first:end + 1]).max()
    xs = w[k0:k0 + cnt]
    if ext:                                                   # (and then sample (b+1) L + 1 is readable too: H >= 1)
        slope = w[k0 + 1:k0 + cnt + 1] - xs
    else:                                                     # the block ends the row: its last sample takes the backward differences
        slope = np.append(xs[1:] - xs[:-1], xs[-1] - xs[-2])
    ph = phase_np(xs, slope, A)
    dp = ph[1:] - ph[:-1]
    overlong = long_[:L].copy()
    overlong[:cnt - 1] |= long_[1:]
    if not ext:
        dp = np.append(dp, ph[-1] - ph[-2])
        overlong[-1] |= long_[-2]
    return deliver(A[:L], ph[:L], freq_np(dp), ln[:L], long_[:L], overlong)
