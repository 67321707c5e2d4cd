"""The numpy statement of the wave-filter stream's rule (include/pyitd_hip.h, itd_wave_stream_*), block by
block — a plain helper of the tests.  Block b of a row x[0 .. P L) is decided from x[b L - H, (b+1) L + H) clipped to what exists
and from nothing else; nothing here knows of rings, slots or LDS.

For a sample j of block b, on absolute indices (i is a crossing index iff i >= 1, x[i+1] lies inside the range read and the sign
changes strictly between x[i] and x[i+1]):
    backward   the last crossing index c with b L - H <= c < j: the half wave begins at c + 1.  None: it begins at 0 if the range
               begins at the stream's start, else it is longer than H -> +0.0
    forward    the first crossing index c with j <= c and c + 1 < (b+1) L + H: the half wave ends at c.  None: it ends at the last
               sample if the range ends at the (flushed) stream's end, else it is longer than H -> +0.0
    keep       length <= H and amp_lo <= A <= amp_hi and len_lo <= length <= len_hi, A = max |x| over the half wave
"""
import numpy as np


def run_length_signal(rng, L, H, blocks, zeros=False):
    """Alternating-sign runs with lengths from {1, 2, 3, H-1, H, H+1, L, L+1, 2H+1}, amplitudes from a few values, each run's peak
    at its first, its last or an inner sample; some run boundaries forced onto b L - 1, b L, b L + 1; zeros: exact 0.0 and -0.0
    samples inside runs (they make no crossing).
    Whatever the draws, the row opens with a run of 2 samples and three runs of ONE sample with the amplitudes 0.25, 1.0 and 3.0 (so
    any amplitude window that splits these keeps and zeroes samples in every stream, however short), then, where 2 H + 7 samples
    fit, runs of H and H + 1 samples — a half wave of exactly the horizon and one a sample longer — and otherwise, where H + 6
    fit, one of H + 1: every row of at least H + 6 samples holds a half wave longer than H."""
    n = blocks * L
    lengths = [v for v in (1, 2, 3, H - 1, H, H + 1, L, L + 1, 2 * H + 1) if v >= 1]
    amps = (0.25, 1.0, 3.0)
    x = np.empty(n)
    forced = set()
    for b in range(1, blocks):
        forced.add(b * L + int(rng.integers(-1, 2)))
    pos, sign = 0, 1.0 if rng.random() < 0.5 else -1.0
    k0 = int(rng.integers(3))
    opening = [(2, None)] + [(1, amps[(k0 + i) % 3]) for i in range(3)]
    if n >= 2 * H + 7:
        opening += [(H, None), (H + 1, None)]
    elif n >= H + 6:
        opening += [(H + 1, None)]
    while pos < n:
        free = not opening
        ln, amp = opening.pop(0) if opening else (int(lengths[rng.integers(len(lengths))]), None)
        end = min(pos + ln, n)
        cut = [f for f in forced if pos < f < end]
        if cut and free and rng.random() < 0.7:
            end = min(cut)
        ln = end - pos
        run = np.full(ln, 0.125)
        run[[0, ln - 1, ln // 2][int(rng.integers(3))]] = amps[rng.integers(len(amps))] if amp is None else amp
        if zeros and ln >= 3:
            k = int(rng.integers(1, ln - 1))
            if run[k] == 0.125:
                run[k] = 0.0 if rng.random() < 0.5 else -0.0
        x[pos:end] = sign * run
        pos, sign = end, -sign
    return x


def ref_stream_block(x, L, H, b, bounds):
    """Block b of the stream's output for the flushed row x (P L samples), from x[b L - H, (b+1) L + H) alone."""
    n = x.size
    lo, hi = max(b * L - H, 0), min((b + 1) * L + H, n)
    at_start, at_end = lo == 0, hi == n
    w = np.array(x[lo:hi], dtype=np.float64)                  # everything below reads w only
    m = w.size
    cross = np.zeros(m, bool)
    with np.errstate(invalid="ignore"):
        cross[:m - 1] = ((w[:-1] > 0) & (w[1:] < 0)) | ((w[:-1] < 0) & (w[1:] > 0))
    if lo == 0:
        cross[0] = False                                      # index 0 of the stream is never a crossing index
    amp_lo, amp_hi, len_lo, len_hi = (np.float64(v) for v in bounds)
    out = np.zeros(L)
    cidx = np.flatnonzero(cross)
    for j in range(b * L, (b + 1) * L):
        k = j - lo
        before = cidx[cidx < k]
        after = cidx[cidx >= k]
        if before.size:
            s = int(before[-1]) + 1
        elif at_start:
            s = 0
        else:
            continue
        if after.size:
            e = int(after[0])
        elif at_end:
            e = m - 1
        else:
            continue
        length = e - s + 1
        A = np.abs(w[s:e + 1]).max()
        with np.errstate(invalid="ignore"):
            keep = length <= H and amp_lo <= A <= amp_hi and len_lo <= np.float64(length) <= len_hi
        if keep:
            out[j - b * L] = w[k]
    return out


def ref_stream_filter(x, L, H, bounds):
    """The whole stream's output for one row x of P L samples."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.ndim == 1 and x.size % L == 0 and x.size >= L
    return np.concatenate([ref_stream_block(x, L, H, b, bounds) for b in range(x.size // L)])
