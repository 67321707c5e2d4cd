"""The numpy statement of the histogram stream's rule (include/pyitd_hip.h, itd_hist_stream_*), block by block
— a plain helper of the tests.  Block b of a row x[0 .. P L) is decided from x[b L - H, (b+1) L + H) clipped to what exists and from
nothing else; nothing here knows of rings, slots or LDS.

Crossing indices and the ends of a half wave are found as in wave_stream_ref.ref_stream_block.  A half wave s..e that touches the
block, with the maxima of |x| ML left of the block, MB inside it and MR right of it:
    no begin or no end inside the range read, or e - s + 1 > H    each of its samples in the block adds 1 to overlong[cell]
    otherwise its peak lies in the block iff (s >= b L or ML < MB) and MR <= MB; then it is counted once, in the cell of the first
    sample of the block's part with |x| == MB, with wave_hist_ref's bins: count and samples, or outside

whole_row_hist is the statement the rule is held to: waves_ref.ref_table's half waves, those of at most H samples through
wave_hist_ref.hist_of_table, the others' samples into overlong.
"""
import numpy as np

import wave_hist_ref as whr
import waves_ref

NAMES = ("count", "samples", "outside", "overlong")


def ref_hist_block(x, L, H, b, ae, le, hop):
    """(count[C, Na, Nl], samples[C, Na, Nl], outside[C], overlong[C]) of block b of the flushed row x (P L samples), all int32."""
    ae, le = np.asarray(ae, dtype=np.float64), np.asarray(le, dtype=np.float64)
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
    cidx = np.flatnonzero(cross)
    mag = np.abs(w)
    o = b * L - lo                                            # the block's first sample in w
    C, Na, Nl = L // hop, ae.size - 1, le.size - 1
    count, samples = np.zeros((C, Na, Nl), np.int32), np.zeros((C, Na, Nl), np.int32)
    outside, overlong = np.zeros(C, np.int32), np.zeros(C, np.int32)
    j = o
    while j < o + L:                                          # j: the first sample of the block's part of the next half wave
        k = int(np.searchsorted(cidx, j))                     # cidx[k - 1] < j <= cidx[k]
        s = int(cidx[k - 1]) + 1 if k > 0 else (0 if at_start else None)
        e = int(cidx[k]) if k < cidx.size else (m - 1 if at_end else None)
        last = o + L - 1 if e is None else min(e, o + L - 1)  # the last sample of the block's part
        if s is None or e is None or e - s + 1 > H:
            np.add.at(overlong, (np.arange(j, last + 1) - o) // hop, 1)
        else:
            part = mag[j:last + 1]
            MB = part.max()
            here = (s >= o or mag[s:o].max() < MB) and (e < o + L or mag[o + L:e + 1].max() <= MB)
            if here:
                t = (j + int(np.argmax(part == MB)) - o) // hop
                length = e - s + 1
                (ia, in_a), (il, in_l) = whr.bin_of(MB, ae), whr.bin_of(np.float64(length), le)
                if in_a and in_l:
                    count[t, ia, il] += 1
                    samples[t, ia, il] += length
                else:
                    outside[t] += 1
        j = last + 1
    return count, samples, outside, overlong


def ref_hist_stream(x, L, H, ae, le, hop):
    """The concatenated slices of the whole stream for one row x of P L samples: count, samples [T, Na, Nl], outside, overlong [T]."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.ndim == 1 and x.size % L == 0 and x.size >= L and L % hop == 0
    blocks = [ref_hist_block(x, L, H, b, ae, le, hop) for b in range(x.size // L)]
    return tuple(np.concatenate([blk[i] for blk in blocks]) for i in range(4))


def whole_row_hist(x, H, ae, le, hop, table=None):
    """The whole-row statement (x.size a multiple of hop); table: waves_ref.ref_table(x) if the caller has it."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    start, length, peak, value = waves_ref.ref_table(x) if table is None else table
    ok = length <= H
    count, samples, outside = whr.hist_of_table(x.size, length[ok], peak[ok], value[ok], ae, le, hop)
    long_sample = np.zeros(x.size, np.int64)
    for s, ln in zip(start[~ok], length[~ok]):
        long_sample[s:s + ln] = 1
    overlong = long_sample.reshape(-1, hop).sum(axis=1).astype(np.int32)
    return count, samples, outside, overlong


def tied_maxima(x):
    """x with every half wave's largest magnitude repeated at its first and its last sample (its sign kept): ties between the parts of a
    half wave on both sides of a seam, where the earlier index must win."""
    x = np.array(x, dtype=np.float64)
    start, length, _, value = waves_ref.ref_table(x)
    for s, ln, v in zip(start, length, value):
        if v != 0.0:
            x[s] = x[s + ln - 1] = v
    return x


def same_ints(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == np.int32 and w.dtype == np.int32 and g.shape == w.shape, "%s %s: %s %s vs %s %s" % (
            what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), "%s: %s differs at %s" % (what, name, np.argwhere(g != w)[:4].tolist())
