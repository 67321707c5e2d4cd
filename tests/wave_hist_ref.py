"""The numpy statement of the half waves' joint amplitude-length histogram (include/pyitd_hip.h): what
itd_wave_hist_batch_* / pyitd_amd.wave_histogram must deliver, integer for integer — a plain helper of the tests.

On waves_ref.ref_table's half waves (start, length, peak, value) of a row, with A = |value|:
    amplitude bin   i = searchsorted(ae, A, "right") - 1 where ae[0] <= A < ae[-1]
    length bin      j = searchsorted(le, float(length), "right") - 1 where le[0] <= length < le[-1]
    time bin        t = peak // hop, T = ceil(n / hop)
    both exist      count[t, i, j] += 1, samples[t, i, j] += length;   otherwise outside[t] += 1
Nothing here knows of tiles.
"""
import numpy as np

import waves_ref


def bin_of(v, edges):
    """(k int64[...], inside bool[...]): the half-open bin of every value between strictly increasing edges."""
    v, edges = np.asarray(v, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    inside = (edges[0] <= v) & (v < edges[-1])
    return np.searchsorted(edges, v, "right") - 1, inside


def hist_of_table(n, length, peak, value, ae, le, hop):
    """(count int32[T, Na, Nl], samples int32[T, Na, Nl], outside int32[T]) of a row's table of half waves."""
    ae, le = np.asarray(ae, dtype=np.float64), np.asarray(le, dtype=np.float64)
    Na, Nl, T = ae.size - 1, le.size - 1, -(-n // hop)
    i, in_a = bin_of(np.abs(value), ae)
    j, in_l = bin_of(length.astype(np.float64), le)
    t = peak.astype(np.int64) // hop
    ok = in_a & in_l
    count, samples = np.zeros((T, Na, Nl), np.int64), np.zeros((T, Na, Nl), np.int64)
    np.add.at(count, (t[ok], i[ok], j[ok]), 1)
    np.add.at(samples, (t[ok], i[ok], j[ok]), length[ok].astype(np.int64))
    outside = np.bincount(t[~ok], minlength=T)
    return count.astype(np.int32), samples.astype(np.int32), outside.astype(np.int32)


def default_hop(n):
    """What the wrapper passes for hop=None: the multiple of 512 that is >= n."""
    return -(-n // 512) * 512


def ref_hist(x, ae, le, hop=None, table=None):
    """The histogram of one row (float64; a float32 row is widened exactly first)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    _, length, peak, value = waves_ref.ref_table(x) if table is None else table
    return hist_of_table(x.size, length, peak, value, ae, le, default_hop(x.size) if hop is None else hop)
