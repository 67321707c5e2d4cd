"""The numpy statement of single-wave analysis (pyitd_amd.single_waves, pyitd_amd.wave_filter) — a plain helper of the tests.

On oracle.exact_tfe.structure()'s crossing flags and half-wave index, per half wave k of a row x (float64; a float32 row is
widened exactly first):
    start_k, end_k   its first and last sample; length_k = end_k - start_k + 1
    A_k              max |x| over it
    peak_k           the smallest index of the half wave with |x| == A_k
    value_k          x[peak_k]
and the filter: a sample of half wave k is kept iff amp_lo <= A_k <= amp_hi and len_lo <= length_k <= len_hi (IEEE comparisons
on float64), any other sample is +0.0.  Nothing here knows of tiles, records or scans.
"""
import numpy as np

from oracle import exact_tfe as et


def ref_table(x):
    """(start int32[count], length int32[count], peak int32[count], value float64[count])."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    _, hw, amp, _, _, _ = et.structure(x)
    n = x.size
    first = np.flatnonzero(np.concatenate(([True], hw[1:] != hw[:-1])))       # every half wave's first sample
    end = np.concatenate((first[1:] - 1, [n - 1]))
    at_max = np.flatnonzero(np.abs(x) == amp)                                 # ascending: a half wave's first one is its peak
    _, where = np.unique(hw[at_max], return_index=True)
    peak = at_max[where]
    assert peak.size == first.size
    return first.astype(np.int32), (end - first + 1).astype(np.int32), peak.astype(np.int32), x[peak].copy()


def ref_filter(x, bounds):
    """x with the samples of the half waves outside bounds = (amp_lo, amp_hi, len_lo, len_hi) set to +0.0 (float64)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    _, hw, amp, _, _, _ = et.structure(x)
    length = np.bincount(hw).astype(np.float64)[hw]
    amp_lo, amp_hi, len_lo, len_hi = (np.float64(b) for b in bounds)
    with np.errstate(invalid="ignore"):
        keep = (amp_lo <= amp) & (amp <= amp_hi) & (len_lo <= length) & (length <= len_hi)
    return np.where(keep, x, 0.0)
