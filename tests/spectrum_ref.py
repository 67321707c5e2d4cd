"""The numpy statement of the time-frequency-energy spectrum's definition (include/pyitd_hip.h): what
itd_tfe_spectrum_* / pyitd_amd.tfe_spectrum must deliver bit for bit, given a row's instantaneous amplitude A and frequency f.

    bin of sample j     k = searchsorted(edges, f, "right") - 1 where edges[0] <= f < edges[-1]; every other sample (NaN too) is outside
    step sum            the 64 samples of step s, each in its own bin's column of a dense [steps, 64, F] array of masked weights
                        (+0.0 elsewhere), reduced by the adjacent-pair tree: v = v[:, 0::2] + v[:, 1::2], six times
    cell                S[t] = +0.0, then += the step sums of the steps with 64 s // hop == t, one after the other
    outside[t]          the outside samples with j // hop == t
"""
import numpy as np

WEIGHTS = ("count", "amplitude", "energy")


def bins_of(f, edges):
    """(k int64[n], inside bool[n]): the frequency bin of every sample, valid where inside."""
    f = np.asarray(f, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = (f >= edges[0]) & (f < edges[-1])
    k = np.searchsorted(edges, np.where(inside, f, edges[0]), "right") - 1
    return k, inside


def weights_of(A, weight):
    A = np.asarray(A, dtype=np.float64)
    if weight == "count":
        return np.ones(A.size)
    if weight == "amplitude":
        return A
    if weight == "energy":
        with np.errstate(over="ignore"):
            return A * A
    raise KeyError(weight)


def spectrum_from_bins(w, k, inside, F, hop):
    """(S float64[T, F], outside int32[T]) of weights w with bins k (valid where inside)."""
    n = w.size
    steps, T = -(-n // 64), -(-n // hop)
    j = np.arange(n)
    v = np.zeros((steps * 64, F))
    v[j[inside], k[inside]] = w[inside]
    v = v.reshape(steps, 64, F)
    with np.errstate(over="ignore"):
        for _ in range(6):
            v = v[:, 0::2] + v[:, 1::2]
        S = np.zeros((T, F))
        for s in range(steps):
            S[64 * s // hop] += v[s, 0]
    outside = np.bincount(j[~inside] // hop, minlength=T).astype(np.int32)
    return S, outside


def spectrum_ref(A, f, edges, hop, weight):
    """The spectrum of one row from its instantaneous amplitude and frequency."""
    edges = np.asarray(edges, dtype=np.float64)
    k, inside = bins_of(f, edges)
    return spectrum_from_bins(weights_of(A, weight), k, inside, edges.size - 1, hop)


def uniform_edges(F, lo=0.0, hi=0.5):
    return np.linspace(lo, hi, F + 1)


def log_edges(F, lo=1e-4, hi=0.5):
    return np.geomspace(lo, hi, F + 1)


def pi_edges(F):
    """(k + 1 / pi) / (F + 1), k = 0 .. F: inside (0, 1), away from every frequency a short exact ratio gives."""
    return (np.arange(F + 1) + 1.0 / np.pi) / (F + 1)
