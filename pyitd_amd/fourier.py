"""The ITD-Fourier cascade of itd_fourier_decomposition.py (:131-303) on the GPU.

  fourier_mode_decomposition_any(rotation)    :171-209   one rotation -> its Fourier mode (zeros when rejected)
  fourier_mode_decomposition_valid(rotation)  :131-168
  itd_fourier_decomposition(signal, sample_rate)        :212-255   [modes of row 0..., row 0, modes of row 1..., row 1, ..., residual]
  itd_fourier_decomposition_lean(signal, sample_rate)   :258-303   [accumulated modes 0, row 0, ..., residual]
plus *_batch forms over signals of one length and one sample rate.

The band plan (itd_sine_wrapper :33-47: the knots of every band are the zero crossings of a sine made by numpy, find_extrema) is
built once per (n, sample_rate) on the host; the bands, the FFTs, the selection, the mode test and the next signal run on the device
with one host synchronisation per round (itd_fourier_cascade_host_f64).  Upstream, the lean cascade calls the undefined
`itd_fourier_wrapper` (:269, :276); it is read as itd_sine_wrapper, the file's only wrapper.
The reference prints its progress; here that is `verbose=True`.  The reference loops until no row yields a mode; `max_rounds`
caps the rounds (default: no cap).
"""
import ctypes

import numpy

from ._place import Numpy
from .engine import _np_ptr
from .itd import _engine_for, find_extrema, generate_sine_wave

_NO_CAP = 2 ** 31 - 1
_plans = {}


def band_plan(n, sample_rate, device=0):
    """The knot lists of itd_sine_wrapper's bands for signals of n samples: (knots int64 back to back, idx int64 per band).
    Raises IndexError where a band's extrapolated last knot lies beyond the signal, as itd_sine_wrapper does."""
    key = (int(n), float(sample_rate), int(device))
    plan = _plans.get(key)
    if plan is not None:
        return plan
    duration = n / sample_rate
    frequencies = numpy.arange(2, sample_rate // 2 - 1, 96)[::-1]
    lists, idxs = [], []
    for k in range(1, frequencies.size):
        ext, idx = find_extrema(generate_sine_wave(frequencies[k], sample_rate, duration), device)
        ext = numpy.asarray(ext)
        if idx + 1 > ext.shape[0]:
            raise IndexError("index %d is out of bounds for axis 0 with size %d" % (idx, ext.shape[0]))
        used = ext[: idx + 1]
        over = used[used >= n]
        if over.size:
            raise IndexError("index %d is out of bounds for axis 0 with size %d" % (int(over[0]), n))
        if idx < 2:
            raise ValueError("band %d (%g Hz) has fewer than two knots in %d samples" % (k, frequencies[k], n))
        lists.append(used.astype(numpy.int64))
        idxs.append(idx)
    plan = (numpy.concatenate(lists) if lists else numpy.zeros(0, numpy.int64), numpy.asarray(idxs, dtype=numpy.int64))
    _plans[key] = plan
    return plan


def _signals(signals):
    x = numpy.ascontiguousarray(numpy.asarray(signals, dtype=numpy.float64))
    if x.ndim != 2 or x.shape[1] < 4:
        raise ValueError("expected signals[B, N] with N >= 4")
    return x


def _cascade(x, sample_rate, lean, max_rounds, device):
    B, n = x.shape
    knots, idx = band_plan(n, sample_rate, device)
    K = idx.shape[0]
    cap = _NO_CAP if max_rounds is None else int(max_rounds)
    if cap < 1:
        raise ValueError("max_rounds must be >= 1")
    if K == 0:      # no band: itd_sine_wrapper returns the signal alone, no row yields a mode
        z = numpy.zeros(B, numpy.int32)
        return x[:, None, :].copy(), None, z, z.copy(), numpy.zeros(B, numpy.int64), numpy.zeros((0, 8), numpy.int32), None
    eng = _engine_for(n, device)
    rows = numpy.empty((B, K + 1, n))
    acc = numpy.empty((B, K, n)) if lean else None
    rounds = numpy.zeros(B, numpy.int32)
    capped = numpy.zeros(B, numpy.int32)
    counts = numpy.zeros(B, numpy.int64)
    rc = eng._L.itd_fourier_cascade_host_f64(eng._h, _np_ptr(x), n, B, float(sample_rate), K, _np_ptr(knots), _np_ptr(idx), 1 if lean else 0,
                                             cap, _np_ptr(rows), _np_ptr(acc), _np_ptr(rounds), _np_ptr(capped), _np_ptr(counts))
    if rc == 6:
        raise ValueError("the signal contains NaN (the cubic operator has no NaN branch upstream)")
    eng._check(rc)
    total = int(counts.sum())
    recs = numpy.zeros((total, 8), numpy.int32)
    modes = None if lean else numpy.empty((total, n))
    eng._check(eng._L.itd_fourier_modes_f64(eng._h, _np_ptr(modes), total, _np_ptr(recs), 1))
    return rows, acc, rounds, capped, counts, recs, modes


def _print_progress(recs, rounds, n_modes):
    for r in range(1, int(rounds) + 1):
        print("Iteration %d: Found %d Fourier modes" % (r, int((recs[:, 1] == r).sum())))
    print("No more Fourier modes found, finalizing decomposition...")
    print("Total decomposition complete: %d Fourier modes extracted over %d iterations" % (n_modes, int(rounds)))


def itd_fourier_decomposition_batch(signals, sample_rate, lean=False, max_rounds=None, verbose=False, return_info=False, device=0):
    """The cascade of every signal of signals[B, N] (one length, one sample rate) in one call.  Returns a list of B output lists
    (each as itd_fourier_decomposition / _lean returns it); with return_info also a list of B dicts: rounds (rounds that found
    modes: the reference's iteration count), capped (stopped at max_rounds), records int32[m, 7] (round, source row, peak_max,
    first_peak, last_peak, mina, minb per mode, in the order found)."""
    x = _signals(signals)
    rows, acc, rounds, capped, counts, recs, modes = _cascade(x, sample_rate, lean, max_rounds, device)
    K = rows.shape[1] - 1
    outs, infos = [], []
    for b in range(x.shape[0]):
        sel = numpy.flatnonzero(recs[:, 0] == b)
        r = recs[sel]
        out = []
        for i in range(K):
            if lean:
                out.append(acc[b, i])
            else:
                out.extend(modes[j] for j in sel[r[:, 2] == i])
            out.append(rows[b, i])
        out.append(rows[b, K])
        outs.append(out)
        if verbose:
            _print_progress(r, rounds[b], int(counts[b]))
        infos.append({"rounds": int(rounds[b]), "capped": bool(capped[b]), "records": r[:, 1:].copy()})
    return (outs, infos) if return_info else outs


def itd_fourier_decomposition(signal, sample_rate, max_rounds=None, verbose=False, return_info=False, device=0):
    """itd_fourier_decomposition.py:212-255: the modes found in each rotation, by source row, each followed by the row it came
    from, then the residual."""
    x = numpy.asarray(signal, dtype=numpy.float64)
    if x.ndim != 1:
        raise ValueError("expected a 1-D signal")
    res = itd_fourier_decomposition_batch(x[None, :], sample_rate, False, max_rounds, verbose, return_info, device)
    return (res[0][0], res[1][0]) if return_info else res[0]


def itd_fourier_decomposition_lean(signal, sample_rate, max_rounds=None, verbose=False, return_info=False, device=0):
    """itd_fourier_decomposition.py:258-303 (its `itd_fourier_wrapper` read as itd_sine_wrapper): [accumulated modes of row 0,
    row 0, ..., residual]."""
    x = numpy.asarray(signal, dtype=numpy.float64)
    if x.ndim != 1:
        raise ValueError("expected a 1-D signal")
    res = itd_fourier_decomposition_batch(x[None, :], sample_rate, True, max_rounds, verbose, return_info, device)
    return (res[0][0], res[1][0]) if return_info else res[0]


def fourier_mode_batch(rows, rule="any", device=0):
    """The selector over rows[B, N] at once: (modes float64[B, N], records int32[B, 6]: status, peak_max, first_peak, last_peak,
    mina, minb; -1 where the rule did not get that far)."""
    x = _signals(rows)
    B, n = x.shape
    eng = _engine_for(n, device)
    fn = {"any": eng._L.itd_fourier_mode_any_f64, "valid": eng._L.itd_fourier_mode_valid_f64}[rule]
    with Numpy(device) as S:        # one buffer: the rows, the modes, the records
        buf = S.empty(2 * x.nbytes + B * 32, numpy.uint8)
        buf.upload(x)
        eng._check(fn(eng._h, buf.ptr, n, B, n, buf.ptr + x.nbytes, n, buf.ptr + 2 * x.nbytes, None))
        modes = buf.download(numpy.empty((B, n)), x.nbytes)
        recs = buf.download(numpy.empty((B, 8), numpy.int32), 2 * x.nbytes)
    return modes, recs[:, :6].copy()


def fourier_mode_decomposition_any(rotation, device=0):
    """itd_fourier_decomposition.py:171-209."""
    x = numpy.asarray(rotation, dtype=numpy.float64)
    return fourier_mode_batch(x[None, :], "any", device)[0][0]


def fourier_mode_decomposition_valid(rotation, device=0):
    """itd_fourier_decomposition.py:131-168."""
    x = numpy.asarray(rotation, dtype=numpy.float64)
    return fourier_mode_batch(x[None, :], "valid", device)[0][0]


def debug_fft(x, inverse=False, device=0):
    """The engine's FFT of x[B, N] complex (tests): numpy.fft.fft / ifft along the last axis."""
    z = numpy.ascontiguousarray(numpy.atleast_2d(numpy.asarray(x, dtype=numpy.complex128)))
    B, n = z.shape
    eng = _engine_for(max(n, 3), device)
    with Numpy(device) as S:
        buf = S.empty(2 * z.nbytes, numpy.uint8)
        buf.upload(z)
        eng._check(eng._L.itd_debug_fft_f64(eng._h, ctypes.c_void_p(buf.ptr), ctypes.c_void_p(buf.ptr + z.nbytes), n, B, 1 if inverse else 0))
        return buf.download(numpy.empty((B, n), numpy.complex128), z.nbytes)
