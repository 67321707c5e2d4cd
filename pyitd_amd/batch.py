"""Row-wise / channel-wise forms of the single-level operators (numpy in -> numpy out) over the asynchronous batched entry
points of the C ABI (itd_baseline_extract_batch_f64, itd_detect_batch_f64, itd_baseline_extract_cubic_batch_f64), and the
instantaneous amplitude / phase / frequency of many rows (itd_instantaneous_batch_*; numpy or torch CUDA tensors) and their
single-wave analysis: the table of half waves, the feature filter and the half waves' joint amplitude-length histogram
(itd_waves_batch_*, itd_wave_filter_batch_*, itd_wave_hist_batch_*).

The reference applies its operators row by row under numba.prange (siftED2D.ipynb cell 1) and re-uses retained extrema along
channels (itd.cpp:40-44); here a whole batch is one launch sequence and no knot count crosses PCIe in between.  Every call is
written once against a placement (_place.py): numpy rows are staged through the C ABI's own allocator (no torch needed), a torch
CUDA tensor is used where it lies.
"""
from collections import namedtuple

import numpy

from ._lib import ITDError
from ._place import Numpy, Tensor, _is_torch, _np_dtype, _row_stride, rows_of
from .engine import DETECT_KNOTS, ITD_ERR_NONFINITE
from .itd import _engine_for, _wave_bounds_for


def _rows(x):
    x = numpy.ascontiguousarray(x, dtype=numpy.float64)
    if x.ndim != 2:
        raise ValueError("expected a 2-D array [signals, samples]")
    return x


def itd_baseline_extract_batch(x, device=0, want_counts=False):
    """itd_baseline_extract (ITD.py:79-121) of every row of x[B, n]: (rotation[B, n], baseline[B, n]).  Rows that hold a NaN
    are re-run one by one through the single-signal operator, which follows detect_peaks' NaN branch (ITD.py:46-51)."""
    x = _rows(x)
    B, n = x.shape
    eng = _engine_for(n, device)
    with Numpy(device, x) as S:
        d_rot, d_base, d_info = S.empty(x.shape, x.dtype), S.empty(x.shape, x.dtype), S.empty(B, numpy.int32)
        S.run(eng.extract_batch_dev, S.x, n, B, n, S.ptr(d_rot), n, S.ptr(d_base), n, S.ptr(d_info))
        info, rot, base = S.host(d_info), S.host(d_rot), S.host(d_base)
    counts = numpy.where(info < 0, -1 - info, info).astype(numpy.int64)
    for b in numpy.flatnonzero(info < 0):
        r, bs, kn, _ = eng.baseline_extract_host(x[b], want_knots=True)
        rot[b], base[b], counts[b] = r, bs, len(kn)
    return (rot, base, counts) if want_counts else (rot, base)


def count_knots_batch(x, mode=DETECT_KNOTS, device=0):
    """Number of knots of every row of x[B, n] under predicate `mode` (engine.DETECT_*, 3 = itd.cpp:161-168, 4 = sign
    changes); no index list is built or copied.  Rows that hold a NaN are counted by the single-signal operator."""
    x = _rows(x)
    B, n = x.shape
    eng = _engine_for(n, device)
    with Numpy(device, x) as S:
        d_info = S.empty(B, numpy.int32)
        S.run(eng.detect_batch_dev, S.x, n, B, n, mode, None, 0, S.ptr(d_info))
        info = S.host(d_info)
    out = info.astype(numpy.int64)
    for b in numpy.flatnonzero(info < 0):
        out[b] = len(eng.detect_host(x[b], mode)) if mode <= 2 else -1 - info[b]
    return out


def detect_knots_batch(x, mode=DETECT_KNOTS, device=0):
    """The ordered knot lists of every row of x[B, n] (list of int64 arrays)."""
    x = _rows(x)
    B, n = x.shape
    eng = _engine_for(n, device)
    stride = max(n - 2, 1)
    with Numpy(device, x) as S:
        d_idx, d_info = S.empty((B, stride), numpy.int32), S.empty(B, numpy.int32)
        S.run(eng.detect_batch_dev, S.x, n, B, n, mode, S.ptr(d_idx), stride, S.ptr(d_info))
        info, idx = S.host(d_info), S.host(d_idx)
    out = []
    for b in range(B):
        if info[b] < 0 and mode <= 2:
            out.append(eng.detect_host(x[b], mode))
        else:
            m = info[b] if info[b] >= 0 else -1 - info[b]
            out.append(idx[b, :m].astype(numpy.int64))
    return out


def itd_baseline_extract_fast_channels(x, extrema_input, idx, device=0):
    """itd_baseline_extract_fast (itd_fourier_decomposition.py:49-122) of every channel of x[C, n] on ONE retained knot list
    (itd.cpp:40-44: "simply estimate the extrema the first time ... retain the extrema ... reuse the extrema but evaluate and
    produce the baseline on new data").  extrema_input: idx + 1 entries; None: every channel's own extrema (itd.cpp:159-169).
    Returns baselines[C, n]; channels left without a spline (fewer than 2 knots) come back as zeros, like the reference's
    freshly allocated result."""
    x = _rows(x)
    C, n = x.shape
    eng = _engine_for(n, device)
    with Numpy(device, x) as S:
        d_base, d_info, d_e = S.full(x.shape, x.dtype, 0.0), S.empty(C, numpy.int32), None
        if extrema_input is not None:
            e = numpy.ascontiguousarray(extrema_input, dtype=numpy.int64)
            if e.shape[0] < idx + 1:
                raise ValueError("extrema_input needs idx+1 entries")
            if e[: idx + 1].min() < 0 or e[: idx + 1].max() >= n:
                raise IndexError("extrema outside the signal")      # what the reference's indexing would raise
            d_e = S.put(e[: idx + 1].astype(numpy.int32))
        S.run(eng.cubic_batch_dev, S.x, n, C, n, S.ptr(d_e), 0, 0 if d_e is None else int(idx), S.ptr(d_base), n, S.ptr(d_info))
        info = S.host(d_info)
        if (info == -1).any():
            raise ValueError("extrema_input must be strictly increasing")
        if (info == -2).any():
            raise ValueError("NaN in the signal (the cubic operator has no NaN branch)")
        return S.host(d_base)


_INSTANTANEOUS = ("amplitude", "phase", "frequency")


def _refuse_nan(info):
    bad = numpy.flatnonzero(info < 0)
    if bad.size:
        raise ITDError(ITD_ERR_NONFINITE, "NaN in rows %s%s" % (bad[:16].tolist(), " ..." if bad.size > 16 else ""))


def _out_dtype(out_dtype):
    odt = numpy.dtype(numpy.float64 if out_dtype is None else _np_dtype(out_dtype))
    if odt not in (numpy.dtype(numpy.float32), numpy.dtype(numpy.float64)):
        raise ValueError("out_dtype must be float32 or float64")
    return odt


def instantaneous_batch(rows, device=0, out_dtype=None, want=_INSTANTANEOUS):
    """Instantaneous amplitude, phase and frequency (pyitd_amd.instantaneous) of every row of rows[..., n] in one asynchronous
    call: the rows of a batched decomposition as itd_batch delivers them, float64 or float32 (widened exactly on the GPU).

    rows: a numpy array (staged through hipMalloc'd buffers; torch is not needed) or a torch CUDA tensor (used in place; its
    leading axes must collapse to one row stride, its last axis must be dense).  want: which of "amplitude", "phase", "frequency"
    to compute, in the order they are returned (a tuple of arrays with the input's shape; tensors on the input's device for a
    tensor).  out_dtype: None / float64, or float32 (numpy or torch): each element the float64 one rounded once on the GPU.
    Raises ITDError (non-finite) naming the rows that hold a NaN."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in _INSTANTANEOUS for w in want) or len(set(want)) != len(want):
        raise ValueError("want: a non-empty selection of %s without repeats, got %r" % (_INSTANTANEOUS, want))
    odt = _out_dtype(out_dtype)
    place, idt, shape, n, R, stride = rows_of(rows, "the instantaneous step", device)
    with place as S:
        outs = {w: S.empty(shape, odt) for w in want}
        info = S.empty(R, numpy.int32)
        eng = _engine_for(3, S.dev)
        S.run(eng.instantaneous_batch_dev, S.x, idt, n, R, stride, *[S.ptr(outs.get(w)) for w in _INSTANTANEOUS], n, odt == numpy.float32,
              S.ptr(info))
        _refuse_nan(S.host(info))
        return tuple(S.result(outs[w]) for w in want)


# ---- the time-frequency-energy spectrum (itd_tfe_spectrum_*) ---------------------------------------------------------------
Spectrum = namedtuple("Spectrum", "power outside")
_WEIGHTS = ("count", "amplitude", "energy")
MAX_BINS = 512


def _legal_hop(hop):
    """The spectrum's hop rule, the many-row call's and the stream's: a positive multiple of 64, below 512 only 64, 128 or 256."""
    return not isinstance(hop, bool) and int(hop) == hop and hop >= 64 and hop % 64 == 0 and (hop >= 512 or hop in (64, 128, 256))


def _spectrum_args(edges, hop, weight):
    """The checked (edges float64 [F + 1], hop, weight code) of tfe_spectrum."""
    if _is_torch(edges):
        edges = edges.detach().cpu().numpy()
    e = numpy.ascontiguousarray(edges, dtype=numpy.float64)
    if e.ndim != 1 or not 2 <= e.size <= MAX_BINS + 1:
        raise ValueError("edges: a 1-D array of 2 to %d entries, got shape %s" % (MAX_BINS + 1, e.shape))
    if not numpy.isfinite(e).all() or not (e[1:] > e[:-1]).all():
        raise ValueError("edges must be finite and strictly increasing")
    if not _legal_hop(hop):
        raise ValueError("hop: a positive multiple of 64 (below 512: 64, 128 or 256), got %r" % (hop,))
    if weight not in _WEIGHTS:
        raise ValueError("weight: one of %s, got %r" % (_WEIGHTS, weight))
    return e, int(hop), _WEIGHTS.index(weight)


def tfe_spectrum(rows, edges, hop, weight="energy", device=0):
    """The time-frequency-energy spectrum of every row of rows[..., n] in one asynchronous call: the row's instantaneous amplitude A
    and frequency f (instantaneous_batch; cycles per sample) binned over time — T = ceil(n / hop) bins of hop samples — and over
    frequency — F = len(edges) - 1 bins, sample j in bin k where edges[k] <= f[j] < edges[k+1].  Returns
    Spectrum(power[..., T, F] float64, outside[..., T] int32): power sums 1 ("count"), A ("amplitude") or A * A ("energy") over the
    samples of a cell; outside counts the samples of a time bin whose frequency lies in no bin.  The order of every sum is fixed
    (include/pyitd_hip.h): the result is the same bits from run to run and in any batch position, and A and f are never stored.

    rows: float64 or float32, a numpy array or a torch CUDA tensor (used in place; its leading axes must collapse to one row stride,
    its last axis must be dense; tensors come back on its device).  edges: 2 to 513 finite, strictly increasing values.  hop: a
    positive multiple of 64, below 512 only 64, 128 or 256.  The parallel grain is (row, time bin): a caller who wants the
    marginal spectrum sums a spectrum of many time bins rather than asking for hop >= n.  Raises ValueError for bad edges, hop or
    weight, ITDError (non-finite) naming the rows that hold a NaN."""
    e, hop, wcode = _spectrum_args(edges, hop, weight)
    place, idt, shape, n, R, stride = rows_of(rows, "the spectrum", device)
    F, T = e.size - 1, -(-n // hop)
    lead = shape[:-1]
    with place as S:
        power, outside, info, d_e = S.empty(lead + (T, F), numpy.float64), S.empty(lead + (T,), numpy.int32), S.empty(R, numpy.int32), S.put(e)
        eng = _engine_for(3, S.dev)
        S.run(eng.tfe_spectrum_dev, S.x, idt, n, R, stride, S.ptr(d_e), F, hop, wcode, S.ptr(power), T * F, S.ptr(outside), S.ptr(info))
        _refuse_nan(S.host(info))
        return Spectrum(S.result(power), S.result(outside))


# ---- single-wave analysis: the table of half waves and the feature filter (itd_waves_batch_*, itd_wave_filter_batch_*) -------
Waves =namedtuple("Waves", "count start length peak value")


def _refuse_overflow(count, cap):
    over = numpy.flatnonzero(count > cap)
    if over.size:
        raise ValueError("cap = %d is less than the half waves of rows %s%s (up to %d)"
                         % (cap, over[:16].tolist(), " ..." if over.size > 16 else "", int(count.max())))


def single_waves(rows, cap=None, device=0):
    """The half waves of every row of rows[..., n] — the runs of samples between strict sign changes, the waves the
    instantaneous amplitude is the maximum of — as a table: Waves(count[...], start[..., cap], length[..., cap], peak[..., cap],
    value[..., cap]).  Half wave k of a row begins at sample start, lasts length samples, attains its largest magnitude first at
    sample peak and has value = rows[..., peak] there (the signed extremum: its sign is the half wave's polarity).  Entries at or
    beyond a row's count are -1 (start, length, peak; int32) and nan (value; float64).

    rows: float64 or float32, a numpy array or a torch CUDA tensor (used in place; its leading axes must collapse to one row
    stride, its last axis must be dense; tensors come back on its device).  cap: the tables' last axis; None counts first and takes
    the largest count; an explicit cap makes one call and raises ValueError naming the rows with more half waves.  Raises
    ITDError (non-finite) naming the rows that hold a NaN."""
    if cap is not None:
        if int(cap) != cap or int(cap) < 1:
            raise ValueError("cap must be a positive integer or None, got %r" % (cap,))
        cap = int(cap)
    place, idt, shape, n, R, stride = rows_of(rows, "single-wave analysis", device)
    lead = shape[:-1]
    with place as S:
        count, info = S.empty(lead, numpy.int32), S.empty(R, numpy.int32)
        eng = _engine_for(3, S.dev)
        if cap is None:
            S.run(eng.waves_batch_dev, S.x, idt, n, R, stride, None, None, None, None, 0, 0, S.ptr(count), S.ptr(info))
            _refuse_nan(S.host(info))
            cap = int(S.host(count).max())
        tabs = [S.full(lead + (cap,), numpy.int32, -1) for _ in range(3)] + [S.full(lead + (cap,), numpy.float64, numpy.nan)]
        S.run(eng.waves_batch_dev, S.x, idt, n, R, stride, *[S.ptr(t) for t in tabs], cap, cap, S.ptr(count), S.ptr(info))
        _refuse_nan(S.host(info))
        counts = S.host(count)
        _refuse_overflow(counts, cap)
        return Waves(S.result(count, counts), *[S.result(t) for t in tabs])


def _wave_bounds(amplitude, length, lead):
    """The filter's bounds as float64 [4] (one set for every row) or [R, 4]; refuses NaN bounds and lo > hi."""
    cols = []
    for name, pair in (("amplitude", amplitude), ("length", length)):
        try:
            lo, hi = pair
        except (TypeError, ValueError):
            raise ValueError("%s: a pair (lo, hi), got %r" % (name, pair))
        lo, hi = numpy.asarray(lo, dtype=numpy.float64), numpy.asarray(hi, dtype=numpy.float64)
        if numpy.isnan(lo).any() or numpy.isnan(hi).any():
            raise ValueError("%s: a NaN bound" % name)
        try:
            both = numpy.broadcast_arrays(lo, hi)
        except ValueError:
            raise ValueError("%s: lo %s and hi %s do not broadcast" % (name, lo.shape, hi.shape))
        if (both[0] > both[1]).any():
            raise ValueError("%s: lo > hi" % name)
        cols += [lo, hi]
    if all(c.ndim == 0 for c in cols):
        return numpy.array([float(c) for c in cols])
    try:
        cols = [numpy.broadcast_to(c, lead) for c in cols]
    except ValueError:
        raise ValueError("the bounds (shapes %s) do not broadcast to the leading axes %s of rows" % ([c.shape for c in cols], lead))
    return numpy.ascontiguousarray(numpy.stack([c.reshape(-1) for c in cols], axis=1))


def wave_filter(rows, amplitude=(0.0, numpy.inf), length=(0.0, numpy.inf), out_dtype=None, device=0):
    """Feature-based filtering on single waves: every row of rows[..., n] with the samples of the half waves (single_waves) whose
    amplitude A = |value| or whose length lies outside the closed intervals amplitude = (lo, hi), length = (lo, hi) set to +0.0,
    all others copied.  Each bound is a scalar or an array that broadcasts to the leading axes of rows: every row — every level of
    a decomposition, with its own time-scale — may have its own.  The default bounds copy the rows bit for bit.

    rows as for single_waves; out_dtype: None / float64, or float32 (numpy or torch): each kept sample rounded once on the GPU.
    Returns an array (tensor for a tensor) shaped like rows.  Raises ITDError (non-finite) naming the rows that hold a NaN."""
    odt = _out_dtype(out_dtype)
    place, idt, shape, n, R, stride = rows_of(rows, "the wave filter", device)
    bounds = _wave_bounds(amplitude, length, shape[:-1])
    bstride = 0 if bounds.ndim == 1 else 4
    with place as S:
        out, info, d_b = S.empty(shape, odt), S.empty(R, numpy.int32), S.put(bounds)
        eng = _engine_for(3, S.dev)
        S.run(eng.wave_filter_batch_dev, S.x, idt, n, R, stride, S.ptr(d_b), bstride, S.ptr(out), n, odt == numpy.float32, S.ptr(info))
        _refuse_nan(S.host(info))
        return S.result(out)


# ---- the joint amplitude-length histogram of the half waves (itd_wave_hist_batch_*) ------------------------------------------
WaveHistogram = namedtuple("WaveHistogram", "count samples outside")
MAX_WAVE_BINS = 64          # per axis
MAX_WAVE_CELLS = 1024       # amplitude bins * length bins
_WAVE_TILE = 512


def _hist_edges(edges, name, lead):
    """One axis's edges as float64 [N + 1] (one set for every row) or [R, N + 1]; refuses NaN and edges that do not increase."""
    if _is_torch(edges):
        edges = edges.detach().cpu().numpy()
    e = numpy.asarray(edges, dtype=numpy.float64)
    if e.ndim < 1 or not 2 <= e.shape[-1] <= MAX_WAVE_BINS + 1:
        raise ValueError("%s: 2 to %d edges along the last axis, got shape %s" % (name, MAX_WAVE_BINS + 1, e.shape))
    if numpy.isnan(e).any():
        raise ValueError("%s: a NaN edge" % name)
    if not (e[..., 1:] > e[..., :-1]).all():
        raise ValueError("%s must be strictly increasing" % name)
    if e.ndim == 1:
        return numpy.ascontiguousarray(e)
    try:
        e = numpy.broadcast_to(e, lead + e.shape[-1:])
    except ValueError:
        raise ValueError("%s (shape %s) do not broadcast to the leading axes %s of rows" % (name, e.shape, lead))
    return numpy.ascontiguousarray(e).reshape(-1, e.shape[-1])


def _hist_hop(hop, n):
    if hop is None:
        return -(-n // _WAVE_TILE) * _WAVE_TILE
    if isinstance(hop, bool) or int(hop) != hop or hop < _WAVE_TILE or hop % _WAVE_TILE != 0:
        raise ValueError("hop: None or a positive multiple of %d, got %r" % (_WAVE_TILE, hop))
    return int(hop)


def wave_histogram(rows, amplitude_edges, length_edges, hop=None, device=0):
    """The joint amplitude-length histogram of the half waves (single_waves) of every row of rows[..., n] in one asynchronous call,
    without their table: the picture from which wave_filter's bounds are chosen.  Half wave k falls into amplitude bin i where
    amplitude_edges[i] <= A_k < amplitude_edges[i+1], length bin j where length_edges[j] <= length_k < length_edges[j+1] and time
    bin t = peak_k // hop of T = ceil(n / hop).  Returns WaveHistogram(count[..., T, Na, Nl], samples[..., T, Na, Nl],
    outside[..., T]), all int32: the half waves of a cell, the samples they hold, and the half waves of a time bin that lie in no
    cell.  count.sum() + outside.sum() is the row's number of half waves.  Every update is an integer add: the same bits from run
    to run and in any batch position.

    rows as for single_waves.  Each edge argument is a 1-D array (one set for every row) or an array whose leading axes broadcast to
    the leading axes of rows — every level of a decomposition, with its own time-scale, may have its own; 1 to 64 bins per axis, at
    most 1024 cells, strictly increasing, -inf / +inf allowed at the ends.  hop: None (one time bin) or a positive multiple of 512.
    Raises ValueError for bad edges or hop, ITDError (non-finite) naming the rows that hold a NaN."""
    place, idt, shape, n, R, stride = rows_of(rows, "the wave histogram", device)
    lead = shape[:-1]
    ae, le = _hist_edges(amplitude_edges, "amplitude_edges", lead), _hist_edges(length_edges, "length_edges", lead)
    Na, Nl = ae.shape[-1] - 1, le.shape[-1] - 1
    if Na * Nl > MAX_WAVE_CELLS:
        raise ValueError("%d x %d bins are more than %d cells" % (Na, Nl, MAX_WAVE_CELLS))
    hop = _hist_hop(hop, n)
    T = -(-n // hop)
    astride, lstride = (0 if ae.ndim == 1 else Na + 1), (0 if le.ndim == 1 else Nl + 1)
    with place as S:
        count, samples = S.empty(lead + (T, Na, Nl), numpy.int32), S.empty(lead + (T, Na, Nl), numpy.int32)
        outside, info = S.empty(lead + (T,), numpy.int32), S.empty(R, numpy.int32)
        d_a, d_l = S.put(ae), S.put(le)
        eng = _engine_for(3, S.dev)
        S.run(eng.wave_hist_batch_dev, S.x, idt, n, R, stride, S.ptr(d_a), astride, Na, S.ptr(d_l), lstride, Nl, hop, S.ptr(count),
              S.ptr(samples), T * Na * Nl, S.ptr(outside), S.ptr(info))
        _refuse_nan(S.host(info))
        return WaveHistogram(S.result(count), S.result(samples), S.result(outside))


# ---- the wave filter's bounds from the histogram's quantiles (itd_wave_bounds_batch) -----------------------------------------
def _bounds_params(amplitude_q, length_q, amplitude_scale, length_scale, lead):
    """The eight parameters (aq_lo, aq_hi, lq_lo, lq_hi, as_lo, as_hi, ls_lo, ls_hi) as float64 [8] (one set for every row) or
    [R, 8]; refuses NaN, quantiles outside [0, 1] and lo > hi."""
    cols = []
    for name, pair, quantile in (("amplitude_q", amplitude_q, True), ("length_q", length_q, True),
                                 ("amplitude_scale", amplitude_scale, False), ("length_scale", length_scale, False)):
        try:
            lo, hi = pair
        except (TypeError, ValueError):
            raise ValueError("%s: a pair (lo, hi), got %r" % (name, pair))
        lo, hi = numpy.asarray(lo, dtype=numpy.float64), numpy.asarray(hi, dtype=numpy.float64)
        if numpy.isnan(lo).any() or numpy.isnan(hi).any():
            raise ValueError("%s: a NaN" % name)
        if quantile:
            if (lo < 0).any() or (lo > 1).any() or (hi < 0).any() or (hi > 1).any():
                raise ValueError("%s: quantiles lie in [0, 1]" % name)
            try:
                both = numpy.broadcast_arrays(lo, hi)
            except ValueError:
                raise ValueError("%s: lo %s and hi %s do not broadcast" % (name, lo.shape, hi.shape))
            if (both[0] > both[1]).any():
                raise ValueError("%s: lo > hi" % name)
        cols += [lo, hi]
    if all(c.ndim == 0 for c in cols):
        return numpy.array([float(c) for c in cols])
    try:
        cols = [numpy.broadcast_to(c, lead) for c in cols]
    except ValueError:
        raise ValueError("the parameters (shapes %s) do not broadcast to the leading axes %s of hist" % ([c.shape for c in cols], lead))
    return numpy.ascontiguousarray(numpy.stack([c.reshape(-1) for c in cols], axis=1))


def _bounds_hist(hist, device):
    """The acceptance of hist[..., T, Na, Nl], int32 — a numpy array (made contiguous) or a torch CUDA tensor (used in place; its last
    three axes dense, its leading axes collapsing to one stride) — before anything is allocated: (the placement to open, shape, row
    count, row stride)."""
    torch_in = _is_torch(hist)
    a = hist if torch_in else numpy.asarray(hist)
    if str(a.dtype).split(".")[-1] != "int32":
        raise ValueError("hist must be int32, got %s" % (a.dtype,))
    shape = tuple(a.shape)
    if len(shape) < 3 or min(shape[-3:]) < 1:
        raise ValueError("expected hist[..., T, Na, Nl], got shape %s" % (shape,))
    T, Na, Nl = shape[-3:]
    if Na > MAX_WAVE_BINS or Nl > MAX_WAVE_BINS or Na * Nl > MAX_WAVE_CELLS:
        raise ValueError("%d x %d bins: at most %d per axis and %d cells" % (Na, Nl, MAX_WAVE_BINS, MAX_WAVE_CELLS))
    if T >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 time bins")
    R = int(numpy.prod(shape[:-3], dtype=numpy.int64))
    if R < 1:
        raise ValueError("no rows in a histogram of shape %s" % (shape,))
    slot = T * Na * Nl
    if not torch_in:
        return Numpy(device, numpy.ascontiguousarray(a).reshape(R, slot)), shape, R, slot
    if not a.is_cuda:
        raise ValueError("expected a CUDA tensor")
    strides = tuple(a.stride())
    dense = all(d == 1 or st == want for d, st, want in zip(shape[-3:], strides[-3:], (Na * Nl, Nl, 1)))
    stride = _row_stride(shape[:-3] + (slot,), strides[:-3] + (1,)) if dense else None
    if stride is None:
        raise ValueError("a tensor with strides %s: its last three axes must be dense and its leading axes collapse to one stride" % (strides,))
    return Tensor(a), shape, R, stride


def wave_filter_bounds(hist, amplitude_edges, length_edges, amplitude_q=(0.0, 1.0), length_q=(0.0, 1.0), amplitude_scale=(1.0, 1.0),
                       length_scale=(1.0, 1.0), time_bins=None, want_total=False, device=0):
    """wave_filter's bounds chosen on the device from the quantiles of a histogram hist[..., T, Na, Nl] (int32; `count` or `samples`
    of wave_histogram or of a WaveHistogramStream's slices), in one asynchronous call.  Per row and axis, with the marginal m over
    the time bins time_bins = (t0, t1) (None: all) and the other axis, its inclusive prefix sums cum and its total N: iL is the
    first bin with cum > q_lo N (q_lo = 1: the last non-empty bin), iU the first bin at or behind iL with cum >= q_hi N; the bounds
    are edges[iL] * scale_lo and edges[iU + 1] * scale_hi.  The bins iL .. iU hold at least (q_hi - q_lo) N; an empty histogram
    gives the whole edge range.  The filter's intervals are closed, so a half wave exactly on the upper edge is kept as well.  All
    sums are integers: the same bits from run to run and in any batch position.

    hist: a numpy array or a torch CUDA tensor.  Each edge argument as wave_histogram takes it; every parameter pair (lo, hi) holds
    scalars or arrays that broadcast to the leading axes of hist.  Returns float64 [..., 4] = (amp_lo, amp_hi, len_lo, len_hi) per
    row (a tensor for a tensor) — what WaveFilterStream.push takes as bounds=, Engine.wave_filter_batch_dev and the streams' push_dev
    by pointer where it lies, and wave_filter column by column: amplitude=(b[..., 0], b[..., 1]), length=(b[..., 2], b[..., 3]) —;
    with want_total also N, int64 [...].
    Raises ValueError for a quantile outside [0, 1], lo > hi, a NaN, bad edges or a bad range of time bins."""
    place, shape, R, stride = _bounds_hist(hist, device)
    lead, (T, Na, Nl) = shape[:-3], shape[-3:]
    ae, le = _hist_edges(amplitude_edges, "amplitude_edges", lead), _hist_edges(length_edges, "length_edges", lead)
    if ae.shape[-1] != Na + 1 or le.shape[-1] != Nl + 1:
        raise ValueError("hist has %d x %d bins, the edges are %d and %d" % (Na, Nl, ae.shape[-1], le.shape[-1]))
    q = _bounds_params(amplitude_q, length_q, amplitude_scale, length_scale, lead)
    try:
        t0, t1 = (0, T) if time_bins is None else time_bins
        ok = int(t0) == t0 and int(t1) == t1 and 0 <= t0 < t1 <= T
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("time_bins: None or (t0, t1) with 0 <= t0 < t1 <= %d, got %r" % (T, time_bins))
    astride, lstride, qstride = (0 if ae.ndim == 1 else Na + 1), (0 if le.ndim == 1 else Nl + 1), (0 if q.ndim == 1 else 8)
    with place as S:
        bounds, total = S.empty((R, 4), numpy.float64), S.empty((R,), numpy.int64) if want_total else None
        d_a, d_l, d_q = S.put(ae), S.put(le), S.put(q)
        S.run(_wave_bounds_for(S.dev).batch_dev, S.x, R, stride, T, int(t0), int(t1), Na, Nl, S.ptr(d_a), astride, S.ptr(d_l), lstride, S.ptr(d_q),
              qstride, S.ptr(bounds), 4, S.ptr(total))
        b = S.result(bounds).reshape(lead + (4,))
        return (b, S.result(total).reshape(lead)) if want_total else b
