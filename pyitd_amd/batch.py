"""Row-wise / channel-wise forms of the single-level operators (numpy in -> numpy out) over the asynchronous batched entry
points of the C ABI (itd_baseline_extract_batch_f64, itd_detect_batch_f64, itd_baseline_extract_cubic_batch_f64), and the
instantaneous amplitude / phase / frequency of many rows (itd_instantaneous_batch_*; numpy or torch CUDA tensors) and their
single-wave analysis: the table of half waves, the feature filter and the half waves' joint amplitude-length histogram
(itd_waves_batch_*, itd_wave_filter_batch_*, itd_wave_hist_batch_*).

The reference applies its operators row by row under numba.prange (siftED2D.ipynb cell 1) and re-uses retained extrema along
channels (itd.cpp:40-44); here a whole batch is one launch sequence and no knot count crosses PCIe in between.  Device
memory comes from the C ABI's own allocator (engine.DeviceBuffer): no torch needed.
"""
import contextlib
from collections import namedtuple

import numpy

from ._lib import ITDError
from .engine import DETECT_KNOTS, ITD_ERR_NONFINITE, DeviceBuffer
from .itd import _engine_for, _is_torch, _np_dtype


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
    d_x, d_rot, d_base, d_info = (DeviceBuffer(x.nbytes, device), DeviceBuffer(x.nbytes, device), DeviceBuffer(x.nbytes, device),
                                  DeviceBuffer(4 * B, device))
    try:
        d_x.upload(x)
        eng.extract_batch_dev(d_x.ptr, n, B, n, d_rot.ptr, n, d_base.ptr, n, d_info.ptr)
        info = d_info.download(numpy.empty(B, numpy.int32))      # itd_dev_copy synchronises
        rot, base = d_rot.download(numpy.empty_like(x)), d_base.download(numpy.empty_like(x))
    finally:
        for b in (d_x, d_rot, d_base, d_info):
            b.free()
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
    d_x, d_info = DeviceBuffer(x.nbytes, device), DeviceBuffer(4 * B, device)
    try:
        d_x.upload(x)
        eng.detect_batch_dev(d_x.ptr, n, B, n, mode, None, 0, d_info.ptr)
        info = d_info.download(numpy.empty(B, numpy.int32))
    finally:
        d_x.free()
        d_info.free()
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
    d_x, d_idx, d_info = DeviceBuffer(x.nbytes, device), DeviceBuffer(4 * B * stride, device), DeviceBuffer(4 * B, device)
    try:
        d_x.upload(x)
        eng.detect_batch_dev(d_x.ptr, n, B, n, mode, d_idx.ptr, stride, d_info.ptr)
        info = d_info.download(numpy.empty(B, numpy.int32))
        idx = d_idx.download(numpy.empty((B, stride), numpy.int32))
    finally:
        for b in (d_x, d_idx, d_info):
            b.free()
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
    d_x, d_base, d_info = DeviceBuffer(x.nbytes, device), DeviceBuffer(x.nbytes, device), DeviceBuffer(4 * C, device)
    d_e = None
    try:
        d_x.upload(x)
        d_base.upload(numpy.zeros_like(x))
        if extrema_input is not None:
            e = numpy.ascontiguousarray(extrema_input, dtype=numpy.int64)
            if e.shape[0] < idx + 1:
                raise ValueError("extrema_input needs idx+1 entries")
            if e[: idx + 1].min() < 0 or e[: idx + 1].max() >= n:
                raise IndexError("extrema outside the signal")      # what the reference's indexing would raise
            e32 = e[: idx + 1].astype(numpy.int32)
            d_e = DeviceBuffer(e32.nbytes, device)
            d_e.upload(e32)
            eng.cubic_batch_dev(d_x.ptr, n, C, n, d_e.ptr, 0, int(idx), d_base.ptr, n, d_info.ptr)
        else:
            eng.cubic_batch_dev(d_x.ptr, n, C, n, None, 0, 0, d_base.ptr, n, d_info.ptr)
        info = d_info.download(numpy.empty(C, numpy.int32))
        if (info == -1).any():
            raise ValueError("extrema_input must be strictly increasing")
        if (info == -2).any():
            raise ValueError("NaN in the signal (the cubic operator has no NaN branch)")
        return d_base.download(numpy.empty_like(x))
    finally:
        for b in (d_x, d_base, d_info, d_e):
            if b is not None:
                b.free()


_INSTANTANEOUS = ("amplitude", "phase", "frequency")


def _row_stride(shape, strides):
    """The one stride (in elements) between consecutive rows of an array [..., n] whose last axis is dense, or None if its
    leading axes do not collapse to one."""
    if strides[-1] != 1:
        return None
    lead = [(d, st) for d, st in zip(shape[:-1], strides[:-1]) if d > 1]
    if not lead:
        return shape[-1]
    for (_, outer), (d, inner) in zip(lead[:-1], lead[1:]):
        if outer != d * inner:
            return None
    return lead[-1][1] if lead[-1][1] >= shape[-1] else None


def _accept_rows(rows, what):
    """The acceptance of rows[..., n]: (torch?, the array or tensor, input dtype, shape, n, row count)."""
    torch_in = _is_torch(rows)
    a = rows if torch_in else numpy.asarray(rows)
    idt = numpy.dtype(_np_dtype(a.dtype))
    if idt not in (numpy.dtype(numpy.float32), numpy.dtype(numpy.float64)):
        raise ValueError("rows must be float32 or float64, got %s" % (a.dtype,))
    shape = tuple(a.shape)
    if len(shape) < 2:
        raise ValueError("expected rows[..., n] with at least one leading axis, got shape %s" % (shape,))
    if shape[-1] < 3:
        raise ValueError("%s needs at least 3 samples" % what)
    R = int(numpy.prod(shape[:-1], dtype=numpy.int64))
    if R < 1:
        raise ValueError("no rows in an array of shape %s" % (shape,))
    return torch_in, a, idt, shape, shape[-1], R


def _tensor_stride(a, shape):
    if not a.is_cuda:
        raise ValueError("expected a CUDA tensor")
    stride = _row_stride(shape, tuple(a.stride()))
    if stride is None:
        raise ValueError("the leading axes of a tensor with strides %s do not collapse to one row stride" % (tuple(a.stride()),))
    return stride


def _refuse_nan(info):
    bad = numpy.flatnonzero(info < 0)
    if bad.size:
        raise ITDError(ITD_ERR_NONFINITE, "NaN in rows %s%s" % (bad[:16].tolist(), " ..." if bad.size > 16 else ""))


def _out_dtype(out_dtype):
    odt = numpy.dtype(numpy.float64 if out_dtype is None else _np_dtype(out_dtype))
    if odt not in (numpy.dtype(numpy.float32), numpy.dtype(numpy.float64)):
        raise ValueError("out_dtype must be float32 or float64")
    return odt


class _Staged(contextlib.ExitStack):
    """The device buffers of one numpy-staged call (hipMalloc through the C ABI), freed when the block is left."""

    def __init__(self, device):
        super().__init__()
        self.dev = int(device)

    def empty(self, nbytes):
        b = DeviceBuffer(nbytes, self.dev)
        self.callback(b.free)
        return b

    def upload(self, array):
        b = self.empty(array.nbytes)
        b.upload(array)
        return b


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
    torch_in, a, idt, shape, n, R = _accept_rows(rows, "the instantaneous step")
    if torch_in:
        import torch
        stride = _tensor_stride(a, shape)
        dev = a.device.index
        tdt = torch.float32 if odt == numpy.float32 else torch.float64
        outs = {w: torch.empty(shape, dtype=tdt, device=a.device) for w in want}
        info = torch.empty(R, dtype=torch.int32, device=a.device)
        eng = _engine_for(3, dev)
        torch.cuda.synchronize(a.device)    # the engine runs on its own stream
        eng.instantaneous_batch_dev(a.data_ptr(), idt, n, R, stride, *[outs[w].data_ptr() if w in outs else None for w in _INSTANTANEOUS],
                                    n, odt == numpy.float32, info.data_ptr())
        torch.cuda.synchronize(a.device)
        _refuse_nan(info.cpu().numpy())
        return tuple(outs[w] for w in want)
    a = numpy.ascontiguousarray(a).reshape(R, n)
    with _Staged(device) as S:
        bufs = {w: S.empty(R * n * odt.itemsize) for w in want}
        d_x, d_info = S.upload(a), S.empty(4 * R)
        eng = _engine_for(3, S.dev)
        eng.instantaneous_batch_dev(d_x.ptr, idt, n, R, n, *[bufs[w].ptr if w in bufs else None for w in _INSTANTANEOUS],
                                    n, odt == numpy.float32, d_info.ptr)
        _refuse_nan(d_info.download(numpy.empty(R, numpy.int32)))      # itd_dev_copy synchronises
        return tuple(bufs[w].download(numpy.empty((R, n), odt)).reshape(shape) for w in want)


# ---- the time-frequency-energy spectrum (itd_tfe_spectrum_*) ---------------------------------------------------------------
Spectrum = namedtuple("Spectrum", "power outside")
_WEIGHTS = ("count", "amplitude", "energy")
MAX_BINS = 512


def _spectrum_args(edges, hop, weight):
    """The checked (edges float64 [F + 1], hop, weight code) of tfe_spectrum."""
    if _is_torch(edges):
        edges = edges.detach().cpu().numpy()
    e = numpy.ascontiguousarray(edges, dtype=numpy.float64)
    if e.ndim != 1 or not 2 <= e.size <= MAX_BINS + 1:
        raise ValueError("edges: a 1-D array of 2 to %d entries, got shape %s" % (MAX_BINS + 1, e.shape))
    if not numpy.isfinite(e).all() or not (e[1:] > e[:-1]).all():
        raise ValueError("edges must be finite and strictly increasing")
    if isinstance(hop, bool) or int(hop) != hop or hop < 64 or hop % 64 != 0 or (hop < 512 and hop not in (64, 128, 256)):
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
    torch_in, a, idt, shape, n, R = _accept_rows(rows, "the spectrum")
    F, T = e.size - 1, -(-n // hop)
    lead = shape[:-1]
    if torch_in:
        import torch
        stride = _tensor_stride(a, shape)
        dev = a.device.index
        power = torch.empty((R, T, F), dtype=torch.float64, device=a.device)
        outside = torch.empty((R, T), dtype=torch.int32, device=a.device)
        info = torch.empty(R, dtype=torch.int32, device=a.device)
        d_e = torch.from_numpy(e).to(a.device)
        eng = _engine_for(3, dev)
        torch.cuda.synchronize(a.device)    # the engine runs on its own stream
        eng.tfe_spectrum_dev(a.data_ptr(), idt, n, R, stride, d_e.data_ptr(), F, hop, wcode, power.data_ptr(), T * F, outside.data_ptr(),
                             info.data_ptr())
        torch.cuda.synchronize(a.device)
        _refuse_nan(info.cpu().numpy())
        return Spectrum(power.reshape(lead + (T, F)), outside.reshape(lead + (T,)))
    a = numpy.ascontiguousarray(a).reshape(R, n)
    with _Staged(device) as S:
        d_x, d_e, d_p, d_o, d_info = S.upload(a), S.upload(e), S.empty(8 * R * T * F), S.empty(4 * R * T), S.empty(4 * R)
        eng = _engine_for(3, S.dev)
        eng.tfe_spectrum_dev(d_x.ptr, idt, n, R, n, d_e.ptr, F, hop, wcode, d_p.ptr, T * F, d_o.ptr, d_info.ptr)
        _refuse_nan(d_info.download(numpy.empty(R, numpy.int32)))          # itd_dev_copy synchronises
        return Spectrum(d_p.download(numpy.empty((R, T, F))).reshape(lead + (T, F)),
                        d_o.download(numpy.empty((R, T), numpy.int32)).reshape(lead + (T,)))


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
    torch_in, a, idt, shape, n, R = _accept_rows(rows, "single-wave analysis")
    lead = shape[:-1]
    if torch_in:
        import torch
        stride = _tensor_stride(a, shape)
        dev = a.device.index
        count = torch.empty(R, dtype=torch.int32, device=a.device)
        info = torch.empty(R, dtype=torch.int32, device=a.device)
        eng = _engine_for(3, dev)
        torch.cuda.synchronize(a.device)    # the engine runs on its own stream
        if cap is None:
            eng.waves_batch_dev(a.data_ptr(), idt, n, R, stride, None, None, None, None, 0, 0, count.data_ptr(), info.data_ptr())
            torch.cuda.synchronize(a.device)
            _refuse_nan(info.cpu().numpy())
            cap = int(count.max())
        ints = [torch.full((R, cap), -1, dtype=torch.int32, device=a.device) for _ in range(3)]
        value = torch.full((R, cap), float("nan"), dtype=torch.float64, device=a.device)
        torch.cuda.synchronize(a.device)
        eng.waves_batch_dev(a.data_ptr(), idt, n, R, stride, *[t.data_ptr() for t in ints], value.data_ptr(), cap, cap,
                            count.data_ptr(), info.data_ptr())
        torch.cuda.synchronize(a.device)
        _refuse_nan(info.cpu().numpy())
        _refuse_overflow(count.cpu().numpy(), cap)
        return Waves(count.reshape(lead), *[t.reshape(lead + (cap,)) for t in ints], value.reshape(lead + (cap,)))
    a = numpy.ascontiguousarray(a).reshape(R, n)
    with _Staged(device) as S:
        d_x, d_count, d_info = S.upload(a), S.empty(4 * R), S.empty(4 * R)
        eng = _engine_for(3, S.dev)
        if cap is None:
            eng.waves_batch_dev(d_x.ptr, idt, n, R, n, None, None, None, None, 0, 0, d_count.ptr, d_info.ptr)
            _refuse_nan(d_info.download(numpy.empty(R, numpy.int32)))       # itd_dev_copy synchronises
            cap = int(d_count.download(numpy.empty(R, numpy.int32)).max())
        fill_i, fill_v = numpy.full((R, cap), -1, numpy.int32), numpy.full((R, cap), numpy.nan)
        fills = (fill_i, fill_i, fill_i, fill_v)
        tabs = [S.upload(f) for f in fills]
        eng.waves_batch_dev(d_x.ptr, idt, n, R, n, *[b.ptr for b in tabs], cap, cap, d_count.ptr, d_info.ptr)
        _refuse_nan(d_info.download(numpy.empty(R, numpy.int32)))
        count = d_count.download(numpy.empty(R, numpy.int32))
        _refuse_overflow(count, cap)
        outs = [b.download(numpy.empty_like(f)).reshape(lead + (cap,)) for b, f in zip(tabs, fills)]
        return Waves(count.reshape(lead), *outs)


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
    torch_in, a, idt, shape, n, R = _accept_rows(rows, "the wave filter")
    bounds = _wave_bounds(amplitude, length, shape[:-1])
    bstride = 0 if bounds.ndim == 1 else 4
    if torch_in:
        import torch
        stride = _tensor_stride(a, shape)
        dev = a.device.index
        out = torch.empty(shape, dtype=torch.float32 if odt == numpy.float32 else torch.float64, device=a.device)
        info = torch.empty(R, dtype=torch.int32, device=a.device)
        d_b = torch.from_numpy(bounds).to(a.device)
        eng = _engine_for(3, dev)
        torch.cuda.synchronize(a.device)    # the engine runs on its own stream
        eng.wave_filter_batch_dev(a.data_ptr(), idt, n, R, stride, d_b.data_ptr(), bstride, out.data_ptr(), n, odt == numpy.float32,
                                  info.data_ptr())
        torch.cuda.synchronize(a.device)
        _refuse_nan(info.cpu().numpy())
        return out
    a = numpy.ascontiguousarray(a).reshape(R, n)
    with _Staged(device) as S:
        d_x, d_b, d_out, d_info = S.upload(a), S.upload(bounds), S.empty(R * n * odt.itemsize), S.empty(4 * R)
        eng = _engine_for(3, S.dev)
        eng.wave_filter_batch_dev(d_x.ptr, idt, n, R, n, d_b.ptr, bstride, d_out.ptr, n, odt == numpy.float32, d_info.ptr)
        _refuse_nan(d_info.download(numpy.empty(R, numpy.int32)))           # itd_dev_copy synchronises
        return d_out.download(numpy.empty((R, n), odt)).reshape(shape)


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
    torch_in, a, idt, shape, n, R = _accept_rows(rows, "the wave histogram")
    lead = shape[:-1]
    ae, le = _hist_edges(amplitude_edges, "amplitude_edges", lead), _hist_edges(length_edges, "length_edges", lead)
    Na, Nl = ae.shape[-1] - 1, le.shape[-1] - 1
    if Na * Nl > MAX_WAVE_CELLS:
        raise ValueError("%d x %d bins are more than %d cells" % (Na, Nl, MAX_WAVE_CELLS))
    hop = _hist_hop(hop, n)
    T = -(-n // hop)
    astride, lstride = (0 if ae.ndim == 1 else Na + 1), (0 if le.ndim == 1 else Nl + 1)
    slot = T * Na * Nl
    if torch_in:
        import torch
        stride = _tensor_stride(a, shape)
        dev = a.device.index
        count, samples = (torch.empty((R, T, Na, Nl), dtype=torch.int32, device=a.device) for _ in range(2))
        outside = torch.empty((R, T), dtype=torch.int32, device=a.device)
        info = torch.empty(R, dtype=torch.int32, device=a.device)
        d_a, d_l = torch.from_numpy(ae).to(a.device), torch.from_numpy(le).to(a.device)
        eng = _engine_for(3, dev)
        torch.cuda.synchronize(a.device)    # the engine runs on its own stream
        eng.wave_hist_batch_dev(a.data_ptr(), idt, n, R, stride, d_a.data_ptr(), astride, Na, d_l.data_ptr(), lstride, Nl, hop,
                                count.data_ptr(), samples.data_ptr(), slot, outside.data_ptr(), info.data_ptr())
        torch.cuda.synchronize(a.device)
        _refuse_nan(info.cpu().numpy())
        return WaveHistogram(count.reshape(lead + (T, Na, Nl)), samples.reshape(lead + (T, Na, Nl)), outside.reshape(lead + (T,)))
    a = numpy.ascontiguousarray(a).reshape(R, n)
    with _Staged(device) as S:
        d_x, d_a, d_l = S.upload(a), S.upload(ae), S.upload(le)
        d_c, d_s, d_o, d_info = S.empty(4 * R * slot), S.empty(4 * R * slot), S.empty(4 * R * T), S.empty(4 * R)
        eng = _engine_for(3, S.dev)
        eng.wave_hist_batch_dev(d_x.ptr, idt, n, R, n, d_a.ptr, astride, Na, d_l.ptr, lstride, Nl, hop, d_c.ptr, d_s.ptr, slot, d_o.ptr,
                                d_info.ptr)
        _refuse_nan(d_info.download(numpy.empty(R, numpy.int32)))          # itd_dev_copy synchronises
        return WaveHistogram(*[b.download(numpy.empty((R, T, Na, Nl), numpy.int32)).reshape(lead + (T, Na, Nl)) for b in (d_c, d_s)],
                             d_o.download(numpy.empty((R, T), numpy.int32)).reshape(lead + (T,)))
