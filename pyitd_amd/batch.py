"""Row-wise / channel-wise forms of the single-level operators (numpy in -> numpy out) over the asynchronous batched entry
points of the C ABI (itd_baseline_extract_batch_f64, itd_detect_batch_f64, itd_baseline_extract_cubic_batch_f64), and the
instantaneous amplitude / phase / frequency of many rows (itd_instantaneous_batch_*; numpy or torch CUDA tensors).

The reference applies its operators row by row under numba.prange (siftED2D.ipynb cell 1) and re-uses retained extrema along
channels (itd.cpp:40-44); here a whole batch is one launch sequence and no knot count crosses PCIe in between.  Device
memory comes from the C ABI's own allocator (engine.DeviceBuffer): no torch needed.
"""
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
    odt = numpy.dtype(numpy.float64 if out_dtype is None else _np_dtype(out_dtype))
    if odt not in (numpy.dtype(numpy.float32), numpy.dtype(numpy.float64)):
        raise ValueError("out_dtype must be float32 or float64")
    torch_in = _is_torch(rows)
    a = rows if torch_in else numpy.asarray(rows)
    idt = numpy.dtype(_np_dtype(a.dtype))
    if idt not in (numpy.dtype(numpy.float32), numpy.dtype(numpy.float64)):
        raise ValueError("rows must be float32 or float64, got %s" % (a.dtype,))
    shape = tuple(a.shape)
    if len(shape) < 2:
        raise ValueError("expected rows[..., n] with at least one leading axis, got shape %s" % (shape,))
    n = shape[-1]
    if n < 3:
        raise ValueError("the instantaneous step needs at least 3 samples")
    R = int(numpy.prod(shape[:-1], dtype=numpy.int64))
    if R < 1:
        raise ValueError("no rows in an array of shape %s" % (shape,))

    def refuse(info):
        bad = numpy.flatnonzero(info < 0)
        if bad.size:
            raise ITDError(ITD_ERR_NONFINITE, "NaN in rows %s%s" % (bad[:16].tolist(), " ..." if bad.size > 16 else ""))

    if torch_in:
        import torch
        if not a.is_cuda:
            raise ValueError("expected a CUDA tensor")
        stride = _row_stride(shape, tuple(a.stride()))
        if stride is None:
            raise ValueError("the leading axes of a tensor with strides %s do not collapse to one row stride" % (tuple(a.stride()),))
        dev = a.device.index
        tdt = torch.float32 if odt == numpy.float32 else torch.float64
        outs = {w: torch.empty(shape, dtype=tdt, device=a.device) for w in want}
        info = torch.empty(R, dtype=torch.int32, device=a.device)
        eng = _engine_for(3, dev)
        torch.cuda.synchronize(a.device)    # the engine runs on its own stream
        eng.instantaneous_batch_dev(a.data_ptr(), idt, n, R, stride, *[outs[w].data_ptr() if w in outs else None for w in _INSTANTANEOUS],
                                    n, odt == numpy.float32, info.data_ptr())
        torch.cuda.synchronize(a.device)
        refuse(info.cpu().numpy())
        return tuple(outs[w] for w in want)
    a = numpy.ascontiguousarray(a).reshape(R, n)
    dev = int(device)
    bufs = {w: DeviceBuffer(R * n * odt.itemsize, dev) for w in want}
    d_x, d_info = DeviceBuffer(a.nbytes, dev), DeviceBuffer(4 * R, dev)
    try:
        d_x.upload(a)
        eng = _engine_for(3, dev)
        eng.instantaneous_batch_dev(d_x.ptr, idt, n, R, n, *[bufs[w].ptr if w in bufs else None for w in _INSTANTANEOUS],
                                    n, odt == numpy.float32, d_info.ptr)
        refuse(d_info.download(numpy.empty(R, numpy.int32)))       # itd_dev_copy synchronises
        return tuple(bufs[w].download(numpy.empty((R, n), odt)).reshape(shape) for w in want)
    finally:
        for b in list(bufs.values()) + [d_x, d_info]:
            b.free()
