"""Where one call's arrays live.  A many-row call is written once against a placement: Numpy stages through hipMalloc'd buffers
of the C ABI (engine.DeviceBuffer; torch is not needed) and frees them when its block is left, Tensor lets torch allocate on the
input tensor's device and hands the tensors themselves back.  Both answer

    empty(shape, dtype), full(shape, dtype, value), put(host_array)   -> a handle (an output: in the shape the caller receives)
    ptr(handle)                  the device address the engine is given (None stays None: an output that was not asked for)
    run(entry, *arguments)       the engine call
    host(handle)                 a numpy copy that waits for the device first: info words, counts
    result(handle, host=None)    what the caller receives: a fresh array (host: the copy the body already took), or the tensor
    dev, x                       the device index; inside the block, the address of the input rows

rows_of() is the acceptance of rows[..., n] and opens the placement that fits them.
"""
import contextlib
import math

import numpy

from .engine import DeviceBuffer


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _np_dtype(dtype):
    """torch.float32 / torch.float64 as numpy's; everything else as given."""
    if _is_torch(dtype):
        return {"torch.float32": numpy.float32, "torch.float64": numpy.float64}.get(str(dtype), str(dtype))
    return dtype


class Numpy(contextlib.ExitStack):
    """The device buffers of one numpy-staged call, freed when the block is left; rows (optional): the input, uploaded on entry."""

    def __init__(self, device, rows=None):
        super().__init__()
        self.dev, self._rows, self.x = int(device), rows, None

    def __enter__(self):
        super().__enter__()
        if self._rows is not None:
            try:
                self.x = self.put(self._rows).ptr
            except BaseException:
                self.close()
                raise
        return self

    def empty(self, shape, dtype):
        count = shape if isinstance(shape, int) else math.prod(shape)      # (numpy.prod costs microseconds per buffer)
        b = DeviceBuffer(count * numpy.dtype(dtype).itemsize, self.dev)
        self.callback(b.free)
        b.shape, b.dtype = shape, dtype
        return b

    def full(self, shape, dtype, value):
        return self.put(numpy.full(shape, value, dtype))

    def put(self, array):
        b = self.empty(array.shape, array.dtype)
        b.upload(array)
        return b

    def ptr(self, b):
        return None if b is None else b.ptr

    def run(self, entry, *args, **kw):
        entry(*args, **kw)

    def settled(self):
        pass

    def host(self, b):
        return b.download(numpy.empty(b.shape, b.dtype))       # itd_dev_copy synchronises

    def result(self, b, host=None):
        return self.host(b) if host is None else host


_TORCH_DTYPES = {}      # numpy dtype -> torch's, filled by the first Tensor (dtype.name is a Python property: microseconds per use)


class Tensor:
    """The tensors of one call on t's device.  The engine runs on its own stream: the device is synchronised before an engine call
    that follows work of torch's (the input's producer, a fill, an upload) and before anything of a running call is read or handed
    back, and at no other time."""

    def __init__(self, t):
        import torch
        self._torch, self._t, self.dev, self.x = torch, t, t.device.index, None
        self._torch_busy, self._running = True, False
        if not _TORCH_DTYPES:
            _TORCH_DTYPES.update({numpy.dtype(name): getattr(torch, name) for name in ("float32", "float64", "int32", "int64")})

    def __enter__(self):
        self.x = self._t.data_ptr()
        return self

    def __exit__(self, *exc):
        return False

    def empty(self, shape, dtype):
        return self._torch.empty(shape, dtype=_TORCH_DTYPES[numpy.dtype(dtype)], device=self._t.device)

    def full(self, shape, dtype, value):
        self._torch_busy = True
        return self._torch.full(shape, value, dtype=_TORCH_DTYPES[numpy.dtype(dtype)], device=self._t.device)

    def put(self, array):
        self._torch_busy = True
        return self._torch.from_numpy(array).to(self._t.device)

    def ptr(self, t):
        return None if t is None else t.data_ptr()

    def run(self, entry, *args, **kw):
        if self._torch_busy:
            self._torch.cuda.synchronize(self._t.device)
            self._torch_busy = False
        entry(*args, **kw)
        self._running = True

    def settled(self):
        """The caller has waited for the engine's stream by other means (Engine.summary)."""
        self._running = False

    def _wait(self):
        if self._running:
            self._torch.cuda.synchronize(self._t.device)
            self._running = False

    def host(self, t):
        self._wait()
        return t.cpu().numpy()

    def result(self, t, host=None):
        self._wait()
        return t


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


def rows_of(rows, what, device):
    """The acceptance of rows[..., n], float32 or float64 — a numpy array (made contiguous) or a torch CUDA tensor (used in place on
    its own device, `device` ignored; its leading axes must collapse to one row stride, its last axis must be dense) —, before
    anything is allocated: (the placement to open, input dtype, shape, n, row count, row stride)."""
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
    n, R = shape[-1], int(numpy.prod(shape[:-1], dtype=numpy.int64))
    if R < 1:
        raise ValueError("no rows in an array of shape %s" % (shape,))
    if not torch_in:
        return Numpy(device, numpy.ascontiguousarray(a).reshape(R, n)), idt, shape, n, R, n
    if not a.is_cuda:
        raise ValueError("expected a CUDA tensor")
    stride = _row_stride(shape, tuple(a.stride()))
    if stride is None:
        raise ValueError("the leading axes of a tensor with strides %s do not collapse to one row stride" % (tuple(a.stride()),))
    return Tensor(a), idt, shape, n, R, stride
