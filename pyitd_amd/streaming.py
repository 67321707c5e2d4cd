"""Block-wise (streaming) operation for unbounded signals — host handle over itd_stream_* (include/pyitd_hip.h).

The reference gives the recipe in a comment only (itd.cpp:31-38): "use a circular buffer with modulous tracking to rotate
the samples / re-assess extrema in the entire buffer every iteration / use from the last extrema in the first buffer to the
first extrema in the last buffer / set the first and last baseline knots manually to said values / update the j array /
compute only the baseline[i] array for the inner third of the buffer overall / rotate buffers, rinse and repeat", and the
reuse of retained extrema along channels (itd.cpp:40-44).  Everything numeric runs on the GPU inside the library: the ring
of the last three blocks, the window's extrema, the knot selection and the operator (pyitd_amd/csrc/itd_stream.hpp,
itd_engine_batch.inc; the three fixed-latency streams: itd_ring_streams.inc); this module only hands blocks in and out.  The recipe's exact statement (window geometry, knot selection) is in include/pyitd_hip.h
and DESIGN.md section 7; the GPU tests hold these classes to an independent CPU statement of it.

    st = Stream(4096, kind="linear")             # tier-1 operator, ITD.py:79-121
    for block in blocks:
        out = st.push(block)                     # None for the first block, then (rotation, baseline) of the PREVIOUS block
    last = st.flush()

kind "cubic": itd_baseline_extract_fast (itd_fourier_decomposition.py:49-122) on the extrema from `margin` in front of the
emitted block to margin + 2 behind it (the recipe's literal choice is margin 1); blocks with fewer than 4 such extrema are
returned unchanged (itd.cpp:170-172).  `shared_knots`: channel 0's extrema serve every channel (itd.cpp:40-44).
A NaN: a block whose knot-giving window (the channel's own; channel 0's under `shared_knots`) holds one is returned unchanged
with rotation 0 — nothing is built on such a window; a channel that holds a NaN while channel 0's window is finite gets a
spline through the NaN (unspecified samples).  A NaN in ANY channel sets status() to 2 until reset(), and push / flush raise
ITDError (ITD_ERR_NONFINITE) from the first emitting call on.
kind "linear": itd_baseline_extract on the window — away from a couple of knots at the window's ends bit-identical to the
whole-signal operator, so a stream whose blocks hold a few knots each reproduces the whole-signal rows exactly.

LevelsStream: the full multi-level decomposition block by block.  WaveFilterStream: the single-wave feature filter
(pyitd_amd.wave_filter) block by block at a fixed latency — what takes a LevelsStream's rows and gives feature-filtered components,
entirely on the device.  SpectrumStream: the time-frequency-energy spectrum (pyitd_amd.tfe_spectrum) block by
block at a fixed latency — finished time slices of a live decomposition's spectrum.  InstantaneousStream: the
per-sample amplitude, phase, frequency and half-wave length themselves (pyitd_amd.instantaneous_batch) block by block at the same
latency.  WaveHistogramStream: the half waves' joint amplitude-length histogram (pyitd_amd.wave_histogram)
block by block at the wave filter's latency — the distribution a live filter's bounds follow.
WaveTableStream: the half-wave table itself (pyitd_amd.single_waves) block by block with no horizon and no latency — every half wave
leaves in the push in which its end becomes known; the open half wave is carried from push to push.
WaveBoundsStream: the wave filter's bounds from the quantiles of a sliding window over a WaveHistogramStream's slices, one launch per
push — what joins the histogram stream to a live WaveFilterStream on the device.
"""
import ctypes
from collections import namedtuple

import numpy

from . import _lib
from ._lib import ITDError

KINDS = {"cubic": 0, "linear": 1}


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


_NO_STREAM = object()


class _Handle:
    """Owns one itd_stream* of the library: what every kind of stream does with its handle."""

    _L = _h = None

    def _open(self, create, detail, *args):
        """self._h = the stream `create`(*args) makes; ITDError(status, detail) if it does not"""
        self._L = _lib.load()
        h = ctypes.c_void_p()
        rc = getattr(self._L, create)(ctypes.byref(h), *args)
        if rc:
            raise ITDError(rc, detail)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.itd_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise ITDError(rc, self._L.itd_stream_last_error(self._h).decode())

    def _call(self, name, *args, stream=_NO_STREAM):
        """One push or flush entry `name`(handle, *args, &emitted[, stream]): True if it emitted a block."""
        em = ctypes.c_int32(0)
        tail = (ctypes.byref(em),) if stream is _NO_STREAM else (ctypes.byref(em), stream)
        self._check(getattr(self._L, name)(self._h, *args, *tail))
        return bool(em.value)

    @property
    def blocks_held(self):
        return self._L.itd_stream_blocks(self._h)

    def reset(self):
        self._check(self._L.itd_stream_reset(self._h))

    def status(self):
        """Synchronises the device; 0, or 2 if some block of some channel pushed since the last reset held a NaN."""
        v = ctypes.c_int32(0)
        self._check(self._L.itd_stream_status(self._h, ctypes.byref(v)))
        return v.value

    def _block(self, samples, rows):
        """samples as float64 [rows, block], and whether they came without the row axis"""
        x = numpy.ascontiguousarray(samples, dtype=numpy.float64)
        flat = x.ndim == 1
        x2 = x.reshape(1, -1) if flat else x
        if x2.shape != (rows, self.block):
            raise ValueError("expected blocks of shape (%d, %d)" % (rows, self.block))
        return x2, flat


class Stream(_Handle):
    """One stream = `channels` channels in lock step, blocks of `block` samples."""

    def __init__(self, block, channels=1, kind="cubic", margin=8, shared_knots=False, device=0):
        if kind not in KINDS:
            raise ValueError("kind must be 'cubic' or 'linear'")
        if block < 8 or channels < 1 or (kind == "cubic" and margin < 1):
            raise ValueError("block >= 8 samples, channels >= 1, margin >= 1 extremum")
        if kind == "linear" and shared_knots:
            raise ValueError("the tier-1 operator's knots are the signal's own (ITD.py:87-98): shared_knots needs kind='cubic'")
        self._open("itd_stream_create", "itd_stream_create(block=%d, channels=%d, kind=%s)" % (block, channels, kind), int(device), int(block),
                   int(channels), KINDS[kind], int(margin), 1 if shared_knots else 0)
        self.block, self.channels, self.kind, self.margin, self.device = int(block), int(channels), kind, int(margin), int(device)

    # ---- device buffers (raw pointers; asynchronous on `stream`) ----------------------------------------------------
    def push_dev(self, block_ptr, in_stride, base_ptr, base_stride, rot_ptr=None, rot_stride=0, stream=None):
        """Store one block of every channel; True if the previous block's baseline (rotation) was written."""
        return self._call("itd_stream_push_f64", block_ptr, in_stride, base_ptr, base_stride, rot_ptr, rot_stride, stream=stream)

    def flush_dev(self, base_ptr, base_stride, rot_ptr=None, rot_stride=0, stream=None):
        return self._call("itd_stream_flush_f64", base_ptr, base_stride, rot_ptr, rot_stride, stream=stream)

    # ---- numpy in -> numpy out (one synchronisation per call) ----------------------------------------------------------
    def _shape_out(self, a, flat):
        return a[0] if flat else a

    def push(self, samples):
        """samples [channels, block] (or [block] for one channel).  Returns None for the first block; afterwards the PREVIOUS
        block's baseline (cubic) or (rotation, baseline) (linear), shaped like the input."""
        x2, flat = self._block(samples, self.channels)
        base = numpy.empty_like(x2)
        rot = numpy.empty_like(x2) if self.kind == "linear" else None
        if not self._call("itd_stream_push_host_f64", _np_ptr(x2), _np_ptr(base), _np_ptr(rot)):
            return None
        if self.kind == "linear":
            return self._shape_out(rot, flat), self._shape_out(base, flat)
        return self._shape_out(base, flat)

    def flush(self, flat=None):
        """The last block's result (it has no successor); None if the stream holds nothing."""
        base = numpy.empty((self.channels, self.block))
        rot = numpy.empty_like(base) if self.kind == "linear" else None
        if not self._call("itd_stream_flush_host_f64", _np_ptr(base), _np_ptr(rot)):
            return None
        flat = (self.channels == 1) if flat is None else flat
        if self.kind == "linear":
            return self._shape_out(rot, flat), self._shape_out(base, flat)
        return self._shape_out(base, flat)


class BlockwiseCubic(Stream):
    """One channel of the cubic recipe: push(block) -> baseline of the previous block."""

    def __init__(self, block, margin=8, device=0):
        super().__init__(block, 1, "cubic", margin, False, device)


class BlockwiseLinear(Stream):
    """One channel of the tier-1 operator: push(block) -> (rotation, baseline) of the previous block."""

    def __init__(self, block, device=0):
        super().__init__(block, 1, "linear", 1, False, device)


def _as_rows(x, block, two_d=False):
    """x as float64 [rows, n_blocks * block], and whether it came without the row axis"""
    x = numpy.asarray(x, dtype=numpy.float64)
    flat = x.ndim == 1
    x2 = x.reshape(1, -1) if flat else x
    if two_d and x2.ndim != 2:
        raise ValueError("rows: [R, n] or [n]")
    rows, n = x2.shape
    if n % block or n < block:
        raise ValueError("the length must be a multiple of the block")
    return x2, flat


def _push_then_drain(st, x2, args=None, **flush_kw):
    """Every block of x2 through st.push, then st.flush until it gives None; st is closed.  args(st): what push takes behind the
    block and flush in front of flush_kw.  Returns what the calls gave, in order."""
    outs = []
    try:
        a = args(st) if args else ()
        for k in range(x2.shape[1] // st.block):
            r = st.push(x2[:, k * st.block:(k + 1) * st.block], *a)
            if r is not None:
                outs.append(r)
        while (r := st.flush(*a, **flush_kw)) is not None:
            outs.append(r)
    finally:
        st.close()
    return outs


def blockwise(x, block, kind="cubic", margin=8, shared_knots=False, device=0):
    """Run a whole array x[channels, n_blocks * block] (or [n]) through a stream: what a caller with an unbounded source
    does block by block.  Returns baseline (cubic) or (rotation, baseline) (linear)."""
    x2, flat = _as_rows(x, block)
    outs = _push_then_drain(Stream(block, x2.shape[0], kind, margin, shared_knots, device), x2, flat=False)
    if kind == "linear":
        rot = numpy.concatenate([o[0] for o in outs], axis=1)
        base = numpy.concatenate([o[1] for o in outs], axis=1)
        return (rot[0], base[0]) if flat else (rot, base)
    base = numpy.concatenate(outs, axis=1)
    return base[0] if flat else base


class LevelsStream(_Handle):
    """The full multi-level ITD block by block (itd_levels_stream_* in include/pyitd_hip.h): a chain of levels + 1 tier-1
    stages, stage k >= 1 on the baselines of stage k-1; every step is ONE launch on the GPU for blocks up to 2730 samples, a launch
    sequence (bit-identical) for longer ones.

        st = LevelsStream(1024, levels=8)
        for block in blocks:
            out = st.push(block)         # None for the first levels + 1 pushes, then (rows[levels+1, block], exact)
        while (out := st.flush()) is not None: ...

    rows 0 .. M-1 of a block are its rotations of stages 0 .. M-1, row M stage M's rotation + baseline (ITD.py:418-426); block j
    leaves on push j + M + 1.  exact[c] = 1 certifies that the block's rows equal the whole-signal rows of
    ITD().itd(x, max_iteration=M-1) of the concatenated blocks, bit for bit (where that run does not stop naturally).  A window
    holding a NaN is never certified and sets status() bit 2."""

    def __init__(self, block, levels, channels=1, device=0):
        if block < 8 or 3 * block >= 2 ** 31 - 65536:
            raise ValueError("block must be at least 8 samples (and 3 blocks below 2^31)")
        if not 1 <= levels <= 21:
            raise ValueError("levels must be 1 .. 21")
        if not 1 <= channels <= 65535:
            raise ValueError("channels must be 1 .. 65535")
        self._open("itd_levels_stream_create", "itd_levels_stream_create(block=%d, channels=%d, levels=%d)" % (block, channels, levels),
                   int(device), int(block), int(channels), int(levels))
        self.block, self.levels, self.channels, self.device = int(block), int(levels), int(channels), int(device)

    @property
    def form(self):
        """'one-launch' (blocks up to 2730 samples) or 'sequence' (longer blocks, or forced)"""
        return "sequence" if self._L.itd_levels_stream_form(self._h) == 1 else "one-launch"

    def force_sequence(self, on=True):
        """Run every step as the launch sequence even where one launch would do (bit-identical; for comparing the forms)."""
        self._check(self._L.itd_levels_stream_set_sequence(self._h, 1 if on else 0))

    # ---- device buffers (raw pointers; asynchronous on `stream`) ----------------------------------------------------
    def push_dev(self, block_ptr, in_stride, rows_ptr, row_stride, chan_stride, exact_ptr=None, stream=None):
        """Store one block of every channel; True if a block's rows (and flags) were written."""
        return self._call("itd_levels_stream_push_f64", block_ptr, in_stride, rows_ptr, row_stride, chan_stride, exact_ptr, stream=stream)

    def flush_dev(self, rows_ptr, row_stride, chan_stride, exact_ptr=None, stream=None):
        return self._call("itd_levels_stream_flush_f64", rows_ptr, row_stride, chan_stride, exact_ptr, stream=stream)

    # ---- numpy in -> numpy out (one synchronisation per call) ----------------------------------------------------------
    def _out(self, rows, exact, flat):
        ex = exact.astype(bool)
        return (rows[0], ex[0]) if flat else (rows, ex)

    def push(self, samples):
        """samples [channels, block] (or [block] for one channel).  None, or (rows[channels, levels+1, block], exact[channels])
        with the channel axis dropped for 1-D input."""
        x2, flat = self._block(samples, self.channels)
        rows = numpy.empty((self.channels, self.levels + 1, self.block))
        exact = numpy.zeros(self.channels, dtype=numpy.uint8)
        em = self._call("itd_levels_stream_push_host_f64", _np_ptr(x2), _np_ptr(rows), _np_ptr(exact))
        return self._out(rows, exact, flat) if em else None

    def flush(self, flat=None):
        """The next block still held (one per call); None once the stream is empty."""
        rows = numpy.empty((self.channels, self.levels + 1, self.block))
        exact = numpy.zeros(self.channels, dtype=numpy.uint8)
        if not self._call("itd_levels_stream_flush_host_f64", _np_ptr(rows), _np_ptr(exact)):
            return None
        return self._out(rows, exact, self.channels == 1 if flat is None else flat)


def blockwise_itd(x, block, levels, device=0):
    """Run x[channels, n_blocks * block] (or [n]) through a LevelsStream.  Returns (rows[channels, levels+1, n],
    exact[channels, n_blocks]) (no channel axis for 1-D input)."""
    x2, flat = _as_rows(x, block)
    outs = _push_then_drain(LevelsStream(block, levels, x2.shape[0], device), x2, flat=False)
    rows = numpy.concatenate([o[0] for o in outs], axis=2)
    exact = numpy.stack([o[1] for o in outs], axis=1)
    return (rows[0], exact[0]) if flat else (rows, exact)


class _RingStream(_Handle):
    """What the four fixed-latency streams share (itd_<_NAME>_stream_* in include/pyitd_hip.h): `rows` rows in lock step, blocks of
    `block` samples, a horizon, D = latency blocks between a push and its block's results.  A kind gives its name, its validation of
    the block, the arguments of its device entries, and for the numpy form _outputs() (the arrays a call fills, None where one is not
    wanted) and _result(outs)."""

    _NAME = None

    @staticmethod
    def _check_rows_horizon(rows, horizon):
        if not 1 <= rows <= 65535:
            raise ValueError("rows must be 1 .. 65535")
        if not 1 <= horizon <= 2 ** 22:
            raise ValueError("horizon must be 1 .. 2^22 samples")

    def _create(self, block, rows, horizon, device, extra=(), detail=""):
        name = "itd_%s_stream_create" % self._NAME
        self._open(name, "%s(block=%d, rows=%d, horizon=%d%s)" % (name, block, rows, horizon, detail), int(device), int(block), int(rows),
                   int(horizon), *extra)
        self.block, self.rows, self.horizon, self.device = int(block), int(rows), int(horizon), int(device)
        self._flat = False          # the last push took a 1-D block: the blocks that leave have no row axis either

    @property
    def latency(self):
        """D: push p emits block p - D.  D = ceil(horizon / block) for the wave filter and the histogram, ceil((horizon + 1) / block)
        for the spectrum and the instantaneous stream."""
        return getattr(self._L, "itd_%s_stream_latency" % self._NAME)(self._h)

    # ---- device buffers (raw pointers; asynchronous on `stream`): the kinds' push_dev / flush_dev name their arguments ----------
    def _dev(self, step, args, stream):
        return self._call("itd_%s_stream_%s_f64" % (self._NAME, step), *args, stream=stream)

    # ---- numpy in -> numpy out (one synchronisation per call) ----------------------------------------------------------
    def _host(self, block, params=()):
        """One call of the host form: a push of `block` (what _block made of the caller's samples), or a flush step (None).
        params: what the entry takes between the block and the outputs.  The kind's result, or None if nothing was emitted."""
        step, head = "flush", ()
        if block is not None:
            x2, flat = block
            step, head = "push", (_np_ptr(x2),)
        outs = self._outputs()
        em = self._call("itd_%s_stream_%s_host_f64" % (self._NAME, step), *head, *params, *[_np_ptr(o) for o in outs])
        if block is not None:
            self._flat = flat
        return self._result(outs) if em else None


class WaveFilterStream(_RingStream):
    """The single-wave feature filter block by block at a fixed latency (itd_wave_stream_* in include/pyitd_hip.h): blocks of
    `rows` rows go in, the same blocks come out with the samples of the half waves outside the bounds set to +0.0 — bit for bit
    pyitd_amd.wave_filter of the concatenated rows with the upper length bound capped at `horizon`.  A half wave longer than
    `horizon` samples is never kept: that is the price of the bounded latency.  ONE launch per push on the GPU.

        st = WaveFilterStream(1024, rows=9, horizon=2048)
        st.latency                                      # D = ceil(horizon / block) = 2
        for block in blocks:                            # block: [rows, 1024]
            out = st.push(block, bounds)                # None for the first D pushes, then the filtered block p - D
        while (out := st.flush(bounds)) is not None: ...

    bounds: (amp_lo, amp_hi, len_lo, len_hi) as float64 [4] (one set for every row) or [rows, 4]; or amplitude=(lo, hi),
    length=(lo, hi) as wave_filter takes them.  A block is filtered with the bounds given when it is emitted.  A NaN in a pushed block
    sets status() bit 2 until reset(); that row's output is unspecified from then on.

    Samples in, feature-filtered components out, entirely on the device — a LevelsStream's rows pushed by pointer:

        lv = LevelsStream(1024, levels=4, channels=2)
        wf = WaveFilterStream(1024, rows=2 * 5, horizon=2048)
        # rows_d [2, 5, 1024], out_d [10, 1024], bounds_d [10, 4] float64 on the device, all on one stream `s`
        if lv.push_dev(block_ptr, 1024, rows_ptr, 1024, 5 * 1024, None, s):
            if wf.push_dev(rows_ptr, 1024, bounds_ptr, 4, out_ptr, 1024, s):
                ...                                     # out_d holds the filtered rows of the block pushed levels + 1 + D steps ago
    """

    _NAME = "wave"

    def __init__(self, block, rows=1, horizon=None, device=0):
        horizon = block if horizon is None else horizon
        if not 8 <= block <= 8192:
            raise ValueError("block must be 8 .. 8192 samples")
        self._check_rows_horizon(rows, horizon)
        self._create(block, rows, horizon, device)

    # ---- device buffers (raw pointers; asynchronous on `stream`) ----------------------------------------------------
    def push_dev(self, block_ptr, in_stride, bounds_ptr, bounds_stride, out_ptr, out_stride, stream=None):
        """Store one block of every row; True if a filtered block was written."""
        return self._dev("push", (block_ptr, in_stride, bounds_ptr, bounds_stride, out_ptr, out_stride), stream)

    def flush_dev(self, bounds_ptr, bounds_stride, out_ptr, out_stride, stream=None):
        return self._dev("flush", (bounds_ptr, bounds_stride, out_ptr, out_stride), stream)

    # ---- numpy in -> numpy out (one synchronisation per call) ----------------------------------------------------------
    def _bounds(self, bounds, amplitude, length):
        if bounds is None:
            from .batch import _wave_bounds
            inf = (0.0, numpy.inf)
            bounds = _wave_bounds(inf if amplitude is None else amplitude, inf if length is None else length, (self.rows,))
        elif amplitude is not None or length is not None:
            raise ValueError("give bounds or amplitude= / length=, not both")
        b = numpy.asarray(bounds, dtype=numpy.float64)
        if b.shape == (4,):
            b = numpy.broadcast_to(b, (self.rows, 4))
        if b.shape != (self.rows, 4):
            raise ValueError("bounds: [4] or [%d, 4], got %s" % (self.rows, b.shape))
        return numpy.ascontiguousarray(b)

    def push(self, samples, bounds=None, amplitude=None, length=None):
        """samples [rows, block] (or [block] for one row).  None for the first `latency` pushes, then the filtered block pushed
        `latency` pushes ago, shaped like the input."""
        block = self._block(samples, self.rows)
        b = self._bounds(bounds, amplitude, length)
        return self._host(block, (_np_ptr(b),))

    def flush(self, bounds=None, amplitude=None, length=None):
        """The next block still held (one per call), shaped like the blocks of the last push; None once the stream is empty."""
        b = self._bounds(bounds, amplitude, length)
        return self._host(None, (_np_ptr(b),))

    def _outputs(self):
        return (numpy.empty((self.rows, self.block)),)

    def _result(self, outs):
        return outs[0][0] if self._flat else outs[0]


def blockwise_wave_filter(rows, block, horizon, amplitude=(0.0, numpy.inf), length=(0.0, numpy.inf), device=0):
    """Run rows[R, n_blocks * block] (or [n]) through a WaveFilterStream: what a caller with an unbounded source does block by
    block.  Returns the filtered rows, shaped like the input: wave_filter(rows, amplitude, (length[0], min(length[1], horizon)))."""
    x2, flat = _as_rows(rows, block, two_d=True)
    outs = _push_then_drain(WaveFilterStream(block, x2.shape[0], horizon, device), x2, lambda st: (st._bounds(None, amplitude, length),))
    y = numpy.concatenate(outs, axis=1)
    return y[0] if flat else y


StreamSpectrum = namedtuple("StreamSpectrum", "power outside overlong")


class SpectrumStream(_RingStream):
    """The time-frequency-energy spectrum block by block at a fixed latency (itd_spectrum_stream_* in include/pyitd_hip.h): blocks
    of `rows` rows go in, finished time slices of their spectra come out — the cells pyitd_amd.tfe_spectrum gives for the
    concatenated rows, bit for bit, wherever no half wave is longer than `horizon` samples.  A sample whose half wave, or whose
    successor's half wave, is longer than that is OVERLONG (the stream's last sample, which has no successor: its predecessor's):
    it is counted outside (and in `overlong`) whatever its frequency would be — the price of the bounded latency.  ONE launch per
    push on the GPU.

        st = SpectrumStream(1024, rows=9, horizon=2048, edges=numpy.linspace(0.0, 0.5, 65), hop=256)
        st.latency                                      # D = ceil((horizon + 1) / block) = 3
        for block in blocks:                            # block: [rows, 1024]
            out = st.push(block)                        # None for the first D pushes, then block p - D's cells:
            ...                                         # out.power [rows, 4, 64], out.outside [rows, 4], out.overlong [rows, 4]
        while (out := st.flush()) is not None: ...

    block: a multiple of hop, 64 .. 4096; hop: what tfe_spectrum accepts (a multiple of 64; below 512 only 64, 128 or 256), by
    default the block where that is a legal hop.  edges: float64 [F + 1] (one set for every row) or [rows, F + 1], finite and
    strictly increasing, 1 <= F <= 512; push(samples, edges=...) replaces them from that push on.  weight: "count", "amplitude"
    or "energy".  A NaN in a pushed block sets status() bit 2 until reset(); that row is unspecified from then on.

    Samples in, a running waterfall of every component out, entirely on the device — a LevelsStream's rows pushed by pointer:

        lv = LevelsStream(1024, levels=3, channels=2)
        sp = SpectrumStream(1024, rows=2 * 4, horizon=2048, edges=edges, hop=256)
        # rows_d [2, 4, 1024] float64, edges_d [65] float64, power_d [8, 4, 64] float64, out_d / ovl_d [8, 4] int32: on the device,
        # everything on one stream `s`
        if lv.push_dev(block_ptr, 1024, rows_ptr, 1024, 4 * 1024, None, s):
            if sp.push_dev(rows_ptr, 1024, edges_ptr, 0, power_ptr, 4 * 64, out_ptr, ovl_ptr, 4, s):
                ...                                     # power_d holds the cells of the block pushed levels + 1 + D steps ago
    """

    _NAME = "spectrum"

    def __init__(self, block, rows=1, horizon=None, edges=None, hop=None, weight="energy", device=0):
        from .batch import _WEIGHTS, _legal_hop
        horizon = block if horizon is None else horizon
        if isinstance(block, bool) or int(block) != block or not 64 <= block <= 4096:
            raise ValueError("block must be 64 .. 4096 samples")
        if hop is None:
            if not _legal_hop(block):
                raise ValueError("hop must be given: a block of %d samples is no legal hop" % block)
            hop = block
        if not _legal_hop(hop) or block % hop:
            raise ValueError("hop: a positive multiple of 64 (below 512: 64, 128 or 256) that divides the block, got %r" % (hop,))
        self._check_rows_horizon(rows, horizon)
        if weight not in _WEIGHTS:
            raise ValueError("weight: one of %s, got %r" % (_WEIGHTS, weight))
        if edges is None:
            raise ValueError("edges: float64 [F + 1] or [rows, F + 1]")
        self.rows, self.hop, self.weight = int(rows), int(hop), weight
        self.cells = int(block) // self.hop
        self.bins = None
        self._edges = self._check_edges(edges)
        self.bins = self._edges.shape[-1] - 1
        self._create(block, rows, horizon, device, (self.hop, self.bins, _WEIGHTS.index(weight)), ", hop=%d, bins=%d" % (hop, self.bins))

    def _check_edges(self, edges):
        e = numpy.ascontiguousarray(edges, dtype=numpy.float64)
        if e.ndim not in (1, 2) or (e.ndim == 2 and e.shape[0] != self.rows) or not 2 <= e.shape[-1] <= 513:
            raise ValueError("edges: [F + 1] or [%d, F + 1] with 1 <= F <= 512, got shape %s" % (self.rows, e.shape))
        if self.bins is not None and e.shape[-1] != self.bins + 1:
            raise ValueError("edges: the stream has %d bins, got %d edges" % (self.bins, e.shape[-1]))
        if not numpy.isfinite(e).all() or not (e[..., 1:] > e[..., :-1]).all():
            raise ValueError("edges must be finite and strictly increasing")
        return e

    # ---- device buffers (raw pointers; asynchronous on `stream`) ----------------------------------------------------
    def push_dev(self, block_ptr, in_stride, edges_ptr, edges_stride, power_ptr, power_stride, outside_ptr=None, overlong_ptr=None,
                 count_stride=0, stream=None):
        """Store one block of every row; True if a block's cells were written."""
        return self._dev("push", (block_ptr, in_stride, edges_ptr, edges_stride, power_ptr, power_stride, outside_ptr, overlong_ptr,
                                  count_stride), stream)

    def flush_dev(self, edges_ptr, edges_stride, power_ptr, power_stride, outside_ptr=None, overlong_ptr=None, count_stride=0,
                  stream=None):
        return self._dev("flush", (edges_ptr, edges_stride, power_ptr, power_stride, outside_ptr, overlong_ptr, count_stride), stream)

    # ---- numpy in -> numpy out (one synchronisation per call) ----------------------------------------------------------
    def _outputs(self):
        return (numpy.empty((self.rows, self.cells, self.bins)), numpy.empty((self.rows, self.cells), numpy.int32),
                numpy.empty((self.rows, self.cells), numpy.int32))

    def _result(self, outs):
        return StreamSpectrum(*[o[0] for o in outs]) if self._flat else StreamSpectrum(*outs)

    def _edge_params(self, edges):
        if edges is not None:
            self._edges = self._check_edges(edges)
        e = self._edges
        return _np_ptr(e), e.shape[-1] if e.ndim == 2 else 0

    def push(self, samples, edges=None):
        """samples [rows, block] (or [block] for one row).  None for the first `latency` pushes, then StreamSpectrum(power[rows, C,
        F], outside[rows, C], overlong[rows, C]) of the block pushed `latency` pushes ago (no row axis for 1-D input)."""
        block = self._block(samples, self.rows)
        return self._host(block, self._edge_params(edges))

    def flush(self, edges=None):
        """The next block still held (one per call); None once the stream is empty."""
        return self._host(None, self._edge_params(edges))


StreamInstant = namedtuple("StreamInstant", "amplitude phase frequency length long overlong")
_INSTANT = ("amplitude", "phase", "frequency", "length")


def _check_want(want):
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in _INSTANT for w in want):
        raise ValueError("want: a non-empty subset of %s, got %r" % (_INSTANT, want))
    return want


class InstantaneousStream(_RingStream):
    """The instantaneous amplitude, phase and frequency and every sample's half-wave length block by block at a fixed latency
    (itd_inst_stream_* in include/pyitd_hip.h): blocks of `rows` rows go in, the same blocks' per-sample quantities come out —
    wherever a value is delivered, bit for bit what pyitd_amd.instantaneous_batch (and single_waves, for the length) gives for the
    concatenated rows.  A sample whose half wave is longer than `horizon` samples is LONG: its amplitude and phase are the NaN
    pattern 0x7FF8000000000000 and its length is 0.  A sample that is long or whose successor is (the stream's last sample: or whose
    predecessor is) is OVERLONG: its frequency is that NaN — a sample in front of a too-long half wave keeps its amplitude and
    phase and loses only its frequency.  That is the price of the bounded latency.  ONE launch per push on the GPU.

        st = InstantaneousStream(1024, rows=9, horizon=2048)
        st.latency                                      # D = ceil((horizon + 1) / block) = 3
        for block in blocks:                            # block: [rows, 1024]
            out = st.push(block)                        # None for the first D pushes, then block p - D's StreamInstant:
            ...                                         # out.amplitude, out.phase, out.frequency [rows, 1024]; out.long, out.overlong [rows]
        while (out := st.flush()) is not None: ...

    block: 8 .. 4096 samples, any value.  want: a non-empty subset of "amplitude", "phase", "frequency", "length"; a field that is
    not wanted is None and is not computed.  long / overlong: the block's counts of such samples per row (int32).  A NaN in a pushed
    block sets status() bit 2 until reset(); that row is unspecified from then on.

    Behind a LevelsStream on device pointers, everything on one stream `s`:

        lv = LevelsStream(1024, levels=3, channels=2)
        it = InstantaneousStream(1024, rows=2 * 4, horizon=2048)
        # rows_d [2, 4, 1024], amp_d / ph_d / fr_d [8, 1024] float64, len_d [8, 1024] and cnt_d [8, 2] int32: on the device
        if lv.push_dev(block_ptr, 1024, rows_ptr, 1024, 4 * 1024, None, s):
            if it.push_dev(rows_ptr, 1024, amp_ptr, ph_ptr, fr_ptr, len_ptr, 1024, cnt_ptr, 2, s):
                ...                                     # the block pushed levels + 1 + D steps ago; any per-sample rule on amplitude,
                                                        # frequency, phase and length is an elementwise operation on these
    """

    _NAME = "inst"

    def __init__(self, block, rows=1, horizon=None, want=("amplitude", "phase", "frequency"), device=0):
        horizon = block if horizon is None else horizon
        if isinstance(block, bool) or int(block) != block or not 8 <= block <= 4096:
            raise ValueError("block must be 8 .. 4096 samples")
        self._check_rows_horizon(rows, horizon)
        self.want = _check_want(want)
        self._create(block, rows, horizon, device)

    # ---- device buffers (raw pointers; asynchronous on `stream`) ----------------------------------------------------
    def push_dev(self, block_ptr, in_stride, amp_ptr, phase_ptr, freq_ptr, length_ptr, out_stride, counts_ptr=None, counts_stride=0,
                 stream=None):
        """Store one block of every row; True if a block's outputs were written (a None output is skipped)."""
        return self._dev("push", (block_ptr, in_stride, amp_ptr, phase_ptr, freq_ptr, length_ptr, out_stride, counts_ptr, counts_stride),
                         stream)

    def flush_dev(self, amp_ptr, phase_ptr, freq_ptr, length_ptr, out_stride, counts_ptr=None, counts_stride=0, stream=None):
        return self._dev("flush", (amp_ptr, phase_ptr, freq_ptr, length_ptr, out_stride, counts_ptr, counts_stride), stream)

    # ---- numpy in -> numpy out (one synchronisation per call) ----------------------------------------------------------
    def _outputs(self):
        shape = (self.rows, self.block)
        return [numpy.empty(shape, numpy.int32 if w == "length" else numpy.float64) if w in self.want else None for w in _INSTANT] + \
            [numpy.empty((self.rows, 2), numpy.int32)]

    def _result(self, outs):
        outs, counts = outs[:4], outs[4]
        if self._flat:
            return StreamInstant(*[None if o is None else o[0] for o in outs], counts[0, 0], counts[0, 1])
        return StreamInstant(*outs, counts[:, 0].copy(), counts[:, 1].copy())

    def push(self, samples):
        """samples [rows, block] (or [block] for one row).  None for the first `latency` pushes, then the StreamInstant of the block
        pushed `latency` pushes ago (no row axis for 1-D input)."""
        return self._host(self._block(samples, self.rows))

    def flush(self):
        """The next block still held (one per call); None once the stream is empty."""
        return self._host(None)


def blockwise_instantaneous(rows, block, horizon, want=("amplitude", "phase", "frequency"), device=0):
    """Run rows[R, n_blocks * block] (or [n]) through an InstantaneousStream: what a caller with an unbounded source does block by
    block.  Returns StreamInstant: the wanted arrays shaped like the input (the others None), long and overlong as int32
    [R, n_blocks] ([n_blocks] for 1-D input)."""
    x2, flat = _as_rows(rows, block, two_d=True)
    outs = _push_then_drain(InstantaneousStream(block, x2.shape[0], horizon, want, device), x2)
    fields = [None if outs[0][i] is None else numpy.concatenate([o[i] for o in outs], axis=1) for i in range(4)]
    fields += [numpy.stack([o[i] for o in outs], axis=1) for i in (4, 5)]
    return StreamInstant(*[None if f is None else (f[0] if flat else f) for f in fields])


StreamHistogram = namedtuple("StreamHistogram", "count samples outside overlong")
MAX_STREAM_HIST_CELLS = 8192          # cells per block: (block / hop) * amplitude bins * length bins
MAX_BOUNDS_WINDOW = 65536             # pushes in a WaveBoundsStream's window


class WaveHistogramStream(_RingStream):
    """The half waves' joint amplitude-length histogram block by block at a fixed latency (itd_hist_stream_* in include/pyitd_hip.h):
    blocks of `rows` rows go in, finished time slices of their histograms come out — the distribution a live WaveFilterStream's bounds
    follow.  A half wave of at most `horizon` samples is counted exactly once, in the time bin of its peak: wherever no half wave is
    longer than that, the slices are pyitd_amd.wave_histogram of the concatenated rows integer for integer.  A longer one is in no
    cell and not in `outside`; each of its samples adds 1 to `overlong` of its time bin — the price of the bounded latency.  ONE
    launch per push on the GPU.

        st = WaveHistogramStream(1024, rows=9, horizon=2048, amplitude_edges=ae, length_edges=le, hop=512)
        st.latency                                      # D = ceil(horizon / block) = 2
        for block in blocks:                            # block: [rows, 1024]
            out = st.push(block)                        # None for the first D pushes, then block p - D's StreamHistogram:
            ...                                         # out.count, out.samples [rows, 2, Na, Nl]; out.outside, out.overlong [rows, 2]
        while (out := st.flush()) is not None: ...

    block: a multiple of hop, 64 .. 4096; hop: a positive multiple of 64 that divides the block, by default the block.  Each edge
    argument as wave_histogram checks it: float64 [N + 1] (one set for every row) or [rows, N + 1], strictly increasing, no NaN,
    -inf / +inf allowed at the ends, 1 <= N <= 64, at most 1024 cells, and at most 8192 cells per block ((block / hop) Na Nl);
    push(samples, amplitude_edges=, length_edges=) replaces them from that push on.  All four outputs are int32.  A NaN in a pushed
    block sets status() bit 2 until reset(); that row is unspecified from then on.

    Behind a LevelsStream on device pointers, everything on one stream `s`:

        lv = LevelsStream(1024, levels=3, channels=2)
        hs = WaveHistogramStream(1024, rows=2 * 4, horizon=2048, amplitude_edges=ae, length_edges=le, hop=512)
        # rows_d [2, 4, 1024] float64, ae_d [Na + 1], le_d [Nl + 1] float64, count_d / samples_d [8, 2, Na, Nl], out_d / ovl_d [8, 2] int32
        if lv.push_dev(block_ptr, 1024, rows_ptr, 1024, 4 * 1024, None, s):
            if hs.push_dev(rows_ptr, 1024, ae_ptr, 0, le_ptr, 0, count_ptr, samples_ptr, 2 * Na * Nl, out_ptr, ovl_ptr, 2, s):
                ...                                     # the cells of the block pushed levels + 1 + D steps ago
    """

    _NAME = "hist"

    def __init__(self, block, rows=1, horizon=None, amplitude_edges=None, length_edges=None, hop=None, device=0):
        horizon = block if horizon is None else horizon
        if isinstance(block, bool) or int(block) != block or not 64 <= block <= 4096:
            raise ValueError("block must be 64 .. 4096 samples")
        hop = block if hop is None else hop
        if isinstance(hop, bool) or int(hop) != hop or hop < 64 or hop % 64 or block % hop:
            raise ValueError("hop: a positive multiple of 64 that divides the block, got %r" % (hop,))
        self._check_rows_horizon(rows, horizon)
        if amplitude_edges is None or length_edges is None:
            raise ValueError("amplitude_edges and length_edges: float64 [N + 1] or [rows, N + 1]")
        self.rows, self.hop = int(rows), int(hop)
        self.cells = int(block) // self.hop
        self.abins = self.lbins = None
        self._ae, self._le = self._check_edges(amplitude_edges, "amplitude_edges"), self._check_edges(length_edges, "length_edges")
        self.abins, self.lbins = self._ae.shape[-1] - 1, self._le.shape[-1] - 1
        from .batch import MAX_WAVE_CELLS
        if self.abins * self.lbins > MAX_WAVE_CELLS:
            raise ValueError("%d x %d bins are more than %d cells" % (self.abins, self.lbins, MAX_WAVE_CELLS))
        if self.cells * self.abins * self.lbins > MAX_STREAM_HIST_CELLS:
            raise ValueError("%d time bins of %d x %d bins are more than %d cells per block" %
                             (self.cells, self.abins, self.lbins, MAX_STREAM_HIST_CELLS))
        self._create(block, rows, horizon, device, (self.hop, self.abins, self.lbins),
                     ", hop=%d, bins=%d x %d" % (hop, self.abins, self.lbins))

    def _check_edges(self, edges, name):
        from .batch import _hist_edges
        e = _hist_edges(edges, name, (self.rows,))
        bins = self.abins if name == "amplitude_edges" else self.lbins
        if bins is not None and e.shape[-1] != bins + 1:
            raise ValueError("%s: the stream has %d bins, got %d edges" % (name, bins, e.shape[-1]))
        return e

    # ---- device buffers (raw pointers; asynchronous on `stream`) ----------------------------------------------------
    def push_dev(self, block_ptr, in_stride, aedges_ptr, aedges_stride, ledges_ptr, ledges_stride, count_ptr, samples_ptr, hist_stride,
                 outside_ptr=None, overlong_ptr=None, count_stride=0, stream=None):
        """Store one block of every row; True if a block's cells were written."""
        return self._dev("push", (block_ptr, in_stride, aedges_ptr, aedges_stride, ledges_ptr, ledges_stride, count_ptr, samples_ptr,
                                  hist_stride, outside_ptr, overlong_ptr, count_stride), stream)

    def flush_dev(self, aedges_ptr, aedges_stride, ledges_ptr, ledges_stride, count_ptr, samples_ptr, hist_stride, outside_ptr=None,
                  overlong_ptr=None, count_stride=0, stream=None):
        return self._dev("flush", (aedges_ptr, aedges_stride, ledges_ptr, ledges_stride, count_ptr, samples_ptr, hist_stride, outside_ptr,
                                   overlong_ptr, count_stride), stream)

    # ---- numpy in -> numpy out (one synchronisation per call) ----------------------------------------------------------
    def _outputs(self):
        hist, cnt = (self.rows, self.cells, self.abins, self.lbins), (self.rows, self.cells)
        return tuple(numpy.empty(shape, numpy.int32) for shape in (hist, hist, cnt, cnt))

    def _result(self, outs):
        return StreamHistogram(*[o[0] for o in outs]) if self._flat else StreamHistogram(*outs)

    def _edge_params(self, amplitude_edges, length_edges):
        if amplitude_edges is not None:
            self._ae = self._check_edges(amplitude_edges, "amplitude_edges")
        if length_edges is not None:
            self._le = self._check_edges(length_edges, "length_edges")
        ae, le = self._ae, self._le
        return _np_ptr(ae), ae.shape[-1] if ae.ndim == 2 else 0, _np_ptr(le), le.shape[-1] if le.ndim == 2 else 0

    def push(self, samples, amplitude_edges=None, length_edges=None):
        """samples [rows, block] (or [block] for one row).  None for the first `latency` pushes, then StreamHistogram(count[rows, C, Na,
        Nl], samples[rows, C, Na, Nl], outside[rows, C], overlong[rows, C]) of the block pushed `latency` pushes ago (no row axis for
        1-D input)."""
        block = self._block(samples, self.rows)
        return self._host(block, self._edge_params(amplitude_edges, length_edges))

    def flush(self, amplitude_edges=None, length_edges=None):
        """The next block still held (one per call); None once the stream is empty."""
        return self._host(None, self._edge_params(amplitude_edges, length_edges))


def blockwise_wave_histogram(rows, block, horizon, amplitude_edges, length_edges, hop=None, device=0):
    """Run rows[R, n_blocks * block] (or [n]) through a WaveHistogramStream: what a caller with an unbounded source does block by
    block.  Returns StreamHistogram with the blocks' slices concatenated along the time axis: count, samples [R, T, Na, Nl], outside,
    overlong [R, T] with T = n / hop (no row axis for 1-D input)."""
    x2, flat = _as_rows(rows, block, two_d=True)
    outs = _push_then_drain(WaveHistogramStream(block, x2.shape[0], horizon, amplitude_edges, length_edges, hop, device), x2)
    fields = [numpy.concatenate([o[i] for o in outs], axis=1) for i in range(4)]
    return StreamHistogram(*[f[0] if flat else f for f in fields])


StreamWaves = namedtuple("StreamWaves", "count start length peak value")


class WaveTableStream(_Handle):
    """The half-wave table block by block, with no horizon and no latency (itd_table_stream_* in include/pyitd_hip.h): blocks of
    `rows` rows go in, every half wave — start, length, peak, signed extremum — comes out in the push in which its end becomes known,
    whatever its length.  The events of every push and of the flush, concatenated row by row, are pyitd_amd.single_waves of the
    concatenated rows: positions integer for integer, value bit for bit.  What a real-time detector works on ("this half wave was 40
    samples long and 5 uV high"), at 32 bytes per half wave.  ONE launch per push on the GPU; the state between two pushes is the open
    half wave, 48 bytes per row.

        st = WaveTableStream(1024, rows=9)
        for block in blocks:                            # block: [rows, 1024]
            w = st.push(block)                          # StreamWaves: w.count [rows] int32, the tables [rows, 1025]
            ...                                         # row r: entries [0, w.count[r]) ended in this push (a stream's first push:
                                                        # at most block - 2, later ones: at most block); entry w.count[r] is the
                                                        # half wave still open — its start, its length, peak and value so far
        last = st.flush()                               # count == 1, tables [rows, 1]: the final half wave; None if the stream is empty

    block: 8 .. 4096 samples, any value.  origin: added to every reported start and peak (a recording's sample clock).  start, length
    and peak are int64, value float64.  Whether a block's last sample ends a half wave is known from the next block's first sample:
    that event leaves with the next push.  A NaN in a pushed block sets status() bit 2 until reset(); that row's entries are
    unspecified from then on.  reset() drops the open half wave; blocks_held counts the blocks pushed since the stream began.

    Behind a LevelsStream on device pointers, everything on one stream `s`:

        lv = LevelsStream(1024, levels=3, channels=2)
        tb = WaveTableStream(1024, rows=2 * 4)
        # rows_d [2, 4, 1024] float64; start_d, length_d, peak_d [8, 1025] int64, value_d [8, 1025] float64, count_d [8] int32
        if lv.push_dev(block_ptr, 1024, rows_ptr, 1024, 4 * 1024, None, s):
            tb.push_dev(rows_ptr, 1024, start_ptr, length_ptr, peak_ptr, value_ptr, 1025, count_ptr, s)
    """

    def __init__(self, block, rows=1, origin=0, device=0):
        if isinstance(block, bool) or int(block) != block or not 8 <= block <= 4096:
            raise ValueError("block must be 8 .. 4096 samples")
        if not 1 <= rows <= 65535:
            raise ValueError("rows must be 1 .. 65535")
        if int(origin) != origin or not -2 ** 62 <= origin <= 2 ** 62:
            raise ValueError("origin must be an integer of at most 2^62 in magnitude")
        self._open("itd_table_stream_create", "itd_table_stream_create(block=%d, rows=%d, origin=%d)" % (block, rows, origin), int(device),
                   int(block), int(rows), int(origin))
        self.block, self.rows, self.origin, self.device = int(block), int(rows), int(origin), int(device)
        self._flat = False          # the last push took a 1-D block: what leaves has no row axis either

    # ---- device buffers (raw pointers; asynchronous on `stream`) ----------------------------------------------------
    def push_dev(self, block_ptr, in_stride, start_ptr, length_ptr, peak_ptr, value_ptr, event_stride, count_ptr, stream=None):
        """One block of every row; always True.  Row r's slot: event_stride entries in each table (a None table is skipped)."""
        return self._call("itd_table_stream_push_f64", block_ptr, in_stride, start_ptr, length_ptr, peak_ptr, value_ptr, event_stride,
                          count_ptr, stream=stream)

    def flush_dev(self, start_ptr, length_ptr, peak_ptr, value_ptr, event_stride, count_ptr, stream=None):
        """The open half wave into entry 0 of every row's slot, count = 1; False (nothing written) if the stream is empty."""
        return self._call("itd_table_stream_flush_f64", start_ptr, length_ptr, peak_ptr, value_ptr, event_stride, count_ptr, stream=stream)

    # ---- numpy in -> numpy out (one synchronisation per call) ----------------------------------------------------------
    def _host(self, name, head):
        slot = self.block + 1
        tabs = [numpy.empty((self.rows, slot), numpy.float64 if k == 3 else numpy.int64) for k in range(4)]
        count = numpy.zeros(self.rows, numpy.int32)
        if not self._call(name, *head, *[_np_ptr(t) for t in tabs], _np_ptr(count)):
            return None
        return count, tabs

    def push(self, samples):
        """samples [rows, block] (or [block] for one row).  StreamWaves(count[rows] int32, start, length, peak [rows, block + 1] int64,
        value [rows, block + 1] float64) (no row axis for 1-D input); entries behind `count` of a row are not meaningful."""
        x2, flat = self._block(samples, self.rows)
        count, tabs = self._host("itd_table_stream_push_host_f64", (_np_ptr(x2),))
        self._flat = flat
        return StreamWaves(count[0], *[t[0] for t in tabs]) if flat else StreamWaves(count, *tabs)

    def flush(self):
        """The final half wave: StreamWaves with count == 1 and tables [rows, 1], shaped like the last push's; None if the stream
        is empty."""
        r = self._host("itd_table_stream_flush_host_f64", ())
        if r is None:
            return None
        count, tabs = r
        tabs = [numpy.ascontiguousarray(t[:, :1]) for t in tabs]
        return StreamWaves(count[0], *[t[0] for t in tabs]) if self._flat else StreamWaves(count, *tabs)


def blockwise_single_waves(rows, block, origin=0, device=0):
    """Run rows[R, n_blocks * block] (or [n]) through a WaveTableStream: what a caller with an unbounded source does block by block.
    Returns batch.Waves(count, start, length, peak, value) with every row's events concatenated, the tables padded to the largest
    count as single_waves pads them (-1; nan): for origin = 0 it equals single_waves(rows) entry for entry, with int64 positions."""
    from .batch import Waves
    x2, flat = _as_rows(rows, block, two_d=True)
    R = x2.shape[0]
    st = WaveTableStream(block, R, origin, device)
    try:
        steps = [st.push(x2[:, k * block:(k + 1) * block]) for k in range(x2.shape[1] // block)]
        steps.append(st.flush())
    finally:
        st.close()
    count = numpy.sum([w.count for w in steps], axis=0).astype(numpy.int32)
    cap = int(count.max())
    tabs = [numpy.full((R, cap), numpy.nan if k == 3 else -1, numpy.float64 if k == 3 else numpy.int64) for k in range(4)]
    for r in range(R):
        at = 0
        for w in steps:
            c = int(w.count[r])
            for k in range(4):
                tabs[k][r, at:at + c] = w[1 + k][r, :c]
            at += c
    return Waves(count[0], *[t[0] for t in tabs]) if flat else Waves(count, *tabs)


class WaveBoundsStream(_Handle):
    """The wave filter's bounds from the quantiles of a sliding window over a histogram stream's slices (itd_bounds_stream_* in
    include/pyitd_hip.h): push by push the `slices` time slices [rows, slices, Na, Nl] (int32) a WaveHistogramStream emits per block go
    in, and the bounds of the last min(window, pushes) pushes come out — by definition pyitd_amd.wave_filter_bounds of the concatenated
    slices with time_bins = (max(0, p + 1 - window) * slices, (p + 1) * slices) after push p, bit for bit.  No latency, no flush.  ONE
    launch per push on the GPU; the state is a ring of per-push marginals and their running sums, exact integers.

        bs = WaveBoundsStream(rows=9, Na=32, Nl=32, slices=2, window=16)
        b = bs.push(hist.count, ae, le, amplitude_q=(0.1, 0.9))     # float64 [rows, 4]: WaveFilterStream.push(block, bounds=b)

    On device pointers, per block and everything on one stream `s`: the histogram stream's push, this push, the wave-filter stream's
    push with the same horizon — block p - D is then filtered with bounds that already include its own half waves:

        if hs.push_dev(rows_ptr, L, ae_ptr, 0, le_ptr, 0, count_ptr, samples_ptr, C * Na * Nl, None, None, 0, s):
            bs.push_dev(count_ptr, C * Na * Nl, ae_ptr, 0, le_ptr, 0, q_ptr, 0, bounds_ptr, 4, None, s)
        wf.push_dev(rows_ptr, L, bounds_ptr, 4, out_ptr, L, s)

    reset() empties the window; blocks_held counts the pushes since the stream began."""

    def __init__(self, rows, Na, Nl, slices, window, device=0):
        from .batch import MAX_WAVE_BINS, MAX_WAVE_CELLS
        for name, v in (("rows", rows), ("Na", Na), ("Nl", Nl), ("slices", slices), ("window", window)):
            if isinstance(v, bool) or int(v) != v or v < 1:
                raise ValueError("%s must be a positive integer, got %r" % (name, v))
        if rows > 65535:
            raise ValueError("rows must be 1 .. 65535")
        if Na > MAX_WAVE_BINS or Nl > MAX_WAVE_BINS or Na * Nl > MAX_WAVE_CELLS:
            raise ValueError("%d x %d bins: at most %d per axis and %d cells" % (Na, Nl, MAX_WAVE_BINS, MAX_WAVE_CELLS))
        if slices * Na * Nl > MAX_STREAM_HIST_CELLS:
            raise ValueError("%d time slices of %d x %d bins are more than %d cells per push" % (slices, Na, Nl, MAX_STREAM_HIST_CELLS))
        if window > MAX_BOUNDS_WINDOW:
            raise ValueError("window must be 1 .. %d pushes" % MAX_BOUNDS_WINDOW)
        self._open("itd_bounds_stream_create", "itd_bounds_stream_create(rows=%d, bins=%d x %d, slices=%d, window=%d)" %
                   (rows, Na, Nl, slices, window), int(device), int(rows), int(Na), int(Nl), int(slices), int(window))
        self.rows, self.abins, self.lbins, self.slices, self.window, self.device = int(rows), int(Na), int(Nl), int(slices), int(window), int(device)

    # ---- device buffers (raw pointers; asynchronous on `stream`) ----------------------------------------------------
    def push_dev(self, hist_ptr, hist_stride, aedges_ptr, aedges_stride, ledges_ptr, ledges_stride, quant_ptr, quant_stride, bounds_ptr,
                 bounds_stride=4, total_ptr=None, stream=None):
        """One push's slices of every row in, the window's bounds (and totals, int64 [rows]) out; strides of 0: one set for every row."""
        self._check(self._L.itd_bounds_stream_push(self._h, hist_ptr, hist_stride, aedges_ptr, aedges_stride, ledges_ptr, ledges_stride,
                                                   quant_ptr, quant_stride, bounds_ptr, bounds_stride, total_ptr, stream))

    # ---- numpy in -> numpy out (one synchronisation per call) ----------------------------------------------------------
    def push(self, hist, amplitude_edges, length_edges, amplitude_q=(0.0, 1.0), length_q=(0.0, 1.0), amplitude_scale=(1.0, 1.0),
             length_scale=(1.0, 1.0), want_total=False):
        """hist [rows, slices, Na, Nl] int32; edges and parameters as wave_filter_bounds takes them for the leading axis (rows,).
        Returns the bounds float64 [rows, 4]; with want_total also the window's totals, int64 [rows]."""
        from .batch import _bounds_params, _hist_edges
        h = numpy.ascontiguousarray(hist)
        if h.dtype != numpy.int32 or h.shape != (self.rows, self.slices, self.abins, self.lbins):
            raise ValueError("expected int32 slices of shape (%d, %d, %d, %d)" % (self.rows, self.slices, self.abins, self.lbins))
        ae, le = _hist_edges(amplitude_edges, "amplitude_edges", (self.rows,)), _hist_edges(length_edges, "length_edges", (self.rows,))
        if ae.shape[-1] != self.abins + 1 or le.shape[-1] != self.lbins + 1:
            raise ValueError("the stream has %d x %d bins, the edges are %d and %d" % (self.abins, self.lbins, ae.shape[-1], le.shape[-1]))
        q = _bounds_params(amplitude_q, length_q, amplitude_scale, length_scale, (self.rows,))
        bounds = numpy.empty((self.rows, 4), numpy.float64)
        total = numpy.empty(self.rows, numpy.int64) if want_total else None
        self._check(self._L.itd_bounds_stream_push_host(self._h, _np_ptr(h), _np_ptr(ae), ae.shape[-1] if ae.ndim == 2 else 0, _np_ptr(le),
                                                        le.shape[-1] if le.ndim == 2 else 0, _np_ptr(q), 8 if q.ndim == 2 else 0,
                                                        _np_ptr(bounds), _np_ptr(total)))
        return (bounds, total) if want_total else bounds
