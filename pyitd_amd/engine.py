"""Thin Python handle over the C-ABI engine (include/pyitd_hip.h).

Python never touches samples: it marshals pointers, sizes, a stream and the level count.
Device memory for the device-resident entry points is whatever the caller owns (torch tensors,
hipMalloc'd buffers, ...) — only raw pointers cross the boundary.
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import ITDError, MAX_ROWS

STOP_NATURAL, STOP_TIMEOUT = 0, 1
DETECT_KNOTS, DETECT_VALLEYS, DETECT_PEAKS = 0, 1, 2
ITD_OK, ITD_ERR_INVALID_ARG, ITD_ERR_NONFINITE = 0, 1, 6
LEVEL0_AUTO, LEVEL0_RECORDS, LEVEL0_FUSED = 0, 1, 2
TIME_EXTRACT, TIME_EXTRACT_L0, TIME_EXTRACT_FINAL, TIME_DECOMPOSE, TIME_SCAN0, TIME_KF_APPLY, TIME_KF_KNOTS = 0, 1, 2, 3, 4, 5, 6
NAN_INPUT_FOLLOW, NAN_INPUT_REJECT = 0, 1
RESIDENT_AUTO, RESIDENT_OFF, RESIDENT_ONLY = 0, 1, 2
SPLINE_AUTO, SPLINE_SERIAL, SPLINE_PARALLEL = 0, 1, 2
FUSE_AUTO, FUSE_OFF, FUSE_ONLY = 0, 1, 2


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def rows_dtype_of(dtype):
    """The element type of a decomposition's rows: None / float64 (the default) or float32 (the itd_decompose_rows32_* entries);
    anything else raises ValueError."""
    if dtype is None:
        return np.dtype(np.float64)
    try:
        dt = np.dtype(dtype)
    except TypeError:
        dt = None
    if dt is None or dt.kind != "f" or dt.itemsize not in (4, 8):
        raise ValueError("the rows of a decomposition are float64 or float32, not %r" % (dtype,))
    return dt


def selection_of(select, max_iteration):
    """select= of the decompositions as the C entries take it (itd_decompose_select_*): (rotation_mask, want_residual, S).
    select is a strictly ascending sequence of rotation indices 0 .. max_iteration, -1 in the last place standing for the residual:
    [2, 3, -1] keeps rotations 2 and 3 and the residual, in that order.  Anything else — an empty sequence, unsorted or repeated
    indices, an index above max_iteration, -1 anywhere but last, something that is not an integer — raises ValueError."""
    try:
        items = list(select)
    except TypeError:
        raise ValueError("select must be a sequence of rotation indices, -1 last for the residual, not %r" % (select,))
    if not items:
        raise ValueError("select must name at least one row")
    for v in items:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("select holds integers (rotation indices, -1 for the residual), not %r" % (v,))
    items = [int(v) for v in items]
    residual = items[-1] == -1
    rot = items[:-1] if residual else items
    mask = 0
    for k, r in enumerate(rot):
        if r == -1:
            raise ValueError("-1 (the residual) must be the last entry of select")
        if r < 0 or r > max_iteration:
            raise ValueError("select: rotation index %d is outside 0..%d (max_iteration)" % (r, max_iteration))
        if k and r <= rot[k - 1]:
            raise ValueError("select must be strictly ascending (no repeats), got %r" % (items,))
        mask |= 1 << r
    return mask, 1 if residual else 0, len(items)


def zero_absent_slots(rows, select, n_rows):
    """A selected result's slots of rotations the decomposition did not reach (index > n_rows - 2; their content is unspecified)
    set to zero, in place: rows is [S, n] with n_rows an int, or [B, S, n] with n_rows [B].  x is still the sum of all rotations and the residual."""
    rot = np.asarray([r for r in select if r != -1], dtype=np.int64)
    if rows.ndim == 2:
        for k in np.nonzero(rot > int(n_rows) - 2)[0]:
            rows[int(k)] = 0
    else:
        absent = np.zeros(rows.shape[:2], dtype=bool)       # [B, S]: the residual's slot is never absent
        absent[:, : len(rot)] = rot[None, :] > (np.asarray(n_rows, dtype=np.int64)[:, None] - 2)
        if absent.any():                                    # one masked fill (a torch device tensor: one launch)
            if isinstance(rows, np.ndarray):
                rows[absent] = 0
            else:
                import torch
                rows[torch.from_numpy(absent).to(rows.device)] = 0
    return rows


# the C entries of each delivery of a decomposition's rows: device float32 / float64 input, host float32 / float64 input
_ENTRIES = {"full": ("itd_decompose_f32", "itd_decompose_f64", "itd_decompose_host_f32", "itd_decompose_host_f64"),
            "rows32": ("itd_decompose_rows32_f32", "itd_decompose_rows32_f64", "itd_decompose_rows32_host_f32", "itd_decompose_rows32_host_f64"),
            "select": ("itd_decompose_select_f32", "itd_decompose_select_f64", "itd_decompose_select_host_f32", "itd_decompose_select_host_f64")}


def rows_mode(rows_dtype, select, max_iteration):
    """(rows_dtype, select) of a decomposition resolved once, as the C entries take them: a dict of "entries", the four C entries
    (_ENTRIES); "pre" / "post", their arguments in front of and right behind the rows' pointer; "dtype" and "S", the rows' element type
    and their number per signal; "no_baselines", None where the entries take baselines, else what they deliver instead.  A bad
    rows_dtype or select raises ValueError."""
    rdt = rows_dtype_of(rows_dtype)
    r32 = rdt == np.float32
    if select is not None:
        mask, want_res, S = selection_of(select, max_iteration)
        return {"entries": _ENTRIES["select"], "pre": (mask, want_res), "post": (1 if r32 else 0,), "dtype": rdt, "S": S,
                "no_baselines": "selected rows"}
    return {"entries": _ENTRIES["rows32" if r32 else "full"], "pre": (), "post": (), "dtype": rdt, "S": max_iteration + 2,
            "no_baselines": "float32 rows" if r32 else None}


class Engine:
    """One engine = one GPU + one workspace sized for (max_n, max_batch).  Not thread-safe."""

    def __init__(self, max_n, max_batch=1, device=0):
        self._L = _lib.load()
        h = ctypes.c_void_p()
        rc = self._L.itd_engine_create(ctypes.byref(h), int(device), int(max_n), int(max_batch))
        if rc:
            raise ITDError(rc, "itd_engine_create(max_n=%d, max_batch=%d, device=%d)" % (max_n, max_batch, device))
        self._h = h
        self.max_n, self.max_batch, self.device = int(max_n), int(max_batch), int(device)
        mode = os.environ.get("PYITD_LEVEL0_MODE")      # diagnostic override: run a whole test suite in one level-0 mode
        if mode:
            self.set_level0_mode(int(mode))
        mode = os.environ.get("PYITD_FUSE_MODE")        # the fused sparse levels (FUSE_*)
        if mode:
            self.set_fuse_mode(int(mode))
        mode = os.environ.get("PYITD_FUSE_LEVEL")       # the first fused level (diagnostic sweeps)
        if mode:
            self.set_fuse_level(int(mode))
        mode = os.environ.get("PYITD_FUSE_CAP")         # capped fused levels (a whole suite with the fused levels cut at this level)
        if mode:
            self.set_fuse_cap(int(mode))
        mode = os.environ.get("PYITD_FUSE_RANGE")       # tiles per knot-side workgroup of the fused levels (sweeps; 16 / 32 / 64)
        if mode:
            self.set_fuse_range(int(mode))
        mode = os.environ.get("PYITD_FUSE_MIN")         # samples per launch sequence from which FUSE_AUTO fuses (tests: 65536)
        if mode:
            self.set_fuse_min_samples(int(mode))
        mode = os.environ.get("PYITD_RESIDENT_MODE")    # and for the one-workgroup form of short signals (RESIDENT_*)
        if mode:
            self.set_resident_mode(int(mode))

    def close(self):
        if getattr(self, "_h", None):
            self._L.itd_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, allow=()):
        if rc and rc not in allow:
            raise ITDError(rc, self._L.itd_last_error(self._h).decode())
        return rc

    @property
    def workspace_bytes(self):
        return self._L.itd_engine_workspace_bytes(self._h)

    # ---- device-resident path ---------------------------------------------------------------
    def decompose_dev(self, x_ptr, dtype, n, batch, x_stride, max_iteration, rows_ptr, baselines_ptr=None,
                      stream=None, rows_dtype=np.float64, select=None):
        """Enqueue a decomposition of device data (no host sync).  Pointers are ints.
        rows_dtype: float64, or float32 — rows_ptr is then [batch][max_iteration + 2][n] float32, every element the float64 row's
        rounded once at its store; no baselines in that mode.
        select: only these rows (selection_of): rows_ptr is [batch][S][n] of rows_dtype, the selected rotations in ascending order and
        the residual last; nothing else is stored anywhere.  The slot of a rotation above summary()'s n_rows - 2 holds unspecified
        values.  No baselines either."""
        mode = rows_mode(rows_dtype, select, max_iteration)
        if mode["no_baselines"] and baselines_ptr:
            raise ValueError("baselines are not kept with " + mode["no_baselines"])
        f = getattr(self._L, mode["entries"][0 if np.dtype(dtype) == np.float32 else 1])
        bases = () if mode["no_baselines"] else (baselines_ptr,)
        self._check(f(self._h, x_ptr, n, batch, x_stride, max_iteration, *mode["pre"], rows_ptr, *mode["post"], *bases, stream))

    def summary(self, batch):
        n_rows = np.zeros(batch, np.int32)
        n_b = np.zeros(batch, np.int32)
        stop = np.zeros(batch, np.int32)
        kc = np.zeros((batch, MAX_ROWS + 1), np.int64)
        nanlv = np.zeros(batch, np.int32)
        self._check(self._L.itd_get_summary(self._h, _np_ptr(n_rows), _np_ptr(n_b), _np_ptr(stop), _np_ptr(kc),
                                            _np_ptr(nanlv)))
        return {"n_rows": n_rows, "n_baselines": n_b, "stop": stop, "knot_counts": kc, "nan_levels": nanlv}

    def set_timing(self, max_decompositions, stride=1):
        """Record hipEvent pairs around the extraction launches of the next `max_decompositions` runs (0 = off);
        only every `stride`-th run is instrumented."""
        self._check(self._L.itd_set_kernel_timing_stride(self._h, int(stride)))
        self._check(self._L.itd_set_kernel_timing(self._h, int(max_decompositions)))

    def set_nan_input_mode(self, mode):
        """NAN_INPUT_FOLLOW (default: a NaN in the input is treated as the reference treats it, ITD.py:46-51) or NAN_INPUT_REJECT."""
        self._check(self._L.itd_set_nan_input_mode(self._h, int(mode)))

    def set_level0_mode(self, mode):
        """LEVEL0_AUTO (fused level 0, record-driven repeat if the input is too smooth), LEVEL0_RECORDS, LEVEL0_FUSED."""
        self._check(self._L.itd_set_level0_mode(self._h, int(mode)))

    def set_fuse_mode(self, mode):
        """FUSE_AUTO (long signals: the sparse levels run on the knot list, the samples take one pass for all of them; a call whose
        verification fails is repeated level by level), FUSE_OFF, FUSE_ONLY (never repeat)."""
        self._check(self._L.itd_set_fuse_mode(self._h, int(mode)))

    def set_valid_flags(self, valid_dev_ptr):
        """valid_dev_ptr: device pointer to int32[batch] (0 / None = off): behind every later decomposition's last launch the engine
        writes 1 where a signal's rows are final, 0 where `summary()` still has a level-by-level repeat to run (include/pyitd_hip.h)."""
        self._check(self._L.itd_set_valid_flags(self._h, ctypes.c_void_p(int(valid_dev_ptr or 0))))

    def set_device_repair(self, on=True):
        """The level-by-level repeat of a refused optimistic form enqueued by the engine itself, guarded per signal on the device:
        the rows are final when the stream has drained (no `summary()` needed in between; graph-capturable)."""
        self._check(self._L.itd_set_device_repair(self._h, 1 if on else 0))

    @property
    def device_repairs(self):
        return int(self._L.itd_get_device_repairs(self._h))

    def set_timing_mode(self, mode):
        """0: every launch class carries events; 1: only each decomposition's level-0 launch (step_periods())."""
        self._check(self._L.itd_set_kernel_timing_mode(self._h, int(mode)))

    def kernel_timing_samples(self, which=TIME_EXTRACT, cap=4096):
        """The individual durations (ms) of the recorded launches of class `which`, in launch order."""
        buf = (ctypes.c_double * cap)()
        cnt = ctypes.c_int32(0)
        self._check(self._L.itd_get_kernel_timing_samples(self._h, which, buf, cap, ctypes.byref(cnt)))
        return np.array(buf[: min(cnt.value, cap)], dtype=np.float64)

    def step_periods(self, cap=4096):
        """ms from one recorded decomposition's first launch to the next one's (set_timing_mode(1), back-to-back calls)."""
        buf = (ctypes.c_double * cap)()
        cnt = ctypes.c_int32(0)
        self._check(self._L.itd_get_step_periods(self._h, buf, cap, ctypes.byref(cnt)))
        return np.array(buf[: min(cnt.value, cap)], dtype=np.float64)

    def set_fuse_range(self, tiles):
        """Tiles per knot-side workgroup of the fused levels: 64, 32, 16, or 0 = automatic (halved after a call whose lists outgrew them)."""
        self._check(self._L.itd_set_fuse_range(self._h, int(tiles)))

    def debug_kf_fault(self, kind, level=3, where=0, slot=0, delta=1):
        """Tests only: arm one fault in what the fused levels' knot side hands to their sample pass (include/pyitd_hip.h:
        itd_debug_kf_fault); kind < 0 disarms."""
        self._check(self._L.itd_debug_kf_fault(self._h, int(kind), int(level), int(where), int(slot), int(delta)))

    def debug_kf_fault_signal(self, signal):
        """Tests only: the armed fault lands in signal `signal` of the batch (default 0)."""
        self._check(self._L.itd_debug_kf_fault_signal(self._h, int(signal)))

    def set_fuse_cap(self, first_level_not_fused):
        """Capped fused levels: 0 (default) = automatic (a refusal's failing level caps the next calls' fused levels, the rest runs level
        by level), -1 = never, 4 .. max_iteration + 1 = always this cap."""
        self._check(self._L.itd_set_fuse_cap(self._h, int(first_level_not_fused)))

    @property
    def last_fuse_cap(self):
        """The cap of the last decomposition's fused levels as enqueued (0 = none)."""
        return self._L.itd_get_last_fuse_cap(self._h)

    def set_fuse_level(self, first_fused_level):
        """The first fused level, 2 .. max_iteration, or 0 (default) = automatic: 2 where a launch sequence covers >= 2^22 samples, else 3."""
        self._check(self._L.itd_set_fuse_level(self._h, int(first_fused_level)))

    def set_fuse_min_samples(self, samples):
        """FUSE_AUTO fuses calls whose launch sequences cover at least this many samples (default 6 * 2^20: below that every
        launch is bound by its boundary and the fused form has more of them)."""
        self._check(self._L.itd_set_fuse_min_samples(self._h, int(samples)))

    @property
    def fuse_repeats(self):
        """Calls of this engine that itd_get_summary had to repeat level by level because the fused levels reported a failure."""
        return self._L.itd_get_fuse_repeats(self._h)

    @property
    def last_fuse_level(self):
        """The first fused level of the last decomposition as enqueued (2, 3, ...), 0 = one launch per level / resident form."""
        return self._L.itd_get_last_fuse_level(self._h)

    @property
    def fuse_signal_repairs(self):
        """Single signals of batches that itd_get_summary re-ran on their own (at most one in eight of a batch refused the fused
        form: the rest of the batch kept its fused result)."""
        return int(self._L.itd_get_fuse_signal_repairs(self._h))

    def set_resident_mode(self, mode):
        """RESIDENT_AUTO (signals of <= 8192 samples run as one workgroup each in one launch, the signal resident in LDS; a call
        that meets a non-finite value is repeated level by level), RESIDENT_OFF, RESIDENT_ONLY (never repeat)."""
        self._check(self._L.itd_set_resident_mode(self._h, int(mode)))

    def set_resident_window(self, segments):
        """Knot-to-knot segments of a level the resident form holds in LDS per pass (0 = automatic); results do not depend on it."""
        self._check(self._L.itd_set_resident_window(self._h, int(segments)))

    @property
    def resident_repeats(self):
        """Resident calls of this engine that itd_get_summary had to repeat level by level so far."""
        return self._L.itd_get_resident_repeats(self._h)

    def set_batch_chunk(self, signals_per_chunk):
        """Signals per launch sequence of a batched decomposition (0 = automatic, about 2^24 samples per chunk)."""
        self._check(self._L.itd_set_batch_chunk(self._h, int(signals_per_chunk)))

    def set_batch_streams(self, streams):
        """1 or 2: the chunks of a batched decomposition alternate over that many streams."""
        self._check(self._L.itd_set_batch_streams(self._h, int(streams)))

    def kernel_timing(self, which=TIME_EXTRACT):
        """(total ms, launches) of the recorded launches of class `which` (TIME_*)."""
        ms, cnt = ctypes.c_double(0), ctypes.c_int32(0)
        self._check(self._L.itd_get_kernel_timing(self._h, which, ctypes.byref(ms), ctypes.byref(cnt)))
        return ms.value, cnt.value

    # ---- numpy in -> numpy out ----------------------------------------------------------------
    def decompose_host(self, x, max_iteration, want_baselines=True, out=None, rows_dtype=np.float64, select=None):
        """want_baselines: True = copy them back now; False = none; "lazy" = leave them on the device: the result carries
        `n_baselines` and `fetch_baselines()`, valid until this engine's next host-form decomposition.
        out: a caller-owned float64 C-contiguous array of at least (max_iteration + 2, n) the rows are written into (a loop over
        calls then neither allocates nor releases 8 (max_iteration + 2) n bytes per call).
        rows_dtype: float64, or float32 — the rows (and `out`) are float32 then, each element the float64 row's rounded once on the
        device; the result carries no baselines in that mode, whatever want_baselines says.
        select: only these rows (selection_of): the result's "rows" (and `out`) are [S, n], the selected rotations in ascending
        order and the residual last, with "n_rows" the full decomposition's count; the slots of rotations it did not reach
        (index > n_rows - 2) are zero.  No baselines in that mode either."""
        mode = rows_mode(rows_dtype, select, max_iteration)
        rdt, R, full = mode["dtype"], mode["S"], mode["no_baselines"] is None
        x = np.ascontiguousarray(x)
        if x.dtype != np.float32:
            x = np.ascontiguousarray(x, dtype=np.float64)
        n = x.shape[0]
        if out is None:
            rows = np.empty((R, n), rdt)
        else:
            if not (isinstance(out, np.ndarray) and out.dtype == rdt and out.ndim == 2 and out.shape[0] >= R
                    and out.shape[1] == n and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]):
                raise ValueError("out must be a writable C-contiguous %s array of shape (>= %d, %d)" % (rdt.name, R, n))
            rows = out
        lazy = full and want_baselines == "lazy"
        if full:
            self._check(self._L.itd_set_host_keep_baselines(self._h, 1 if lazy else 0))
        bases = np.zeros((R, n), np.float64) if (full and want_baselines and not lazy) else None
        n_rows, n_b, stop = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        kc = np.zeros(MAX_ROWS + 1, np.int64)
        f = getattr(self._L, mode["entries"][2 if x.dtype == np.float32 else 3])
        rc = self._check(f(self._h, _np_ptr(x), n, max_iteration, *mode["pre"], _np_ptr(rows), *mode["post"],
                           *((_np_ptr(bases), ctypes.byref(n_rows), ctypes.byref(n_b)) if full else (ctypes.byref(n_rows),)),
                           ctypes.byref(stop), _np_ptr(kc)), allow=(ITD_ERR_NONFINITE,))
        out = {"rows": rows[: n_rows.value], "stop": stop.value, "knot_counts": kc, "nonfinite": rc == ITD_ERR_NONFINITE}
        if select is not None:     # all S slots, and the full decomposition's count beside them
            out.update(rows=zero_absent_slots(rows[:R], list(select), n_rows.value), n_rows=n_rows.value)
        if lazy:
            nb = n_b.value
            out["n_baselines"] = nb

            def fetch_baselines():
                b = np.zeros((nb, n), np.float64)
                self._check(self._L.itd_get_last_baselines_host(self._h, _np_ptr(b), n, nb))
                return b
            out["fetch_baselines"] = fetch_baselines
        elif bases is not None:
            out["baselines"] = bases[: n_b.value]
        return out

    def baseline_extract_host(self, x, want_knots=False):
        x = np.ascontiguousarray(x, dtype=np.float64)
        n = x.shape[0]
        rot, base = np.empty(n), np.empty(n)
        kn = np.empty(n, np.int64) if want_knots else None
        bk = np.empty(n + 2) if want_knots else None
        m = ctypes.c_int64(0)
        self._check(self._L.itd_baseline_extract_host_f64(self._h, _np_ptr(x), n, _np_ptr(rot), _np_ptr(base),
                                                          _np_ptr(kn), ctypes.byref(m), _np_ptr(bk)))
        if want_knots:
            return rot, base, kn[: m.value].copy(), bk[: m.value + 2].copy()
        return rot, base

    def detect_host(self, x, mode=DETECT_KNOTS):
        x = np.ascontiguousarray(x, dtype=np.float64)
        n = x.shape[0]
        idx = np.empty(n, np.int64)
        m = ctypes.c_int64(0)
        self._check(self._L.itd_detect_host_f64(self._h, _np_ptr(x), n, mode, _np_ptr(idx), ctypes.byref(m)))
        return idx[: m.value].copy()

    def knot_values_host(self, baseline_knots, x, extrema_indices):
        x = np.ascontiguousarray(x, dtype=np.float64)
        e = np.ascontiguousarray(extrema_indices, dtype=np.int64)
        bk = np.ascontiguousarray(baseline_knots, dtype=np.float64)
        self._check(self._L.itd_knot_values_host_f64(self._h, _np_ptr(x), x.shape[0], _np_ptr(e), e.shape[0] - 2,
                                                     _np_ptr(bk)))
        return bk

    def knot_values_dev(self, x_ptr, n, extrema_ptr, m, bk_ptr, stream=None):
        """baseline_knot_estimation on device buffers (itd_knot_values_f64): x float64[n], extrema int32[m+2], bk float64[m+2]
        (bk[1..m] are written); asynchronous on `stream`."""
        self._check(self._L.itd_knot_values_f64(self._h, x_ptr, n, extrema_ptr, m, bk_ptr, stream))

    # ---- cubic-spline baseline variant (include/pyitd_hip.h: itd_baseline_extract_cubic_*, itd_find_extrema_*) ----------
    def find_extrema_host(self, signal):
        """find_extrema (itd_fourier_decomposition.py:17-31): (extrema int64[n] zero padded, idx)."""
        s = np.ascontiguousarray(signal, dtype=np.float64)
        n = s.shape[0]
        ext = np.zeros(n, np.int64)
        idx = ctypes.c_int64(0)
        self._check(self._L.itd_find_extrema_host_f64(self._h, _np_ptr(s), n, _np_ptr(ext), ctypes.byref(idx)))
        return ext, int(idx.value)

    def _cubic_host(self, fn, arr, n, extrema, idx, what):
        """The host forms of the natural-cubic operator: fn the ABI entry, arr its float64 input (n samples, one or two values each)."""
        base = np.empty(n)
        got = ctypes.c_int64(0)
        if extrema is None:
            kn = np.zeros(n, np.int64)
            self._check(fn(self._h, _np_ptr(arr), n, None, 0, _np_ptr(base), ctypes.byref(got), _np_ptr(kn)))
            return (base if got.value >= 2 else None), kn, int(got.value)
        e = np.ascontiguousarray(extrema, dtype=np.int64)
        if e.shape[0] < idx + 1:
            raise ValueError("%s needs idx+1 entries" % what)
        self._check(fn(self._h, _np_ptr(arr), n, _np_ptr(e), int(idx), _np_ptr(base), ctypes.byref(got), None))
        return base, e, int(idx)

    def cubic_extract_host(self, x, extrema=None, idx=0):
        """itd_baseline_extract_fast (itd_fourier_decomposition.py:49-122).  extrema=None: the knots are detected with
        itd.cpp's predicate (itd.cpp:161-168).  Returns (baseline or None when fewer than 2 knots, knots int64, idx)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        return self._cubic_host(self._L.itd_baseline_extract_cubic_host_f64, x, x.shape[0], extrema, idx, "extrema_input")

    def iq_extract_host(self, z, extrema=None, idx=0):
        """itd_baseline_extract_iq (itd.cpp:58-154): ONE real natural-cubic baseline for complex data — knots where both components
        have an extremum (extrema=None) or the caller's, the operator on the components' mean.  Returns (baseline or None when fewer
        than 2 knots, knots int64, idx)."""
        z = np.ascontiguousarray(z, dtype=np.complex128)
        # interleaved (re, im)
        return self._cubic_host(self._L.itd_baseline_extract_iq_host_f64, z.view(np.float64), z.shape[0], extrema, idx, "extrema")

    # ---- batched single-level operators on device buffers (asynchronous; include/pyitd_hip.h: *_batch_f64) ---------------
    def extract_batch_dev(self, x_ptr, n, batch, x_stride, rot_ptr, rot_stride, base_ptr, base_stride, info_ptr=None, stream=None):
        """itd_baseline_extract (ITD.py:79-121) of every row; info int32[batch]: knot count, -1 - count if the row holds a NaN."""
        self._check(self._L.itd_baseline_extract_batch_f64(self._h, x_ptr, n, batch, x_stride, rot_ptr, rot_stride, base_ptr,
                                                           base_stride, info_ptr, stream))

    def detect_batch_dev(self, x_ptr, n, batch, x_stride, mode=DETECT_KNOTS, idx_ptr=None, idx_stride=0, info_ptr=None, stream=None):
        """Knots of every row by predicate `mode`; idx_ptr None: counts only."""
        self._check(self._L.itd_detect_batch_f64(self._h, x_ptr, n, batch, x_stride, mode, idx_ptr, idx_stride, info_ptr, stream))

    def cubic_batch_dev(self, x_ptr, n, batch, x_stride, extrema_ptr, extrema_stride, idx, base_ptr, base_stride, info_ptr=None,
                        stream=None):
        """itd_baseline_extract_fast of every row; extrema_stride 0: one retained knot list for every row (itd.cpp:40-44)."""
        self._check(self._L.itd_baseline_extract_cubic_batch_f64(self._h, x_ptr, n, batch, x_stride, extrema_ptr, extrema_stride,
                                                                 idx, base_ptr, base_stride, info_ptr, stream))

    def instantaneous_batch_dev(self, rows_ptr, dtype, n, rows, row_stride, amp_ptr, phase_ptr, freq_ptr, out_stride, out_f32=False,
                                info_ptr=None, stream=None):
        """Instantaneous amplitude / phase / frequency of every row (float32 or float64 by `dtype`) into the outputs that are not
        None, float32 when out_f32; info int32[rows]: zero-crossing count, -1 - count if the row holds a NaN.  Pointers in, nothing
        copied, nothing awaited."""
        fn = self._L.itd_instantaneous_batch_f32 if np.dtype(dtype) == np.float32 else self._L.itd_instantaneous_batch_f64
        self._check(fn(self._h, rows_ptr, n, rows, row_stride, amp_ptr, phase_ptr, freq_ptr, out_stride, 1 if out_f32 else 0,
                       info_ptr, stream))

    def tfe_spectrum_dev(self, rows_ptr, dtype, n, rows, row_stride, edges_ptr, bins, hop, weight, spec_ptr, spec_stride,
                         outside_ptr=None, info_ptr=None, stream=None):
        """The time-frequency-energy spectrum of every row (float32 or float64 by `dtype`): float64 [T, bins] per row at
        spec_stride elements, T = ceil(n / hop); edges float64 [bins + 1] in device memory; weight 0 count, 1 amplitude, 2 energy;
        outside int32 [rows, T] (optional); info as for instantaneous_batch_dev.  Pointers in, nothing copied, nothing awaited."""
        fn = self._L.itd_tfe_spectrum_f32 if np.dtype(dtype) == np.float32 else self._L.itd_tfe_spectrum_f64
        self._check(fn(self._h, rows_ptr, n, rows, row_stride, edges_ptr, bins, hop, weight, spec_ptr, spec_stride, outside_ptr,
                       info_ptr, stream))

    def waves_batch_dev(self, rows_ptr, dtype, n, rows, row_stride, start_ptr, length_ptr, peak_ptr, value_ptr, wave_stride, cap,
                        count_ptr=None, info_ptr=None, stream=None):
        """The half waves of every row (float32 or float64 by `dtype`): start / length / peak int32 and value float64 at
        wave_stride entries per row, the first min(count, cap) of each written; count int32[rows] the true count; info as for
        instantaneous_batch_dev.  All four table pointers None: counts only.  Pointers in, nothing copied, nothing awaited."""
        fn = self._L.itd_waves_batch_f32 if np.dtype(dtype) == np.float32 else self._L.itd_waves_batch_f64
        self._check(fn(self._h, rows_ptr, n, rows, row_stride, start_ptr, length_ptr, peak_ptr, value_ptr, wave_stride, cap, count_ptr,
                       info_ptr, stream))

    def wave_filter_batch_dev(self, rows_ptr, dtype, n, rows, row_stride, bounds_ptr, bounds_stride, out_ptr, out_stride, out_f32=False,
                              info_ptr=None, stream=None):
        """Every row with the samples of the half waves outside the float64 bounds (amp_lo, amp_hi, len_lo, len_hi) zeroed;
        bounds_stride 0: one set for every row, >= 4: one per row.  Pointers in, nothing copied, nothing awaited."""
        fn = self._L.itd_wave_filter_batch_f32 if np.dtype(dtype) == np.float32 else self._L.itd_wave_filter_batch_f64
        self._check(fn(self._h, rows_ptr, n, rows, row_stride, bounds_ptr, bounds_stride, out_ptr, out_stride, 1 if out_f32 else 0,
                       info_ptr, stream))

    def wave_hist_batch_dev(self, rows_ptr, dtype, n, rows, row_stride, aedges_ptr, aedges_stride, abins, ledges_ptr, ledges_stride, lbins,
                            hop, count_ptr, samples_ptr, hist_stride, outside_ptr=None, info_ptr=None, stream=None):
        """Every row's half waves binned over time (T = ceil(n / hop), by the peak), amplitude and length: count and samples int32
        [T, abins, lbins] per row at hist_stride elements (either may be None), outside int32 [rows, T] (optional); the float64
        edges in device memory, a stride of 0: one set for every row.  Pointers in, nothing copied, nothing awaited."""
        fn = self._L.itd_wave_hist_batch_f32 if np.dtype(dtype) == np.float32 else self._L.itd_wave_hist_batch_f64
        self._check(fn(self._h, rows_ptr, n, rows, row_stride, aedges_ptr, aedges_stride, abins, ledges_ptr, ledges_stride, lbins, hop,
                       count_ptr, samples_ptr, hist_stride, outside_ptr, info_ptr, stream))

    # ---- the FITPACK flavour of the baseline and its 2-D consumers (itd_baseline_extract_spline_*, itd_crossways_*) --------
    def spline_extract_host(self, x, min_extrema=10, want_rotation=False, want_baseline_knots=False):
        """x[B, n] float64 -> (baseline[B, n], rotation[B, n] or None, knots[B]) (numba_accelerated_itd.py:182-211);
        want_baseline_knots: a fourth item, the knot count of every produced baseline (counted on the device)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        B, n = x.shape
        base = np.empty((B, n))
        rot = np.empty((B, n)) if want_rotation else None
        knots = np.zeros(B, np.int32)
        bk = np.zeros(B, np.int32) if want_baseline_knots else None
        self._check(self._L.itd_baseline_extract_spline_host2_f64(self._h, _np_ptr(x), n, B, int(min_extrema), _np_ptr(base),
                                                                  _np_ptr(rot), _np_ptr(knots), _np_ptr(bk)))
        return (base, rot, knots, bk) if want_baseline_knots else (base, rot, knots)

    def set_spline_solver(self, solver):
        """SPLINE_AUTO (parallel in the knots for few long signals, FITPACK's serial sweep for many rows), SPLINE_SERIAL (bit-level
        against scipy), SPLINE_PARALLEL (not-a-knot moment form: equal to rounding)."""
        self._check(self._L.itd_set_spline_solver(self._h, int(solver)))

    def count_knots_host(self, x, mode=DETECT_KNOTS):
        """Knot counts of x[B, n] (or one signal [n]) under predicate `mode`: no index list is built or copied."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        x2 = x.reshape(1, -1) if x.ndim == 1 else x
        out = np.zeros(x2.shape[0], np.int32)
        self._check(self._L.itd_count_knots_host_f64(self._h, _np_ptr(x2), x2.shape[1], x2.shape[0], int(mode), _np_ptr(out)),
                    allow=(ITD_ERR_NONFINITE,))
        return out

    # ---- MEITD's operators on device-resident signals (pointers are ints; only scalars come back) ----------------------------
    def count_knots_dev(self, x_ptr, n, mode=DETECT_KNOTS, stream=None):
        """The knot count of the n float64 samples at x_ptr (matlab_detect_peaks(x).size + matlab_detect_peaks(-x).size)."""
        out = np.zeros(1, np.int32)
        self._check(self._L.itd_count_knots_f64(self._h, x_ptr, n, 1, n, int(mode), _np_ptr(out), stream), allow=(ITD_ERR_NONFINITE,))
        return int(out[0])

    def wpe3_dev(self, x_ptr, n, want_knots=False, stream=None):
        """(weights[6], windows[6]) of the six order-3 permutation patterns of the n samples at x_ptr (MEITD.py:79-128), in
        numpy.unique's order of the reference's hash values; want_knots: a third item, x's knot count (same synchronisation)."""
        w = np.zeros(6, np.float64)
        c = np.zeros(6, np.int64)
        k = np.zeros(1, np.int32) if want_knots else None
        self._check(self._L.itd_wpe3_f64(self._h, x_ptr, n, _np_ptr(w), _np_ptr(c), _np_ptr(k), stream), allow=(ITD_ERR_NONFINITE,))
        return (w, c, int(k[0])) if want_knots else (w, c)

    def wpe_dev(self, x_ptr, n, order, stream=None):
        """(sums[order^order], windows[order^order]) by the reference's hash value, for any order 2 .. 5 (MEITD.py:79-128)."""
        nh = int(order) ** int(order)
        w = np.zeros(nh, np.float64)
        c = np.zeros(nh, np.int64)
        self._check(self._L.itd_wpe_f64(self._h, x_ptr, n, int(order), _np_ptr(w), _np_ptr(c), stream))
        return w, c

    def spline_extract_dev(self, x_ptr, n, base_ptr, rot_ptr=None, min_extrema=0, want_baseline_knots=False, stream=None):
        """The spline baseline of the n samples at x_ptr into base_ptr (x - baseline into rot_ptr): returns the signal's knot
        count, and the produced baseline's with want_baseline_knots."""
        k = np.zeros(1, np.int32)
        bk = np.zeros(1, np.int32) if want_baseline_knots else None
        self._check(self._L.itd_baseline_extract_spline2_f64(self._h, x_ptr, n, 1, n, int(min_extrema), base_ptr, n, rot_ptr, n,
                                                             _np_ptr(k), _np_ptr(bk), stream))
        return (int(k[0]), int(bk[0])) if want_baseline_knots else int(k[0])

    MEITD_PROBE = np.dtype([("w", np.float64, 6), ("c", np.int32, 6), ("count", np.int32), ("pad", np.int32), ("wpe", np.float64)])

    def meitd_small_dev(self, rows_ptr, n, wpemax, stream=None):
        """MEITD's selection loop on the device rows at rows_ptr (include/pyitd_hip.h: itd_meitd_small_f64; the signal in row 5):
        returns (result[24] = status, high rows, low rows, residual's row, probes, extractions, turns, 0, then the launch's time per
        operator kind in 10 ns units: probes, extractions, counts, copies; the probes' log)."""
        res = np.zeros(24, np.int32)
        log = np.zeros(1024, self.MEITD_PROBE)
        self._check(self._L.itd_meitd_small_f64(self._h, rows_ptr, n, float(wpemax), _np_ptr(res), _np_ptr(log), len(log), stream))
        return res, log[:min(int(res[4]), len(log))]

    def meitd_batch_dev(self, rows_ptr, n, batch, rows_stride, wpemax, x=None, xitd=False, stream=None):
        """The same loop on `batch` signals, one workgroup each, in one launch (include/pyitd_hip.h: itd_meitd_batch_f64): signal b's
        50 rows at rows_ptr + 8 * b * rows_stride; x (optional, float64[batch, n]) is copied into row 5 of every block first.  Returns
        (result[batch, 24] as meitd_small_dev's, logs[batch, 1024] — signal b's first min(result[b, 4], 1024) entries are its log —,
        and with xitd XITD's sums and window counts [batch, 22, 6] of each delivered signal's high rows, low rows and residual, else
        None, None)."""
        res = np.zeros((batch, 24), np.int32)
        logs = np.empty((batch, 1024), self.MEITD_PROBE)
        xw = np.zeros((batch, 22, 6), np.float64) if xitd else None
        xc = np.zeros((batch, 22, 6), np.int64) if xitd else None
        if x is not None:
            x = np.ascontiguousarray(x, dtype=np.float64)
            if x.shape != (batch, n):
                raise ValueError("meitd_batch_dev: x must be [batch, n]")
        self._check(self._L.itd_meitd_batch_f64(self._h, rows_ptr, n, batch, rows_stride, _np_ptr(x), float(wpemax), _np_ptr(res),
                                                _np_ptr(logs), logs.shape[1], _np_ptr(xw), _np_ptr(xc), stream))
        return res, logs, xw, xc

    def gather_rows_dev(self, src_ptr, src_elems, offsets, n, dst_ptr, out=None, stream=None):
        """rows of n float64 at the element offsets `offsets` of src_ptr (a buffer of src_elems), one after the other into dst_ptr;
        out (optional, a C-contiguous float64[len(offsets), n]): then downloaded into it."""
        tab = np.ascontiguousarray(offsets, dtype=np.int64)
        if out is not None and (out.dtype != np.float64 or not out.flags["C_CONTIGUOUS"] or out.shape != (len(tab), n)):
            raise ValueError("gather_rows_dev: out must be a C-contiguous float64[%d, %d]" % (len(tab), n))
        self._check(self._L.itd_gather_rows_f64(self._h, src_ptr, src_elems, _np_ptr(tab), len(tab), n, dst_ptr, _np_ptr(out), stream))

    def subtract_dev(self, a_ptr, b_ptr, out_ptr, count, stream=None):
        self._check(self._L.itd_subtract_f64(self._h, a_ptr, b_ptr, out_ptr, count, stream))

    def copy(self, dst, src, nbytes, kind, wait=False, stream=None):
        """A copy ordered on the engine's stream: kind 0 device -> host, 1 host -> device, 2 device -> device, 3 zero fill."""
        self._check(self._L.itd_copy(self._h, dst, src, nbytes, int(kind), 1 if wait else 0, stream))

    def crossways_host(self, images, min_extrema=10):
        """images[P, rows, cols] float64 -> crossways_itd_baseline_extract of every plane (siftED2D.ipynb cell 1)."""
        img = np.ascontiguousarray(images, dtype=np.float64)
        P, r, c = img.shape
        out = np.empty((P, r, c))
        self._check(self._L.itd_crossways_host_f64(self._h, _np_ptr(img), P, r, c, int(min_extrema), _np_ptr(out)))
        return out

    def instantaneous_host(self, rotation):
        """(amplitude, phase, frequency) of a proper rotation, float64[n] each (include/pyitd_hip.h: itd_instantaneous_*)."""
        x = np.ascontiguousarray(rotation, dtype=np.float64)
        n = x.shape[0]
        a, p, f = np.empty(n), np.empty(n), np.empty(n)
        self._check(self._L.itd_instantaneous_host_f64(self._h, _np_ptr(x), n, _np_ptr(a), _np_ptr(p), _np_ptr(f)))
        return a, p, f


class DeviceBuffer:
    """hipMalloc'd bytes on one GPU through the C ABI (itd_dev_alloc / itd_dev_copy / itd_dev_free): what the numpy
    entry points use for device-resident staging when the caller brings no allocator of its own (no torch needed)."""

    def __init__(self, nbytes, device=0):
        self._L = _lib.load()
        self.device, self.nbytes = int(device), int(nbytes)
        p = ctypes.c_void_p()
        rc = self._L.itd_dev_alloc(self.device, max(self.nbytes, 1), ctypes.byref(p))
        if rc:
            raise ITDError(rc, "itd_dev_alloc(%d bytes, device %d)" % (nbytes, device))
        self.ptr = p.value

    def upload(self, a, offset=0):
        a = np.ascontiguousarray(a)
        if offset < 0 or offset + a.nbytes > self.nbytes:
            raise ValueError("upload of %d bytes at offset %d into a buffer of %d" % (a.nbytes, offset, self.nbytes))
        rc = self._L.itd_dev_copy(self.device, self.ptr + offset, _np_ptr(a), a.nbytes, 1)
        if rc:
            raise ITDError(rc, "itd_dev_copy(host -> device)")

    def download(self, out, offset=0):
        if not out.flags["C_CONTIGUOUS"] or offset < 0 or offset + out.nbytes > self.nbytes:
            raise ValueError("download of %d bytes at offset %d from a buffer of %d (or a non-contiguous target)" % (out.nbytes, offset, self.nbytes))
        rc = self._L.itd_dev_copy(self.device, _np_ptr(out), self.ptr + offset, out.nbytes, 0)
        if rc:
            raise ITDError(rc, "itd_dev_copy(device -> host)")
        return out

    def free(self):
        if getattr(self, "ptr", None):
            self._L.itd_dev_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class WaveBounds:
    """The handle of the many-row bounds call (itd_bounds_* in include/pyitd_hip.h): a stream and a workspace of its own, apart from
    every Engine, so that nothing another operator does can reach the call's result."""

    def __init__(self, device=0):
        self._L = _lib.load()
        h = ctypes.c_void_p()
        rc = self._L.itd_bounds_create(ctypes.byref(h), int(device))
        if rc:
            raise ITDError(rc, "itd_bounds_create(device=%d)" % device)
        self._h, self.device = h, int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._L.itd_bounds_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def batch_dev(self, hist_ptr, rows, hist_stride, T, t0, t1, abins, lbins, aedges_ptr, aedges_stride, ledges_ptr, ledges_stride,
                  quant_ptr, quant_stride, bounds_ptr, bounds_stride=4, total_ptr=None, stream=None):
        """The wave filter's bounds (amp_lo, amp_hi, len_lo, len_hi), float64 at bounds_stride per row, from the quantiles of the time
        bins [t0, t1) of every row's int32 histogram [T, abins, lbins] (hist_stride elements apart); edges and the eight float64
        parameters in device memory, a stride of 0: one set for every row; total int64 [rows] (optional).  Pointers in, nothing
        copied, nothing awaited; stream None: the handle's own."""
        rc = self._L.itd_wave_bounds_batch(self._h, hist_ptr, rows, hist_stride, T, t0, t1, abins, lbins, aedges_ptr, aedges_stride,
                                           ledges_ptr, ledges_stride, quant_ptr, quant_stride, bounds_ptr, bounds_stride, total_ptr, stream)
        if rc:
            raise ITDError(rc, self._L.itd_bounds_last_error(self._h).decode())
