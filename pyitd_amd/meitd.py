"""Host-side mirror of MEITD.py's selection drivers, on top of the GPU operators:

  weighted_permutation_entropy(time_series, order=3, normalize=False)   MEITD.py:79-128   (orders 2 .. 5)
  retrieve_proper_rotation(x, WPEMAX)                                    MEITD.py:344-368
  determine_if_first_is_proper_rotation(x, WPEMAX)                       MEITD.py:371-392
  MEITD(data, max_iteration=40, WPEMAX=0.6) -> (high, low, residual)     MEITD.py:395-534
  XITD(data)                                                             MEITD.py:536-549

The drivers are control logic around three operators, all of which run on the GPU on arrays that STAY on the GPU for the whole
loop (include/pyitd_hip.h, "MEITD's operators on device-resident signals"): the cubic-spline baseline extraction (MEITD.py:303-338
-> itd_baseline_extract_spline2_f64), the extrema count (matlab_detect_peaks(x).size + matlab_detect_peaks(-x).size ->
itd_count_knots_f64) and the entropy's pass over the samples (itd_wpe3_f64: six weighted sums, taken in the reference's order).
Per pass a few scalars come back — the counts, the six sums — and the threshold tests are drawn from them here; the signal is
uploaded once and the components are downloaded once.

Upstream quirks kept: `max_iteration` is never used by MEITD (:395); XITD passes its WPEMAX estimate in that position (:541), so
MEITD runs with WPEMAX = 0.6 there (the estimate itself, :538-540, has no consumer and is not computed); nothing is printed.
One piece of upstream's work is NOT repeated because nothing can observe it: when the entropy test of retrieve_proper_rotation
fails, its loop (:359-366) keeps extracting down to fewer than 6 extrema and then returns its INPUT (:368) — on the golden signals
that is 209-249 of the ~290 extractions of a MEITD call.
"""
import threading
from math import factorial

import numpy

from .engine import DeviceBuffer
from .spline import _eng


def _entropy_from_bins(weights, windows, order=3, normalize=False):
    """MEITD.py:119-128 from the patterns' weighted counts (in numpy.unique's order; a pattern without windows is absent).  The same
    numpy operations on the same (short) arrays as upstream: the result's bits depend on numpy's summation order and its log2."""
    wc = weights[windows > 0]
    p = numpy.true_divide(wc, wc.sum())
    pe = -numpy.multiply(p, numpy.log2(p)).sum()
    if normalize:
        pe /= numpy.log2(factorial(order))
    return pe


def weighted_permutation_entropy(time_series, order=3, normalize=False, device=0):
    """MEITD.py:79-128: permutation patterns of the embedded series, each window weighted by its variance.  The pass over the samples
    runs on the GPU (order 3, the only one MEITD.py itself uses: itd_wpe3_f64; orders 2, 4, 5: itd_wpe_f64); the entropy is drawn
    here from the patterns' weighted counts.  Orders above 5 are refused (order^order hash values: the operator is not built for
    them)."""
    x = numpy.ascontiguousarray(numpy.array(time_series), dtype=numpy.float64)
    if x.ndim != 1 or not 2 <= int(order) <= 5 or len(x) < int(order):
        raise ValueError("weighted_permutation_entropy: a 1-D series of at least `order` samples, order 2 .. 5")
    buf = DeviceBuffer(x.nbytes, device)
    try:
        buf.upload(x)
        eng = _eng(len(x), device)
        w, c = eng.wpe3_dev(buf.ptr, len(x)) if int(order) == 3 else eng.wpe_dev(buf.ptr, len(x), int(order))
    finally:
        buf.free()
    return _entropy_from_bins(w, c, int(order), normalize)


_ROWS_KEPT = 22          # MEITD returns once more than 20 components are kept (:414-415): 21 rows at most, in either list


class _Work:
    """The device arrays of one MEITD run — rows of n float64 in one allocation: four working rows that change roles by
    renaming (no copies), the two lists of kept rotations."""

    def __init__(self, n, device, solver="auto"):
        self.n, self.device, self.solver = n, device, solver
        self.eng = _eng(n, device, solver)
        self.buf = DeviceBuffer((6 + 2 * _ROWS_KEPT) * n * 8, device)
        self.free_rows = [self.row(i) for i in range(6)]
        self.high0, self.low0 = self.row(6), self.row(6 + _ROWS_KEPT)
        # the whole loop as one launch: where an extraction of this signal is the one-workgroup parallel-in-knots operator anyway
        self.one_launch = _one_launch(n, solver)
        self.last = {}

    def row(self, i):
        return self.buf.ptr + i * self.n * 8

    def kept(self, first, k):
        return first + k * self.n * 8

    def take(self):
        return self.free_rows.pop()

    def give(self, p):
        self.free_rows.append(p)

    # ---- the operators -------------------------------------------------------------------------------------------------------
    def upload(self, x, dst):
        self.eng.copy(dst, x.ctypes.data, x.nbytes, 1, wait=True)

    def download(self, src, rows=1):
        out = numpy.empty((rows, self.n))
        self.eng.copy(out.ctypes.data, src, out.nbytes, 0, wait=True)
        return out

    def assign(self, dst, src):
        self.eng.copy(dst, src, self.n * 8, 2)

    def zero(self, dst):
        self.eng.copy(dst, None, self.n * 8, 3)

    def probe(self, src):
        """(normalised entropy, extrema count) of a row: MEITD.py:346-351 / :373-378."""
        w, c, count = self.eng.wpe3_dev(src, self.n, want_knots=True)
        return numpy.mean(_entropy_from_bins(w, c, 3, True)), count

    def count(self, src):
        return self.eng.count_knots_dev(src, self.n)

    def entropy(self, src):
        """weighted_permutation_entropy(row, order=3, normalize=True)"""
        return _entropy_from_bins(*self.eng.wpe3_dev(src, self.n), 3, True)

    def subtract(self, a, b, out):
        self.eng.subtract_dev(a, b, out, self.n)

    def reset(self):
        """every working row is free again (a call that raised may have left some taken)"""
        self.free_rows = [self.row(i) for i in range(6)]

    def extract(self, src, base, rot=None, want_baseline_count=False):
        """itd_baseline_extract (MEITD.py:303-338): src -> (rot, base); with the extrema count of the produced baseline."""
        r = self.eng.spline_extract_dev(src, self.n, base, rot, 0, want_baseline_knots=want_baseline_count)
        knots = r[0] if want_baseline_count else r
        if knots < 2:
            raise TypeError("m > k must hold")        # what scipy.interpolate.splrep raises for fewer than 4 data sites
        return r[1] if want_baseline_count else None


_work = {}
_CACHE_MAX_BYTES = 64 << 20        # device rows kept between calls per device (50 rows x n x 8 B): larger ones are freed when the call returns
_lock = threading.RLock()          # the module-level API keeps one set of device rows per device: calls are serialised


def _work_for(n, device, solver="auto"):
    key = int(device)
    w = _work.get(key)
    if w is None or w.n != n or w.solver != solver or w.eng is not _eng(n, device, solver):
        if w is not None:
            w.buf.free()
        w = _work[key] = _Work(n, device, solver)
    w.eng.set_spline_solver({"auto": 0, "serial": 1, "parallel": 2}[solver])
    w.reset()
    return w


def release(device=None):
    """Free the device rows this module keeps between calls (all devices, or one)."""
    with _lock:
        for key in [k for k in _work if device is None or k == int(device)]:
            _work.pop(key).buf.free()
        for key in [k for k in _batch_rows if device is None or k == int(device)]:
            _batch_rows.pop(key).free()


def _done(w):
    """after a call: rows of a long signal do not stay allocated (a 2^24-sample call holds 6.7 GB)"""
    if isinstance(w, _Work) and (6 + 2 * _ROWS_KEPT) * w.n * 8 > _CACHE_MAX_BYTES:
        release(w.device)


def _proper(wpe, WPEMAX):
    return wpe < WPEMAX and not wpe < 0.2             # MEITD.py:364 / :387


def _retrieve(wk, rot, WPEMAX):
    """retrieve_proper_rotation on the row `rot`: returns (row holding the result, proper)."""
    wpe, count = wk.probe(rot)
    if count > 5 and _proper(wpe, WPEMAX):            # the first extraction is the answer (:360-365)
        base, out = wk.take(), wk.take()
        wk.extract(rot, base, out)
        wk.give(base)
        wk.give(rot)
        return out, 1
    return rot, 0                                     # "I can't retrieve a proper rotation" / the loop that returns its input


def _determine(wk, src, rot, base, WPEMAX, probed=None):
    """determine_if_first_is_proper_rotation(src) into the rows rot / base (base None: not wanted).  Returns proper."""
    wpe, count = probed if probed is not None else wk.probe(src)
    if count < 5:
        wk.assign(rot, src)
        if base is not None:
            wk.zero(base)
        return 0
    tmp = base if base is not None else wk.take()
    wk.extract(src, tmp, rot)
    if base is None:
        wk.give(tmp)
    return 1 if _proper(wpe, WPEMAX) else 0


def retrieve_proper_rotation(x, WPEMAX, device=0, solver="auto"):
    """MEITD.py:344-368 — the first extraction's rotation if the entropy of the INPUT passes the test, else the input."""
    x = numpy.ascontiguousarray(numpy.asarray(x).astype(dtype=numpy.float64))
    with _lock:
        wk = _work_for(len(x), device, solver)
        rot = wk.take()
        wk.upload(x, rot)
        rot, proper = _retrieve(wk, rot, WPEMAX)
        out = wk.download(rot)[0] if proper else x
        wk.give(rot)
        _done(wk)
    return out, proper


def determine_if_first_is_proper_rotation(x, WPEMAX, device=0, solver="auto"):
    """MEITD.py:371-392 — one extraction; proper if the input's entropy lies in [0.2, WPEMAX)."""
    x = numpy.ascontiguousarray(numpy.asarray(x).astype(dtype=numpy.float64))
    with _lock:
        wk = _work_for(len(x), device, solver)
        src, rot, base = wk.take(), wk.take(), wk.take()
        wk.upload(x, src)
        proper = _determine(wk, src, rot, base, WPEMAX)
        r, b = wk.download(rot)[0], wk.download(base)[0]
        for p in (src, rot, base):
            wk.give(p)
        _done(wk)
    return r, b, proper


_ONE_LAUNCH_MAX = 8192      # itd_meitd_small_f64: one workgroup holds the signal's run


def _one_launch(n, solver):
    """Whether MEITD's selection loop on a signal of n samples runs as one launch: where every extraction of the host-driven loop
    would be the one-workgroup parallel-in-knots operator anyway (csrc/itd_policy.hpp: meitd_one_launch, which the engine's entries
    apply; tests/test_policy_host.py holds the two equal)."""
    return 3 <= n <= _ONE_LAUNCH_MAX and (solver == "parallel" or (solver == "auto" and n >= 1024))


def _proper_rows(log, WPEMAX):
    """the threshold test of every logged probe, from entropies re-drawn with the reference's numpy expression (_entropy_from_bins)"""
    full = (log["c"] > 0).all(axis=1)
    wpe = numpy.empty(len(log))
    if full.any():                    # (all six patterns present: the same numpy operations row by row, in one call)
        w = log["w"][full]
        p = numpy.true_divide(w, w.sum(axis=1)[:, None])
        pe = -numpy.multiply(p, numpy.log2(p)).sum(axis=1)
        pe /= numpy.log2(factorial(3))
        wpe[full] = pe
    for i in numpy.flatnonzero(~full):
        wpe[i] = _entropy_from_bins(log["w"][i], log["c"][i], 3, True)
    return (wpe < WPEMAX) & ~(wpe < 0.2)


def _meitd_one_launch(wk, data, WPEMAX):
    """The loop as ONE launch (include/pyitd_hip.h: itd_meitd_small_f64; csrc/itd_meitd.hpp).  Returns "host" when the device did not
    deliver — a NaN, an extraction scipy would refuse, a threshold test that numpy's log2 and the device's draw differently: the
    host-driven loop below then runs the call and reproduces the reference's behaviour —, else what _meitd returns."""
    wk.upload(data, wk.row(5))
    res, log = wk.eng.meitd_small_dev(wk.buf.ptr, wk.n, WPEMAX)
    status = int(res[0])
    wk.last = {"one_launch": True, "status": status, "probes": int(res[4]), "extractions": int(res[5]), "turns": int(res[6]),
               "us": {k: int(v) / 100.0 for k, v in zip(("probes", "extractions", "counts", "copies", "probe_sums", "probe_entropy", "", "", "x_knots", "x_values", "x_rows", "x_forward",
                                                         "x_backward", "x_eval"), res[8:22]) if k}}
    if status >= 2:
        return "host"
    if len(log):
        wd = log["wpe"]
        if not numpy.array_equal(_proper_rows(log, WPEMAX), (wd < WPEMAX) & ~(wd < 0.2)):
            wk.last["status"] = -1
            return "host"
    if status == 1:
        return None
    x = wk.row(int(res[3]))
    wk.free_rows.remove(x)
    return int(res[1]), int(res[2]), x


def _meitd(wk, data, WPEMAX):
    """MEITD.py:395-534 on device rows.  Returns (n_high, n_low, row of the residual) or None for the early return of :411-413."""
    if getattr(wk, "one_launch", False):
        r = _meitd_one_launch(wk, data, WPEMAX)
        if not isinstance(r, str):
            return r
        wk.reset()
    x, rotation, baseline = wk.take(), wk.take(), wk.take()
    wk.upload(data, x)
    n_high = n_low = 0
    probed = wk.probe(x)
    proper = _determine(wk, x, rotation, baseline, WPEMAX, probed)
    changed, on_signal, digs = False, True, 1           # xchanged, HILO == 1, soft_reset
    count = probed[1]
    if count < 4:
        for p in (x, rotation, baseline):
            wk.give(p)
        return None
    while count > 5:
        if n_high + n_low > 20:
            break
        if proper == 0:      # not proper yet, but decomposable: go down its own baselines
            rotation, proper = _retrieve(wk, rotation, WPEMAX)
        if proper == 1:
            if on_signal:
                wk.assign(wk.kept(wk.high0, n_high), rotation)
                n_high += 1
            else:
                wk.assign(wk.kept(wk.low0, n_low), rotation)
                n_low += 1
            digs = 0
            wk.subtract(x, rotation, x)
            changed = True
        if changed and on_signal:
            count = wk.count(x)
            if count < 5:
                continue
            wk.extract(x, baseline)
            proper = _determine(wk, baseline, rotation, None, WPEMAX)
            changed, on_signal = False, False
            continue
        elif on_signal:
            proper = _determine(wk, baseline, rotation, None, WPEMAX)
            on_signal = False
            continue
        if changed and not on_signal:
            probed = wk.probe(x)
            count = probed[1]
            if count < 5:
                continue
            proper = _determine(wk, x, rotation, baseline, WPEMAX, probed)
            changed, on_signal = False, True
            continue
        if not changed and not on_signal:
            if digs == 0:
                wk.extract(x, baseline, rotation)
                digs = 1
            count = wk.count(baseline)
            if count < 5:
                continue
            for _ in range(digs):
                deeper = wk.take()
                count = wk.extract(baseline, deeper, rotation, want_baseline_count=True)
                wk.give(baseline)
                baseline = deeper
                if count < 5:
                    break
            digs += 1
            continue
    wk.give(rotation)
    wk.give(baseline)
    return n_high, n_low, x


def MEITD(data, max_iteration=40, WPEMAX=0.6, device=0, solver="auto"):
    """MEITD.py:395-534 — alternate between peeling a proper rotation off the signal (the "high" list) and off its baseline
    (the "low" list); dig further down the baselines when neither succeeds.  Returns (high[h, N], low[l, N], residual[N]).

    solver: how the spline baselines are solved (pyitd_amd.spline._eng).  "auto" (default) takes the parallel-in-knots form for signals
    of >= 1024 samples: baselines and entropies then equal scipy's / the reference's to rounding (~1e-14 of the signal's scale), not bit
    for bit — and the driver's decisions are hard thresholds on them (extrema counts of nearly flat baselines against 5, entropies
    against 0.2 / WPEMAX): a signal that sits on a threshold may select different components than MEITD.py.  "serial" (FITPACK's own
    sweep, bit-level against scipy) removes that difference at one GPU thread per extraction.  The module keeps one set of device rows
    per device between calls (freed above 64 MB; `release()`); calls are serialised by a lock."""
    data = numpy.ascontiguousarray(numpy.asarray(data).astype(dtype=numpy.float64))
    with _lock:
        wk = _work_for(len(data), device, solver)
        r = _meitd(wk, data, WPEMAX)
        if r is None:
            zero = numpy.zeros(len(data))
            return zero, zero, data
        n_high, n_low, x = r
        high = wk.download(wk.high0, n_high) if n_high else numpy.zeros((0, len(data)))
        low = wk.download(wk.low0, n_low) if n_low else numpy.zeros((0, len(data)))
        residual = wk.download(x)[0]
        wk.give(x)
        _done(wk)
    return high, low, residual


def _xitd_early(data, device):
    """XITD of a signal with fewer than 4 extrema (MEITD.py:411-413): zeros, zeros and the data, ordered by their entropy"""
    zero = numpy.zeros(len(data))
    rotations = numpy.vstack((numpy.vstack((zero, zero)), data))
    ent = [weighted_permutation_entropy(rotations[i, :], order=3, normalize=True, device=device) for i in range(3)]
    return rotations[numpy.argsort(ent), :]


def XITD(data, device=0, solver="auto"):
    """MEITD.py:536-549 — MEITD's components and residual, ordered by their entropy (taken on the device rows).  solver: see MEITD."""
    data = numpy.ascontiguousarray(numpy.asarray(data).astype(dtype=numpy.float64))
    with _lock:
        wk = _work_for(len(data), device, solver)
        r = _meitd(wk, data, 0.6)                        # upstream passes its WPEMAX estimate where max_iteration goes (:541)
        if r is None:
            return _xitd_early(data, device)
        n_high, n_low, x = r
        rows = [wk.kept(wk.high0, k) for k in range(n_high)] + [wk.kept(wk.low0, k) for k in range(n_low)] + [x]
        ent = [wk.entropy(p) for p in rows]
        out = numpy.empty((len(rows), wk.n))
        for k, i in enumerate(numpy.argsort(ent)):
            out[k] = wk.download(rows[i])[0]
        wk.give(x)
        _done(wk)
    return out


# ---- many short signals of one length: MEITD_batch / XITD_batch ------------------------------------------------------------------
_batch_rows = {}                   # device -> DeviceBuffer of a batch's rows, kept between calls up to _CACHE_MAX_BYTES
_BATCH_BYTES = 1 << 30             # the default chunk keeps a launch's device memory (rows and the engine's scratch) at about this many bytes
_GRID_MAX = 65535                  # signals per launch of itd_meitd_batch_f64
last_batch = {}                    # the last MEITD_batch / XITD_batch: launches, status counts, signals handed back, ...


def _batch_bytes(n):
    """device bytes per signal of a batch: its (6 + 2 * 22) rows of n float64, and its share of itd_meitd_batch_f64's workspace —
    knot indices and six solver arrays of n + 2, the signal's staging copy, XITD's sums, the result, and its probe log twice (1024
    entries of 88 bytes: the kernel's log and the packed copy that goes to the host), with room for alignment"""
    return (6 + 2 * _ROWS_KEPT) * n * 8 + 4 * (n + 2) + 6 * 8 * (n + 2) + 8 * n + _ROWS_KEPT * 6 * 16 + 96 + 2 * 1024 * 88 + 1024


def _batch_chunk(n):
    """signals per chunk by default: about _BATCH_BYTES of device memory in all (>= 271 signals for n <= 8192)"""
    return max(1, min(_GRID_MAX, _BATCH_BYTES // _batch_bytes(n)))


def _batch_buffer(nbytes, device):
    key = int(device)
    buf = _batch_rows.get(key)
    if buf is None or buf.nbytes < nbytes:
        if buf is not None:
            _batch_rows.pop(key).free()
        buf = _batch_rows[key] = DeviceBuffer(nbytes, device)
    return buf


def _batch(data, WPEMAX, device, solver, chunk, xitd):
    global last_batch
    what = "XITD_batch" if xitd else "MEITD_batch"
    arr = numpy.asarray(data)
    if arr.ndim != 2 or arr.shape[1] < 3:
        raise ValueError("%s: data must be 2-D [B, N] with N >= 3 (got shape %s)" % (what, arr.shape))
    if chunk is not None and int(chunk) < 1:
        raise ValueError("%s: chunk must be at least 1" % what)
    arr = numpy.ascontiguousarray(arr.astype(dtype=numpy.float64))
    B, n = arr.shape
    wpemax = 0.6 if xitd else WPEMAX               # (XITD runs MEITD with WPEMAX = 0.6: see XITD)

    def single(x):
        return XITD(x, device=device, solver=solver) if xitd else MEITD(x, WPEMAX=WPEMAX, device=device, solver=solver)

    stats = last_batch = {"signals": B, "launches": 0, "chunks": 0, "status": {}, "handed_back": 0, "looped": 0}
    with _lock:
        if not _one_launch(n, solver):
            stats["looped"] = B                    # no one-launch form for this length / solver: the single-signal path, one by one
            return [single(x) for x in arr]
        per = (6 + 2 * _ROWS_KEPT) * n             # elements of one signal's rows
        c = min(B, int(chunk) if chunk is not None else _batch_chunk(n))
        buf = _batch_buffer(c * per * 8, device)
        out = []
        try:
            for c0 in range(0, B, c):
                xs = arr[c0:c0 + c]
                m = len(xs)
                # (the engine is shared: a single-signal call of the chunk before — a fallback, XITD's entropies of a signal with
                # fewer than 4 extrema — may have set its solver to something else)
                eng = _eng(n, device, solver)
                res, logs, xw, xc = eng.meitd_batch_dev(buf.ptr, n, m, per, wpemax, x=xs, xitd=xitd)
                stats["chunks"] += 1
                stats["launches"] += (m + _GRID_MAX - 1) // _GRID_MAX
                status = res[:, 0]
                for v, k in zip(*numpy.unique(status, return_counts=True)):
                    stats["status"][int(v)] = stats["status"].get(int(v), 0) + int(k)
                # the logged threshold tests of every delivered signal, re-drawn with numpy in one call (as _meitd_one_launch)
                ok = numpy.flatnonzero(status == 0)
                if len(ok):
                    probes = res[ok, 4].astype(numpy.int64)
                    log = numpy.concatenate([logs[b, :p] for b, p in zip(ok, probes)])
                    wd = log["wpe"]
                    agree = _proper_rows(log, wpemax) == ((wd < wpemax) & ~(wd < 0.2))
                    ok = numpy.setdiff1d(ok, numpy.repeat(ok, probes)[~agree])
                # one table of the delivered signals' rows (XITD: in the order of their entropies), one gather, one download
                tab, spans = [], {}
                for b in ok:
                    nh, nl, xr = (int(v) for v in res[b, 1:4])
                    base = int(b) * per
                    rows = [base + (6 + k) * n for k in range(nh)] + [base + (6 + _ROWS_KEPT + k) * n for k in range(nl)] + [base + xr * n]
                    if xitd:
                        ent = [_entropy_from_bins(xw[b, k], xc[b, k], 3, True) for k in range(len(rows))]
                        rows = [rows[i] for i in numpy.argsort(ent)]
                    spans[int(b)] = (len(tab), nh, nl)
                    tab += rows
                got = numpy.empty((len(tab), n))
                if tab:
                    dst = DeviceBuffer(got.nbytes, device)
                    try:
                        eng.gather_rows_dev(buf.ptr, m * per, tab, n, dst.ptr, out=got)
                    finally:
                        dst.free()
                for b in range(m):
                    if b in spans:
                        r0, nh, nl = spans[b]
                        out.append(got[r0:r0 + nh + nl + 1] if xitd else (got[r0:r0 + nh], got[r0 + nh:r0 + nh + nl], got[r0 + nh + nl]))
                    elif status[b] == 1:               # fewer than 4 extrema (MEITD.py:411-413)
                        x = xs[b].copy()
                        zero = numpy.zeros(n)
                        out.append(_xitd_early(x, device) if xitd else (zero, zero, x))
                    else:                              # not delivered, or a threshold test numpy draws otherwise: the single-signal path
                        stats["handed_back"] += 1
                        out.append(single(xs[b]))
        finally:
            if buf.nbytes > _CACHE_MAX_BYTES:
                _batch_rows.pop(int(device)).free()
    return out


def MEITD_batch(data, max_iteration=40, WPEMAX=0.6, device=0, solver="auto", chunk=None):
    """[MEITD(x, max_iteration, WPEMAX) for x in data] for data[B, N], bit for bit — the same components, the same exception for the
    first signal that raises — with the loop of every signal in one launch, one workgroup (one CU) per signal
    (include/pyitd_hip.h: itd_meitd_batch_f64).  A signal the launch does not deliver (a NaN, an extraction scipy would refuse, a
    threshold test that numpy's log2 draws otherwise) goes through MEITD on its own; the rest keep the launch's result.  Only where
    MEITD itself takes the one-launch form: N <= 8192 and solver "parallel", or "auto" with N >= 1024.  Other lengths / solvers loop
    over MEITD signal by signal: correct, not faster.  chunk: signals per launch (default: about 1 GiB of device memory, at least 256
    signals for N <= 8192); the results do not depend on it.  `last_batch` describes the call."""
    return _batch(data, WPEMAX, device, solver, chunk, False)


def XITD_batch(data, device=0, solver="auto", chunk=None):
    """[XITD(x) for x in data] for data[B, N], bit for bit: MEITD_batch's launch, which also returns the six entropy sums of every
    kept row and the residual; the entropies are drawn and ordered here as XITD draws them.  See MEITD_batch."""
    return _batch(data, 0.6, device, solver, chunk, True)
