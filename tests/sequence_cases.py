"""The registry of cells of the order tests (tests/test_sequences_cpu.py, tests/test_gpu_sequences.py, tools/sequence_fuzz.py).

Every Python call on a device runs in one process-wide engine (pyitd_amd.itd._engine_for) whose workspaces only grow and are shared by
all operators ("Order of calls").  A cell is one operator family as a caller reaches it on that engine:

    name       the cell's name
    entries    the C entries of include/pyitd_hip.h it calls
    buffers    the engine's buffers it touches, read off itd_engine.hip / itd_engine_batch.inc / itd_fourier.inc
    decided_by the kernel that settles that its result is the same bits from run to run (no floating-point atomics, no reduction whose
               order depends on scheduling): every cell here is compared with a fresh engine bit for bit, BY_RULE is empty
    make(size, seed)   its inputs (a dict of numpy arrays; finite, and inside the operator's working branch)
    run(P, inputs)     the calls, on the process engine, through pyitd_amd (P) or the C entries on that engine: a tuple of numpy arrays
    reference(inputs)  the reference's own result in the shape of run()'s (for a CPU model of the GPU result: the model's output)
    check(inputs, got) got held to the reference the operator's own test file uses, with that file's comparison rule (imported,
                       never restated)

Sizes: S  n = 1030 (three tiles, the last of 6 samples), 2 rows;  L  n = 2 * 512 + 514 = 1538 for the half-wave family and
5 * 512 + 77 = 2637 elsewhere, 7 rows;  G  n = 20011, 3 rows (only where an arena or the Python engine has to be re-created).
The carve offsets of every arena (knot_workspace, nak_small_ws, the tile records) follow n and the row count, so they differ between
any two of the sizes.
"""
import ctypes
import functools
import importlib

import numpy as np

import batch_cases as bc
import cascade_ref as cr
import fft_cases as fc
import spectrum_ref as sr
import wave_hist_ref
import waves_ref
from helpers import DevArrays, assert_bits_equal, fuzz_signal
from oracle import cpu_oracle, exact_spline as ex, exact_tfe as et, iq_oracle, meitd_oracle, spline_oracle as so
from test_oracle_exact_tfe import family

SENT = -7.25e300
ISENT = -123456
PAD = 7
OK, INVALID, NONFINITE = 0, 1, 6
M = 5                               # max_iteration of every decomposition cell
SIZES = {"S": {"n": 1030, "n_hw": 1030, "rows": 2},
         "L": {"n": 5 * 512 + 77, "n_hw": 2 * 512 + 514, "rows": 7},
         "G": {"n": 20011, "n_hw": 20011, "rows": 3}}
LONG_N = 1 << 18                    # the repository's smallest size that keeps the fused levels busy (test (e)'s long cell)


# ---- the comparison rules of the operators' own test files (imported where they are used: those modules are GPU test modules) ----
def _bits(a, b, what):
    assert_bits_equal(np.asarray(a), np.asarray(b), what)


def _same(a, b, what):
    """Equal arrays of any type, bit for bit (any NaN = any NaN for floats)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s%s against %s%s" % (what, a.dtype, a.shape, b.dtype, b.shape)
    if a.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        ok = (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))
    else:
        ok = a == b
    assert ok.all(), "%s: %d of %d entries differ, first at %s" % (what, (~ok).sum(), ok.size, np.argwhere(~ok)[0])


def same_results(got, want, what):
    """What "equals fresh" means: the same number of arrays, each the same type, shape and bits."""
    assert len(got) == len(want), "%s: %d arrays against %d" % (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, "%s: output %d" % (what, i))


def spline_check(what, r, got, x, ref_fp64):
    """oracle/exact_spline with the 4 ref + 64 eps S bound (tests/test_gpu_spline_exact.py)."""
    from test_gpu_spline_exact import _check
    return _check(what, r, got, x, ref_fp64)


def tfe_check(x, a, p, f, what):
    """oracle/exact_tfe with the bounds of tests/test_gpu_instantaneous_exact.py."""
    from test_gpu_instantaneous_exact import check
    check(x, a, p, f, what=what)


def close_1e12(got, ref, what):
    from test_gpu_spline import _close
    _close(got, ref, what)


def close_meitd(got, ref, what):
    from test_gpu_meitd_batch import _close
    _close(got, ref, what)


# ---- signals ---------------------------------------------------------------------------------------------------------------------
KINDS = ("noise", "seams", "quantised", "sine", "fam_quantised", "fam_noise", "quantised")


def one_signal(kind, n, rng):
    """The seam, quantised and noise families of helpers.fuzz_signal and test_oracle_exact_tfe.family (and a sine in noise)."""
    if kind == "noise":
        return fuzz_signal(rng, 0, n)
    if kind == "quantised":
        return fuzz_signal(rng, 2, n)
    if kind == "sine":
        return fuzz_signal(rng, 4, n)
    if kind == "seams":
        return family("seams", n) * (1.0 + rng.integers(0, 3))
    if kind == "fam_quantised":
        return family("quantised", n)
    if kind == "fam_noise":
        return family("noise", n) * 2.0 ** int(rng.integers(-3, 4))
    raise KeyError(kind)


def signals(n, rows, seed, kinds=KINDS):
    rng = np.random.default_rng([seed, n, rows])
    x = np.stack([one_signal(kinds[r % len(kinds)], n, rng) for r in range(rows)])
    assert np.isfinite(x).all()
    return x


def smooth_kinds():
    """For the spline operators: every row keeps at least ten knots and no long plateau."""
    return ("noise", "seams", "sine", "fam_noise")


def scaled_rows(base, rows):
    """rows signals of which only the first two differ: row r = c_r * base[r % 2] with c_r a signed power of two, so that every
    operator that is homogeneous in the signal has the exact result c_r * (that of the base row) and two exact references serve
    all rows.  Returns (x[rows, n], factors[rows], source[rows])."""
    factors = np.array([1.0, 1.0, -0.5, 2.0, 4.0, -1.0, 0.25, -8.0])[:rows]
    src = np.arange(rows) % 2
    return base[src] * factors[:, None], factors, src


def mod(name):
    """A submodule of pyitd_amd (pyitd_amd.itd the module, not the function of that name)."""
    return importlib.import_module("pyitd_amd." + name)


def eng_of(P, n):
    """The process-wide engine every Python call on device 0 runs in."""
    return mod("itd")._engine_for(n)


def spline_eng(P, n, solver):
    return mod("spline")._eng(n, 0, solver)


def _i64(v=0):
    return ctypes.c_int64(v)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Cell:
    entries = ()
    buffers = ()
    decided_by = ""
    halfwave = False            # the half-wave family takes n_hw of a size
    model = False               # the reference is a CPU model of the GPU result (a composition, a port): reference() is its output
    stream_form = False         # has a device form that does not synchronise: enqueue(eng, d, inputs, stream) / collect(eng, d, inputs)

    @property
    def name(self):
        return type(self).__name__

    def dims(self, size):
        s = SIZES[size]
        return (s["n_hw"] if self.halfwave else s["n"]), s["rows"]

    def inputs(self, size):
        return _inputs(self.name, size)

    def run(self, P, inp):
        raise NotImplementedError

    def reference(self, inp):
        raise NotImplementedError

    def check(self, inp, got, P=None):
        raise NotImplementedError

    def reaches_working_branch(self, inp):
        """The oracle's statement that the input is inside the operator's working branch."""
        return True


class DevCell(Cell):
    """A cell whose calls are enqueued on a stream without a host synchronisation."""
    stream_form = True
    staged = ()                 # the arrays of arrays() that are inputs (test (e) fills them by copies on the caller's stream)

    def arrays(self, inp):
        raise NotImplementedError

    def enqueue(self, eng, d, inp, stream):
        raise NotImplementedError

    def collect(self, eng, d, inp):
        raise NotImplementedError

    def run(self, P, inp):
        eng = eng_of(P, inp["n"])
        d = DevArrays(eng, **self.arrays(inp))
        try:
            self.enqueue(eng, d, inp, None)
            return self.collect(eng, d, inp)
        finally:
            d.free()


@functools.lru_cache(maxsize=None)
def _inputs(name, size):
    cell = CELLS[name]
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 9973
    inp = cell.make(size, seed)
    inp["size"] = size
    for v in inp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    inp["_memo"] = {}
    return inp


def memo(inp, key, f):
    """A reference computed once per cell and size and left unchanged."""
    m = inp["_memo"]
    if key not in m:
        m[key] = f()
    return m[key]


def pad_rows(rows, pad=PAD, sent=SENT):
    """rows flattened with `pad` sentinels behind them: an output buffer as the device forms are given it."""
    return np.full(int(np.prod(rows)) + pad, sent)


def pad_ok(buf, used, sent=SENT):
    return bool(np.all(buf[used:] == sent))


# ================================================================================================================================
# the decomposition
# ================================================================================================================================
def _dec_ref(inp, key="x"):
    return memo(inp, "dec_" + key, lambda: cpu_oracle.itd(inp[key], M))


def _kc_pad(kc, x):
    """knot_counts as the engine reports them: [0] the signal's own knots, [j >= 1] what the reference prints (ITD.py:403), -1 behind."""
    out = np.full(23, -1, np.int64)
    out[0] = len(cpu_oracle.knots(np.asarray(x, dtype=np.float64)))
    out[1: 1 + len(kc)] = kc
    return out


def _kc_lenient(got, ref, at):
    """got with its knot_counts (the outputs `at`) cut to what the operator's own test compares (tests/test_gpu_parity.py: entry 0 and
    the entries the reference prints; what the engine reports behind them is not the reference's to say)."""
    got = list(got)
    for k in at:
        g, r = got[k].copy(), ref[k]
        keep = r >= 0
        g[~keep] = -1
        got[k] = g
    return tuple(got)


def _select_ref(rows, select):
    """The rows a selection delivers: rotation r's slot holds rows[r] if r <= n_rows - 2, else zeros; the residual's slot rows[-1]."""
    n_rows = rows.shape[0]
    out = []
    for r in select:
        out.append(rows[-1] if r == -1 else (rows[r] if r <= n_rows - 2 else np.zeros(rows.shape[1])))
    return np.stack(out)


SELECT = [0, 2, -1]


class DecMake:
    def make(self, size, seed):
        n, _ = self.dims(size)
        x = signals(n, 2, seed, ("noise", "quantised"))[0 if size != "L" else 1]
        if size == "L":
            x = x + fuzz_signal(np.random.default_rng(seed), 4, n)      # quantised steps on a tone: plateaus and many levels
        return {"n": n, "x": x, "x32": x.astype(np.float32)}

    def reaches_working_branch(self, inp):
        return len(cpu_oracle.knots(inp["x"])) > 10 and _dec_ref(inp)["rows"].shape[0] >= 3


DEC_BUFFERS = ("d_io_x", "d_io_rows", "d_io_bases", "h_pin", "d_pp", "d_counts", "d_recs", "d_gsum", "d_state", "h_state")


class decompose_host(DecMake, Cell):
    """ITD().itd of a float64 and of a float32 signal, the baselines kept on the device and fetched afterwards."""
    entries = ("itd_decompose_host_f64", "itd_decompose_host_f32", "itd_set_host_keep_baselines", "itd_get_last_baselines_host")
    buffers = DEC_BUFFERS
    decided_by = "k_resident / k_extract: every sample one thread, integer atomics on the knot totals only"

    def run(self, P, inp):
        out = []
        for key in ("x", "x32"):
            d = P.ITD()
            rows = d.itd(inp[key], max_iteration=M)
            out += [rows.copy(), d.get_baselines().copy(), np.asarray(d.knot_counts, np.int64)]
        return tuple(out)

    def reference(self, inp):
        out = []
        for key in ("x", "x32"):
            o = _dec_ref(inp, key)
            out += [o["rows"], o["baselines"], _kc_pad(o["knot_counts"], inp[key])]
        return tuple(out)

    def check(self, inp, got, P=None):
        ref = self.reference(inp)
        same_results(_kc_lenient(got, ref, (2, 5)), ref, self.name)


class decompose_rows32_host(DecMake, Cell):
    entries = ("itd_decompose_rows32_host_f64", "itd_decompose_rows32_host_f32")
    buffers = DEC_BUFFERS
    decided_by = "the decomposition's kernels with Trow = float: one rounding at the store"

    def run(self, P, inp):
        return tuple(P.ITD().itd(inp[key], max_iteration=M, out_dtype=np.float32).copy() for key in ("x", "x32"))

    def reference(self, inp):
        with np.errstate(over="ignore", under="ignore"):
            return tuple(_dec_ref(inp, key)["rows"].astype(np.float32) for key in ("x", "x32"))

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


class decompose_select_host(DecMake, Cell):
    entries = ("itd_decompose_select_host_f64", "itd_decompose_select_host_f32")
    buffers = DEC_BUFFERS
    decided_by = "the decomposition's kernels with SEL = true: the same values, fewer stores"

    def run(self, P, inp):
        a = P.ITD().itd(inp["x"], max_iteration=M, select=SELECT).copy()
        b = P.ITD().itd(inp["x32"], max_iteration=M, select=SELECT, out_dtype=np.float32).copy()
        return a, b

    def reference(self, inp):
        with np.errstate(over="ignore", under="ignore"):
            return (_select_ref(_dec_ref(inp, "x")["rows"], SELECT),
                    _select_ref(_dec_ref(inp, "x32")["rows"], SELECT).astype(np.float32))

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


class decompose_dev(DecMake, DevCell):
    """The six device entries with one signal, on the process engine, each finished by itd_get_summary."""
    entries = ("itd_decompose_f64", "itd_decompose_f32", "itd_decompose_rows32_f64", "itd_decompose_rows32_f32",
               "itd_decompose_select_f64", "itd_decompose_select_f32", "itd_get_summary", "itd_copy")
    buffers = ("d_pp", "d_counts", "d_recs", "d_gsum", "d_state", "h_state")
    decided_by = "as decompose_host"
    staged = ("x", "x32")
    FORMS = (("x", np.float64, np.float64, None, True), ("x32", np.float32, np.float64, None, False),
             ("x", np.float64, np.float32, None, False), ("x32", np.float32, np.float32, None, False),
             ("x", np.float64, np.float64, SELECT, False), ("x32", np.float32, np.float32, SELECT, False))

    def arrays(self, inp):
        n = inp["n"]
        a = {"x": inp["x"], "x32": inp["x32"], "bases": pad_rows((M + 2, n))}
        for k, (_, _, rdt, sel, _) in enumerate(self.FORMS):
            a["rows%d" % k] = np.full((len(sel) if sel else M + 2) * n + PAD, SENT, rdt)
        return a

    stream_outputs = 5          # on a caller's stream only the first form is enqueued: the outputs it fills

    def enqueue(self, eng, d, inp, stream):
        """stream None: all six forms, each finished by its summary; a caller's stream: the float64 form with baselines alone, with no
        synchronisation (collect reads its summary)."""
        self.summaries = []
        for k, (key, xdt, rdt, sel, bases) in enumerate(self.FORMS):
            eng.decompose_dev(d.ptr(key), xdt, inp["n"], 1, inp["n"], M, d.ptr("rows%d" % k), d.ptr("bases") if bases else None,
                              stream, rows_dtype=rdt, select=sel)
            if stream is not None:
                return
            self.summaries.append(eng.summary(1))

    def collect(self, eng, d, inp):
        n = inp["n"]
        if not self.summaries:
            self.summaries = [eng.summary(1)]
        out = []
        for k, (_, _, _, sel, bases) in enumerate(self.FORMS[: len(self.summaries)]):
            s = self.summaries[k]
            buf = d.get("rows%d" % k)
            R = len(sel) if sel else int(s["n_rows"][0])
            rows = buf[: R * n].reshape(R, n).copy()
            if sel:
                from pyitd_amd.engine import zero_absent_slots
                zero_absent_slots(rows, sel, int(s["n_rows"][0]))
            out += [rows, buf[(len(sel) if sel else M + 2) * n:].copy()]
            if bases:
                b = d.get("bases")
                out += [b[: int(s["n_baselines"][0]) * n].reshape(-1, n).copy(), b[(M + 2) * n:].copy(), s["knot_counts"][0].copy()]
        return tuple(out)

    def reference(self, inp):
        out = []
        with np.errstate(over="ignore", under="ignore"):
            for key, _, rdt, sel, bases in self.FORMS:
                o = _dec_ref(inp, key)
                rows = _select_ref(o["rows"], sel) if sel else o["rows"]
                out += [rows.astype(rdt), np.full(PAD, SENT, rdt)]
                if bases:
                    out += [o["baselines"], np.full(PAD, SENT), _kc_pad(o["knot_counts"], inp[key])]
        return tuple(out)

    def check(self, inp, got, P=None):
        ref = self.reference(inp)
        same_results(_kc_lenient(got, ref, (4,)), ref, self.name)


class decompose_batch(Cell):
    """itd_batch over rows signals (the batch engine of pyitd_amd.itd: the other process-wide engine), baselines kept."""
    entries = ("itd_decompose_f64", "itd_get_summary")
    buffers = ("d_pp", "d_counts", "d_recs", "d_gsum", "d_state", "h_state", "dirty_sig / dirty_gs of both sets")
    decided_by = "as decompose_host"

    def make(self, size, seed):
        n, rows = self.dims(size)
        return {"n": n, "x": signals(n, rows, seed)}

    def run(self, P, inp):
        r = P.itd_batch(inp["x"], max_iteration=M, keep_baselines=True)
        rows, bases = r["rows"].copy(), r["baselines"].copy()
        for b in range(rows.shape[0]):                  # rows past n_rows are unspecified
            rows[b, r["n_rows"][b]:] = 0
            bases[b, r["n_baselines"][b]:] = 0
        return rows, bases, r["n_rows"].copy(), r["n_baselines"].copy(), r["knot_counts"].copy()

    def reference(self, inp):
        x = inp["x"]
        B, n = x.shape
        rows, bases = np.zeros((B, M + 2, n)), np.zeros((B, M + 2, n))
        nr, nb, kc = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros((B, 23), np.int64)
        for b in range(B):
            o = memo(inp, "dec%d" % b, lambda: cpu_oracle.itd(x[b], M))
            nr[b], nb[b], kc[b] = len(o["rows"]), len(o["baselines"]), _kc_pad(o["knot_counts"], x[b])
            rows[b, : nr[b]], bases[b, : nb[b]] = o["rows"], o["baselines"]
        return rows, bases, nr, nb, kc

    def check(self, inp, got, P=None):
        ref = self.reference(inp)
        same_results(_kc_lenient(got, ref, (4,)), ref, self.name)


# ================================================================================================================================
# the single-level operators behind helper_ws()
# ================================================================================================================================
def oracle_detect(x, mode):
    from test_gpu_device_entries import oracle_detect as f
    return f(x, mode)


class OneSignal:
    kind = None

    def make(self, size, seed):
        n, _ = self.dims(size)
        kinds = ("quantised", "noise", "seams") if self.kind is None else (self.kind,)
        x = signals(n, 1, seed + len(size), kinds[seed % len(kinds):] + kinds)[0]
        return {"n": n, "x": x, "x32": x.astype(np.float32)}

    def reaches_working_branch(self, inp):
        return len(cpu_oracle.knots(inp["x"])) > 10


HELPER_WS = ("d_lists", "d_kidx", "d_total", "d_hcounts", "d_hrecs", "d_hgsum", "d_hstate")


class detect_host(OneSignal, Cell):
    entries = ("itd_detect_host_f64", "itd_find_extrema_host_f64")
    buffers = HELPER_WS + ("d_io_x",)
    decided_by = "k_scan / k_compact: prefix counts, integer"

    def run(self, P, inp):
        x = inp["x"]
        e, idx = P.find_extrema(x)
        return P.detect_knots(x), P.detect_peaks(x), P.matlab_detect_peaks(x), np.asarray(e), np.array([idx], np.int64)

    def reference(self, inp):
        x = inp["x"]
        e, idx = cpu_oracle.find_extrema(x)
        return tuple(oracle_detect(x, m) for m in range(3)) + (e, np.array([idx], np.int64))

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


class detect_dev(OneSignal, Cell):
    """itd_detect_f64 / _f32 in each mode (they synchronise for the count)."""
    entries = ("itd_detect_f64", "itd_detect_f32", "itd_copy")
    buffers = HELPER_WS
    decided_by = "k_scan / k_compact"

    def run(self, P, inp):
        n = inp["n"]
        eng = eng_of(P, n)
        out = []
        d = DevArrays(eng, x=inp["x"], x32=inp["x32"], kn=np.full(n + PAD, ISENT, np.int32))
        try:
            for fn, key in ((eng._L.itd_detect_f64, "x"), (eng._L.itd_detect_f32, "x32")):
                for mode in range(5):
                    d.put("kn", np.full(n + PAD, ISENT, np.int32))
                    m = _i64(-5)
                    rc = fn(eng._h, d.ptr(key), n, mode, d.ptr("kn"), ctypes.byref(m), None)
                    assert rc == OK, (key, mode, rc)
                    kn = d.get("kn")
                    assert np.all(kn[m.value:] == ISENT), "written past the count"
                    out.append(kn[: m.value].astype(np.int64))
        finally:
            d.free()
        return tuple(out)

    def reference(self, inp):
        return tuple(oracle_detect(inp[key].astype(np.float64), m) for key in ("x", "x32") for m in range(5))

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


class extract_host(OneSignal, Cell):
    entries = ("itd_baseline_extract_host_f64",)
    buffers = HELPER_WS + ("d_io_x", "d_io_rows")
    decided_by = "k_scan / k_compact / k_extract"

    def run(self, P, inp):
        return eng_of(P, inp["n"]).baseline_extract_host(inp["x"], want_knots=True)

    def reference(self, inp):
        return cpu_oracle.itd_baseline_extract(inp["x"], want_knots=True)

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


class extract_dev(OneSignal, DevCell):
    """itd_baseline_extract_f64 / _f32 with the knots on the device and no count on the host: nothing synchronises."""
    entries = ("itd_baseline_extract_f64", "itd_baseline_extract_f32", "itd_copy")
    buffers = HELPER_WS
    decided_by = "k_scan / k_compact / k_extract"
    staged = ("x", "x32")

    def arrays(self, inp):
        n = inp["n"]
        return dict(x=inp["x"], x32=inp["x32"], rot=np.full(n + PAD, SENT), base=np.full(n + PAD, SENT),
                    kn=np.full(n + PAD, ISENT, np.int32), rot32=np.full(n + PAD, SENT), base32=np.full(n + PAD, SENT))

    def enqueue(self, eng, d, inp, stream):
        n = inp["n"]
        assert eng._L.itd_baseline_extract_f64(eng._h, d.ptr("x"), n, d.ptr("rot"), d.ptr("base"), d.ptr("kn"), None, stream) == OK
        assert eng._L.itd_baseline_extract_f32(eng._h, d.ptr("x32"), n, d.ptr("rot32"), d.ptr("base32"), None, None, stream) == OK

    def collect(self, eng, d, inp):
        return tuple(d.get(k) for k in ("rot", "base", "kn", "rot32", "base32"))

    def reference(self, inp):
        n = inp["n"]
        rot, base, kn, _ = cpu_oracle.itd_baseline_extract(inp["x"], want_knots=True)
        r32, b32 = cpu_oracle.itd_baseline_extract(inp["x32"].astype(np.float64))
        knb = np.full(n + PAD, ISENT, np.int32)
        knb[: len(kn)] = kn
        tail = np.full(PAD, SENT)
        return (np.concatenate((rot, tail)), np.concatenate((base, tail)), knb, np.concatenate((r32, tail)), np.concatenate((b32, tail)))

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


def _ext_knots(x):
    k = cpu_oracle.knots(x)
    return np.concatenate(([0], k, [len(x) - 1])).astype(np.int64)


class knot_values_host(OneSignal, Cell):
    entries = ("itd_knot_values_host_f64",)
    buffers = ("d_io_x", "d_cub_e", "d_io_rows")
    decided_by = "k_knot_values: one thread per knot"

    def run(self, P, inp):
        e = _ext_knots(inp["x"])
        bk = np.zeros(len(e))
        bk[0], bk[-1] = np.mean(inp["x"][:2]), np.mean(inp["x"][-2:])
        return (np.asarray(P.baseline_knot_estimation(bk, inp["x"], e)),)

    def reference(self, inp):
        e = _ext_knots(inp["x"])
        want = cpu_oracle.knot_values(inp["x"], e)
        want[0], want[-1] = np.mean(inp["x"][:2]), np.mean(inp["x"][-2:])
        return (want,)

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


class knot_values_dev(OneSignal, DevCell):
    entries = ("itd_knot_values_f64", "itd_copy")
    buffers = ()
    decided_by = "k_knot_values"
    staged = ("x", "e")

    def arrays(self, inp):
        e = _ext_knots(inp["x"])
        return dict(x=inp["x"], e=e.astype(np.int32), bk=np.full(len(e) + PAD, -5.0))

    def enqueue(self, eng, d, inp, stream):
        eng.knot_values_dev(d.ptr("x"), inp["n"], d.ptr("e"), len(d.host["e"]) - 2, d.ptr("bk"), stream)

    def collect(self, eng, d, inp):
        return (d.get("bk"),)

    def reference(self, inp):
        e = _ext_knots(inp["x"])
        want = np.full(len(e) + PAD, -5.0)
        want[1: len(e) - 1] = cpu_oracle.knot_values(inp["x"], e)[1:-1]
        return (want,)

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


# ================================================================================================================================
# the natural cubic operator, its float32 and I/Q forms, its batch
# ================================================================================================================================
def _caller_list(x):
    """A caller's list that is not the signal's own: every third of its extrema (itd.cpp's predicate), then the 0 behind them."""
    e, idx = cpu_oracle.extrema_cpp(x)
    k = e[:idx][::3]
    return np.concatenate((k, [0])).astype(np.int64), len(k)


class CubicMake(OneSignal):
    def make(self, size, seed):
        n, _ = self.dims(size)
        kinds = ("noise", "fam_quantised", "seams")
        x = signals(n, 1, seed, kinds[(seed + len(size)) % 3:] + kinds)[0]
        lst, idx = _caller_list(x)
        rng = np.random.default_rng(seed + 5)
        q = 0.5 * x + 0.25 * np.max(np.abs(x)) * rng.standard_normal(n)
        return {"n": n, "x": x, "x32": x.astype(np.float32), "lst": lst, "idx": np.array([idx]), "q": q}

    def reaches_working_branch(self, inp):
        return int(inp["idx"][0]) >= 10 and cpu_oracle.extrema_cpp(inp["x"])[1] >= 10 and iq_oracle.extrema_iq(inp["x"] + 1j * inp["q"])[1] >= 10

    def _exact(self, inp, key, mode):
        x = inp[key].astype(np.float64)
        if mode == "list":
            lst, idx = inp["lst"], int(inp["idx"][0])
        else:
            lst, idx = cpu_oracle.extrema_cpp(x)
        return memo(inp, ("nat", key, mode), lambda: (ex.natural(x, lst, idx), cpu_oracle.itd_baseline_extract_fast(x, lst, idx), idx))

    def _check_cubic(self, inp, got, forms):
        """got: one baseline per (key, mode) of forms, then one int64 array of the idx each call reported."""
        for g, (key, mode) in zip(got, forms):
            r, ref, _ = self._exact(inp, key, mode)
            spline_check("%s %s/%s %s" % (self.name, key, mode, inp["size"]), r, g, inp[key].astype(np.float64), ref)
        assert list(got[len(forms)]) == [self._exact(inp, key, mode)[2] for key, mode in forms], got[len(forms)]

    def _reference_cubic(self, inp, forms):
        return tuple(self._exact(inp, key, mode)[1] for key, mode in forms) + (np.array([self._exact(inp, k, m)[2] for k, m in forms], np.int64),)


CUBIC_BUFFERS = HELPER_WS + ("d_cub", "d_cub_e")


class cubic_host(CubicMake, Cell):
    """Natural cubic with the caller's list and with detected knots, host forms."""
    entries = ("itd_baseline_extract_cubic_host_f64",)
    buffers = CUBIC_BUFFERS + ("d_io_x", "d_io_rows")
    decided_by = "k_cubic_*: the sweeps are scans in a fixed tree order"
    FORMS = (("x", "list"), ("x", "detect"))

    def run(self, P, inp):
        a = P.itd_baseline_extract_fast(inp["x"], inp["lst"], int(inp["idx"][0]))
        b, kn = P.itd_baseline_extract_cubic(inp["x"], want_knots=True)
        return a, b, np.array([int(inp["idx"][0]), len(kn)], np.int64), kn

    def reference(self, inp):
        e, idx = cpu_oracle.extrema_cpp(inp["x"])
        return self._reference_cubic(inp, self.FORMS) + (e[:idx],)

    def check(self, inp, got, P=None):
        self._check_cubic(inp, got, self.FORMS)
        e, idx = cpu_oracle.extrema_cpp(inp["x"])
        _same(got[3], e[:idx], "detected knots")


def _cubic_dev(eng, fn, d, key, n, lst_key, idx):
    got = _i64(-5)
    rc = fn(eng._h, d.ptr(key), n, None if lst_key is None else d.ptr(lst_key), idx, d.ptr("base"), ctypes.byref(got), None)
    return rc, got.value


class cubic_dev(CubicMake, Cell):
    """itd_baseline_extract_cubic_f64 and _f32 on device buffers, list and detected knots."""
    entries = ("itd_baseline_extract_cubic_f64", "itd_baseline_extract_cubic_f32", "itd_copy")
    buffers = CUBIC_BUFFERS
    decided_by = "k_cubic_*"
    FORMS = (("x", "list"), ("x", "detect"), ("x32", "list"), ("x32", "detect"))

    def run(self, P, inp):
        n = inp["n"]
        eng = eng_of(P, n)
        d = DevArrays(eng, x=inp["x"], x32=inp["x32"], e=inp["lst"].astype(np.int32), base=np.full(n + PAD, SENT))
        out, idxs = [], []
        try:
            for key, mode in self.FORMS:
                d.put("base", np.full(n + PAD, SENT))
                fn = eng._L.itd_baseline_extract_cubic_f64 if key == "x" else eng._L.itd_baseline_extract_cubic_f32
                rc, idx = _cubic_dev(eng, fn, d, key, n, "e" if mode == "list" else None, int(inp["idx"][0]) if mode == "list" else 0)
                assert rc == OK, (key, mode, rc)
                b = d.get("base")
                assert pad_ok(b, n), "written past the baseline"
                out.append(b[:n].copy())
                idxs.append(idx)
        finally:
            d.free()
        return tuple(out) + (np.array(idxs, np.int64),)

    def reference(self, inp):
        return self._reference_cubic(inp, self.FORMS)

    def check(self, inp, got, P=None):
        self._check_cubic(inp, got, self.FORMS)


class iq(CubicMake, Cell):
    """The I/Q form: host list, host detected, device list."""
    entries = ("itd_baseline_extract_iq_host_f64", "itd_baseline_extract_iq_f64", "itd_copy")
    buffers = CUBIC_BUFFERS + ("d_iq_avg", "d_io_x", "d_io_rows")
    decided_by = "k_iq_mean + k_cubic_*"

    def run(self, P, inp):
        n, idx = inp["n"], int(inp["idx"][0])
        z = inp["x"] + 1j * inp["q"]
        a = P.itd_baseline_extract_iq(z, inp["lst"], idx)
        b, kn, got = P.itd_baseline_extract_iq(z, want_knots=True)
        eng = eng_of(P, n)
        d = DevArrays(eng, iq=np.ascontiguousarray(z).view(np.float64), e=inp["lst"].astype(np.int32), base=np.full(n + PAD, SENT))
        try:
            g = _i64(-5)
            rc = eng._L.itd_baseline_extract_iq_f64(eng._h, d.ptr("iq"), n, d.ptr("e"), idx, d.ptr("base"), ctypes.byref(g), None)
            assert rc == OK, rc
            c = d.get("base")
        finally:
            d.free()
        assert pad_ok(c, n)
        return a, b, c[:n].copy(), kn

    def _refs(self, inp):
        def f():
            I, Q, idx = inp["x"], inp["q"], int(inp["idx"][0])
            avg = (I + Q) / 2.0
            e, ie = iq_oracle.extrema_iq(I + 1j * Q)
            return ((ex.iq(I, Q, inp["lst"], idx), cpu_oracle.itd_baseline_extract_fast(avg, inp["lst"], idx)),
                    (ex.iq(I, Q, e, ie), cpu_oracle.itd_baseline_extract_fast(avg, e, ie)), e[:ie])
        return memo(inp, "iq", f)

    def reference(self, inp):
        (_, a), (_, b), kn = self._refs(inp)
        return a, b, a, kn

    def check(self, inp, got, P=None):
        (ra, fa), (rb, fb), kn = self._refs(inp)
        S = np.maximum(np.abs(inp["x"]), np.abs(inp["q"]))
        spline_check("iq host list", ra, got[0], S, fa)
        spline_check("iq host detect", rb, got[1], S, fb)
        spline_check("iq dev list", ra, got[2], S, fa)
        _same(got[3], kn, "iq knots")


class Rows:
    kinds = KINDS

    def make(self, size, seed):
        n, rows = self.dims(size)
        x = signals(n, rows, seed, self.kinds)
        return {"n": n, "x": x, "x32": x.astype(np.float32)}

    def reaches_working_branch(self, inp):
        return all(len(cpu_oracle.knots(r)) >= 10 for r in inp["x"])


class ScaledRows:
    def make(self, size, seed):
        n, rows = self.dims(size)
        base = signals(n, 2, seed, ("noise", "seams") if len(size + self.name) % 2 else ("sine", "fam_noise"))
        x, factors, src = scaled_rows(base, rows)
        lst, idx = _caller_list(base[0])
        return {"n": n, "x": x, "base": base, "factors": factors, "src": src, "lst": lst, "idx": np.array([idx])}

    def reaches_working_branch(self, inp):
        return all(len(cpu_oracle.knots(r)) >= 10 for r in inp["base"]) and int(inp["idx"][0]) >= 10


class cubic_batch(ScaledRows, DevCell):
    """itd_baseline_extract_cubic_batch_f64: one shared list for every row, then every row's own detected knots."""
    entries = ("itd_baseline_extract_cubic_batch_f64", "itd_copy")
    buffers = ("d_dw (knot_workspace)", "d_cub")
    decided_by = "k_scan_batch / k_cubic_*"
    staged = ("x", "e")

    def arrays(self, inp):
        B, n = inp["x"].shape
        return dict(x=inp["x"], e=inp["lst"].astype(np.int32), shared=np.full(B * n + PAD, SENT), own=np.full(B * n + PAD, SENT),
                    info=np.full(2 * B + PAD, ISENT, np.int32))

    def enqueue(self, eng, d, inp, stream):
        B, n = inp["x"].shape
        eng.cubic_batch_dev(d.ptr("x"), n, B, n, d.ptr("e"), 0, int(inp["idx"][0]), d.ptr("shared"), n, d.ptr("info"), stream)
        eng.cubic_batch_dev(d.ptr("x"), n, B, n, None, 0, 0, d.ptr("own"), n, d.ptr("info") + 4 * B, stream)

    def collect(self, eng, d, inp):
        return d.get("shared"), d.get("own"), d.get("info")

    def _exact(self, inp):
        def f():
            out = {}
            idx = int(inp["idx"][0])
            for s in (0, 1):
                x = inp["base"][s]
                e, ie = cpu_oracle.extrema_cpp(x)
                out[s] = ((ex.natural(x, inp["lst"], idx), cpu_oracle.itd_baseline_extract_fast(x, inp["lst"], idx), idx),
                          (ex.natural(x, e, ie), cpu_oracle.itd_baseline_extract_fast(x, e, ie), ie))
            return out
        return memo(inp, "cb", f)

    def reference(self, inp):
        B, n = inp["x"].shape
        E = self._exact(inp)
        tail = np.full(PAD, SENT)
        shared = np.concatenate([inp["factors"][b] * E[inp["src"][b]][0][1] for b in range(B)] + [tail])
        own = np.concatenate([inp["factors"][b] * E[inp["src"][b]][1][1] for b in range(B)] + [tail])
        info = np.full(2 * B + PAD, ISENT, np.int32)
        info[:B] = int(inp["idx"][0])
        info[B: 2 * B] = [E[inp["src"][b]][1][2] for b in range(B)]
        return shared, own, info

    def check(self, inp, got, P=None):
        B, n = inp["x"].shape
        E = self._exact(inp)
        _same(got[2], self.reference(inp)[2], "cubic batch info")
        for k, buf in enumerate(got[:2]):
            assert pad_ok(buf, B * n), "written past the rows"
            for b in range(B):
                r, ref, _ = E[inp["src"][b]][k]
                spline_check("cubic batch %s row %d" % (("shared", "own")[k], b), r, buf[b * n:(b + 1) * n] / inp["factors"][b],
                             inp["base"][inp["src"][b]], ref)


class detect_batch(Rows, DevCell):
    """itd_detect_batch_f64: lists in the modes KNOTS, CPP and ZERO_CROSS, counts alone in VALLEYS and PEAKS."""
    entries = ("itd_detect_batch_f64", "itd_copy")
    buffers = ("d_dw (knot_workspace)",)
    decided_by = "k_scan_batch / k_compact_batch"
    staged = ("x",)
    LISTS, COUNTS = (0, 3, 4), (1, 2)

    def arrays(self, inp):
        B, n = inp["x"].shape
        a = dict(x=inp["x"], info=np.full(5 * B + PAD, ISENT, np.int32))
        for m in self.LISTS:
            a["idx%d" % m] = np.full(B * (n - 2) + PAD, ISENT, np.int32)
        return a

    def enqueue(self, eng, d, inp, stream):
        B, n = inp["x"].shape
        for m in self.LISTS:
            eng.detect_batch_dev(d.ptr("x"), n, B, n, m, d.ptr("idx%d" % m), n - 2, d.ptr("info") + 4 * B * m, stream)
        for m in self.COUNTS:
            eng.detect_batch_dev(d.ptr("x"), n, B, n, m, None, 0, d.ptr("info") + 4 * B * m, stream)

    def collect(self, eng, d, inp):
        B, n = inp["x"].shape
        info = d.get("info")
        out = [info]
        for m in self.LISTS:       # entries [count, n - 2) of a slot are unspecified: cleared before any comparison
            buf = d.get("idx%d" % m)
            body = buf[: B * (n - 2)].reshape(B, n - 2)
            for b in range(B):
                c = int(info[B * m + b])
                if 0 <= c <= n - 2:
                    body[b, c:] = ISENT
            out.append(buf)
        return tuple(out)

    def reference(self, inp):
        B, n = inp["x"].shape
        info = np.full(5 * B + PAD, ISENT, np.int32)
        out = []
        for m in range(5):
            lists, i = memo(inp, ("det", m), lambda: bc.detect_reference(inp["x"], m))
            info[B * m: B * (m + 1)] = i
            if m in self.LISTS:
                buf = np.full(B * (n - 2) + PAD, ISENT, np.int32)
                for b, k in enumerate(lists):
                    buf[b * (n - 2): b * (n - 2) + len(k)] = k
                out.append(buf)
        return (info,) + tuple(out)

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


class extract_batch(Rows, DevCell):
    entries = ("itd_baseline_extract_batch_f64", "itd_copy")
    buffers = ("d_bw (knot_workspace)",)
    decided_by = "k_scan_batch / k_extract"
    staged = ("x",)

    def arrays(self, inp):
        B, n = inp["x"].shape
        return dict(x=inp["x"], rot=np.full(B * n + PAD, SENT), base=np.full(B * n + PAD, SENT), info=np.full(B + PAD, ISENT, np.int32))

    def enqueue(self, eng, d, inp, stream):
        B, n = inp["x"].shape
        eng.extract_batch_dev(d.ptr("x"), n, B, n, d.ptr("rot"), n, d.ptr("base"), n, d.ptr("info"), stream)

    def collect(self, eng, d, inp):
        return d.get("rot"), d.get("base"), d.get("info")

    def reference(self, inp):
        B = inp["x"].shape[0]
        rot, base, info = memo(inp, "ext", lambda: bc.extract_reference(inp["x"]))
        ib = np.full(B + PAD, ISENT, np.int32)
        ib[:B] = info
        tail = np.full(PAD, SENT)
        return np.concatenate((rot.ravel(), tail)), np.concatenate((base.ravel(), tail)), ib

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


class count_knots(Rows, Cell):
    entries = ("itd_count_knots_host_f64", "itd_count_knots_f64", "itd_copy")
    buffers = ("d_dw (knot_workspace)", "d_io_x", "h_small", "small_seq")
    decided_by = "k_scan_batch: integer counts"

    def run(self, P, inp):
        B, n = inp["x"].shape
        eng = eng_of(P, n)
        host = np.stack([eng.count_knots_host(inp["x"], m) for m in range(5)])
        d = DevArrays(eng, x=inp["x"])
        try:
            dev = np.zeros((5, B), np.int32)
            for m in range(5):
                assert eng._L.itd_count_knots_f64(eng._h, d.ptr("x"), n, B, n, m, _p(dev[m]), None) == OK
        finally:
            d.free()
        return host, dev

    def reference(self, inp):
        c = np.stack([bc.detect_reference(inp["x"], m)[1] for m in range(5)]).astype(np.int32)
        return c, c

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


# ================================================================================================================================
# the FITPACK flavour, its 2-D consumer, MEITD's operators and loops
# ================================================================================================================================
SPLINE_BUFFERS = ("d_sp (knot_workspace)", "d_cub (nak_small_ws)", "d_io_x", "d_io_rows", "spline_solver")


class SplineCell(ScaledRows, Cell):
    """itd_baseline_extract_modified of every row (min_extrema 10) through the three entries of the operator, one solver."""
    entries = ("itd_baseline_extract_spline_host2_f64", "itd_baseline_extract_spline_host_f64", "itd_baseline_extract_spline_f64",
               "itd_set_spline_solver", "itd_copy")
    buffers = SPLINE_BUFFERS
    solver = None

    def run(self, P, inp):
        B, n = inp["x"].shape
        x = np.ascontiguousarray(inp["x"])
        a = mod("spline").itd_baseline_extract_rows(x, 10, solver=self.solver)
        eng = spline_eng(P, n, self.solver)
        b, rot, kn = np.empty((B, n)), np.empty((B, n)), np.zeros(B, np.int32)
        assert eng._L.itd_baseline_extract_spline_host_f64(eng._h, _p(x), n, B, 10, _p(b), _p(rot), _p(kn)) == OK
        d = DevArrays(eng, x=x, base=np.full(B * n + PAD, SENT))
        try:
            kd = np.zeros(B, np.int32)
            assert eng._L.itd_baseline_extract_spline_f64(eng._h, d.ptr("x"), n, B, n, 10, d.ptr("base"), n, None, n, _p(kd), None) == OK
            c = d.get("base")
        finally:
            d.free()
        assert pad_ok(c, B * n)
        return a, b, c[: B * n].reshape(B, n).copy(), rot, kn, kd

    def _exact(self, inp):
        return memo(inp, "nak", lambda: [(ex.nak(x, 10), so.baseline(x, 10), len(cpu_oracle.knots(x))) for x in inp["base"]])

    def reference(self, inp):
        E = self._exact(inp)
        base = np.stack([inp["factors"][b] * E[inp["src"][b]][1] for b in range(len(inp["factors"]))])
        kn = np.array([E[s][2] for s in inp["src"]], np.int32)
        return base, base, base, inp["x"] - base, kn, kn

    def check(self, inp, got, P=None):
        E = self._exact(inp)
        for k in range(3):
            for b in range(got[k].shape[0]):
                r, ref, _ = E[inp["src"][b]]
                spline_check("%s form %d row %d" % (self.name, k, b), r, got[k][b] / inp["factors"][b], inp["base"][inp["src"][b]], ref)
        _bits(got[3], inp["x"] - got[1], "rotation = x - baseline")
        kn = np.array([E[s][2] for s in inp["src"]], np.int32)
        _same(got[4], kn, "knot counts (host)")
        _same(got[5], kn, "knot counts (device)")


class spline_serial(SplineCell):
    solver = "serial"
    decided_by = "k_fitpack_rows: one thread per signal, FITPACK's own order"


class spline_parallel(SplineCell):
    solver = "parallel"
    decided_by = "k_nak_* (itd_nak.hpp): scans in a fixed tree order"


class spline2(OneSignal, Cell):
    """MEITD's extraction on device rows (min_extrema 0, parallel solver) with the produced baseline's knot count."""
    entries = ("itd_baseline_extract_spline2_f64", "itd_set_spline_solver", "itd_copy")
    buffers = SPLINE_BUFFERS + ("h_small", "small_seq")
    decided_by = "k_nak_small: one workgroup, fixed order"
    kind = "sine"

    def run(self, P, inp):
        n = inp["n"]
        eng = spline_eng(P, n, "parallel")
        d = DevArrays(eng, x=inp["x"], base=np.full(n + PAD, SENT), rot=np.full(n + PAD, SENT))
        try:
            kn, bk = eng.spline_extract_dev(d.ptr("x"), n, d.ptr("base"), d.ptr("rot"), 0, want_baseline_knots=True)
            base, rot = d.get("base"), d.get("rot")
        finally:
            d.free()
        assert pad_ok(base, n) and pad_ok(rot, n)
        return base[:n].copy(), rot[:n].copy(), np.array([kn, bk], np.int64)

    def _exact(self, inp):
        return memo(inp, "nak0", lambda: (ex.nak(inp["x"], 0), so.baseline(inp["x"], 0)))

    def reference(self, inp):
        _, ref = self._exact(inp)
        return ref, inp["x"] - ref, np.array([len(cpu_oracle.knots(inp["x"])), len(cpu_oracle.knots(ref))], np.int64)

    def check(self, inp, got, P=None):
        r, ref = self._exact(inp)
        spline_check("spline2 " + inp["size"], r, got[0], inp["x"], ref)
        _bits(got[1], inp["x"] - got[0], "rotation = x - baseline")
        assert got[2][0] == len(cpu_oracle.knots(inp["x"])) and got[2][1] == len(cpu_oracle.knots(got[0])), got[2]


class crossways(Cell):
    entries = ("itd_crossways_host_f64", "itd_crossways_f64", "itd_copy")
    buffers = ("d_sp (knot_workspace)", "d_sp2", "d_flag", "d_io_x", "d_io_rows")
    decided_by = "k_fitpack_rows (the image sweeps are always serial), k_transpose, k_mean2"
    SHAPES = {"S": (2, 24, 43), "L": (7, 41, 64), "G": (3, 101, 198)}

    def make(self, size, seed):
        p, r, c = self.SHAPES[size]
        rng = np.random.default_rng([seed, r, c])
        img = rng.integers(0, 256, (p, r, c)).astype(np.float64)
        img[-1] = np.round(80 * np.sin(np.arange(r)[:, None] / 5.0) * np.cos(np.arange(c)[None, :] / 7.0))
        return {"n": max(r, c), "img": img}

    def reaches_working_branch(self, inp):
        img = inp["img"]
        return all(len(cpu_oracle.knots(row)) >= 10 for row in img[0]) and all(len(cpu_oracle.knots(col)) >= 10 for col in img[0].T)

    def run(self, P, inp):
        img = inp["img"]
        p, r, c = img.shape
        eng = spline_eng(P, max(r, c), "auto")
        host = eng.crossways_host(img, 10)
        d = DevArrays(eng, img=img, out=np.full(img.size + PAD, SENT))
        try:
            assert eng._L.itd_crossways_f64(eng._h, d.ptr("img"), p, r, c, 10, d.ptr("out"), None) == OK
            out = d.get("out")
        finally:
            d.free()
        assert pad_ok(out, img.size)
        return host, out[: img.size].reshape(img.shape).copy()

    def reference(self, inp):
        ref = memo(inp, "cw", lambda: np.stack([so.crossways(p, 10) for p in inp["img"]]))
        return ref, ref

    def check(self, inp, got, P=None):
        ref = self.reference(inp)[0]
        _bits(got[1], got[0], "device form = host form")
        for p in range(ref.shape[0]):
            close_1e12(got[0][p], ref[p], "crossways plane %d" % p)


def _meitd_signals(n, count, seed):
    from test_gpu_meitd_batch import _signals
    return _signals(n, count, seed)


class MeitdOne:
    kind = "sine"

    def make(self, size, seed):
        n, _ = self.dims(size)
        return {"n": n, "x": _meitd_signals(n, 1, seed + n)[0]}

    def reaches_working_branch(self, inp):
        return len(cpu_oracle.knots(inp["x"])) > 5


class wpe(MeitdOne, Cell):
    """weighted_permutation_entropy of order 3 (itd_wpe3_f64, with the knot count) and of order 4 (itd_wpe_f64)."""
    entries = ("itd_wpe3_f64", "itd_wpe_f64", "itd_copy")
    buffers = ("d_wpe", "h_small", "small_seq")
    decided_by = "k_wpe3 / k_wpe: sums one by one in index order up to 65536 windows"

    def run(self, P, inp):
        n, x = inp["n"], inp["x"]
        eng = spline_eng(P, n, "auto")
        d = DevArrays(eng, x=x)
        try:
            w, c, kn = eng.wpe3_dev(d.ptr("x"), n, want_knots=True)
        finally:
            d.free()
        e3 = mod("meitd").weighted_permutation_entropy(x, order=3, normalize=True)
        e4 = mod("meitd").weighted_permutation_entropy(x, order=4, normalize=True)
        return w, c, np.array([kn], np.int64), np.array([e3, e4])

    def reference(self, inp):
        x = inp["x"]
        w, c = meitd_oracle.bins(x)
        e = [meitd_oracle.weighted_permutation_entropy(x, order=o, normalize=True) for o in (3, 4)]
        return np.asarray(w, np.float64), np.asarray(c, np.int64), np.array([len(cpu_oracle.knots(x))], np.int64), np.array(e)

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


class _cpu_model:
    """pyitd_amd.meitd's loops over the oracle's operators (oracle.meitd_oracle.CpuWork): the CPU model of the MEITD cells."""

    def __enter__(self):
        from pyitd_amd import meitd
        self.m, self.saved = meitd, (meitd._work_for, meitd.weighted_permutation_entropy)
        meitd._work_for = lambda nn, device=0, solver="auto": meitd_oracle.CpuWork(nn)
        meitd.weighted_permutation_entropy = lambda ts, order=3, normalize=False, device=0: meitd_oracle.weighted_permutation_entropy(ts, order, normalize)
        return meitd

    def __exit__(self, *a):
        self.m._work_for, self.m.weighted_permutation_entropy = self.saved


def _meitd_model(x):
    with _cpu_model() as meitd, np.errstate(all="ignore"):
        hi, lo, res = meitd.MEITD(x.copy())
        return hi, lo, res, meitd.XITD(x.copy())


def _check_meitd(got, ref, what):
    for g, r, part in zip(got, ref, ("high", "low", "residual", "XITD")):
        assert g.shape == r.shape, "%s %s: %s components against the model's %s" % (what, part, g.shape, r.shape)
        if r.size:
            close_meitd(g, r, "%s %s" % (what, part))


class MeitdCell(MeitdOne, Cell):
    model = True
    solver = "auto"

    def run(self, P, inp):
        hi, lo, res = mod("meitd").MEITD(inp["x"].copy(), solver=self.solver)
        return hi, lo, res, mod("meitd").XITD(inp["x"].copy(), solver=self.solver)

    def reference(self, inp):
        return memo(inp, "model", lambda: _meitd_model(inp["x"]))

    def check(self, inp, got, P=None):
        _check_meitd(got, self.reference(inp), self.name + " " + inp["size"])

    def reaches_working_branch(self, inp):
        hi, lo, _, _ = self.reference(inp)
        return len(cpu_oracle.knots(inp["x"])) > 5 and hi.shape[0] + lo.shape[0] >= 1


class meitd_one_launch(MeitdCell):
    """MEITD and XITD of one signal of 1024 .. 8192 samples under the automatic solver: the whole loop as one launch (above 8192
    samples, size G, the host-driven loop under the parallel-in-knots solver)."""
    entries = ("itd_meitd_small_f64", "itd_set_spline_solver", "itd_copy", "itd_wpe3_f64")
    buffers = ("d_cub (nak_small_ws)", "h_small", "small_seq", "d_wpe")
    decided_by = "k_meitd_small: one workgroup, fixed order"


class meitd_host_driven(MeitdCell):
    """The same under the serial solver: one launch per operator, scalars through h_small."""
    entries = ("itd_baseline_extract_spline2_f64", "itd_count_knots_f64", "itd_wpe3_f64", "itd_subtract_f64", "itd_copy", "itd_set_spline_solver")
    buffers = ("d_sp (knot_workspace)", "d_dw (knot_workspace)", "d_wpe", "h_small", "small_seq")
    decided_by = "k_fitpack_rows, k_scan_batch, k_wpe3, k_subtract"
    solver = "serial"


class meitd_batch(Cell):
    """MEITD_batch and XITD_batch: one workgroup per signal, one launch, the components gathered by itd_gather_rows_f64."""
    entries = ("itd_meitd_batch_f64", "itd_gather_rows_f64", "itd_set_spline_solver")
    buffers = ("d_mb", "d_rowtab", "d_cub (nak_small_ws)")
    decided_by = "k_meitd_batch: one workgroup per signal, fixed order; k_gather_rows"
    model = True

    def make(self, size, seed):
        n, rows = self.dims(size)
        n = min(n, 8192)                                # the launch takes signals of up to 8192 samples
        return {"n": n, "x": _meitd_signals(n, rows, seed + n)}

    def run(self, P, inp):
        m = mod("meitd").MEITD_batch(inp["x"])
        xs = mod("meitd").XITD_batch(inp["x"])
        out = []
        for (hi, lo, res), xi in zip(m, xs):
            out += [hi, lo, res, xi]
        return tuple(out)

    def reference(self, inp):
        def f():
            out = []
            for x in inp["x"]:
                out += list(_meitd_model(x))
            return tuple(out)
        return memo(inp, "model", f)

    def check(self, inp, got, P=None):
        ref = self.reference(inp)
        assert len(got) == len(ref)
        for b in range(len(ref) // 4):
            _check_meitd(got[4 * b: 4 * b + 4], ref[4 * b: 4 * b + 4], "%s signal %d" % (self.name, b))

    def reaches_working_branch(self, inp):
        return all(len(cpu_oracle.knots(x)) > 5 for x in inp["x"])


class gather_rows(Rows, Cell):
    entries = ("itd_gather_rows_f64", "itd_copy")
    buffers = ("d_rowtab",)
    decided_by = "k_gather_rows: a copy"

    def _offsets(self, inp):
        B, n = inp["x"].shape
        return np.array([(B - 1 - b) * n for b in range(B)] + [n // 2], np.int64)

    def run(self, P, inp):
        B, n = inp["x"].shape
        eng = eng_of(P, n)
        off = self._offsets(inp)
        d = DevArrays(eng, src=inp["x"], dst=np.full(len(off) * n + PAD, SENT))
        try:
            out = np.empty((len(off), n))
            eng.gather_rows_dev(d.ptr("src"), B * n, off, n, d.ptr("dst"), out)
            dst = d.get("dst")
        finally:
            d.free()
        return out, dst

    def reference(self, inp):
        B, n = inp["x"].shape
        flat = inp["x"].ravel()
        rows = np.stack([flat[o: o + n] for o in self._offsets(inp)])
        return rows, np.concatenate((rows.ravel(), np.full(PAD, SENT)))

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


class subtract(Rows, DevCell):
    entries = ("itd_subtract_f64", "itd_copy")
    buffers = ()
    decided_by = "k_subtract: one thread per sample"
    staged = ("x",)

    def arrays(self, inp):
        B, n = inp["x"].shape
        return dict(x=inp["x"], out=np.full(n + PAD, SENT))

    def enqueue(self, eng, d, inp, stream):
        n = inp["n"]
        eng.subtract_dev(d.ptr("x"), d.ptr("x") + 8 * n, d.ptr("out"), n, stream)

    def collect(self, eng, d, inp):
        return (d.get("out"),)

    def reference(self, inp):
        return (np.concatenate((inp["x"][0] - inp["x"][1], np.full(PAD, SENT))),)

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


# ================================================================================================================================
# the half-wave family: instantaneous step, single waves, histogram, spectrum
# ================================================================================================================================
HW_KINDS = ("seams", "fam_quantised", "noise", "quantised", "fam_noise", "sine", "seams")


class HwRows:
    halfwave = True

    def make(self, size, seed):
        n, rows = self.dims(size)
        x = signals(n, rows, seed, HW_KINDS)
        with np.errstate(over="ignore"):
            return {"n": n, "x": x, "x32": x.astype(np.float32)}

    def reaches_working_branch(self, inp):
        return all(np.count_nonzero(et.structure(r)[0]) >= 10 for r in inp["x"])


def _tfe_hi(inp, key, b):
    def f():
        e = et.exact_tfe(inp[key][b].astype(np.float64))
        return e.amp, e.phase_hi, e.freq_hi
    return memo(inp, ("tfe", key, b), f)


class instantaneous_host(HwRows, Cell):
    entries = ("itd_instantaneous_host_f64",)
    buffers = HELPER_WS + ("d_cub (amp_bits)", "d_io_x", "d_io_rows")
    decided_by = "k_tfe_amp: atomicMax on the magnitudes' bits (an integer maximum), k_tfe_phase"

    def run(self, P, inp):
        return P.instantaneous(inp["x"][0])

    def reference(self, inp):
        return _tfe_hi(inp, "x", 0)

    def check(self, inp, got, P=None):
        tfe_check(inp["x"][0], got[0], got[1], got[2], self.name + " " + inp["size"])


class instantaneous_dev(HwRows, DevCell):
    """itd_instantaneous_f64 on device buffers: it reads helper_ws().tbase, left there by its own scan's k_compact."""
    entries = ("itd_instantaneous_f64", "itd_copy")
    buffers = HELPER_WS + ("d_cub (amp_bits)",)
    decided_by = "k_tfe_amp, k_tfe_phase"
    staged = ("x",)

    def arrays(self, inp):
        n = inp["n"]
        return dict(x=inp["x"][1], a=np.full(n + PAD, SENT), p=np.full(n + PAD, SENT), f=np.full(n + PAD, SENT))

    def enqueue(self, eng, d, inp, stream):
        assert eng._L.itd_instantaneous_f64(eng._h, d.ptr("x"), inp["n"], d.ptr("a"), d.ptr("p"), d.ptr("f"), stream) == OK

    def collect(self, eng, d, inp):
        return d.get("a"), d.get("p"), d.get("f")

    def reference(self, inp):
        tail = np.full(PAD, SENT)
        return tuple(np.concatenate((v, tail)) for v in _tfe_hi(inp, "x", 1))

    def check(self, inp, got, P=None):
        n = inp["n"]
        assert all(pad_ok(g, n) for g in got)
        tfe_check(inp["x"][1], got[0][:n], got[1][:n], got[2][:n], self.name + " " + inp["size"])


class instantaneous_batch(HwRows, DevCell):
    entries = ("itd_instantaneous_batch_f64", "itd_instantaneous_batch_f32", "itd_copy")
    buffers = ("d_ib",)
    decided_by = "k_inst_tile / k_inst_carry / k_inst_apply: integer maxima, fixed order (its own test asserts call-to-call bits)"
    staged = ("x", "x32")

    def arrays(self, inp):
        R, n = inp["x"].shape
        a = dict(x=inp["x"], x32=inp["x32"], info=np.full(2 * R + PAD, ISENT, np.int32))
        for k in ("a", "p", "f", "a32", "p32", "f32"):
            a[k] = np.full(R * n + PAD, SENT)
        return a

    def enqueue(self, eng, d, inp, stream):
        R, n = inp["x"].shape
        eng.instantaneous_batch_dev(d.ptr("x"), np.float64, n, R, n, d.ptr("a"), d.ptr("p"), d.ptr("f"), n, False, d.ptr("info"), stream)
        eng.instantaneous_batch_dev(d.ptr("x32"), np.float32, n, R, n, d.ptr("a32"), d.ptr("p32"), d.ptr("f32"), n, False,
                                    d.ptr("info") + 4 * R, stream)

    def collect(self, eng, d, inp):
        return tuple(d.get(k) for k in ("a", "p", "f", "a32", "p32", "f32", "info"))

    def _info(self, inp):
        R = inp["x"].shape[0]
        info = np.full(2 * R + PAD, ISENT, np.int32)
        info[:R] = [np.count_nonzero(et.structure(r)[0]) for r in inp["x"]]
        info[R: 2 * R] = [np.count_nonzero(et.structure(r.astype(np.float64))[0]) for r in inp["x32"]]
        return info

    def reference(self, inp):
        R = inp["x"].shape[0]
        tail = np.full(PAD, SENT)
        out = []
        for key in ("x", "x32"):
            t = [_tfe_hi(inp, key, b) for b in range(R)]
            out += [np.concatenate([t[b][k] for b in range(R)] + [tail]) for k in range(3)]
        return tuple(out) + (self._info(inp),)

    def check(self, inp, got, P=None):
        R, n = inp["x"].shape
        _same(got[6], self._info(inp), "crossing counts")
        for j, key in enumerate(("x", "x32")):
            a, p, f = got[3 * j: 3 * j + 3]
            assert pad_ok(a, R * n) and pad_ok(p, R * n) and pad_ok(f, R * n)
            for b in range(R):
                s = slice(b * n, (b + 1) * n)
                tfe_check(inp[key][b].astype(np.float64), a[s], p[s], f[s], "%s %s row %d" % (self.name, key, b))


class waves(HwRows, DevCell):
    entries = ("itd_waves_batch_f64", "itd_waves_batch_f32", "itd_copy")
    buffers = ("d_wv",)
    decided_by = "k_wave_tile / k_wave_carry / k_wave_table (itd_halfwave.hpp: integer atomicMax / atomicMin in LDS)"
    staged = ("x", "x32")

    def arrays(self, inp):
        R, n = inp["x"].shape
        a = dict(x=inp["x"], x32=inp["x32"], count=np.full(2 * R + PAD, ISENT, np.int32), info=np.full(2 * R + PAD, ISENT, np.int32))
        for sfx in ("", "32"):
            for k in ("start", "length", "peak"):
                a[k + sfx] = np.full(R * (n - 1) + PAD, -1, np.int32)
            a["value" + sfx] = np.full(R * (n - 1) + PAD, SENT)
        return a

    def enqueue(self, eng, d, inp, stream):
        R, n = inp["x"].shape
        for j, (key, dt, sfx) in enumerate((("x", np.float64, ""), ("x32", np.float32, "32"))):
            eng.waves_batch_dev(d.ptr(key), dt, n, R, n, d.ptr("start" + sfx), d.ptr("length" + sfx), d.ptr("peak" + sfx), d.ptr("value" + sfx),
                                n - 1, n - 1, d.ptr("count") + 4 * R * j, d.ptr("info") + 4 * R * j, stream)

    def collect(self, eng, d, inp):
        return tuple(d.get(k + s) for s in ("", "32") for k in ("start", "length", "peak", "value")) + (d.get("count"), d.get("info"))

    def reference(self, inp):
        R, n = inp["x"].shape
        out = []
        count, info = np.full(2 * R + PAD, ISENT, np.int32), np.full(2 * R + PAD, ISENT, np.int32)
        for j, key in enumerate(("x", "x32")):
            bufs = [np.full(R * (n - 1) + PAD, -1, np.int32) for _ in range(3)] + [np.full(R * (n - 1) + PAD, SENT)]
            for b in range(R):
                t = memo(inp, ("tab", key, b), lambda: waves_ref.ref_table(inp[key][b].astype(np.float64)))
                for buf, col in zip(bufs, t):
                    buf[b * (n - 1): b * (n - 1) + len(col)] = col
                count[R * j + b], info[R * j + b] = len(t[0]), len(t[0]) - 1
            out += bufs
        return tuple(out) + (count, info)

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


def _bounds(x):
    """One set per row: amplitudes above a third of the row's largest, lengths 2 .. 40."""
    return np.stack([np.array([np.max(np.abs(r)) / 3.0, np.inf, 2.0, 40.0]) for r in x])


class wave_filter(HwRows, DevCell):
    entries = ("itd_wave_filter_batch_f64", "itd_wave_filter_batch_f32", "itd_copy")
    buffers = ("d_wv",)
    decided_by = "k_wave_tile / k_wave_carry / k_wave_filter"
    staged = ("x", "x32", "bounds")

    def arrays(self, inp):
        R, n = inp["x"].shape
        return dict(x=inp["x"], x32=inp["x32"], bounds=_bounds(inp["x"]), out=np.full(R * n + PAD, SENT),
                    out32=np.full(R * n + PAD, np.float32(-7.25e30), np.float32), info=np.full(2 * R + PAD, ISENT, np.int32))

    def enqueue(self, eng, d, inp, stream):
        R, n = inp["x"].shape
        eng.wave_filter_batch_dev(d.ptr("x"), np.float64, n, R, n, d.ptr("bounds"), 4, d.ptr("out"), n, False, d.ptr("info"), stream)
        eng.wave_filter_batch_dev(d.ptr("x32"), np.float32, n, R, n, d.ptr("bounds"), 0, d.ptr("out32"), n, True, d.ptr("info") + 4 * R, stream)

    def collect(self, eng, d, inp):
        return d.get("out"), d.get("out32"), d.get("info")

    def reference(self, inp):
        R, n = inp["x"].shape
        bd = _bounds(inp["x"])
        out = np.concatenate([waves_ref.ref_filter(inp["x"][b], bd[b]) for b in range(R)] + [np.full(PAD, SENT)])
        with np.errstate(over="ignore"):
            o32 = np.concatenate([waves_ref.ref_filter(inp["x32"][b].astype(np.float64), bd[0]).astype(np.float32) for b in range(R)]
                                 + [np.full(PAD, np.float32(-7.25e30), np.float32)])
        info = np.full(2 * R + PAD, ISENT, np.int32)
        info[:R] = [np.count_nonzero(et.structure(r)[0]) for r in inp["x"]]
        info[R: 2 * R] = [np.count_nonzero(et.structure(r.astype(np.float64))[0]) for r in inp["x32"]]
        return out, o32, info

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


class wave_hist(HwRows, DevCell):
    entries = ("itd_wave_hist_batch_f64", "itd_wave_hist_batch_f32", "itd_copy")
    buffers = ("d_wv",)
    decided_by = "k_wave_hist: integer adds (its own test asserts call-to-call bits)"
    staged = ("x", "x32", "ae", "le")
    HOP, AB, LB = 512, 6, 5

    def _edges(self, inp):
        top = float(np.max(np.abs(inp["x"])))
        return np.linspace(0.0, top * 0.75, self.AB + 1), np.array([1.0, 2.0, 3.0, 5.0, 9.0, 64.0])

    def arrays(self, inp):
        R, n = inp["x"].shape
        T = -(-n // self.HOP)
        cells = T * self.AB * self.LB
        ae, le = self._edges(inp)
        a = dict(x=inp["x"], x32=inp["x32"], ae=ae, le=le, info=np.full(2 * R + PAD, ISENT, np.int32))
        for s in ("", "32"):
            a["count" + s] = np.full(R * cells + PAD, ISENT, np.int32)
            a["samples" + s] = np.full(R * cells + PAD, ISENT, np.int32)
            a["outside" + s] = np.full(R * T + PAD, ISENT, np.int32)
        return a

    def enqueue(self, eng, d, inp, stream):
        R, n = inp["x"].shape
        cells = -(-n // self.HOP) * self.AB * self.LB
        for j, (key, dt, s) in enumerate((("x", np.float64, ""), ("x32", np.float32, "32"))):
            eng.wave_hist_batch_dev(d.ptr(key), dt, n, R, n, d.ptr("ae"), 0, self.AB, d.ptr("le"), 0, self.LB, self.HOP, d.ptr("count" + s),
                                    d.ptr("samples" + s), cells, d.ptr("outside" + s), d.ptr("info") + 4 * R * j, stream)

    def collect(self, eng, d, inp):
        return tuple(d.get(k + s) for s in ("", "32") for k in ("count", "samples", "outside")) + (d.get("info"),)

    def reference(self, inp):
        R, n = inp["x"].shape
        ae, le = self._edges(inp)
        tail = np.full(PAD, ISENT, np.int32)
        out = []
        info = np.full(2 * R + PAD, ISENT, np.int32)
        for j, key in enumerate(("x", "x32")):
            h = [wave_hist_ref.ref_hist(inp[key][b].astype(np.float64), ae, le, self.HOP) for b in range(R)]
            out += [np.concatenate([h[b][k].ravel() for b in range(R)] + [tail]) for k in range(3)]
            info[R * j: R * (j + 1)] = [np.count_nonzero(et.structure(inp[key][b].astype(np.float64))[0]) for b in range(R)]
        return tuple(out) + (info,)

    def check(self, inp, got, P=None):
        same_results(got, self.reference(inp), self.name)


class tfe_spectrum(HwRows, DevCell):
    """itd_tfe_spectrum_f64 / _f32, held to the numpy statement on the instantaneous amplitude and frequency the same run delivers
    (themselves held to the exact reference)."""
    entries = ("itd_tfe_spectrum_f64", "itd_tfe_spectrum_f32", "itd_instantaneous_batch_f64", "itd_instantaneous_batch_f32", "itd_copy")
    buffers = ("d_ts", "d_ib")
    decided_by = "k_spectrum_*: the order of every sum is part of the definition, no global atomics (its own test asserts bits)"
    staged = ("x", "x32", "edges")
    model = True
    F, HOP, WEIGHT = 16, 256, "energy"
    FORMS = (("x", np.float64, ""), ("x32", np.float32, "32"))

    def arrays(self, inp):
        R, n = inp["x"].shape
        T = -(-n // self.HOP)
        a = dict(x=inp["x"], x32=inp["x32"], edges=sr.uniform_edges(self.F), info=np.full(2 * R + PAD, ISENT, np.int32))
        for s in ("", "32"):
            a["spec" + s] = np.full(R * T * self.F + PAD, SENT)
            a["outside" + s] = np.full(R * T + PAD, ISENT, np.int32)
            a["a" + s], a["f" + s] = np.full(R * n + PAD, SENT), np.full(R * n + PAD, SENT)
        return a

    def enqueue(self, eng, d, inp, stream):
        R, n = inp["x"].shape
        T = -(-n // self.HOP)
        w = sr.WEIGHTS.index(self.WEIGHT)
        for j, (key, dt, s) in enumerate(self.FORMS):
            eng.instantaneous_batch_dev(d.ptr(key), dt, n, R, n, d.ptr("a" + s), None, d.ptr("f" + s), n, False, None, stream)
            eng.tfe_spectrum_dev(d.ptr(key), dt, n, R, n, d.ptr("edges"), self.F, self.HOP, w, d.ptr("spec" + s), T * self.F,
                                 d.ptr("outside" + s), d.ptr("info") + 4 * R * j, stream)

    def collect(self, eng, d, inp):
        return tuple(d.get(k + s) for s in ("", "32") for k in ("spec", "outside", "a", "f")) + (d.get("info"),)

    def _spectra(self, inp, A, f):
        """(spectrum, outside) buffers of the rows with amplitude A[R, n] and frequency f[R, n]."""
        edges = sr.uniform_edges(self.F)
        s = [sr.spectrum_ref(a_, f_, edges, self.HOP, self.WEIGHT) for a_, f_ in zip(A, f)]
        return (np.concatenate([v[0].ravel() for v in s] + [np.full(PAD, SENT)]),
                np.concatenate([v[1].ravel() for v in s] + [np.full(PAD, ISENT, np.int32)]))

    def reference(self, inp):
        """The model: the numpy statement on the exact reference's amplitude and frequency."""
        R, n = inp["x"].shape
        tail = np.full(PAD, SENT)
        out = []
        for key, _, _ in self.FORMS:
            t = [_tfe_hi(inp, key, b) for b in range(R)]
            A, f = [v[0] for v in t], [v[2] for v in t]
            out += list(self._spectra(inp, A, f)) + [np.concatenate(A + [tail]), np.concatenate(f + [tail])]
        return tuple(out) + (instantaneous_batch._info(self, inp),)

    def check(self, inp, got, P=None):
        from test_gpu_instantaneous_exact import F_TOL
        R, n = inp["x"].shape
        _same(got[8], instantaneous_batch._info(self, inp), "crossing counts")
        for j, (key, _, _) in enumerate(self.FORMS):
            spec, outside, a, f = got[4 * j: 4 * j + 4]
            assert pad_ok(a, R * n) and pad_ok(f, R * n)
            A, Fq = a[: R * n].reshape(R, n), f[: R * n].reshape(R, n)
            for b in range(R):                          # amplitude exact, frequency inside its bound
                e = memo(inp, ("ex", key, b), lambda: et.exact_tfe(inp[key][b].astype(np.float64)))
                _bits(A[b], e.amp, "%s amplitude row %d" % (key, b))
                assert e.freq_err(Fq[b]).max() <= F_TOL, "%s frequency row %d" % (key, b)
            want = self._spectra(inp, A, Fq)
            _same(spec, want[0], key + ": spectrum = the numpy statement on the delivered amplitude and frequency")
            _same(outside, want[1], key + ": outside")


# ================================================================================================================================
# the FFT, the selectors, the cascade
# ================================================================================================================================
FFT_BUFFERS = ("d_fft_x", "d_fft_y", "d_fft_a", "d_fft_b", "fft_chirp_n")


class fft(Cell):
    entries = ("itd_debug_fft_f64",)
    buffers = FFT_BUFFERS
    decided_by = "k_fft_lds / four-step / Bluestein: butterflies in a fixed order, no atomics on values"

    def make(self, size, seed):
        n, rows = self.dims(size)
        rng = np.random.default_rng([seed, n])
        z = rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))
        z[-1] = signals(n, 1, seed)[0]
        return {"n": n, "z": z}

    def run(self, P, inp):
        return mod("fourier").debug_fft(inp["z"]), mod("fourier").debug_fft(inp["z"], inverse=True)

    def reference(self, inp):
        return np.fft.fft(inp["z"], axis=1), np.fft.ifft(inp["z"], axis=1)

    def check(self, inp, got, P=None):
        assert fc.LONGDOUBLE_OK, fc.LONGDOUBLE_WHY
        for g, inv in zip(got, (False, True)):
            ref, u, y_fft, y_seq, idx = memo(inp, ("yard", inv), lambda: fc.yardsticks(inp["z"], inv))
            err, limit = fc.err_units(g, ref, u), fc.bound(y_fft, y_seq)
            assert (err <= limit).all(), "%s inverse %d: %s units, allowed %s" % (self.name, inv, err, limit)


class selectors(DevCell):
    """Both Fourier mode selectors on designed rows (every comparison of the rules decided by a margin above 2^-40)."""
    entries = ("itd_fourier_mode_any_f64", "itd_fourier_mode_valid_f64", "itd_copy")
    buffers = FFT_BUFFERS + ("d_fft_rec",)
    decided_by = "the FFT kernels and k_fourier_select: one workgroup per row, integer decisions"
    staged = ("x",)

    def make(self, size, seed):
        n, rows = self.dims(size)
        x = []
        for r in range(rows):
            pm = n // 8 + 3 * r
            if r % 2 == 0:
                mags = fc._flat(n, seed + r, **{"k%d" % pm: 60.0, "k%d" % (pm // 2): 25.0, "k%d" % (2 * pm): 24.0})
            else:                                       # the runner-up right beside the peak: `any` rejects
                mags = fc._flat(n, seed + r, **{"k%d" % pm: 60.0, "k%d" % (pm + 1): 25.0, "k%d" % (pm // 2): 12.0})
            x.append(fc._row_of(mags, seed + 100 + r))
        return {"n": n, "x": np.stack(x)}

    def _expected(self, inp, rule):
        return memo(inp, ("exp", rule), lambda: [fc.expected(x, rule) for x in inp["x"]])

    def reaches_working_branch(self, inp):
        ok = True
        for rule in ("any", "valid"):
            e = self._expected(inp, rule)
            ok = ok and all(m > fc.MARGIN for _, m, _ in e) and any(rec[0] for rec, _, _ in e)
        return ok and any(not rec[0] for rec, _, _ in self._expected(inp, "any"))

    def arrays(self, inp):
        B, n = inp["x"].shape
        return dict(x=inp["x"], any=np.full(B * n + PAD, SENT), valid=np.full(B * n + PAD, SENT), rec=np.full(16 * B + PAD, ISENT, np.int32))

    def enqueue(self, eng, d, inp, stream):
        B, n = inp["x"].shape
        assert eng._L.itd_fourier_mode_any_f64(eng._h, d.ptr("x"), n, B, n, d.ptr("any"), n, d.ptr("rec"), stream) == OK
        assert eng._L.itd_fourier_mode_valid_f64(eng._h, d.ptr("x"), n, B, n, d.ptr("valid"), n, d.ptr("rec") + 32 * B, stream) == OK

    def collect(self, eng, d, inp):
        return d.get("any"), d.get("valid"), d.get("rec")

    def reference(self, inp):
        B, n = inp["x"].shape
        rec = np.full(16 * B + PAD, ISENT, np.int32)
        out = []
        for j, rule in enumerate(("any", "valid")):
            e = self._expected(inp, rule)
            out.append(np.concatenate([m for _, _, m in e] + [np.full(PAD, SENT)]))
            r = rec[8 * B * j: 8 * B * (j + 1)].reshape(B, 8)
            r[:, 6:] = 0
            r[:, :6] = [v for v, _, _ in e]
        return out[0], out[1], rec

    def check(self, inp, got, P=None):
        from test_gpu_fourier_selectors import MODE_TOL
        B, n = inp["x"].shape
        ref = self.reference(inp)
        _same(got[2], ref[2], "selector records")
        for j, rule in enumerate(("any", "valid")):
            assert pad_ok(got[j], B * n)
            for b, (rec, _, mode) in enumerate(self._expected(inp, rule)):
                g = got[j][b * n:(b + 1) * n]
                if not rec[0]:
                    assert (g == 0.0).all(), "%s row %d: rejected, but the mode is not all zero" % (rule, b)
                else:
                    err, tol = float(np.max(np.abs(g - mode))), MODE_TOL * float(np.max(np.abs(inp["x"][b])))
                    assert err <= tol, "%s row %d: mode off by %.3g, allowed %.3g" % (rule, b, err, tol)


CASCADE_SR, CASCADE_CAP = 421, 2


def _bands(n):
    """A caller's band plan (the entries take any): two retained knot lists, every 5th and every 23rd sample, the 0 behind them."""
    lists = [np.concatenate((np.arange(0, n - 1, step), [0])).astype(np.int64) for step in (5, 23)]
    return lists, [len(k) - 1 for k in lists]


def gpu_ops(P):
    def cubic(problem, knots, idx):
        return P.itd_baseline_extract_fast(problem, knots, idx)

    def select(row):
        modes, recs = mod("fourier").fourier_mode_batch(row[None, :], "any")
        return modes[0], recs[0]
    return cubic, select


def cpu_ops():
    from test_fourier_cpu import restate

    def select(row):
        rec, mode = restate(row, "any")
        return mode, rec
    return cpu_oracle.itd_baseline_extract_fast, select


class cascade(Cell):
    """The ITD-Fourier cascade on a caller's band plan, capped at two rounds: the host entry full and lean, the device entry."""
    entries = ("itd_fourier_cascade_host_f64", "itd_fourier_cascade_f64", "itd_fourier_modes_f64", "itd_copy")
    buffers = FFT_BUFFERS + ("d_fc", "d_fio", "d_fmodes", "d_fplan", "frec", "d_cub (the cubic operator's jobs)")
    decided_by = "k_band_step, k_fourier_apply, k_fourier_sum, k_copy_rows over the cubic's and the selector's kernels"
    model = True
    KEYS = ("rows", "acc", "rounds", "capped", "counts", "recs", "modes")

    def make(self, size, seed):
        n, rows = self.dims(size)
        rows = min(rows, 3)
        return {"n": n, "x": np.stack([cr.signal(n, CASCADE_SR, seed + b) for b in range(rows)])}

    def _flatten(self, res, lean):
        return [np.zeros(0) if res[k] is None else np.asarray(res[k]) for k in self.KEYS if not (lean and k == "modes") and not (not lean and k == "acc")]

    def run(self, P, inp):
        from test_gpu_fourier_cascade import _dev_call, _host_call
        n = inp["n"]
        eng = eng_of(P, n)
        bands = _bands(n)
        out = []
        for lean in (False, True):
            out += self._flatten(_host_call(eng, inp["x"], CASCADE_SR, bands, lean, CASCADE_CAP), lean)
        rc, got = _dev_call(eng, inp["x"], CASCADE_SR, bands, False, CASCADE_CAP)
        assert rc == OK, rc
        return tuple(out + self._flatten(got, False))

    def _compose(self, inp, ops, tag):
        bands = _bands(inp["n"])
        return memo(inp, ("compose", tag), lambda: [cr.compose(x, CASCADE_SR, ops[0], ops[1], max_rounds=CASCADE_CAP, bands=bands) for x in inp["x"]])

    def _as_call(self, wants, lean):
        """The compositions of the signals in the shape of a C call's result (records: signal, round, row, ...; by round, signal, row)."""
        recs, modes = [], []
        for b, w in enumerate(wants):
            for rec, mode in zip(w["records"], w["modes"]):
                recs.append((int(rec[0]), b, int(rec[1]), [b] + [int(v) for v in rec], mode))
        recs.sort(key=lambda t: t[:3])
        res = dict(rows=np.stack([w["rows"] for w in wants]), acc=np.stack([cr.lean_acc(w) for w in wants]) if lean else None,
                   rounds=np.array([w["rounds"] for w in wants], np.int32), capped=np.array([w["capped"] for w in wants], np.int32),
                   counts=np.array([len(w["modes"]) for w in wants], np.int64),
                   recs=np.array([t[3] for t in recs], np.int32).reshape(-1, 8),
                   modes=None if lean else np.stack([t[4] for t in recs]) if recs else np.zeros((0, wants[0]["rows"].shape[1])))
        return self._flatten(res, lean)

    def reference(self, inp, ops=None):
        wants = self._compose(inp, ops or cpu_ops(), "gpu" if ops else "cpu")
        return tuple(self._as_call(wants, False) + self._as_call(wants, True) + self._as_call(wants, False))

    def check(self, inp, got, P=None):
        """The composition runs over the GPU's own single calls where there is a GPU (P: every decision is theirs, so bit for bit),
        over the CPU oracles for the model's own output."""
        same_results(got, self.reference(inp, gpu_ops(P) if P is not None else None), self.name)

    def reaches_working_branch(self, inp):
        return any(w["rounds"] >= 1 for w in self._compose(inp, cpu_ops(), "cpu"))


# ================================================================================================================================
# the streams: engines of their own, beside the shared one
# ================================================================================================================================
class streams_alongside(Cell):
    """A LevelsStream and a SpectrumStream pushed block by block while the shared engine runs tfe_spectrum of the same rows between
    the pushes: the streams own their engines and do not touch the shared one, nor it them."""
    entries = ("itd_tfe_spectrum_f64", "itd_instantaneous_batch_f64")
    buffers = ("d_ts", "d_ib", "(the streams' own memory)")
    decided_by = "k_levels_stream, k_spectrum_stream: fixed order (their own tests assert bits)"
    model = True
    halfwave = True
    L, LEVELS, F = 512, 3, 16

    def make(self, size, seed):
        n, rows = self.dims(size)
        nb = {"S": 3, "L": 5, "G": 8}[size]
        rows = min(rows, 3)
        rng = np.random.default_rng([seed, nb])
        return {"n": nb * self.L, "x": rng.standard_normal((rows, nb * self.L))}

    def run(self, P, inp):
        x = inp["x"]
        C, n = x.shape
        edges = sr.uniform_edges(self.F)
        lv = mod("streaming").LevelsStream(self.L, self.LEVELS, C)
        sp = P.SpectrumStream(self.L, C, horizon=self.L, edges=edges, hop=256, weight="energy")
        rows, exact, power, overlong = [], [], [], []
        whole = None
        try:
            for k in range(n // self.L):
                blk = x[:, k * self.L:(k + 1) * self.L]
                r = lv.push(blk)
                if r is not None:
                    rows.append(r[0]); exact.append(r[1])
                whole = P.tfe_spectrum(x, edges, 256, "energy")           # the shared engine, between the pushes
                s = sp.push(blk)
                if s is not None:
                    power.append(s.power); overlong.append(s.overlong)
            while True:
                r = lv.flush(flat=False)
                if r is None:
                    break
                rows.append(r[0]); exact.append(r[1])
            while True:
                s = sp.flush()
                if s is None:
                    break
                power.append(s.power.reshape(C, -1, self.F)); overlong.append(s.overlong.reshape(C, -1))
        finally:
            lv.close()
            sp.close()
        a, f = P.instantaneous_batch(x, want=("amplitude", "frequency"))
        return (np.concatenate(rows, axis=2), np.stack(exact, axis=1).astype(np.uint8), np.concatenate([p.reshape(C, -1, self.F) for p in power], axis=1),
                np.concatenate([o.reshape(C, -1) for o in overlong], axis=1).astype(np.int32), whole.power, a, f)

    def _levels(self, inp):
        from test_levels_stream_cpu import levels_composition
        return memo(inp, "lv", lambda: levels_composition(inp["x"], self.L, self.LEVELS))

    def reference(self, inp):
        from test_gpu_tfe import numpy_tfe
        rows, flags, _ = self._levels(inp)
        t = [numpy_tfe(r) for r in inp["x"]]
        A, f = np.stack([v[0] for v in t]), np.stack([v[2] for v in t])
        spec = np.stack([sr.spectrum_ref(a_, f_, sr.uniform_edges(self.F), 256, "energy")[0] for a_, f_ in zip(A, f)])
        return rows, flags.astype(np.uint8), spec, np.zeros(spec.shape[:2], np.int32), spec, A, f

    def check(self, inp, got, P=None):
        rows, flags, finite = self._levels(inp)
        assert finite
        _bits(got[0], rows, "LevelsStream rows = the composition of the block-wise oracle")
        _same(got[1], flags.astype(np.uint8), "LevelsStream flags")
        assert not got[3].any(), "a half wave of white noise longer than a block"
        _bits(got[2], got[4], "SpectrumStream = tfe_spectrum of the concatenated rows")
        want = np.stack([sr.spectrum_ref(a_, f_, sr.uniform_edges(self.F), 256, "energy")[0] for a_, f_ in zip(got[5], got[6])])
        _bits(got[4], want, "tfe_spectrum = the numpy statement on the delivered amplitude and frequency")
        for b, x in enumerate(inp["x"]):
            e = memo(inp, ("ex", b), lambda: et.exact_tfe(x))
            _bits(got[5][b], e.amp, "amplitude row %d" % b)


# ================================================================================================================================
# the registry
# ================================================================================================================================
CELLS = {}
for _c in (decompose_host, decompose_rows32_host, decompose_select_host, decompose_dev, decompose_batch,
           detect_host, detect_dev, extract_host, extract_dev, knot_values_host, knot_values_dev,
           cubic_host, cubic_dev, iq, cubic_batch, detect_batch, extract_batch, count_knots,
           spline_serial, spline_parallel, spline2, crossways, wpe, meitd_one_launch, meitd_host_driven, meitd_batch, gather_rows, subtract,
           instantaneous_host, instantaneous_dev, instantaneous_batch, waves, wave_filter, wave_hist, tfe_spectrum,
           fft, selectors, cascade, streams_alongside):
    CELLS[_c.__name__] = _c()
NAMES = tuple(CELLS)

# Operators compared by their rule alone instead of bit for bit with a fresh engine.  None: the library has no floating-point atomic
# (every atomic* in pyitd_amd/csrc is on an integer: counts, flags, tickets, magnitudes' bit patterns) and every reduction of values
# runs in an order fixed by the data's layout (Cell.decided_by names the kernel that settles it for each cell).
BY_RULE = {}


def fresh_engines(P):
    """Forget the process's engines: the next call creates new ones (what "fresh" means)."""
    mod("meitd").release()
    P.release_engines()


# ================================================================================================================================
# refusing calls: each returns its documented status, writes nothing it was given, leaves nothing behind
# ================================================================================================================================
def _nan_row(n, seed):
    x = signals(n, 1, seed, ("noise",))[0].copy()
    x[n // 2] = np.nan
    return x


def refuse_nan_cubic(P, n):
    """A row with a NaN: the natural cubic (detected knots), its I/Q form, the spline flavour and the instantaneous step answer
    ITD_ERR_NONFINITE."""
    eng = eng_of(P, n)
    x = _nan_row(n, 1)
    iqz = np.empty(2 * n)
    iqz[0::2], iqz[1::2] = x, x[::-1]
    d = DevArrays(eng, x=x, iq=iqz, o=np.full(n + PAD, SENT), o2=np.full(n + PAD, SENT), o3=np.full(n + PAD, SENT))
    try:
        g = _i64(-5)
        L, h = eng._L, eng._h
        assert L.itd_baseline_extract_cubic_f64(h, d.ptr("x"), n, None, 0, d.ptr("o"), ctypes.byref(g), None) == NONFINITE
        assert L.itd_baseline_extract_iq_f64(h, d.ptr("iq"), n, None, 0, d.ptr("o"), ctypes.byref(g), None) == NONFINITE
        assert L.itd_baseline_extract_spline_f64(h, d.ptr("x"), n, 1, n, 0, d.ptr("o"), n, d.ptr("o2"), n, None, None) == NONFINITE
        assert L.itd_instantaneous_f64(h, d.ptr("x"), n, d.ptr("o3"), None, None, None) == NONFINITE
        assert np.all(d.get("o3") == SENT), "the refused instantaneous step wrote its amplitude"
    finally:
        d.free()


def refuse_nan_cascade(P, n):
    """A signal with a NaN: the cascade's host entry answers ITD_ERR_NONFINITE and writes nothing."""
    eng = eng_of(P, n)
    lists, idxs = _bands(n)
    knots, idx = np.ascontiguousarray(np.concatenate(lists)), np.asarray(idxs, np.int64)
    x = np.stack((signals(n, 1, 2, ("noise",))[0], _nan_row(n, 3)))
    rows = np.full((2, 3, n), SENT)
    rounds, capped, counts = np.full(2, -1, np.int32), np.full(2, -1, np.int32), np.full(2, -1, np.int64)
    rc = eng._L.itd_fourier_cascade_host_f64(eng._h, _p(x), n, 2, float(CASCADE_SR), 2, _p(knots), _p(idx), 0, CASCADE_CAP, _p(rows), None,
                                             _p(rounds), _p(capped), _p(counts))
    assert rc == NONFINITE, rc
    assert np.all(rows == SENT), "a refused cascade wrote its rows"


def refuse_nan_batched(P, n):
    """A NaN row among finite ones in the half-wave wrappers: ITDError (non-finite) naming the row."""
    x = np.stack((signals(n, 1, 4, ("noise",))[0], _nan_row(n, 5)))
    for call in (lambda: P.instantaneous_batch(x), lambda: P.tfe_spectrum(x, sr.uniform_edges(8), 256), lambda: P.single_waves(x),
                 lambda: P.wave_filter(x, amplitude=(0.1, np.inf))):
        try:
            call()
        except P.ITDError as err:
            assert err.status == NONFINITE, err.args
        else:
            raise AssertionError("a row with a NaN was accepted")


def refuse_bad_list(P, n):
    """A knot list that does not increase: ITD_ERR_INVALID_ARG from the device and the host form, the baseline untouched."""
    eng = eng_of(P, n)
    x = signals(n, 1, 6, ("noise",))[0]
    lst = np.array([0, 10, 10, 50, 0], np.int32)
    d = DevArrays(eng, x=x, e=lst, o=np.full(n + PAD, SENT))
    try:
        g = _i64(-5)
        assert eng._L.itd_baseline_extract_cubic_f64(eng._h, d.ptr("x"), n, d.ptr("e"), 4, d.ptr("o"), ctypes.byref(g), None) == INVALID
        assert np.all(d.get("o") == SENT), "a refused call wrote its baseline"
    finally:
        d.free()
    base = np.full(n + PAD, SENT)
    bad = np.array([0, 3, -1, 9, 12, 15], np.int64)
    assert eng._L.itd_baseline_extract_cubic_host_f64(eng._h, _p(x), n, _p(bad), 5, _p(base), ctypes.byref(g), None) == INVALID
    assert np.all(base == SENT)


def refuse_n_over_max(P, n):
    """n beyond the engine's max_n: ITD_ERR_INVALID_ARG before anything is enqueued."""
    eng = eng_of(P, n)
    big = eng.max_n + 1
    x = signals(n, 1, 7, ("noise",))[0]
    d = DevArrays(eng, x=x, o=np.full(n + PAD, SENT), o2=np.full(n + PAD, SENT), kn=np.full(n + PAD, ISENT, np.int32))
    try:
        m = _i64(-5)
        L, h = eng._L, eng._h
        assert L.itd_baseline_extract_f64(h, d.ptr("x"), big, d.ptr("o"), d.ptr("o2"), None, ctypes.byref(m), None) == INVALID
        assert L.itd_detect_f64(h, d.ptr("x"), big, 0, d.ptr("kn"), ctypes.byref(m), None) == INVALID
        assert L.itd_baseline_extract_cubic_f64(h, d.ptr("x"), big, None, 0, d.ptr("o"), ctypes.byref(m), None) == INVALID
        assert L.itd_instantaneous_f64(h, d.ptr("x"), big, d.ptr("o"), None, None, None) == INVALID
        assert L.itd_decompose_f64(h, d.ptr("x"), big, 1, big, M, d.ptr("o"), None, None) == INVALID
        assert np.all(d.get("o") == SENT) and np.all(d.get("o2") == SENT) and np.all(d.get("kn") == ISENT)
    finally:
        d.free()


def refuse_too_few_knots(P, n):
    """Too few knots: a caller's list with idx = 1 is ITD_ERR_INVALID_ARG; a ramp has no knot of its own — the detected form reports
    the count and leaves the baseline untouched (itd.cpp:170), and MEITD's extraction is refused as scipy refuses it."""
    eng = eng_of(P, n)
    ramp = np.linspace(-1.0, 2.0, n)
    d = DevArrays(eng, x=ramp, e=np.array([0, 0], np.int32), o=np.full(n + PAD, SENT))
    try:
        g = _i64(-5)
        assert eng._L.itd_baseline_extract_cubic_f64(eng._h, d.ptr("x"), n, d.ptr("e"), 1, d.ptr("o"), ctypes.byref(g), None) == INVALID
        assert eng._L.itd_baseline_extract_cubic_f64(eng._h, d.ptr("x"), n, None, 0, d.ptr("o"), ctypes.byref(g), None) == OK
        assert g.value < 2 and np.all(d.get("o") == SENT), "fewer than two knots leave the buffer alone"
    finally:
        d.free()
    try:
        mod("spline").itd_baseline_extract_spline(ramp)
    except TypeError:
        pass
    else:
        raise AssertionError("an extraction with fewer than two knots was accepted")


REFUSALS = {f.__name__: f for f in (refuse_nan_cubic, refuse_nan_cascade, refuse_nan_batched, refuse_bad_list, refuse_n_over_max,
                                    refuse_too_few_knots)}


# ================================================================================================================================
# the schedules: deterministic functions of a seed
# ================================================================================================================================
def pair_schedule():
    """Test (a): for every first cell A, every second cell B: A(L); B(S), then A(S); B(L).  [(A, sizeA, B, sizeB)]"""
    out = []
    for a in NAMES:
        for b in NAMES:
            out.append((a, "L", b, "S"))
            out.append((a, "S", b, "L"))
    return out


WALKS, WALK_CALLS = 8, 60
SOLVER_POKES = (0, 1, 2)
FUSE_MIN_POKES = (65536, 2 << 20)


def _cut(flat, calls):
    return [flat[k:k + calls] for k in range(0, len(flat), calls)]


def _transitions(flat, calls):
    out = set()
    for w in _cut(flat, calls):
        out |= {(a[1], b[1], b[0]) for a, b in zip(w[:-1], w[1:])}
    return out


def walk_schedule(seed=0, walks=WALKS, calls=WALK_CALLS):
    """Test (b): `walks` walks of `calls` calls.  A step is a dict: cell, size, and what is done in front of it — refusal (a name of
    REFUSALS or None), solver and fuse_min (the engine's sticky settings poked to these values, or None).  The concatenated walks
    start with four passes over one seeded permutation of the cells, the sizes S, S, L, L, ... shifted by one per pass, which makes
    nearly every cell the second call of each of S->S, S->L, L->L and L->S; the transitions the passes' ends and the cuts between
    walks cost are added as pairs behind them, and the rest is drawn, sometimes at G."""
    rng = np.random.default_rng([20221, seed])
    N = len(NAMES)
    perm = rng.permutation(N)
    flat = [(NAMES[c], "SSLL"[(i + p) % 4]) for p in range(4) for i, c in enumerate(perm)]
    if len(flat) % 2:
        flat.append((NAMES[int(rng.integers(0, N))], "S"))
    need = {(a, b, c) for a in "SL" for b in "SL" for c in NAMES}
    for a, b, c in sorted(need - _transitions(flat, calls)):        # (an even offset: a pair never straddles a cut)
        flat += [(NAMES[int(rng.integers(0, N))], a), (c, b)]
    total = walks * calls
    assert len(flat) <= total, "the walks are too short for %d cells" % N
    while len(flat) < total:
        size = "G" if rng.random() < 0.06 else ("S", "L")[int(rng.integers(0, 2))]
        flat.append((NAMES[int(rng.integers(0, N))], size))
    refusals = list(REFUSALS)
    steps = []
    for cell, size in flat:
        steps.append({"cell": cell, "size": size,
                      "refusal": refusals[int(rng.integers(0, len(refusals)))] if rng.random() < 0.25 else None,
                      "solver": int(rng.choice(SOLVER_POKES)) if rng.random() < 0.5 else None,
                      "fuse_min": int(rng.choice(FUSE_MIN_POKES)) if rng.random() < 0.3 else None})
    return _cut(steps, calls)


def refusal_schedule():
    """Test (c): every refusing call in front of every family, the family at S.  [(refusal, cell)]"""
    return [(r, c) for r in REFUSALS for c in NAMES]


def size_transitions(steps):
    """{(previous size, size, cell)} of consecutive calls of one walk."""
    return {(a["size"], b["size"], b["cell"]) for a, b in zip(steps[:-1], steps[1:])}
