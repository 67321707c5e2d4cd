"""What a many-row call hands the engine, pinned without a GPU: the five operators of pyitd_amd.batch (instantaneous_batch,
tfe_spectrum, single_waves, wave_filter, wave_histogram) and its four numpy-only helpers run on numpy rows over a host-backed
DeviceBuffer and an engine that records each *_dev call.  Pinned: the entry and its plain arguments, every buffer's size as
include/pyitd_hip.h documents it, that no buffer outlives the call (normal return, a refused row, an engine that raises), and the
shapes and dtypes that come back.
"""
import ctypes
import inspect

import numpy as np
import pytest

LEAD, N = (2, 3), 1030
R = 6
HOP, T = 512, 3
WAVES = 7                    # what the recording engine reports as every row's half-wave count


class HostBuffer:
    """DeviceBuffer on host memory: a numpy byte array whose ptr is its address; LIVE lists the buffers not yet freed."""
    LIVE = []

    def __init__(self, nbytes, device=0):
        self.device, self.nbytes = int(device), int(nbytes)
        self._mem = np.zeros(max(self.nbytes, 1), np.uint8)
        self.ptr = self._mem.ctypes.data
        HostBuffer.LIVE.append(self)

    def upload(self, a, offset=0):
        a = np.ascontiguousarray(a)
        assert 0 <= offset and offset + a.nbytes <= self.nbytes, "upload beyond the buffer"
        ctypes.memmove(self.ptr + offset, a.ctypes.data, a.nbytes)

    def download(self, out, offset=0):
        assert out.flags["C_CONTIGUOUS"] and 0 <= offset and offset + out.nbytes <= self.nbytes, "download beyond the buffer"
        ctypes.memmove(out.ctypes.data, self.ptr + offset, out.nbytes)
        return out

    def free(self):
        if self.ptr is not None:
            HostBuffer.LIVE.remove(self)
            self.ptr = None


class RecordingEngine:
    """Every *_dev entry of Engine under its own signature: records (name, arguments by name, size of every live buffer by
    pointer), zeroes the info words — `refuse`: writes -1 into one — and reports WAVES half waves per row; `fail`: raises."""
    ENTRIES = ("instantaneous_batch_dev", "tfe_spectrum_dev", "waves_batch_dev", "wave_filter_batch_dev", "wave_hist_batch_dev",
               "extract_batch_dev", "detect_batch_dev", "cubic_batch_dev")

    def __init__(self, refuse=False, fail=False):
        from pyitd_amd.engine import Engine
        self.calls, self.refuse, self.fail = [], refuse, fail
        for name in self.ENTRIES:
            setattr(self, name, self._entry(name, inspect.signature(getattr(Engine, name))))

    def _entry(self, name, sig):
        def call(*a, **k):
            if self.fail:
                raise RuntimeError("the engine failed")
            bound = sig.bind(self, *a, **k)
            bound.apply_defaults()
            args = dict(bound.arguments)
            self.calls.append((name, args, {b.ptr: b.nbytes for b in HostBuffer.LIVE}))
            rows = args["rows"] if "rows" in args else args["batch"]
            info = (ctypes.c_int32 * rows).from_address(args["info_ptr"])
            info[:] = [0] * rows
            if self.refuse:
                info[rows - 2] = -1
            if args.get("count_ptr"):
                (ctypes.c_int32 * rows).from_address(args["count_ptr"])[:] = [WAVES] * rows
        return call

    # what the two detecting helpers fall back to for a row whose info word is negative
    def baseline_extract_host(self, x, want_knots=False):
        return np.zeros_like(x), np.zeros_like(x), np.zeros(2, np.int64), None

    def detect_host(self, x, mode):
        return np.zeros(2, np.int64)


@pytest.fixture
def engine(monkeypatch):
    from pyitd_amd import _place, batch
    eng = RecordingEngine()
    HostBuffer.LIVE.clear()
    monkeypatch.setattr(batch, "_engine_for", lambda n, device=0: eng)
    monkeypatch.setattr(_place, "DeviceBuffer", HostBuffer)
    yield eng
    HostBuffer.LIVE.clear()


def rows_of(dtype):
    return np.random.default_rng(3).standard_normal(LEAD + (N,)).astype(dtype)


def f32(dt):
    return np.dtype(dt) == np.float32


AE, LE = np.array([0.0, 0.5, 1.0, np.inf]), np.array([1.0, 10.0, np.inf])          # 3 x 2 cells
AE_ROWS = np.arange(R)[:, None] + AE[None, :]                                        # one set per row, [R, 4]
EDGES = np.linspace(0.0, 0.5, 9)                                                     # 8 frequency bins
BOUNDS_ROWS = (np.linspace(0.0, 1.0, R).reshape(LEAD), 2.0)                          # amplitude lo per row


def check(args, sizes, plain, buffers):
    """The recorded call's plain arguments and the size of the buffer behind each pointer (None: the pointer must be None)."""
    for k, v in plain.items():
        assert args[k] == v, (k, args[k], v)
    for k, nbytes in buffers.items():
        if nbytes is None:
            assert args[k] is None, k
        else:
            assert sizes[args[k]] == nbytes, (k, sizes[args[k]], nbytes)
    assert len({args[k] for k, v in buffers.items() if v is not None}) == sum(v is not None for v in buffers.values())
    assert args["stream"] is None


# ---- the five operators: (call, what it must hand the engine, what it must return) per case --------------------------------
def op_instantaneous(idt, odt, want):
    import pyitd_amd

    def run():
        return pyitd_amd.instantaneous_batch(rows_of(idt), out_dtype=odt, want=want)

    def sent(calls):
        (name, args, sizes), = calls
        assert name == "instantaneous_batch_dev" and np.dtype(args["dtype"]) == idt
        out = R * N * np.dtype(odt).itemsize
        check(args, sizes, {"n": N, "rows": R, "row_stride": N, "out_stride": N, "out_f32": f32(odt)},
              {"rows_ptr": R * N * np.dtype(idt).itemsize, "info_ptr": 4 * R,
               "amp_ptr": out if "amplitude" in want else None, "phase_ptr": out if "phase" in want else None,
               "freq_ptr": out if "frequency" in want else None})

    def got(res):
        assert isinstance(res, tuple) and len(res) == len(want)
        for a in res:
            assert isinstance(a, np.ndarray) and a.shape == LEAD + (N,) and a.dtype == odt
    return run, sent, got


def op_spectrum(idt, weight):
    import pyitd_amd

    def run():
        return pyitd_amd.tfe_spectrum(rows_of(idt), EDGES, HOP, weight=weight)

    def sent(calls):
        (name, args, sizes), = calls
        assert name == "tfe_spectrum_dev" and np.dtype(args["dtype"]) == idt
        check(args, sizes, {"n": N, "rows": R, "row_stride": N, "bins": 8, "hop": HOP, "spec_stride": T * 8,
                            "weight": ("count", "amplitude", "energy").index(weight)},
              {"rows_ptr": R * N * np.dtype(idt).itemsize, "edges_ptr": 8 * 9, "spec_ptr": 8 * R * T * 8, "outside_ptr": 4 * R * T,
               "info_ptr": 4 * R})

    def got(res):
        assert type(res).__name__ == "Spectrum"
        assert res.power.shape == LEAD + (T, 8) and res.power.dtype == np.float64
        assert res.outside.shape == LEAD + (T,) and res.outside.dtype == np.int32
    return run, sent, got


def op_waves(idt, cap):
    import pyitd_amd
    width = WAVES if cap is None else cap

    def run():
        return pyitd_amd.single_waves(rows_of(idt), cap=cap)

    def sent(calls):
        assert [c[0] for c in calls] == ["waves_batch_dev"] * (2 if cap is None else 1)
        tables = ("start_ptr", "length_ptr", "peak_ptr", "value_ptr")
        common = {"rows_ptr": R * N * np.dtype(idt).itemsize, "count_ptr": 4 * R, "info_ptr": 4 * R}
        if cap is None:                                                  # the counting call: no table
            _, args, sizes = calls[0]
            check(args, sizes, {"n": N, "rows": R, "row_stride": N, "wave_stride": 0, "cap": 0}, {**common, **dict.fromkeys(tables)})
        _, args, sizes = calls[-1]
        assert np.dtype(args["dtype"]) == idt
        check(args, sizes, {"n": N, "rows": R, "row_stride": N, "wave_stride": width, "cap": width},
              {**common, "start_ptr": 4 * R * width, "length_ptr": 4 * R * width, "peak_ptr": 4 * R * width, "value_ptr": 8 * R * width})
        if cap is None:                                                  # one input, one count, one info for both calls
            assert all(calls[0][1][k] == args[k] for k in common)

    def got(res):
        assert type(res).__name__ == "Waves"
        assert res.count.shape == LEAD and res.count.dtype == np.int32 and (res.count == WAVES).all()
        for a in (res.start, res.length, res.peak):
            assert a.shape == LEAD + (width,) and a.dtype == np.int32 and (a == -1).all()      # the fill the engine did not touch
        assert res.value.shape == LEAD + (width,) and res.value.dtype == np.float64 and np.isnan(res.value).all()
    return run, sent, got


def op_filter(idt, odt, per_row):
    import pyitd_amd

    def run():
        return pyitd_amd.wave_filter(rows_of(idt), amplitude=BOUNDS_ROWS if per_row else (0.5, 2.0), length=(2, 40), out_dtype=odt)

    def sent(calls):
        (name, args, sizes), = calls
        assert name == "wave_filter_batch_dev" and np.dtype(args["dtype"]) == idt
        check(args, sizes, {"n": N, "rows": R, "row_stride": N, "bounds_stride": 4 if per_row else 0, "out_stride": N, "out_f32": f32(odt)},
              {"rows_ptr": R * N * np.dtype(idt).itemsize, "bounds_ptr": 32 * (R if per_row else 1),
               "out_ptr": R * N * np.dtype(odt).itemsize, "info_ptr": 4 * R})

    def got(res):
        assert isinstance(res, np.ndarray) and res.shape == LEAD + (N,) and res.dtype == odt
    return run, sent, got


def op_histogram(idt, hop, per_row):
    import pyitd_amd
    bins = 1 if hop is None else T
    ae = AE_ROWS.reshape(LEAD + (4,)) if per_row else AE

    def run():
        return pyitd_amd.wave_histogram(rows_of(idt), ae, LE, hop=hop)

    def sent(calls):
        (name, args, sizes), = calls
        assert name == "wave_hist_batch_dev" and np.dtype(args["dtype"]) == idt
        check(args, sizes, {"n": N, "rows": R, "row_stride": N, "aedges_stride": 4 if per_row else 0, "abins": 3, "ledges_stride": 0,
                            "lbins": 2, "hop": 1536 if hop is None else hop, "hist_stride": bins * 6},
              {"rows_ptr": R * N * np.dtype(idt).itemsize, "aedges_ptr": 8 * 4 * (R if per_row else 1), "ledges_ptr": 8 * 3,
               "count_ptr": 4 * R * bins * 6, "samples_ptr": 4 * R * bins * 6, "outside_ptr": 4 * R * bins, "info_ptr": 4 * R})

    def got(res):
        assert type(res).__name__ == "WaveHistogram"
        # (the recording engine's "half waves per row" lands in the count buffer: only shapes and dtypes are this test's)
        for a in (res.count, res.samples):
            assert a.shape == LEAD + (bins, 3, 2) and a.dtype == np.int32
        assert res.outside.shape == LEAD + (bins,) and res.outside.dtype == np.int32
    return run, sent, got


F4, F8 = np.dtype(np.float32), np.dtype(np.float64)
OPERATORS = {
    "instantaneous-f64": lambda: op_instantaneous(F8, F8, ("amplitude", "phase", "frequency")),
    "instantaneous-f32-to-f32": lambda: op_instantaneous(F4, F4, ("frequency", "amplitude")),
    "instantaneous-f32-phase": lambda: op_instantaneous(F4, F8, ("phase",)),
    "spectrum-f64": lambda: op_spectrum(F8, "energy"),
    "spectrum-f32-count": lambda: op_spectrum(F4, "count"),
    "waves-f64-counted": lambda: op_waves(F8, None),
    "waves-f32-cap": lambda: op_waves(F4, 9),
    "filter-f64": lambda: op_filter(F8, F8, False),
    "filter-f32-per-row-to-f32": lambda: op_filter(F4, F4, True),
    "histogram-f64": lambda: op_histogram(F8, None, False),
    "histogram-f32-hop-per-row": lambda: op_histogram(F4, HOP, True),
}


@pytest.mark.parametrize("case", sorted(OPERATORS))
def test_an_operator_hands_the_engine_what_the_header_documents(engine, case):
    run, sent, got = OPERATORS[case]()
    res = run()
    sent(engine.calls)
    got(res)
    assert not HostBuffer.LIVE


@pytest.mark.parametrize("case", sorted(OPERATORS))
def test_an_operator_frees_its_buffers_when_a_row_is_refused_or_the_engine_raises(engine, case):
    from pyitd_amd import ITDError
    run, _, _ = OPERATORS[case]()
    engine.refuse = True
    with pytest.raises(ITDError, match=r"NaN in rows \[%d\]" % (R - 2)):
        run()
    assert engine.calls and not HostBuffer.LIVE
    engine.refuse, engine.fail = False, True
    with pytest.raises(RuntimeError, match="the engine failed"):
        run()
    assert not HostBuffer.LIVE


def test_a_cap_below_the_count_is_refused_and_frees_its_buffers(engine):
    import pyitd_amd
    with pytest.raises(ValueError, match=r"cap = %d is less than the half waves of rows \[0, 1, 2, 3, 4, 5\] \(up to %d\)" % (WAVES - 1, WAVES)):
        pyitd_amd.single_waves(rows_of(F8), cap=WAVES - 1)
    assert not HostBuffer.LIVE


# ---- the four numpy-only helpers: rows [R, N], float64 on the device whatever comes in ---------------------------------------
def helper_extract(idt):
    from pyitd_amd.batch import itd_baseline_extract_batch

    def run():
        return itd_baseline_extract_batch(rows_of(idt).reshape(R, N), want_counts=True)

    def sent(calls):
        (name, args, sizes), = calls
        assert name == "extract_batch_dev"
        check(args, sizes, {"n": N, "batch": R, "x_stride": N, "rot_stride": N, "base_stride": N},
              {"x_ptr": 8 * R * N, "rot_ptr": 8 * R * N, "base_ptr": 8 * R * N, "info_ptr": 4 * R})

    def got(res):
        rot, base, counts = res
        assert rot.shape == base.shape == (R, N) and rot.dtype == base.dtype == np.float64
        assert counts.shape == (R,) and counts.dtype == np.int64
    return run, sent, got


def helper_count(idt):
    from pyitd_amd.batch import count_knots_batch

    def run():
        return count_knots_batch(rows_of(idt).reshape(R, N), mode=2)

    def sent(calls):
        (name, args, sizes), = calls
        assert name == "detect_batch_dev"
        check(args, sizes, {"n": N, "batch": R, "x_stride": N, "mode": 2, "idx_stride": 0},
              {"x_ptr": 8 * R * N, "idx_ptr": None, "info_ptr": 4 * R})

    def got(res):
        assert res.shape == (R,) and res.dtype == np.int64
    return run, sent, got


def helper_detect(idt):
    from pyitd_amd.batch import detect_knots_batch

    def run():
        return detect_knots_batch(rows_of(idt).reshape(R, N), mode=1)

    def sent(calls):
        (name, args, sizes), = calls
        assert name == "detect_batch_dev"
        check(args, sizes, {"n": N, "batch": R, "x_stride": N, "mode": 1, "idx_stride": N - 2},
              {"x_ptr": 8 * R * N, "idx_ptr": 4 * R * (N - 2), "info_ptr": 4 * R})

    def got(res):
        assert isinstance(res, list) and len(res) == R and all(a.dtype == np.int64 and a.ndim == 1 for a in res)
    return run, sent, got


def helper_channels(idt, retained):
    from pyitd_amd.batch import itd_baseline_extract_fast_channels
    knots = np.array([0, 100, 300, 700, 1029, 0, 0])

    def run():
        return itd_baseline_extract_fast_channels(rows_of(idt).reshape(R, N), knots if retained else None, 4 if retained else None)

    def sent(calls):
        (name, args, sizes), = calls
        assert name == "cubic_batch_dev"
        check(args, sizes, {"n": N, "batch": R, "x_stride": N, "extrema_stride": 0, "idx": 4 if retained else 0, "base_stride": N},
              {"x_ptr": 8 * R * N, "extrema_ptr": 4 * 5 if retained else None, "base_ptr": 8 * R * N, "info_ptr": 4 * R})

    def got(res):
        assert res.shape == (R, N) and res.dtype == np.float64 and not res.any()       # the zero fill the engine did not touch
    return run, sent, got


HELPERS = {
    "extract-f64": lambda: helper_extract(F8), "extract-f32": lambda: helper_extract(F4),
    "count-f64": lambda: helper_count(F8), "count-f32": lambda: helper_count(F4),
    "detect-f64": lambda: helper_detect(F8), "detect-f32": lambda: helper_detect(F4),
    "channels-f64-retained": lambda: helper_channels(F8, True), "channels-f32-own": lambda: helper_channels(F4, False),
}


@pytest.mark.parametrize("case", sorted(HELPERS))
def test_a_helper_hands_the_engine_what_the_header_documents(engine, case):
    run, sent, got = HELPERS[case]()
    res = run()
    sent(engine.calls)
    got(res)
    assert not HostBuffer.LIVE


@pytest.mark.parametrize("case", sorted(HELPERS))
def test_a_helper_frees_its_buffers_on_a_negative_info_word_and_when_the_engine_raises(engine, case):
    run, _, got = HELPERS[case]()
    engine.refuse = True
    if case.startswith("channels"):
        with pytest.raises(ValueError, match="strictly increasing"):       # the cubic operator's -1: a bad knot list
            run()
    else:
        got(run())                                                         # a NaN row: repeated by the single-signal operator
    assert engine.calls and not HostBuffer.LIVE
    engine.refuse, engine.fail = False, True
    with pytest.raises(RuntimeError, match="the engine failed"):
        run()
    assert not HostBuffer.LIVE
