"""The table stream without a GPU: the block-by-block statement with a carried open half wave (tests/table_stream_ref.py) gives, push
after push, exactly the half waves of tests/waves_ref.ref_table of the concatenated row — every event, the push it leaves in, every
open entry, under every origin; the library exports the new entries and refuses bad arguments before touching a device."""
import ctypes
import os

import numpy as np
import pytest

import table_stream_ref as tsr
import waves_ref
from helpers import fuzz_signal
from wave_stream_ref import run_length_signal

ENTRIES = ("itd_table_stream_create", "itd_table_stream_push_f64", "itd_table_stream_flush_f64", "itd_table_stream_push_host_f64",
           "itd_table_stream_flush_host_f64")
ORIGINS = (0, 2 ** 31 - 3, 2 ** 40)
BLOCKS = (1, 2, 3, 7)


def signals(rng, L, blocks):
    """every kind of row the GPU tests push, once"""
    out = [run_length_signal(rng, L, H, blocks, zeros=z) for H in (max(L // 2, 1), 2 * L + 1) for z in (False, True)]
    out += [fuzz_signal(rng, kind, blocks * L) for kind in (0, 1, 4)]
    out += [make(rng, L, blocks) for make in tsr.CONSTRUCTED]
    return out


def check_row(x, L, origin, what):
    """the stream's statement against ref_table of the whole row; returns the steps"""
    start, length, peak, value = (np.asarray(t) for t in waves_ref.ref_table(x))
    end = start.astype(np.int64) + length - 1
    steps, last = tsr.ref_pushes(x, L, origin)
    P = x.size // L
    got = tsr.all_events(steps, last)
    assert np.array_equal(got[0], start.astype(np.int64) + origin), what
    assert np.array_equal(got[1], length.astype(np.int64)), what
    assert np.array_equal(got[2], peak.astype(np.int64) + origin), what
    assert np.array_equal(got[3].view(np.uint64), value.view(np.uint64)), what
    k = 0
    for p, (events, op) in enumerate(steps):
        # the push a half wave leaves in: the one that brings the sample behind its last one
        lo, hi = max(1, p * L - 1), (p + 1) * L - 2
        n = int(((end[:-1] >= lo) & (end[:-1] <= hi)).sum())
        assert len(events) == n, "%s: push %d emits %d, not %d" % (what, p, len(events), n)
        assert len(events) <= (L - 2 if p == 0 else L), what
        k += n
        # the open entry: half wave k cut at the push's last sample
        s = int(start[k])
        seen = x[s:(p + 1) * L]
        at = s + int(np.flatnonzero(np.abs(seen) == np.abs(seen).max())[0])
        assert op[:3] == (origin + s, (p + 1) * L - s, origin + at), "%s: open entry of push %d" % (what, p)
        assert np.float64(op[3]).view(np.uint64) == x[at:at + 1].view(np.uint64)[0], what
    assert k == start.size - 1 and P == len(steps), what
    return steps, last


@pytest.mark.parametrize("L", [8, 9, 64, 65, 100, 512])
def test_the_carried_statement_is_ref_table_of_the_concatenated_row(L):
    rng = np.random.default_rng(2700 + L)
    rows = 0
    shown = None
    for blocks in BLOCKS:
        xs = signals(rng, L, blocks)
        steps = []
        for i, x in enumerate(xs):
            per_origin = [check_row(x, L, origin, "L=%d blocks=%d signal %d origin=%d" % (L, blocks, i, origin)) for origin in ORIGINS]
            steps.append(per_origin[0])                                   # (the conditions: on the stream's own indices)
            rows += 1
        cond = tsr.conditions(np.stack(xs), L, steps)
        shown = cond if shown is None else {k: shown[k] or v for k, v in cond.items()}
    print("L=%d: %d rows" % (L, rows))
    for name, ok in shown.items():
        assert ok, "L=%d: no row shows %s" % (L, name)


def test_the_alternating_row_fills_every_push():
    for L in (8, 65):
        steps, last = tsr.ref_pushes(tsr.alternating(np.random.default_rng(L), L, 4), L)
        assert [len(ev) for ev, _ in steps] == [L - 2, L, L, L]
        assert last[:2] == (4 * L - 1, 1)


def test_a_zeros_only_half_wave_reports_its_first_sample():
    L = 16
    x = tsr.zeros(np.random.default_rng(1), L, 1)
    steps, last = tsr.ref_pushes(x, L)
    assert steps[0][0] == [] and last[:3] == (0, L, 0) and np.signbit(last[3]) and last[3] == 0.0
    st = tsr.RefTableStream(L)
    assert st.flush() is None                                             # a flush of an empty stream emits nothing


@pytest.fixture(scope="module")
def lib():
    from pyitd_amd import _lib
    _lib.build()
    return _lib.load()


def test_the_library_exports_the_table_stream_entries(lib):
    from pyitd_amd._lib import ABI
    for name in ENTRIES:
        assert name in ABI and hasattr(lib, name), name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pyitd_hip.h")).read()
    for name in ENTRIES:
        assert "int %s(" % name in header, name
    assert "#define ITD_STREAM_TABLE 7" in header and lib.itd_abi_version() == 12
    import pyitd_amd
    assert pyitd_amd.WaveTableStream is pyitd_amd.streaming.WaveTableStream
    assert pyitd_amd.blockwise_single_waves is pyitd_amd.streaming.blockwise_single_waves
    assert pyitd_amd.StreamWaves._fields == tsr.NAMES == pyitd_amd.Waves._fields


def test_every_entry_refuses_a_null_stream_before_touching_a_device(lib):
    buf = ctypes.create_string_buffer(8 * 64)
    em = ctypes.c_int32(0)
    assert lib.itd_table_stream_create(None, 0, 64, 1, 0) == 1
    assert lib.itd_table_stream_push_f64(None, buf, 64, buf, buf, buf, buf, 65, buf, ctypes.byref(em), None) == 1
    assert lib.itd_table_stream_flush_f64(None, buf, buf, buf, buf, 65, buf, ctypes.byref(em), None) == 1
    assert lib.itd_table_stream_push_host_f64(None, buf, buf, buf, buf, buf, buf, ctypes.byref(em)) == 1
    assert lib.itd_table_stream_flush_host_f64(None, buf, buf, buf, buf, buf, ctypes.byref(em)) == 1


BAD = (dict(block=7), dict(block=4097), dict(block=0), dict(block=-8), dict(rows=0), dict(rows=65536), dict(rows=-1))


def test_create_refuses_bad_shapes_before_touching_a_device(lib):
    h = ctypes.c_void_p()
    for kw in BAD:
        a = dict(dict(block=1024, rows=1), **kw)
        assert lib.itd_table_stream_create(ctypes.byref(h), 0, a["block"], a["rows"], 0) == 1 and not h.value, kw


def test_a_valid_create_without_a_gpu_is_a_loud_failure(lib):
    import torch
    h = ctypes.c_void_p()
    for block, rows, origin in ((8, 1, 0), (4096, 65535, 2 ** 40), (100, 3, -5)):
        rc = lib.itd_table_stream_create(ctypes.byref(h), 0, block, rows, origin)
        if torch.cuda.is_available():                                     # (with a GPU the same calls make streams)
            assert rc == 0 and h.value
            lib.itd_stream_destroy(h)
        else:
            assert rc == 2 and not h.value                                # ITD_ERR_NO_DEVICE


def test_the_python_surface_refuses_the_same_values_before_any_call():
    from pyitd_amd import streaming
    for kw in BAD:
        with pytest.raises(ValueError):
            streaming.WaveTableStream(**dict(dict(block=1024, rows=1), **kw))
    with pytest.raises(ValueError):
        streaming.WaveTableStream(64.5)
    with pytest.raises(ValueError):
        streaming.WaveTableStream(64, origin=0.5)
    with pytest.raises(ValueError):
        streaming.blockwise_single_waves(np.zeros(1000), 512)             # no multiple of the block
    with pytest.raises(ValueError):
        streaming.blockwise_single_waves(np.zeros((2, 3, 512)), 512)
