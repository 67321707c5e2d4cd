"""MEITD_batch / XITD_batch without a GPU: the new C-ABI entries refuse a NULL engine or pointer before any HIP call, and the Python
surface takes what the issue's contract names."""
import ctypes
import inspect

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from pyitd_amd import _lib
    _lib.build()
    return _lib.load()


def test_batch_entries_refuse_a_null_engine_or_pointer(lib):
    res = (ctypes.c_int32 * 24)()
    tab = (ctypes.c_int64 * 1)()
    fake = ctypes.create_string_buffer(1 << 16)           # never dereferenced: a NULL argument is refused first
    rows = ctypes.create_string_buffer(8 * 50 * 100)
    # itd_meitd_batch_f64(e, rows, n, batch, rows_stride, x_host, wpemax, result, logs, log_cap, xitd_sums, xitd_windows, stream)
    assert lib.itd_meitd_batch_f64(None, rows, 100, 1, 5000, None, 0.6, res, None, 0, None, None, None) == 1
    assert lib.itd_meitd_batch_f64(fake, None, 100, 1, 5000, None, 0.6, res, None, 0, None, None, None) == 1
    assert lib.itd_meitd_batch_f64(fake, rows, 100, 1, 5000, None, 0.6, None, None, 0, None, None, None) == 1
    assert lib.itd_meitd_batch_f64(fake, rows, 100, 1, 5000, None, 0.6, res, None, 16, None, None, None) == 1   # a log without its buffer
    # itd_gather_rows_f64(e, src, src_elems, offsets, rows, n, dst, dst_host, stream)
    assert lib.itd_gather_rows_f64(None, rows, 5000, tab, 1, 100, rows, None, None) == 1
    assert lib.itd_gather_rows_f64(fake, None, 5000, tab, 1, 100, rows, None, None) == 1
    assert lib.itd_gather_rows_f64(fake, rows, 5000, None, 1, 100, rows, None, None) == 1
    assert lib.itd_gather_rows_f64(fake, rows, 5000, tab, 1, 100, None, None, None) == 1


def test_batch_entries_refuse_bad_shapes_before_touching_the_engine(lib):
    res = (ctypes.c_int32 * 24)()
    tab = (ctypes.c_int64 * 2)(0, 4950)                   # the second row would end past the source
    fake = ctypes.create_string_buffer(1 << 16)
    rows = ctypes.create_string_buffer(8 * 50 * 100)
    assert lib.itd_meitd_batch_f64(fake, rows, 100, 1, 4999, None, 0.6, res, None, 0, None, None, None) == 1   # rows_stride < 50 n
    assert lib.itd_meitd_batch_f64(fake, rows, 9000, 1, 450000, None, 0.6, res, None, 0, None, None, None) == 1   # n > 8192
    assert lib.itd_meitd_batch_f64(fake, rows, 100, 0, 5000, None, 0.6, res, None, 0, None, None, None) == 1
    w = (ctypes.c_double * 132)()
    assert lib.itd_meitd_batch_f64(fake, rows, 100, 1, 5000, None, 0.6, res, None, 0, w, None, None) == 1      # sums without counts
    assert lib.itd_gather_rows_f64(fake, rows, 5000, tab, 2, 100, rows, None, None) == 1


def test_batch_signatures():
    from pyitd_amd import meitd
    p = inspect.signature(meitd.MEITD_batch).parameters
    assert list(p) == ["data", "max_iteration", "WPEMAX", "device", "solver", "chunk"]
    assert p["max_iteration"].default == 40 and p["WPEMAX"].default == 0.6 and p["device"].default == 0
    assert p["solver"].default == "auto" and p["chunk"].default is None
    p = inspect.signature(meitd.XITD_batch).parameters
    assert list(p) == ["data", "device", "solver", "chunk"]
    assert p["device"].default == 0 and p["solver"].default == "auto" and p["chunk"].default is None


@pytest.mark.parametrize("bad", [np.zeros(3000), np.zeros((2, 3, 3000)), np.zeros((4, 2))])
def test_batch_refuses_anything_but_a_2d_batch(bad):
    from pyitd_amd import meitd
    with pytest.raises(ValueError):
        meitd.MEITD_batch(bad)
    with pytest.raises(ValueError):
        meitd.XITD_batch(bad)


def test_default_chunk_keeps_rows_near_a_gibibyte():
    from pyitd_amd import meitd
    for n in (3, 1024, 3000, 4800, 8192):
        c = meitd._batch_chunk(n)
        assert c * 50 * n * 8 <= 1 << 30 and c <= 65535
        assert c >= 256
