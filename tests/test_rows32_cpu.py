"""float32 result rows (itd_decompose_rows32_*), the part that needs no GPU: the four entries exist on both sides of the ABI, refuse
bad arguments before they touch the device, and the Python surface carries the row type."""
import ctypes
import inspect

import numpy as np
import pytest

ENTRIES = ("itd_decompose_rows32_f32", "itd_decompose_rows32_f64", "itd_decompose_rows32_host_f32", "itd_decompose_rows32_host_f64")
ITD_ERR_INVALID_ARG = 1


@pytest.fixture(scope="module")
def lib():
    from pyitd_amd import _lib
    _lib.build()
    return _lib.load()


def test_the_four_entries_are_exported_and_declared(lib):
    from pyitd_amd._lib import ABI
    for name in ENTRIES:
        assert hasattr(lib, name), "libpyitd_hip.so does not export %s" % name
        assert name in ABI, "%s is missing from pyitd_amd/_lib.py" % name
    # additive: the revision stays
    assert lib.itd_abi_version() == 12


def test_null_engine_or_null_rows_is_an_invalid_argument_before_any_device_call(lib):
    """No engine exists on a host without a GPU: the entries must refuse on the pointers alone.  The stand-in for an engine is
    zeroed host memory that a refusal never reads."""
    x32, x64 = np.zeros(16, np.float32), np.zeros(16, np.float64)
    rows = np.zeros((3, 16), np.float32)
    fake = ctypes.create_string_buffer(1 << 16)
    eng = ctypes.cast(fake, ctypes.c_void_p)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for f, x in ((lib.itd_decompose_rows32_f32, x32), (lib.itd_decompose_rows32_f64, x64)):
        assert f(None, p(x), 16, 1, 16, 1, p(rows), None) == ITD_ERR_INVALID_ARG
        assert f(eng, p(x), 16, 1, 16, 1, None, None) == ITD_ERR_INVALID_ARG
        assert f(eng, None, 16, 1, 16, 1, p(rows), None) == ITD_ERR_INVALID_ARG
    nr, why = ctypes.c_int32(0), ctypes.c_int32(0)
    for f, x in ((lib.itd_decompose_rows32_host_f32, x32), (lib.itd_decompose_rows32_host_f64, x64)):
        assert f(None, p(x), 16, 1, p(rows), ctypes.byref(nr), ctypes.byref(why), None) == ITD_ERR_INVALID_ARG
        assert f(eng, p(x), 16, 1, None, ctypes.byref(nr), ctypes.byref(why), None) == ITD_ERR_INVALID_ARG
        assert f(eng, None, 16, 1, p(rows), ctypes.byref(nr), ctypes.byref(why), None) == ITD_ERR_INVALID_ARG


def test_the_python_surface_carries_the_row_type():
    import pyitd_amd
    from pyitd_amd.engine import Engine
    sig = inspect.signature(pyitd_amd.ITD.itd).parameters
    assert list(sig)[:5] == ["self", "data", "max_iteration", "out", "out_dtype"]
    assert sig["out_dtype"].default is None and sig["out"].default is None and sig["max_iteration"].default == 11
    assert inspect.signature(pyitd_amd.itd_batch).parameters["out_dtype"].default is None
    for fn in (Engine.decompose_dev, Engine.decompose_host):
        assert inspect.signature(fn).parameters["rows_dtype"].default is np.float64


@pytest.mark.parametrize("bad", [np.float16, np.int32, np.complex128, "float128x", object])
def test_any_other_row_type_is_a_value_error(bad):
    """Raised on the type alone: before a signal is looked at, an engine is created or the device is asked for."""
    import pyitd_amd
    x = np.sin(np.arange(100.0))
    with pytest.raises(ValueError):
        pyitd_amd.ITD().itd(x, 3, out_dtype=bad)
    with pytest.raises(ValueError):
        pyitd_amd.itd_batch(np.stack([x, x]), 3, out_dtype=bad)


def test_float32_rows_come_without_baselines():
    import pyitd_amd
    x = np.sin(np.arange(100.0))
    with pytest.raises(ValueError, match="baselines"):
        pyitd_amd.itd_batch(np.stack([x, x]), 3, keep_baselines=True, out_dtype=np.float32)
