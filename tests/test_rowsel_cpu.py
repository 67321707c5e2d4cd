"""Selected result rows (itd_decompose_select_*, select=), the part that needs no GPU: the four entries exist on both sides of the ABI
and in the header, refuse bad arguments before they touch the device, and the Python surface parses select= and raises ValueError for
everything that is not a selection."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ENTRIES = ("itd_decompose_select_f32", "itd_decompose_select_f64", "itd_decompose_select_host_f32", "itd_decompose_select_host_f64")
ITD_ERR_INVALID_ARG = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pyitd_amd import _lib
    _lib.build()
    return _lib.load()


def test_the_four_entries_are_exported_declared_and_in_the_header(lib):
    from pyitd_amd._lib import ABI
    header = open(os.path.join(ROOT, "include", "pyitd_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name), "libpyitd_hip.so does not export %s" % name
        assert name in ABI, "%s is missing from pyitd_amd/_lib.py" % name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, "%s is not declared in include/pyitd_hip.h" % name
        args = decl.group(1)
        assert "uint32_t rotation_mask" in args and "int32_t want_residual" in args and "int32_t rows_f32" in args
        assert len(args.split(",")) == len(ABI[name][1])
    assert lib.itd_abi_version() == 12          # additive: the revision stays


def test_refusals_come_before_any_device_call(lib):
    """No engine exists on a host without a GPU, so all this test can show is that these calls come back with
    ITD_ERR_INVALID_ARG without touching a device or the rows.  The stand-in for an engine is zeroed host memory (max_n = 0): it
    would make every call an invalid argument by itself, so the return codes here say nothing about WHICH rule refused — the entries
    test the selection before they look at the engine, but only a live engine with otherwise valid arguments proves the selection's
    rules: tests/test_gpu_rowsel.py::test_rejected_selections.  The rules themselves are checked below on the Python side
    (selection_of), which needs no engine."""
    x32, x64 = np.zeros(16, np.float32), np.zeros(16, np.float64)
    rows = np.zeros((3, 16), np.float64)
    fake = ctypes.create_string_buffer(1 << 16)
    eng = ctypes.cast(fake, ctypes.c_void_p)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    bad = [(1 << 2, 1),         # bit 2 with max_iteration = 1
           (1 << 31, 0),
           (0, 0),              # S = 0
           (1, 2), (1, -1)]     # the residual flag is 0 or 1
    for f, x in ((lib.itd_decompose_select_f32, x32), (lib.itd_decompose_select_f64, x64)):
        for mask, res in bad:
            assert f(eng, p(x), 16, 1, 16, 1, mask, res, p(rows), 0, None) == ITD_ERR_INVALID_ARG, (mask, res)
        assert f(eng, p(x), 16, 1, 16, 1, 3, 1, p(rows), 2, None) == ITD_ERR_INVALID_ARG            # the row type is 0 or 1
        assert f(None, p(x), 16, 1, 16, 1, 3, 1, p(rows), 0, None) == ITD_ERR_INVALID_ARG
        assert f(eng, p(x), 16, 1, 16, 1, 3, 1, None, 0, None) == ITD_ERR_INVALID_ARG               # NULL rows
        assert f(eng, None, 16, 1, 16, 1, 3, 1, p(rows), 0, None) == ITD_ERR_INVALID_ARG
    nr, why = ctypes.c_int32(0), ctypes.c_int32(0)
    for f, x in ((lib.itd_decompose_select_host_f32, x32), (lib.itd_decompose_select_host_f64, x64)):
        for mask, res in bad:
            assert f(eng, p(x), 16, 1, mask, res, p(rows), 0, ctypes.byref(nr), ctypes.byref(why), None) == ITD_ERR_INVALID_ARG, (mask, res)
        assert f(eng, p(x), 16, 1, 3, 1, p(rows), 2, ctypes.byref(nr), ctypes.byref(why), None) == ITD_ERR_INVALID_ARG
        assert f(None, p(x), 16, 1, 3, 1, p(rows), 0, ctypes.byref(nr), ctypes.byref(why), None) == ITD_ERR_INVALID_ARG
        assert f(eng, p(x), 16, 1, 3, 1, None, 0, ctypes.byref(nr), ctypes.byref(why), None) == ITD_ERR_INVALID_ARG
        assert f(eng, None, 16, 1, 3, 1, p(rows), 0, ctypes.byref(nr), ctypes.byref(why), None) == ITD_ERR_INVALID_ARG
    assert not rows.any()


def test_the_python_surface_carries_the_selection():
    import pyitd_amd
    from pyitd_amd.engine import Engine
    sig = inspect.signature(pyitd_amd.ITD.itd).parameters
    assert list(sig)[:6] == ["self", "data", "max_iteration", "out", "out_dtype", "select"]
    assert sig["select"].default is None
    assert inspect.signature(pyitd_amd.itd_batch).parameters["select"].default is None
    for fn in (Engine.decompose_dev, Engine.decompose_host):
        assert inspect.signature(fn).parameters["select"].default is None


@pytest.mark.parametrize("select, m, want", [
    ([2, 3, -1], 7, (0b1100, 1, 3)),
    ([-1], 0, (0, 1, 1)),
    ((0,), 0, (1, 0, 1)),
    ([0, 1, 2, 3, -1], 3, (0b1111, 1, 5)),
    (np.array([1, 20]), 20, ((1 << 1) | (1 << 20), 0, 2)),
    (range(0, 8, 2), 7, (0b1010101, 0, 4)),
])
def test_selections_parse(select, m, want):
    from pyitd_amd.engine import selection_of
    assert selection_of(select, m) == want


BAD = [
    ([], "empty"),
    ([3, 2], "unsorted"),
    ([2, 2], "a duplicate"),
    ([0, 2, 2, -1], "a duplicate in front of the residual"),
    ([4], "an index above max_iteration"),
    ([0, 4, -1], "an index above max_iteration"),
    ([-1, 0], "-1 not last"),
    ([0, -1, 2], "-1 not last"),
    ([-1, -1], "-1 twice"),
    ([-2], "a negative index"),
    ([1.0], "not an integer"),
    ([True], "not an integer"),
    (["0"], "not an integer"),
    (3, "not a sequence"),
]


@pytest.mark.parametrize("select, why", BAD)
def test_anything_else_is_a_value_error(select, why):
    """Raised on the selection alone: before a signal is looked at, an engine is created or the device is asked for."""
    import pyitd_amd
    from pyitd_amd.engine import selection_of
    x = np.sin(np.arange(100.0))
    with pytest.raises(ValueError):
        selection_of(select, 3)
    with pytest.raises(ValueError):
        pyitd_amd.ITD().itd(x, 3, select=select)
    with pytest.raises(ValueError):
        pyitd_amd.itd_batch(np.stack([x, x]), 3, select=select)
    with pytest.raises(ValueError):
        pyitd_amd.itd_batch(np.stack([x, x]), 3, select=select, out_dtype=np.float32)


def test_selected_rows_come_without_baselines():
    import pyitd_amd
    x = np.sin(np.arange(100.0))
    with pytest.raises(ValueError, match="baselines"):
        pyitd_amd.itd_batch(np.stack([x, x]), 3, keep_baselines=True, select=[0, -1])


def test_absent_slots_are_zero_filled():
    from pyitd_amd.engine import zero_absent_slots
    rows = np.ones((4, 5))
    zero_absent_slots(rows, [0, 2, 5, -1], 4)          # n_rows = 4: rotations 0 .. 2 exist, rotation 5 does not
    assert rows[:2].all() and not rows[2].any() and rows[3].all()
    b = np.ones((3, 3, 4), np.float32)
    zero_absent_slots(b, [1, 3, -1], np.array([6, 3, 1]))
    assert b[0].all()
    assert b[1, 0].all() and not b[1, 1].any() and b[1, 2].all()
    assert not b[2, :2].any() and b[2, 2].all()
