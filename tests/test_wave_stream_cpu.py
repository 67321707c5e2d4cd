"""The wave-filter stream without a GPU: the block-local rule (tests/wave_stream_ref.py) equals the whole-row filter with the
upper length bound capped at the horizon (tests/waves_ref.ref_filter), bit for bit; the library exports the new entries and every
one of them refuses bad arguments before touching a device."""
import ctypes

import numpy as np
import pytest

from helpers import assert_bits_equal
from waves_ref import ref_filter
from wave_stream_ref import ref_stream_filter, run_length_signal

ENTRIES = ("itd_wave_stream_create", "itd_wave_stream_latency", "itd_wave_stream_push_f64", "itd_wave_stream_flush_f64",
           "itd_wave_stream_push_host_f64", "itd_wave_stream_flush_host_f64")


def capped(bounds, H):
    """the whole-row filter's bounds that the stream's are: len_hi -> min(len_hi, H); a NaN len_hi stays (it keeps nothing)"""
    a, b, c, d = (np.float64(v) for v in bounds)
    return (a, b, c, d if np.isnan(d) else min(d, np.float64(H)))


@pytest.mark.parametrize("L", [8, 16, 24])
def test_the_block_local_rule_is_the_capped_whole_row_filter(L):
    rng = np.random.default_rng(2100 + L)
    inf = np.inf
    checked = kept = zeroed = 0
    for H in (1, 2, L - 1, L, L + 1, 2 * L, 2 * L + 3):
        for blocks in range(1, 9):
            for zeros in (False, True):
                x = run_length_signal(rng, L, H, blocks, zeros)
                for bounds in ((0.0, inf, 0.0, inf), (0.5, 2.0, 2.0, inf), (0.0, inf, 0.0, float(H // 2)), (0.0, 1.0, 1.0, float(H)),
                               (0.0, inf, 0.0, np.nan)):
                    want = ref_filter(x, capped(bounds, H))
                    got = ref_stream_filter(x, L, H, bounds)
                    assert_bits_equal(got, want, "L=%d H=%d blocks=%d zeros=%s bounds=%s" % (L, H, blocks, zeros, bounds))
                    checked += 1
                    kept += int(np.count_nonzero(want))
                    zeroed += int(np.count_nonzero((want == 0) & (x != 0)))
    assert checked == 7 * 8 * 2 * 5 and kept > 1000 and zeroed > 1000


def test_a_half_wave_of_exactly_the_horizon_behind_a_crossing_at_the_first_readable_sample_is_kept():
    """H = D L: the crossing index b L - H - ... sits exactly at the first readable sample; the half wave behind it has length H."""
    L, H = 8, 8
    x = np.concatenate((-np.ones(8), np.ones(8), -np.ones(8), np.ones(8)))      # crossings at 7, 15, 23
    x[12] = 2.0
    got = ref_stream_filter(x, L, H, (0.0, np.inf, 0.0, np.inf))
    assert_bits_equal(got, x, "every half wave has length 8 = H")
    got = ref_stream_filter(x, L, 7, (0.0, np.inf, 0.0, np.inf))
    assert_bits_equal(got, np.zeros(32), "none fits a horizon of 7")


@pytest.fixture(scope="module")
def lib():
    from pyitd_amd import _lib
    _lib.build()
    return _lib.load()


def test_the_library_exports_the_wave_stream_entries(lib):
    from pyitd_amd._lib import ABI
    for name in ENTRIES:
        assert name in ABI and hasattr(lib, name), name


def test_every_entry_refuses_a_null_stream_before_touching_a_device(lib):
    buf = ctypes.create_string_buffer(8 * 64)
    em = ctypes.c_int32(0)
    assert lib.itd_wave_stream_create(None, 0, 64, 1, 64) == 1
    assert lib.itd_wave_stream_latency(None) == -1
    assert lib.itd_wave_stream_push_f64(None, buf, 64, buf, 0, buf, 64, ctypes.byref(em), None) == 1
    assert lib.itd_wave_stream_flush_f64(None, buf, 0, buf, 64, ctypes.byref(em), None) == 1
    assert lib.itd_wave_stream_push_host_f64(None, buf, buf, buf, ctypes.byref(em)) == 1
    assert lib.itd_wave_stream_flush_host_f64(None, buf, buf, ctypes.byref(em)) == 1


def test_create_refuses_bad_shapes_before_touching_a_device(lib):
    h = ctypes.c_void_p()
    for L, R, H in ((7, 1, 8), (8193, 1, 8), (64, 0, 8), (64, 1, 0), (64, 65536, 8), (64, 1, (1 << 22) + 1), (64, -1, 8), (64, 1, -1)):
        assert lib.itd_wave_stream_create(ctypes.byref(h), 0, L, R, H) == 1, (L, R, H)
        assert not h.value


def test_the_python_surface_refuses_the_same_values():
    from pyitd_amd import streaming
    for kw in (dict(block=7, rows=1, horizon=8), dict(block=8193, rows=1, horizon=8), dict(block=64, rows=0, horizon=8),
               dict(block=64, rows=1, horizon=0), dict(block=64, rows=1, horizon=(1 << 22) + 1)):
        with pytest.raises(ValueError):
            streaming.WaveFilterStream(**kw)
    with pytest.raises(ValueError):
        streaming.blockwise_wave_filter(np.zeros(100), 64, 64)
