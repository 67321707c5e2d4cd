"""The instantaneous stream without a GPU: the block-local rule (tests/inst_stream_ref.py) equals the whole-row statement — the half
waves of tests/waves_ref.py, the long and overlong masks, the NaN pattern where a value is not delivered — bit for bit; known-answer
cases of the horizon; the library exports the new entries and every one of them refuses bad arguments before touching a device."""
import ctypes

import numpy as np
import pytest

import inst_stream_ref as isr
import spectrum_stream_ref as ssr
from wave_stream_ref import run_length_signal

ENTRIES = ("itd_inst_stream_create", "itd_inst_stream_latency", "itd_inst_stream_push_f64", "itd_inst_stream_flush_f64",
           "itd_inst_stream_push_host_f64", "itd_inst_stream_flush_host_f64")
NAMES = ("amplitude", "phase", "frequency", "length", "long", "overlong")


def same_bits(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, "%s %s: %s %s vs %s %s" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if g.dtype == np.float64:
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert np.array_equal(g, w), "%s: %s differs" % (what, name)


def latency(L, H):
    return -(-(H + 1) // L)


def run_blocks(x, L, H):
    got = [isr.block_features(x, L, H, b) for b in range(x.size // L)]
    return tuple(np.concatenate([g[i] for g in got]) for i in range(6))


def check_masks(feat):
    """the NaN pattern stands exactly where the masks say, and nowhere else"""
    amp, ph, fr, ln, long_, overlong = feat
    none = lambda a: a.view(np.uint64) == isr.NONE_BITS
    assert np.array_equal(none(amp), long_) and np.array_equal(none(ph), long_) and np.array_equal(none(fr), overlong)
    assert np.array_equal(ln == 0, long_) and not (long_ & ~overlong).any()
    assert not np.isnan(amp[~long_]).any() and not np.isnan(ph[~long_]).any() and not np.isnan(fr[~overlong]).any()


@pytest.mark.parametrize("L", [8, 100, 128])
def test_the_block_local_rule_is_the_whole_row_statement(L):
    """Samples seen per (L, H), as (delivered, overlong but not long, long), with the seeds below:
        L = 8:    H = 1 (35, 26, 179)     H = 7 (149, 9, 82)       H = 8 (290, 15, 143)      H = 9 (281, 17, 150)      H = 16 (450, 15, 255)
        L = 100:  H = 1 (39, 26, 2935)    H = 99 (1592, 11, 1397)  H = 100 (3363, 18, 2219)  H = 101 (4364, 12, 1224)  H = 200 (6172, 14, 2814)
        L = 128:  H = 1 (39, 33, 3768)    H = 127 (2419, 11, 1410) H = 128 (5089, 15, 2064)  H = 129 (5217, 13, 1938)  H = 256 (7650, 15, 3855)
    (run with -s to print them)."""
    rng = np.random.default_rng(2400 + L)
    lat = []
    for H in (1, L - 1, L, L + 1, 2 * L):
        D = latency(L, H)
        lat.append(D)
        seen = np.zeros(3, np.int64)
        for blocks in range(1, 2 * D + 4):
            for zeros in (False, True):
                x = run_length_signal(rng, L, H, blocks, zeros) * ssr.envelope(blocks * L, rng)
                want = isr.whole_row_features(x, H)
                got = run_blocks(x, L, H)
                same_bits(got, want, "L=%d H=%d blocks=%d zeros=%s" % (L, H, blocks, zeros))
                check_masks(got)
                seen += (int((~want[5]).sum()), int((want[5] & ~want[4]).sum()), int(want[4].sum()))
        print("L=%d H=%d delivered, overlong only, long: %s" % (L, H, tuple(int(v) for v in seen)))
        assert (seen > 0).all(), (L, H, seen)
    assert lat == [1, 1, 2, 2, 3]                                          # D steps at H = L - 1 -> L and at 2 L - 1 -> 2 L


def waves(lengths, first=1.0):
    """alternating runs of the given lengths, each a half sine arch, the first one positive"""
    out, sign = [], first
    for ln in lengths:
        out.append(sign * np.sin(np.pi * (np.arange(ln) + 0.5) / ln))
        sign = -sign
    return np.concatenate(out)


def is_none(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64) == isr.NONE_BITS


def test_a_half_wave_of_exactly_the_horizon_is_delivered_and_one_a_sample_longer_is_not():
    L, H = 64, 10
    x = waves([3, 4, H, 5, H + 1, 6, 7, 24])                              # 70 samples, padded to two blocks below
    x = np.concatenate((x, waves([6] * 12, -1.0)[:2 * L - x.size]))
    got = run_blocks(x, L, H)
    same_bits(got, isr.whole_row_features(x, H), "known answer")
    amp, ph, fr, ln, long_, overlong = got
    at = np.cumsum([0, 3, 4, H, 5, H + 1, 6, 7])
    a, b = at[2], at[3]                                                   # the half wave of exactly H samples
    assert np.all(ln[a:b] == H) and not overlong[a:b].any() and np.all(amp[a:b] == np.abs(x[a:b]).max())
    a, b = at[4], at[5]                                                   # the one of H + 1
    assert np.all(ln[a:b] == 0) and long_[a:b].all() and is_none(amp[a:b]).all() and is_none(ph[a:b]).all() and is_none(fr[a:b]).all()
    assert np.all(ln[at[3]:at[4]] == 5) and overlong[at[4] - 1] and not overlong[at[3]:at[4] - 1].any()


def test_the_sample_in_front_of_a_long_half_wave_across_a_block_seam_loses_only_its_frequency():
    """block 0's last sample is a crossing index; the half wave that begins with block 1 has H + 1 samples"""
    L, H = 64, 70
    x = waves([20, 44, H + 1, 30, 27])                                    # 192 samples; crossings at 19, 63, 134, 164
    assert x.size == 3 * L
    got = run_blocks(x, L, H)
    same_bits(got, isr.whole_row_features(x, H), "seam")
    amp, ph, fr, ln, long_, overlong = isr.block_features(x, L, H, 0)
    assert overlong[63] and not long_[63] and ln[63] == 44
    assert amp[63] == np.abs(x[20:64]).max() and not is_none(ph[63]) and is_none(fr[63])
    assert not overlong[:63].any()
    assert got[4].reshape(3, L).sum(axis=1).tolist() == [0, 64, 7] and got[5].reshape(3, L).sum(axis=1).tolist() == [1, 64, 7]
    # with a horizon one longer everything is delivered, and the reach is still enough
    got = run_blocks(x, L, H + 1)
    same_bits(got, isr.whole_row_features(x, H + 1), "seam, H + 1")
    assert not got[5].any() and got[3][64] == H + 1


def test_the_last_sample_behind_a_long_half_wave_loses_only_its_frequency():
    """the crossing index is n - 2: the flushed stream's last sample is a half wave of its own, its backward difference needs the
    phase of a sample of the long half wave in front of it"""
    L, H = 64, 10
    x = waves([5, 6, 7, 8, 9, 10, 7, H + 1, 1])
    assert x.size == L
    got = isr.block_features(x, L, H, 0)
    same_bits(got, isr.whole_row_features(x, H), "last sample")
    amp, ph, fr, ln, long_, overlong = got
    assert long_[52:63].all() and not long_[63] and overlong[63]
    assert ln[63] == 1 and amp[63] == abs(x[63]) and not is_none(ph[63]) and is_none(fr[63])
    assert overlong[51] and not long_[51] and not overlong[:51].any()


def test_a_crossing_exactly_at_the_first_readable_sample():
    """H = L: for block 2 the first readable sample is L, a crossing index; the half wave behind it has exactly H samples and reaches
    block 2's first sample"""
    L, H = 64, 64
    x = waves([L + 1, H, 30, 3 * L - (L + 1) - H - 30])                   # crossings at 64, 128, 158
    assert x.size == 3 * L
    got = run_blocks(x, L, H)
    same_bits(got, isr.whole_row_features(x, H), "first readable sample")
    amp, ph, fr, ln, long_, overlong = isr.block_features(x, L, H, 2)
    assert not overlong[0] and ln[0] == H and amp[0] == np.abs(x[L + 1:2 * L + 1]).max()
    assert got[5].reshape(3, L).sum(axis=1).tolist() == [64, 1, 0] and got[4].reshape(3, L).sum(axis=1).tolist() == [64, 1, 0]


@pytest.fixture(scope="module")
def lib():
    from pyitd_amd import _lib
    _lib.build()
    return _lib.load()


def test_the_library_exports_the_instantaneous_stream_entries(lib):
    from pyitd_amd._lib import ABI
    for name in ENTRIES:
        assert name in ABI and hasattr(lib, name), name
    import pyitd_amd
    assert pyitd_amd.InstantaneousStream is pyitd_amd.streaming.InstantaneousStream
    assert pyitd_amd.blockwise_instantaneous is pyitd_amd.streaming.blockwise_instantaneous
    assert pyitd_amd.StreamInstant._fields == NAMES


def test_every_entry_refuses_a_null_stream_before_touching_a_device(lib):
    buf = ctypes.create_string_buffer(8 * 64)
    em = ctypes.c_int32(0)
    assert lib.itd_inst_stream_create(None, 0, 64, 1, 64) == 1
    assert lib.itd_inst_stream_latency(None) == -1
    assert lib.itd_inst_stream_push_f64(None, buf, 64, buf, buf, buf, buf, 64, buf, 2, ctypes.byref(em), None) == 1
    assert lib.itd_inst_stream_flush_f64(None, buf, buf, buf, buf, 64, buf, 2, ctypes.byref(em), None) == 1
    assert lib.itd_inst_stream_push_host_f64(None, buf, buf, buf, buf, buf, buf, ctypes.byref(em)) == 1
    assert lib.itd_inst_stream_flush_host_f64(None, buf, buf, buf, buf, buf, ctypes.byref(em)) == 1


BAD = (dict(block=7), dict(block=4097), dict(rows=0), dict(rows=65536), dict(horizon=0), dict(horizon=(1 << 22) + 1))


def test_create_refuses_bad_shapes_before_touching_a_device(lib):
    h = ctypes.c_void_p()
    ok = dict(block=100, rows=1, horizon=100)
    for kw in BAD:
        a = dict(ok, **kw)
        assert lib.itd_inst_stream_create(ctypes.byref(h), 0, a["block"], a["rows"], a["horizon"]) == 1, kw
        assert not h.value


def test_the_python_surface_refuses_the_same_values():
    from pyitd_amd import streaming
    ok = dict(block=100, rows=1, horizon=100)
    for kw in BAD:
        with pytest.raises(ValueError):
            streaming.InstantaneousStream(**dict(ok, **kw))
    for want in ((), [], ("power",), ("amplitude", "outside"), "long"):
        with pytest.raises(ValueError):
            streaming.InstantaneousStream(100, want=want)
        with pytest.raises(ValueError):
            streaming.blockwise_instantaneous(np.zeros(200), 100, 100, want=want)
