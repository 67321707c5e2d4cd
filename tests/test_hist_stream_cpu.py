"""The histogram stream without a GPU: the block-local rule (tests/hist_stream_ref.py) equals the whole-row statement — the half waves
of tests/waves_ref.py, those of at most H samples through tests/wave_hist_ref.hist_of_table, the others' samples into overlong —
integer for integer; known-answer cases of peaks at seams; the library exports the new entries and the wrapper refuses bad arguments
before touching a device."""
import ctypes
import os

import numpy as np
import pytest

import hist_stream_ref as hsr
import waves_ref
from wave_stream_ref import run_length_signal

ENTRIES = ("itd_hist_stream_create", "itd_hist_stream_latency", "itd_hist_stream_push_f64", "itd_hist_stream_flush_f64",
           "itd_hist_stream_push_host_f64", "itd_hist_stream_flush_host_f64")
COVER = (np.array([0.0, 0.2, 0.5, 2.0, np.inf]), np.array([1.0, 2.0, 4.0, 64.0, 600.0, np.inf]))   # every amplitude, every length
PART = (np.array([0.2, 0.5, 2.0]), np.array([2.0, 4.0, 64.0, 600.0]))                               # some half waves fall outside


def hops(L):
    return [h for h in range(64, L + 1, 64) if L % h == 0]


def horizons(L):
    return (1, 2, L - 1, L, L + 1, 2 * L + 3)


def check_row(x, L, H, hop, what):
    """the rule against the statement for both edge sets; returns the table and the covering result"""
    table = waves_ref.ref_table(x)
    for ae, le in (COVER, PART):
        want = hsr.whole_row_hist(x, H, ae, le, hop, table)
        got = hsr.ref_hist_stream(x, L, H, ae, le, hop)
        hsr.same_ints(got, want, what)
        # every sample is in a counted half wave, in an outside one or overlong
        start, length, peak, value = table
        ok = length <= H
        inside = hsr.whr.bin_of(np.abs(value), ae)[1] & hsr.whr.bin_of(length.astype(np.float64), le)[1]
        assert int(got[1].sum()) + int(length[ok & ~inside].sum()) + int(got[3].sum()) == x.size, what
        assert int(got[2].sum()) == int((ok & ~inside).sum()), what
        if ae is COVER[0]:
            cover = got
    return table, cover, got


@pytest.mark.parametrize("L", [64, 128, 512])
def test_the_block_local_rule_is_the_whole_row_statement(L):
    rng = np.random.default_rng(2500 + L)
    exact = longer = outside = overlong = 0
    for H in horizons(L):
        for blocks in range(1, 10):
            for zeros in (False, True):
                x = run_length_signal(rng, L, H, blocks, zeros)
                for hop in hops(L):
                    what = "L=%d hop=%d H=%d blocks=%d zeros=%s" % (L, hop, H, blocks, zeros)
                    table, cover, part = check_row(x, L, H, hop, what)
                    assert cover[0].sum() > 0 and cover[2].sum() == 0, what
                    outside += int(part[2].sum())
                    overlong += int(part[3].sum())
                exact += int((table[1] == H).sum())
                longer += int((table[1] == H + 1).sum())
    print("L=%d: half waves of exactly H: %d, of H + 1: %d; outside %d, overlong samples %d" % (L, exact, longer, outside, overlong))
    assert exact > 0 and longer > 0 and outside > 0 and overlong > 0


def seam_ties(x, H, hop):
    """half waves of at most H samples whose maximum is attained in two different cells"""
    start, length, _, value = waves_ref.ref_table(x)
    ties = 0
    for s, ln, v in zip(start, length, value):
        if ln <= H:
            at = s + np.flatnonzero(np.abs(x[s:s + ln]) == abs(v))
            ties += int(at[0] // hop != at[-1] // hop)
    return ties


def test_a_maximum_repeated_on_both_sides_of_a_seam_belongs_to_the_first():
    ties = 0
    for L in (64, 128, 512):
        rng = np.random.default_rng(2600 + L)
        for H in horizons(L):
            for blocks in (2, 3, 5, 9):
                x = hsr.tied_maxima(run_length_signal(rng, L, H, blocks, zeros=bool(blocks & 1)))
                for hop in hops(L):
                    check_row(x, L, H, hop, "tied L=%d hop=%d H=%d blocks=%d" % (L, hop, H, blocks))
                    ties += seam_ties(x, H, hop)
    print("tied maxima on both sides of a cell seam: %d" % ties)
    assert ties >= 50


def runs(*specs):
    """alternating runs (length, offsets of the peaks in the run, amplitude) over a floor of 0.125, the first one positive"""
    out, sign = [], 1.0
    for ln, at, amp in specs:
        r = np.full(ln, 0.125)
        r[list(at)] = amp
        out.append(sign * r)
        sign = -sign
    return np.concatenate(out)


BIG = (np.array([0.0, 1.0, 2.0, 4.0]), np.array([1.0, 1000.0]))          # amplitude 3.0 alone in bin 2


def where_big(x, L, H, hop=None):
    """the time bins' counts of the half waves of amplitude 3.0, from the rule (checked against the statement)"""
    hop = L if hop is None else hop
    got = hsr.ref_hist_stream(x, L, H, *BIG, hop)
    hsr.same_ints(got, hsr.whole_row_hist(x, H, *BIG, hop), "known answer")
    return got[0][:, 2, 0].tolist(), got


def test_a_peak_at_the_last_sample_before_a_block_at_its_first_and_at_its_last():
    L, H = 64, 64
    for peak, t in ((63, 0), (64, 1), (127, 1)):
        a = peak - 13                                                     # the half wave a .. a + 19 holds the peak at offset 13
        x = runs((5, (0,), 1.0), (a - 5, (1,), 1.0), (20, (13,), 3.0), (3 * L - a - 20, (2,), 1.0))
        assert x.size == 3 * L and abs(x[peak]) == 3.0
        big, _ = where_big(x, L, H)
        assert big == [int(t == b) for b in range(3)], (peak, big)
    # the last sample of a block as the last sample of its half wave
    x = runs((100, (3,), 1.0), (28, (27,), 3.0), (64, (5,), 1.0))
    assert abs(x[127]) == 3.0
    assert where_big(x, L, H)[0] == [0, 1, 0]


def test_a_half_wave_over_three_whole_blocks_with_its_peak_in_the_middle_one():
    L, H = 64, 256
    x = runs((60, (3,), 1.0), (200, (90,), 3.0), (60, (5,), 1.0))           # 60 .. 259: blocks 1, 2, 3 whole; the peak at 150
    assert x.size == 5 * L
    big, got = where_big(x, L, H)
    assert big == [0, 0, 1, 0, 0] and got[1][2, 2, 0] == 200 and not got[3].any()
    # a horizon one sample short: it is overlong, every one of its samples
    big, got = where_big(x, L, 199)
    assert big == [0] * 5 and got[3].tolist() == [4, 64, 64, 64, 4]


def test_equal_maxima_in_the_first_and_the_last_of_three_blocks_the_first_wins():
    L, H = 64, 256
    x = runs((60, (3,), 1.0), (200, (10, 190), 3.0), (60, (5,), 1.0))       # maxima at 70 (block 1) and 250 (block 3)
    big, got = where_big(x, L, H)
    assert big == [0, 1, 0, 0, 0] and got[1][1, 2, 0] == 200
    # and across a cell seam inside one block
    big, _ = where_big(x, 320, H, hop=64)
    assert big == [0, 1, 0, 0, 0]


def test_an_all_zero_half_wave_across_a_seam_has_its_peak_at_its_first_sample():
    L = 64
    x = np.zeros(2 * L)
    x[5] = -0.0
    ae, le = np.array([0.0, 1.0]), np.array([1.0, 1000.0])
    got = hsr.ref_hist_stream(x, L, 2 * L, ae, le, L)
    hsr.same_ints(got, hsr.whole_row_hist(x, 2 * L, ae, le, L), "all zero")
    assert got[0][:, 0, 0].tolist() == [1, 0] and got[1][:, 0, 0].tolist() == [2 * L, 0]
    # zeros behind a last crossing: the row's last half wave begins with one non-zero sample, the rest is zero across the seam
    x = runs((40, (3,), 1.0), (88, (0,), 3.0))
    x[41:] = 0.0
    big, got = where_big(x, L, 2 * L)
    assert big == [1, 0] and got[1][0, 2, 0] == 88


def test_a_crossing_index_at_the_first_readable_sample():
    """H = L: for block 2 the first readable sample is L, a crossing index; the half wave behind it has exactly H samples, reaches
    block 2 with its last sample and has its peak there"""
    L, H = 64, 64
    x = runs((L + 1, (7,), 1.0), (H, (H - 1,), 3.0), (30, (2,), 1.0), (3 * L - (L + 1) - H - 30, (1,), 1.0))
    assert x.size == 3 * L and abs(x[2 * L]) == 3.0
    big, got = where_big(x, L, H)
    assert big == [0, 0, 1] and got[1][2, 2, 0] == H
    assert got[3].tolist() == [64, 1, 0]                                   # the first half wave has L + 1 samples


@pytest.fixture(scope="module")
def lib():
    from pyitd_amd import _lib
    _lib.build()
    return _lib.load()


def test_the_library_exports_the_histogram_stream_entries(lib):
    from pyitd_amd._lib import ABI
    for name in ENTRIES:
        assert name in ABI and hasattr(lib, name), name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pyitd_hip.h")).read()
    for name in ENTRIES:
        assert "int %s(" % name in header, name
    assert "#define ITD_STREAM_HIST 6" in header and lib.itd_abi_version() == 12
    import pyitd_amd
    assert pyitd_amd.WaveHistogramStream is pyitd_amd.streaming.WaveHistogramStream
    assert pyitd_amd.blockwise_wave_histogram is pyitd_amd.streaming.blockwise_wave_histogram
    assert pyitd_amd.StreamHistogram._fields == hsr.NAMES


def test_every_entry_refuses_a_null_stream_before_touching_a_device(lib):
    buf = ctypes.create_string_buffer(8 * 64)
    em = ctypes.c_int32(0)
    assert lib.itd_hist_stream_create(None, 0, 64, 1, 64, 64, 1, 1) == 1
    assert lib.itd_hist_stream_latency(None) == -1
    assert lib.itd_hist_stream_push_f64(None, buf, 64, buf, 0, buf, 0, buf, buf, 1, buf, buf, 1, ctypes.byref(em), None) == 1
    assert lib.itd_hist_stream_flush_f64(None, buf, 0, buf, 0, buf, buf, 1, buf, buf, 1, ctypes.byref(em), None) == 1
    assert lib.itd_hist_stream_push_host_f64(None, buf, buf, 0, buf, 0, buf, buf, buf, buf, ctypes.byref(em)) == 1
    assert lib.itd_hist_stream_flush_host_f64(None, buf, 0, buf, 0, buf, buf, buf, buf, ctypes.byref(em)) == 1


OK = dict(block=1024, rows=1, horizon=1024, hop=512, na=32, nl=32)
BAD = (dict(block=63), dict(block=4160, hop=64), dict(block=1000, hop=500), dict(rows=0), dict(rows=65536), dict(horizon=0),
       dict(horizon=(1 << 22) + 1), dict(hop=0), dict(hop=96), dict(hop=384), dict(hop=2048), dict(na=0), dict(nl=0), dict(na=65, nl=1),
       dict(na=33), dict(hop=64, na=32, nl=17), dict(block=4096, hop=512, na=32, nl=33))


def test_create_refuses_bad_shapes_before_touching_a_device(lib):
    h = ctypes.c_void_p()
    for kw in BAD:
        a = dict(OK, **kw)
        rc = lib.itd_hist_stream_create(ctypes.byref(h), 0, a["block"], a["rows"], a["horizon"], a["hop"], a["na"], a["nl"])
        assert rc == 1 and not h.value, kw


def test_the_python_surface_refuses_the_same_values_before_any_call():
    from pyitd_amd import streaming
    edges = lambda n: np.linspace(0.0, 1.0, n + 1)
    for kw in BAD:
        a = dict(OK, **kw)
        with pytest.raises(ValueError):
            streaming.WaveHistogramStream(a["block"], a["rows"], a["horizon"], edges(a["na"]), edges(a["nl"]), a["hop"])
    ok = lambda **kw: streaming.WaveHistogramStream(**dict(dict(block=512, amplitude_edges=edges(4), length_edges=edges(4)), **kw))
    with pytest.raises(ValueError):
        ok(hop=320)                                                        # does not divide the block
    with pytest.raises(ValueError):
        ok(amplitude_edges=edges(32), length_edges=edges(33))              # Na Nl > 1024
    with pytest.raises(ValueError):
        ok(hop=64, amplitude_edges=edges(32), length_edges=edges(33))
    with pytest.raises(ValueError):
        ok(block=4096, hop=64, amplitude_edges=edges(16), length_edges=edges(9))     # C Na Nl = 64 * 144 > 8192
    with pytest.raises(ValueError):
        ok(amplitude_edges=[0.0, 2.0, 1.0])                                # unordered
    with pytest.raises(ValueError):
        ok(length_edges=[1.0, 1.0, 2.0])                                   # not strictly increasing
    with pytest.raises(ValueError):
        ok(amplitude_edges=[0.0, np.nan, 1.0])
    with pytest.raises(ValueError):
        ok(length_edges=None)
    with pytest.raises(ValueError):
        ok(rows=3, amplitude_edges=np.tile(edges(4), (2, 1)))              # two rows of edges for three rows
    with pytest.raises(ValueError):
        streaming.blockwise_wave_histogram(np.zeros(1000), 512, 512, edges(4), edges(4))
