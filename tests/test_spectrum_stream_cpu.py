"""The spectrum stream without a GPU: the block-local rule (tests/spectrum_stream_ref.py) equals the whole-row statement — the half
waves of tests/waves_ref.py, the overlong mask, spectrum_ref on the whole row — bit for bit; known-answer cases of the horizon; the
library exports the new entries and every one of them refuses bad arguments before touching a device."""
import ctypes

import numpy as np
import pytest

import spectrum_ref as sr
import spectrum_stream_ref as ssr
from wave_stream_ref import run_length_signal

ENTRIES = ("itd_spectrum_stream_create", "itd_spectrum_stream_latency", "itd_spectrum_stream_push_f64", "itd_spectrum_stream_flush_f64",
           "itd_spectrum_stream_push_host_f64", "itd_spectrum_stream_flush_host_f64")


def legal_hops(L):
    return [h for h in range(64, L + 1, 64) if L % h == 0 and (h >= 512 or h in (64, 128, 256))]


def same_bits(got, want, what):
    for g, w, name in zip(got, want, ("power", "outside", "overlong")):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, "%s %s: %s %s vs %s %s" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if g.dtype == np.float64:
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert np.array_equal(g, w), "%s: %s differs" % (what, name)


def latency(L, H):
    return -(-(H + 1) // L)


@pytest.mark.parametrize("L", [64, 128])
def test_the_block_local_rule_is_the_whole_row_statement(L):
    rng = np.random.default_rng(2200 + L)
    edges = sr.uniform_edges(7, 0.03, 0.45)                               # part of the axis: samples fall outside without being overlong
    checked = n_overlong = n_inside = n_plain = 0
    lat = []
    for H in (1, 2, L - 2, L - 1, L, L + 1, 2 * L - 1, 2 * L):
        lat.append(latency(L, H))
        for blocks in range(1, 8):
            for zeros in (False, True):
                x = run_length_signal(rng, L, H, blocks, zeros) * ssr.envelope(blocks * L, rng)
                A, f, ln = ssr.whole_row_inst(x)
                overlong = ssr.overlong_of(ln, H)
                local = [ssr.block_inst(x, L, H, b) for b in range(blocks)]
                for hop in legal_hops(L):
                    for weight in sr.WEIGHTS:
                        want = ssr.masked_spectrum(A, f, overlong, edges, hop, weight)
                        got = [ssr.masked_spectrum(a, fr, ov, edges, hop, weight) for a, fr, ov in local]
                        got = tuple(np.concatenate([g[i] for g in got]) for i in range(3))
                        same_bits(got, want, "L=%d H=%d blocks=%d zeros=%s hop=%d %s" % (L, H, blocks, zeros, hop, weight))
                        checked += 1
                _, inside = sr.bins_of(f, edges)
                n_overlong += int(overlong.sum())
                n_inside += int((inside & ~overlong).sum())
                n_plain += int((~inside & ~overlong).sum())
    assert lat == [1, 1, 1, 1, 2, 2, 2, 3]                                # D steps at H = L - 1 -> L and at 2 L - 1 -> 2 L
    assert checked == 8 * 7 * 2 * len(legal_hops(L)) * 3
    assert n_overlong > 1000 and n_inside > 1000 and n_plain > 100, (n_overlong, n_inside, n_plain)


def waves(lengths, first=1.0):
    """alternating runs of the given lengths, each a half sine arch (so that frequencies are moderate), the first one positive"""
    out, sign = [], first
    for ln in lengths:
        out.append(sign * np.sin(np.pi * (np.arange(ln) + 0.5) / ln))
        sign = -sign
    return np.concatenate(out)


def run_blocks(x, L, H, edges, hop, weight="count"):
    got = [ssr.ref_stream_block(x, L, H, b, edges, hop, weight) for b in range(x.size // L)]
    return tuple(np.concatenate([g[i] for g in got]) for i in range(3))


def test_a_half_wave_of_exactly_the_horizon_is_binned_and_one_a_sample_longer_is_not():
    L, H = 64, 10
    x = waves([3, 4, H, 5, H + 1, 6, 7, 24])                              # 70 samples, padded to two blocks below
    x = np.concatenate((x, waves([6] * 12, -1.0)[:2 * L - x.size]))
    edges = np.array([0.0, 1.0])                                          # one bin that takes every frequency in [0, 1)
    power, outside, overlong = run_blocks(x, L, H, edges, 64)
    same_bits((power, outside, overlong), ssr.whole_row_spectrum(x, H, edges, 64, "count"), "known answer")
    _, _, ov = ssr.block_inst(x, L, H, 0)
    at = np.cumsum([0, 3, 4, H, 5, H + 1, 6, 7])
    assert not ov[at[2]:at[3]].any(), "the half wave of exactly H samples is binned"
    assert not ov[at[3]:at[4] - 1].any() and ov[at[4] - 1], "only the crossing index in front of the long half wave is overlong"
    assert ov[at[4]:at[5]].all(), "the half wave of H + 1 samples is not binned"
    assert not ov[at[5]:at[6]].any()
    assert ov[at[7]:L].all(), "24 samples > H"
    assert overlong[0] == 1 + (H + 1) + 1 + (L - at[7]) and outside[0] == overlong[0] and power[0, 0] == L - overlong[0]


def test_a_crossing_index_in_front_of_an_overlong_half_wave_is_overlong_across_the_block_seam():
    """block 0's last sample is a crossing index; the half wave that begins with block 1 has H + 1 samples"""
    L, H = 64, 70
    x = waves([20, 44, H + 1, 30, 27])                                    # 192 samples; crossings at 19, 63, 134, 164
    assert x.size == 3 * L
    edges = np.array([0.0, 1.0])
    got = run_blocks(x, L, H, edges, 64)
    same_bits(got, ssr.whole_row_spectrum(x, H, edges, 64, "count"), "seam")
    assert got[2].tolist() == [1, 64, 7]                                  # sample 63; all of block 1; samples 128 .. 134
    # with a horizon one longer nothing is overlong, and the reach is still enough
    got = run_blocks(x, L, H + 1, edges, 64)
    same_bits(got, ssr.whole_row_spectrum(x, H + 1, edges, 64, "count"), "seam, H + 1")
    assert got[2].tolist() == [0, 0, 0] and got[1].tolist() == [0, 0, 0]


def test_a_crossing_exactly_at_the_first_readable_sample():
    """H = L: for block 1 the first readable sample is 0 ... for block 2 it is L, a crossing index; the half wave behind it has exactly H
    samples and reaches block 2's first sample"""
    L, H = 64, 64
    x = waves([L + 1, H, 30, 3 * L - (L + 1) - H - 30])                   # crossings at 64, 128, 158
    assert x.size == 3 * L
    edges = np.array([0.0, 1.0])
    got = run_blocks(x, L, H, edges, 64)
    same_bits(got, ssr.whole_row_spectrum(x, H, edges, 64, "count"), "first readable sample")
    A, f, ov = ssr.block_inst(x, L, H, 2)
    assert not ov[0] and A[0] == np.abs(x[L + 1:2 * L + 1]).max(), "sample 2 L closes the half wave of exactly H samples"
    assert got[2].tolist() == [64, 1, 0]                                  # the first half wave has L + 1 samples: overlong up to sample L


@pytest.fixture(scope="module")
def lib():
    from pyitd_amd import _lib
    _lib.build()
    return _lib.load()


def test_the_library_exports_the_spectrum_stream_entries(lib):
    from pyitd_amd._lib import ABI
    for name in ENTRIES:
        assert name in ABI and hasattr(lib, name), name
    import pyitd_amd
    assert pyitd_amd.SpectrumStream is pyitd_amd.streaming.SpectrumStream


def test_every_entry_refuses_a_null_stream_before_touching_a_device(lib):
    buf = ctypes.create_string_buffer(8 * 64)
    em = ctypes.c_int32(0)
    assert lib.itd_spectrum_stream_create(None, 0, 64, 1, 64, 64, 4, 2) == 1
    assert lib.itd_spectrum_stream_latency(None) == -1
    assert lib.itd_spectrum_stream_push_f64(None, buf, 64, buf, 0, buf, 4, buf, buf, 1, ctypes.byref(em), None) == 1
    assert lib.itd_spectrum_stream_flush_f64(None, buf, 0, buf, 4, buf, buf, 1, ctypes.byref(em), None) == 1
    assert lib.itd_spectrum_stream_push_host_f64(None, buf, buf, 0, buf, buf, buf, ctypes.byref(em)) == 1
    assert lib.itd_spectrum_stream_flush_host_f64(None, buf, 0, buf, buf, buf, ctypes.byref(em)) == 1


BAD = (dict(L=63), dict(L=4160), dict(L=320, hop=128), dict(L=192, hop=192), dict(L=384, hop=192), dict(F=0), dict(F=513), dict(weight=3),
       dict(weight=-1), dict(H=0), dict(H=(1 << 22) + 1), dict(rows=0), dict(rows=65536), dict(hop=0), dict(hop=32), dict(L=32, hop=32))


def test_create_refuses_bad_shapes_before_touching_a_device(lib):
    h = ctypes.c_void_p()
    ok = dict(L=256, rows=1, H=100, hop=64, F=4, weight=2)
    for kw in BAD:
        a = dict(ok, **kw)
        assert lib.itd_spectrum_stream_create(ctypes.byref(h), 0, a["L"], a["rows"], a["H"], a["hop"], a["F"], a["weight"]) == 1, kw
        assert not h.value


def test_the_python_surface_refuses_the_same_values():
    from pyitd_amd import streaming
    ok = dict(block=256, rows=1, horizon=100, hop=64, edges=np.linspace(0, 0.5, 5), weight="energy")
    names = dict(L="block", H="horizon", F=None)
    for kw in BAD:
        a = dict(ok)
        for k, v in kw.items():
            if k == "F":
                a["edges"] = np.linspace(0, 0.5, v + 1)
            elif k == "weight":
                a["weight"] = "power"
            else:
                a[names.get(k, k)] = v
        with pytest.raises(ValueError):
            streaming.SpectrumStream(**a)
    for edges in ([0.0, 0.2, 0.2], [0.0, np.nan, 0.3], [0.0, np.inf], [0.3, 0.1], np.zeros((2, 3))):
        with pytest.raises(ValueError):
            streaming.SpectrumStream(256, edges=edges, hop=64)
    with pytest.raises(ValueError):                                       # 192 is no legal hop: it has to be given
        streaming.SpectrumStream(192, edges=[0.0, 0.5])
    with pytest.raises(ValueError):
        streaming.SpectrumStream(256)
