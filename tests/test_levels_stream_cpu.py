"""The levels stream without a GPU: the C ABI refuses bad arguments before touching a device, and the exactness rule, stated
here in plain numpy over the composition of oracle_blockwise_linear, is sound against the whole-signal oracle.

The rule (the device's statement: pyitd_amd/csrc/itd_stream.hpp, k_stream_levels).  Stage k's block j is exact when
  (a) k = 0, or stage k-1's blocks in the window are all exact;
  (b) every window sample is finite;
  (c) the window starts at the stream start, or >= 2 knots lie in window samples 1 .. lo;
  (d) the block is the stream's last (its window ends at the stream end), or >= 2 knots lie in window samples hi .. n-2;
knots by the 3-sample predicate of ITD.py:44-59 / 87-98 (dx[i-1] <= 0 < dx[i] or dx[i-1] >= 0 > dx[i]).  A block's flag is
stage M's."""
import ctypes

import numpy as np
import pytest

from helpers import fuzz_signal


def window_knots(w):
    """interior knots of the window w, plain comparisons"""
    d0, d1 = w[1:-1] - w[:-2], w[2:] - w[1:-1]
    with np.errstate(invalid="ignore"):
        f = ((d1 > 0) & (d0 <= 0)) | ((d1 < 0) & (d0 >= 0))
    return np.nonzero(f)[0] + 1


def stage_exact(x, L, prev):
    """E_k of every block of every channel: x[C, n] is the stage's input, prev[C, n_blocks] stage k-1's flags (None: k = 0)"""
    from oracle.stream_oracle import windows
    C, n = x.shape
    nb = n // L
    out = np.zeros((C, nb), dtype=bool)
    for c in range(C):
        for j, (w0, wl, lo, hi) in enumerate(windows(nb, L)):
            w = x[c, w0:w0 + wl]
            kn = window_knots(w)
            ok = prev is None or bool(prev[c, w0 // L:(w0 + wl) // L].all())
            ok = ok and bool(np.isfinite(w).all())
            ok = ok and (w0 == 0 or int(np.count_nonzero(kn <= lo)) >= 2)
            ok = ok and (j == nb - 1 or int(np.count_nonzero(kn >= hi)) >= 2)
            out[c, j] = ok
    return out


def levels_composition(x, L, M):
    """(rows[C, M+1, n], exact[C, n_blocks], finite): oracle_blockwise_linear applied M+1 times, each to the previous baseline,
    and the rule above; finite = no stage input held a non-finite sample (else the oracle's NaN branch is not the stream's)"""
    from oracle.stream_oracle import oracle_blockwise_linear
    cur = np.atleast_2d(np.asarray(x, dtype=np.float64))
    rows, flags, finite = [], None, True
    for k in range(M + 1):
        finite = finite and bool(np.isfinite(cur).all())
        with np.errstate(all="ignore"):
            rot, base = oracle_blockwise_linear(cur, L)
        flags = stage_exact(cur, L, flags)
        with np.errstate(all="ignore"):
            rows.append(rot if k < M else rot + base)
        cur = base
    return np.stack(rows, axis=1), flags, finite


def whole_rows(x, M):
    from oracle import cpu_oracle
    with np.errstate(all="ignore"):
        r = cpu_oracle.itd(np.asarray(x, dtype=np.float64), M - 1)
    return r["rows"], r["stop"]


def rich_signal(n):
    """white noise: knots stay dense enough through level 6 for 1024-sample blocks (found with the rule above)"""
    return np.random.default_rng(2).standard_normal(n)


# ---- argument refusals (no device is touched) ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pyitd_amd import _lib
    _lib.build()
    return _lib.load()


def test_create_refuses_bad_shapes_before_touching_a_device(lib):
    h = ctypes.c_void_p()
    for L, C, M in ((7, 1, 4), (4, 1, 4), (1 << 30, 1, 4), (64, 0, 4), (64, 65536, 4), (64, 1, 0), (64, 1, 22), (64, 1, -1)):
        assert lib.itd_levels_stream_create(ctypes.byref(h), 0, L, C, M) == 1, (L, C, M)
        assert not h.value
    assert lib.itd_levels_stream_create(None, 0, 64, 1, 4) == 1


def test_push_and_flush_refuse_a_null_stream_or_block(lib):
    buf = ctypes.create_string_buffer(8 * 64 * 8)
    em = ctypes.c_int32(0)
    assert lib.itd_levels_stream_push_f64(None, buf, 64, buf, 64, 512, None, ctypes.byref(em), None) == 1
    assert lib.itd_levels_stream_flush_f64(None, buf, 64, 512, None, ctypes.byref(em), None) == 1
    assert lib.itd_levels_stream_push_host_f64(None, buf, buf, None, ctypes.byref(em)) == 1
    assert lib.itd_levels_stream_flush_host_f64(None, buf, None, ctypes.byref(em)) == 1
    assert lib.itd_levels_stream_set_sequence(None, 1) == 1
    assert lib.itd_levels_stream_form(None) == -1


def test_python_surface_refuses_bad_shapes():
    from pyitd_amd import streaming
    for kw in (dict(block=7, levels=4), dict(block=1 << 30, levels=4), dict(block=64, levels=0), dict(block=64, levels=22),
               dict(block=64, levels=4, channels=0)):
        with pytest.raises(ValueError):
            streaming.LevelsStream(**kw)
    with pytest.raises(ValueError):
        streaming.blockwise_itd(np.zeros(100), 64, 4)


# ---- the rule, on the CPU oracles alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,L,M", [(4, 64, 3), (3, 100, 2), (1, 64, 2), (0, 24, 5), (6, 32, 2), (2, 50, 3)])
def test_certified_blocks_equal_the_whole_signal(kind, L, M):
    rng = np.random.default_rng(100 + kind)
    nb = 9
    x = fuzz_signal(rng, kind, nb * L)
    rows, exact, finite = levels_composition(x, L, M)
    whole, stop = whole_rows(x, M)
    assert stop == "timeout" and finite, "the draws are fixed: the whole run ends out of time, every stage input is finite"
    for j in np.nonzero(exact[0])[0]:
        s = slice(j * L, (j + 1) * L)
        assert np.array_equal(rows[0][:, s].view(np.uint64), whole[:, s].view(np.uint64)), (kind, L, M, j)


def test_a_rich_signal_certifies_every_block():
    L, M, nb = 1024, 6, 6
    x = rich_signal(nb * L)
    rows, exact, finite = levels_composition(x, L, M)
    whole, stop = whole_rows(x, M)
    assert finite and stop == "timeout"
    assert exact.all()
    assert np.array_equal(rows[0].view(np.uint64), whole.view(np.uint64))


def test_deep_levels_with_short_blocks_need_the_flag():
    L, M, nb = 64, 8, 12
    x = fuzz_signal(np.random.default_rng(7), 0, nb * L)
    rows, exact, finite = levels_composition(x, L, M)
    whole, stop = whole_rows(x, M)
    assert finite and stop == "timeout"
    differs = [j for j in range(nb) if not np.array_equal(rows[0][:, j * L:(j + 1) * L].view(np.uint64),
                                                          whole[:, j * L:(j + 1) * L].view(np.uint64))]
    assert differs, "no block differs: pick another draw"
    assert not exact[0, differs].any()
