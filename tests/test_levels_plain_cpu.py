"""The levels stream's plain-rules reference (tests/levels_plain_ref.py) anchored without a GPU:
  * on finite draws it equals the C-oracle composition (test_levels_stream_cpu.levels_composition) bit for bit, rows and flags;
  * its flags are sound against the whole-signal oracle (oracle/cpu_oracle.itd(x, M-1)) on a fuzz grid of six signal families times
    four modes (one NaN, one infinity, a leading plateau, clean): every certified block equals the whole-signal rows bit for bit,
    also where a non-finite sample elsewhere sends the whole-signal run through its NaN branch (rule (b) of itd_stream.hpp);
  * known answers of rules (c) and (d) at their edges, on hand-built windows."""
import functools

import numpy as np
import pytest

from helpers import assert_bits_equal
from levels_plain_ref import (EDGE_BLOCK, EDGE_BLOCKS, EDGE_CASES, EDGE_L, GRID_DRAWS, certified_against_whole, edge_signal, grid_cells,
                              grid_draws, plain_composition)
from test_levels_stream_cpu import levels_composition, stage_exact, window_knots

MIN_TIMEOUTS, MIN_CERTIFIED = 30, 50            # per cell of 100 draws: the fuzz cannot pass empty


@functools.lru_cache(maxsize=None)
def cell(kind, mode):
    """per draw of the cell: (x, L, M, rows, exact, status)"""
    out = []
    for x, L, M in grid_draws(kind, mode):
        rows, exact, status = plain_composition(x, L, M)
        out.append((x, L, M, rows, exact, status))
    return out


@pytest.mark.parametrize("kind,mode", grid_cells())
def test_certified_blocks_equal_the_whole_signal_whatever_lies_elsewhere(kind, mode):
    timeouts = compared = 0
    for i, (x, L, M, rows, exact, status) in enumerate(cell(kind, mode)):
        ended, n_cert, unsound = certified_against_whole(x, L, M, rows[0], exact[0])
        assert not unsound, "kind %d mode %s draw %d (L=%d M=%d): certified blocks %s differ from the whole signal" % (kind, mode, i, L, M, unsound)
        timeouts += ended
        compared += n_cert
    print("kind %d mode %-7s: %d of %d draws end 'timeout', %d certified blocks compared" % (kind, mode, timeouts, GRID_DRAWS, compared))
    assert timeouts >= MIN_TIMEOUTS, "only %d draws ended 'timeout': pick another seed" % timeouts
    assert compared >= MIN_CERTIFIED, "only %d certified blocks compared: pick another seed" % compared


def test_finite_draws_equal_the_c_oracle_composition():
    finite_draws = 0
    for kind, mode in grid_cells():
        if mode in ("nan", "inf"):
            continue                                       # never finite
        for i, (x, L, M, rows, exact, status) in enumerate(cell(kind, mode)):
            with np.errstate(all="ignore"):
                ref_rows, ref_exact, finite = levels_composition(x, L, M)
            if not finite:
                continue
            finite_draws += 1
            assert status == 0
            assert_bits_equal(rows, ref_rows, "kind %d mode %s draw %d rows" % (kind, mode, i))
            np.testing.assert_array_equal(exact, ref_exact)
    print("%d finite draws compared" % finite_draws)
    assert finite_draws >= 300, "every clean draw of five families is finite"


def test_modes_do_what_they_say():
    """the non-finite modes are never certified in a window that holds the sample, and set status 2 where it is a NaN"""
    for kind, mode in grid_cells():
        for x, L, M, rows, exact, status in cell(kind, mode)[:20]:
            bad = np.nonzero(~np.isfinite(x))[0]
            assert len(bad) == (1 if mode in ("nan", "inf") else 0)
            if mode == "nan":
                assert status == 2
            if mode == "clean" and kind in (0, 4, 6):
                assert status == 0                         # (a quantised draw may start on a plateau: 0/0 in its first segment)
            for p in bad:
                j = int(p) // L
                assert not exact[0, max(j - 1, 0):j + 2].any()


@pytest.mark.parametrize("knots,expected", EDGE_CASES)
def test_known_answers_at_the_rules_edges(knots, expected):
    L, j = EDGE_L, EDGE_BLOCK
    x = edge_signal(knots)
    w = x[(j - 1) * L:(j + 2) * L]
    assert [int(k) for k in window_knots(w)] == [k for k in knots if 1 <= k <= 3 * L - 2], "the hand-built window's knots"
    assert bool(stage_exact(x[None], L, None)[0, j]) == expected
    # stage M's flag implies stage 0's of the same block (rule (a))
    rows, exact, status = plain_composition(x, L, 1)
    assert status == 0 and len(x) == L * EDGE_BLOCKS
    if not expected:
        assert not exact[0, j]
