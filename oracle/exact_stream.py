"""The exact statement of the block-wise cubic stream — TEST INFRASTRUCTURE ONLY (never imported by pyitd_amd).

oracle/stream_oracle.py states the recipe (windows, the knot-giving window, select_knots, MIN_KNOTS) and runs it over fp64
operators; this file runs the SAME statement (stream_oracle.selections) over oracle/exact_spline.natural, so that every emitted
sample is known as a double-double and the GPU stream can be held to a bound of a few ulps instead of 1e-9 of the scale.
"""
from collections import namedtuple

import numpy as np

from . import cpu_oracle, exact_spline, stream_oracle

# exact: exact_spline.Exact whose samples index the CHANNEL's row (block j = samples j L .. (j+1) L - 1); sel: the selected
# knots (window samples); m: the knot-giving window's knot count; w0, wl: the window's first sample and length in the row
ExactBlock = namedtuple("ExactBlock", "exact sel m w0 wl")

# A channel whose own window holds a NaN while the knots come from channel 0's finite window (shared_knots): a spline is built
# and the NaN spreads through the sweeps in scan order — the samples are not specified.
UNSPECIFIED = "unspecified"


def exact_blockwise_cubic(x, L, margin=8, shared_knots=False):
    """x[C, n_blocks * L] -> out[c][j]: None (the block is emitted unchanged), UNSPECIFIED, or an ExactBlock."""
    x2 = np.atleast_2d(np.asarray(x, dtype=np.float64))
    C, n = x2.shape
    wins = stream_oracle.windows(n // L, L)
    out = [[None] * (n // L) for _ in range(C)]
    for c, j, W, lo, hi, knots, sel in stream_oracle.selections(cpu_oracle.extrema_cpp, x2, L, margin, shared_knots):
        if len(sel) < stream_oracle.MIN_KNOTS:
            continue
        if np.isnan(W).any():
            out[c][j] = UNSPECIFIED
            continue
        r = exact_spline.natural(W, sel, len(sel) - 1, samples=np.arange(lo, hi))
        out[c][j] = ExactBlock(exact_spline.Exact(r.samples - lo + j * L, r.hi, r.lo), sel, len(knots), wins[j][0], wins[j][1])
    return out


def scale(row, blk):
    """S = max(|window|, |exact|) of one emitted block: the scale of the bound."""
    return blk.exact.scale(row[blk.w0:blk.w0 + blk.wl])
