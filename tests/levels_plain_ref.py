"""The levels stream's reference under the plain rules — TEST INFRASTRUCTURE ONLY.

plain_composition states what itd_levels_stream_* promises on ANY input (a NaN, an infinity, a plateau under a window start,
silence): the recipe of oracle/stream_oracle.py (windows / blockwise_linear) with the tier-1 operator under the plain rules,
oracle/numpy_itd.baseline_extract(w, plain_nan=True) — a comparison with a NaN is false, nothing is overwritten with +inf, the
arithmetic of ITD.py:100-117 runs as written — applied M+1 times, each stage on the previous stage's baseline.  It shares no code with
the device, with the single-level streams or with the C oracle; test_levels_plain_cpu.py holds it to the C-oracle composition
(test_levels_stream_cpu.levels_composition) bit for bit wherever that one is defined, and its flags to the whole-signal oracle.
"""
import numpy as np

from oracle import numpy_itd
from oracle.stream_oracle import blockwise_linear
from test_levels_stream_cpu import stage_exact


def _extract(w):
    return numpy_itd.baseline_extract(w, plain_nan=True)[:2]


def plain_composition(x, L, M):
    """(rows[C, M+1, n], exact[C, n_blocks], status) of x[C, n_blocks * L] (or one channel [n]): rows 0 .. M-1 the rotations of stages
    0 .. M-1, row M stage M's rotation + baseline (added in that order); the flags by the rule of test_levels_stream_cpu.stage_exact;
    status 2 if any stage's input holds a NaN, else 0."""
    cur = np.atleast_2d(np.asarray(x, dtype=np.float64))
    rows, flags, status = [], None, 0
    for k in range(M + 1):
        if np.isnan(cur).any():
            status = 2
        rot, base = blockwise_linear(_extract, cur, L)
        with np.errstate(all="ignore"):
            flags = stage_exact(cur, L, flags)
            rows.append(rot if k < M else rot + base)
        cur = base
    return np.stack(rows, axis=1), flags, status


# ---- the draws of the soundness fuzz grid (test_levels_plain_cpu.py, test_gpu_levels_stream_hard.py, tools/stream_fuzz.py) ---
FAMILIES = (0, 4, 6, 2, 1, 7)                   # fuzz_signal kinds: noise, sines + noise, alternating, quantised, random walk, 1e+-300
MODES = ("nan", "inf", "plateau", "clean")
GRID_SEED = 20261023                            # (a seed under which every cell meets the tests' conditions; 20261021 / 22 leave the random walk short)
GRID_DRAWS = 100


def grid_draw(rng, kind, mode):
    """one draw of a cell: (x[n_blocks * L], L, M)"""
    from helpers import fuzz_signal
    L = int(rng.choice((8, 9, 13, 16)))
    M = int(rng.integers(1, 4))
    nb = int(rng.integers(6, 16))
    x = fuzz_signal(rng, kind, nb * L)
    if mode == "nan":
        x[rng.integers(0, nb * L)] = np.nan
    elif mode == "inf":
        x[rng.integers(0, nb * L)] = np.inf if rng.random() < 0.5 else -np.inf
    elif mode == "plateau":
        x[:rng.integers(2, 6)] = x[0]
    return x, L, M


def grid_cells():
    return [(kind, mode) for kind in FAMILIES for mode in MODES]


def grid_draws(kind, mode, count=GRID_DRAWS):
    """the first `count` draws of a cell; a cell's draws depend on the seed and the cell alone"""
    rng = np.random.default_rng([GRID_SEED, kind, MODES.index(mode)])
    return [grid_draw(rng, kind, mode) for _ in range(count)]


# ---- known answers at the rule's edges ------------------------------------------------------------------------------------
EDGE_L, EDGE_BLOCKS, EDGE_BLOCK = 8, 5, 2       # block 2 of 5: its window is stream samples 8 .. 31 (n = 24, lo = 8, hi = 16)
# (knots in window samples, stage 0's flag of the block by rules (c) and (d)): left = knots in 1 .. lo, right = knots in hi .. n-2
EDGE_CASES = [
    ((3, 6, 17, 20), True),       # two either side
    ((3, 17, 20), False),         # exactly one on the left
    ((17, 20), False),            # none on the left
    ((3, 8, 17, 20), True),       # a knot exactly at lo counts on the left
    ((8, 17, 20), False),         # ... but it is one knot
    ((3, 9, 17, 20), False),      # lo + 1 does not count
    ((3, 6, 17), False),          # exactly one on the right
    ((3, 6), False),              # none on the right
    ((3, 6, 16, 20), True),       # a knot exactly at hi counts on the right
    ((3, 6, 16), False),          # ... but it is one knot
    ((3, 6, 15, 20), False),      # hi - 1 does not count
    ((3, 8, 15), False),          # lo counts left, hi - 1 on neither side
    ((3, 6, 20, 22), True),       # n - 2 is the last sample that can be a knot
    ((3, 6, 20, 23), False),      # n - 1 is the window's end, never an interior knot
    ((1, 2, 21, 22), True),       # the outermost samples that count
    ((3, 6, 10, 13, 17, 20), True),   # knots inside the block change nothing
    ((10, 13), False),
]


def edge_signal(knots):
    """EDGE_BLOCKS blocks of EDGE_L samples: a zigzag of slope +-1 that turns exactly at the given window samples of block
    EDGE_BLOCK's window (and nowhere else: no plateaus, no other knots)"""
    n = EDGE_L * EDGE_BLOCKS
    turn = np.zeros(n, dtype=bool)
    turn[np.asarray(knots, dtype=np.int64) + (EDGE_BLOCK - 1) * EDGE_L] = True
    x, slope = np.zeros(n), 1.0
    for i in range(1, n):
        if turn[i - 1]:
            slope = -slope
        x[i] = x[i - 1] + slope
    return x


def certified_against_whole(x, L, M, rows, exact):
    """(ended "timeout" with M+1 rows, certified blocks compared, [unsound blocks]) of one channel's rows[M+1, n] / exact[n_blocks]
    against the whole-signal oracle cpu_oracle.itd(x, M-1)"""
    from test_levels_stream_cpu import whole_rows
    whole, stop = whole_rows(np.array(x, dtype=np.float64), M)       # (a copy: the oracle's NaN branch overwrites)
    if stop != "timeout" or whole.shape[0] != M + 1:
        return False, 0, []
    a, b = np.ascontiguousarray(rows), np.ascontiguousarray(whole)
    same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    cert = np.nonzero(exact)[0]
    return True, len(cert), [int(j) for j in cert if not same[:, j * L:(j + 1) * L].all()]
