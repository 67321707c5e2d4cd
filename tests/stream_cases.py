"""Layouts, references and the comparison of the exact tests of the block-wise cubic stream (itd_stream_* with ITD_STREAM_CUBIC).
Nothing here needs a GPU: tests/test_stream_exact_cpu.py holds the generators to the conditions they are named after and the
comparison to raising on planted defects, tests/test_gpu_stream_exact.py runs the device stream through the same comparison.

Every designed layout is an exact_spline.zigzag, so both knot detectors find exactly the designed knots.  A case is
dict(x float64[C, nb L], L, margin, shared); its exact statement is oracle/exact_stream.py's, its fp64 yardstick
oracle/stream_oracle.py's oracle_blockwise_cubic.

The bound is tests/test_gpu_spline_exact.py's, per emitted block, with S = max(|window|, |exact|) and eps = 2^-52:
    max err(stream) <= C_REF max err(fp64 oracle) + C_ABS eps S;
a block the exact statement emits unchanged must equal the input bit for bit (rotation: exactly 0).
"""
import functools

import numpy as np

from oracle import cpu_oracle, exact_spline as ex, exact_stream as es, stream_oracle as so

EPS = 2.0 ** -52
C_REF, C_ABS = 4.0, 64.0      # restated from tests/test_gpu_spline_exact.py (test_stream_exact_cpu.py holds them equal)
SENT = -7.25e300              # sentinel of stride gaps and of blocks not yet emitted

GEOM_L = (8, 24, 64, 100, 511, 512, 513, 1000, 1024, 2048, 4096)
GEOM_FAMILIES = ("designed", "alt", "noise", "sparse")
MARGINS = (1, 2, 8, 64)
RING_NB = (1, 2, 3, 4, 7)     # seven blocks pass every ring slot twice
SEAMS = {"m1": (-1,), "0": (0,), "p1": (1,), "all": (-1, 0, 1)}
SEAM_L, SEAM_NB = 24, 4
COUNTS_PER_BLOCK = (0, 0, 0, 1, 1, 1, 2)       # knots per block: the windows hold 0, 0, 1, 2, 3, 4, 3
COUNTS_PER_WINDOW = (0, 0, 1, 2, 3, 4, 3)


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31)


def _zig(n, kn, rng, amp=1.0, offset=0.0):
    return ex.zigzag(n, kn, ex.alternating_values(len(kn), rng, amp, offset))


def seam_knots(nb, L, offsets):
    """A few knots inside every block and, at every block seam g = j L, knots at g + offsets (stream samples)."""
    inner = np.unique(np.linspace(3, L - 4, 5).astype(np.int64))
    parts = [j * L + inner for j in range(nb)]
    parts += [g + np.asarray(offsets, dtype=np.int64) for g in range(L, nb * L, L)]
    return np.unique(np.concatenate(parts))


def family_signal(fam, nb, L, rng):
    n = nb * L
    if fam == "designed":
        return _zig(n, seam_knots(nb, L, SEAMS["all"]), rng)
    if fam == "alt":                                # L - 2 knots per block: every sample but a block's first and last
        i = np.arange(n)
        return _zig(n, i[(i % L != 0) & (i % L != L - 1)], rng)
    if fam == "noise":
        # white noise has 2/3 knots per sample, 321 .. 361 per 512-sample tile: never below the evaluation's staging limit (318
        # knots of the tile and one either side).  A first-order moving average of it has 290 .. 346: tiles on both sides
        w = rng.standard_normal(n + 1)
        return w[1:] + 0.2 * w[:-1]
    assert fam == "sparse"                          # one knot every ~L/7 samples
    step = max(1, L // 7)
    kn = ex.knots_from_spacings(2, rng.integers(max(1, step - step // 4), step + step // 4 + 2, 8 * nb + 8))
    return _zig(n, kn[kn <= n - 3], rng)


def names():
    out = ["seam_%s_m%d" % (s, m) for s in SEAMS for m in MARGINS]
    out += ["counts_m1", "counts_m8", "behind2_m1", "behind3_m1"]
    out += ["geom_%s_L%d" % (f, L) for f in GEOM_FAMILIES for L in GEOM_L]
    out += ["ring_%s_nb%d" % (f, nb) for f in ("noise", "designed") for nb in RING_NB]
    out += ["chan3_%s_L%d" % (k, L) for k in ("own", "shared") for L in (100, 512)]
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(_seed(name))
    kind, _, rest = name.partition("_")
    shared = False
    if kind == "seam":
        which, _, m = rest.partition("_m")
        L, margin = SEAM_L, int(m)
        x = _zig(SEAM_NB * L, seam_knots(SEAM_NB, L, SEAMS[which]), rng)
    elif kind == "counts":
        L, margin = 64, int(rest[1:])
        kn = [j * L + p for j, c in enumerate(COUNTS_PER_BLOCK) for p in ((30,) if c == 1 else (20, 40) if c == 2 else ())]
        x = _zig(len(COUNTS_PER_BLOCK) * L, np.asarray(kn, dtype=np.int64), rng)
    elif kind in ("behind2", "behind3"):
        # margin 1, no knot inside the emitted block 1: one knot in front of it and 2 (3) behind it are selected
        L, margin = 64, 1
        kn = [20, 40] + ([2 * L + 20, 2 * L + 40] if kind == "behind2" else [2 * L + 20, 2 * L + 35, 2 * L + 50])
        x = _zig(3 * L, np.asarray(kn, dtype=np.int64), rng)
    elif kind == "geom":
        fam, _, l = rest.partition("_L")
        L, margin = int(l), {"designed": 1, "sparse": 2}.get(fam, 8)       # few knots per block: margins that do not take them all
        x = family_signal(fam, 4, L, rng)
    elif kind == "ring":
        fam, _, nb = rest.partition("_nb")
        L, margin = (100, 8) if fam == "noise" else (64, 2)
        x = family_signal(fam, int(nb), L, rng)
    else:
        assert kind == "chan3"
        k, _, l = rest.partition("_L")
        L, nb, shared = int(l), 4, k == "shared"
        margin = 8 if L == 512 else 2
        rows = []
        for amp, offset, first in ((1.0, 0.0, 2), (0.7, 3.0, 5), (2.0, -1.0, 3)):   # other zigzags: their extrema are not channel 0's
            step = max(2, L // 12)
            kn = ex.knots_from_spacings(first, rng.integers(step - step // 3, step + step // 3 + 2, 16 * nb + 16))
            rows.append(_zig(nb * L, kn[kn <= nb * L - 3], rng, amp, offset))
        x = np.stack(rows)
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    x.setflags(write=False)
    return dict(x=x, L=L, margin=margin, shared=shared)


@functools.lru_cache(maxsize=None)
def exact(name):
    c = case(name)
    return es.exact_blockwise_cubic(c["x"], c["L"], c["margin"], c["shared"])


@functools.lru_cache(maxsize=None)
def oracle(name):
    c = case(name)
    ref = so.oracle_blockwise_cubic(c["x"], c["L"], c["margin"], c["shared"])
    ref.setflags(write=False)
    return ref


def selections(name):
    """[(channel, block, W, lo, hi, knots, sel)] of a case (stream_oracle.selections over cpu_oracle.extrema_cpp)."""
    c = case(name)
    return list(so.selections(cpu_oracle.extrema_cpp, c["x"], c["L"], c["margin"], c["shared"]))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def check(what, blocks, got, x, L, ref, rot=None):
    """Hold got[C, nb L] (and rot) to the exact statement `blocks`; ref: the fp64 oracle's result.  Prints one RATIO line;
    returns (max err(got), max err(fp64 oracle)) in eps S over the emitted splines."""
    got = np.atleast_2d(got)
    assert got.shape == x.shape, what
    worst_g = worst_r = 0.0
    splines = unchanged = 0
    for c, row in enumerate(blocks):
        for j, blk in enumerate(row):
            sl = slice(j * L, (j + 1) * L)
            where = "%s: channel %d block %d" % (what, c, j)
            if blk is es.UNSPECIFIED:
                continue
            if blk is None:
                unchanged += 1
                assert _same_bits(got[c, sl], x[c, sl]), where + " is not the input bit for bit"
                if rot is not None:
                    assert _same_bits(rot[c, sl], np.zeros(L)), where + ": the rotation of an unchanged block is not 0"
                continue
            splines += 1
            S = es.scale(x[c], blk)
            assert np.all(np.isfinite(got[c, sl])), where
            e_g = float(np.max(blk.exact.err(got[c]))) / (EPS * S)
            e_r = float(np.max(blk.exact.err(ref[c]))) / (EPS * S)
            worst_g, worst_r = max(worst_g, e_g), max(worst_r, e_r)
            assert e_g <= C_REF * e_r + C_ABS, "%s: err %.3g eps S, fp64 oracle %.3g eps S" % (where, e_g, e_r)
            if rot is not None:
                assert _same_bits(rot[c, sl], x[c, sl] - got[c, sl]), where + ": rotation != x - baseline"
    print("RATIO %-40s gpu %9.3g  fp64 %9.3g  (eps S)  %d splines, %d unchanged" % (what, worst_g, worst_r, splines, unchanged))
    return worst_g, worst_r


# ---- the I/Q operator on detected common knots --------------------------------------------------------------------------
IQ_N = (513, 1025, 2 * 512 + 514, 64 * 512 + 700)     # the last one: above 64 tiles


@functools.lru_cache(maxsize=None)
def iq_case(n, extra):
    """dict(I, Q, knots): both components have their extrema exactly at `knots`.  extra = False: Q = 0.5 I + offset; True: Q is a
    zigzag on a superset — inside some of I's monotone segments Q has a maximum and a minimum more, which must not become knots."""
    rng = np.random.default_rng([n, int(extra)])
    kn = ex.knots_from_spacings(3, rng.integers(1, 9, n // 4))
    kn = kn[kn <= n - 3]
    I = _zig(n, kn, rng)
    if not extra:
        return dict(I=I, Q=0.5 * I + 3.0, knots=kn)
    sup = []
    for a, b in zip(kn[:-1], kn[1:]):
        sup.append(a)
        if b - a >= 4 and rng.random() < 0.5:       # a + 1 and a + 2 are not next to b: I's predicate at a, b sees I alone
            sup += [a + 1, a + 2]
    sup.append(kn[-1])
    sup = np.asarray(sup, dtype=np.int64)
    assert sup.size > kn.size
    return dict(I=I, Q=_zig(n, sup, rng, 0.8, -2.0), knots=kn)
