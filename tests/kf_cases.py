"""The case table of the fused sparse levels' deliver-or-refuse decisions (tests/test_kf_decisions_cpu.py holds the model's decision
for every case to the pinned oracle and the table to its conditions; tests/test_gpu_kf_decisions.py holds the GPU's decision to the
model's).  A case is a name, the recipe of its signal (seeds and parameters, never arrays), max_iteration, the first fused level and
the tiles per knot-side workgroup.  The signals are tiny — three full ranges and a ragged one at most — because ITD_FUSE_ONLY fuses
any length."""
import collections

import numpy as np

from helpers import chirp, coarse, fuzz_signal, sines_noise

Case = collections.namedtuple("Case", "name make m L0 tiles group edge")

# 3 (2, 2) full ranges of 16 (32, 64) tiles and a ragged one of 777 samples: 4 (3, 3) knot-side workgroups
LENGTHS = {16: 3 * 8192 + 777, 32: 2 * 16384 + 777, 64: 2 * 32768 + 777}
FAMILIES = ["white noise", "random walk", "quantised", "smooth + few knots", "sine + noise", "constant stretches", "alternating",
            "extreme magnitudes", "sines_noise", "16-bit PCM", "12-bit PCM", "chirp", "coarse"]


def pcm(x, bits):
    """x as `bits`-bit PCM in float32 (the reference's own domain)."""
    sc = float(1 << (bits - 1))
    return (np.round(x.astype(np.float64) / np.abs(x).max() * (sc - 1)) / sc).astype(np.float32)


def family_signal(fam, n, seed, dtype):
    """Family 0 .. 7: helpers.fuzz_signal's kinds; 8 sines_noise; 9 / 10 the same as 16- / 12-bit PCM (float32); 11 chirp (float32);
    12 coarse(sines_noise)."""
    if fam < 8:
        return fuzz_signal(np.random.default_rng(seed), fam, n).astype(dtype)
    if fam == 8:
        return sines_noise(n, seed=seed, dtype=dtype)
    if fam in (9, 10):
        return pcm(sines_noise(n, seed=seed), 16 if fam == 9 else 12)
    if fam == 11:
        return chirp(n)
    return coarse(sines_noise(n, seed=seed, dtype=dtype))


def zigzag(n, seed, lo=8, hi=40):
    """Piecewise linear, every vertex an extremum (heights of alternating sign, random size), vertices `lo` .. `hi` - 1 samples apart:
    the knots of every level sit at vertices.  Returns the signal and the vertex positions."""
    rng = np.random.default_rng(seed)
    pos = np.concatenate(([0], np.cumsum(rng.integers(lo, hi, size=n // lo + 2))))
    pos = pos[pos < n - 1]
    pos = np.concatenate((pos, [n - 1]))
    h = ((-1.0) ** np.arange(len(pos))) * (0.5 + rng.random(len(pos)))
    return np.interp(np.arange(n), pos, h), pos


def quiet(x, a, b):
    """x with samples [a, b) replaced by a dyadic ramp under a triangle wave of period 64: knots every 32 samples at level 0 (well inside
    the fused level-0 launch's reach), and a strictly monotone baseline — no knot at any later level — because every knot value
    B_k = x[k-1]/4 + x[k]/2 + x[k+1]/4 is exact and lies on the ramp."""
    i = np.arange(a, b)
    x = x.copy()
    x[a:b] = (i - a) / 128.0 + 1.0 - np.abs((i % 64) - 32) / 16.0
    return x


def seam_signal(n, seed, tiles, layout):
    """layouts: "plain" the zigzag alone, "pair" with 100 alternating samples across the seam of ranges 0 and 1 (the table lists seeds
    whose level-2 knots sit at the last sample of range 0, at the first of range 1, or at both: tests/test_kf_decisions_cpu.py checks
    where they sit); "empty" range 1 quiet between two dense ones;
    "last" every full range quiet: the only knots from level 1 on sit in the last, ragged range."""
    span = tiles * 512
    x, _ = zigzag(n, seed)
    if layout == "pair":        # every sample a knot at level 0 across the seam: adjacent knots survive here and there
        x[span - 50:span + 50] = ((-1.0) ** np.arange(100)) * (1 + np.random.default_rng(seed + 7).random(100))
    # (the ramp's last vertex, 64 samples in front of the stretch's end, is a knot of every level: the stretches reach 128 samples into
    #  the next range so that it is that range's)
    if layout == "empty":
        x = quiet(x, span - 64, 2 * span + 128)
    elif layout == "last":
        x = quiet(x, 0, (n // span) * span + 128)
    return x


def edge_signal(n, seed, parts):
    """A sparse carrier (sines_noise, float64) with stretches (start, length, kind) replaced: "alt" = alternating signs with random
    amplitudes (every sample a knot at level 0, the lists shrink ~2.6x per level), a number f = 1.5 sin(2 pi f i + 0.3) (f = 0.25: knots
    and sticky candidates that last through the levels; f = 0.45: 0.3 knots per sample at level 2).  The lengths were tuned with the
    model (oracle/knotfirst_model.py: decide()["loads"]) until the densest workgroup / tile sits exactly at a limit, then one above."""
    x = sines_noise(n, seed=seed, dtype=np.float64)
    for a, length, kind in parts:
        i = np.arange(length)
        if kind == "alt":
            x[a:a + length] = ((-1.0) ** i) * (1 + np.random.default_rng(seed + 1).random(length))
        else:
            x[a:a + length] = 1.5 * np.sin(2 * np.pi * kind * i + 0.3)
    return x


# (limit, load at the limit / one above, n, tiles, max_iteration, first fused level, parts at the limit, parts one above)
EDGES = [
    ("kKcCapH", 1720, LENGTHS[32], 32, 3, 2, [(16500, 8436, "alt"), (30000, 8, 0.25)], [(16500, 8464, "alt")]),
    ("kKcCap", 1024, LENGTHS[16], 16, 3, 2, [(8300, 1844, 0.25)], [(8300, 1818, 0.25), (15000, 10, 0.25)]),
    ("kKcSlab", 3200, LENGTHS[64], 64, 11, 2, [(40000, 868, 0.25), (60000, 13, 0.25)], [(40000, 886, 0.25), (60000, 13, 0.25)]),
    ("kKfCap", 128, LENGTHS[16], 16, 3, 2, [(8714, 412, 0.45)], [(8714, 406, 0.45), (9150, 12, 0.25)]),
]

# (max_iteration, first fused level): max_iteration in {3, 7, 11}, the first fused level in {2, 3, max_iteration}
LEVELS = [(3, 2), (3, 3), (7, 2), (7, 3), (7, 7), (11, 2), (11, 3), (11, 11)]

# (layout, seed) of seam_signal(LENGTHS[16], seed, 16, layout) whose level-2 knots include sample 8191 only / 8192 only / both
# (found with the model)
SEAM_SEEDS = {"last sample of range 0": ("plain", 82), "first sample of range 1": ("plain", 169), "both seam samples": ("pair", 418)}


def _family_cases():
    out = []
    k = 0
    for fam, fname in enumerate(FAMILIES):
        for tiles in (16, 32, 64):
            n = LENGTHS[tiles]
            for r in range(2):
                m, L0 = LEVELS[(k + 3 * r) % len(LEVELS)]
                k += 1
                if fam == 11:       # (the chirp sweeps up to 0.3 cycles per sample here: fused from level 2 its densest tiles also outgrow kKfCap — two reasons)
                    m, L0 = ((11, 3), (7, 3)) [r] if tiles < 64 else ((11, 3), (7, 2))[r]
                dtype = np.float64 if fam == 7 else np.float32 if fam in (9, 10, 11) else (np.float32, np.float64)[(k + fam) % 2]
                seed = 1000 + 17 * fam + tiles + r
                name = "%s seed %d n %d %s m %d L0 %d tiles %d" % (fname, seed, n, np.dtype(dtype).name, m, L0, tiles)
                out.append(Case(name, (lambda fam=fam, n=n, seed=seed, dtype=dtype: family_signal(fam, n, seed, dtype)), m, L0, tiles, "family", None))
    # each length also with the other two range sizes
    for fam in (0, 8, 9, 6):
        for tiles_n in (16, 32, 64):
            n = LENGTHS[tiles_n]
            for tiles in (16, 32, 64):
                if tiles == tiles_n:
                    continue
                m, L0 = (7, 3) if fam in (0, 6) else (7, 2)
                dtype = np.float32 if fam in (8, 9) else np.float64
                seed = 2000 + fam
                name = "%s seed %d n %d %s m %d L0 %d tiles %d" % (FAMILIES[fam], seed, n, np.dtype(dtype).name, m, L0, tiles)
                out.append(Case(name, (lambda fam=fam, n=n, seed=seed, dtype=dtype: family_signal(fam, n, seed, dtype)), m, L0, tiles, "family", None))
    # the chirp at the one length the automatic mode fuses (>= 65536 samples), with the two smaller ranges: verification at level 4
    for tiles, m in ((16, 7), (32, 11)):
        n = LENGTHS[64]
        name = "%s seed %d n %d %s m %d L0 %d tiles %d" % (FAMILIES[11], 0, n, "float32", m, 2, tiles)
        out.append(Case(name, (lambda n=n: family_signal(11, n, 0, np.float32)), m, 2, tiles, "family", None))
    # smooth + few knots: seed 3002 has its level-0 knots further apart than the fused level-0 launch reaches (the family's usual fate
    # at 70 000 samples and more), seed 3009 (25 cycles: a knot every ~500 samples at level 0, 2 per level from level 1 on) is in reach
    for tiles in (16, 32, 64):
        n = LENGTHS[tiles]
        for seed, dtype in ((3002, np.float32), (3002, np.float64), (3009, np.float64)):
            name = "%s seed %d n %d %s m %d L0 %d tiles %d" % (FAMILIES[3], seed, n, np.dtype(dtype).name, 7, 2, tiles)
            out.append(Case(name, (lambda n=n, seed=seed, dtype=dtype: family_signal(3, n, seed, dtype)), 7, 2, tiles, "family", None))
    return out


def _seam_cases():
    out = []
    n = LENGTHS[16]
    for what, (layout, seed) in SEAM_SEEDS.items():
        out.append(Case("seam: a level-2 knot at the %s, zigzag seed %d" % (what, seed), (lambda layout=layout, seed=seed: seam_signal(n, seed, 16, layout)), 7, 2, 16, "seam", what))
    for tiles in (16, 32):
        nn = LENGTHS[16] if tiles == 16 else 3 * 16384 + 777
        out.append(Case("seam: an empty range between two dense ones, zigzag seed 5 n %d tiles %d" % (nn, tiles), (lambda nn=nn, tiles=tiles: seam_signal(nn, 5, tiles, "empty")), 7, 2, tiles, "seam", "empty"))
    out.append(Case("seam: knots in the last, ragged range only, zigzag seed 6", (lambda: seam_signal(n, 6, 16, "last")), 7, 2, 16, "seam", "last"))
    out.append(Case("seam: knots in the last, ragged range only, zigzag seed 6, from level 3", (lambda: seam_signal(n, 6, 16, "last")), 11, 3, 16, "seam", "last"))
    return out


def _edge_cases():
    out = []
    for limit, load, n, tiles, m, L0, at, above in EDGES:
        out.append(Case("edge: %s at %d" % (limit, load), (lambda n=n, at=at: edge_signal(n, 0, at)), m, L0, tiles, "edge", (limit, load)))
        out.append(Case("edge: %s at %d" % (limit, load + 1), (lambda n=n, above=above: edge_signal(n, 0, above)), m, L0, tiles, "edge", (limit, load + 1)))
    return out


CASES = _family_cases() + _seam_cases() + _edge_cases()
