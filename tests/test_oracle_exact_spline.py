"""The exact spline references (oracle/exact_spline.py) and the layouts the GPU tests run them on (test_gpu_spline_exact.py).

1. The exact restatements reproduce every reference-generated golden of their operator to 1e-12 of the scale: that is what
   makes them the same operation, not a second transcription of the kernels.
2. zigzag() puts the detected knots exactly where a layout designs them, under both knot detectors.
3. The fp64 yardsticks of the GPU bounds (cpu_oracle.itd_baseline_extract_fast, spline_oracle.baseline) stay finite and within
   a bounded distance of the exact result on every layout, so that a numerically meaningless layout is caught here.
"""
import functools
import os

import numpy as np
import pytest

from helpers import GOLDEN
from oracle import cpu_oracle, exact_spline as ex

CUBIC = os.path.join(GOLDEN, "cubic")
SPLINE = os.path.join(GOLDEN, "spline")
YARDSTICK_ULPS = 2.0 ** 24      # fp64 oracle error / (eps * S) above which a layout is numerically meaningless

# ---- layouts ------------------------------------------------------------------------------------------------------------
# The natural operator's sweeps: a workgroup owns 1792 elements (element q = knot 1 + q forward, knot idx-2-q backward), starts
# 256 elements early, walks rounds of 1024; the evaluation stages up to 318 knots of a 512-sample tile (plus one either side).
COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1791, 1792, 1793, 2047, 2048, 2049, 3583, 3584, 3585,
          5376, 5377)
TILE_COUNTS = (317, 318, 319, 320, 321, 322)
NAK_COUNTS = (10, 15, 16, 17, 63, 64, 65, 80, 81, 1023, 1024, 1025, 1040)
RATIOS = (1e-4, 1.0, 1e4)
FAMILIES = ("uniform1", "geometric", "hugegap", "alt1_1000", "loguniform", "gap2p20")


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31)


def _geometric(up):
    g = np.maximum(1, np.round(1.087 ** np.arange(1, up + 1))).astype(np.int64)
    return np.concatenate((g, g[::-1]))


def _family_spacings(fam, rng, nak=False):
    if fam == "uniform1":
        return np.ones(2999, np.int64)
    if fam == "geometric":
        # spacings growing then shrinking at 1.087 (128 knots each way): the bound case of the backward sweep's damping,
        # v_i = h_i / (h_{i-1} + h_i) ~ 0.52.  The natural layout puts one such bump in the warm-up window in front of the first
        # forward seam (knots 1537 .. 1792) and one in the window above the first backward seam (knots idx-1794 .. idx-1538).
        bump = _geometric(128)
        if nak:
            return np.concatenate((np.full(60, 3), bump, np.full(60, 3)))
        h = np.full(3699, 2, np.int64)
        h[1537:1537 + bump.size] = bump
        h[1906:1906 + bump.size] = bump
        return h
    if fam == "hugegap":
        # isolated 2^16 gaps among spacing-1 runs (h[i-1] >> h[i], h[i-2]: the forward pair product nears 1/2), at and around the
        # first two forward seams (knots 1793, 3585)
        h = np.ones(1200 if nak else 4000, np.int64)
        for g in ((300, 649, 900) if nak else (1600, 1700, 1789, 1791, 1793, 3583)):
            h[g] = 1 << 16
        return h
    if fam == "alt1_1000":
        return np.tile(np.array([1, 1000], np.int64), 300 if nak else 1050)
    if fam == "loguniform":
        return np.round(2.0 ** (16.0 * rng.random(250 if nak else 1850))).astype(np.int64).clip(1, 1 << 16)
    if fam == "gap2p20":
        h = rng.integers(1, 5, 400)
        h[200] = 1 << 20
        return h
    raise KeyError(fam)


def _make(n_or_none, kn, rng, amp=1.0, offset=0.0):
    n = int(kn[-1]) + 4 if n_or_none is None else n_or_none
    return ex.zigzag(n, kn, ex.alternating_values(len(kn), rng, amp, offset))


def natural_layouts():
    names = ["count%d" % c for c in COUNTS] + ["tile%d" % c for c in TILE_COUNTS] + list(FAMILIES)
    names += ["uniform1_off", "hugegap_off", "gap2p20_off", "count1025_off", "edges"]
    return names


@functools.lru_cache(maxsize=None)
def natural_layout(name):
    """dict(x, knots = the designed (and detected) extrema, lst = the caller's list of idx + 1 entries, idx)."""
    rng = np.random.default_rng(_seed(name))
    base = name.partition("_off")[0]
    amp, offset = (1e-2, 1e6) if name.endswith("_off") else (1.0, 0.0)
    if base.startswith("count"):
        c = int(base[5:])                                   # elements of the sweeps: idx - 1 for the caller's list
        kn = ex.knots_from_spacings(3, rng.integers(1, 9, c + 1))
        x = _make(None, kn, rng, amp, offset)
        return dict(x=x, knots=kn, lst=kn, idx=len(kn) - 1)
    if base.startswith("tile"):
        c = int(base[4:])                                   # knots in the 512-sample tile 1536 .. 2047
        inside = np.sort(rng.choice(np.arange(1536, 2048), c, replace=False))
        kn = np.concatenate((np.arange(2, 1536, 5), inside, np.arange(2051, 4000, 5))).astype(np.int64)
        x = _make(4003, kn, rng)
        return dict(x=x, knots=kn, lst=kn, idx=len(kn) - 1)
    if base == "edges":
        # a caller's list on samples 0, 511, 512 and n-1 (every tile edge of the first tiles, and the signal's ends)
        n = 2000
        kn = ex.knots_from_spacings(2, rng.integers(2, 6, 500))
        kn = kn[kn < n - 2]
        x = _make(n, kn, rng)
        lst = np.unique(np.concatenate(([0, 511, 512, 1023, 1024, n - 1], kn[::2]))).astype(np.int64)
        return dict(x=x, knots=kn, lst=lst, idx=len(lst) - 1)
    h = _family_spacings(base, rng)
    kn = ex.knots_from_spacings(1 if base == "uniform1" else 3, h)
    x = _make(int(kn[-1]) + 2 if base == "uniform1" else None, kn, rng, amp, offset)
    return dict(x=x, knots=kn, lst=kn, idx=len(kn) - 1)


def nak_layouts():
    names = ["nak%d" % c for c in NAK_COUNTS]
    names += ["ends_%g_%g" % (a, b) for a in RATIOS for b in RATIOS]
    names += ["naks_" + f for f in FAMILIES] + ["n4990", "n4991", "n8192", "n8193"]
    return names


@functools.lru_cache(maxsize=None)
def nak_layout(name):
    """dict(x, knots = the designed (and detected) interior knots)."""
    rng = np.random.default_rng(_seed(name))
    if name.startswith("nak"):
        if name.startswith("naks_"):
            kn = ex.knots_from_spacings(2, _family_spacings(name[5:], rng, nak=True))
            return dict(x=_make(None, kn, rng), knots=kn)
        kn = ex.knots_from_spacings(2, rng.integers(1, 9, int(name[3:]) - 1))
        return dict(x=_make(None, kn, rng), knots=kn)
    if name.startswith("ends_"):
        # h0 / h1 and h_last / h_prev (sites 0 and n-1 included) at 1e-4, 1, 1e4: the folded not-a-knot rows at extreme ratios
        r0, r1 = (float(v) for v in name[5:].split("_"))
        mid = rng.integers(3, 8, 40)
        first = {1e-4: (1, 10000), 1.0: (40, 40), 1e4: (10000, 1)}[r0]
        last = {1e-4: (1, 10000), 1.0: (40, 40), 1e4: (10000, 1)}[r1]
        # h0 = first knot - 0, h1 = second - first; mirrored: h_last = (n-1) - last knot, h_prev = last - second to last
        h = np.concatenate(([first[1]], mid, [last[1]]))
        kn = ex.knots_from_spacings(first[0], h)
        n = int(kn[-1]) + last[0] + 1
        return dict(x=_make(n, kn, rng), knots=kn)
    n = int(name[1:])
    kn = ex.knots_from_spacings(3, rng.integers(1, 7, n))
    kn = kn[kn < n - 3]
    return dict(x=_make(n, kn, rng), knots=kn)


@functools.lru_cache(maxsize=None)
def natural_exact(name, mode):
    """mode "list": the caller's list; "detect": the detected knots with the e[idx] = 0 tail."""
    L = natural_layout(name)
    if mode == "list":
        return ex.natural(L["x"], L["lst"], L["idx"])
    return ex.natural(L["x"], np.concatenate((L["knots"], [0])), len(L["knots"]))


@functools.lru_cache(maxsize=None)
def nak_exact(name):
    L = nak_layout(name)
    return ex.nak(L["x"], 0, knots=L["knots"])


# ---- 1. the restatements against the reference-generated goldens ----------------------------------------------------------
def _scale(*a):
    return max(1.0, max(float(np.max(np.abs(v))) for v in a))


@pytest.mark.parametrize("name", sorted(f[:-4] for f in os.listdir(CUBIC) if f.endswith(".npz")))
def test_natural_matches_reference_goldens(name):
    g = np.load(os.path.join(CUBIC, name + ".npz"))
    r = ex.natural(g["I"], g["extrema"], int(g["idx"]))
    if "detect" in name:
        assert int(g["extrema"][int(g["idx"])]) == 0          # the e[idx] = 0 tail of detect mode
    assert np.max(r.err(g["baseline"])) <= 1e-12 * _scale(g["I"], g["baseline"]), name


@pytest.mark.parametrize("name", sorted(f[:-4] for f in os.listdir(SPLINE) if f.startswith("row_")))
def test_nak_matches_reference_goldens(name):
    g = np.load(os.path.join(SPLINE, name + ".npz"))
    r = ex.nak(g["x"], 10)
    assert np.max(r.err(g["baseline"])) <= 1e-12 * _scale(g["x"], g["baseline"]), name
    if name == "row_monotone64":
        assert np.array_equal(r.hi, g["x"]) and not r.lo.any()  # fewer than 10 knots: x itself
        return
    r0 = ex.nak(g["x"], 0)                                       # MEITD's form: no early-out
    assert np.max(r0.err(g["meitd_baseline"])) <= 1e-12 * _scale(g["x"], g["meitd_baseline"]), name


def test_iq_is_the_natural_operator_on_the_exact_mean():
    g = np.load(os.path.join(CUBIC, "cubic_radio4000_sine440.npz"))
    I = g["I"]
    Q = np.roll(I, 7) * 0.75 + 1e-3
    r = ex.iq(I, Q, g["extrema"], int(g["idx"]))
    avg = (I + Q) / 2                                            # rounded once: a few ulps, far inside 1e-12
    ref = cpu_oracle.itd_baseline_extract_fast(avg, g["extrema"], int(g["idx"]))
    assert np.max(r.err(ref)) <= 1e-12 * _scale(avg, ref)


def test_sample_subset_covers_knots_tile_edges_and_ends():
    n = 200000
    sites = np.array([0, 10, 70000, 150001, n - 1])
    s = ex.sample_subset(n, sites)
    want = {0, 9, 11, 69999, 70000, 70001, 150000, 150002, 511, 512, 1023, 1024, 599, n - 600, n - 1, 35005}
    assert want <= set(s.tolist())
    assert np.array_equal(ex.sample_subset(1000, sites[:2]), np.arange(1000))


# ---- 2. the generator: the designed knots are exactly the detected ones ---------------------------------------------------
@pytest.mark.parametrize("name", natural_layouts())
def test_natural_layout_detects_the_designed_knots(name):
    L = natural_layout(name)
    e, idx = cpu_oracle.extrema_cpp(L["x"])
    np.testing.assert_array_equal(e[:idx], L["knots"])
    if name.startswith("tile"):
        c = int(name[4:])
        assert np.count_nonzero((L["knots"] >= 1536) & (L["knots"] < 2048)) == c


@pytest.mark.parametrize("name", nak_layouts())
def test_nak_layout_detects_the_designed_knots(name):
    L = nak_layout(name)
    np.testing.assert_array_equal(cpu_oracle.knots(L["x"]), L["knots"])
    if name.startswith("ends_"):
        s = np.concatenate(([0], L["knots"], [L["x"].size - 1]))
        h = np.diff(s)
        r0, r1 = (float(v) for v in name[5:].split("_"))
        assert np.isclose(h[0] / h[1], r0) and np.isclose(h[-1] / h[-2], r1), (h[:2], h[-2:])


# ---- 3. the fp64 yardsticks stay finite and bounded -------------------------------------------------------------------------
@pytest.mark.parametrize("name", natural_layouts())
def test_natural_fp64_yardstick_is_bounded(name):
    L = natural_layout(name)
    x = L["x"]
    r = natural_exact(name, "list")
    u = r.ulps(cpu_oracle.itd_baseline_extract_fast(x, L["lst"], L["idx"]), x)
    print("%s list: err(fp64 oracle) = %.3g eps S" % (name, u))
    assert np.isfinite(u) and u <= YARDSTICK_ULPS, (name, u)
    if name != "edges":
        rd = natural_exact(name, "detect")
        e, idx = cpu_oracle.extrema_cpp(x)
        ud = rd.ulps(cpu_oracle.itd_baseline_extract_fast(x, e, idx), x)
        print("%s detect: err(fp64 oracle) = %.3g eps S" % (name, ud))
        assert np.isfinite(ud) and ud <= YARDSTICK_ULPS, (name, ud)


@pytest.mark.parametrize("name", nak_layouts())
def test_nak_fp64_yardstick_is_bounded(name):
    from oracle import spline_oracle
    L = nak_layout(name)
    r = nak_exact(name)
    u = r.ulps(spline_oracle.baseline(L["x"], 0), L["x"])
    print("%s: err(scipy) = %.3g eps S" % (name, u))
    assert np.isfinite(u) and u <= YARDSTICK_ULPS, (name, u)
