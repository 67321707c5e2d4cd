"""pyitd_amd/meitd.py's selection loop against the reference's own MEITD / XITD / retrieve_proper_rotation /
determine_if_first_is_proper_rotation (MEITD.py:344-549) on tests/golden/meitd/: cases oracle/gen_golden.py (make_meitd_branch_cases)
chose so that together they take every branch of the reference's three functions — the dig loop, the three early exits, thresholds
other than 0.6 — and that the reference decides with room to spare.  Here the loop runs over numpy rows and the oracle's operators
(oracle.meitd_oracle.CpuWork): bit for bit.  No GPU; tests/test_gpu_meitd_reference.py runs the same cases on the device."""
import hashlib
import os

import numpy as np
import pytest
import scipy

from helpers import GOLDEN, assert_bits_equal
from oracle import meitd_oracle
import pyitd_amd.meitd as mm

MEITD = os.path.join(GOLDEN, "meitd")
INDEX = np.load(os.path.join(MEITD, "index.npz"))
NAMES = [str(s) for s in INDEX["names"]]


def load(name):
    return np.load(os.path.join(MEITD, name + ".npz"))


@pytest.fixture
def cpu_work(monkeypatch):
    """pyitd_amd.meitd's device rows and operators replaced by CpuWork, its entropy by the oracle's: the works of the test's calls"""
    works = []

    def work_for(n, device=0, solver="auto"):
        works.append(meitd_oracle.CpuWork(n))
        return works[-1]

    monkeypatch.setattr(mm, "_work_for", work_for)
    monkeypatch.setattr(mm, "weighted_permutation_entropy",
                        lambda ts, order=3, normalize=False, device=0: meitd_oracle.weighted_permutation_entropy(ts, order, normalize))
    return works


def test_the_index_names_the_files():
    assert sorted(NAMES) == sorted(f[:-4] for f in os.listdir(MEITD) if f != "index.npz")
    assert 16 <= len(NAMES) <= 28


def test_the_cases_reach_every_branch_of_the_reference():
    executable, unreached = set(INDEX["executable_lines"].tolist()), set(INDEX["unreached"].tolist())
    assert unreached <= {488} and unreached <= executable
    if unreached:
        assert int(INDEX["short_candidates_searched"]) >= 5000
    g = {name: load(name) for name in NAMES}

    def union(sel):
        return set().union(*[set(g[k]["lines"].tolist()) for k in NAMES if sel(g[k])])

    assert union(lambda r: True) == executable - unreached
    # the lengths the one-launch kernels take reach the same lines
    device = union(lambda r: 1024 <= r["x"].size <= 8192)
    assert device == executable - unreached
    at06 = union(lambda r: float(r["wpemax"]) == 0.6)
    assert {461, 508} <= at06
    assert {414, 433, 461, 508, 513} <= device
    lengths = {int(g[k]["x"].size) for k in NAMES}
    assert {1024, 4800, 5000, 8192, 600} <= lengths and all(n in (1024, 4800, 5000, 8192, 600) or 100 <= n <= 300 for n in lengths)
    assert len({float(g[k]["wpemax"]) for k in NAMES}) >= 4
    for k in NAMES:
        assert float(g[k]["margin_entropy"]) >= 1e-6 and float(g[k]["margin_perturbed"]) <= 1e-10 and float(g[k]["margin_ties"]) >= 1e-12, k
        if "margin_xitd" in g[k]:
            assert float(g[k]["margin_xitd"]) >= 1e-9, k
        if g[k]["x"].size >= 4800:
            assert len(g[k]["high"]) + len(g[k]["low"]) <= 8, k


def test_the_fixtures_stay_small():
    sizes = [os.path.getsize(os.path.join(MEITD, f)) for f in os.listdir(MEITD)]
    assert max(sizes) <= 1 << 20 and sum(sizes) < 4 * 1000 * 1000


@pytest.mark.parametrize("name", NAMES)
def test_meitd_matches_the_reference_bit_for_bit(name, cpu_work):
    g = load(name)
    assert str(g["scipy_version"]) == scipy.__version__, "the goldens were generated with another scipy: regenerate"
    x, w = g["x"], float(g["wpemax"])
    with np.errstate(all="ignore"):
        hi, lo, res = mm.MEITD(x.copy(), WPEMAX=w)
    assert np.shape(hi) == g["high"].shape and np.shape(lo) == g["low"].shape, name
    assert_bits_equal(hi, g["high"], name + " high")
    assert_bits_equal(lo, g["low"], name + " low")
    assert_bits_equal(res, g["residual"], name + " residual")
    assert [cpu_work[-1].calls[k] for k in ("extract", "count", "probe")] == g["port_calls"].tolist(), name
    if "xitd_order" in g:
        with np.errstate(all="ignore"):
            xi = mm.XITD(x.copy())
        rows = np.vstack((np.vstack((g["high"], g["low"])), g["residual"]))
        assert len(xi) == int(g["xitd_rows"]) == len(rows)
        assert_bits_equal(xi, rows[g["xitd_order"]], name + " XITD")


@pytest.mark.parametrize("name", NAMES)
def test_helpers_match_the_reference(name):
    """_determine / _retrieve over CpuWork against the reference's determine_if_first_is_proper_rotation / retrieve_proper_rotation on
    the case's signal (arrays are stored up to 1024 samples, the flags for all; retrieve returns its input where it finds nothing)"""
    g = load(name)
    x, w = g["x"], float(g["wpemax"])
    with np.errstate(all="ignore"):
        cw = meitd_oracle.CpuWork(len(x))
        src, rot, base = cw.take(), cw.take(), cw.take()
        cw.upload(x, src)
        assert mm._determine(cw, src, rot, base, w) == int(g["determine_proper"])
        det = cw.rows[rot].copy(), cw.rows[base].copy()
        cw = meitd_oracle.CpuWork(len(x))
        rot = cw.take()
        cw.upload(x, rot)
        out, proper = mm._retrieve(cw, rot, w)
        assert proper == int(g["retrieve_proper"])
        if not proper:
            assert_bits_equal(cw.rows[out], x, name + " retrieve returns its input")
    if "determine_rotation" in g:
        assert_bits_equal(det[0], g["determine_rotation"], name + " determine: rotation")
        assert_bits_equal(det[1], g["determine_baseline"], name + " determine: baseline")
        assert_bits_equal(cw.rows[out], g["retrieve_rotation"], name + " retrieve")
    else:
        assert len(x) > 1024


def test_the_earlier_goldens_stay_as_they_are():
    """tests/golden/spline/meitd_*.npz: not regenerated with the new directory"""
    want = {"meitd_am.npz": "cae9da2f4f615cfb4c71edfe8d1a445b96f2dbf691d17e116a1c154983a0ec45",
            "meitd_two_tone_noise.npz": "7adec71aa605dd56ac914715d86b1352111136559e16ad4676058405e8e3fbb2",
            "meitd_walk.npz": "fc8066929fc7d900e6a137bed15f5b3914de6c4fab4b937339b92e07b96ddedb"}
    for f, digest in want.items():
        with open(os.path.join(GOLDEN, "spline", f), "rb") as fh:
            assert hashlib.sha256(fh.read()).hexdigest() == digest, f
