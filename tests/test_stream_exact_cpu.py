"""The exact statement of the block-wise cubic stream (oracle/exact_stream.py), the layouts of tests/stream_cases.py and the
comparison tests/test_gpu_stream_exact.py runs the device stream through — everything that can be held without a GPU.

1. The exact statement against the fp64 oracle (stream_oracle.oracle_blockwise_cubic) and the reference-generated goldens: within
   the yardstick of tests/test_oracle_exact_spline.py on every layout, the "emitted unchanged" decisions identical.
2. The generators: the detected knots are the designed ones, and the conditions a layout is named after hold (knots exactly at
   lo / hi, 3 against 4 selected knots, clipping in front and behind, the list lengths at the sweeps' and the staging's limits).
3. The comparison raises on one planted defect at a time (applied to the fp64 oracle): that is what shows the GPU test can fail.
"""
import os

import numpy as np
import pytest

import stream_cases as sc
from helpers import GOLDEN
from oracle import cpu_oracle, exact_stream as es, iq_oracle, stream_oracle as so
from test_oracle_exact_spline import YARDSTICK_ULPS

STREAM = os.path.join(GOLDEN, "stream")


def test_the_bound_is_the_spline_tests():
    import test_gpu_spline_exact as t
    assert (sc.EPS, sc.C_REF, sc.C_ABS, sc.SENT) == (t.EPS, t.C_REF, t.C_ABS, t.SENT)


# ---- 1. the exact statement against the fp64 oracle and the goldens ---------------------------------------------------------
def _yardstick(what, blocks, x, L, ref):
    """err(ref) <= YARDSTICK_ULPS eps S on every spline block, unchanged blocks identical; returns the decisions."""
    dec = []
    for c, row in enumerate(blocks):
        for j, blk in enumerate(row):
            sl = slice(j * L, (j + 1) * L)
            same = np.array_equal(ref[c, sl], x[c, sl])
            dec.append(blk is None)
            assert same == (blk is None), "%s: channel %d block %d: the two statements decide differently" % (what, c, j)
            if blk is not None:
                u = float(np.max(blk.exact.err(ref[c]))) / (sc.EPS * es.scale(x[c], blk))
                assert np.isfinite(u) and u <= YARDSTICK_ULPS, (what, c, j, u)
    return dec


@pytest.mark.parametrize("name", sc.names())
def test_fp64_oracle_within_the_yardstick_and_same_decisions(name):
    c = sc.case(name)
    ref = sc.oracle(name)
    assert np.all(np.isfinite(ref))
    _yardstick(name, sc.exact(name), c["x"], c["L"], ref)
    sc.check("oracle/" + name, sc.exact(name), ref, c["x"], c["L"], ref, rot=c["x"] - ref)   # the comparison accepts the oracle


@pytest.mark.parametrize("name", sorted(f[:-4] for f in os.listdir(STREAM) if f.startswith("cubic_")))
def test_reference_generated_goldens_within_the_yardstick(name):
    g = np.load(os.path.join(STREAM, name + ".npz"))
    x = np.atleast_2d(g["x"])
    L = int(g["block"])
    blocks = es.exact_blockwise_cubic(x, L, int(g["margin"]), bool(g["shared_knots"]))
    dec = _yardstick(name, blocks, x, L, np.atleast_2d(g["baseline"]))
    assert not all(dec), "no spline in the golden"


def test_nan_windows_of_the_statement():
    """A block whose knot-giving window holds a NaN is emitted unchanged; under shared knots a NaN in another channel leaves
    that channel's blocks unspecified and channel 0's untouched."""
    rng = np.random.default_rng(5)
    L, nb = 64, 7
    for shared in (False, True):
        for ch in (0, 1):
            x = rng.standard_normal((2, nb * L))
            clean = es.exact_blockwise_cubic(x, L, 2, shared)
            x[ch, 2 * L + 17] = np.nan
            blocks = es.exact_blockwise_cubic(x, L, 2, shared)
            ref = so.oracle_blockwise_cubic(x, L, 2, shared)
            for c in range(2):
                for j in range(nb):
                    hit = j in (1, 2, 3) and (c == ch or (shared and ch == 0))
                    if hit and shared and ch == 1:
                        assert blocks[c][j] is es.UNSPECIFIED
                    elif hit:
                        assert blocks[c][j] is None
                        assert np.array_equal(ref[c, j * L:(j + 1) * L], x[c, j * L:(j + 1) * L], equal_nan=True)
                    else:
                        assert np.array_equal(blocks[c][j].exact.hi, clean[c][j].exact.hi)


# ---- 2. the generators --------------------------------------------------------------------------------------------------
def _designed_knots(name):
    """The designed stream knots of a zigzag case's channel 0 (None for noise)."""
    kind = name.split("_")[0]
    c = sc.case(name)
    nb = c["x"].shape[1] // c["L"]
    if kind == "seam":
        return sc.seam_knots(nb, c["L"], sc.SEAMS[name.split("_")[1]])
    if name.startswith(("geom_designed", "ring_designed")):
        return sc.seam_knots(nb, c["L"], sc.SEAMS["all"])
    if name.startswith("geom_alt"):
        i = np.arange(c["x"].shape[1])
        return i[(i % c["L"] != 0) & (i % c["L"] != c["L"] - 1)]
    return None


@pytest.mark.parametrize("name", sc.names())
def test_windows_detect_the_designed_knots(name):
    c = sc.case(name)
    x, L = c["x"], c["L"]
    nb = x.shape[1] // L
    if "noise" in name:
        assert np.all(np.diff(x[0]) != 0)
        return
    wins = so.windows(nb, L)
    for ch in range(x.shape[0]):
        # a zigzag's knots are its strict extrema: both detectors find them on the whole row ...
        e, m = cpu_oracle.extrema_cpp(x[ch])
        whole = e[:m]
        np.testing.assert_array_equal(whole, cpu_oracle.knots(x[ch]))
        if ch == 0 and _designed_knots(name) is not None:
            np.testing.assert_array_equal(whole, _designed_knots(name))
        # ... and a window finds those of them that lie strictly inside it
        for w0, wl, lo, hi in wins:
            e, m = cpu_oracle.extrema_cpp(np.ascontiguousarray(x[ch, w0:w0 + wl]))
            np.testing.assert_array_equal(e[:m], whole[(whole > w0) & (whole < w0 + wl - 1)] - w0)


@pytest.mark.parametrize("which", sorted(sc.SEAMS))
def test_seam_layouts_put_knots_exactly_at_lo_and_hi(which):
    hits = 0
    for c, j, W, lo, hi, knots, sel in sc.selections("seam_%s_m1" % which):
        for d in sc.SEAMS[which]:
            for edge in (lo, hi):
                if 1 <= edge + d <= len(W) - 2 and 0 < edge < len(W):
                    assert edge + d in knots, (which, j, edge + d)
                    hits += 1
        for d in set((-1, 0, 1)) - set(sc.SEAMS[which]):
            assert lo + d not in knots and hi + d not in knots
    assert hits == len(sc.SEAMS[which]) * 2 * (sc.SEAM_NB - 1)     # first block: hi; inner: lo and hi; last: lo
    # side = "left" decides: with a knot exactly at lo or hi the other side selects another list
    if 0 in sc.SEAMS[which]:
        differ = [not np.array_equal(sel, knots[max(np.searchsorted(knots, lo, "right") - 1, 0):
                                                min(np.searchsorted(knots, hi, "right") + 3, len(knots))])
                  for c, j, W, lo, hi, knots, sel in sc.selections("seam_%s_m1" % which)]
        assert all(differ)


def test_clipping_in_front_behind_and_margins_beyond_the_list():
    seen = {m: set() for m in sc.MARGINS}
    for margin in sc.MARGINS:
        for c, j, W, lo, hi, knots, sel in sc.selections("seam_all_m%d" % margin):
            a, b, m = np.searchsorted(knots, lo), np.searchsorted(knots, hi), len(knots)
            if 0 < a < margin:
                seen[margin].add("front")             # fewer than margin knots in front of the block
            if b + margin + 2 > m:
                seen[margin].add("back")
            if a >= margin and b + margin + 2 <= m:
                seen[margin].add("none")
                assert len(sel) == b - a + 2 * margin + 2 and sel[0] > 0
            if margin > m:
                seen[margin].add("whole")
                assert np.array_equal(sel, knots)
    assert seen[1] >= {"none", "back"} and seen[2] >= {"none", "back"}, seen
    assert seen[8] >= {"front", "back"} and seen[64] >= {"front", "back", "whole"}, seen


def test_counts_at_the_threshold():
    for margin in (1, 8):
        rows = sc.selections("counts_m%d" % margin)
        assert tuple(len(r[5]) for r in rows) == sc.COUNTS_PER_WINDOW
        assert [b is not None for b in sc.exact("counts_m%d" % margin)[0]] == [n >= 4 for n in sc.COUNTS_PER_WINDOW]
    assert [len(r[6]) for r in sc.selections("counts_m8")] == list(sc.COUNTS_PER_WINDOW)
    for name, want in (("behind2_m1", 3), ("behind3_m1", 4)):
        c, j, W, lo, hi, knots, sel = sc.selections(name)[1]
        assert not np.any((knots >= lo) & (knots < hi)), "no knot inside the emitted block"
        assert np.count_nonzero(knots < lo) == 2 and np.count_nonzero(knots >= hi) == want - 1
        assert len(sel) == want and sel[0] == knots[1]
        assert (sc.exact(name)[0][1] is None) == (want == 3)


def test_geometry_reaches_the_kernels_paths():
    """first > 1 (a sub-list of the compaction's list), lists above the sweep workgroup's 1792 elements, tiles above and below
    the evaluation's 320 staged knots, blocks on and off the 512-sample tile grid."""
    for L in (2048, 4096):
        for c, j, W, lo, hi, knots, sel in sc.selections("geom_alt_L%d" % L):
            assert len(knots) == (len(W) // L) * (L - 2)
            assert len(sel) - 2 > 1792 + 256, "a sweep seam and its warm-up inside the selected list"
            if j >= 2:
                assert np.searchsorted(knots, sel[0]) > 1792, "the sub-list starts behind the first workgroup's elements"
    for c, j, W, lo, hi, knots, sel in sc.selections("geom_alt_L1024"):
        per_tile = np.bincount((sel[(sel >= lo) & (sel < hi)] - lo) // 512)
        assert per_tile.min() > 320                                     # dense tiles
    per_tile = np.concatenate([np.bincount((sel[(sel >= lo) & (sel < hi)] - lo) // 512, minlength=L // 512)[:L // 512]
                               for L in (1024, 2048, 4096) for c, j, W, lo, hi, knots, sel in sc.selections("geom_noise_L%d" % L)])
    assert per_tile.min() < 318 - 8 and 318 + 8 < per_tile.max(), (per_tile.min(), per_tile.max())   # noise straddles the limit
    assert 0.2 < np.mean(per_tile <= 318) < 0.8
    for c, j, W, lo, hi, knots, sel in sc.selections("geom_sparse_L1000"):
        assert 5 <= np.count_nonzero((knots >= lo) & (knots < hi)) <= 10
    assert {L % 512 == 0 for L in sc.GEOM_L} == {True, False}
    firsts = [np.searchsorted(knots, sel[0]) for n in sc.names() for c, j, W, lo, hi, knots, sel in sc.selections(n) if len(sel)]
    assert min(firsts) == 0 and max(firsts) > 0


@pytest.mark.parametrize("name", ["chan3_shared_L100", "chan3_shared_L512"])
def test_shared_channels_have_other_extrema(name):
    x = sc.case(name)["x"]
    k0 = set(cpu_oracle.extrema_cpp(x[0])[0][:cpu_oracle.extrema_cpp(x[0])[1]].tolist())
    for ch in (1, 2):
        e, m = cpu_oracle.extrema_cpp(x[ch])
        assert len(k0 & set(e[:m].tolist())) < m // 4
    own = es.exact_blockwise_cubic(x, sc.case(name)["L"], sc.case(name)["margin"], False)
    sh = sc.exact(name)
    assert np.array_equal(own[0][1].exact.hi, sh[0][1].exact.hi) and not np.array_equal(own[1][1].exact.hi, sh[1][1].exact.hi)
    assert np.array_equal(sh[1][1].sel, sh[0][1].sel)


@pytest.mark.parametrize("n", sc.IQ_N)
@pytest.mark.parametrize("extra", [False, True])
def test_iq_layouts_share_exactly_the_designed_knots(n, extra):
    c = sc.iq_case(n, extra)
    e, idx = iq_oracle.extrema_iq(c["I"] + 1j * c["Q"])
    np.testing.assert_array_equal(e[:idx], c["knots"])
    eq, mq = cpu_oracle.extrema_cpp(c["Q"])
    assert (mq > idx) == extra                       # Q's further extrema are not common knots
    if n == sc.IQ_N[-1]:
        assert n > 64 * 512


# ---- 3. the comparison raises on planted defects --------------------------------------------------------------------------
def _oracle_with(monkeypatch, name, select=None, min_knots=None, x=None):
    c = sc.case(name)
    if select is not None:
        monkeypatch.setattr(so, "select_knots", select)
    if min_knots is not None:
        monkeypatch.setattr(so, "MIN_KNOTS", min_knots)
    got = so.oracle_blockwise_cubic(c["x"] if x is None else x, c["L"], c["margin"], c["shared"])
    monkeypatch.undo()
    return got


def _raises(name, got):
    c = sc.case(name)
    with pytest.raises(AssertionError):
        sc.check("defect/" + name, sc.exact(name), got, c["x"], c["L"], sc.oracle(name))


def _select(side="left", behind=2, shift=0):
    def f(knots, lo, hi, margin):
        m = len(knots)
        a = int(np.searchsorted(knots, lo, side=side))
        b = int(np.searchsorted(knots, hi, side=side))
        first, last = max(a - margin, 0), min(b + margin + behind, m)
        return knots[min(first + shift, m): min(last + shift, m)]
    return f


def test_defect_side_right(monkeypatch):
    for name in ("seam_0_m1", "seam_all_m2", "geom_designed_L512"):
        _raises(name, _oracle_with(monkeypatch, name, select=_select(side="right")))


def test_defect_one_knot_less_behind(monkeypatch):
    for name in ("seam_m1_m1", "geom_sparse_L100", "behind3_m1"):
        _raises(name, _oracle_with(monkeypatch, name, select=_select(behind=1)))


def test_defect_threshold_of_three(monkeypatch):
    for name in ("behind2_m1", "counts_m8"):
        _raises(name, _oracle_with(monkeypatch, name, min_knots=3))


def test_defect_list_offset_by_one(monkeypatch):
    for name in ("seam_p1_m2", "geom_alt_L2048", "geom_noise_L513"):
        _raises(name, _oracle_with(monkeypatch, name, select=_select(shift=1)))


def test_defect_small_bump_at_a_sweep_seam():
    name = "geom_alt_L2048"
    c = sc.case(name)
    blk = sc.exact(name)[0][2]
    assert len(blk.sel) > 1793
    p = blk.w0 + int(blk.sel[1792]) + 1             # the sample behind entry 1792 of the selected list, as a stream sample
    assert 2 * c["L"] <= p < 3 * c["L"]
    got = np.array(sc.oracle(name))
    got[0, p] += 1e-11 * es.scale(c["x"][0], blk)
    _raises(name, got)
    got = np.array(sc.oracle(name))                  # (and an error the bound allows does not raise)
    got[0, p] += 8 * sc.EPS * es.scale(c["x"][0], blk)
    sc.check("allowed/" + name, sc.exact(name), got, c["x"], c["L"], sc.oracle(name))


def test_defect_block_from_the_wrong_ring_slot(monkeypatch):
    for name in ("ring_noise_nb7", "ring_designed_nb4"):
        c = sc.case(name)
        L = c["L"]
        x = np.array(c["x"])
        x[:, 3 * L:4 * L] = x[:, 0:L]                # block 3 never reached slot 0: block 0 is still there
        _raises(name, _oracle_with(monkeypatch, name, x=x))


def test_defect_unchanged_block_gets_a_spline_and_back():
    name = "counts_m8"
    c = sc.case(name)
    L = c["L"]
    got = np.array(sc.oracle(name))
    got[0, 5 * L:6 * L] = c["x"][0, 5 * L:6 * L]     # the one spline block emitted unchanged
    _raises(name, got)
    got = np.array(sc.oracle(name))
    got[0, 2 * L + 3] = np.nextafter(got[0, 2 * L + 3], 9.0)     # one ulp in an unchanged block
    _raises(name, got)
    with pytest.raises(AssertionError):
        sc.check("rot", sc.exact(name), sc.oracle(name), c["x"], L, sc.oracle(name), rot=c["x"] - sc.oracle(name) + 1e-300)
