"""The CPU model's deliver-or-refuse decisions (oracle/knotfirst_model.py: decide()) for every case of tests/kf_cases.py, held to the
pinned C oracle: what the model delivers equals the oracle's baselines and per-level knot lists bit for bit; what it refuses it refuses
for exactly one reason, at a level where that reason can be checked against the oracle.  And the table itself is held to what it has to
show: enough delivered cases per range size, enough refusals per fail bit, both sides of every capacity limit, knots where the seam
layouts promise them.  tests/test_gpu_kf_decisions.py then holds the GPU's decisions to these."""
import os
import re

import numpy as np
import pytest

from helpers import ROOT, canon_u64, kf_rates_tally
from kf_cases import CASES
from oracle import cpu_oracle, knotfirst_model as kf

_BY_NAME = {c.name: c for c in CASES}
_DECIDED = {}


def _decided(case):
    """(signal, decision, the oracle's levels: knot lists and every level's input) of a case, computed once and shared."""
    if case.name not in _DECIDED:
        x = case.make()
        ref = cpu_oracle.itd_lean(x, case.m, want_knots=True)
        lv = [np.asarray(x, dtype=np.float64)]
        for _ in range(len(ref["knots"])):
            lv.append(cpu_oracle.itd_baseline_extract(lv[-1])[1])
        _DECIDED[case.name] = (x, kf.decide(x, case.m, case.L0, case.tiles), ref, lv)
    return _DECIDED[case.name]


def test_the_model_s_constants_are_the_kernel_s():
    src = open(os.path.join(ROOT, "pyitd_amd", "csrc", "itd_knotfirst.hpp")).read()

    def const(name):
        return int(re.search(r"constexpr int (?:[A-Za-z0-9_ =,]*, *)?%s = (\d+)[,;]" % name, src).group(1))

    assert (const("kKfCap"), const("kKcTiles"), const("kKcCap"), const("kKcCapH"), const("kKcSlab")) == (
        kf.K_KF_CAP, kf.K_KC_TILES, kf.K_KC_CAP, kf.K_KC_CAP_H, kf.K_KC_SLAB)
    assert (const("kKfFailVerify"), const("kKfFailCapacity"), const("kKfFailNonFinite"), const("kKfFailTies"), const("kKfFailWait")) == (
        kf.FAIL_VERIFY, kf.FAIL_CAPACITY, kf.FAIL_NONFINITE, kf.FAIL_TIES, kf.FAIL_WAIT) == (1, 2, 4, 8, 16)
    assert kf.TILE == 512 and re.search(r"static_assert\(TW == 512 ", src)
    k = open(os.path.join(ROOT, "pyitd_amd", "csrc", "itd_kernels.hpp")).read()
    assert int(re.search(r"constexpr int kReach = (\d+);", k).group(1)) * 510 + 128 == kf.L0_REACH
    assert float.fromhex(re.search(r"constexpr double kNearTie = (0x1p-\d+);", k).group(1)) == kf.NEAR


def test_names_are_unique_and_inputs_finite():
    assert len(_BY_NAME) == len(CASES)
    for c in CASES:
        assert np.all(np.isfinite(c.make())), c.name


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_the_model_s_decision_is_held_to_the_oracle(name):
    case = _BY_NAME[name]
    x, d, ref, lv = _decided(case)
    L0, ks = case.L0, ref["knots"]
    if d["outcome"] == "delivered" and not d["fused"]:
        # stopped before the first fused level: nothing runs fused
        assert ref["stop"] == "natural" and len(ks) <= L0 and len(cpu_oracle.knots(lv[len(ks)])) < 2, name
        return
    if d["outcome"] == "delivered":
        # the contract of test_oracle_knotfirst.py: knot lists and baselines of every fused level, bit for bit
        assert d["bits"] == 0 and d["fail_lev"] == 99 and d["lend"] == len(ks) - 1, name
        assert (ref["stop"] == "natural") == bool(d["natural"]), name
        for q, L in enumerate(d["levels"]):
            np.testing.assert_array_equal(L["pos"], ks[L0 + q], err_msg="%s: knots of level %d" % (name, L0 + q))
            assert np.array_equal(canon_u64(d["bases"][q]), canon_u64(lv[L0 + q + 1])), "%s: baseline of level %d" % (name, L0 + q)
            assert d["mlev"][L0 + q] == len(ks[L0 + q]), name
        assert (len(d["last"]) < 2) == (d["mlev"][d["lend"] + 1] < 2), name
        return
    # refused: exactly one reason, at a stated level, and an honest one
    assert d["bits"] in (kf.FAIL_VERIFY, kf.FAIL_CAPACITY, kf.FAIL_NONFINITE), "%s: more than one reason: %s" % (name, d["what"])
    assert d["level"] is not None and L0 <= d["level"] <= case.m + 2, name
    if d["bits"] == kf.FAIL_VERIFY:
        # every level in front of the failing one is the oracle's, and at the failing one the knot side's list is NOT the oracle's:
        # the shortcut missed (or invented) a knot there
        q = d["level"] - L0
        assert q >= 1 and d["fail_lev"] in (d["level"], 99), name
        for j in range(q):
            np.testing.assert_array_equal(d["levels"][j]["pos"], ks[L0 + j], err_msg="%s: knots of level %d" % (name, L0 + j))
            assert np.array_equal(canon_u64(d["bases"][j]), canon_u64(lv[L0 + j + 1])), "%s: baseline of level %d" % (name, L0 + j)
        mine = d["levels"][q]["pos"] if q < len(d["levels"]) else d["last"]
        theirs = ks[L0 + q] if L0 + q < len(ks) else cpu_oracle.knots(lv[L0 + q])
        assert not np.array_equal(mine, theirs), name
    elif d["bits"] == kf.FAIL_CAPACITY:
        loads = d["loads"]
        over = [loads["kKcCapH"] > kf.K_KC_CAP_H, max(loads["kKcCap"]) > kf.K_KC_CAP, max(loads["kKcSlab"]) > kf.K_KC_SLAB,
                bool(loads["kKfCap"]) and max(loads["kKfCap"]) > kf.K_KF_CAP]
        assert any(over) and d["fail_lev"] == 99, name
    else:
        assert d["fail_lev"] == 99 or d["fail_lev"] == d["level"], name
        assert "NaN" in d["what"][0] or "reach" in d["what"][0] or "non-finite" in d["what"][0], name


def test_the_table_shows_something(capsys):
    tally, edges, levels = {}, {}, {}
    for c in CASES:
        _, d, _, _ = _decided(c)
        key = (c.tiles, "delivered" if d["outcome"] == "delivered" else "refused 0x%x" % d["bits"], "fused" if d["fused"] else "not fused")
        tally[key] = tally.get(key, 0) + 1
        if c.edge and c.group == "edge":
            limit, load = c.edge
            got = d["loads"][limit]
            edges[(limit, load)] = (got if isinstance(got, int) else max(got), d["outcome"], d["bits"])
            levels[(limit, load)] = d["level"]
    with capsys.disabled():
        print("\n%d cases: tiles per workgroup, outcome, count" % len(CASES))
        for key in sorted(tally):
            print("  %2d  %-14s %-9s %3d" % (key + (tally[key],)))
        for key in sorted(edges):
            print("  edge %-8s stated %4d: load %4d, %s (bits %d)" % (key + edges[key]))
    for tiles in (16, 32, 64):
        assert tally.get((tiles, "delivered", "fused"), 0) >= 10, "delivered cases with %d-tile ranges" % tiles
    for bit in (1, 2, 4):
        assert sum(v for k, v in tally.items() if k[1] == "refused 0x%x" % bit) >= 3, "cases refused with bit %d" % bit
    # both sides of every capacity limit: exactly at it — delivered —, one above — refused for the capacity and nothing else
    for limit, cap in (("kKcCapH", kf.K_KC_CAP_H), ("kKcCap", kf.K_KC_CAP), ("kKcSlab", kf.K_KC_SLAB), ("kKfCap", kf.K_KF_CAP)):
        assert edges[(limit, cap)] == (cap, "delivered", 0), limit
        assert edges[(limit, cap + 1)] == (cap + 1, "refused", kf.FAIL_CAPACITY), limit
    # ... reached where the layouts put it: at the hand-over (level 2), behind its step, at the last level's table (12), in the sample pass
    assert [levels[(limit, cap + 1)] for limit, cap in (("kKcCapH", kf.K_KC_CAP_H), ("kKcCap", kf.K_KC_CAP), ("kKcSlab", kf.K_KC_SLAB), ("kKfCap", kf.K_KF_CAP))] == [2, 2, 12, 2]


def test_the_seam_layouts_put_the_knots_where_they_say():
    seen = set()
    for c in CASES:
        if c.group != "seam":
            continue
        _, d, _, _ = _decided(c)
        assert d["outcome"] == "delivered" and d["fused"], c.name
        span = c.tiles * kf.TILE
        pos = d["levels"][0]["pos"]          # the knots of the first fused level
        per = np.bincount(pos // span, minlength=4)
        if c.edge == "last sample of range 0":
            assert span - 1 in pos and span not in pos, c.name
        elif c.edge == "first sample of range 1":
            assert span in pos and span - 1 not in pos, c.name
        elif c.edge == "both seam samples":
            assert span - 1 in pos and span in pos, c.name
        elif c.edge == "empty":
            assert per[1] == 0 and per[0] >= 50 and per[2] >= 50, c.name
            assert all(np.all((L["pos"] < span) | (L["pos"] >= 2 * span)) for L in d["levels"]), c.name
        else:
            last = len(per) - 1
            assert c.edge == "last" and per[last] >= 2 and np.all(per[:last] == 0), c.name
            assert 0 < len(c.make()) - last * span < span, c.name      # ... and that range is ragged
        seen.add(c.edge)
    assert seen == {"last sample of range 0", "first sample of range 1", "both seam samples", "empty", "last"}


def test_kf_rates_counts_every_wrong_result():
    """tools/kf_rates.py reports "WRONG (32 tiles)" for a wrong result with halved ranges: counted like a plain "WRONG"."""
    tallies, wrong = kf_rates_tally([(3, 7, "delivered"), (3, 7, "WRONG (32 tiles)"), (3, 7, "refused 0x4"), (0, 11, "WRONG"), (0, 11, "delivered (16 tiles)")])
    assert wrong == 2
    assert tallies == {(3, 7): {"delivered": 1, "WRONG (32 tiles)": 1, "refused 0x4": 1}, (0, 11): {"WRONG": 1, "delivered (16 tiles)": 1}}
    assert kf_rates_tally([(1, 3, "delivered")]) == ({(1, 3): {"delivered": 1}}, 0)
