"""The fused sparse levels' deliver-or-refuse DECISIONS on the GPU (pyitd_amd/csrc/itd_knotfirst.hpp: k_kf_knots, k_kf_apply) held to
the CPU model's (oracle/knotfirst_model.py: decide()) for every case of tests/kf_cases.py: delivered exactly where the model delivers
— and then bit for bit the pinned oracle's result —, refused with the model's fail bit where it refuses.  tests/test_gpu_fused.py
holds "never wrong"; this file holds "never refused without the stated reason", which the automatic mode hides (a refused call is
repeated level by level: exact rows, only slower).

Every engine is fresh and every knob that decides the form is set explicitly, so the suite's other modes (PYITD_FUSE_RANGE,
PYITD_FUSE_CAP, PYITD_FUSE_LEVEL, PYITD_LEVEL0_MODE, ...) do not change what is tested."""
import re

import numpy as np
import pytest

from helpers import assert_bits_equal, chirp
from kf_cases import CASES, LENGTHS, edge_signal

pytestmark = pytest.mark.gpu

_BY_NAME = {c.name: c for c in CASES}
_REF = {}


def _ref(case):
    """(signal, the model's decision, the oracle's result) of a table case: computed once, shared, never changed."""
    if case.name not in _REF:
        from oracle import cpu_oracle, knotfirst_model
        x = case.make()
        _REF[case.name] = (x, knotfirst_model.decide(x, case.m, case.L0, case.tiles), cpu_oracle.itd_lean(x, case.m))
    return _REF[case.name]


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _engine(P, n, batch, mode, L0, tiles, cap, min_samples=1024):
    from pyitd_amd.engine import LEVEL0_AUTO
    eng = P.Engine(n, batch, 0)
    eng.set_level0_mode(LEVEL0_AUTO)         # (record-driven level 0 keeps every call level by level)
    eng.set_fuse_mode(mode)
    eng.set_fuse_level(L0)
    eng.set_fuse_range(tiles)
    eng.set_fuse_cap(cap)
    eng.set_fuse_min_samples(min_samples)
    return eng


def _call(eng, torch, xd, dtype, n, batch, m, rows):
    """One decomposition and its summary: ("delivered", summary) or ("refused", fail bits)."""
    from pyitd_amd import ITDError
    rows.fill_(float("nan"))
    torch.cuda.synchronize()                 # (the fill runs on torch's stream, the engine on its own)
    try:
        eng.decompose_dev(xd.data_ptr(), dtype, n, batch, n, m, rows.data_ptr(), None, None)
        return "delivered", eng.summary(batch)
    except ITDError as err:
        got = re.search(r"fused sparse levels.*fail bits (0x[0-9a-f]+)", str(err))
        assert got, "an error that is not the fused levels' refusal: %s" % err
        return "refused", int(got.group(1), 16)


def _assert_oracle(s, rows, b, ref, what):
    nr = int(s["n_rows"][b])
    assert nr == ref["rows"].shape[0], what + ": rows"
    assert ("natural", "timeout")[int(s["stop"][b])] == ref["stop"], what + ": stop reason"
    assert_bits_equal(rows[:nr].cpu().numpy(), ref["rows"], what)
    kc = [int(v) for v in s["knot_counts"][b] if v >= 0]
    assert kc[: len(ref["knot_counts"])] == ref["knot_counts"].tolist(), what + ": knots per level"


def _assert_decision(outcome, got, eng, rows, model, ref, what):
    assert outcome == model["outcome"], "%s: the GPU %s, the model %s (%s)" % (
        what, outcome if outcome == "delivered" else "refused with fail bits 0x%x" % got, model["outcome"], "; ".join(model["what"]) or "no reason to refuse")
    if outcome == "delivered":
        assert eng.fuse_repeats == 0, what
        _assert_oracle(got, rows, 0, ref, what)
    else:
        # bit 16: a halo wait met a neighbour that had given up — only ever beside the capacity that made it give up (0x12)
        assert (got & 15) == model["bits"] and (not (got & 16) or (got & 2)), "%s: refused with fail bits 0x%x, the model's 0x%x (%s)" % (
            what, got, model["bits"], "; ".join(model["what"]))


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_decision_parity(P, torch, name):
    """ITD_FUSE_ONLY: delivered <=> the model delivers; delivered rows, their number, the stop reason and the knots per level are the
    oracle's and nothing was repeated; refused => the model's fail bit."""
    from pyitd_amd.engine import FUSE_ONLY
    case = _BY_NAME[name]
    x, model, ref = _ref(case)
    n = len(x)
    eng = _engine(P, n, 1, FUSE_ONLY, case.L0, case.tiles, -1)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    rows = torch.empty((case.m + 2, n), dtype=torch.float64, device="cuda")
    try:
        outcome, got = _call(eng, torch, xd, x.dtype, n, 1, case.m, rows)
        if outcome == "delivered":
            assert eng.last_fuse_level == case.L0 and eng.last_fuse_cap == 0, name
        _assert_decision(outcome, got, eng, rows, model, ref, name)
    finally:
        eng.close()


def _learns_a_cap(case):
    """The verification and non-finite cases whose failing level the engine can cap the next calls at (itd_policy.hpp: two fused
    levels at least, within the call's), at a length the automatic mode fuses (FormPolicy::kFusedMinN)."""
    from oracle import knotfirst_model
    x, d, _ = _ref(case)
    if len(x) < 65536:
        return False
    return d["bits"] in (knotfirst_model.FAIL_VERIFY, knotfirst_model.FAIL_NONFINITE) and case.L0 + 2 <= d["fail_lev"] <= case.m + 1


def test_fail_level_parity(P, torch):
    """ITD_FUSE_AUTO with the automatic cap: the refused call is repeated level by level (exact rows), the next one runs fused up to
    the model's failing level and is delivered without a repeat — KfSig::fail_lev is the level the model names."""
    from pyitd_amd.engine import FUSE_AUTO
    cases = [c for c in CASES if _learns_a_cap(c)]
    assert len(cases) >= 3
    for case in cases:
        x, model, ref = _ref(case)
        n = len(x)
        eng = _engine(P, n, 1, FUSE_AUTO, case.L0, case.tiles, 0)
        xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        rows = torch.empty((case.m + 2, n), dtype=torch.float64, device="cuda")
        try:
            outcome, s = _call(eng, torch, xd, x.dtype, n, 1, case.m, rows)
            assert outcome == "delivered" and eng.fuse_repeats == 1, case.name
            _assert_oracle(s, rows, 0, ref, case.name + " (call 1, repeated)")
            outcome, s = _call(eng, torch, xd, x.dtype, n, 1, case.m, rows)
            assert outcome == "delivered", case.name
            assert (eng.last_fuse_level, eng.last_fuse_cap, eng.fuse_repeats) == (case.L0, model["fail_lev"], 1), case.name
            _assert_oracle(s, rows, 0, ref, case.name + " (call 2, capped at the model's level)")
        finally:
            eng.close()


@pytest.mark.parametrize("odd", [(5, 15), (0, 1)])
def test_per_signal_decisions_in_a_batch(P, torch, odd):
    """16 signals in one chunk, two of them refused by the model (one for a capacity — the slab one entry above its limit —, one by
    verification): exactly those two are run again on their own, the call is not repeated, every row is the oracle's.  (66 313
    samples each: the automatic mode, whose refusals are repaired, fuses no shorter signal.)"""
    from oracle import cpu_oracle, knotfirst_model
    from pyitd_amd.engine import FUSE_AUTO
    n, m, L0, tiles, B = LENGTHS[64], 11, 2, 64, 16
    slab = [c for c in CASES if c.edge == ("kKcSlab", knotfirst_model.K_KC_SLAB + 1)][0]
    xs = np.stack([edge_signal(n, 100 + b, []) for b in range(B)])
    xs[odd[0]] = slab.make()
    xs[odd[1]] = chirp(n).astype(np.float64)
    decisions = [knotfirst_model.decide(xs[b], m, L0, tiles) for b in range(B)]
    assert [b for b in range(B) if decisions[b]["outcome"] == "refused"] == sorted(odd), "the model refuses exactly the two odd members"
    assert all(d["fused"] for d in decisions) and {decisions[b]["bits"] for b in odd} == {1, 2}
    eng = _engine(P, n, B, FUSE_AUTO, L0, tiles, -1)
    eng.set_batch_chunk(B)
    xd = torch.from_numpy(xs).cuda()
    rows = torch.empty((B, m + 2, n), dtype=torch.float64, device="cuda")
    try:
        outcome, s = _call(eng, torch, xd, np.float64, n, B, m, rows)
        assert outcome == "delivered"
        assert (eng.fuse_signal_repairs, eng.fuse_repeats) == (2, 0)
        for b in range(B):
            _assert_oracle(s, rows[b], b, cpu_oracle.itd_lean(xs[b], m), "signal %d" % b)
    finally:
        eng.close()


@pytest.mark.parametrize("name", [c.name for c in CASES if c.group == "edge"])
def test_same_answer_twice(P, torch, name):
    """A capacity-edge case gives the same decision on two consecutive calls of one engine: the knot side's accumulators and tickets
    clean themselves between calls, also behind a workgroup that gave up."""
    from pyitd_amd.engine import FUSE_ONLY
    case = _BY_NAME[name]
    x, model, ref = _ref(case)
    n = len(x)
    eng = _engine(P, n, 1, FUSE_ONLY, case.L0, case.tiles, -1)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    rows = torch.empty((case.m + 2, n), dtype=torch.float64, device="cuda")
    try:
        for call in range(2):
            outcome, got = _call(eng, torch, xd, x.dtype, n, 1, case.m, rows)
            _assert_decision(outcome, got, eng, rows, model, ref, "%s, call %d" % (name, call + 1))
    finally:
        eng.close()
