"""The order tests' registry (tests/sequence_cases.py) without a GPU: every work-enqueuing entry of the C ABI belongs to a cell, every
cell's check accepts its own reference at both sizes, every input is inside its operator's working branch, and the schedules the GPU
tests run hold every ordered pair, every size transition and every refusal in front of every family."""
import os
import re

import numpy as np
import pytest

import sequence_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine_entries():
    """The entries of include/pyitd_hip.h that take an itd_engine (parsed as tests/test_abi_cpu.py parses the header)."""
    src = open(os.path.join(ROOT, "include", "pyitd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = []
    for name, args in re.findall(r"\b(itd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        if re.search(r"\bitd_engine\b", args):
            out.append(name)
    return sorted(set(out))


# Entries that take an engine and enqueue no operator's work: creators, destroyers, setters, getters, timing and the itd_debug_kf_* hooks.
# Nothing else may stand here: an operator belongs to a cell.
EXEMPT = {
    "itd_engine_create": "creator",
    "itd_engine_destroy": "destroyer",
    "itd_engine_workspace_bytes": "getter",
    "itd_engine_device": "getter",
    "itd_last_error": "getter",
    "itd_set_valid_flags": "setter",
    "itd_set_device_repair": "setter",
    "itd_get_device_repairs": "getter",
    "itd_set_nan_input_mode": "setter",
    "itd_set_level0_mode": "setter",
    "itd_set_fuse_mode": "setter",
    "itd_set_fuse_level": "setter",
    "itd_set_fuse_range": "setter",
    "itd_set_fuse_min_samples": "setter (the walks poke it)",
    "itd_set_fuse_cap": "setter",
    "itd_get_last_fuse_cap": "getter",
    "itd_debug_kf_fault": "itd_debug_kf_* hook",
    "itd_debug_kf_fault_signal": "itd_debug_kf_* hook",
    "itd_get_fuse_repeats": "getter",
    "itd_get_last_fuse_level": "getter",
    "itd_get_fuse_signal_repairs": "getter",
    "itd_set_resident_mode": "setter",
    "itd_get_resident_repeats": "getter",
    "itd_set_resident_window": "setter",
    "itd_set_batch_chunk": "setter",
    "itd_set_batch_streams": "setter",
    "itd_set_kernel_timing": "timing",
    "itd_set_kernel_timing_stride": "timing",
    "itd_get_kernel_timing": "timing",
    "itd_get_kernel_timing_samples": "timing",
    "itd_set_kernel_timing_mode": "timing",
    "itd_get_step_periods": "timing",
}
# setters and getters by name that are work all the same and must be claimed: the summary repeats a refused form, the baselines' getter
# copies what an earlier call left in d_io_bases, and the two settings below are part of a cell's own calls
WORK_ALL_THE_SAME = ("itd_get_summary", "itd_get_last_baselines_host", "itd_set_host_keep_baselines", "itd_set_spline_solver")
ALLOWED_EXEMPT = re.compile(r"^itd_(engine_(create|destroy|workspace_bytes|device)|last_error|set_[a-z0-9_]+|get_[a-z0-9_]+|debug_kf_[a-z_]+)$")


def test_every_work_enqueuing_entry_belongs_to_a_cell():
    entries = _engine_entries()
    assert len(entries) > 90, len(entries)
    claimed = {e for c in sc.CELLS.values() for e in c.entries}
    assert claimed <= set(entries), "cells name entries the header does not declare (with an engine): %s" % sorted(claimed - set(entries))
    assert set(EXEMPT) <= set(entries), "the exempt table names entries the header does not declare: %s" % sorted(set(EXEMPT) - set(entries))
    for name in EXEMPT:
        assert ALLOWED_EXEMPT.match(name) and name not in WORK_ALL_THE_SAME, "%s may not be exempt" % name
    assert not claimed & set(EXEMPT), sorted(claimed & set(EXEMPT))
    unclaimed = [e for e in entries if e not in claimed and e not in EXEMPT]
    assert not unclaimed, "entries that take an engine and belong to no cell of tests/sequence_cases.py: %s" % unclaimed
    for name in WORK_ALL_THE_SAME:
        assert name in claimed, name


def test_every_cell_is_described():
    for name, c in sc.CELLS.items():
        assert c.entries and c.decided_by and isinstance(c.buffers, tuple), name
    assert not sc.BY_RULE, "a cell compared by its rule alone needs its reason here and in DESIGN.md"


@pytest.mark.parametrize("size", ("S", "L"))
@pytest.mark.parametrize("name", sc.NAMES)
def test_check_accepts_the_reference_and_the_input_reaches_the_working_branch(name, size):
    """The cell's check accepts the reference's own result (for a CPU model of the GPU result: the model's output), so the inputs
    stay inside the rule without any GPU; the input is finite and inside the operator's working branch, by the oracles."""
    cell = sc.CELLS[name]
    inp = cell.inputs(size)
    for k, v in inp.items():
        if isinstance(v, np.ndarray) and v.dtype.kind in "fc":
            assert np.isfinite(v).all(), (name, size, k)
    with np.errstate(all="ignore"):
        assert cell.reaches_working_branch(inp), "%s %s: the input misses the operator's working branch" % (name, size)
        ref = cell.reference(inp)
        assert isinstance(ref, tuple) and all(isinstance(a, np.ndarray) for a in ref), (name, size)
        cell.check(inp, ref)


def test_check_refuses_a_wrong_result():
    """One flipped last bit, one moved index: the comparison with a fresh engine and the checks notice."""
    for name in ("decompose_host", "extract_batch", "waves", "wave_hist"):
        cell = sc.CELLS[name]
        inp = cell.inputs("S")
        ref = [a.copy() for a in cell.reference(inp)]
        k = next(i for i, a in enumerate(ref) if a.size)
        a = ref[k].reshape(-1)
        if a.dtype.kind == "f":
            a[a.size // 3] = np.nextafter(a[a.size // 3], np.inf)
        else:
            a[a.size // 3] += 1
        with pytest.raises(AssertionError):
            cell.check(inp, tuple(ref))
        with pytest.raises(AssertionError):
            sc.same_results(tuple(ref), cell.reference(inp), name)


def test_sizes_differ_in_every_carve():
    for a, b in (("S", "L"), ("S", "G"), ("L", "G")):
        for k in ("n", "n_hw", "rows"):
            assert sc.SIZES[a][k] != sc.SIZES[b][k]
    assert sc.SIZES["S"]["n"] == 2 * 512 + 6 and sc.SIZES["L"]["n_hw"] == 2 * 512 + 514 and sc.SIZES["L"]["n"] == 5 * 512 + 77


def test_the_schedules_hold_every_pair_transition_and_refusal():
    names = set(sc.NAMES)
    pairs = sc.pair_schedule()
    assert {(a, b) for a, _, b, _ in pairs} == {(a, b) for a in names for b in names}
    assert {(sa, sb, b) for _, sa, b, sb in pairs} == {(s, t, b) for s, t in (("L", "S"), ("S", "L")) for b in names}
    walks = sc.walk_schedule(0)
    assert walks == sc.walk_schedule(0) and walks != sc.walk_schedule(1), "the walks are a function of the seed"
    assert len(walks) == sc.WALKS == 8 and all(len(w) == sc.WALK_CALLS == 60 for w in walks)
    steps = [s for w in walks for s in w]
    assert {s["cell"] for s in steps} == names
    assert any(s["size"] == "G" for s in steps) and sum(s["size"] == "G" for s in steps) < len(steps) // 8
    assert {s["refusal"] for s in steps} >= set(sc.REFUSALS)
    assert {s["solver"] for s in steps} >= set(sc.SOLVER_POKES) and {s["fuse_min"] for s in steps} >= set(sc.FUSE_MIN_POKES)
    seen = set()
    for w in walks:
        seen |= sc.size_transitions(w)
    for t in (("S", "S"), ("L", "L"), ("S", "L"), ("L", "S")):
        missing = sorted(c for c in names if t + (c,) not in seen)
        assert not missing, "no walk has %s -> %s in front of %s" % (t[0], t[1], missing)
    assert set(sc.refusal_schedule()) == {(r, c) for r in sc.REFUSALS for c in names}
    assert len(sc.REFUSALS) >= 4
