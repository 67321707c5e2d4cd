"""The engine's choice of form and what it learns when a form falls short (pyitd_amd/csrc/itd_policy.hpp), built for the host with
g++ and driven call by call the way itd_engine.hip drives it: decisions while a call is enqueued, the summary's outcome afterwards.
Restates what tests/test_gpu_fused.py and tests/test_gpu_resident.py assert on a GPU, plus the transitions nothing else pins.
A check of the policy, not a fallback: pyitd_amd never loads this build."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# include/pyitd_hip.h
RESIDENT_AUTO, RESIDENT_OFF, RESIDENT_ONLY = 0, 1, 2
LEVEL0_AUTO, LEVEL0_RECORDS, LEVEL0_FUSED = 0, 1, 2
FUSE_AUTO, FUSE_OFF, FUSE_ONLY = 0, 1, 2
# KfSig::fail bits (itd_knotfirst.hpp)
VERIFY, CAPACITY, WAIT = 1, 2, 16
# what the summary does after a refusal
FAIL, REPAIR_SIGNALS, REPEAT_CALL = 0, 1, 2
SPLINE_AUTO, SPLINE_SERIAL, SPLINE_PARALLEL = 0, 1, 2
# the form of a spline extraction (tests/c_client/policy_host.cpp: policy_spline_form)
SERIAL, PARALLEL, SMALL = 0, 1, 2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("policy") / "libpolicy_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                    os.path.join(ROOT, "tests", "c_client", "policy_host.cpp")], check=True, capture_output=True)
    L = ctypes.CDLL(so)
    P, I, I64, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_char_p
    sigs = {
        "policy_new": (P, []), "policy_free": (None, [P]),
        "policy_set": (I, [P, S, I64]), "policy_get": (I64, [P, S, ctypes.POINTER(I)]),
        "policy_resident": (I, [P, I, I]), "policy_level0_fused": (I, [P]), "policy_fused_levels": (I, [P, I64, I64, I, I]),
        "policy_first_level": (I, [P, I64, I]), "policy_tiles_per_wg": (I, [P]), "policy_cap": (I, [P, I, I]),
        "policy_tickets": (I, [P, I64, I64]),
        "policy_workspace_unavailable": (I, [P]), "policy_resident_failed": (I, [P]), "policy_level0_fell_short": (I, [P]),
        "policy_fused_levels_delivered": (None, [P, I, I]), "policy_fused_levels_refused": (I, [P, I, I, I, I, I, I, I]),
        "policy_device_repaired": (None, [P, I, I, I, I]),
        "policy_spline_form": (I, [I, I64, I]), "policy_meitd_one_launch": (I, [I, I64]),
    }
    for name, (res, args) in sigs.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


class Policy:
    def __init__(self, L):
        self.L, self.p = L, L.policy_new()

    def __getattr__(self, name):
        ok = ctypes.c_int(0)
        v = self.L.policy_get(self.p, name.encode(), ctypes.byref(ok))
        if not ok.value:
            raise AttributeError(name)
        return v

    def set(self, name, value):
        assert self.L.policy_set(self.p, name.encode(), value) == 0, name

    def call(self, n=1 << 17, batch=1, m=6):
        """What enqueue_any asks for one (non-resident) call of `batch` signals in one launch sequence: (fused level 0, fused
        sparse levels, first fused level, cap) as enqueue_decompose would enqueue them.  The gating line below restates
        enqueue_decompose's own (pyitd_amd/csrc/itd_engine.hip: `kf = kf && fuse0 && p.L0 >= 2 && p.L0 <= M ...`): keep them in step."""
        L, seq = self.L, n * batch
        f0 = bool(L.policy_level0_fused(self.p))
        kf = bool(L.policy_fused_levels(self.p, n, seq, m, f0))
        l0 = L.policy_first_level(self.p, seq, m)
        kf = kf and f0 and 2 <= l0 <= m
        return f0, kf, l0, (L.policy_cap(self.p, l0, m) if kf else 0)

    def refused(self, bits, fail_lev=99, l0=3, cap=0, m=6, nfail=1, batch=1):
        return self.L.policy_fused_levels_refused(self.p, bits, fail_lev, l0, cap, m, nfail, batch)

    def delivered(self, cap=0, m=6):
        self.L.policy_fused_levels_delivered(self.p, 1 if cap else 0, m)


@pytest.fixture
def pol(lib):
    p = Policy(lib)
    p.set("fuse_min_samples", 65536)      # (as the GPU tests set it: 2^17-sample signals qualify)
    yield p
    lib.policy_free(p.p)


def test_a_workload_refused_every_time_backs_off_exponentially(pol):
    attempts = []
    for call in range(1, 61):
        _, kf, l0, _ = pol.call()
        if kf:
            attempts.append(call)
            assert l0 == 3
            assert pol.refused(VERIFY, l0=l0) == REPEAT_CALL
    assert attempts == [1, 18, 51] and pol.fuse_repeats == 3
    assert pol.fuse_off_span == 64
    # the next attempt, delivered: the pause starts over at 16
    call = 60
    while not pol.call()[1]:
        call += 1
    assert call + 1 == 51 + 64 + 1
    pol.delivered()
    assert pol.fuse_off_span == 16 and not pol.fuse_probe
    assert pol.refused(VERIFY) == REPEAT_CALL and pol.fuse_off_left == 16


def test_a_refusal_at_one_level_learns_a_cap_that_is_probed(pol):
    n, m = 1 << 20, 9
    _, kf, l0, cap = pol.call(n=n, m=m)
    assert kf and l0 == 3 and cap == 0
    assert pol.refused(VERIFY | 8, fail_lev=8, l0=l0, cap=cap, m=m) == REPEAT_CALL
    assert pol.fuse_cap_auto == 8 and pol.fuse_cap_span == 16 and pol.fuse_off_left == 0   # capped next, no pause
    forms = [(l0, cap)]
    for call in range(1, 40):
        _, kf, l0, cap = pol.call(n=n, m=m)
        assert kf
        forms.append((l0, cap))
        if cap:
            pol.delivered(cap, m)
        else:      # the probe: refused at the same level again, the next probe comes later
            assert pol.refused(VERIFY, fail_lev=8, l0=l0, cap=cap, m=m) == REPEAT_CALL
    assert [k for k, f in enumerate(forms) if f[1] == 0] == [0, 17], forms
    assert all(f == (3, 8) for k, f in enumerate(forms) if k not in (0, 17))
    assert pol.fuse_cap_span == 32 and pol.fuse_repeats == 2
    # another workload: the capped calls deliver it, and the probe behind them (32 calls after the last one) drops the cap
    seen = []
    for call in range(40):
        _, kf, l0, cap = pol.call(n=n, m=m)
        seen.append(cap)
        pol.delivered(cap, m)
    assert seen.index(0) == 17 + 1 + 32 - 40 and seen[-1] == 0
    assert pol.fuse_cap_auto == 0 and pol.fuse_cap_span == 16 and pol.fuse_cap_calls == 0 and pol.fuse_repeats == 2


def test_a_refusal_outside_the_call_s_levels_learns_no_cap(pol):
    assert pol.refused(VERIFY, fail_lev=4, l0=3, m=6) == REPEAT_CALL             # (fewer than two fused levels in front of it)
    assert pol.fuse_cap_auto == 0 and pol.fuse_off_left == 16
    pol.set("fuse_mode", FUSE_AUTO)
    pol.set("fuse_cap", -1)                                                       # a cap set by the caller: nothing is learned
    assert pol.refused(VERIFY, fail_lev=6, l0=3, m=6) == REPEAT_CALL and pol.fuse_cap_auto == 0


def test_capacity_fails_move_the_first_level_then_halve_the_range(pol):
    n = 1 << 22
    _, kf, l0, _ = pol.call(n=n, m=8)
    assert kf and l0 == 2 and pol.L.policy_tiles_per_wg(pol.p) == 64
    assert pol.refused(CAPACITY, l0=2, m=8) == REPEAT_CALL
    assert pol.fuse_level2_off and pol.fuse_off_left == 0
    ranges = []
    for _ in range(3):
        _, kf, l0, _ = pol.call(n=n, m=8)
        assert kf and l0 == 3
        ranges.append(pol.L.policy_tiles_per_wg(pol.p))
        pol.refused(CAPACITY, l0=3, m=8)
    assert ranges == [64, 32, 16] and pol.kf_shrink == 2
    # 16 tiles and still too many knots: the calls go level by level for a while
    assert pol.fuse_off_left == 16
    assert [pol.call(n=n, m=8)[1] for _ in range(17)] == [False] * 16 + [True]


def test_a_wait_only_fail_switches_to_tickets_once(pol):
    assert not pol.L.policy_tickets(pol.p, 100, 1000) and pol.L.policy_tickets(pol.p, 1001, 1000)
    assert pol.refused(WAIT) == REPEAT_CALL
    assert pol.kf_force_tickets and pol.fuse_off_left == 0
    assert pol.L.policy_tickets(pol.p, 100, 1000)
    assert pol.refused(WAIT) == REPEAT_CALL and pol.fuse_off_left == 16         # the second time: a pause
    pol.set("fuse_mode", FUSE_AUTO)
    assert pol.refused(WAIT | VERIFY) == REPEAT_CALL and pol.fuse_off_left == 16  # (not a wait-only fail)


def test_a_few_refused_signals_of_a_batch_are_repaired_without_a_pause(pol):
    assert pol.refused(VERIFY, fail_lev=5, nfail=2, batch=16) == REPAIR_SIGNALS
    assert pol.fuse_off_left == 0 and pol.fuse_cap_auto == 0 and pol.fuse_repeats == 0
    assert pol.refused(CAPACITY, l0=3, nfail=1, batch=8) == REPAIR_SIGNALS and pol.kf_shrink == 1   # (back_off is learned)
    assert pol.refused(VERIFY, nfail=3, batch=16) == REPEAT_CALL and pol.fuse_repeats == 1
    pol.set("fuse_mode", FUSE_ONLY)
    assert pol.refused(VERIFY) == FAIL and pol.fuse_repeats == 1 and pol.fuse_off_left == 0


def test_a_resident_fail_keeps_the_next_16_calls_level_by_level(pol):
    L = pol.L
    assert L.policy_resident(pol.p, 1, 0) and not L.policy_resident(pol.p, 0, 0) and not L.policy_resident(pol.p, 1, 1)
    assert L.policy_resident_failed(pol.p) and pol.resident_repeats == 1
    assert [bool(L.policy_resident(pol.p, 1, 0)) for _ in range(17)] == [False] * 16 + [True]
    pol.set("resident_mode", RESIDENT_ONLY)
    assert not L.policy_resident_failed(pol.p) and pol.resident_repeats == 1 and pol.resident_off_left == 0
    pol.set("resident_mode", RESIDENT_AUTO)
    pol.set("l0_mode", LEVEL0_RECORDS)
    assert not L.policy_resident(pol.p, 1, 0)                                     # (a level-0 mode means the level-by-level form)


def test_a_level0_shortfall_keeps_the_next_16_calls_record_driven(pol):
    L = pol.L
    assert L.policy_level0_fell_short(pol.p)
    forms = [pol.call() for _ in range(17)]
    assert [f[0] for f in forms] == [False] * 16 + [True]
    assert not any(f[1] for f in forms[:16])                                      # (no fused sparse levels without fused level 0)
    pol.set("l0_mode", LEVEL0_FUSED)
    assert not L.policy_level0_fell_short(pol.p) and pol.l0_records_left == 0


def test_the_device_side_repair_learns_only_from_many_failed_signals(pol):
    L = pol.L
    L.policy_device_repaired(pol.p, 2, 1 | 2 | 4 | (VERIFY << 3), 32, 3)          # a few of 32: counted, nothing learned
    assert pol.device_repairs == 2 and pol.fuse_off_left == 0 and pol.l0_records_left == 0 and pol.resident_off_left == 0
    L.policy_device_repaired(pol.p, 1, 1 | 2 | 4 | (VERIFY << 3), 1, 3)
    assert pol.device_repairs == 3 and pol.fuse_off_left == 16 and pol.l0_records_left == 16 and pol.resident_off_left == 16
    assert pol.fuse_repeats == 0 and pol.resident_repeats == 0
    pol.set("fuse_mode", FUSE_AUTO)
    L.policy_device_repaired(pol.p, 1, 1 | (CAPACITY << 3), 1, 3)                 # a back-off that stays fused: no pause
    assert pol.kf_shrink == 1 and pol.fuse_off_left == 0


def test_running_out_of_memory_leaves_the_fused_levels_for_good(pol):
    assert pol.L.policy_workspace_unavailable(pol.p) and pol.fuse_no_memory
    assert not any(pol.call()[1] for _ in range(40))
    pol.set("fuse_mode", FUSE_ONLY)
    assert pol.call()[1]


def test_the_automatic_choices_follow_the_call_s_geometry(pol):
    L = pol.L
    assert L.policy_first_level(pol.p, 1 << 22, 8) == 2 and L.policy_first_level(pol.p, (1 << 22) - 1, 8) == 3
    assert L.policy_first_level(pol.p, 1 << 20, 2) == 2                           # (fewer levels asked for than level 3)
    assert not L.policy_fused_levels(pol.p, 65535, 1 << 24, 8, 1)                 # too short a signal
    assert not L.policy_fused_levels(pol.p, 1 << 16, 65535, 8, 1)                 # too few samples per launch sequence
    assert not L.policy_fused_levels(pol.p, 1 << 20, 1 << 20, 1, 1)               # too few levels
    assert not L.policy_fused_levels(pol.p, 1 << 20, 1 << 20, 8, 0)               # behind record-driven level 0
    pol.set("fuse_level", 5)
    assert L.policy_first_level(pol.p, 1 << 24, 8) == 5 and not L.policy_fused_levels(pol.p, 1 << 20, 1 << 20, 4, 1)
    assert L.policy_cap(pol.p, 2, 8) == 0
    pol.set("fuse_cap", 6)
    assert L.policy_cap(pol.p, 2, 8) == 6 and L.policy_cap(pol.p, 5, 8) == 0 and L.policy_cap(pol.p, 2, 4) == 0


def test_each_setter_clears_what_belongs_to_it(pol):
    L = pol.L
    L.policy_resident_failed(pol.p)
    L.policy_level0_fell_short(pol.p)
    pol.refused(CAPACITY, l0=2, m=8)             # level 2 off
    pol.refused(CAPACITY, l0=3, m=8)             # range halved
    pol.refused(VERIFY)                          # a pause
    pol.refused(VERIFY, fail_lev=6, l0=3, m=8)   # cap learned
    pol.call()                                   # (counts l0_records_left down)
    learned = dict(resident_off_left=16, l0_records_left=15, fuse_level2_off=1, kf_shrink=1, fuse_cap_auto=6, fuse_off_left=16)
    assert {k: getattr(pol, k) for k in learned} == learned
    expect = dict(learned)
    for what, cleared in (("resident_mode", {"resident_off_left": 0}), ("l0_mode", {"l0_records_left": 0}),
                          ("fuse_level", {"fuse_level2_off": 0}), ("fuse_range", {"kf_shrink": 0}),
                          ("fuse_cap", {"fuse_cap_auto": 0}), ("fuse_mode", {"fuse_off_left": 0}), ("fuse_min_samples", {})):
        pol.set(what, 0 if what != "fuse_min_samples" else 65536)
        expect.update(cleared)
        assert {k: getattr(pol, k) for k in learned} == expect, what
    # the rest of what the setters reset
    pol.refused(VERIFY)
    pol.call()
    for _ in range(16):
        pol.call()
    assert pol.fuse_probe
    pol.refused(VERIFY)                          # a refused probe: the next pause is longer
    assert pol.fuse_off_span == 32
    pol.set("fuse_mode", FUSE_AUTO)
    assert pol.fuse_off_span == 16 and pol.fuse_off_left == 0 and not pol.fuse_probe
    pol.refused(VERIFY, fail_lev=6, l0=3, m=8)
    pol.delivered(6, 8)
    assert pol.fuse_cap_calls == 1
    pol.set("fuse_cap", 0)
    assert pol.fuse_cap_auto == 0 and pol.fuse_cap_calls == 0 and pol.fuse_cap_span == 16
    # the counters stay
    assert pol.resident_repeats == 1 and pol.fuse_repeats >= 4


def test_the_spline_form_at_every_edge_of_its_table(lib):
    """spline_form(solver, n, batch).  The rule: parallel in the knots when the solver is set to it, or automatically for fewer than
    256 signals of at least 1024 samples; then one signal of at most 8192 samples takes the one-workgroup form.  Every value below
    is written out from that rule."""
    batches = (1, 2, 255, 256)
    expect = {
        (SPLINE_AUTO, 1023): (SERIAL, SERIAL, SERIAL, SERIAL),
        (SPLINE_AUTO, 1024): (SMALL, PARALLEL, PARALLEL, SERIAL),
        (SPLINE_AUTO, 8192): (SMALL, PARALLEL, PARALLEL, SERIAL),
        (SPLINE_AUTO, 8193): (PARALLEL, PARALLEL, PARALLEL, SERIAL),
        (SPLINE_SERIAL, 1023): (SERIAL, SERIAL, SERIAL, SERIAL),
        (SPLINE_SERIAL, 1024): (SERIAL, SERIAL, SERIAL, SERIAL),
        (SPLINE_SERIAL, 8192): (SERIAL, SERIAL, SERIAL, SERIAL),
        (SPLINE_SERIAL, 8193): (SERIAL, SERIAL, SERIAL, SERIAL),
        (SPLINE_PARALLEL, 1023): (SMALL, PARALLEL, PARALLEL, PARALLEL),
        (SPLINE_PARALLEL, 1024): (SMALL, PARALLEL, PARALLEL, PARALLEL),
        (SPLINE_PARALLEL, 8192): (SMALL, PARALLEL, PARALLEL, PARALLEL),
        (SPLINE_PARALLEL, 8193): (PARALLEL, PARALLEL, PARALLEL, PARALLEL),
    }
    for (solver, n), forms in expect.items():
        got = tuple(lib.policy_spline_form(solver, n, b) for b in batches)
        assert got == forms, (solver, n, got)


ONE_LAUNCH_N = (2, 3, 1023, 1024, 8192, 8193)
ONE_LAUNCH = {
    SPLINE_AUTO: (False, False, False, True, True, False),
    SPLINE_SERIAL: (False, False, False, False, False, False),
    SPLINE_PARALLEL: (False, True, True, True, True, False),
}


def test_meitd_is_one_launch_where_its_extractions_take_the_one_workgroup_form(lib):
    """meitd_one_launch(solver, n): at least 3 samples, at most 8192, and the parallel-in-knots form of ONE signal (set, or
    automatic from 1024 samples) — written out from that rule."""
    for solver, expect in ONE_LAUNCH.items():
        got = tuple(bool(lib.policy_meitd_one_launch(solver, n)) for n in ONE_LAUNCH_N)
        assert got == expect, (solver, got)


def test_the_python_driver_s_one_launch_rule_is_the_engine_s(lib):
    """pyitd_amd/meitd.py decides by its own restatement whether to call the one-launch entries; the entries refuse a call the
    engine's rule does not cover, so the two must agree."""
    from pyitd_amd import meitd
    for name, solver in (("auto", SPLINE_AUTO), ("serial", SPLINE_SERIAL), ("parallel", SPLINE_PARALLEL)):
        for n, expect in zip(ONE_LAUNCH_N, ONE_LAUNCH[solver]):
            assert bool(meitd._one_launch(n, name)) == bool(lib.policy_meitd_one_launch(solver, n)) == expect, (name, n)
