"""The ring streams' window arithmetic and block counting (pyitd_amd/csrc/itd_ring_plan.hpp: ring_plan, ring_push, ring_flush), built
for the host with g++ (tests/c_client/ring_plan_host.cpp) and held, step by step, to a brute-force model: the list of the samples that
exist, the window [b L - H, (b+1) L + H + reach) clipped to it (reach: the 0 or 1 samples a kind reads beyond the horizon, which also
enter D = ceil((H + reach) / L)), and slot = block mod 2 D + 1.  A check of the header, not a fallback: pyitd_amd never loads this
build."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, I64 = ctypes.c_int32, ctypes.c_int64
FIELDS = ("emit", "store_slot", "slot0", "rd_lo", "rd_hi", "at_start", "at_end")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ring_plan") / "libring_plan_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                    os.path.join(ROOT, "tests", "c_client", "ring_plan_host.cpp")], check=True, capture_output=True)
    L = ctypes.CDLL(so)
    P = ctypes.c_void_p
    L.ring_args_bytes.restype, L.ring_args_bytes.argtypes = ctypes.c_int, []
    L.ring_count_fresh.restype, L.ring_count_fresh.argtypes = None, [P]
    L.ring_count_held.restype, L.ring_count_held.argtypes = I64, [P]
    L.ring_count_flushing.restype, L.ring_count_flushing.argtypes = ctypes.c_int, [P]
    L.ring_count_step.restype = ctypes.c_int
    L.ring_count_step.argtypes = [P, I64, I64, I64, I64, ctypes.c_int, ctypes.c_int, P, P, P, P, P]
    return L


class Count:
    """The library's count (t, P, sent) of one stream and one step on it."""

    def __init__(self, lib, L, H, reach):
        self.lib, self.L, self.H, self.reach = lib, L, H, reach
        self.D = -(-(H + reach) // L)
        self.c = (I64 * 3)()
        lib.ring_count_fresh(self.c)

    def state(self):
        return tuple(self.c)

    def held(self):
        return self.lib.ring_count_held(self.c)

    def flushing(self):
        return bool(self.lib.ring_count_flushing(self.c))

    def step(self, flush, fail=0):
        """(return code, emitted, the plan as a dict or None where no launch was planned)"""
        em, ran, b = I32(-1), I32(-1), I64(0)
        fields, wide = (I32 * 7)(), (I64 * 2)()
        rc = self.lib.ring_count_step(self.c, self.L, self.D, self.H, self.reach, 1 if flush else 0, fail, ctypes.byref(em),
                                      ctypes.byref(ran), ctypes.byref(b), fields, wide)
        plan = None
        if ran.value:
            plan = dict(zip(FIELDS, fields), base=wide[0], arr=wide[1], b=b.value)
        return rc, em.value, plan


def model_plan(L, H, reach, D, n_exist, b, flushing, arriving):
    """What a step that emits block b (None: none) plans when `n_exist` blocks exist; arriving: the number of the block it stores."""
    R = 2 * D + 1
    plan = dict(emit=0, store_slot=0, slot0=0, rd_lo=0, rd_hi=0, at_start=0, at_end=0, base=0,
                arr=(arriving if arriving is not None else n_exist) * L, b=-1)
    if arriving is not None:
        plan["store_slot"] = arriving % R
    if b is None:
        return plan
    exist = range(n_exist * L)                                               # the samples that exist
    win = [j for j in range(b * L - H, (b + 1) * L + H + reach) if j in exist]
    assert win and win == list(range(win[0], win[-1] + 1))
    base = (b - D) * L
    # every block the window touches is in the ring, window block k in slot (slot0 + k) % R = its own number mod R
    slot0 = (b - D) % R
    for q in range(win[0] // L, win[-1] // L + 1):
        assert b - D <= q <= b + D and q < n_exist
        assert (slot0 + q - (b - D)) % R == q % R
    plan.update(emit=1, slot0=slot0, base=base, rd_lo=win[0] - base, rd_hi=win[-1] + 1 - base, at_start=int(0 in win),
                at_end=int(flushing and n_exist * L - 1 in win), b=b)
    return plan


def run_stream(c, n_blocks):
    """n_blocks pushes, then flush steps to empty, each held to the model; the count ends fresh."""
    L, H, reach, D = c.L, c.H, c.reach, c.D
    sent = 0
    assert c.held() == 0 and not c.flushing()
    for p in range(n_blocks):
        rc, em, plan = c.step(flush=False)
        emits = p >= D
        assert rc == 0 and em == int(emits)
        assert plan == model_plan(L, H, reach, D, p + 1, p - D if emits else None, False, p)
        sent += emits
        assert c.held() == p + 1 - sent and not c.flushing()
    while sent < n_blocks:
        rc, em, plan = c.step(flush=True)
        assert rc == 0 and em == 1
        assert plan == model_plan(L, H, reach, D, n_blocks, sent, True, None)
        sent += 1
        assert c.held() == n_blocks - sent
        assert c.flushing() == (sent < n_blocks)                              # the last block: pushes are taken again
    assert sent == n_blocks and sent - min(n_blocks, D) == max(0, n_blocks - D)   # flush gave min(pushed, D) blocks
    rc, em, plan = c.step(flush=True)                                         # empty: nothing runs
    assert (rc, em, plan) == (0, 0, None)
    assert c.state() == (0, -1, 0)


def test_args_layout(lib):
    # 7 pointers / int64 and 10 int32: the kernels' argument structs keep it as their first member, 8-byte aligned behind it
    assert lib.ring_args_bytes() == 7 * 8 + 10 * 4


@pytest.mark.parametrize("reach", [0, 1])
@pytest.mark.parametrize("L", [8, 64])
def test_plan_and_count_against_model(lib, L, reach):
    for H in range(1, 2 * L + 2):
        c = Count(lib, L, H, reach)
        assert c.D == -(-(H + reach) // L)
        for n_blocks in range(0, 3 * c.D + 3):
            run_stream(c, n_blocks)
            run_stream(c, c.D + 1)                                            # a second stream on the same count: the restart


@pytest.mark.parametrize("reach", [0, 1])
@pytest.mark.parametrize("L", [8, 64])
def test_failed_steps_change_nothing(lib, L, reach):
    for H in (1, L - 1, L, L + 1, 2 * L + 1):
        c = Count(lib, L, H, reach)
        D = c.D
        for n_blocks in range(1, 3 * D + 3):
            for p in range(n_blocks):
                if p == n_blocks // 2:                                        # a push whose launch fails
                    before = c.state()
                    rc, em, plan = c.step(flush=False, fail=7)
                    assert rc == 7 and plan is not None and c.state() == before
                assert c.step(flush=False)[0] == 0
            # the first flush step fails: t, P, sent as they were, and a push is accepted afterwards
            before = c.state()
            rc, em, plan = c.step(flush=True, fail=7)
            assert rc == 7 and em == 0 and c.state() == before and not c.flushing()
            assert plan == model_plan(L, H, reach, D, n_blocks, max(0, n_blocks - D), True, None)   # (it was planned on the fixed length)
            rc, em, plan = c.step(flush=False)
            assert rc == 0 and plan == model_plan(L, H, reach, D, n_blocks + 1, n_blocks - D if n_blocks >= D else None, False, n_blocks)
            total, sent = n_blocks + 1, max(0, n_blocks + 1 - D)
            # a later flush step fails: the stream stays in its flush, nothing is counted
            assert c.step(flush=True)[:2] == (0, 1)
            sent += 1
            if sent < total:
                before = c.state()
                rc, em, plan = c.step(flush=True, fail=7)
                assert rc == 7 and em == 0 and c.state() == before and c.flushing()
                assert c.held() == total - sent
            while sent < total:
                assert c.step(flush=True)[:2] == (0, 1)
                sent += 1
            assert c.state() == (0, -1, 0)
