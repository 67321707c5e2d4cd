"""The type that owns the engine's and the streams' device and pinned memory (pyitd_amd/csrc/itd_memory.hpp), built for the host with
g++ and the address / undefined-behaviour sanitizers over malloc-backed, counting stand-ins for the runtime's allocation calls
(tests/c_client/memory_host.cpp): which calls it makes, in which order, and that every block is freed exactly once.
A check of the ownership rules, not a fallback: pyitd_amd never loads this build, and it never touches a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITD_OK, ITD_ERR_NOMEM = 0, 4          # include/pyitd_hip.h
HIP_SUCCESS, HIP_OOM = 0, 2           # the stand-ins' hipError_t


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("memory") / "memory_host")
    # (the sanitizers' runtimes linked statically: the program does not depend on what else the process has loaded)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", out, os.path.join(ROOT, "tests", "c_client", "memory_host.cpp")],
                   check=True, capture_output=True)
    return out


def run(exe, case, poison="0"):
    """The case's lines as tuples of words, numbers as ints.  A sanitizer report fails the run; leaks are what "live" counts."""
    r = subprocess.run([exe, case], capture_output=True, text=True,
                       env=dict(os.environ, PYITD_POISON=poison, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and not r.stderr, r.stderr
    lines = [tuple(int(w) if w.lstrip("-").isdigit() else w for w in ln.split()) for ln in r.stdout.splitlines()]
    assert ("bad-free",) not in lines and ("unknown-case",) not in lines
    assert lines[-1] == ("live", 0), lines          # every case ends with nothing allocated
    return lines[:-1]


def test_reserve_is_grow_only_and_frees_before_it_allocates(exe):
    assert run(exe, "reserve") == [
        ("malloc", "dev", 1, 100), ("rc", ITD_OK),
        ("rc", ITD_OK), ("same", 1),                                        # large enough: no call at all
        ("free", "dev", 1), ("malloc", "dev", 2, 200), ("rc", ITD_OK),      # the old block goes first; exactly what was asked for
        ("bytes", 200),
        ("free", "dev", 2),
    ]


def test_a_failed_reserve_leaves_an_empty_buffer_and_nomem(exe):
    assert run(exe, "reserve_fails") == [
        ("malloc", "dev", 1, 100), ("rc", ITD_OK),
        ("free", "dev", 1), ("refuse", "dev", 200), ("rc", ITD_ERR_NOMEM), ("why", HIP_OOM), ("empty", 1),
        ("malloc", "dev", 3, 50), ("rc", ITD_OK),
        ("free", "dev", 3),
    ]
    assert run(exe, "alloc_fails") == [("refuse", "dev", 64), ("hip", HIP_OOM), ("empty", 1)]


def test_release_and_the_destructor_free_once(exe):
    assert run(exe, "release") == [("malloc", "dev", 1, 64), ("hip", HIP_SUCCESS), ("free", "dev", 1), ("empty", 1), ("scope-ends",)]


def test_a_moved_from_buffer_frees_nothing(exe):
    assert run(exe, "move") == [
        ("malloc", "dev", 1, 10), ("hip", HIP_SUCCESS), ("malloc", "dev", 2, 20), ("hip", HIP_SUCCESS),
        ("moved", 1),
        ("free", "dev", 2), ("moved", 1),                                   # move assignment frees what the target held
        ("scope-ends",),
        ("free", "dev", 1),                                                 # once, by the buffer that holds it at the end
    ]


def test_a_retired_block_is_freed_once_at_its_list_s_end(exe):
    assert run(exe, "retire") == [
        ("malloc", "dev", 1, 100), ("hip", HIP_SUCCESS),
        ("malloc", "dev", 2, 200), ("hip", HIP_SUCCESS),                    # (no free in between: block 1 is the list's)
        ("malloc", "dev", 3, 400), ("hip", HIP_SUCCESS),
        ("owner-ends",), ("free", "dev", 3),
        ("list-ends",), ("free", "dev", 1), ("free", "dev", 2),
    ]


def test_only_a_counted_allocation_adds_to_the_counter(exe):
    lines = run(exe, "counted")
    assert [ln for ln in lines if ln[0] == "total"] == [("total", 100), ("total", 400)]
    assert all(ln[1] in (HIP_SUCCESS, ITD_OK) for ln in lines if ln[0] in ("hip", "rc"))
    frees = [ln for ln in lines if ln[0] == "free"]
    mallocs = [ln for ln in lines if ln[0] == "malloc"]
    assert sorted(f[2] for f in frees) == sorted(m[2] for m in mallocs) and len(mallocs) == 5


def test_pinned_memory_takes_its_flags_and_its_own_free(exe):
    assert run(exe, "pinned") == [
        ("malloc", "pin", 1, 16, "flags", 0), ("hip", HIP_SUCCESS),
        ("malloc", "pin", 2, 256, "flags", 6), ("hip", HIP_SUCCESS),
        ("free", "pin", 1), ("malloc", "pin", 3, 32, "flags", 0), ("rc", ITD_OK),
        ("free", "pin", 2), ("free", "pin", 3),
    ]


def test_every_device_block_is_poisoned_before_the_caller_s_own_fill(exe):
    assert run(exe, "poison", poison="1") == [
        ("malloc", "dev", 1, 8), ("memset", 1, 255, 8), ("sync",), ("hip", HIP_SUCCESS), ("filled", 1),
        ("memset", 1, 0, 8), ("hip", HIP_SUCCESS),
        ("malloc", "pin", 2, 8, "flags", 0), ("hip", HIP_SUCCESS),          # host memory is not poisoned
        ("free", "dev", 1), ("malloc", "dev", 3, 16), ("memset", 3, 255, 16), ("sync",), ("rc", ITD_OK),
        ("free", "pin", 2), ("free", "dev", 3),
    ]
    assert ("sync",) not in run(exe, "reserve")
