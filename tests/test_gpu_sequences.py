"""A result does not depend on what the engine ran before.

Every Python call on a device runs in one process-wide engine with grow-only workspaces that all operators share ("Order
of calls").  The other GPU tests use it in one fixed order; here every cell of tests/sequence_cases.py — one per operator family —
follows every other one, at sizes whose carve offsets differ, and is compared with what a newly created engine gives: bit for bit
(sequence_cases.BY_RULE, the operators compared by their rule alone, is empty), the fresh result itself first held to the operator's
own reference by the cell's check.

  a  ordered pairs: A(L); B(S) and A(S); B(L) for every A and B, one engine per A
  b  eight seeded walks of sixty calls over all cells and the sizes S, L and sometimes G (which re-creates the Python engine), refusing
     calls and pokes at the sticky settings (spline solver, fuse threshold) in between
  c  a refused call leaves nothing behind: the next call of every family equals fresh, the decomposition in front of it still
     delivers its summary and its lazily kept baselines
  d  lazily kept baselines survive every other cell, and the engine's re-creation by growth
  e  back to back on a caller's stream: input copies, a long decomposition and the short cell with no host synchronisation in between
The file also passes with PYITD_POISON=1 and in the modes of tools/suite_modes.sh.
"""
import numpy as np
import pytest

import sequence_cases as sc
from helpers import DevArrays, assert_bits_equal, sines_noise
from oracle import cpu_oracle

pytestmark = pytest.mark.gpu
WALK_SEED = 0


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


def _g_cells():
    return sorted({s["cell"] for w in sc.walk_schedule(WALK_SEED) for s in w if s["size"] == "G"} | {"decompose_host", "extract_host"})


@pytest.fixture(scope="module")
def fresh(P):
    """{(cell, size): the cell's result on a newly created engine}, computed once before any sequence and left unchanged
    (test_fresh_results_hold_their_references holds each to its reference)."""
    out = {}
    for name, cell in sc.CELLS.items():
        for size in ("S", "L") + (("G",) if name in _g_cells() else ()):
            sc.fresh_engines(P)
            got = cell.run(P, cell.inputs(size))
            for a in got:
                a.setflags(write=False)
            out[name, size] = got
    sc.fresh_engines(P)
    return out


class Differences(list):
    """The calls of a sequence that differ from fresh: a sequence runs to its end and reports all of them."""

    def run(self, P, fresh, name, size, what):
        got = sc.CELLS[name].run(P, sc.CELLS[name].inputs(size))
        try:
            sc.same_results(got, fresh[name, size], "%s: %s(%s) against a fresh engine" % (what, name, size))
        except AssertionError as err:
            self.append(str(err))

    def none(self):
        assert not self, "%d calls differ from a fresh engine:\n%s" % (len(self), "\n".join(self[:12]))


@pytest.mark.parametrize("size", ("S", "L"))
@pytest.mark.parametrize("name", sc.NAMES)
def test_fresh_results_hold_their_references(P, fresh, name, size):
    """What everything below is compared with is itself the operator's: the cell's check, with its own test file's rule."""
    cell = sc.CELLS[name]
    with np.errstate(all="ignore"):
        cell.check(cell.inputs(size), fresh[name, size], P)
    for g in _g_cells():
        if g == name:
            with np.errstate(all="ignore"):
                cell.check(cell.inputs("G"), fresh[name, "G"], P)


# ---- a ---------------------------------------------------------------------------------------------------------------------------
PAIR_PARTS = 4          # of the B range, so that the slowest A (MEITD driven from the host, run once in front of every B) stays at a few seconds


@pytest.mark.parametrize("part", range(PAIR_PARTS))
@pytest.mark.parametrize("first", sc.NAMES)
def test_ordered_pairs(P, fresh, first, part):
    """A(L); B(S), compare B; A(S); B(L), compare B — for every B of this part of the cells, all on the one engine this A started."""
    sc.fresh_engines(P)
    diff = Differences()
    for a, sa, b, sb in sc.pair_schedule():
        if a != first or sc.NAMES.index(b) % PAIR_PARTS != part:
            continue
        diff.run(P, fresh, a, sa, "first call")
        diff.run(P, fresh, b, sb, "%s(%s) in front" % (a, sa))
    diff.none()


# ---- b ---------------------------------------------------------------------------------------------------------------------------
def _process_engine():
    return sc.mod("itd")._engine_for(3)


def walk(P, fresh_of, steps, what):
    """Run the steps of one walk; returns the index of the first call that differs from fresh and its message, or (None, None)."""
    for i, s in enumerate(steps):
        n = sc.SIZES[s["size"]]["n"]
        if s["solver"] is not None:
            _process_engine().set_spline_solver(s["solver"])
        if s["fuse_min"] is not None:
            _process_engine().set_fuse_min_samples(s["fuse_min"])
        if s["refusal"] is not None:
            sc.REFUSALS[s["refusal"]](P, n)
        got = sc.CELLS[s["cell"]].run(P, sc.CELLS[s["cell"]].inputs(s["size"]))
        try:
            sc.same_results(got, fresh_of(s["cell"], s["size"]), "%s call %d: %s(%s) after %s" % (
                what, i, s["cell"], s["size"], [(t["cell"], t["size"], t["refusal"]) for t in steps[max(0, i - 3):i]]))
        except AssertionError as err:
            return i, str(err)
    return None, None


@pytest.mark.parametrize("w", range(sc.WALKS))
def test_walks_on_the_process_engine(P, fresh, w):
    sc.fresh_engines(P)
    i, msg = walk(P, lambda c, s: fresh[c, s], sc.walk_schedule(WALK_SEED)[w], "walk %d" % w)
    assert i is None, msg


# ---- c ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refusal", sorted(sc.REFUSALS))
def test_a_refused_call_leaves_nothing_behind(P, fresh, refusal):
    """(The sentinels of the outputs a refused call was given are asserted by the refusing call itself, sequence_cases.refuse_*.)"""
    sc.fresh_engines(P)
    n = sc.SIZES["S"]["n"]
    inp = sc.CELLS["decompose_host"].inputs("S")
    ref = cpu_oracle.itd(inp["x"], sc.M)
    # a decomposition whose baselines stay on the device, and a device decomposition whose summary has not been read
    dec = P.ITD()
    rows = dec.itd(inp["x"], max_iteration=sc.M)
    eng = sc.eng_of(P, n)
    d = DevArrays(eng, x=inp["x"], rows=np.full((sc.M + 2) * n, sc.SENT))
    try:
        eng.decompose_dev(d.ptr("x"), np.float64, n, 1, n, sc.M, d.ptr("rows"), None, None)
        sc.REFUSALS[refusal](P, n)
        s = eng.summary(1)
        assert int(s["n_rows"][0]) == len(ref["rows"]) and int(s["nan_levels"][0]) == -1
        assert_bits_equal(d.get("rows")[: len(ref["rows"]) * n].reshape(-1, n), ref["rows"], "the device decomposition in front of the refusal")
    finally:
        d.free()
    assert_bits_equal(rows, ref["rows"], "the rows in front of the refusal")
    assert_bits_equal(dec.get_baselines(), ref["baselines"], "the baselines kept in front of the refusal")
    diff = Differences()
    for r, cell in sc.refusal_schedule():
        if r == refusal:
            sc.REFUSALS[r](P, n)
            diff.run(P, fresh, cell, "S", "%s in front" % r)
    diff.none()


# ---- d ---------------------------------------------------------------------------------------------------------------------------
HOST_DECOMPOSITIONS = ("decompose_host", "decompose_rows32_host", "decompose_select_host")


@pytest.mark.parametrize("size", ("S", "L", "G"))
def test_lazy_baselines_survive_every_other_cell(P, fresh, size):
    """dec.itd(x) with its baselines left on the device; then every cell that is no host decomposition, once; then — from S and L — a
    single-level call at G, which closes and re-creates the engine (the baselines must have been brought home first); then the
    baselines.  The host decompositions run behind that: ITD.itd brings another instance's baselines home itself."""
    sc.fresh_engines(P)
    inp = sc.CELLS["decompose_host"].inputs(size)
    ref = cpu_oracle.itd(inp["x"], sc.M)
    dec = P.ITD()
    rows = dec.itd(inp["x"], max_iteration=sc.M).copy()
    other = {"S": "L", "L": "S", "G": "S"}[size]
    diff = Differences()
    for name in sc.NAMES:
        if name not in HOST_DECOMPOSITIONS:
            diff.run(P, fresh, name, other, "lazy baselines of %s pending" % size)
    assert dec._fetch is not None, "the baselines were fetched before anybody asked"
    if size != "G":
        before = sc.eng_of(P, 3)
        diff.run(P, fresh, "extract_host", "G", "growth")
        assert sc.eng_of(P, 3) is not before, "the call at G did not re-create the engine"
    assert_bits_equal(rows, ref["rows"], "rows")
    assert_bits_equal(dec.get_baselines(), ref["baselines"], "the baselines fetched at the end")
    dec2 = P.ITD()
    dec2.itd(inp["x"], max_iteration=sc.M)
    for name in HOST_DECOMPOSITIONS:
        diff.run(P, fresh, name, other, "another instance's baselines pending")
    assert_bits_equal(dec2.get_baselines(), ref["baselines"], "the baselines another instance's call brought home")
    diff.none()


@pytest.mark.parametrize("size", ("S", "L"))
def test_kept_baselines_of_the_c_level_survive_every_cell_but_a_host_decomposition(P, fresh, size):
    """itd_set_host_keep_baselines / itd_get_last_baselines_host: valid until the engine's next host-form decomposition."""
    sc.fresh_engines(P)
    inp = sc.CELLS["decompose_host"].inputs(size)
    ref = cpu_oracle.itd(inp["x"], sc.M)
    eng = sc.eng_of(P, inp["n"])
    res = eng.decompose_host(inp["x"], sc.M, want_baselines="lazy")
    assert res["n_baselines"] == len(ref["baselines"])
    diff = Differences()
    for name in sc.NAMES:
        if name not in HOST_DECOMPOSITIONS:
            diff.run(P, fresh, name, "L" if size == "S" else "S", "kept baselines of %s pending" % size)
    diff.none()
    assert sc.eng_of(P, 3) is eng
    assert_bits_equal(res["fetch_baselines"](), ref["baselines"], "itd_get_last_baselines_host at the end")
    assert_bits_equal(res["rows"], ref["rows"], "rows")


# ---- e ---------------------------------------------------------------------------------------------------------------------------
STREAM_CELLS = tuple(n for n in sc.NAMES if sc.CELLS[n].stream_form)


def _junk(a):
    """What an input buffer holds before the copy on the caller's stream fills it: the reversed values of a float array (another
    signal), zeros for an index list (in range for every consumer)."""
    return np.ascontiguousarray(a.reshape(-1)[::-1].reshape(a.shape)) if a.dtype.kind == "f" else np.zeros_like(a)


@pytest.mark.parametrize("size", ("S", "L"))
@pytest.mark.parametrize("name", STREAM_CELLS)
def test_back_to_back_on_a_callers_stream(P, fresh, name, size):
    """include/pyitd_hip.h: calls ordered on one stream are ordered with respect to each other.  On one torch stream: the copies that
    fill the cell's inputs, a decomposition of 2^18 samples, the cell — no host synchronisation in between; that stream alone is
    synchronised once at the end.  A launch or memset the library put on the engine's own stream instead of the caller's would run
    ahead of the copies and of the long call's kernels, and show here as a result that differs from fresh.  It would show only if the
    hardware happened to schedule it early: a pass cannot prove that no such race exists, and the case runs once."""
    import torch
    cell = sc.CELLS[name]
    inp = cell.inputs(size)
    eng = sc.eng_of(P, sc.LONG_N)
    arrays = cell.arrays(inp)
    for k in cell.staged:
        arrays["stage_" + k] = arrays[k]
        arrays[k] = _junk(arrays[k])
    long_x = sines_noise(sc.LONG_N, seed=3, dtype=np.float64)
    s = torch.cuda.Stream()
    d = DevArrays(eng, **arrays)
    dl = DevArrays(eng, x=long_x, rows=np.zeros((sc.M + 2) * sc.LONG_N))
    try:
        for k in cell.staged:
            eng.copy(d.ptr(k), d.ptr("stage_" + k), arrays[k].nbytes, 2, wait=False, stream=s.cuda_stream)
        eng.decompose_dev(dl.ptr("x"), np.float64, sc.LONG_N, 1, sc.LONG_N, sc.M, dl.ptr("rows"), None, s.cuda_stream)
        cell.enqueue(eng, d, inp, s.cuda_stream)
        s.synchronize()
        got = cell.collect(eng, d, inp)
    finally:
        d.free()
        dl.free()
    want = fresh[name, size]
    count = getattr(cell, "stream_outputs", len(want))
    sc.same_results(got, want[:count], "%s(%s) behind its input copies and a long decomposition on one stream" % (name, size))
