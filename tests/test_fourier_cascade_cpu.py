"""tests/cascade_ref.py on the CPU: the composition over the float64 oracles (oracle/cpu_oracle.py's find_extrema and
itd_baseline_extract_fast, test_fourier_cpu.restate) must reproduce the four cascade goldens — records and iteration count exactly,
the full and lean outputs within the project's 1e-6 of scale (the reference runs its inverse in float32) — and its plan, cap and
lean forms must be what tests/test_gpu_fourier_cascade.py takes them for.
"""
import numpy as np
import pytest

import cascade_ref as cr
from test_fourier_cpu import FOURIER, cascade_cases, restate


def _cubic(problem, knots, idx):
    from oracle import cpu_oracle
    return cpu_oracle.itd_baseline_extract_fast(problem, knots, idx)


def _select(row):
    rec, mode = restate(row, "any")
    return mode, rec


def _find_extrema(signal):
    from oracle import cpu_oracle
    return cpu_oracle.find_extrema(signal)


_memo = {}


def _golden(name):
    """(x, sample_rate, golden, the full composition, the lean one), computed once and left unchanged."""
    if name not in _memo:
        z = np.load("%s/cascade_%s.npz" % (FOURIER, name))
        x, sr = z["x"], int(z["sample_rate"])
        _memo[name] = (x, sr, z, cr.compose(x, sr, _cubic, _select, find_extrema=_find_extrema),
                       cr.compose(x, sr, _cubic, _select, lean=True, find_extrema=_find_extrema))
    return _memo[name]


@pytest.mark.parametrize("name", cascade_cases())
def test_composition_over_the_oracles_reproduces_the_goldens(name):
    x, sr, z, full_c, lean_c = _golden(name)
    scale = np.max(np.abs(x))
    full, recs = z["full"].astype(np.float64), z["records"]
    lean, j = [], 0          # the lean reference from `full`, as tests/test_gpu_fourier.py derives it
    for i in range(len(full) - len(recs) - 1):
        k = int((recs[:, 1] == i).sum())
        lean += [full[j:j + k].sum(axis=0) if k else np.zeros_like(x), full[j + k]]
        j += k + 1
    lean.append(full[-1])
    for res, is_lean, ref in ((full_c, False, full), (lean_c, True, np.stack(lean))):
        assert res["rounds"] == int(z["iterations"]) and not res["capped"]
        assert np.array_equal(res["records"], recs)
        out = cr.outputs(res, is_lean)
        assert len(out) == ref.shape[0]
        err = max(float(np.max(np.abs(o - r))) for o, r in zip(out, ref))
        print("%s %s: %.3g of scale" % (name, "lean" if is_lean else "full", err / scale))
        assert err <= 1e-6 * scale, (name, is_lean, err)


TABLE = {**cr.VALID_PAIRS, **cr.GOLDEN_PAIRS}


@pytest.mark.parametrize("pair", sorted(TABLE))
def test_every_pair_of_the_table_is_a_valid_plan(pair):
    lists, idxs = cr.plan(pair[0], pair[1], _find_extrema)
    assert tuple(idxs) == TABLE[pair]
    for kn, idx in zip(lists, idxs):
        # 0, the sine's sign changes, the extrapolated index, and the zero behind it that find_extrema's idx counts
        assert kn.shape == (idx + 1,) and kn[0] == 0 and kn[idx] == 0 and (kn >= 0).all() and (kn < pair[0]).all()
        assert (np.diff(kn[:idx]) > 0).all() or idx == 2          # idx = 2: no sign change, the extrapolation of 0, 0 is 0


def test_the_smallest_spline_is_among_the_pairs():
    assert sum(2 in idx for idx in cr.VALID_PAIRS.values()) >= 2
    assert {len(idx) for idx in cr.VALID_PAIRS.values()} >= {1, 2, 4, 5}


@pytest.mark.parametrize("pair", cr.INVALID_PAIRS)
def test_invalid_neighbours_raise(pair):
    with pytest.raises((IndexError, ValueError)):
        cr.plan(pair[0], pair[1], _find_extrema)


def test_max_rounds_is_the_composition_stopped_after_that_round():
    name = next(nm for nm in cascade_cases() if _golden(nm)[3]["rounds"] >= 3 and _golden(nm)[0].shape[0] <= 2000)
    x, sr, _, free, free_lean = _golden(name)
    for lean, ref in ((False, free), (True, free_lean)):
        for cap in (1, 2):
            res = cr.compose(x, sr, _cubic, _select, lean=lean, max_rounds=cap, find_extrema=_find_extrema)
            rows, n_modes, acc = ref["per_round"][cap - 1]
            assert res["capped"] and res["rounds"] == cap
            assert np.array_equal(res["rows"].view(np.uint64), rows.view(np.uint64))
            assert len(res["modes"]) == n_modes
            for a, b in zip(res["modes"], ref["modes"]):
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
            assert np.array_equal(res["records"], ref["records"][:n_modes])
            if lean:
                assert np.array_equal(res["acc"].view(np.uint64), acc.view(np.uint64))
    with pytest.raises(ValueError):
        cr.compose(x, sr, _cubic, _select, max_rounds=0, find_extrema=_find_extrema)


@pytest.mark.parametrize("name", cascade_cases())
def test_lean_and_full_compositions_agree(name):
    _, _, _, full, lean = _golden(name)
    assert np.array_equal(full["rows"].view(np.uint64), lean["rows"].view(np.uint64))
    assert np.array_equal(full["records"], lean["records"]) and full["rounds"] == lean["rounds"]
    for k in range(lean["acc"].shape[0]):
        a = np.zeros_like(full["rows"][0])
        for j in np.flatnonzero(full["records"][:, 1] == k):
            a = a + full["modes"][j]
        assert np.array_equal(lean["acc"][k].view(np.uint64), a.view(np.uint64))
    assert np.array_equal(cr.lean_acc(full).view(np.uint64), lean["acc"].view(np.uint64))


def test_the_seeded_family_holds_the_cases_over_the_oracles():
    """What tests/test_gpu_fourier_cascade.py asserts of its own compositions, here over the oracles: the seeds end, and hold a
    signal with 0 rounds, one with at least 3, a round with at least 2 modes and a hit on the last non-residual row."""
    zero = deep = two = last_row = 0
    for pair, idx in sorted(cr.VALID_PAIRS.items()):
        for seed in cr.SEEDS[pair]:
            res = cr.compose(cr.signal(pair[0], pair[1], seed), pair[1], _cubic, _select, find_extrema=_find_extrema)
            rec = res["records"]
            zero += res["rounds"] == 0
            deep += res["rounds"] >= 3
            two += any((rec[:, 0] == r).sum() >= 2 for r in range(1, res["rounds"] + 1))
            last_row += bool((rec[:, 1] == len(idx) - 1).any())
    assert zero >= 1 and deep >= 1 and two >= 1 and last_row >= 1, (zero, deep, two, last_row)


def test_the_signal_family_is_seeded():
    a, b = cr.signal(211, 421, 3), cr.signal(211, 421, 3)
    assert np.array_equal(a, b) and not np.array_equal(a, cr.signal(211, 421, 4))
