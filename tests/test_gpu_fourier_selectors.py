"""The Fourier mode selectors (k_fourier_select<VALID>, select_rows: itd_fourier_mode_any_f64 / _valid_f64) on the designed and
noisy rows of tests/fft_cases.py, whose every comparison is decided on the long-double spectrum by a relative margin above 2^-40.

Records: exact, the -1 entries of steps not reached included.  Modes: within the project's 1e-11 of the row's scale of the
restatement built from the long-double spectrum (mask, complex64 rounding, full complex inverse, real part); a rejection's mode is
all zero, compared with == 0.0.
The C entries directly, on sentinel-filled buffers with a pad behind every output: row and mode strides of n + 7, no record buffer,
the caller's stream, accepted and rejected rows in one batch: bit for bit the dense call.  kMaxGridY + 2 rows (more than one
launch and one workspace chunk hold): every copy is its single-row result.  n = 3 is refused and nothing is written.
"""
import numpy as np
import pytest

import fft_cases as fc
from helpers import DevArrays, assert_bits_equal

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not fc.LONGDOUBLE_OK, reason=fc.LONGDOUBLE_WHY)]
SENT = -7.25e300
ISENT = -123456
PAD = 7
OK, INVALID = 0, 1
RULES = ("any", "valid")
MODE_TOL = 1e-11            # of the row's scale: the project's bound on a mode against the long-double restatement


@pytest.fixture(scope="module")
def eng():
    import pyitd_amd
    e = pyitd_amd.Engine(16384, 1, 0)
    yield e
    e.close()


def _by_length(rule):
    groups = {}
    for case in fc.selector_cases(rule)[0]:
        groups.setdefault(case[2].shape[0], []).append(case)
    return groups


@pytest.mark.parametrize("rule", RULES)
def test_records_and_modes_of_every_decided_case(rule):
    from pyitd_amd.fourier import fourier_mode_batch
    groups = _by_length(rule)
    assert set(fc.SELECTOR_NS) | set(fc.NOISY_NS) == set(groups)
    wrong = []
    for n, cases in sorted(groups.items()):
        modes, recs = fourier_mode_batch(np.stack([c[2] for c in cases]), rule)
        for b, (name, _, x, rec, mode) in enumerate(cases):
            if not np.array_equal(recs[b], rec):
                wrong.append("%s: record %s, expected %s" % (name, recs[b], rec))
            elif not rec[0]:
                if not (modes[b] == 0.0).all():
                    wrong.append("%s: rejected, but the mode is not all zero" % name)
            else:
                err, tol = float(np.max(np.abs(modes[b] - mode))), MODE_TOL * float(np.max(np.abs(x)))
                if not err <= tol:
                    wrong.append("%s: mode off by %.3g, allowed %.3g" % (name, err, tol))
    assert not wrong, "\n" + "\n".join(wrong)


def _entry(eng, rule):
    return {"any": eng._L.itd_fourier_mode_any_f64, "valid": eng._L.itd_fourier_mode_valid_f64}[rule]


def _select(eng, rule, x, stride, with_rec, stream=None):
    """One call of the C entry on rows x[B, n] laid out with `stride` (the gaps and a pad behind each buffer hold sentinels):
    (rc, modes[B, n], recs[B, 6] or None).  Whatever lies between and behind the modes must come back untouched, and the rows too."""
    B, n = x.shape
    rows = np.full(B * stride + PAD, SENT)
    rows[:B * stride].reshape(B, stride)[:, :n] = x
    arrays = dict(rows=rows, modes=np.full(B * stride + PAD, SENT))
    if with_rec:
        arrays["rec"] = np.full(B * 8 + PAD, ISENT, np.int32)
    d = DevArrays(eng, **arrays)
    try:
        rc = _entry(eng, rule)(eng._h, d.ptr("rows"), n, B, stride, d.ptr("modes"), stride, d.ptr("rec") if with_rec else None,
                               None if stream is None else stream.cuda_stream)
        if stream is not None:
            stream.synchronize()
        got, recs = d.get("modes"), None
        assert_bits_equal(d.get("rows"), rows, "the rows were changed")
        assert (got[B * stride:] == SENT).all() and (got[:B * stride].reshape(B, stride)[:, n:] == SENT).all(), "written past a mode"
        if with_rec:
            r = d.get("rec")
            assert (r[B * 8:] == ISENT).all(), "written past the records"
            recs = r[:B * 8].reshape(B, 8)
            assert rc != OK or (recs[:, 6:] == 0).all()
            recs = recs[:, :6]
        return rc, got[:B * stride].reshape(B, stride)[:, :n].copy(), recs
    finally:
        d.free()


@pytest.mark.parametrize("n", (1001, 8193, 10007))          # tier 1, four-step, Bluestein
@pytest.mark.parametrize("rule", RULES)
def test_strided_rows_without_records_on_the_callers_stream(eng, rule, n):
    import torch
    cases = [c for c in _by_length(rule)[n] if not c[0].startswith("noisy")]
    want = np.stack([c[3] for c in cases])
    assert (want[:, 0] == 1).any() and (want[:, 0] == 0).any()          # accepted and rejected rows in one batch
    x = np.stack([c[2] for c in cases])
    rc, dense, recs = _select(eng, rule, x, n, True)
    assert rc == OK and np.array_equal(recs, want), (recs, want)
    assert (dense[want[:, 0] == 0] == 0.0).all()
    rc, strided, _ = _select(eng, rule, x, n + PAD, False, stream=torch.cuda.Stream())
    assert rc == OK
    assert_bits_equal(strided, dense, "%s n=%d: strides of n + 7, no records, the caller's stream" % (rule, n))


@pytest.mark.parametrize("rule", RULES)
def test_more_rows_than_one_launch_takes(eng, rule):
    n, B = 64, fc.K_MAX_GRID_Y + 2
    cases = [c for c in _by_length(rule)[n]]
    pick = [c for c in cases if c[3][0]][:3] + [c for c in cases if not c[3][0]][:3]
    assert len(pick) == 6
    x = np.stack([c[2] for c in pick])
    single = [_select(eng, rule, x[b:b + 1], n, True) for b in range(6)]
    for b, (rc, _, rec) in enumerate(single):
        assert rc == OK and np.array_equal(rec[0], pick[b][3]), (pick[b][0], rec[0], pick[b][3])
    reps = (B + 5) // 6
    rc, modes, recs = _select(eng, rule, np.tile(x, (reps, 1))[:B], n, True)
    assert rc == OK
    assert_bits_equal(modes, np.tile(np.concatenate([s[1] for s in single]), (reps, 1))[:B], "%s: kMaxGridY + 2 rows" % rule)
    assert np.array_equal(recs, np.tile(np.concatenate([s[2] for s in single]), (reps, 1))[:B])


@pytest.mark.parametrize("rule", RULES)
def test_three_samples_are_refused_and_nothing_is_written(eng, rule):
    x = np.array([[1.0, -2.0, 0.5], [0.25, 3.0, -1.0]])
    rc, modes, recs = _select(eng, rule, x, 3 + PAD, True)
    assert rc == INVALID
    assert (modes == SENT).all() and (recs == ISENT).all()
