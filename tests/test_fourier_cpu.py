"""The ITD-Fourier cascade's surface, argument checks and selector goldens without a GPU (pyitd_amd/fourier.py,
include/pyitd_hip.h: itd_debug_fft_f64, itd_fourier_mode_*_f64, itd_fourier_cascade_*, itd_fourier_modes_f64).

The goldens (tests/golden/fourier/, tools/gen_fourier_golden.py) hold the reference's own modes; the float64 restatement of both
selectors here must take the same decisions and come within 1e-6 of scale of them (the reference builds its inverse from complex64).
"""
import ctypes
import glob
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOURIER = os.path.join(ROOT, "tests", "golden", "fourier")
INVALID = 1


def restate(x, rule):
    """fourier_mode_decomposition_any (:171-209) / _valid (:131-168) in float64: (rec int32[6], mode float64).  rec: status,
    peak_max, first_peak, last_peak, mina, minb (-1: not reached)."""
    X = np.fft.fft(np.asarray(x, dtype=np.float64))
    a = np.abs(X)
    n = a.shape[0]
    half = n // 2
    pm = fp = lp = mina = minb = -1
    ok = False
    if rule == "any":
        pm = int(np.argmax(a[1:half])) + 1
        if pm != 1 and pm != half - 1:
            fp = int(np.argmax(a[:pm]))
            lp = int(np.argmax(a[pm + 1:half])) + pm + 1
            ok = not (fp == pm - 1 or lp == pm + 1)
    else:
        peaks = [i for i in range(1, half - 1) if a[i] > a[i - 1] and a[i] > a[i + 1]]
        if len(peaks) >= 3:
            pm = sorted(peaks, key=lambda i: a[i], reverse=True)[0]
            below = [i for i in peaks if i < pm - 1]
            above = [i for i in peaks if i > pm + 1]
            if below and above:
                fp, lp, ok = max(below), min(above), True
    xn = np.zeros(n, dtype=np.complex64)
    if ok:
        mina = fp + int(np.argmin(a[fp:pm + 1]))
        minb = pm + int(np.argmin(a[pm:lp + 1]))
        xn[mina:minb] = X[mina:minb]
        xn[-minb:-mina] = X[-minb:-mina]
    return np.array([int(ok), pm, fp, lp, mina, minb], np.int32), np.fft.ifft(xn.astype(np.complex128)).real


def selector_cases():
    out = []
    for f in sorted(glob.glob(os.path.join(FOURIER, "selectors_*.npz"))):
        z = np.load(f)
        for i, (name, rule) in enumerate(zip(z["names"], z["rules"])):
            lo, hi = z["offs"][i], z["offs"][i + 1]
            out.append(("%s_%s" % (name, rule), str(rule), z["x"][lo:hi].astype(np.float64), z["recs"][i], z["modes"][lo:hi].astype(np.float64)))
    return out


def cascade_cases():
    return sorted(os.path.basename(f)[8:-4] for f in glob.glob(os.path.join(FOURIER, "cascade_*.npz")))


def test_goldens_cover_what_the_selectors_need():
    cases = selector_cases()
    names = {c[0] for c in cases}
    assert len(cases) >= 100
    for must in ("n8191_any", "n8192_any", "n8193_any", "n10007_any", "n12000_any", "n44100_any", "delta64_any", "delta64_valid"):
        assert must in names, must
    recs = np.stack([c[3] for c in cases])
    assert (recs[:, 0] == 0).any() and (recs[:, 0] == 1).any()          # rejections and modes
    ties = [c for c in cases if c[0].startswith("tie_")]
    assert len(ties) >= 6                                              # exact ties, both rules
    mina0 = [c for c in ties if c[1] == "any" and c[3][0] == 1 and c[3][4] == 0]
    assert len(mina0) >= 3                                             # mina == 0: the second slice xn[-minb:-0] is empty
    for c in mina0:
        a = np.abs(np.fft.fft(c[2]))
        pm, fp, lp, mina, minb = c[3][1:]
        assert fp == 0 and (a[:pm] == a[0]).all()                      # first_peak: an argmax tie, the first index wins
        assert (a[minb:lp + 1] == a[minb]).sum() >= 2 or a[minb] == 0   # minb: an argmin over a run of exact zeros
    assert len(cascade_cases()) >= 3


@pytest.mark.parametrize("case", selector_cases(), ids=lambda c: c[0])
def test_float64_restatement_reproduces_the_reference_selectors(case):
    name, rule, x, rec, mode_ref = case
    mine, mode = restate(x, rule)
    assert np.array_equal(mine, rec), (name, mine, rec)
    scale = max(np.max(np.abs(x)), 1e-300)
    assert np.max(np.abs(mode - mode_ref)) <= 1e-6 * scale


def test_python_surface_takes_the_reference_parameters():
    import pyitd_amd
    for f in (pyitd_amd.fourier_mode_decomposition_any, pyitd_amd.fourier_mode_decomposition_valid):
        assert list(inspect.signature(f).parameters)[0] == "rotation"
    for f in (pyitd_amd.itd_fourier_decomposition, pyitd_amd.itd_fourier_decomposition_lean):
        p = inspect.signature(f).parameters
        assert list(p)[:2] == ["signal", "sample_rate"]
        assert p["max_rounds"].default is None and p["verbose"].default is False
    assert "signals" in inspect.signature(pyitd_amd.itd_fourier_decomposition_batch).parameters


def test_new_entries_refuse_null_arguments_before_any_hip_call():
    from pyitd_amd import _lib
    _lib.build()
    L = _lib.load()
    buf = (ctypes.c_double * 64)()
    i64 = (ctypes.c_int64 * 4)(0, 1, 2, 0)
    idx = (ctypes.c_int64 * 1)(2)
    i32 = (ctypes.c_int32 * 4)()
    o64 = (ctypes.c_int64 * 4)()
    assert L.itd_debug_fft_f64(None, buf, buf, 8, 1, 0) == INVALID
    for fn in (L.itd_fourier_mode_any_f64, L.itd_fourier_mode_valid_f64):
        assert fn(None, buf, 8, 1, 8, buf, 8, None, None) == INVALID
    assert L.itd_fourier_cascade_f64(None, buf, 8, 1, 8, 100.0, 1, i64, idx, 0, 5, buf, None, i32, i32, o64) == INVALID
    assert L.itd_fourier_cascade_host_f64(None, buf, 8, 1, 100.0, 1, i64, idx, 0, 5, buf, None, i32, i32, o64) == INVALID
    assert L.itd_fourier_modes_f64(None, None, 0, None, 1) == INVALID
