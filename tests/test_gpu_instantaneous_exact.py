"""The instantaneous amplitude / phase / frequency operator (itd_tfe.hpp) against its EXACT results (oracle/exact_tfe.py), at
the lengths and on the signals where its two code paths can go wrong: the inner-tile path (s >= 64 and s + 514 <= n) and the
generic loop, lane 63's hand-over to the next step, the last sample's backward difference, the segmented maximum inside a step
and the atomic maximum across tiles, and the per-tile crossing bases of the ordered compaction.

Bounds, with u = ulp(2 pi) = 2^-50: amplitude bit for bit; phase within 4 u of the exact value and inside its quadrant's interval;
frequency within 8 u / (2 pi) as a distance mod 1, and as a plain distance (the wrap decided as the exact one decides it)
wherever the exact phase difference exceeds 8 u.  The file also passes with PYITD_POISON=1.
"""
import itertools

import numpy as np
import pytest

from helpers import DevArrays
from oracle import exact_tfe as et
from test_oracle_exact_tfe import FAMILIES, family

pytestmark = pytest.mark.gpu
U = et.ULP_2PI
PH_TOL = 4 * U
F_TOL = 8 * U / (2 * np.pi)
SENT = -7.25e300


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


def check(x, a, p, f, samples=None, what=""):
    """The three outputs of the operator on x against the exact results (at `samples`, default every sample)."""
    ex = et.exact_tfe(x, samples)
    s = ex.samples
    _bits(a[s], ex.amp, "%s: amplitude" % what)
    pe = ex.phase_err(p)
    assert pe.max() <= PH_TOL, "%s: phase off by %.3g u at sample %d" % (what, pe.max() / U, s[np.argmax(pe)])
    lo, hi = et.quadrant_bounds(ex.quad)
    ps = p[s]
    live = ~ex.zero_amp
    assert np.all(ps[ex.zero_amp] == 0.0), "%s: phase of an all-zero half wave" % what
    out = live & ((ps < lo - PH_TOL) | (ps > hi + PH_TOL))
    assert not out.any(), "%s: phase outside its quadrant at samples %s" % (what, s[out][:8])
    fe = ex.freq_err(f)
    assert fe.max() <= F_TOL, "%s: frequency off by %.3g u/2pi at sample %d" % (what, fe.max() * 2 * np.pi / U, s[np.argmax(fe)])
    decided = np.abs(ex.dp) > 8 * U
    fl = ex.freq_err(f, circular=False)[decided]
    assert fl.size == 0 or fl.max() <= F_TOL, "%s: the wrap decided the other way at sample %d" % (
        what, s[decided][np.argmax(fl)])


LENGTHS = sorted({n for n in range(3, 1601) if n % 64 in (0, 1, 2, 3)} |
                 {512 * k + d for k in (1, 2, 3) for d in (513, 514, 515)})


@pytest.mark.parametrize("fam", ["seams", "quantised"])
def test_every_length_near_the_step_and_tile_seams(P, fam):
    for n in LENGTHS:
        x = family(fam, n)
        a, p, f = P.instantaneous(x)
        check(x, a, p, f, what="%s n=%d" % (fam, n))


@pytest.mark.parametrize("fam", FAMILIES)
def test_signal_families(P, fam):
    for n in (3, 5, 64, 65, 1025, 2 * 512 + 514, 20011):
        x = family(fam, n)
        a, p, f = P.instantaneous(x)
        check(x, a, p, f, what="%s n=%d" % (fam, n))


def test_half_waves_of_many_tiles(P):
    n = 60000
    x = family("slow", n)
    a, p, f = P.instantaneous(x)
    check(x, a, p, f, what="slow")
    c = np.flatnonzero(et.structure(x)[0])
    assert np.diff(c).min() >= 3 * 512


def test_a_signal_of_two_million_samples(P):
    """2^20 + 3 samples: a tone of ~2000 crossings, crossings forced onto step and tile seams in the first and last tiles;
    exact on a subset (every crossing +-1, every tile edge +-1, the ends and a stride)."""
    n = (1 << 20) + 3
    t = np.arange(n, dtype=np.float64)
    x = np.sin(2 * np.pi * t / 1031.0 + 0.1) * (1.0 + 0.5 * np.sin(2 * np.pi * t / 90001.0))
    x[:2048] = family("seams", 2048)
    x[-2048:] = family("seams", 2048)
    a, p, f = P.instantaneous(x)
    check(x, a, p, f, samples=et.sample_subset(n, x), what="2^20+3")


@pytest.mark.parametrize("fam", ["seams", "quantised", "noise", "slow"])
def test_power_of_two_scaling(P, fam):
    """Every operation is homogeneous in x: the amplitude scales exactly, phase and frequency are bit-identical."""
    for n in (1031, 2 * 512 + 514):
        x = family(fam, n)
        a, p, f = P.instantaneous(x)
        for k in (400, -400):
            a2, p2, f2 = P.instantaneous(np.ldexp(x, k))
            _bits(a2, np.ldexp(a, k), "%s 2^%d amplitude" % (fam, k))
            _bits(p2, p, "%s 2^%d phase" % (fam, k))
            _bits(f2, f, "%s 2^%d frequency" % (fam, k))


def test_a_row_with_a_nan_is_refused_with_the_outputs_untouched(P):
    """1030 samples are three tiles, the last of 6 samples; the NaN sits in the second.  itd_instantaneous_f64 answers
    ITD_ERR_NONFINITE and has written nothing: every element of the three outputs keeps its sentinel."""
    from pyitd_amd.engine import ITD_ERR_NONFINITE
    from pyitd_amd.itd import _engine_for
    n = 1030
    x = family("noise", n)
    x[700] = np.nan
    eng = _engine_for(n)
    sent = np.full(n + 13, SENT)
    d = DevArrays(eng, x=x, a=sent, p=sent, f=sent)
    rc = eng._L.itd_instantaneous_f64(eng._h, d.ptr("x"), n, d.ptr("a"), d.ptr("p"), d.ptr("f"), None)
    assert rc == ITD_ERR_NONFINITE, rc
    for k in ("a", "p", "f"):
        assert np.all(d.get(k) == SENT), "%s is written" % k
    d.free()


def test_device_form_every_subset_of_outputs_on_a_callers_stream(P):
    """itd_instantaneous_f64 on device buffers: the input is filled by a copy queued on the caller's stream, the call runs on
    that stream, the results are read after that stream alone has been synchronised; every non-empty subset of outputs equals
    the full call bit for bit; the outputs not asked for and the pad behind each output keep their sentinels, the input is
    left alone."""
    import torch
    from pyitd_amd.itd import _engine_for
    n, pad = 5 * 512 + 77, 13
    x_old = family("noise", n)
    x_new = family("seams", n)
    eng = _engine_for(n)
    full = [np.full(n + pad, SENT) for _ in range(3)]
    d = DevArrays(eng, x=x_old, stage=x_new, a=full[0], p=full[1], f=full[2])
    s = torch.cuda.Stream()
    names = ("a", "p", "f")
    ref = None
    for mask in [(1, 1, 1)] + [m for m in itertools.product((0, 1), repeat=3) if 0 < sum(m) < 3]:
        d.put("x", x_old)
        for k in names:
            d.put(k, np.full(n + pad, SENT))
        eng.copy(d.ptr("x"), d.ptr("stage"), x_new.nbytes, 2, wait=False, stream=s.cuda_stream)
        ptrs = [d.ptr(k) if on else None for k, on in zip(names, mask)]
        rc = eng._L.itd_instantaneous_f64(eng._h, d.ptr("x"), n, *ptrs, s.cuda_stream)
        assert rc == 0, rc
        s.synchronize()
        got = {k: d.get(k) for k in names}
        _bits(d.get("x"), x_new, "the input is left alone")
        for k, on in zip(names, mask):
            assert np.all(got[k][n:] == SENT), "%s: the pad behind %s is written" % (mask, k)
            if not on:
                assert np.all(got[k] == SENT), "%s: %s was not asked for" % (mask, k)
        if ref is None:
            ref = {k: got[k][:n] for k in names}
            check(x_new, ref["a"], ref["p"], ref["f"], what="device form")
        else:
            for k, on in zip(names, mask):
                if on:
                    _bits(got[k][:n], ref[k], "%s: %s = the full call's" % (mask, k))
    d.free()
