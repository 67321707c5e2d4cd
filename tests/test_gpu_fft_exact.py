"""The engine's FFT (itd_fft.hpp, itd_fourier.inc: itd_debug_fft_f64) against the long-double reference of tests/fft_cases.py.

Accuracy: every listed length (tier 1 with its unrolled and generic stages and thread seams, four-step, Bluestein), every input family,
both directions: max_k |got_k - ref_k| <= 4 max(yard_fft, yard_seq) + 8 units per row (fft_cases: the units, the yardsticks and why
4 and 8).  The error is taken over all outputs, so also over the yard_seq indices.
Round trip: ifft(fft(x)) against x within twice that bound in the inverse's unit (2^-53 ||fft x||2 / n = 2^-53 ||x||2 / sqrt(n)); the
yardstick is the largest of both directions' yardsticks on x and of float64 numpy's own round trip.
The first run of these tests found 32 rows over the bound, tones and constants all: the tone of 16382 = 2 x 8191 points (8191 terms of
one phase rounding the same way at every step of the generic stage's plain sum: 1e-13 of the peak), constants of 2^k points (radix 8 as a
plain 8-term sum) and 6720 = 8 8 3 5 7 (odd radices term by term, twiddle ratios rounded over (-1, 1]); itd_fft.hpp's butterflies, its
compensated sum and its octant-folded twiddles are the fix, and those rows are the cases that show it.
Plumbing, bit for bit on device buffers of the test's own (sentinels behind every output): a transform's result does not depend on
where it sits in a batch, on the kMaxGridY split, on the workspace chunks of the four-step and Bluestein forms, on running in place,
on the cached chirp spectrum, or on what the engine ran before.
"""
import ctypes

import numpy as np
import pytest

import fft_cases as fc
from helpers import assert_bits_equal

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not fc.LONGDOUBLE_OK, reason=fc.LONGDOUBLE_WHY)]
SENT = -7.25e300
PAD = 7
TIER_LENGTHS = (1001, 8194, 8209)          # one per tier: generic and unrolled stages; a four-step with a generic stage; Bluestein


def _units_report(n, names, inverse, err, y_fft, y_seq, limit):
    lines = []
    for b, name in enumerate(names):
        lines.append("n=%d %s %s row %d: err %.2f units, yard_fft %.2f, yard_seq %s, bound %.2f%s" % (
            n, name, "inverse" if inverse else "forward", b, err[b], y_fft[b], "-" if y_seq is None else "%.2f" % y_seq[b], limit[b],
            "" if err[b] <= limit[b] else "   <-- EXCEEDS"))
    return lines


@pytest.mark.parametrize("n", fc.LENGTHS)
def test_fft_accuracy(n):
    from pyitd_amd.fourier import debug_fft
    names, x, by_dir = fc.length_case(n)
    report, bad = [], 0
    for inverse in (False, True):
        ref, u, y_fft, y_seq, idx = by_dir[inverse]
        got = debug_fft(x, inverse)
        err = fc.err_units(got, ref, u)
        limit = fc.bound(y_fft, y_seq)
        report += _units_report(n, names, inverse, err, y_fft, y_seq, limit)
        bad += int((~(err <= limit)).sum())
    print("\n".join(report))
    assert bad == 0, "\n" + "\n".join(r for r in report if r.endswith("EXCEEDS"))


@pytest.mark.parametrize("n", fc.LENGTHS)
def test_fft_round_trip(n):
    from pyitd_amd.fourier import debug_fft
    names, x, by_dir = fc.length_case(n)
    got = debug_fft(debug_fft(x, False), True)
    u = fc.EPS * np.linalg.norm(x, axis=1) / np.sqrt(n)
    err = fc.err_units(got, x.astype(np.clongdouble), u)
    yard = fc.err_units(np.fft.ifft(np.fft.fft(x, axis=1), axis=1), x.astype(np.clongdouble), u)
    for inverse in (False, True):
        _, _, y_fft, y_seq, _ = by_dir[inverse]
        yard = np.maximum(yard, y_fft if y_seq is None else np.maximum(y_fft, y_seq))
    limit = 2.0 * (fc.K * yard + fc.F)
    report = ["n=%d %s round trip row %d: err %.2f units, yard %.2f, bound %.2f%s" % (
        n, name, b, err[b], yard[b], limit[b], "" if err[b] <= limit[b] else "   <-- EXCEEDS") for b, name in enumerate(names)]
    print("\n".join(report))
    assert (err <= limit).all(), "\n" + "\n".join(r for r in report if r.endswith("EXCEEDS"))


@pytest.mark.parametrize("n", (8, 64, 4096, 24576))
def test_a_constant_cancels_exactly(n):
    """Radices 2, 4, 8 and 3 cancel equal inputs exactly (sums and differences first; cos 2 pi / 3 = -1/2), as numpy.fft does: a
    constant row of 2^k or 3 * 2^k points leaves exact zeros beside its one output.  (Radix 8 as a plain 8-term sum left an ulp of
    the inputs in every output: 10 to 170 units at 4096 to 2^20 points against a yardstick of exactly 0.)"""
    from pyitd_amd.fourier import debug_fft
    n1 = fc.four_step_split(n) if n > fc.LDS_MAX else 1
    assert set(fc.radices(n1) + fc.radices(n // n1)) <= {2, 3, 4, 8}
    x = np.full((1, n), 0.75 + 0j)
    assert not np.fft.fft(x)[0, 1:].any()
    for inverse in (False, True):
        got = debug_fft(x, inverse)[0]
        assert got[0] == (0.75 * n * (1.0 / n) if inverse else 0.75 * n) and not got[1:].any(), (n, inverse, got[0], np.abs(got[1:]).max())


# ---- plumbing -------------------------------------------------------------------------------------------------------------
def _engine():
    import pyitd_amd
    return pyitd_amd.Engine(4096, 1, 0)


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


def _fft(eng, x, inverse, in_place=False, check_input=True):
    """itd_debug_fft_f64 on the rows x[B, n] in a device buffer of the test's own: [input | output, zeroed | pad], or
    [input = output | pad] in place.  The pad comes back untouched, and so does the input of an out-of-place call."""
    from pyitd_amd.engine import DeviceBuffer
    z = np.ascontiguousarray(np.atleast_2d(x), dtype=np.complex128)
    B, n = z.shape
    out_off = 0 if in_place else z.nbytes
    pad = np.full(2 * PAD, SENT)
    buf = DeviceBuffer(out_off + z.nbytes + pad.nbytes)
    try:
        buf.upload(z)
        if not in_place:
            eng.copy(buf.ptr + out_off, None, z.nbytes, 3, wait=True)
        buf.upload(pad, out_off + z.nbytes)
        rc = eng._L.itd_debug_fft_f64(eng._h, ctypes.c_void_p(buf.ptr), ctypes.c_void_p(buf.ptr + out_off), n, B, 1 if inverse else 0)
        eng._check(rc)
        out = buf.download(np.empty((B, n), np.complex128), out_off)
        assert (buf.download(np.empty(2 * PAD), out_off + z.nbytes) == SENT).all(), "the pad behind the output was written"
        if not in_place and check_input:
            assert np.array_equal(buf.download(np.empty((B, n), np.complex128)).view(np.uint64), z.view(np.uint64)), "the input changed"
    finally:
        buf.free()
    return out


def _same(a, b, what):
    assert_bits_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64), what)


def _rows(n, count, seed=0):
    rng = np.random.default_rng(1009 * n + seed)
    return rng.standard_normal((count, n)) + 1j * rng.standard_normal((count, n))


def _held_to_the_reference(x, got, inverse, what):
    ref, u, y_fft, y_seq, _ = fc.yardsticks(x, inverse)
    err, limit = fc.err_units(got, ref, u), fc.bound(y_fft, y_seq)
    assert (err <= limit).all(), (what, err, y_fft, y_seq, limit)


@pytest.mark.parametrize("n", TIER_LENGTHS)
def test_a_batch_is_its_transforms_one_by_one(eng, n):
    x = _rows(n, 7)
    for inverse in (False, True):
        single = np.concatenate([_fft(eng, x[b], inverse) for b in range(7)])
        for B in (1, 2, 7):
            _same(_fft(eng, x[:B], inverse), single[:B], "n=%d inverse=%d batch of %d" % (n, inverse, B))
            _same(_fft(eng, x[7 - B:], inverse), single[7 - B:], "n=%d inverse=%d the last %d" % (n, inverse, B))


def _tiled(eng, n, B, distinct, inverse, what):
    x = _rows(n, distinct)
    single = np.concatenate([_fft(eng, x[b], inverse) for b in range(distinct)])
    got = _fft(eng, np.tile(x, ((B + distinct - 1) // distinct, 1))[:B], inverse, check_input=False)
    want = np.tile(single, ((B + distinct - 1) // distinct, 1))[:B]
    _same(got, want, what)
    return x, single


@pytest.mark.parametrize("n", (8, 16))
def test_more_transforms_than_one_launch_takes(eng, n):
    for inverse in (False, True):
        x, single = _tiled(eng, n, fc.K_MAX_GRID_Y + 3, 5, inverse, "n=%d inverse=%d, kMaxGridY + 3 transforms" % (n, inverse))
        _held_to_the_reference(x, single, inverse, "n=%d" % n)


def test_four_step_across_its_workspace_chunk(eng):
    n, B = 16384, 1027
    assert fc.path_of(n)[0] == 2 and fc.CHUNK_BYTES // (n * 16) == 1024 < B
    for inverse in (False, True):
        x, single = _tiled(eng, n, B, 5, inverse, "four-step n=%d inverse=%d, %d transforms over chunks of 1024" % (n, inverse, B))
        _held_to_the_reference(x, single, inverse, "four-step n=%d inverse=%d" % (n, inverse))


def test_bluestein_across_its_workspace_chunk(eng):
    n, B = 8209, 515
    assert fc.path_of(n)[0] == 3 and fc.CHUNK_BYTES // (fc.bluestein_m(n) * 16) == 512 < B
    for inverse in (False, True):
        x, single = _tiled(eng, n, B, 5, inverse, "Bluestein n=%d inverse=%d, %d transforms over chunks of 512" % (n, inverse, B))
        _held_to_the_reference(x, single, inverse, "Bluestein n=%d inverse=%d" % (n, inverse))


@pytest.mark.parametrize("n", TIER_LENGTHS)
def test_in_place_is_out_of_place(eng, n):
    x = _rows(n, 3, seed=1)
    for inverse in (False, True):
        _same(_fft(eng, x, inverse, in_place=True), _fft(eng, x, inverse), "n=%d inverse=%d in place" % (n, inverse))


def test_chirp_spectrum_cache_follows_n():
    """8209 and 10007 share M = 32768 and so the chirp buffer; the cache is keyed on n."""
    e = _engine()
    try:
        assert fc.bluestein_m(8209) == fc.bluestein_m(10007)
        xa, xb = _rows(8209, 2, seed=2), _rows(10007, 2, seed=2)
        for inverse in (False, True):
            first, other, third = _fft(e, xa, inverse), _fft(e, xb, inverse), _fft(e, xa, inverse)
            _same(third, first, "n=8209 after n=10007, inverse=%d" % inverse)
            for x, got in ((xa, first), (xb, other), (xa, third)):
                _held_to_the_reference(x, got, inverse, "chirp cache n=%d inverse=%d" % (x.shape[1], inverse))
    finally:
        e.close()


@pytest.mark.parametrize("n", TIER_LENGTHS)
def test_a_direction_does_not_depend_on_the_one_before(n):
    x = _rows(n, 2, seed=3)
    fresh = {}
    for inverse in (False, True):
        e = _engine()
        try:
            fresh[inverse] = _fft(e, x, inverse)
        finally:
            e.close()
    for first in (False, True):
        e = _engine()
        try:
            _fft(e, x, first)
            _same(_fft(e, x, not first), fresh[not first], "n=%d inverse=%d after inverse=%d" % (n, not first, first))
        finally:
            e.close()
