"""The ITD-Fourier cascade on the GPU (pyitd_amd/fourier.py; itd_fft.hpp, itd_fourier.inc) against numpy and the reference's goldens
(tests/golden/fourier/, tools/gen_fourier_golden.py):
  itd_debug_fft_f64            numpy.fft.fft / ifft for n = 1..128, primes, 8192 / 8193, a four-step and a Bluestein length
  the selectors                the goldens' decisions exactly, the float64 restatement to 1e-11, the reference's modes to 1e-6 of scale
  the cascades                 every golden case: outputs, iteration count, per-mode records, values to 1e-6 of scale
  *_batch                      64 signals, bit for bit the single calls; max_rounds; IndexError; NaN
"""
import numpy as np
import pytest

from test_fourier_cpu import cascade_cases, restate, selector_cases, FOURIER

pytestmark = pytest.mark.gpu

FFT_NS = list(range(1, 129)) + [251, 1009, 4099, 8191, 8192, 8193, 3 * 5 * 7 * 11 * 13 * 16, 65537]


@pytest.mark.parametrize("n", FFT_NS)
def test_fft_matches_numpy(n):
    from pyitd_amd.fourier import debug_fft
    rng = np.random.default_rng(n)
    x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
    for inverse, ref in ((False, np.fft.fft(x)), (True, np.fft.ifft(x))):
        got = debug_fft(x, inverse)
        err = np.max(np.abs(got - ref), axis=1)
        assert (err <= 1e-12 * np.linalg.norm(x, axis=1)).all(), (n, inverse, err)


@pytest.mark.parametrize("case", selector_cases(), ids=lambda c: c[0])
def test_selectors_against_the_goldens(case):
    from pyitd_amd.fourier import fourier_mode_batch
    name, rule, x, rec, mode_ref = case
    modes, recs = fourier_mode_batch(x[None, :], rule)
    assert np.array_equal(recs[0], rec), (name, recs[0], rec)
    scale = max(np.max(np.abs(x)), 1e-300)
    _, mode64 = restate(x, rule)
    assert np.max(np.abs(modes[0] - mode64)) <= 1e-11 * scale
    assert np.max(np.abs(modes[0] - mode_ref)) <= 1e-6 * scale


def test_single_row_selectors_are_the_batched_ones():
    import pyitd_amd
    from pyitd_amd.fourier import fourier_mode_batch
    x = np.stack([c[2] for c in selector_cases() if c[2].shape[0] == 1001][:1] * 2)
    for rule, fn in (("any", pyitd_amd.fourier_mode_decomposition_any), ("valid", pyitd_amd.fourier_mode_decomposition_valid)):
        modes, _ = fourier_mode_batch(x, rule)
        assert np.array_equal(fn(x[0]), modes[0])


def _load(name):
    z = np.load("%s/cascade_%s.npz" % (FOURIER, name))
    return z["x"], int(z["sample_rate"]), z


@pytest.mark.parametrize("name", cascade_cases())
def test_cascades_against_the_reference(name):
    import pyitd_amd
    x, sr, z = _load(name)
    scale = np.max(np.abs(x))
    full, recs = z["full"].astype(np.float64), z["records"]
    lean, j = [], 0          # the lean output: each row's modes summed in the order found, then the row (as the generator asserts)
    for i in range(len(full) - len(recs) - 1):
        k = int((recs[:, 1] == i).sum())
        lean += [full[j:j + k].sum(axis=0) if k else np.zeros_like(x), full[j + k]]
        j += k + 1
    lean.append(full[-1])
    for fn, key, ref in ((pyitd_amd.itd_fourier_decomposition, "full", full), (pyitd_amd.itd_fourier_decomposition_lean, "lean", np.stack(lean))):
        out, info = fn(x, sr, return_info=True)
        assert len(out) == ref.shape[0], (key, len(out), ref.shape[0])
        assert info["rounds"] == int(z["iterations"]) and not info["capped"]
        assert np.array_equal(info["records"], z["records"]), key
        err = max(float(np.max(np.abs(o - r))) for o, r in zip(out, ref))
        assert err <= 1e-6 * scale, (key, err)


def test_long_signals_are_covered():
    assert any(_load(name)[0].shape[0] > 8192 for name in cascade_cases())


def _batch_signals():
    rng = np.random.default_rng(5)
    t = np.arange(2000) / 421.0          # (a length and rate for which no band's last knot lies beyond the signal)
    xs = []
    for b in range(64):
        f1, f2 = rng.uniform(20, 90), rng.uniform(100, 200)
        xs.append((1 + rng.uniform(0, 0.6) * np.sin(2 * np.pi * rng.uniform(1, 5) * t)) * np.sin(2 * np.pi * f1 * t) +
                  rng.uniform(0.2, 0.8) * np.sin(2 * np.pi * f2 * t) + 0.1 * rng.standard_normal(t.size))
    return np.stack(xs), 421


def test_batch_is_the_single_calls_bit_for_bit():
    import pyitd_amd
    xs, sr = _batch_signals()
    for lean in (False, True):
        outs, infos = pyitd_amd.itd_fourier_decomposition_batch(xs, sr, lean=lean, return_info=True)
        assert len({i["rounds"] for i in infos}) > 1            # signals that finish after different iteration counts
        single = pyitd_amd.itd_fourier_decomposition_lean if lean else pyitd_amd.itd_fourier_decomposition
        for b in range(xs.shape[0]):
            out, info = single(xs[b], sr, return_info=True)
            assert len(out) == len(outs[b]) and info["rounds"] == infos[b]["rounds"]
            assert np.array_equal(info["records"], infos[b]["records"])
            for o, p in zip(out, outs[b]):
                assert np.array_equal(o.view(np.uint64), p.view(np.uint64))


def test_max_rounds_cap_is_reported():
    import pyitd_amd
    xs, sr = _batch_signals()
    free = pyitd_amd.itd_fourier_decomposition_batch(xs[:8], sr, return_info=True)[1]
    b = int(np.argmax([i["rounds"] for i in free]))
    assert free[b]["rounds"] >= 2
    out, info = pyitd_amd.itd_fourier_decomposition(xs[b], sr, max_rounds=1, return_info=True)
    assert info["capped"] and info["rounds"] == 1
    assert np.max(np.abs(np.sum(out, axis=0) - xs[b])) <= 1e-9 * np.max(np.abs(xs[b]))


def test_index_error_where_the_sine_wrapper_raises_it():
    import pyitd_amd
    rng = np.random.default_rng(1)
    seen = 0
    for n, sr in ((1000, 999), (1001, 1000), (1234, 1100), (997, 800), (1500, 1001)):
        x = rng.standard_normal(n)
        try:
            pyitd_amd.itd_sine_wrapper(x, sr)
        except IndexError:
            seen += 1
            with pytest.raises(IndexError):
                pyitd_amd.itd_fourier_decomposition(x, sr)
    assert seen >= 1


def test_nan_input_is_refused():
    import pyitd_amd
    xs, sr = _batch_signals()
    x = xs[0].copy()
    x[700] = np.nan
    with pytest.raises(ValueError):
        pyitd_amd.itd_fourier_decomposition(x, sr)


def test_cascade_leaves_a_pending_itd_baselines_fetch_alone():
    """ITD().itd() leaves its baselines on the shared engine for a lazy fetch; a cascade on the same engine in between (both forms)
    must not change what that fetch returns."""
    import pyitd_amd
    xs, sr = _batch_signals()
    x = xs[3]
    eager = pyitd_amd.ITD()
    eager.itd(x, max_iteration=5)
    want = np.array(eager.get_baselines(), copy=True)
    for fn in (pyitd_amd.itd_fourier_decomposition_lean, pyitd_amd.itd_fourier_decomposition):
        it = pyitd_amd.ITD()
        it.itd(x, max_iteration=5)
        fn(xs[7], sr)
        assert np.array_equal(np.asarray(it.baselines).view(np.uint64), want.view(np.uint64)), fn.__name__
