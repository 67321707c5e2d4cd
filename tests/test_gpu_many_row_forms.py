"""The two placements of a many-row call give the same bits: every operator of pyitd_amd.batch and itd_batch on numpy rows (staged
through the C ABI's buffers) and on the same rows as a torch CUDA tensor (used in place), and on a tensor view whose row stride is
not its row length.  n = 1030 is three 512-sample tiles, the last of 6 samples; hop = 512 makes T = 3 time bins.  What each
operator computes is held to its definition elsewhere (test_gpu_instantaneous_batch, _tfe_spectrum, _single_waves, _wave_histogram,
_rows32, _rowsel); here only the forms are compared, and the refusals both must make alike.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LEAD, N, HOP = (2, 3), 1030, 512
EDGES = np.linspace(0.0, 0.5, 9)
AE, LE = np.array([0.0, 0.5, 1.0, 2.0, np.inf]), np.array([1.0, 2.0, 4.0, np.inf])
DTYPES = (np.float64, np.float32)


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def rows_of(dtype):
    return np.random.default_rng(1030).standard_normal(LEAD + (N,)).astype(dtype)


def flat(res):
    """The arrays of a result (an array, a tuple, a dict) in order, tensors brought home."""
    items = [res[k] for k in sorted(res)] if isinstance(res, dict) else list(res) if isinstance(res, tuple) else [res]
    return [a if isinstance(a, np.ndarray) else a.cpu().numpy() for a in items]


def same_bits(got, want, what):
    got, want = flat(got), flat(want)
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, "%s[%d]: %s %s, the numpy form gives %s %s" % (what, k, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), "%s[%d]: the forms differ" % (what, k)


def on_device(res, t):
    for a in (res.values() if isinstance(res, dict) else res if isinstance(res, tuple) else (res,)):
        if not isinstance(a, np.ndarray):
            assert a.device == t.device


OPERATORS = {
    "instantaneous": lambda P, r: P.instantaneous_batch(r),
    "instantaneous-f32-two": lambda P, r: P.instantaneous_batch(r, out_dtype=np.float32, want=("frequency", "amplitude")),
    "spectrum": lambda P, r: P.tfe_spectrum(r, EDGES, HOP),
    "spectrum-count": lambda P, r: P.tfe_spectrum(r, EDGES, HOP, weight="count"),
    "waves-counted": lambda P, r: P.single_waves(r),
    "waves-cap": lambda P, r: P.single_waves(r, cap=600),
    "filter": lambda P, r: P.wave_filter(r, amplitude=(0.5, 2.0), length=(2, 40)),
    "filter-f32-per-row": lambda P, r: P.wave_filter(r, amplitude=(np.linspace(0.0, 1.0, r.shape[0])[:, None], 2.5), out_dtype=np.float32),
    "histogram": lambda P, r: P.wave_histogram(r, AE, LE, hop=HOP),
    "histogram-one-bin": lambda P, r: P.wave_histogram(r, AE, LE),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(OPERATORS))
def test_an_operator_gives_the_same_bits_on_numpy_rows_and_on_a_tensor(P, torch, case, dtype):
    rows = rows_of(dtype)
    t = torch.from_numpy(rows).cuda()
    want = OPERATORS[case](P, rows)
    got = OPERATORS[case](P, t)
    on_device(got, t)
    same_bits(got, want, case)
    view = t[:, 1:2, :]                                         # [2, 1, N]: rows 3 N apart
    assert view.stride(0) == 3 * N and not view.is_contiguous()
    got = OPERATORS[case](P, view)
    on_device(got, t)
    same_bits(got, OPERATORS[case](P, rows[:, 1:2, :]), case + " on a strided view")


DECOMPOSITIONS = {
    "plain": {},
    "float32-rows": {"out_dtype": np.float32},
    "selected": {"select": (0, 2, -1)},
    "baselines": {"keep_baselines": True},
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(DECOMPOSITIONS))
def test_itd_batch_gives_the_same_bits_on_numpy_rows_and_on_a_tensor(P, torch, case, dtype):
    x = rows_of(dtype)[0]                                       # B = 3
    t = torch.from_numpy(x).cuda()
    want = P.itd_batch(x, max_iteration=3, **DECOMPOSITIONS[case])
    got = P.itd_batch(t, max_iteration=3, **DECOMPOSITIONS[case])
    assert sorted(got) == sorted(want) and got["rows"].device == t.device
    for k in ("n_rows", "stop", "knot_counts") + (("n_baselines",) if case == "baselines" else ()):
        same_bits(got[k], want[k], "%s %s" % (case, k))
    assert got["rows"].shape == want["rows"].shape == (3, 3 if case == "selected" else 5, N)
    if case == "selected":                                      # every slot is specified: absent rotations are zero
        same_bits(got["rows"], want["rows"], case + " rows")
    for b in range(3):                                          # (beyond n_rows and n_baselines a row is unspecified)
        if case != "selected":
            same_bits(got["rows"][b, :want["n_rows"][b]], want["rows"][b, :want["n_rows"][b]], "%s rows of signal %d" % (case, b))
        if case == "baselines":
            m = want["n_baselines"][b]
            same_bits(got["baselines"][b, :m], want["baselines"][b, :m], "%s baselines of signal %d" % (case, b))
            assert not got["baselines"][b, m:].cpu().numpy().any()              # a tensor's stay zero beyond n_baselines


def refusal(exc, call):
    with pytest.raises(exc) as e:
        call()
    return str(e.value)


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_forms_refuse_a_nan_row_and_a_small_cap_alike(P, torch, dtype):
    rows = rows_of(dtype)
    rows[1, 2, 700] = np.nan                                    # row 5 of 6
    t = torch.from_numpy(rows).cuda()
    for case in sorted(OPERATORS):
        said = refusal(P.ITDError, lambda: OPERATORS[case](P, rows))
        assert "NaN in rows [5]" in said, (case, said)
        assert refusal(P.ITDError, lambda: OPERATORS[case](P, t)) == said, case
    rows = rows_of(dtype)
    t = torch.from_numpy(rows).cuda()
    count = P.single_waves(rows).count
    cap = int(count.max()) - 1
    said = refusal(ValueError, lambda: P.single_waves(rows, cap=cap))
    over = np.flatnonzero(count.ravel() > cap).tolist()
    assert said == "cap = %d is less than the half waves of rows %s (up to %d)" % (cap, over, cap + 1)
    assert refusal(ValueError, lambda: P.single_waves(t, cap=cap)) == said
