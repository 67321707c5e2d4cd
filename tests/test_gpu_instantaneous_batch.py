"""The batched instantaneous step (itd_instantaneous_batch_f64 / _f32, pyitd_amd.instantaneous_batch; itd_tfe_batch.hpp) against
the single-row operator (bit for bit: the same expressions on the same operands) and, independently of it, against the exact
results of oracle/exact_tfe.py with test_gpu_instantaneous_exact.py's bounds: amplitude bit for bit, phase within 4 ulp(2 pi) of
the exact value, frequency within 8 ulp(2 pi) / 2 pi of it — at every length of that file's LENGTHS too.

Where the kernels can go wrong: a half wave inside one 64-sample step, across steps of a tile, across tiles (the tile records and
their scan along the row), across the scan's chunks — k_inst_carry takes K = 2048 records (2^20 samples) per pass on rows of more
than 512 tiles, the forward pass counted from the row's first tile and the backward pass from its last; the row of
(2 K + 1) * 512 + 5 samples below was written for that K, the rows of 512, 513 and 514 tiles for the seam between
k_inst_carry<64> and k_inst_carry<256> — the row's last sample in a tile of its own, strides, output subsets,
float32 rows in and out, NaN rows, more rows than one launch's grid takes, a caller's stream and a captured graph.
The file also passes with PYITD_POISON=1.
"""
import itertools

import numpy as np
import pytest

from helpers import DevArrays
from oracle import exact_tfe as et
from test_gpu_instantaneous_exact import LENGTHS, _bits, check
from test_gpu_tfe import numpy_tfe
from test_oracle_exact_tfe import FAMILIES, family, with_crossings

pytestmark = pytest.mark.gpu
SENT = -7.25e300
NAMES = ("a", "p", "f")
CARRY_K = 2048                  # records per pass of k_inst_carry<256> (kInstCarryChunk)


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


@pytest.fixture
def eng(P):
    from pyitd_amd.itd import _engine_for
    return _engine_for(8192)            # (the cached single-signal engine: nothing in this file outgrows it)


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    assert np.array_equal(a.view(u), b.view(u)), what


def run_dev(eng, rows, mask=(1, 1, 1), row_stride=None, out_stride=None):
    """The C entry on device buffers with the strides asked for: the input's gaps hold 1e308, the outputs (all three exist) are
    filled with SENT.  Returns ({name: [R, out_stride] as left behind}, info, the input [R, row_stride] as left behind)."""
    R, n = rows.shape
    rs = n if row_stride is None else row_stride
    os_ = n if out_stride is None else out_stride
    xin = np.full((R, rs), 1e308, rows.dtype)
    xin[:, :n] = rows
    sent = np.full((R, os_), SENT)
    d = DevArrays(eng, x=xin, a=sent, p=sent, f=sent, info=np.full(R, -77, np.int32))
    try:
        ptrs = [d.ptr(k) if on else None for k, on in zip(NAMES, mask)]
        eng.instantaneous_batch_dev(d.ptr("x"), rows.dtype, n, R, rs, *ptrs, os_, False, d.ptr("info"))
        return {k: d.get(k) for k in NAMES}, d.get("info"), d.get("x")
    finally:
        d.free()


# ---- 1. bit identity with the single-row operator --------------------------------------------------------------------------
def test_bit_identical_to_the_single_row_operator_at_every_seam_length(P):
    for n in LENGTHS:
        rows = np.stack([family(fam, n) for fam in ("seams", "quantised", "noise")])
        a, p, f = P.instantaneous_batch(rows)
        for r in range(3):
            ra, rp, rf = P.instantaneous(rows[r])
            _bits(a[r], ra, "n=%d row %d amplitude" % (n, r))
            _bits(p[r], rp, "n=%d row %d phase" % (n, r))
            _bits(f[r], rf, "n=%d row %d frequency" % (n, r))


# ---- 2. the exact reference, independently of the old kernels --------------------------------------------------------------
@pytest.mark.parametrize("n", (3, 5, 64, 65, 1025, 2 * 512 + 514, 20011))
def test_signal_families_against_the_exact_reference(P, n):
    rows = np.stack([family(fam, n) for fam in FAMILIES])
    a, p, f = P.instantaneous_batch(rows)
    for r, fam in enumerate(FAMILIES):
        check(rows[r], a[r], p[r], f[r], what="%s n=%d" % (fam, n))


def test_every_length_near_the_step_and_tile_seams_against_the_exact_reference(P):
    fams = ("seams", "quantised")
    for n in LENGTHS:
        rows = np.stack([family(fam, n) for fam in fams])
        a, p, f = P.instantaneous_batch(rows)
        for r, fam in enumerate(fams):
            check(rows[r], a[r], p[r], f[r], what="%s n=%d" % (fam, n))


# ---- 3. half waves across many tiles and across the carry's chunk seams ------------------------------------------------------
def test_half_waves_of_many_tiles(P):
    n = 60000
    x = family("slow", n)
    c = np.flatnonzero(et.structure(x)[0])
    assert c.size == 17 and np.diff(c).min() >= 1649
    a, p, f = P.instantaneous_batch(x[None, :])
    check(x, a[0], p[0], f[0], what="slow")


def _check_long(x, a, p, f, what):
    _bits(a, et.structure(x)[2], "%s: the whole amplitude row" % what)
    check(x, a, p, f, samples=et.sample_subset(x.size, x), what=what)


def test_half_waves_over_hundreds_of_tiles(P):
    n = (1 << 18) + 3
    pos = family("positive", n)
    one = pos.copy()
    one[n // 2:] *= -1.0
    assert np.count_nonzero(et.structure(pos)[0]) == 0 and np.count_nonzero(et.structure(one)[0]) == 1
    seams = sorted(512 * k + d for k in (1, 2, 200, 511, 512) for d in (-1, 0, 1))
    at_seams = with_crossings(n, seams, np.random.default_rng(3))
    assert np.flatnonzero(et.structure(at_seams)[0]).tolist() == seams
    rows = np.stack([pos, one, at_seams])
    a, p, f = P.instantaneous_batch(rows)
    for r, what in enumerate(("one half wave over 513 tiles", "one crossing", "crossings at tile seams only")):
        _check_long(rows[r], a[r], p[r], f[r], what)


def test_half_waves_across_the_carry_chunks(P):
    """Rows of (2 K + 1) * 512 + 5 samples with a single crossing: the first half wave's maximum is the row's second sample, the
    second one's the row's last, so each crosses chunk seams of the forward or the backward pass on its way to the other's end."""
    n = (2 * CARRY_K + 1) * 512 + 5
    rng = np.random.default_rng(17)
    rows = []
    for tile in (100, 2 * CARRY_K - 90):
        x = with_crossings(n, [tile * 512 + 300], rng, mag=0.1 + 0.5 * rng.random(n))
        x[1] = 0.9375
        x[-1] = np.sign(x[-1]) * 0.96875
        assert np.count_nonzero(et.structure(x)[0]) == 1
        rows.append(x)
    rows = np.stack(rows)
    a, p, f = P.instantaneous_batch(rows)
    for r in range(2):
        assert a[r, 0] == 0.9375 and a[r, -1] == 0.96875
        _check_long(rows[r], a[r], p[r], f[r], "single crossing, row %d" % r)


@pytest.mark.parametrize("tiles", (512, 513, 514))
def test_one_row_across_the_carry_instantiations(P, tiles):
    """Rows of (tiles - 1) * 512 + 5 samples with a single crossing and the two maxima at the row's second and last sample, as
    above, through the single-row call and through the batched call of one row: 512 tiles is the longest such row that
    k_inst_carry<64> takes (one pass of one wavefront, every thread's eight records in use), 513 and 514 tiles are the shortest
    that go to k_inst_carry<256>."""
    n = (tiles - 1) * 512 + 5
    rng = np.random.default_rng(tiles)
    x = with_crossings(n, [100 * 512 + 300], rng, mag=0.1 + 0.5 * rng.random(n))
    x[1] = 0.9375
    x[-1] = np.sign(x[-1]) * 0.96875
    assert np.count_nonzero(et.structure(x)[0]) == 1
    a, p, f = P.instantaneous(x)
    assert a[0] == 0.9375 and a[-1] == 0.96875
    _check_long(x, a, p, f, "single crossing, %d tiles" % tiles)
    for got, want, what in zip(P.instantaneous_batch(x[None, :]), (a, p, f), NAMES):
        _bits(got[0], want, "%d tiles, batched: %s" % (tiles, what))


# ---- 4. strides and confinement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (5 * 512 + 77, 515))
def test_strides_and_every_subset_of_outputs(eng, n):
    rows = np.stack([family(fam, n) for fam in ("noise", "seams", "quantised")])
    dense, dinfo, _ = run_dev(eng, rows)
    for r in range(3):
        check(rows[r], dense["a"][r], dense["p"][r], dense["f"][r], what="dense row %d" % r)
    for mask in itertools.product((0, 1), repeat=3):
        if not any(mask):
            continue
        got, info, xin = run_dev(eng, rows, mask, n + 13, n + 7)
        assert np.array_equal(info, dinfo)
        _same(xin[:, :n], rows, "the input is left alone")
        assert np.all(xin[:, n:] == 1e308)
        for k, on in zip(NAMES, mask):
            assert np.all(got[k][:, n:] == SENT), "%s: the gap behind %s is written" % (mask, k)
            if on:
                _same(got[k][:, :n], dense[k], "%s: %s = the dense call's" % (mask, k))
            else:
                assert np.all(got[k] == SENT), "%s: %s was not asked for" % (mask, k)


# ---- 5. types --------------------------------------------------------------------------------------------------------------
def test_float32_rows_in_and_out(P):
    for n in (1025, 2 * 512 + 514):
        rows32 = np.stack([family(fam, n) for fam in ("seams", "quantised", "noise", "slow", "negzero")]).astype(np.float32)
        ref = P.instantaneous_batch(rows32.astype(np.float64))
        got = P.instantaneous_batch(rows32)
        both = P.instantaneous_batch(rows32, out_dtype=np.float32)
        for k in range(3):
            assert got[k].dtype == np.float64 and both[k].dtype == np.float32
            _same(got[k], ref[k], "float32 in, output %d" % k)
            _same(both[k], ref[k].astype(np.float32), "float32 in and out, output %d" % k)
        rows = np.stack([family(fam, n) for fam in FAMILIES])          # "subnormal" and "huge" among them
        ref = P.instantaneous_batch(rows)
        got = P.instantaneous_batch(rows, out_dtype=np.float32)
        with np.errstate(over="ignore", under="ignore"):
            want = [r.astype(np.float32) for r in ref]
        sub, huge = FAMILIES.index("subnormal"), FAMILIES.index("huge")
        assert np.all(want[0][sub] == 0) and np.any(np.isinf(want[0][huge]))
        for k in range(3):
            _same(got[k], want[k], "float32 out, output %d" % k)


# ---- 6. info_dev -----------------------------------------------------------------------------------------------------------
def test_info_counts_the_crossings(eng):
    for n in (1025, 2 * 512 + 514):
        rows = np.stack([family(fam, n) for fam in FAMILIES])
        _, info, _ = run_dev(eng, rows, (0, 0, 1))
        assert info.tolist() == [int(np.count_nonzero(et.structure(x)[0])) for x in rows]


@pytest.mark.parametrize("where", ("first", "seam", "last"))
def test_rows_with_a_nan(P, eng, where):
    n = 3 * 512 + 5
    rows = np.stack([family(fam, n) for fam in ("noise", "seams", "quantised", "noise", "slow")])
    rows[3] = rows[3][::-1]
    clean, cinfo, _ = run_dev(eng, rows[[0, 2, 4]])
    bad = rows.copy()
    at = {"first": 0, "seam": 512, "last": n - 1}[where]
    bad[1, at] = np.nan
    bad[3, at - 1 if where == "seam" else at] = np.nan
    got, info, xin = run_dev(eng, bad, (1, 1, 1), n + 13, n + 7)
    with np.errstate(invalid="ignore"):
        counts = [int(np.count_nonzero(et.structure(x)[0])) for x in bad]
    assert info.tolist() == [counts[0], -1 - counts[1], counts[2], -1 - counts[3], counts[4]]
    assert np.array_equal(info[[0, 2, 4]], cinfo)
    for k in NAMES:
        assert np.all(got[k][:, n:] == SENT), "the gap behind %s is written" % k
        _same(got[k][[0, 2, 4], :n], clean[k], "%s of the rows without a NaN" % k)
    with pytest.raises(P.ITDError, match=r"NaN in rows \[1, 3\]"):
        P.instantaneous_batch(bad)


# ---- 7. more rows than one launch takes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (5, 67))
def test_more_rows_than_one_grid(P, n):
    """65 539 rows: 1024 different ones, repeated (row r is base row r % 1024, so the rows on both sides of the chunk seam at
    65 535 differ), against test_gpu_tfe's numpy statement with that file's bound."""
    R = 65539
    base = np.random.default_rng(n).standard_normal((1024, n))
    ref = [np.stack(v) for v in zip(*(numpy_tfe(x) for x in base))]
    idx = np.arange(R) % 1024
    a, p, f = P.instantaneous_batch(base[idx])
    assert np.array_equal(a, ref[0][idx])
    assert np.max(np.abs(p - ref[1][idx])) < 1e-12 and np.max(np.abs(f - ref[2][idx])) < 1e-12


# ---- 8. the caller's stream and a captured graph -----------------------------------------------------------------------------
def test_on_a_callers_stream_and_in_a_graph(P, eng):
    import torch
    n, R = 5 * 512 + 77, 4
    fams = ("noise", "seams", "quantised", "slow")
    x_old = np.stack([family(f, n)[::-1] for f in fams])
    x_new = np.stack([family(f, n) for f in fams])
    want = P.instantaneous_batch(x_new)
    sent = np.full((R, n), SENT)
    d = DevArrays(eng, x=x_old, stage=x_new, a=sent, p=sent, f=sent, info=np.zeros(R, np.int32))
    s = torch.cuda.Stream()
    eng.copy(d.ptr("x"), d.ptr("stage"), x_new.nbytes, 2, wait=False, stream=s.cuda_stream)
    eng.instantaneous_batch_dev(d.ptr("x"), np.float64, n, R, n, d.ptr("a"), d.ptr("p"), d.ptr("f"), n, False, d.ptr("info"), s.cuda_stream)
    s.synchronize()
    for k, w in zip(NAMES, want):
        _bits(d.get(k), w, "on the caller's stream: %s" % k)
    # (the call above was the warm-up of this size: the workspace exists, the capture allocates nothing)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng.instantaneous_batch_dev(d.ptr("x"), np.float64, n, R, n, d.ptr("a"), d.ptr("p"), d.ptr("f"), n, False, d.ptr("info"),
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for y in (x_old, np.stack([family(f, n) for f in ("quantised", "noise", "slow", "seams")])):
        eager = P.instantaneous_batch(y)
        d.put("x", y)
        for k in NAMES:
            d.put(k, sent)
        g.replay()
        torch.cuda.synchronize()
        for k, w in zip(NAMES, eager):
            _bits(d.get(k), w, "replayed: %s" % k)
        assert d.get("info").tolist() == [int(np.count_nonzero(et.structure(r)[0])) for r in y]
    d.free()


def test_a_captured_graph_survives_a_larger_single_row_call(P, eng):
    """The batched call's workspace is its own: a single-row call of 8192 samples on the same engine, after the 2 x 1030 call was
    captured, leaves the captured launches' addresses valid, and the replay equals the uncaptured call bit for bit."""
    import torch
    n, R, big = 1030, 2, 8192
    rows = np.stack([family(f, n) for f in ("seams", "noise")])
    sent = np.full((R, n), SENT)
    d = DevArrays(eng, x=rows, a=sent, p=sent, f=sent, info=np.zeros(R, np.int32),
                  y=family("noise", big), ya=np.zeros(big), yp=np.zeros(big), yf=np.zeros(big))
    args = (d.ptr("x"), np.float64, n, R, n, d.ptr("a"), d.ptr("p"), d.ptr("f"), n, False, d.ptr("info"))
    s = torch.cuda.Stream()
    eng.instantaneous_batch_dev(*args, s.cuda_stream)           # (the warm-up of this size: the capture allocates nothing)
    s.synchronize()
    want = {k: d.get(k) for k in NAMES}
    for r in range(R):
        check(rows[r], want["a"][r], want["p"][r], want["f"][r], what="uncaptured row %d" % r)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng.instantaneous_batch_dev(*args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rc = eng._L.itd_instantaneous_f64(eng._h, d.ptr("y"), big, d.ptr("ya"), d.ptr("yp"), d.ptr("yf"), None)
    assert rc == 0, rc
    for k in NAMES:
        d.put(k, sent)
    g.replay()
    torch.cuda.synchronize()
    for k in NAMES:
        _bits(d.get(k), want[k], "replayed behind the single-row call: %s" % k)
    d.free()


# ---- 10. the torch-tensor path -------------------------------------------------------------------------------------------
def test_rows_of_a_batched_decomposition_as_a_tensor(P):
    import torch
    B, n, m = 3, 4099, 3
    x = np.stack([family("noise", n) + 3.0 * family("slow", n) * (b + 1) for b in range(B)])
    res = P.itd_batch(torch.from_numpy(x).cuda(), max_iteration=m, out_dtype=torch.float32)
    rows = res["rows"]
    assert res["n_rows"].tolist() == [m + 2] * B                    # (every row is written: no NaN left over from torch.empty)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (B, m + 2, n)
    a, p, f = P.instantaneous_batch(rows)
    assert a.device == rows.device and a.dtype == torch.float64 and tuple(a.shape) == (B, m + 2, n)
    host = rows.cpu().numpy().astype(np.float64)
    for b in range(B):
        for r in range(int(res["n_rows"][b])):
            ra, rp, rf = P.instantaneous(host[b, r])
            _bits(a[b, r].cpu().numpy(), ra, "amplitude of signal %d row %d" % (b, r))
            _bits(p[b, r].cpu().numpy(), rp, "phase of signal %d row %d" % (b, r))
            _bits(f[b, r].cpu().numpy(), rf, "frequency of signal %d row %d" % (b, r))
    (a2,) = P.instantaneous_batch(rows[:, 1:2, :], want=("amplitude",), out_dtype=torch.float32)     # row stride (m + 2) n
    assert a2.dtype == torch.float32 and torch.equal(a2, a[:, 1:2, :].float())
    for view in (rows[:, 1:3, :], rows[:, :, ::2]):                 # no one row stride; a strided last axis
        with pytest.raises(ValueError):
            P.instantaneous_batch(view)
