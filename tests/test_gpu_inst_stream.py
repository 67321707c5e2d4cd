"""The instantaneous stream on the GPU (itd_inst_stream_*, pyitd_amd.streaming.InstantaneousStream) — everything bit for bit: the
float64 outputs as uint64 patterns (the NaN pattern 0x7FF8000000000000 included), lengths and counts exactly.

1. Composition: the stream's outputs equal instantaneous_batch of the concatenated rows where the masks from the half waves of
   tests/waves_ref.py deliver them and the NaN pattern elsewhere; length and both counts equal tests/inst_stream_ref.py.
2. With a horizon that holds every half wave: instantaneous_batch without a NaN, single_waves' lengths repeated, counts zero.
3. Independently of the device's own operator: against oracle/exact_tfe.py, by test_gpu_instantaneous_exact.check.
4. The same bits in any batch position and from run to run; 70 rows in one stream.
5. Device forms: every subset of the outputs, strides, padding, guards, NULL counts, nothing written by a push that does not emit,
   a caller's stream.
6. Stream state: flush order, restart, refusals, reset, blocks, a NaN row.
7. Behind a LevelsStream on device pointers.
8. blockwise_instantaneous.
The file also passes with PYITD_POISON=1.
"""
import itertools

import numpy as np
import pytest

import inst_stream_ref as isr
import spectrum_stream_ref as ssr
from helpers import fuzz_signal
from ring_stream_runs import enveloped_signals as signals, latency, push_and_flush

pytestmark = pytest.mark.gpu
SENT = -7.25e300
ISENT = -777
NAMES = ("amplitude", "phase", "frequency", "length", "long", "overlong")
ALL = NAMES[:4]


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


@pytest.fixture(scope="module")
def S():
    from pyitd_amd import streaming
    return streaming


def same(got, want, what, names=NAMES):
    assert len(got) == len(want) == len(names)
    for g, w, name in zip(got, want, names):
        if w is None:
            assert g is None, "%s: %s was not asked for" % (what, name)
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, "%s %s: %s %s vs %s %s" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        gb, wb = (g.view(np.uint64), w.view(np.uint64)) if g.dtype == np.float64 else (g, w)
        bad = np.flatnonzero(gb.ravel() != wb.ravel())
        assert bad.size == 0, "%s: %d of %d %s values differ, first at %d: %r vs %r" % (what, bad.size, g.size, name, bad[0], g.ravel()[bad[0]],
                                                                                     w.ravel()[bad[0]])


def expected(P, x, L, H):
    """(amplitude, phase, frequency, length [R, n], long, overlong [R, n / L]) and the two masks [R, n]: the floats are
    instantaneous_batch's where the masks of the numpy statement deliver them, length and counts are the numpy statement's"""
    a, p, f = P.instantaneous_batch(x, want=("amplitude", "phase", "frequency"))
    ref = [isr.whole_row_features(r, H) for r in x]
    ln, long_, ovl = (np.stack([v[i] for v in ref]) for i in (3, 4, 5))
    R = x.shape[0]
    cnt = lambda m: m.reshape(R, -1, L).sum(axis=2).astype(np.int32)
    return (np.where(long_, isr.NONE, a), np.where(long_, isr.NONE, p), np.where(ovl, isr.NONE, f), ln, cnt(long_), cnt(ovl)), long_, ovl


def run_stream(st, x):
    """push every block, flush until empty: the six fields (per-sample ones [R, n], counts [R, blocks]; None where not wanted), the
    pushes' emission pattern, the flushes that emitted"""
    outs, pattern, flushed = push_and_flush(st, x)
    got = [None if outs[0][i] is None else np.concatenate([o[i] for o in outs], axis=1) for i in range(4)]
    got += [np.stack([o[i] for o in outs], axis=1) for i in (4, 5)]
    return tuple(got), pattern, flushed


def composition(P, S, L, H, counts_of_blocks):
    D = latency(L, H)
    rng = np.random.default_rng(L * 1013 + H)
    st = S.InstantaneousStream(L, 3, H, want=ALL)
    assert st.latency == D and (st.block, st.rows, st.horizon) == (L, 3, H)
    seen = np.zeros(3, np.int64)
    for blocks in counts_of_blocks:                                       # (one stream: it starts afresh after its flush)
        x = signals(rng, L, H, 3, blocks)
        want, long_, ovl = expected(P, x, L, H)
        got, pattern, flushed = run_stream(st, x)
        what = "L=%d H=%d blocks=%d" % (L, H, blocks)
        assert pattern == [p >= D for p in range(blocks)] and flushed == min(blocks, D), what
        same(got, want, what)
        seen += (int((~ovl).sum()), int((ovl & ~long_).sum()), int(long_.sum()))
    assert (seen > 0).all(), "delivered, overlong but not long, long: %s" % (seen,)
    assert st.status() == 0
    st.close()


# ---- 1. composition, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hk", ("1", "L-1", "L", "L+1", "2L"))
@pytest.mark.parametrize("L", (8, 64, 100, 512))
def test_composition_of_the_instantaneous_outputs(P, S, L, hk):
    H = {"1": 1, "L-1": L - 1, "L": L, "L+1": L + 1, "2L": 2 * L}[hk]
    composition(P, S, L, H, range(1, 2 * latency(L, H) + 4))


@pytest.mark.parametrize("hk", ("L", "L+1"))
def test_composition_at_a_ragged_block_above_2048(P, S, hk):
    """2100 = 32 x 64 + 52: the 512-thread instance, its last 64-sample step ragged"""
    L = 2100
    H = {"L": L, "L+1": L + 1}[hk]
    D = latency(L, H)
    composition(P, S, L, H, (1, D, D + 1, 2 * D + 3))


# ---- 2. equality with the whole-row calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (64, 100, 1024))
def test_with_a_horizon_that_holds_every_half_wave_it_is_instantaneous_batch(P, S, L):
    from waves_ref import ref_table
    rng = np.random.default_rng(L + 24)
    blocks = 7
    x = np.stack([fuzz_signal(rng, k, blocks * L) for k in (0, 4, 6)])
    H = int(max(ref_table(r)[1].max() for r in x))                       # exactly the longest half wave
    st = S.InstantaneousStream(L, 3, H, want=ALL)
    got, _, _ = run_stream(st, x)
    st.close()
    a, p, f = P.instantaneous_batch(x, want=("amplitude", "phase", "frequency"))
    w = P.single_waves(x)
    ln = np.stack([np.repeat(w.length[r, :w.count[r]], w.length[r, :w.count[r]]) for r in range(3)]).astype(np.int32)
    zero = np.zeros((3, blocks), np.int32)
    same(got, (a, p, f, ln, zero, zero), "L=%d H=%d" % (L, H))
    assert not np.isnan(a).any() and not np.isnan(p).any() and not np.isnan(f).any() and ln.max() == H


# ---- 3. against the exact reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ("noise", "quantised"))
def test_against_the_exact_reference(S, fam):
    """The long and overlong masks from the half waves of oracle/exact_tfe.py; at the samples that are not overlong amplitude, phase
    and frequency within test_gpu_instantaneous_exact's bounds of the exact values (amplitude bit for bit, PH_TOL, F_TOL)."""
    from oracle import exact_tfe as et
    from test_gpu_instantaneous_exact import check
    from test_oracle_exact_tfe import family
    L, blocks = 256, 8
    H = {"noise": 6, "quantised": 24}[fam]                               # some half waves are longer than that, most are not
    x = family(fam, blocks * L)
    hw = et.structure(x)[1]
    ln = np.bincount(hw)[hw]
    long_, ovl = ln > H, ssr.overlong_of(ln, H)
    assert ovl.any() and not ovl.all()
    st = S.InstantaneousStream(L, 1, H, want=ALL)
    got, _, _ = run_stream(st, x[None])
    st.close()
    a, p, f, length = (g[0] for g in got[:4])
    none = lambda v: v.view(np.uint64) == isr.NONE_BITS
    assert np.array_equal(none(a), long_) and np.array_equal(none(p), long_) and np.array_equal(none(f), ovl)
    assert np.array_equal(length, np.where(long_, 0, ln).astype(np.int32))
    assert np.array_equal(got[4][0], long_.reshape(blocks, L).sum(axis=1)) and np.array_equal(got[5][0], ovl.reshape(blocks, L).sum(axis=1))
    check(x, a, p, f, samples=np.flatnonzero(~ovl), what=fam)


# ---- 4. position and ordering ------------------------------------------------------------------------------------------------------------
def test_the_same_bits_in_any_batch_position_and_from_run_to_run(P, S):
    L, H, blocks, R = 100, 150, 6, 70
    rng = np.random.default_rng(70)
    base = signals(rng, L, H, 7, blocks)
    idx = rng.integers(0, 7, R)
    idx[:7] = np.arange(7)
    x = base[idx]
    st = S.InstantaneousStream(L, R, H, want=ALL)
    a, _, _ = run_stream(st, x)
    b, _, _ = run_stream(st, x)
    st.close()
    same(b, a, "the same stream twice")
    want, _, ovl = expected(P, base, L, H)
    same(a, tuple(w[idx] for w in want), "70 rows")
    assert ovl.any() and not ovl.all()
    one = S.InstantaneousStream(L, 1, H, want=ALL)
    for r in (3, 5):
        got, _, _ = run_stream(one, base[r:r + 1])
        same(got, tuple(w[r:r + 1] for w in want), "row %d alone" % r)
    one.close()


# ---- 5. device forms ------------------------------------------------------------------------------------------------------------------------
SUBSETS = [s for k in range(1, 5) for s in itertools.combinations(range(4), k)]


def test_device_forms_every_subset_strides_guards_and_null_counts(P, S):
    import torch
    L, H, R, blocks = 64, 100, 3, 5
    D = latency(L, H)
    assert len(SUBSETS) == 15 and D == 2
    rng = np.random.default_rng(55)
    x = signals(rng, L, H, R, blocks)
    want, _, ovl = expected(P, x, L, H)
    assert ovl.any() and not ovl.all()
    xs, os_, cs, guard = blocks * L + 5, L + 3, 5, 16
    xin = np.full((R, xs), 1e30)
    xin[:, :blocks * L] = x
    xd = torch.from_numpy(xin).cuda()
    ts = torch.cuda.Stream()
    st = S.InstantaneousStream(L, R, H)                                   # (one stream: it starts afresh after its flush)
    for k, subset in enumerate(SUBSETS):
        counts = k % 2 == 0
        s = ts.cuda_stream if k % 3 == 0 else None                        # a caller's stream, or the stream's own
        fo = torch.full((3, blocks + 1, guard + R * os_ + guard), SENT, dtype=torch.float64, device="cuda")
        lo = torch.full((blocks + 1, guard + R * os_ + guard), ISENT, dtype=torch.int32, device="cuda")
        co = torch.full((blocks + 1, guard + R * cs + guard), ISENT, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def ptrs(o):
            return ([fo[i, o, guard:].data_ptr() if i in subset else None for i in range(3)] +
                    [lo[o, guard:].data_ptr() if 3 in subset else None, os_, co[o, guard:].data_ptr() if counts else None, cs, s])
        o = 0
        for p in range(blocks):
            em = st.push_dev(xd[:, p * L:].data_ptr(), xs, *ptrs(o))
            assert em == (p >= D)
            if not em:                                                    # nothing is written by a push that does not emit
                torch.cuda.synchronize()
                assert bool((fo == SENT).all()) and bool((lo == ISENT).all()) and bool((co == ISENT).all())
            o += em
        while st.flush_dev(*ptrs(o)):
            o += 1
        torch.cuda.synchronize()
        assert o == blocks and st.status() == 0 and st.blocks_held == 0
        foh, loh, coh = fo.cpu().numpy(), lo.cpu().numpy(), co.cpu().numpy()
        what = "outputs %s, counts %s" % ([ALL[i] for i in subset], counts)
        for i, arr, sent in [(0, foh[0], SENT), (1, foh[1], SENT), (2, foh[2], SENT), (3, loh, ISENT)]:
            assert np.all(arr[:, :guard] == sent) and np.all(arr[:, guard + R * os_:] == sent) and np.all(arr[blocks] == sent), what
            body = arr[:blocks, guard:guard + R * os_].reshape(blocks, R, os_)
            assert np.all(body[:, :, L:] == sent), "%s: the padding between rows is written" % what
            if i in subset:
                same((body[:, :, :L].transpose(1, 0, 2).reshape(R, blocks * L),), (want[i],), what, (NAMES[i],))
            else:
                assert np.all(body == sent), "%s: %s was not asked for and is written" % (what, NAMES[i])
        assert np.all(coh[:, :guard] == ISENT) and np.all(coh[:, guard + R * cs:] == ISENT) and np.all(coh[blocks] == ISENT)
        cbody = coh[:blocks, guard:guard + R * cs].reshape(blocks, R, cs)
        if counts:
            assert np.all(cbody[:, :, 2:] == ISENT)
            same((cbody[:, :, 0].T, cbody[:, :, 1].T), want[4:], what, NAMES[4:])
        else:
            assert np.all(cbody == ISENT), "NULL counts"
    st.close()


# ---- 6. stream state ---------------------------------------------------------------------------------------------------------------------
def test_flush_order_restart_refusals_reset_and_blocks(P, S):
    import torch
    from pyitd_amd import ITDError, _lib
    L, H, R, blocks = 100, 150, 2, 5
    D = latency(L, H)
    assert D == 2
    lib = _lib.load()
    rng = np.random.default_rng(6)
    x = signals(rng, L, H, R, blocks)
    want, _, _ = expected(P, x, L, H)
    st = S.InstantaneousStream(L, R, H, want=ALL)
    assert st.blocks_held == 0 and st.flush() is None
    y = signals(rng, L, H, R, 4)
    for p in range(4):                                                    # past the latency: blocks have been emitted
        st.push(y[:, p * L:(p + 1) * L])
    assert st.blocks_held == 2
    st.reset()
    assert st.blocks_held == 0
    got, pattern, flushed = run_stream(st, x)
    assert pattern == [False, False, True, True, True] and flushed == 2
    same(got, want, "after reset")
    got, _, _ = run_stream(st, x)                                         # the stream started afresh after its last flush
    same(got, want, "after a flush")
    # a push between flushes is refused, host and device form; the flush goes on in order
    for p in range(3):
        st.push(x[:, p * L:(p + 1) * L])
    assert st.blocks_held == 2
    first = st.flush()
    assert st.blocks_held == 1
    with pytest.raises(ITDError):
        st.push(x[:, :L])
    buf = torch.zeros(R, L, dtype=torch.float64, device="cuda")
    out = torch.zeros(R, L, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(R, 2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(ITDError):
        st.push_dev(buf.data_ptr(), L, out.data_ptr(), None, None, None, L)
    second = st.flush()
    assert st.flush() is None and st.blocks_held == 0
    w3, _, _ = expected(P, x[:, :3 * L], L, H)
    same(tuple(first), tuple(w[:, L:2 * L] for w in w3[:4]) + tuple(w[:, 1] for w in w3[4:]), "the first flush: block 1")
    same(tuple(second), tuple(w[:, 2 * L:] for w in w3[:4]) + tuple(w[:, 2] for w in w3[4:]), "the second flush: block 2")
    # argument errors on a live stream; the other kinds' entries refuse it and its entries the other kinds
    for p in range(2):
        assert not st.push_dev(buf.data_ptr(), L, None, None, None, None, 0)   # nothing is emitted yet: no output is needed
    with pytest.raises(ITDError):                                         # this push emits: one output at least
        st.push_dev(buf.data_ptr(), L, None, None, None, None, L, cnt.data_ptr(), 2)
    with pytest.raises(ITDError):                                         # strides below the block / the two counts
        st.push_dev(buf.data_ptr(), L - 1, out.data_ptr(), None, None, None, L)
    with pytest.raises(ITDError):
        st.push_dev(buf.data_ptr(), L, out.data_ptr(), None, None, None, L - 1)
    with pytest.raises(ITDError):
        st.push_dev(buf.data_ptr(), L, out.data_ptr(), None, None, None, L, cnt.data_ptr(), 1)
    with pytest.raises(ITDError):
        st.flush_dev(None, None, None, None, L)
    assert st.blocks_held == 2
    assert lib.itd_stream_push_f64(st._h, buf.data_ptr(), L, out.data_ptr(), L, None, 0, None, None) == 1
    assert lib.itd_stream_flush_f64(st._h, out.data_ptr(), L, None, 0, None, None) == 1
    assert lib.itd_levels_stream_push_f64(st._h, buf.data_ptr(), L, out.data_ptr(), L, L, None, None, None) == 1
    assert lib.itd_levels_stream_flush_f64(st._h, out.data_ptr(), L, L, None, None, None) == 1
    assert lib.itd_wave_stream_push_f64(st._h, buf.data_ptr(), L, out.data_ptr(), 0, out.data_ptr(), L, None, None) == 1
    assert lib.itd_wave_stream_flush_f64(st._h, out.data_ptr(), 0, out.data_ptr(), L, None, None) == 1
    assert lib.itd_spectrum_stream_push_f64(st._h, buf.data_ptr(), L, out.data_ptr(), 0, out.data_ptr(), L, None, None, 0, None, None) == 1
    assert lib.itd_spectrum_stream_flush_f64(st._h, out.data_ptr(), 0, out.data_ptr(), L, None, None, 0, None, None) == 1
    assert lib.itd_wave_stream_latency(st._h) == -1 and lib.itd_spectrum_stream_latency(st._h) == -1
    assert lib.itd_levels_stream_form(st._h) == -1
    for other in (S.WaveFilterStream(L, R, H), S.SpectrumStream(128, R, H, edges=[0.0, 0.5], hop=64), S.LevelsStream(L, 2, R)):
        assert lib.itd_inst_stream_latency(other._h) == -1
        assert lib.itd_inst_stream_push_f64(other._h, buf.data_ptr(), L, out.data_ptr(), None, None, None, L, None, 0, None, None) == 1
        assert lib.itd_inst_stream_flush_f64(other._h, out.data_ptr(), None, None, None, L, None, 0, None, None) == 1
        assert lib.itd_inst_stream_push_host_f64(other._h, x[:, :L].ctypes.data, out.data_ptr(), None, None, None, None, None) == 1
        assert lib.itd_inst_stream_flush_host_f64(other._h, out.data_ptr(), None, None, None, None, None) == 1
        other.close()
    torch.cuda.synchronize()
    st.close()


def test_a_nan_sets_the_status_and_leaves_the_other_rows_exact(P, S):
    L, H, R, blocks = 100, 150, 3, 8
    rng = np.random.default_rng(5)
    x = signals(rng, L, H, R, blocks)
    want, _, _ = expected(P, x, L, H)
    x[1, 3 * L + 7] = np.nan
    st = S.InstantaneousStream(L, R, H, want=ALL)
    got, _, _ = run_stream(st, x)
    assert st.status() & 2
    same(tuple(g[[0, 2]] for g in got), tuple(w[[0, 2]] for w in want), "the rows without the NaN")
    st.reset()
    assert st.status() == 0
    st.close()


# ---- 7. the chain ----------------------------------------------------------------------------------------------------------------------------
def test_behind_a_levels_stream_on_device_pointers(S):
    """samples in, the per-sample quantities of every component out: the levels stream's emitted rows go into the instantaneous
    stream by pointer, on one stream, with no host copy in between; the result equals the stream fed with the host copy of the rows"""
    import torch
    L, M, Cn, nb, H = 1024, 3, 2, 10, 300
    R = Cn * (M + 1)
    rng = np.random.default_rng(31)
    t = np.arange(nb * L) / (nb * L)
    # noise, and four slow cycles under a little noise: the last row of that channel follows them in half waves far longer than H
    x = np.stack([fuzz_signal(rng, 0, nb * L), 3.0 * np.sin(2 * np.pi * 4 * t + 0.3) + 0.1 * rng.standard_normal(nb * L)])
    lv = S.LevelsStream(L, M, Cn)
    it = S.InstantaneousStream(L, R, H)
    assert it.latency == 1
    xd = torch.from_numpy(x).cuda()
    rows = torch.zeros(nb, Cn, M + 1, L, dtype=torch.float64, device="cuda")
    fo = torch.zeros(3, nb + 1, R, L, dtype=torch.float64, device="cuda")          # (+1: the pointer of the flush that finds it empty)
    lo = torch.zeros(nb + 1, R, L, dtype=torch.int32, device="cuda")
    co = torch.zeros(nb + 1, R, 2, dtype=torch.int32, device="cuda")
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    torch.cuda.synchronize()
    k = o = 0

    def outs(o):
        return (fo[0, o].data_ptr(), fo[1, o].data_ptr(), fo[2, o].data_ptr(), lo[o].data_ptr(), L, co[o].data_ptr(), 2, s)

    for p in range(nb):
        if lv.push_dev(xd[:, p * L:].data_ptr(), nb * L, rows[k].data_ptr(), L, (M + 1) * L, None, s):
            o += it.push_dev(rows[k].data_ptr(), L, *outs(o))
            k += 1
    while lv.flush_dev(rows[min(k, nb - 1)].data_ptr(), L, (M + 1) * L, None, s):
        o += it.push_dev(rows[k].data_ptr(), L, *outs(o))
        k += 1
    while it.flush_dev(*outs(o)):
        o += 1
    torch.cuda.synchronize()
    assert k == nb and o == nb
    streamed = rows.cpu().numpy().transpose(1, 2, 0, 3).reshape(R, nb * L)        # the concatenated rows the second stage saw
    per_sample = lambda v: v[:nb].cpu().numpy().transpose(1, 0, 2).reshape(R, nb * L)
    got = tuple(per_sample(fo[i]) for i in range(3)) + (per_sample(lo), co[:nb, :, 0].cpu().numpy().T, co[:nb, :, 1].cpu().numpy().T)
    host = S.InstantaneousStream(L, R, H, want=ALL)
    want, _, _ = run_stream(host, streamed)
    host.close()
    same(got, want, "levels stream -> instantaneous stream")
    assert want[5].any() and not want[5].all() and (want[3] > 0).any()    # a row of long half waves beside rows that are delivered
    assert lv.status() == 0 and it.status() == 0
    lv.close()
    it.close()


# ---- 8. the whole pass -----------------------------------------------------------------------------------------------------------------------
def test_blockwise_instantaneous_is_the_push_and_flush_loop(P, S):
    L, H, R, blocks = 100, 99, 3, 6
    rng = np.random.default_rng(8)
    x = signals(rng, L, H, R, blocks)
    st = S.InstantaneousStream(L, R, H, want=ALL)
    want, _, _ = run_stream(st, x)
    st.close()
    got = P.blockwise_instantaneous(x, L, H, want=ALL)
    assert isinstance(got, S.StreamInstant)
    same(tuple(got), want, "all four")
    got = P.blockwise_instantaneous(x, L, H)                              # the default: no length
    same(tuple(got), want[:3] + (None,) + want[4:], "the default selection")
    got = P.blockwise_instantaneous(x[1], L, H, want=("length", "frequency"))
    same(tuple(got), (None, None, want[2][1], want[3][1], want[4][1], want[5][1]), "one row, 1-D")
    with pytest.raises(ValueError):
        P.blockwise_instantaneous(x[:, :L + 1], L, H)
