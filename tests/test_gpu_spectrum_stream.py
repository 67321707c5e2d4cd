"""The spectrum stream on the GPU (itd_spectrum_stream_*, pyitd_amd.streaming.SpectrumStream) — everything bit for bit: power as
uint64 patterns, the counts exactly.

1. Composition: the stream's slices equal spectrum_ref on the amplitude and frequency instantaneous_batch returns for the
   concatenated rows, with the overlong mask from the half waves of tests/waves_ref.py forced outside.
2. With a horizon that holds the longest half wave: tfe_spectrum of the concatenated rows, overlong all zero.
3. Independently of the device's own amplitude and frequency: against oracle/exact_tfe.py.
4. The same bits in any batch position and from run to run; 70 rows in one stream.
5. Device forms: strides, padding, guards, NULL counts, nothing written by a push that does not emit.
6. Stream state: flush order, restart, refusals, reset, blocks, edges that move, a NaN row.
7. Behind a LevelsStream on device pointers.
The file also passes with PYITD_POISON=1.
"""
import numpy as np
import pytest

import spectrum_ref as sr
import spectrum_stream_ref as ssr
from helpers import fuzz_signal
from ring_stream_runs import enveloped_signals as signals, latency, push_and_flush
from waves_ref import ref_table

pytestmark = pytest.mark.gpu
SENT = -7.25e300
ISENT = -777
HOPS = {64: (64,), 128: (64, 128), 512: (256, 512), 1024: (256, 1024)}
BINS = (1, 7, 512)


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


@pytest.fixture(scope="module")
def S():
    from pyitd_amd import streaming
    return streaming


def edges_of(kind, F):
    """uniform on [0.02, 0.6) or logarithmic on [1e-4, 0.5): the frequency 0.5 that a run of one-sample half waves gives — all that
    is left inside a horizon of 1 — lies inside the first and outside the second"""
    return sr.uniform_edges(F, 0.02, 0.6) if kind == 0 else sr.log_edges(F)


def same(got, want, what):
    for g, w, name in zip(got, want, ("power", "outside", "overlong")):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, "%s %s: %s %s vs %s %s" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        gb, wb = (g.view(np.uint64), w.view(np.uint64)) if g.dtype == np.float64 else (g, w)
        bad = np.flatnonzero(gb.ravel() != wb.ravel())
        assert bad.size == 0, "%s: %d of %d %s cells differ, first at %d: %r vs %r" % (what, bad.size, g.size, name, bad[0], g.ravel()[bad[0]],
                                                                                    w.ravel()[bad[0]])


def overlong_rows(x, H):
    return np.stack([ssr.overlong_of(np.repeat(ref_table(r)[1].astype(np.int64), ref_table(r)[1]), H) for r in x])


def expected(A, f, overlong, edges, hop, weight):
    """(power[R, T, F], outside[R, T], overlong[R, T]) of rows with amplitude A, frequency f and the overlong mask; edges [F+1] or [R, F+1]"""
    e = np.broadcast_to(edges, (A.shape[0], np.shape(edges)[-1]))
    out = [ssr.masked_spectrum(a, fr, ov, er, hop, weight) for a, fr, ov, er in zip(A, f, overlong, e)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def run_stream(st, x, edges=None):
    """push every block, flush until empty: (power[R, T, F], outside[R, T], overlong[R, T]), the pushes' emission pattern, the
    flushes that emitted"""
    outs, pattern, flushed = push_and_flush(st, x, (edges,))
    return tuple(np.concatenate([o[i] for o in outs], axis=1) for i in range(3)), pattern, flushed


# ---- 1. composition, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hk", ("1", "L-1", "L", "L+1", "2L"))
@pytest.mark.parametrize("L", sorted(HOPS))
def test_composition_of_the_instantaneous_outputs(P, S, L, hk):
    H = {"1": 1, "L-1": L - 1, "L": L, "L+1": L + 1, "2L": 2 * L}[hk]
    D = latency(L, H)
    rng = np.random.default_rng(L * 1009 + H)
    streams = {}
    n_overlong = n_inside = n_plain = 0
    for blocks in range(1, 2 * D + 4):
        x = signals(rng, L, H, 3, blocks)
        A, f = P.instantaneous_batch(x, want=("amplitude", "frequency"))
        ovl = overlong_rows(x, H)
        for wi, weight in enumerate(sr.WEIGHTS):
            F = BINS[(blocks + wi) % 3]
            hop = HOPS[L][(blocks + wi) % len(HOPS[L])]
            edges = edges_of((blocks + wi // 2) % 2, F)
            key = (hop, F, weight)
            if key not in streams:
                streams[key] = S.SpectrumStream(L, 3, H, edges=edges, hop=hop, weight=weight)
                assert streams[key].latency == D
            st = streams[key]                                             # (reused: it starts afresh after its flush)
            want = expected(A, f, ovl, edges, hop, weight)
            got, pattern, flushed = run_stream(st, x, edges)
            what = "L=%d H=%d blocks=%d hop=%d F=%d %s" % (L, H, blocks, hop, F, weight)
            assert pattern == [p >= D for p in range(blocks)] and flushed == min(blocks, D), what
            same(got, want, what)
            _, inside = sr.bins_of(f.ravel(), edges)
            n_overlong += int(ovl.sum())
            n_inside += int((inside & ~ovl.ravel()).sum())
            n_plain += int((~inside & ~ovl.ravel()).sum())
    assert n_overlong > 0 and n_inside > 0 and n_plain > 0, (n_overlong, n_inside, n_plain)
    for st in streams.values():
        assert st.status() == 0
        st.close()


# ---- 2. equality with the whole-row call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,hop", [(64, 64), (512, 256), (1024, 1024)])
def test_with_a_horizon_that_holds_every_half_wave_it_is_tfe_spectrum(P, S, L, hop):
    rng = np.random.default_rng(L + hop)
    blocks = 7
    x = np.stack([fuzz_signal(rng, k, blocks * L) for k in (0, 4, 6)])
    H = int(max(ref_table(r)[1].max() for r in x))                       # exactly the longest half wave
    edges = sr.log_edges(16)
    for weight in sr.WEIGHTS:
        st = S.SpectrumStream(L, 3, H, edges=edges, hop=hop, weight=weight)
        got, _, _ = run_stream(st, x)
        st.close()
        want = P.tfe_spectrum(x, edges, hop, weight)
        same(got, (want.power, want.outside, np.zeros_like(want.outside)), "L=%d hop=%d H=%d %s" % (L, hop, H, weight))
        assert np.count_nonzero(want.power)


# ---- 3. against the exact reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ("noise", "quantised"))
def test_against_the_exact_reference(S, fam):
    """Amplitudes and bin decisions from oracle/exact_tfe.py with the edges (k + 1/pi) / (F + 1); a cell is left out where a sample of
    its time slice has its exact frequency within 2 F_TOL of one of the cell's edges (the tolerance of
    test_gpu_tfe_spectrum.test_against_the_exact_reference); at most 2 % of the cells may be."""
    from oracle import exact_tfe as et
    from test_gpu_instantaneous_exact import F_TOL
    from test_oracle_exact_tfe import family
    L, hop, blocks = 256, 64, 8
    H = {"noise": 6, "quantised": 24}[fam]                               # some half waves are longer than that, most are not
    n = blocks * L
    x = family(fam, n)
    ex = et.exact_tfe(x)
    ovl = overlong_rows(x[None], H)[0]
    assert ovl.any() and not ovl.all()
    for F in (7, 64):
        edges = sr.pi_edges(F)
        dist = np.abs((ex.freq_hi[:, None] - edges[None, :]) + ex.freq_lo[:, None])
        near = dist <= 2 * F_TOL                                          # [n, F + 1]
        T = n // hop
        skip = np.zeros((T, F), bool)
        skip_out = np.zeros(T, bool)
        for j, e in zip(*np.nonzero(near)):
            t = j // hop
            skip[t, max(e - 1, 0):min(e + 1, F)] = True
            skip_out[t] |= e in (0, F)
        assert skip.mean() <= 0.02 and skip_out.mean() <= 0.02
        for weight in sr.WEIGHTS:
            want = ssr.masked_spectrum(ex.amp, ex.freq_hi, ovl, edges, hop, weight)
            st = S.SpectrumStream(L, 1, H, edges=edges, hop=hop, weight=weight)
            got, _, _ = run_stream(st, x[None])
            st.close()
            what = "%s F=%d %s" % (fam, F, weight)
            same((np.where(skip, 0.0, got[0][0]), np.where(skip_out, 0, got[1][0]), got[2][0]),
                 (np.where(skip, 0.0, want[0]), np.where(skip_out, 0, want[1]), want[2]), what)


# ---- 4. position and ordering ------------------------------------------------------------------------------------------------------------
def test_the_same_bits_in_any_batch_position_and_from_run_to_run(P, S):
    L, H, hop, blocks, R = 128, 200, 64, 6, 70
    rng = np.random.default_rng(70)
    base = signals(rng, L, H, 7, blocks)
    idx = rng.integers(0, 7, R)
    idx[:7] = np.arange(7)
    x = base[idx]
    edges = sr.uniform_edges(7, 0.02, 0.4)
    st = S.SpectrumStream(L, R, H, edges=edges, hop=hop, weight="energy")
    a, _, _ = run_stream(st, x)
    b, _, _ = run_stream(st, x)
    st.close()
    same(b, a, "the same stream twice")
    A, f = P.instantaneous_batch(base, want=("amplitude", "frequency"))
    want = expected(A, f, overlong_rows(base, H), edges, hop, "energy")
    same(a, tuple(w[idx] for w in want), "70 rows")
    one = S.SpectrumStream(L, 1, H, edges=edges, hop=hop, weight="energy")
    got, _, _ = run_stream(one, base[3:4])
    one.close()
    same(got, tuple(w[3:4] for w in want), "a row alone")


# ---- 5. device forms ------------------------------------------------------------------------------------------------------------------------
def test_device_forms_strides_guards_and_null_counts(P, S):
    import torch
    L, H, hop, F, R, blocks = 256, 300, 64, 7, 3, 6
    C, D = L // hop, latency(L, H)
    rng = np.random.default_rng(55)
    x = signals(rng, L, H, R, blocks)
    edges = np.stack([sr.uniform_edges(F, 0.02, 0.4), sr.log_edges(F), sr.uniform_edges(F, 0.1, 0.3)])
    A, f = P.instantaneous_batch(x, want=("amplitude", "frequency"))
    want = expected(A, f, overlong_rows(x, H), edges, hop, "amplitude")
    xs, es, ps, cs, guard = blocks * L + 5, F + 4, C * F + 3, C + 2, 16
    xin = np.full((R, xs), 1e30)
    xin[:, :blocks * L] = x
    ein = np.full((R, es), np.nan)
    ein[:, :F + 1] = edges
    xd, ed = torch.from_numpy(xin).cuda(), torch.from_numpy(ein).cuda()
    for counts in (True, False):
        st = S.SpectrumStream(L, R, H, edges=edges, hop=hop, weight="amplitude")
        pw = torch.full((blocks + 1, guard + R * ps + guard), SENT, dtype=torch.float64, device="cuda")
        oc = torch.full((2, blocks + 1, guard + R * cs + guard), ISENT, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def ptrs(o):
            return (pw[o, guard:].data_ptr(), ps, oc[0, o, guard:].data_ptr() if counts else None,
                    oc[1, o, guard:].data_ptr() if counts else None, cs)
        o = 0
        for p in range(blocks):
            em = st.push_dev(xd[:, p * L:].data_ptr(), xs, ed.data_ptr(), es, *ptrs(o))
            assert em == (p >= D)
            if not em:                                                    # nothing is written by a push that does not emit
                torch.cuda.synchronize()
                assert bool((pw == SENT).all()) and bool((oc == ISENT).all())
            o += em
        while st.flush_dev(ed.data_ptr(), es, *ptrs(o)):
            o += 1
        torch.cuda.synchronize()
        assert o == blocks and st.status() == 0
        st.close()
        pwh, och = pw.cpu().numpy(), oc.cpu().numpy()
        assert np.all(pwh[:, :guard] == SENT) and np.all(pwh[:, guard + R * ps:] == SENT) and np.all(pwh[blocks] == SENT)
        assert np.all(och[:, :, :guard] == ISENT) and np.all(och[:, :, guard + R * cs:] == ISENT) and np.all(och[:, blocks] == ISENT)
        body = pwh[:blocks, guard:guard + R * ps].reshape(blocks, R, ps)
        assert np.all(body[:, :, C * F:] == SENT), "the padding between rows is written"
        power = body[:, :, :C * F].reshape(blocks, R, C, F).transpose(1, 0, 2, 3).reshape(R, blocks * C, F)
        cbody = och[:, :blocks, guard:guard + R * cs].reshape(2, blocks, R, cs)
        if counts:
            assert np.all(cbody[:, :, :, C:] == ISENT)
            cnt = cbody[:, :, :, :C].transpose(0, 2, 1, 3).reshape(2, R, blocks * C)
            same((power, cnt[0], cnt[1]), want, "device form")
        else:
            assert np.all(cbody == ISENT), "NULL outside / overlong"
            same((power,), want[:1], "device form without counts")
    assert want[2].any() and np.count_nonzero(want[0])


# ---- 6. stream state ---------------------------------------------------------------------------------------------------------------------
def test_flush_order_restart_refusals_reset_and_blocks(P, S):
    import torch
    from pyitd_amd import ITDError, _lib
    L, H, hop, F, R, blocks = 128, 200, 64, 7, 2, 5
    D = latency(L, H)
    assert D == 2
    lib = _lib.load()
    rng = np.random.default_rng(6)
    x = signals(rng, L, H, R, blocks)
    edges = sr.uniform_edges(F, 0.02, 0.4)
    A, f = P.instantaneous_batch(x, want=("amplitude", "frequency"))
    want = expected(A, f, overlong_rows(x, H), edges, hop, "energy")
    st = S.SpectrumStream(L, R, H, edges=edges, hop=hop)
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
    ed = torch.from_numpy(edges).cuda()
    pw = torch.zeros(R, (L // hop) * F, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(ITDError):
        st.push_dev(buf.data_ptr(), L, ed.data_ptr(), 0, pw.data_ptr(), pw.shape[1])
    second = st.flush()
    assert st.flush() is None and st.blocks_held == 0
    Af, ff = P.instantaneous_batch(x[:, :3 * L], want=("amplitude", "frequency"))
    w3 = expected(Af, ff, overlong_rows(x[:, :3 * L], H), edges, hop, "energy")
    C = L // hop
    same(tuple(v for v in first), tuple(w[:, C:2 * C] for w in w3), "the first flush: block 1")
    same(tuple(v for v in second), tuple(w[:, 2 * C:] for w in w3), "the second flush: block 2")
    # argument errors on a live stream; the other kinds' entries refuse it and its entries the other kinds
    for p in range(2):
        assert not st.push_dev(buf.data_ptr(), L, None, 0, None, 0)      # nothing is emitted yet: neither edges nor an output is needed
    with pytest.raises(ITDError):                                         # this push emits: the output is required
        st.push_dev(buf.data_ptr(), L, ed.data_ptr(), 0, None, 0)
    with pytest.raises(ITDError):                                         # ... and the edges
        st.push_dev(buf.data_ptr(), L, None, 0, pw.data_ptr(), pw.shape[1])
    with pytest.raises(ITDError):                                         # an edges stride of 1 .. F
        st.push_dev(buf.data_ptr(), L, ed.data_ptr(), F, pw.data_ptr(), pw.shape[1])
    with pytest.raises(ITDError):                                         # strides below the block / the cells
        st.push_dev(buf.data_ptr(), L - 1, ed.data_ptr(), 0, pw.data_ptr(), pw.shape[1])
    with pytest.raises(ITDError):
        st.push_dev(buf.data_ptr(), L, ed.data_ptr(), 0, pw.data_ptr(), pw.shape[1] - 1)
    assert st.blocks_held == 2
    assert lib.itd_stream_push_f64(st._h, buf.data_ptr(), L, pw.data_ptr(), L, None, 0, None, None) == 1
    assert lib.itd_stream_flush_f64(st._h, pw.data_ptr(), L, None, 0, None, None) == 1
    assert lib.itd_levels_stream_push_f64(st._h, buf.data_ptr(), L, pw.data_ptr(), L, L, None, None, None) == 1
    assert lib.itd_levels_stream_flush_f64(st._h, pw.data_ptr(), L, L, None, None, None) == 1
    assert lib.itd_wave_stream_push_f64(st._h, buf.data_ptr(), L, ed.data_ptr(), 0, pw.data_ptr(), L, None, None) == 1
    assert lib.itd_wave_stream_flush_f64(st._h, ed.data_ptr(), 0, pw.data_ptr(), L, None, None) == 1
    assert lib.itd_wave_stream_latency(st._h) == -1 and lib.itd_levels_stream_form(st._h) == -1
    wf = S.WaveFilterStream(L, R, H)
    assert lib.itd_spectrum_stream_latency(wf._h) == -1
    assert lib.itd_spectrum_stream_push_f64(wf._h, buf.data_ptr(), L, ed.data_ptr(), 0, pw.data_ptr(), pw.shape[1], None, None, 0, None, None) == 1
    assert lib.itd_spectrum_stream_flush_f64(wf._h, ed.data_ptr(), 0, pw.data_ptr(), pw.shape[1], None, None, 0, None, None) == 1
    wf.close()
    torch.cuda.synchronize()
    st.close()


def test_edges_changed_between_two_pushes_are_followed(P, S):
    L, H, hop, F, R, blocks = 128, 100, 128, 7, 2, 6
    rng = np.random.default_rng(12)
    x = signals(rng, L, H, R, blocks)
    e0, e1 = sr.uniform_edges(F, 0.02, 0.4), sr.log_edges(F)
    A, f = P.instantaneous_batch(x, want=("amplitude", "frequency"))
    ovl = overlong_rows(x, H)
    w0, w1 = expected(A, f, ovl, e0, hop, "count"), expected(A, f, ovl, e1, hop, "count")
    st = S.SpectrumStream(L, R, H, edges=e0, hop=hop, weight="count")
    outs = []
    for p in range(blocks):
        r = st.push(x[:, p * L:(p + 1) * L], e1 if p == 3 else None)      # from push 3 on: block 3 - D = 2 is the first under e1
        if r is not None:
            outs.append(r)
    while (r := st.flush()) is not None:
        outs.append(r)
    st.close()
    got = tuple(np.concatenate([o[i] for o in outs], axis=1) for i in range(3))
    cut = 3 - latency(L, H)
    same(got, tuple(np.concatenate((a[:, :cut], b[:, cut:]), axis=1) for a, b in zip(w0, w1)), "edges moved at push 3")
    assert not np.array_equal(w0[0], w1[0])


def test_a_nan_sets_the_status_and_leaves_the_other_rows_exact(P, S):
    L, H, hop, F, R, blocks = 64, 100, 64, 7, 3, 8
    rng = np.random.default_rng(5)
    x = signals(rng, L, H, R, blocks)
    edges = sr.uniform_edges(F, 0.02, 0.4)
    A, f = P.instantaneous_batch(x, want=("amplitude", "frequency"))
    want = expected(A, f, overlong_rows(x, H), edges, hop, "energy")
    x[1, 3 * L + 7] = np.nan
    st = S.SpectrumStream(L, R, H, edges=edges, hop=hop)
    got, _, _ = run_stream(st, x)
    assert st.status() & 2
    same(tuple(g[[0, 2]] for g in got), tuple(w[[0, 2]] for w in want), "the rows without the NaN")
    st.reset()
    assert st.status() == 0
    st.close()


# ---- 7. the chain ----------------------------------------------------------------------------------------------------------------------------
def test_behind_a_levels_stream_on_device_pointers(S):
    """samples in, a running spectrum of every component out: the levels stream's emitted rows go into the spectrum stream by pointer,
    on one stream, with no host copy in between; the result equals the spectrum stream fed with the host copy of the same rows"""
    import torch
    L, M, Cn, nb, H, hop, F = 1024, 3, 2, 10, 300, 256, 64
    R, C = Cn * (M + 1), L // hop
    rng = np.random.default_rng(31)
    t = np.arange(nb * L) / (nb * L)
    # noise, and four slow cycles under a little noise: the last row of that channel follows them in half waves far longer than H
    x = np.stack([fuzz_signal(rng, 0, nb * L), 3.0 * np.sin(2 * np.pi * 4 * t + 0.3) + 0.1 * rng.standard_normal(nb * L)])
    edges = sr.log_edges(F)
    lv = S.LevelsStream(L, M, Cn)
    sp = S.SpectrumStream(L, R, H, edges=edges, hop=hop)
    assert sp.latency == 1
    xd = torch.from_numpy(x).cuda()
    ed = torch.from_numpy(edges).cuda()
    rows = torch.zeros(nb, Cn, M + 1, L, dtype=torch.float64, device="cuda")
    pw = torch.zeros(nb + 1, R, C, F, dtype=torch.float64, device="cuda")          # (+1: the pointer of the flush that finds it empty)
    oc = torch.zeros(2, nb + 1, R, C, dtype=torch.int32, device="cuda")
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    torch.cuda.synchronize()
    k = o = 0

    def spectrum_block(k, o):
        return o + (1 if sp.push_dev(rows[k].data_ptr(), L, ed.data_ptr(), 0, pw[o].data_ptr(), C * F, oc[0, o].data_ptr(),
                                     oc[1, o].data_ptr(), C, s) else 0)

    for p in range(nb):
        if lv.push_dev(xd[:, p * L:].data_ptr(), nb * L, rows[k].data_ptr(), L, (M + 1) * L, None, s):
            o = spectrum_block(k, o)
            k += 1
    while lv.flush_dev(rows[min(k, nb - 1)].data_ptr(), L, (M + 1) * L, None, s):
        o = spectrum_block(k, o)
        k += 1
    while sp.flush_dev(ed.data_ptr(), 0, pw[o].data_ptr(), C * F, oc[0, o].data_ptr(), oc[1, o].data_ptr(), C, s):
        o += 1
    torch.cuda.synchronize()
    assert k == nb and o == nb
    streamed = rows.cpu().numpy().transpose(1, 2, 0, 3).reshape(R, nb * L)        # the concatenated rows the second stage saw
    got = (pw[:nb].cpu().numpy().transpose(1, 0, 2, 3).reshape(R, nb * C, F), oc[0, :nb].cpu().numpy().transpose(1, 0, 2).reshape(R, nb * C),
           oc[1, :nb].cpu().numpy().transpose(1, 0, 2).reshape(R, nb * C))
    host = S.SpectrumStream(L, R, H, edges=edges, hop=hop)
    want, _, _ = run_stream(host, streamed)
    host.close()
    same(got, want, "levels stream -> spectrum stream")
    assert np.count_nonzero(want[0]) and want[2].any() and (want[1] > want[2]).any()
    assert lv.status() == 0 and sp.status() == 0
    lv.close()
    sp.close()
