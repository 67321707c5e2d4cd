"""The histogram stream on the GPU (itd_hist_stream_*, pyitd_amd.streaming.WaveHistogramStream) — every comparison integer for integer
on count, samples, outside and overlong.

1. Against the block-local rule of tests/hist_stream_ref.py.
2. With a horizon that holds every half wave: pyitd_amd.wave_histogram of the concatenated rows, overlong all zero.
3. The same integers in any batch position and from run to run.
4. The LDS corners: the most cells a block may hold, the widest axis, the smallest stream; one bin above the cap is refused.
5. Device forms: strides, padding, shared against per-row edges, NULL counts, guards.
6. The ring contract: emission pattern, blocks_held, flushes, the refusal of a push between flushes, restart, reset.
7. Edges that move.  8. A NaN row.  9. Behind a LevelsStream on device pointers.  10. Other calls on the same device in between.
"""
import numpy as np
import pytest

import hist_stream_ref as hsr
import spectrum_stream_ref as ssr
from helpers import fuzz_signal
from ring_stream_runs import enveloped_signals, latency, push_and_flush
from wave_stream_ref import run_length_signal
from waves_ref import ref_table

pytestmark = pytest.mark.gpu
ISENT = -777
INVALID_ARG = 1                                                           # ITD_ERR_INVALID_ARG (include/pyitd_hip.h)
PART = (np.array([0.2, 0.5, 2.0]), np.array([2.0, 4.0, 64.0, 600.0]))     # some half waves fall outside
COVER = (np.array([0.0, 0.2, 0.5, 2.0, np.inf]), np.array([1.0, 2.0, 4.0, 64.0, 600.0, np.inf]))


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


@pytest.fixture(scope="module")
def S():
    from pyitd_amd import streaming
    return streaming


def signals(rng, L, H, blocks):
    """3 rows: two of ring_stream_runs.enveloped_signals and one with every maximum repeated at its half wave's ends"""
    x = enveloped_signals(rng, L, H, 2, blocks)
    return np.concatenate((x, hsr.tied_maxima(run_length_signal(rng, L, H, blocks))[None]))


def expected(x, L, H, ae, le, hop):
    """the rule for rows x; ae, le: [N + 1] or [R, N + 1]"""
    ae, le = np.broadcast_to(ae, (x.shape[0], np.shape(ae)[-1])), np.broadcast_to(le, (x.shape[0], np.shape(le)[-1]))
    out = [hsr.ref_hist_stream(r, L, H, a, l, hop) for r, a, l in zip(x, ae, le)]
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def run_stream(st, x):
    """push every block, flush until empty: the four concatenated outputs, the pushes' emission pattern, the flushes that emitted"""
    outs, pattern, flushed = push_and_flush(st, x)
    return tuple(np.concatenate([o[i] for o in outs], axis=1) for i in range(4)), pattern, flushed


# ---- 1. the rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hk", ("1", "L-1", "L", "L+1", "2L"))
@pytest.mark.parametrize("L,hop", [(64, 64), (128, 64), (512, 512), (1024, 256)])
def test_against_the_block_local_rule(S, L, hop, hk):
    H = {"1": 1, "L-1": L - 1, "L": L, "L+1": L + 1, "2L": 2 * L}[hk]
    D, blocks = latency(L, H, 0), 7
    rng = np.random.default_rng(L * 1013 + H)
    x = signals(rng, L, H, blocks)
    seen = np.zeros(3, np.int64)
    for ae, le in (PART, COVER):
        st = S.WaveHistogramStream(L, 3, H, ae, le, hop)
        assert st.latency == D
        got, pattern, flushed = run_stream(st, x)
        assert st.status() == 0
        st.close()
        what = "L=%d hop=%d H=%d %d x %d bins" % (L, hop, H, ae.size - 1, le.size - 1)
        assert pattern == [p >= D for p in range(blocks)] and flushed == min(blocks, D), what
        want = expected(x, L, H, ae, le, hop)
        hsr.same_ints(got, want, what)
        seen += (int(want[0].sum()), int(want[2].sum()), int(want[3].sum()))
    assert (seen > 0).all(), seen                                          # counted, outside and overlong all occur


# ---- 2. equality with the whole-row call ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,hop", [(512, 512), (1024, 512), (2048, 1024)])
def test_with_a_horizon_that_holds_every_half_wave_it_is_wave_histogram(P, S, L, hop):
    rng = np.random.default_rng(L + hop)
    blocks = 5
    x = np.stack([fuzz_signal(rng, k, blocks * L) for k in (0, 4, 6)])
    H = int(max(ref_table(r)[1].max() for r in x))                        # exactly the longest half wave
    amp = max(float(np.abs(x).max()), 1.0)
    ae, le = np.concatenate(([0.0], np.geomspace(1e-3 * amp, amp * 0.9, 12))), np.array([1.0, 2.0, 3.0, 5.0, 8.0, 13.0, 40.0, 1e6])
    st = S.WaveHistogramStream(L, 3, H, ae, le, hop)
    got, _, _ = run_stream(st, x)
    st.close()
    want = P.wave_histogram(x, ae, le, hop)
    hsr.same_ints(got, (want.count, want.samples, want.outside, np.zeros_like(want.outside)), "L=%d hop=%d H=%d" % (L, hop, H))
    assert want.count.sum() > 0 and want.outside.sum() > 0


# ---- 3. position and ordering ---------------------------------------------------------------------------------------------------------------
def test_the_same_integers_in_any_batch_position_and_from_run_to_run(S):
    L, H, hop, blocks = 128, 200, 64, 6
    rng = np.random.default_rng(73)
    base = signals(rng, L, H, blocks)
    x = base[[1, 2, 0, 1, 0]]
    ae = np.stack([PART[0] * s for s in (1.0, 0.5, 2.0, 1.5, 1.0)])        # per-row edges; rows 2 and 4 carry row 0 of base
    le = np.stack([PART[1] + k for k in (0.0, 1.0, 0.0, 2.0, 0.0)])
    st = S.WaveHistogramStream(L, 5, H, ae, le, hop)
    a, _, _ = run_stream(st, x)
    b, _, _ = run_stream(st, x)
    st.close()
    hsr.same_ints(b, a, "the same stream twice")
    hsr.same_ints(a, expected(x, L, H, ae, le, hop), "5 rows, per-row edges")
    one = S.WaveHistogramStream(L, 1, H, ae[4], le[4], hop)
    got, _, _ = run_stream(one, base[0:1])
    one.close()
    hsr.same_ints(got, tuple(v[4:5] for v in a), "row 0 of 1 against row 4 of 5")
    assert not np.array_equal(a[0][2], a[0][4])                            # row 2: the same samples under other edges


# ---- 4. the LDS corners -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,hop,Na,Nl", [(4096, 512, 32, 32), (4096, 4096, 64, 16), (64, 64, 1, 1)])
def test_the_largest_and_the_smallest_histograms(S, L, hop, Na, Nl):
    rng = np.random.default_rng(Na * Nl + L)
    H, blocks = L, 3
    x = run_length_signal(rng, min(L, 512), 40, blocks * L // min(L, 512))
    x = hsr.tied_maxima(x * ssr.envelope(x.size, rng))[None]
    ae = np.concatenate(([0.0], np.geomspace(0.1, 4.0, Na))) if Na > 1 else np.array([0.2, 2.0])
    le = np.concatenate(([1.0], np.geomspace(2.0, 700.0, Nl))) if Nl > 1 else np.array([1.0, 50.0])
    st = S.WaveHistogramStream(L, 1, H, ae, le, hop)
    got, _, _ = run_stream(st, x)
    st.close()
    want = expected(x, L, H, ae, le, hop)
    hsr.same_ints(got, want, "L=%d hop=%d %d x %d" % (L, hop, Na, Nl))
    assert want[0].sum() > 0 and np.count_nonzero(want[0].reshape(-1, Na * Nl).sum(axis=0)) >= min(Na * Nl, 4)


def test_one_bin_above_the_cap_is_refused_at_create():
    import ctypes
    from pyitd_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    for block, hop, na, nl in ((4096, 512, 32, 33), (4096, 256, 32, 17), (4096, 64, 43, 3), (2048, 64, 33, 8)):
        assert lib.itd_hist_stream_create(ctypes.byref(h), 0, block, 1, 64, hop, na, nl) == INVALID_ARG and not h.value
    assert lib.itd_hist_stream_create(ctypes.byref(h), 0, 4096, 1, 64, 64, 42, 3) == 0 and h.value      # 64 * 126 = 8064 cells
    assert lib.itd_hist_stream_latency(h) == 1 and lib.itd_stream_blocks(h) == 0
    lib.itd_stream_destroy(h)


# ---- 5. device forms -----------------------------------------------------------------------------------------------------------------------------
def test_device_forms_strides_guards_and_null_counts(S):
    import torch
    L, H, hop, R, blocks = 256, 300, 64, 3, 6
    C, D = L // hop, latency(L, H, 0)
    rng = np.random.default_rng(57)
    x = signals(rng, L, H, blocks)
    ae = np.stack([PART[0], PART[0] * 0.5, COVER[0][:3]])
    le = np.stack([PART[1], PART[1] + 1.0, PART[1]])
    Na, Nl = ae.shape[1] - 1, le.shape[1] - 1
    F = C * Na * Nl
    want = expected(x, L, H, ae, le, hop)
    xs, as_, ls, hs, cs, guard = blocks * L + 5, Na + 4, Nl + 3, F + 3, C + 2, 16
    xin = np.full((R, xs), 1e30)
    xin[:, :blocks * L] = x
    ain, lin = np.full((R, as_), np.nan), np.full((R, ls), np.nan)
    ain[:, :Na + 1], lin[:, :Nl + 1] = ae, le
    xd, ad, ld = torch.from_numpy(xin).cuda(), torch.from_numpy(ain).cuda(), torch.from_numpy(lin).cuda()
    for counts in (True, False):
        st = S.WaveHistogramStream(L, R, H, ae, le, hop)
        hist = torch.full((2, blocks + 1, guard + R * hs + guard), ISENT, dtype=torch.int32, device="cuda")
        oc = torch.full((2, blocks + 1, guard + R * cs + guard), ISENT, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def ptrs(o):
            return (ad.data_ptr(), as_, ld.data_ptr(), ls, hist[0, o, guard:].data_ptr(), hist[1, o, guard:].data_ptr(), hs,
                    oc[0, o, guard:].data_ptr() if counts else None, oc[1, o, guard:].data_ptr() if counts else None, cs)
        o = 0
        for p in range(blocks):
            em = st.push_dev(xd[:, p * L:].data_ptr(), xs, *ptrs(o))
            assert em == (p >= D)
            if not em:                                                    # nothing is written by a push that does not emit
                torch.cuda.synchronize()
                assert bool((hist == ISENT).all()) and bool((oc == ISENT).all())
            o += em
        while st.flush_dev(*ptrs(o)):
            o += 1
        torch.cuda.synchronize()
        assert o == blocks and st.status() == 0
        st.close()
        hh, och = hist.cpu().numpy(), oc.cpu().numpy()
        assert np.all(hh[:, :, :guard] == ISENT) and np.all(hh[:, :, guard + R * hs:] == ISENT) and np.all(hh[:, blocks] == ISENT)
        assert np.all(och[:, :, :guard] == ISENT) and np.all(och[:, :, guard + R * cs:] == ISENT) and np.all(och[:, blocks] == ISENT)
        body = hh[:, :blocks, guard:guard + R * hs].reshape(2, blocks, R, hs)
        assert np.all(body[..., F:] == ISENT), "the padding between rows is written"
        cells = body[..., :F].reshape(2, blocks, R, C, Na, Nl).transpose(0, 2, 1, 3, 4, 5).reshape(2, R, blocks * C, Na, Nl)
        cbody = och[:, :blocks, guard:guard + R * cs].reshape(2, blocks, R, cs)
        if counts:
            assert np.all(cbody[..., C:] == ISENT)
            cnt = cbody[..., :C].transpose(0, 2, 1, 3).reshape(2, R, blocks * C)
            hsr.same_ints((cells[0], cells[1], cnt[0], cnt[1]), want, "device form")
        else:
            assert np.all(cbody == ISENT), "NULL outside / overlong"
            hsr.same_ints((cells[0], cells[1]), want[:2], "device form without counts")
    assert want[0].sum() > 0 and want[2].any() and want[3].any()


def test_one_shared_set_of_edges_is_the_same_set_per_row(S):
    import torch
    L, H, hop, R, blocks = 128, 100, 64, 3, 4
    C, D = L // hop, latency(L, H, 0)
    ae, le = PART
    Na, Nl = ae.size - 1, le.size - 1
    F = C * Na * Nl
    rng = np.random.default_rng(58)
    x = signals(rng, L, H, blocks)
    xd = torch.from_numpy(x).cuda()
    got = []
    for shared in (True, False):
        a2, l2 = (ae, le) if shared else (np.tile(ae, (R, 1)), np.tile(le, (R, 1)))
        ad, ld = torch.from_numpy(np.ascontiguousarray(a2)).cuda(), torch.from_numpy(np.ascontiguousarray(l2)).cuda()
        sa, sl = (0, 0) if shared else (Na + 1, Nl + 1)
        st = S.WaveHistogramStream(L, R, H, ae, le, hop)
        hist = torch.zeros(2, blocks + 1, R, F, dtype=torch.int32, device="cuda")
        oc = torch.zeros(2, blocks + 1, R, C, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        args = lambda o: (ad.data_ptr(), sa, ld.data_ptr(), sl, hist[0, o].data_ptr(), hist[1, o].data_ptr(), F, oc[0, o].data_ptr(),
                          oc[1, o].data_ptr(), C)
        o = 0
        for p in range(blocks):
            o += st.push_dev(xd[:, p * L:].data_ptr(), blocks * L, *args(o))
        while st.flush_dev(*args(o)):
            o += 1
        torch.cuda.synchronize()
        st.close()
        assert o == blocks
        h, c = hist[:, :blocks].cpu().numpy(), oc[:, :blocks].cpu().numpy()
        cells = h.reshape(2, blocks, R, C, Na, Nl).transpose(0, 2, 1, 3, 4, 5).reshape(2, R, blocks * C, Na, Nl)
        cnt = c.transpose(0, 2, 1, 3).reshape(2, R, blocks * C)
        got.append((cells[0], cells[1], cnt[0], cnt[1]))
    hsr.same_ints(got[0], expected(x, L, H, ae, le, hop), "stride 0")
    hsr.same_ints(got[1], got[0], "per-row edges against one set")


def test_every_guard_refuses_with_nothing_written(S):
    import torch
    from pyitd_amd import ITDError, _lib
    L, H, hop, R = 128, 128, 64, 2
    C = L // hop
    ae, le = PART
    Na, Nl = ae.size - 1, le.size - 1
    F = C * Na * Nl
    lib = _lib.load()
    st = S.WaveHistogramStream(L, R, H, ae, le, hop)
    buf = torch.zeros(R, L, dtype=torch.float64, device="cuda")
    ad, ld = torch.from_numpy(ae).cuda(), torch.from_numpy(le).cuda()
    hist = torch.full((2, R, F), ISENT, dtype=torch.int32, device="cuda")
    oc = torch.full((2, R, C), ISENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    good = dict(block=buf.data_ptr(), xs=L, a=ad.data_ptr(), sa=0, l=ld.data_ptr(), sl=0, c=hist[0].data_ptr(), s=hist[1].data_ptr(), hs=F,
                o=oc[0].data_ptr(), v=oc[1].data_ptr(), cs=C)

    def push(**kw):
        g = dict(good, **kw)
        return st.push_dev(g["block"], g["xs"], g["a"], g["sa"], g["l"], g["sl"], g["c"], g["s"], g["hs"], g["o"], g["v"], g["cs"])

    assert not push(a=None, l=None, c=None, s=None, o=None, v=None)       # nothing is emitted yet: only the block is needed
    assert st.blocks_held == 1
    bad = (dict(block=None), dict(xs=L - 1), dict(a=None), dict(l=None), dict(c=None), dict(s=None), dict(sa=Na), dict(sl=Nl), dict(sa=-1),
           dict(hs=F - 1), dict(cs=C - 1))
    for kw in bad:
        with pytest.raises(ITDError) as err:
            push(**kw)
        assert err.value.status == INVALID_ARG, kw
        assert st.blocks_held == 1, kw
    torch.cuda.synchronize()
    assert bool((hist == ISENT).all()) and bool((oc == ISENT).all())
    assert push(o=None, v=None, cs=0) and st.blocks_held == 1             # NULL counts need no stride
    # the other kinds' entries refuse it, and its entries the other kinds
    f64 = torch.zeros(R, L, dtype=torch.float64, device="cuda")
    assert lib.itd_stream_push_f64(st._h, buf.data_ptr(), L, f64.data_ptr(), L, None, 0, None, None) == INVALID_ARG
    assert lib.itd_wave_stream_push_f64(st._h, buf.data_ptr(), L, ad.data_ptr(), 0, f64.data_ptr(), L, None, None) == INVALID_ARG
    assert lib.itd_spectrum_stream_flush_f64(st._h, ad.data_ptr(), 0, f64.data_ptr(), L, None, None, 0, None, None) == INVALID_ARG
    assert lib.itd_inst_stream_flush_f64(st._h, f64.data_ptr(), None, None, None, L, None, 0, None, None) == INVALID_ARG
    assert lib.itd_wave_stream_latency(st._h) == -1 and lib.itd_spectrum_stream_latency(st._h) == -1
    wf = S.WaveFilterStream(L, R, H)
    assert lib.itd_hist_stream_latency(wf._h) == -1
    assert lib.itd_hist_stream_push_f64(wf._h, buf.data_ptr(), L, ad.data_ptr(), 0, ld.data_ptr(), 0, hist[0].data_ptr(), hist[1].data_ptr(),
                                        F, None, None, 0, None, None) == INVALID_ARG
    assert lib.itd_hist_stream_flush_f64(wf._h, ad.data_ptr(), 0, ld.data_ptr(), 0, hist[0].data_ptr(), hist[1].data_ptr(), F, None, None, 0,
                                         None, None) == INVALID_ARG
    wf.close()
    torch.cuda.synchronize()
    st.close()


# ---- 6. the ring contract -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hk", range(4))
def test_latency_emission_flush_refusal_restart_and_reset(S, hk):
    import torch
    from pyitd_amd import ITDError
    L, hop, R = 64, 64, 2
    H = (1, L - 1, L, L + 1)[hk]
    D = latency(L, H, reach=0)
    assert D == (1 if H <= L else 2)
    ae, le = PART
    rng = np.random.default_rng(600 + hk)
    x = enveloped_signals(rng, L, H, R, D + 2)
    n = D + 2

    def run(st, x, between=None):
        blocks, outs, held = x.shape[1] // L, [], 0
        assert st.blocks_held == 0
        for p in range(blocks):
            r = st.push(x[:, p * L:(p + 1) * L])
            assert (r is None) == (p < D), "push %d of a stream with latency %d" % (p, D)
            outs += [r] if r is not None else []
            held += r is None
            assert st.blocks_held == held == min(p + 1, D)
        for k in range(min(blocks, D)):                                   # exactly min(pushed, D) flushes emit
            if k == 1 and between:
                between()
            r = st.flush()
            assert r is not None, "flush %d of %d" % (k, min(blocks, D))
            outs.append(r)
            held -= 1
            assert st.blocks_held == held
        assert st.flush() is None and st.flush() is None and st.blocks_held == 0
        assert len(outs) == blocks
        return tuple(np.concatenate([o[i] for o in outs], axis=1) for i in range(4))

    st = S.WaveHistogramStream(L, R, H, ae, le, hop)
    assert st.latency == D and st.flush() is None and st.blocks_held == 0
    want = expected(x, L, H, ae, le, hop)
    hsr.same_ints(run(st, x), want, "a fresh stream")
    for short in (1, D):                                                  # shorter streams: min(pushed, D) = pushed
        hsr.same_ints(run(st, x[:, :short * L]), expected(x[:, :short * L], L, H, ae, le, hop), "%d blocks" % short)
    buf = torch.zeros(R, L, dtype=torch.float64, device="cuda")
    ad, ld = torch.from_numpy(ae).cuda(), torch.from_numpy(le).cuda()
    out = torch.zeros(2, R, 64, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    refused = []

    def push_between():
        held = st.blocks_held
        with pytest.raises(ITDError) as err:
            st.push_dev(buf.data_ptr(), L, ad.data_ptr(), 0, ld.data_ptr(), 0, out[0].data_ptr(), out[1].data_ptr(), 64)
        assert err.value.status == INVALID_ARG
        with pytest.raises(ITDError):
            st.push(x[:, :L])
        assert st.blocks_held == held
        refused.append(held)

    hsr.same_ints(run(st, x, push_between), want, "with a refused push in the flush")
    assert refused == ([D - 1] if D >= 2 else [])
    hsr.same_ints(run(st, x), want, "the same object after its drain")
    for p in range(n):                                                    # reset in mid-stream, blocks emitted and blocks held
        st.push(x[:, p * L:(p + 1) * L])
    assert st.blocks_held == D
    st.reset()
    assert st.blocks_held == 0 and st.flush() is None
    hsr.same_ints(run(st, x), want, "after reset")
    st.close()


# ---- 7., 8. edges that move, a NaN -----------------------------------------------------------------------------------------------------------
def test_edges_changed_between_two_pushes_are_followed_from_the_next_block(S):
    L, H, hop, R, blocks = 128, 100, 64, 2, 6
    C = L // hop
    rng = np.random.default_rng(12)
    x = enveloped_signals(rng, L, H, R, blocks)
    (a0, l0), (a1, l1) = PART, (PART[0] * 0.5, PART[1] + 1.0)
    w0, w1 = expected(x, L, H, a0, l0, hop), expected(x, L, H, a1, l1, hop)
    st = S.WaveHistogramStream(L, R, H, a0, l0, hop)
    outs = []
    for p in range(blocks):
        r = st.push(x[:, p * L:(p + 1) * L], *((a1, l1) if p == 3 else ()))      # from push 3 on: block 3 - D = 2 is the first under them
        if r is not None:
            outs.append(r)
    while (r := st.flush()) is not None:
        outs.append(r)
    st.close()
    got = tuple(np.concatenate([o[i] for o in outs], axis=1) for i in range(4))
    cut = (3 - latency(L, H, 0)) * C
    hsr.same_ints(got, tuple(np.concatenate((a[:, :cut], b[:, cut:]), axis=1) for a, b in zip(w0, w1)), "edges moved at push 3")
    assert not np.array_equal(w0[0][:, cut:], w1[0][:, cut:])


def test_a_nan_sets_the_status_and_leaves_the_other_rows_exact(S):
    L, H, hop, blocks = 64, 100, 64, 8
    rng = np.random.default_rng(5)
    x = signals(rng, L, H, blocks)
    want = expected(x, L, H, *PART, hop)
    x[1, 3 * L + 7] = np.nan
    st = S.WaveHistogramStream(L, 3, H, *PART, hop)
    got, _, _ = run_stream(st, x)
    assert st.status() & 2
    hsr.same_ints(tuple(g[[0, 2]] for g in got), tuple(w[[0, 2]] for w in want), "the rows without the NaN")
    st.reset()
    assert st.status() == 0
    st.close()


# ---- 9. the chain ----------------------------------------------------------------------------------------------------------------------------------
def test_behind_a_levels_stream_on_device_pointers(S):
    """the levels stream's emitted rows go into the histogram stream by pointer, on one stream, with no host copy in between; the result
    is the numpy rule on the rows the levels stream emitted"""
    import torch
    L, M, Cn, nb, H, hop = 512, 3, 2, 8, 300, 256
    R, C = Cn * (M + 1), L // hop
    rng = np.random.default_rng(31)
    t = np.arange(nb * L) / (nb * L)
    x = np.stack([fuzz_signal(rng, 0, nb * L), 3.0 * np.sin(2 * np.pi * 4 * t + 0.3) + 0.1 * rng.standard_normal(nb * L)])
    ae, le = np.concatenate(([0.0], np.geomspace(1e-3, 3.0, 8))), np.array([1.0, 2.0, 4.0, 8.0, 32.0, 128.0, 300.0])
    Na, Nl = ae.size - 1, le.size - 1
    F = C * Na * Nl
    lv = S.LevelsStream(L, M, Cn)
    hs = S.WaveHistogramStream(L, R, H, ae, le, hop)
    assert hs.latency == 1
    xd, ad, ld = torch.from_numpy(x).cuda(), torch.from_numpy(ae).cuda(), torch.from_numpy(le).cuda()
    rows = torch.zeros(nb, Cn, M + 1, L, dtype=torch.float64, device="cuda")
    hist = torch.zeros(2, nb + 1, R, F, dtype=torch.int32, device="cuda")            # (+1: the pointer of the flush that finds it empty)
    oc = torch.zeros(2, nb + 1, R, C, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream().cuda_stream
    torch.cuda.synchronize()
    k = o = 0
    args = lambda o: (ad.data_ptr(), 0, ld.data_ptr(), 0, hist[0, o].data_ptr(), hist[1, o].data_ptr(), F, oc[0, o].data_ptr(),
                      oc[1, o].data_ptr(), C, s)
    for p in range(nb):
        if lv.push_dev(xd[:, p * L:].data_ptr(), nb * L, rows[k].data_ptr(), L, (M + 1) * L, None, s):
            o += hs.push_dev(rows[k].data_ptr(), L, *args(o))
            k += 1
    while lv.flush_dev(rows[min(k, nb - 1)].data_ptr(), L, (M + 1) * L, None, s):
        o += hs.push_dev(rows[k].data_ptr(), L, *args(o))
        k += 1
    while hs.flush_dev(*args(o)):
        o += 1
    torch.cuda.synchronize()
    assert k == nb and o == nb
    streamed = rows.cpu().numpy().transpose(1, 2, 0, 3).reshape(R, nb * L)        # the concatenated rows the second stage saw
    h, c = hist[:, :nb].cpu().numpy(), oc[:, :nb].cpu().numpy()
    cells = h.reshape(2, nb, R, C, Na, Nl).transpose(0, 2, 1, 3, 4, 5).reshape(2, R, nb * C, Na, Nl)
    cnt = c.transpose(0, 2, 1, 3).reshape(2, R, nb * C)
    want = expected(streamed, L, H, ae, le, hop)
    hsr.same_ints((cells[0], cells[1], cnt[0], cnt[1]), want, "levels stream -> histogram stream")
    assert want[0].sum() > 0 and want[3].any()
    assert lv.status() == 0 and hs.status() == 0
    lv.close()
    hs.close()


# ---- 10. order of calls ------------------------------------------------------------------------------------------------------------------------------
def test_other_calls_on_the_device_between_its_pushes_change_nothing(P, S):
    L, H, hop, blocks = 512, 700, 512, 5
    rng = np.random.default_rng(23)
    x = signals(rng, L, H, blocks)
    alone = S.WaveHistogramStream(L, 3, H, *PART, hop)
    want, _, _ = run_stream(alone, x)
    alone.close()
    st = S.WaveHistogramStream(L, 3, H, *PART, hop)
    wf = S.WaveFilterStream(L, 3, H)
    outs = []
    for p in range(blocks):
        r = st.push(x[:, p * L:(p + 1) * L])
        outs += [r] if r is not None else []
        P.wave_histogram(x, COVER[0], COVER[1], 512)                      # a whole-row call and another ring stream in between
        wf.push(x[:, p * L:(p + 1) * L], amplitude=(0.2, 2.0))
    while (r := st.flush()) is not None:
        outs.append(r)
        wf.flush(amplitude=(0.2, 2.0))
    st.close()
    wf.close()
    got = tuple(np.concatenate([o[i] for o in outs], axis=1) for i in range(4))
    hsr.same_ints(got, want, "with other calls in between")
    hsr.same_ints(want, expected(x, L, H, *PART, hop), "alone")
