"""The block-wise cubic stream (itd_stream_* with ITD_STREAM_CUBIC: k_stream_select, the cubic kernels on a sub-list of the
compaction's list, the ring) and the detected-knots form of the I/Q operator against their EXACT results (oracle/exact_stream.py,
oracle/exact_spline.iq) on the layouts of tests/stream_cases.py: knots exactly at the emitted block's ends, 3 against 4 selected
knots, clipped margins, block lengths on and off the evaluation's tile grid, selected lists longer than a sweep workgroup's
elements, every ring phase, own and shared knots.  tests/test_stream_exact_cpu.py holds the layouts to those conditions and shows
that the comparison raises on a side = "right", a margin + 1, a threshold of 3, a list offset by one, a 1e-11 bump at a sweep seam
and a block from the wrong ring slot.

Bound (tests/test_gpu_spline_exact.py's, per emitted block, S = max(|window|, |exact|), eps = 2^-52):
    max err(GPU) <= 4 max err(fp64 oracle) + 64 eps S;
a block the exact statement emits unchanged equals the input bit for bit, rotation exactly 0.  pytest -s prints the measured
err / (eps S) as RATIO lines.

A NaN (what the code does, include/pyitd_hip.h): a block whose knot-giving window — its own; channel 0's under shared knots —
holds a NaN is emitted unchanged with rotation 0; a NaN in ANY channel sets status 2 and makes the host forms return
ITD_ERR_NONFINITE from the first emitting call on.  Before k_stream_store reported NaNs, a NaN in a channel other than 0 under
shared knots set no status at all (the shared cases of test_nan_windows failed on `status() == 2` and on the return codes).
"""
import ctypes

import numpy as np
import pytest

import stream_cases as sc
from oracle import cpu_oracle, exact_spline as ex, exact_stream as es, iq_oracle, stream_oracle as so

pytestmark = pytest.mark.gpu
ITD_ERR_NONFINITE = 6


@pytest.fixture(scope="module")
def S():
    from pyitd_amd import streaming
    return streaming


@pytest.fixture(scope="module")
def P():
    import pyitd_amd
    return pyitd_amd


def _bits(a, b, what):
    """Bit equality, +0 == -0 (as tests/test_gpu_spline_exact.py's)."""
    a, b = np.ascontiguousarray(a) + 0.0, np.ascontiguousarray(b) + 0.0
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


def _device_run(S, x, L, margin, shared):
    """The device form: every push and the flush queued on the caller's stream, snapshots of the output buffers queued behind
    every push, ONE synchronisation at the end.  Strided rows, sentinels in the gaps and in the blocks not yet emitted.
    Returns (baseline, rotation, status)."""
    import torch
    C, n = x.shape
    nb = n // L
    xs, bs, rs = n + 5, n + 3, n + 7
    xh = np.full((C, xs), sc.SENT)
    xh[:, :n] = x
    xd = torch.from_numpy(xh).cuda()
    base = torch.full((C, bs), sc.SENT, dtype=torch.float64, device="cuda")
    rot = torch.full((C, rs), sc.SENT, dtype=torch.float64, device="cuda")
    snap_b = torch.zeros((nb, C, bs), dtype=torch.float64, device="cuda")
    snap_r = torch.zeros((nb, C, rs), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ts = torch.cuda.Stream()
    st = S.Stream(L, C, "cubic", margin, shared)
    try:
        with torch.cuda.stream(ts):
            for k in range(nb):
                o = max(k - 1, 0) * L
                em = st.push_dev(xd[:, k * L:].data_ptr(), xs, base[:, o:].data_ptr(), bs, rot[:, o:].data_ptr(), rs, ts.cuda_stream)
                assert em == (k >= 1)
                snap_b[k].copy_(base, non_blocking=True)
                snap_r[k].copy_(rot, non_blocking=True)
            o = (nb - 1) * L
            assert st.flush_dev(base[:, o:].data_ptr(), bs, rot[:, o:].data_ptr(), rs, ts.cuda_stream)
        ts.synchronize()
        assert st.blocks_held == 0
        status = st.status()
    finally:
        st.close()
    bh, rh = base.cpu().numpy(), rot.cpu().numpy()
    assert np.all(bh[:, n:] == sc.SENT) and np.all(rh[:, n:] == sc.SENT), "the stride gaps are written"
    sb, sr = snap_b.cpu().numpy(), snap_r.cpu().numpy()
    for k in range(nb):                                     # after push k the blocks 0 .. k-2 and k-1 are out, nothing else
        assert np.all(sb[k][:, k * L:] == sc.SENT) and np.all(sr[k][:, k * L:] == sc.SENT), "push %d wrote ahead" % k
        _bits(sb[k][:, :k * L], bh[:, :k * L], "push %d: earlier blocks" % k)
    assert np.array_equal(xd.cpu().numpy().view(np.uint64), xh.view(np.uint64)), "the input is left alone"
    return bh[:, :n], rh[:, :n], status


# ---- every layout: host form, device form, power-of-two scaling ---------------------------------------------------------
@pytest.mark.parametrize("name", sc.names())
def test_stream_layouts(S, name):
    c = sc.case(name)
    x, L, margin, shared = c["x"], c["L"], c["margin"], c["shared"]
    blocks, ref = sc.exact(name), sc.oracle(name)
    got = S.blockwise(x, L, "cubic", margin, shared)
    sc.check("host/" + name, blocks, got, x, L, ref)
    base, rot, status = _device_run(S, x, L, margin, shared)
    assert status == 0
    sc.check("dev/" + name, blocks, base, x, L, ref, rot=rot)
    _bits(base, got, name + ": the two forms")
    for k in (400, -400):               # the knots and sweep_rcp's arguments do not depend on the scale: exact
        _bits(S.blockwise(np.ldexp(x, k), L, "cubic", margin, shared), np.ldexp(got, k), "%s 2^%d" % (name, k))


# ---- reuse ----------------------------------------------------------------------------------------------------------------
def _push_all(st, x, L):
    outs = []
    for k in range(x.shape[1] // L):
        r = st.push(x[:, k * L:(k + 1) * L])
        assert (r is None) == (k == 0)
        if r is not None:
            outs.append(r)
    outs.append(st.flush(flat=False))
    return np.concatenate(outs, axis=1)


def test_reuse_after_flush_and_reset(S):
    from pyitd_amd import ITDError
    first, second = "ring_noise_nb4", "ring_noise_nb3"
    L, margin = sc.case(first)["L"], sc.case(first)["margin"]
    st = S.Stream(L, 1, "cubic", margin)
    for name in (first, second):                            # flush empties the stream: the second run is exact again
        x = sc.case(name)["x"]
        sc.check("reuse/" + name, sc.exact(name), _push_all(st, x, L), x, L, sc.oracle(name))
        assert st.flush() is None and st.status() == 0
    bad = np.array(sc.case(first)["x"][:, :2 * L])
    bad[0, L + 3] = np.nan
    assert st.push(bad[:, :L]) is None
    with pytest.raises(ITDError) as err:
        st.push(bad[:, L:])
    assert err.value.status == ITD_ERR_NONFINITE and st.status() == 2 and st.blocks_held == 2
    st.reset()                                              # in mid-stream: starts afresh, clears the status
    assert st.status() == 0 and st.blocks_held == 0
    x = sc.case(second)["x"]
    sc.check("reset/" + second, sc.exact(second), _push_all(st, x, L), x, L, sc.oracle(second))
    assert st.status() == 0
    st.close()


# ---- NaN windows ------------------------------------------------------------------------------------------------------------
def _host_run_raw(S, x, L, margin, shared):
    """The host form through the ABI: (baseline, the return code of every call) — the wrapper raises and drops the block."""
    C, n = x.shape
    st = S.Stream(L, C, "cubic", margin, shared)
    out, rcs = np.full_like(x, sc.SENT), []
    try:
        for k in range(n // L + 1):
            blk = np.ascontiguousarray(x[:, k * L:(k + 1) * L]) if k < n // L else None
            base = np.full((C, L), sc.SENT)
            em = ctypes.c_int32(0)
            bp = base.ctypes.data_as(ctypes.c_void_p)
            if blk is not None:
                rcs.append(st._L.itd_stream_push_host_f64(st._h, blk.ctypes.data_as(ctypes.c_void_p), bp, None, ctypes.byref(em)))
            else:
                rcs.append(st._L.itd_stream_flush_host_f64(st._h, bp, None, ctypes.byref(em)))
            assert em.value == (1 if k >= 1 else 0)
            if em.value:
                out[:, (k - 1) * L:k * L] = base
        assert st.status() == (2 if any(rcs) else 0)
        st.reset()
        assert st.status() == 0
    finally:
        st.close()
    return out, rcs


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("where", [(2, 17), (0, 0), (6, 63)], ids=["block2", "first_sample", "last_sample"])
@pytest.mark.parametrize("channel", [0, 1])
@pytest.mark.parametrize("shared", [False, True], ids=["own", "shared"])
def test_nan_windows(S, shared, channel, where, form):
    L, nb, margin = 64, 7, 2
    x = np.random.default_rng(11).standard_normal((2, nb * L))
    b, s = where
    x[channel, b * L + s] = np.nan
    blocks = es.exact_blockwise_cubic(x, L, margin, shared)
    with np.errstate(all="ignore"):
        ref = so.oracle_blockwise_cubic(x, L, margin, shared)
    # what the statement says: the blocks whose window holds the NaN are unchanged where the knots come from that window
    hit = [j for j in range(nb) if abs(j - b) <= 1]
    for c in range(2):
        for j in range(nb):
            if j in hit and (c == channel or (shared and channel == 0)):
                assert blocks[c][j] is (es.UNSPECIFIED if shared and channel == 1 else None)
            else:
                assert isinstance(blocks[c][j], es.ExactBlock)
    what = "nan %s/%s ch%d b%d" % (form, "shared" if shared else "own", channel, b)
    if form == "host":
        got, rcs = _host_run_raw(S, x, L, margin, shared)
        sc.check(what, blocks, got, x, L, ref)
        # call k = push k (k < nb) or the flush; the NaN arrives with push b; the first emitting call is push 1
        assert rcs == [ITD_ERR_NONFINITE if k >= max(b, 1) else 0 for k in range(nb + 1)], rcs
    else:
        base, rot, status = _device_run(S, x, L, margin, shared)
        sc.check(what, blocks, base, x, L, ref, rot=rot)
        assert status == 2


# ---- the I/Q operator on detected common knots ------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [False, True], ids=["scaled", "extra_extrema"])
@pytest.mark.parametrize("n", sc.IQ_N)
def test_iq_detected_knots(P, n, extra):
    c = sc.iq_case(n, extra)
    I, Q = c["I"], c["Q"]
    z = I + 1j * Q
    e, idx = iq_oracle.extrema_iq(z)
    got, kn, gi = P.itd_baseline_extract_iq(z, want_knots=True)
    assert gi == idx == len(c["knots"])
    np.testing.assert_array_equal(kn, e[:idx])
    np.testing.assert_array_equal(kn, c["knots"])
    r = ex.iq(I, Q, e, idx)                                 # detect mode: the list's entry idx is 0
    ref = cpu_oracle.itd_baseline_extract_fast((I + Q) / 2.0, e, idx)
    S_ = r.scale(np.maximum(np.abs(I), np.abs(Q)))
    e_g, e_r = float(np.max(r.err(got))) / (sc.EPS * S_), float(np.max(r.err(ref))) / (sc.EPS * S_)
    print("RATIO %-40s gpu %9.3g  fp64 %9.3g  (eps S)" % ("iq detect/n%d%s" % (n, "_extra" if extra else ""), e_g, e_r))
    assert np.all(np.isfinite(got))
    assert e_g <= sc.C_REF * e_r + sc.C_ABS, (n, extra, e_g, e_r)
