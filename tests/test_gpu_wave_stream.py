"""The wave-filter stream on the GPU (itd_wave_stream_*, pyitd_amd.streaming.WaveFilterStream / blockwise_wave_filter) against the
whole-row statement tests/waves_ref.ref_filter with the upper length bound capped at the horizon — bit for bit, +0.0 and -0.0
told apart — with the emission pattern [p >= D] and min(P, D) emitting flushes; against pyitd_amd.wave_filter on the GPU; and
behind a LevelsStream on device pointers."""
import numpy as np
import pytest

from helpers import assert_bits_equal, fuzz_signal
from ring_stream_runs import latency as ring_latency, push_and_flush
from waves_ref import ref_filter, ref_table
from wave_stream_ref import run_length_signal

pytestmark = pytest.mark.gpu

INF = np.inf
COPY = (0.0, INF, 0.0, INF)
SHAPES = [(8, 1), (8, 8), (64, 64), (64, 65), (100, 37), (512, 700), (1000, 3000), (1024, 5000), (8192, 64), (8192, 8193)]
# latencies above 64 blocks: the searches step over the blocks' records in more than one round of 64
SHAPES += [(8, 600), (24, 3001)]


@pytest.fixture(scope="module")
def S():
    from pyitd_amd import streaming
    return streaming


def latency(L, H):
    return ring_latency(L, H, reach=0)


def capped(bounds, H):
    b = np.array(bounds, dtype=np.float64)
    b[..., 3] = np.where(np.isnan(b[..., 3]), b[..., 3], np.minimum(b[..., 3], float(H)))
    return b


def reference(x, bounds, H):
    """ref_filter of every row with len_hi -> min(len_hi, H); bounds [4] or [rows, 4]"""
    b = np.broadcast_to(capped(bounds, H), (x.shape[0], 4))
    return np.stack([ref_filter(x[r], tuple(b[r])) for r in range(x.shape[0])])


def run_stream(st, x, bounds):
    """push every block, flush until empty: (output, the pushes' emission pattern, the flushes that emitted)"""
    outs, pattern, flushed = push_and_flush(st, x, (bounds,), (bounds,))
    return np.concatenate(outs, axis=1), pattern, flushed


def signals(rng, L, H, rows, blocks):
    """(x[rows, blocks L], the constructed rows): two of every three rows are run-length signals (every other one with exact
    zeros), the third a fuzz_signal of kind 0, 1 or 4"""
    x, constructed = [], []
    for r in range(rows):
        if r % 3 == 2:
            x.append(fuzz_signal(rng, (0, 1, 4)[(r // 3) % 3], blocks * L))
        else:
            constructed.append(r)
            x.append(run_length_signal(rng, L, H, blocks, zeros=(r % 3 == 1)))
    return np.stack(x), constructed


# amplitude windows that split run_length_signal's three amplitudes 0.25, 1.0, 3.0: each keeps and zeroes one of the three one-sample
# half waves every constructed row opens with, in every stream however short
WINDOWS = ((0.2, 2.0), (0.5, INF), (0.0, 0.5))


def bound_sets(L, H, rows, i):
    """the bounds a stream is run under: one set for all rows, one set per row (len_hi through inf, H, H // 2 along the rows and
    the runs, the amplitude windows in turn, len_lo 0 or 1 on the constructed rows), the copy set"""
    his = (INF, float(H), float(H // 2))
    shared = np.array([0.2, 2.0, 0.0, his[i % 3]])
    per_row = np.array([list(WINDOWS[(r + r // 3) % 3]) + [float(r % 3), his[(i + 1 + r) % 3]] for r in range(rows)])
    return [("shared", shared), ("per row", per_row), ("copy", np.array(COPY))]


def check_constructed(x, constructed, want, bounds, name, L, H):
    """On the reference alone, for every constructed row under every set of bounds: it holds kept samples and zeroed samples (a
    case that keeps or zeroes everything shows nothing), and where 2 H + 7 samples fit a half wave of exactly H and one of H + 1
    samples.  Two combinations cannot hold both and are named here, and only they are let off:
      * len_hi = H // 2 = 0 (H = 1): no half wave has length 0, the filter keeps nothing by definition;
      * the copy set — under the cap 'everything of length <= H' — on a row without a half wave longer than H: nothing can be
        zeroed.  Every constructed row of at least H + 6 samples holds such a half wave."""
    n = x.shape[1]
    b = np.broadcast_to(bounds, (x.shape[0], 4))
    for r in constructed:
        lengths = ref_table(x[r])[1]
        if n >= 2 * H + 7:
            assert (lengths == H).any() and (lengths == H + 1).any(), "row %d: no half wave of length H / H + 1" % r
        has_long = bool((lengths > H).any())
        assert has_long or n < H + 6, "row %d of %d samples holds no half wave longer than H = %d" % (r, n, H)
        kept = np.count_nonzero(want[r])
        zeroed = np.count_nonzero((want[r] == 0) & (x[r] != 0))
        what = "row %d under the %s bounds %s shows nothing: %d kept, %d zeroed" % (r, name, b[r], kept, zeroed)
        assert kept or b[r, 3] < 1.0, what
        assert zeroed or (name == "copy" and not has_long), what


@pytest.mark.parametrize("rows", [1, 3, 9])
@pytest.mark.parametrize("L,H", SHAPES)
def test_the_stream_is_the_capped_whole_row_filter(S, L, H, rows):
    D = latency(L, H)
    rng = np.random.default_rng(L * 100003 + H * 101 + rows)
    st = S.WaveFilterStream(L, rows, H)
    assert st.latency == D
    long_enough = False
    for i, blocks in enumerate(sorted({1, D, D + 1, 3 * (2 * D + 1) + 1})):
        x, constructed = signals(rng, L, H, rows, blocks)
        long_enough |= x.shape[1] >= 2 * H + 7
        for name, bounds in bound_sets(L, H, rows, i):
            want = reference(x, bounds, H)
            check_constructed(x, constructed, want, bounds, name, L, H)
            got, pattern, flushed = run_stream(st, x, bounds)             # (the stream is reused: it starts afresh after its flush)
            what = "L=%d H=%d rows=%d blocks=%d bounds=%s" % (L, H, rows, blocks, name)
            assert pattern == [p >= D for p in range(blocks)], what
            assert flushed == min(blocks, D), what
            assert_bits_equal(got, want, what)
    assert long_enough, "the longest stream holds half waves of length H and H + 1"
    assert st.status() == 0
    st.close()


@pytest.mark.parametrize("L,H", [(64, 64), (100, 37), (1024, 5000)])
def test_with_len_hi_within_the_horizon_it_is_wave_filter_on_the_gpu(S, L, H):
    import pyitd_amd
    D = latency(L, H)
    rng = np.random.default_rng(L + H)
    x, _ = signals(rng, L, H, 5, 2 * D + 3)
    len_hi = np.array([H, H // 2, H, 3, H - 1], dtype=np.float64)
    got = S.blockwise_wave_filter(x, L, H, amplitude=(0.2, 2.0), length=(1.0, len_hi))
    want = pyitd_amd.wave_filter(x, amplitude=(0.2, 2.0), length=(1.0, len_hi))
    assert_bits_equal(got, want, "L=%d H=%d" % (L, H))
    assert np.count_nonzero(want) and np.count_nonzero((want == 0) & (x != 0))


def test_behind_a_levels_stream_on_device_pointers(S):
    """samples in, feature-filtered components out: the levels stream's emitted rows go into the wave-filter stream by pointer, on
    one stream, with no host copy in between"""
    import torch
    L, M, C, nb, H = 1024, 4, 2, 12, 2048
    R = C * (M + 1)
    rng = np.random.default_rng(31)
    x = np.stack([fuzz_signal(rng, k, nb * L) for k in (0, 4)])
    lv = S.LevelsStream(L, M, C)
    wf = S.WaveFilterStream(L, R, H)
    assert wf.latency == 2
    bounds = np.array([[0.0 if r % 2 else 0.05, INF, 0.0, (INF, float(H), 300.0)[r % 3]] for r in range(R)])
    xd = torch.from_numpy(x).cuda()
    bd = torch.from_numpy(bounds).cuda()
    rows = torch.zeros(nb, C, M + 1, L, dtype=torch.float64, device="cuda")      # what the levels stream emitted, block by block
    out = torch.zeros(nb + 1, R, L, dtype=torch.float64, device="cuda")          # (+1: the pointer of the flush that finds it empty)
    ts = torch.cuda.Stream()                                                     # one stream of the caller's for both stages
    s = ts.cuda_stream
    torch.cuda.synchronize()
    k = o = 0

    def filter_block(k, o):
        return o + (1 if wf.push_dev(rows[k].data_ptr(), L, bd.data_ptr(), 4, out[o].data_ptr(), L, s) else 0)

    for p in range(nb):
        if lv.push_dev(xd[:, p * L:].data_ptr(), nb * L, rows[k].data_ptr(), L, (M + 1) * L, None, s):
            o = filter_block(k, o)
            k += 1
    while lv.flush_dev(rows[min(k, nb - 1)].data_ptr(), L, (M + 1) * L, None, s):
        o = filter_block(k, o)
        k += 1
    while wf.flush_dev(bd.data_ptr(), 4, out[o].data_ptr(), L, s):
        o += 1
    torch.cuda.synchronize()
    assert k == nb and o == nb
    streamed = rows.cpu().numpy().transpose(1, 2, 0, 3).reshape(R, nb * L)       # the concatenated rows the second stage saw
    got = out[:nb].cpu().numpy().transpose(1, 0, 2).reshape(R, nb * L)
    want = reference(streamed, bounds, H)
    assert_bits_equal(got, want, "levels stream -> wave-filter stream")
    assert np.count_nonzero(want) and np.count_nonzero((want == 0) & (streamed != 0))
    assert lv.status() == 0 and wf.status() == 0
    lv.close()
    wf.close()


def test_two_live_streams_with_different_blocks_and_the_shape_of_what_leaves(S):
    """A stream with a shorter block made while one with the longest block lives (both run the kernel's 1024-thread instance) does
    not take the LDS from under it; and with one row the blocks that leave, by push or by flush, are shaped like the last push's."""
    H = 64
    rng = np.random.default_rng(17)
    big = S.WaveFilterStream(8192, 1, H)
    small = S.WaveFilterStream(4096, 1, H)
    bounds = np.array([0.2, 2.0, 0.0, INF])
    xs, _ = signals(rng, 4096, H, 1, 3)
    xb, _ = signals(rng, 8192, H, 1, 3)
    got_s, _, _ = run_stream(small, xs, bounds)                           # 2-D blocks in: 2-D blocks out, the flush's too
    assert got_s.shape == (1, 3 * 4096)
    assert_bits_equal(got_s, reference(xs, bounds, H), "the shorter block")
    outs = [r for p in range(3) if (r := big.push(xb[0, p * 8192:(p + 1) * 8192], bounds)) is not None]
    outs.append(big.flush(bounds))
    assert all(o.shape == (8192,) for o in outs) and big.flush(bounds) is None
    assert_bits_equal(np.concatenate(outs), reference(xb, bounds, H)[0], "the longest block, after the shorter one's stream was made")
    small.close()
    big.close()


def test_reset_in_mid_stream_starts_afresh(S):
    L, H, rows, blocks = 100, 250, 3, 9
    rng = np.random.default_rng(8)
    x, _ = signals(rng, L, H, rows, blocks)
    bounds = np.array([0.2, 2.0, 0.0, INF])
    fresh = S.WaveFilterStream(L, rows, H)
    want, _, _ = run_stream(fresh, x, bounds)
    fresh.close()
    assert_bits_equal(want, reference(x, bounds, H), "a new object")
    st = S.WaveFilterStream(L, rows, H)
    y, _ = signals(rng, L, H, rows, 5)
    for p in range(5):                                                   # past the latency: blocks have been emitted
        st.push(y[:, p * L:(p + 1) * L], bounds)
    assert st.blocks_held == 3
    st.reset()
    assert st.blocks_held == 0
    got, pattern, flushed = run_stream(st, x, bounds)
    assert pattern == [p >= 3 for p in range(blocks)] and flushed == 3
    assert_bits_equal(got, want, "after reset")
    st.close()


def test_a_nan_sets_the_status_and_leaves_the_other_rows_exact(S):
    L, H, rows, blocks = 64, 100, 3, 8
    rng = np.random.default_rng(5)
    x, _ = signals(rng, L, H, rows, blocks)
    bounds = np.array([0.0, 2.0, 0.0, INF])
    want = reference(x, bounds, H)
    x[1, 3 * L + 7] = np.nan
    st = S.WaveFilterStream(L, rows, H)
    got, _, _ = run_stream(st, x, bounds)
    assert st.status() & 2
    assert_bits_equal(got[[0, 2]], want[[0, 2]], "the rows without the NaN")
    st.reset()
    assert st.status() == 0
    st.close()


def test_argument_errors_on_a_live_stream(S):
    import torch
    from pyitd_amd import ITDError, _lib
    L, H, rows = 64, 100, 2
    lib = _lib.load()
    st = S.WaveFilterStream(L, rows, H)
    blk = torch.zeros(rows, L, dtype=torch.float64, device="cuda")
    out = torch.zeros(rows, L, dtype=torch.float64, device="cuda")
    bd = torch.tensor(COPY, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                                             # (the stream's launches run on its own stream)
    for _ in range(2):                                                  # nothing is emitted yet: neither bounds nor an output is needed
        assert not st.push_dev(blk.data_ptr(), L, None, 0, None, 0)
    with pytest.raises(ITDError):                                        # this push emits: the output is required
        st.push_dev(blk.data_ptr(), L, bd.data_ptr(), 0, None, 0)
    with pytest.raises(ITDError):                                        # ... and the bounds
        st.push_dev(blk.data_ptr(), L, None, 0, out.data_ptr(), L)
    with pytest.raises(ITDError):                                        # a bounds stride of 1 .. 3
        st.push_dev(blk.data_ptr(), L, bd.data_ptr(), 3, out.data_ptr(), L)
    with pytest.raises(ITDError):                                        # strides below the block
        st.push_dev(blk.data_ptr(), L - 1, bd.data_ptr(), 0, out.data_ptr(), L)
    with pytest.raises(ITDError):
        st.push_dev(blk.data_ptr(), L, bd.data_ptr(), 0, out.data_ptr(), L - 1)
    assert st.blocks_held == 2
    # the other kinds' entries refuse a wave stream, and its entries the other kinds
    assert lib.itd_stream_push_f64(st._h, blk.data_ptr(), L, out.data_ptr(), L, None, 0, None, None) == 1
    assert lib.itd_stream_flush_f64(st._h, out.data_ptr(), L, None, 0, None, None) == 1
    assert lib.itd_levels_stream_push_f64(st._h, blk.data_ptr(), L, out.data_ptr(), L, L, None, None, None) == 1
    assert lib.itd_levels_stream_flush_f64(st._h, out.data_ptr(), L, L, None, None, None) == 1
    assert lib.itd_levels_stream_form(st._h) == -1
    lin = S.Stream(L, rows, "linear")
    assert lib.itd_wave_stream_latency(lin._h) == -1
    assert lib.itd_wave_stream_push_f64(lin._h, blk.data_ptr(), L, bd.data_ptr(), 0, out.data_ptr(), L, None, None) == 1
    lin.close()
    assert st.flush_dev(bd.data_ptr(), 0, out.data_ptr(), L)
    with pytest.raises(ITDError):                                        # no push once a flush has begun
        st.push_dev(blk.data_ptr(), L, bd.data_ptr(), 0, out.data_ptr(), L)
    with pytest.raises(ITDError):
        st.push(np.zeros((rows, L)), np.array(COPY))
    assert st.flush_dev(bd.data_ptr(), 0, out.data_ptr(), L)
    assert not st.flush_dev(bd.data_ptr(), 0, out.data_ptr(), L)         # empty: the stream starts afresh
    assert not st.push_dev(blk.data_ptr(), L, None, 0, None, 0)
    torch.cuda.synchronize()
    st.close()
