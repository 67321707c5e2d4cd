"""The levels stream (k_stream_levels / k_levels_route, levels_step*, streaming.LevelsStream) on its hard inputs, against the plain-rules
reference tests/levels_plain_ref.plain_composition — numpy over oracle/stream_oracle.py and oracle/numpy_itd.py, no device code and
none of the C oracle (tests/test_levels_plain_cpu.py anchors it).  Every comparison is bit for bit (any NaN equals any NaN); the flags
and status() exactly; through the one-launch form and the forced sequence form wherever three blocks fit 8192 samples.

  * the soundness fuzz grid of test_levels_plain_cpu.py (six families x NaN / infinity / leading plateau / clean), one stream per
    (L, M) reused after its flush; certified blocks against the whole-signal oracle;
  * block lengths either side of every size class of the one-launch kernel, dense (alternating) input, 1 / 2 / 4 blocks;
  * extreme values; 21 levels; 200 blocks, twice; 65535 channels; a form switch on a live stream; the device form's strides."""
import numpy as np
import pytest

from helpers import assert_bits_equal, fuzz_signal
from levels_plain_ref import (EDGE_BLOCK, EDGE_CASES, EDGE_L, certified_against_whole, edge_signal, grid_cells, grid_draws,
                              plain_composition)

pytestmark = pytest.mark.gpu

GPU_DRAWS, MIN_COMPARED = 40, 10


@pytest.fixture(scope="module")
def S():
    from pyitd_amd import streaming
    return streaming


def drain(st, x):
    """every block of x[C, n] through st.push, then st.flush until empty (st stays open: it has started afresh);
    (rows[C, M+1, n], exact[C, n_blocks], status), latency asserted"""
    L, M = st.block, st.levels
    nb = x.shape[1] // L
    outs = []
    for k in range(nb):
        r = st.push(x[:, k * L:(k + 1) * L])
        assert (r is not None) == (k >= M + 1), "latency: push %d" % k
        if r is not None:
            outs.append(r)
    while (r := st.flush(flat=False)) is not None:
        outs.append(r)
    assert len(outs) == nb and st.blocks_held == 0
    return np.concatenate([o[0] for o in outs], axis=2), np.stack([o[1] for o in outs], axis=1), st.status()


def hold(st, x, ref, what):
    """st's results on x are ref = plain_composition(x, L, M); a status of 2 is cleared for the stream's next use"""
    rows, exact, status = drain(st, x)
    if status:
        st.reset()                             # (t = 0 and P = -1 already, by the flush: this clears the recorded status alone)
    assert_bits_equal(rows, ref[0], what + " rows (%s)" % st.form)
    np.testing.assert_array_equal(exact, ref[1], what + " flags (%s)" % st.form)
    assert status == ref[2], what + " status (%s)" % st.form
    return rows, exact


@pytest.fixture(scope="module")
def pool(S):
    """one single-channel stream per (L, M, form), kept across the draws and cells of the grid"""
    streams = {}

    def get(L, M, sequence):
        if (L, M, sequence) not in streams:
            st = S.LevelsStream(L, M, 1)
            if sequence:
                st.force_sequence()
            streams[L, M, sequence] = st
        st = streams[L, M, sequence]
        assert st.form == ("sequence" if sequence else "one-launch")
        return st

    yield get
    for st in streams.values():
        st.close()


def both_forms(S, L, M, C):
    for sequence in (False, True):
        st = S.LevelsStream(L, M, C)
        if sequence:
            st.force_sequence()
        assert st.form == ("sequence" if sequence else "one-launch")
        yield st
        st.close()


# ---- the fuzz grid ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", grid_cells())
def test_fuzz_grid_rows_flags_status_and_certified_blocks(pool, kind, mode):
    timeouts = compared = 0
    for i, (x, L, M) in enumerate(grid_draws(kind, mode, GPU_DRAWS)):
        ref = plain_composition(x, L, M)
        what = "kind %d mode %s draw %d (L=%d M=%d blocks=%d)" % (kind, mode, i, L, M, len(x) // L)
        for sequence in (False, True):
            rows, exact = hold(pool(L, M, sequence), x[None], ref, what)
        ended, n_cert, unsound = certified_against_whole(x, L, M, rows[0], exact[0])
        assert not unsound, what + ": certified blocks %s differ from the whole signal" % unsound
        timeouts += ended
        compared += n_cert
    print("levels grid kind %d mode %-7s: %d of %d draws end 'timeout', %d certified blocks compared" % (kind, mode, timeouts, GPU_DRAWS, compared))
    assert compared >= MIN_COMPARED


def test_known_answers_at_the_rules_edges(S):
    """the hand-built windows of test_levels_plain_cpu.py, one per channel: a block whose stage-0 window misses rule (c) or (d)
    is not certified, and everything equals the reference"""
    x = np.stack([edge_signal(knots) for knots, _ in EDGE_CASES])
    ref = plain_composition(x, EDGE_L, 1)
    for st in both_forms(S, EDGE_L, 1, len(EDGE_CASES)):
        rows, exact = hold(st, x, ref, "rule edges")
        for c, (knots, expected) in enumerate(EDGE_CASES):
            assert expected or not exact[c, EDGE_BLOCK], knots


# ---- block lengths either side of the one-launch kernel's size classes (3L at 256 / 512 / 1024 / 2048 / 4096), and the ends ------
BOUNDARY_L = (64, 85, 86, 128, 170, 171, 341, 342, 682, 683, 1365, 1366, 2729, 2730)


@pytest.mark.parametrize("M", (1, 4))
@pytest.mark.parametrize("L", BOUNDARY_L)
def test_block_lengths_at_the_class_boundaries(S, L, M):
    rng = np.random.default_rng(L * 10 + M)
    xs = {nb: np.stack([fuzz_signal(rng, 6, nb * L), fuzz_signal(rng, 0, nb * L)]) for nb in (1, 2, 4)}
    refs = {nb: plain_composition(x, L, M) for nb, x in xs.items()}
    for st in both_forms(S, L, M, 2):
        for nb in (1, 2, 4):                   # the lone block, the two-block first window, a three-block window
            assert refs[nb][2] == 0
            hold(st, xs[nb], refs[nb], "L=%d M=%d blocks=%d" % (L, M, nb))


# ---- extreme values ---------------------------------------------------------------------------------------------------------
def extreme_rows(L, nb):
    n = L * nb
    rng = np.random.default_rng(77)
    noise = rng.standard_normal(n)
    zeros_in = rng.standard_normal(n)
    zeros_in[rng.integers(0, n, n // 5)] = -0.0
    zeros_in[L - 3:L + 4] = 0.0
    zeros_in[L + 1] = -0.0
    one = np.full(n, 0.75)
    one[2 * L + 17] = -3.0
    return np.stack([
        np.ldexp(noise, 1000),                 # near-overflow: sums of two samples may leave the range
        np.ldexp(noise, -1000),
        np.ldexp(noise, -1060),                # subnormal samples and baselines
        np.zeros(n),
        zeros_in,                              # -0.0 and a plateau of zeros of both signs across a block edge
        rng.standard_normal(n).astype(np.float32).astype(np.float64),
        one,                                   # constant except one sample
        np.cumsum(rng.random(n) + 0.01),       # monotone: no interior knot at any stage
    ])


def test_extreme_values(S):
    L, M, nb = 100, 3, 6
    x = extreme_rows(L, nb)
    ref = plain_composition(x, L, M)
    for st in both_forms(S, L, M, x.shape[0]):
        hold(st, x, ref, "extreme values")


# ---- depth, length, channels ----------------------------------------------------------------------------------------------------
def test_twenty_one_levels(S):
    """deep stages run on windows without an interior knot; the delay line holds 231 blocks per channel"""
    L, M, nb = 64, 21, 26
    rng = np.random.default_rng(21)
    x = np.stack([fuzz_signal(rng, 6, nb * L), fuzz_signal(rng, 0, nb * L)])
    ref = plain_composition(x, L, M)
    for st in both_forms(S, L, M, 2):
        hold(st, x, ref, "M=21")


def test_two_hundred_blocks_twice(S):
    """j % D, b % 4 and arr % 3 wrap many times; the second run goes through the same object after its flush"""
    L, M, nb = 8, 8, 200
    x = fuzz_signal(np.random.default_rng(200), 0, nb * L)[None]
    ref = plain_composition(x, L, M)
    for st in both_forms(S, L, M, 1):
        hold(st, x, ref, "200 blocks, first run")
        hold(st, x, ref, "200 blocks, second run")


@pytest.mark.parametrize("C,L,M,nb", [(65535, 8, 1, 4), (700, 64, 3, 5)])
def test_many_channels(S, C, L, M, nb):
    """16 distinct signals tiled across the channels, four of them holding a NaN: every channel equals its tile's reference"""
    rng = np.random.default_rng(C)
    x16 = np.stack([fuzz_signal(rng, (0, 4, 6, 2)[i % 4], nb * L) for i in range(16)])
    for i in (1, 6, 11, 12):
        x16[i, rng.integers(0, nb * L)] = np.nan
    rows16, exact16, status16 = plain_composition(x16, L, M)
    assert status16 == 2
    tile = np.arange(C) % 16
    x = x16[tile]
    for st in both_forms(S, L, M, C):
        rows, exact, status = drain(st, x)
        assert status == 2
        np.testing.assert_array_equal(exact, exact16[tile], "flags (%s)" % st.form)
        assert_bits_equal(rows, rows16[tile], "C=%d rows (%s)" % (C, st.form))


# ---- a form switch on a live stream -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start_sequence", (False, True))
def test_form_switch_on_a_live_stream(S, start_sequence):
    """Both forms keep the same ring, delay line and flag bytes, and itd_levels_stream_set_sequence takes a stream that holds
    blocks: toggling before every third step (pushes and flush steps alike) gives the bits of either pure form."""
    L, M, nb = 100, 4, 12
    x = fuzz_signal(np.random.default_rng(31), 4, nb * L)[None]
    x[0, 5 * L + 40] = np.nan
    ref = plain_composition(x, L, M)
    for st in both_forms(S, L, M, 1):          # the pure forms give the same bits: ref
        hold(st, x, ref, "pure form")
    st = S.LevelsStream(L, M, 1)
    sequence, step, outs = start_sequence, 0, []
    st.force_sequence(sequence)

    def toggle():
        nonlocal sequence, step
        if step % 3 == 2:
            sequence = not sequence
            st.force_sequence(sequence)
            assert st.form == ("sequence" if sequence else "one-launch")
        step += 1

    for k in range(nb):
        toggle()
        r = st.push(x[:, k * L:(k + 1) * L])
        if r is not None:
            outs.append(r)
    while True:
        toggle()
        if (r := st.flush(flat=False)) is None:
            break
        outs.append(r)
    assert step > nb + M and len(outs) == nb
    assert_bits_equal(np.concatenate([o[0] for o in outs], axis=2), ref[0], "switched rows")
    np.testing.assert_array_equal(np.stack([o[1] for o in outs], axis=1), ref[1])
    assert st.status() == ref[2] == 2
    st.close()


# ---- the device form: strides, gaps, guard, optional flags ----------------------------------------------------------------------
@pytest.mark.parametrize("sequence", (False, True))
def test_device_form_writes_only_what_it_is_given(S, sequence):
    import torch
    L, M, C, nb = 100, 3, 3, 9
    R, rs = M + 1, L + 7
    cs = R * rs + 5
    in_stride = L + 3
    rng = np.random.default_rng(44)
    x = np.stack([fuzz_signal(rng, k, nb * L) for k in (6, 0, 4)])
    x[1, 4 * L + 3] = np.nan
    ref = plain_composition(x, L, M)
    st = S.LevelsStream(L, M, C)
    if sequence:
        st.force_sequence()
    host_rows, host_exact = hold(st, x, ref, "host form")

    SENT, SENT8 = -1.2345e300, 0xA5
    xin = np.full((nb, C, in_stride), SENT)
    xin[:, :, :L] = x.reshape(C, nb, L).transpose(1, 0, 2)
    xin_d = torch.from_numpy(xin).cuda()
    out_d = torch.full((nb, C + 1, cs), SENT, dtype=torch.float64, device="cuda")         # (+1: a guard channel)
    exact_d = torch.full((nb, C + 1), SENT8, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    e = 0
    for k in range(nb):
        emits = k >= M + 1
        ex = exact_d[e].data_ptr() if emits and e % 2 == 0 else None                      # no flags on every other emitting step
        em = st.push_dev(xin_d[k].data_ptr(), in_stride, out_d[e].data_ptr() if emits else None, rs if emits else 0,
                         cs if emits else 0, ex, s)
        assert em == emits
        e += em
    while st.flush_dev(out_d[min(e, nb - 1)].data_ptr(), rs, cs, exact_d[e].data_ptr() if e < nb and e % 2 == 0 else None, s):
        e += 1
    assert e == nb and st.blocks_held == 0
    torch.cuda.synchronize()
    assert st.status() == 2
    st.close()

    out, flags = out_d.cpu().numpy(), exact_d.cpu().numpy()
    sent_bits = np.float64(SENT).view(np.uint64)
    body = out[:, :C, :R * rs].reshape(nb, C, R, rs)
    got = body[..., :L].transpose(1, 2, 0, 3).reshape(C, R, nb * L)
    assert_bits_equal(got, host_rows, "device rows against the host form's")
    assert_bits_equal(got, ref[0], "device rows")
    assert (body[..., L:].view(np.uint64) == sent_bits).all(), "the gaps between rows"
    assert (out[:, :C, R * rs:].view(np.uint64) == sent_bits).all(), "the gaps between channels"
    assert (out[:, C].view(np.uint64) == sent_bits).all(), "the guard channel"
    assert xin_d.cpu().numpy().tobytes() == xin.tobytes(), "the input and its gaps"
    np.testing.assert_array_equal(flags[0::2, :C].T.astype(bool), ref[1][:, 0::2])
    assert set(np.unique(flags[0::2, :C])) <= {0, 1}
    assert (flags[1::2] == SENT8).all(), "flags nobody asked for"
    assert (flags[:, C] == SENT8).all(), "the flags' guard"
