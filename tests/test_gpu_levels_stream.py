"""The levels stream on the GPU (itd_levels_stream_*, pyitd_amd.streaming.LevelsStream / blockwise_itd) against
  * the composition of oracle_blockwise_linear, M+1 times, each on the previous baseline — bit for bit, every emitted block;
  * the numpy statement of the exactness rule in tests/test_levels_stream_cpu.py — the flags exactly;
  * the whole-signal oracle (oracle/cpu_oracle.itd(x, M-1)) on every certified block — bit for bit;
  * hand-chained single-level linear streams where a window holds a NaN, and beside them the plain-rules reference
    tests/levels_plain_ref.plain_composition (rows, flags and status, both forms)."""
import numpy as np
import pytest

from helpers import assert_bits_equal, fuzz_signal
from levels_plain_ref import plain_composition
from test_levels_stream_cpu import levels_composition, rich_signal, whole_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    from pyitd_amd import streaming
    return streaming


def run_stream(S, x, L, M, sequence=False):
    """push every block, flush until empty; returns (rows, exact, pushes that emitted, flushes that emitted, status)"""
    C, n = x.shape
    st = S.LevelsStream(L, M, C)
    if sequence:
        st.force_sequence()
    assert st.form == ("sequence" if sequence or 3 * L > 8192 else "one-launch")
    outs, pushed_em, flushed = [], [], 0
    for k in range(n // L):
        r = st.push(x[:, k * L:(k + 1) * L])
        pushed_em.append(r is not None)
        if r is not None:
            outs.append(r)
    while True:
        r = st.flush(flat=False)
        if r is None:
            break
        flushed += 1
        outs.append(r)
    assert st.blocks_held == 0
    status = st.status()
    st.close()
    rows = np.concatenate([o[0] for o in outs], axis=2)
    exact = np.stack([o[1] for o in outs], axis=1)
    return rows, exact, pushed_em, flushed, status


CASES = [(L, M, C) for L in (8, 24, 100, 512, 1000, 2730, 2731, 4096) for M in (1, 2, 5, 8) for C in (1, 3)]


def draws(rng, L, M, C):
    """the seeded streams of a case: 1, 2, M+1 and M+3 blocks (flush drains short and long streams)"""
    for nb in sorted({1, 2, M + 1, M + 3}):
        yield nb, np.stack([fuzz_signal(rng, (c + nb) % 5 if (c + nb) % 5 != 2 else 4, nb * L) for c in range(C)])


@pytest.mark.parametrize("L,M,C", CASES)
def test_rows_are_the_composition_and_flags_the_rule(S, L, M, C):
    rng = np.random.default_rng(L * 100 + M * 10 + C)
    for nb, x in draws(rng, L, M, C):
        rows, exact, pushed_em, flushed, status = run_stream(S, x, L, M)
        assert pushed_em == [k >= M + 1 for k in range(nb)], "latency"
        assert flushed == min(nb, M + 1)
        ref_rows, ref_exact, finite = levels_composition(x, L, M)
        assert finite, "draws are finite at every stage"
        assert status == 0
        assert_bits_equal(rows, ref_rows, "L=%d M=%d C=%d blocks=%d rows" % (L, M, C, nb))
        np.testing.assert_array_equal(exact, ref_exact, "flags L=%d M=%d C=%d blocks=%d" % (L, M, C, nb))
        for c in range(C):
            whole, stop = whole_rows(x[c], M)
            if stop != "timeout":
                continue
            for j in np.nonzero(exact[c])[0]:
                s = slice(j * L, (j + 1) * L)
                assert_bits_equal(rows[c][:, s], whole[:, s], "certified block %d" % j)


@pytest.mark.parametrize("L,M,C", [c for c in CASES if c[0] <= 2730])
def test_forced_sequence_form_equals_the_one_launch_form(S, L, M, C):
    rng = np.random.default_rng(L * 100 + M * 10 + C)
    for nb, x in draws(rng, L, M, C):
        if nb >= 3:
            x[-1, L + 5] = np.nan                 # a NaN window too: both forms follow the plain rules and set status 2
        one = run_stream(S, x, L, M)
        seq = run_stream(S, x, L, M, sequence=True)
        assert_bits_equal(seq[0], one[0], "L=%d M=%d C=%d blocks=%d rows" % (L, M, C, nb))
        np.testing.assert_array_equal(seq[1], one[1])
        assert seq[2:] == one[2:]
        assert one[4] == (2 if nb >= 3 else 0)


def test_the_sequence_form_cannot_be_left_for_a_long_block(S):
    from pyitd_amd import ITDError
    st = S.LevelsStream(2731, 2)
    assert st.form == "sequence"
    with pytest.raises(ITDError):
        st.force_sequence(False)
    st.close()
    st = S.LevelsStream(2730, 2)
    st.force_sequence()
    assert st.form == "sequence"
    st.force_sequence(False)
    assert st.form == "one-launch"
    st.close()


def test_a_rich_signal_is_certified_everywhere(S):
    L, M = 1024, 6
    x = rich_signal(6 * L)
    rows, exact = S.blockwise_itd(x, L, M)
    assert exact.all()
    whole, stop = whole_rows(x, M)
    assert stop == "timeout"
    assert_bits_equal(rows, whole, "all certified")


def test_deep_levels_in_short_blocks_are_not_certified_where_they_differ(S):
    L, M, nb = 64, 8, 12
    x = fuzz_signal(np.random.default_rng(7), 0, nb * L)
    rows, exact = S.blockwise_itd(x, L, M)
    whole, _ = whole_rows(x, M)
    differs = [j for j in range(nb) if not np.array_equal(rows[:, j * L:(j + 1) * L].view(np.uint64),
                                                          whole[:, j * L:(j + 1) * L].view(np.uint64))]
    assert differs and not exact[differs].any()


def hold_to_plain_composition(S, x, L, M, rows, exact, what):
    """rows / exact (one channel, as blockwise_itd gave them) and both forms' rows, flags and status against the plain-rules reference"""
    ref_rows, ref_exact, ref_status = plain_composition(x, L, M)
    assert_bits_equal(rows, ref_rows[0], what + " rows, plain rules")
    np.testing.assert_array_equal(exact, ref_exact[0], what + " flags, plain rules")
    for sequence in (False, True):
        got = run_stream(S, x[None], L, M, sequence)
        assert_bits_equal(got[0], ref_rows, what + " rows, plain rules, sequence=%s" % sequence)
        np.testing.assert_array_equal(got[1], ref_exact, what + " flags, plain rules, sequence=%s" % sequence)
        assert got[4] == ref_status, what + " status, sequence=%s" % sequence
    return ref_status


def test_plateaus_across_block_edges(S):
    """A plateau under a window's start makes that window's first segment 0/0 (ITD.py:115-116): the stream's baseline holds a
    NaN the whole signal does not, and the later stages follow the single-level stream's plain rules there."""
    L, M, nb = 100, 4, 8
    rng = np.random.default_rng(5)
    x = rng.standard_normal(nb * L)
    x[95:210] = 0.5                                            # across two block edges
    x[398:403] = -0.25                                         # across one
    x[297:300] = x[296]                                        # ending at one
    x[500:504] = x[504]                                        # starting at one
    rows, exact = S.blockwise_itd(x, L, M)
    assert_bits_equal(rows, hand_chain(L, M, x), "plateau rows")
    whole, stop = whole_rows(x, M)
    assert stop == "timeout"
    for j in np.nonzero(exact)[0]:
        assert_bits_equal(rows[:, j * L:(j + 1) * L], whole[:, j * L:(j + 1) * L], "plateau block %d" % j)
    assert not exact[1:4].any()                                # windows whose first segment lies on the long plateau
    assert hold_to_plain_composition(S, x, L, M, rows, exact, "plateau") == 2      # (0/0: a NaN in stage 1's input)


def hand_chain(L, M, x):
    """M+1 single-level linear streams chained by hand through the device forms (which do not stop at a NaN)"""
    import torch
    from pyitd_amd import streaming
    nb = x.shape[0] // L
    xs = torch.from_numpy(x.copy()).cuda()
    cur = [xs[k * L:(k + 1) * L] for k in range(nb)]
    rows = []
    for k in range(M + 1):
        st = streaming.Stream(L, 1, "linear")
        rot = torch.empty(nb, L, dtype=torch.float64, device="cuda")
        base = torch.empty_like(rot)
        out = 0
        for b in range(nb):
            if st.push_dev(cur[b].data_ptr(), L, base[out].data_ptr(), L, rot[out].data_ptr(), L):
                out += 1
        assert st.flush_dev(base[out].data_ptr(), L, rot[out].data_ptr(), L)
        torch.cuda.synchronize()
        st.close()
        rows.append((rot if k < M else rot + base).reshape(-1))
        cur = [base[b] for b in range(nb)]
    return torch.stack(rows).cpu().numpy()


def test_nan_block_sets_status_and_follows_the_hand_chain(S):
    L, M, nb = 64, 3, 7
    x = fuzz_signal(np.random.default_rng(9), 4, nb * L)
    x[3 * L + 10] = np.nan
    st = S.LevelsStream(L, M)
    outs = []
    for k in range(nb):
        r = st.push(x[k * L:(k + 1) * L])
        if r is not None:
            outs.append(r)
    while (r := st.flush()) is not None:
        outs.append(r)
    assert st.status() == 2
    st.close()
    rows = np.concatenate([o[0] for o in outs], axis=1)
    exact = np.array([bool(o[1]) for o in outs])
    assert not exact[2:5].any()                # every window that holds the NaN at stage 0
    assert_bits_equal(rows, hand_chain(L, M, x), "NaN rows")
    assert hold_to_plain_composition(S, x, L, M, rows, exact, "NaN") == 2


def test_leading_silence(S):
    L, M, nb = 128, 3, 6
    x = fuzz_signal(np.random.default_rng(4), 4, nb * L)
    x[:150] = 0.0                               # 0/0 on the first segment: the stage-0 baseline holds NaN there
    rows, exact = S.blockwise_itd(x, L, M)
    assert not exact[:2].any()
    assert_bits_equal(rows, hand_chain(L, M, x), "leading silence")
    assert hold_to_plain_composition(S, x, L, M, rows, exact, "leading silence") == 2


def test_device_form_equals_host_form_and_reuse(S):
    import torch
    L, M, C, nb = 256, 5, 3, 9
    rng = np.random.default_rng(12)
    x = np.stack([fuzz_signal(rng, k, nb * L) for k in (0, 3, 4)])
    ref_rows, ref_exact, _, _, _ = run_stream(S, x, L, M)
    st = S.LevelsStream(L, M, C)
    xd = torch.from_numpy(x).cuda()
    R = M + 1
    rows = torch.full((C, R, nb * L + 7), 7.0, dtype=torch.float64, device="cuda")    # strided rows
    exact = torch.zeros(nb + 1, C, dtype=torch.uint8, device="cuda")       # (+1: the pointers of the flush that finds it empty)
    s = torch.cuda.current_stream().cuda_stream
    for rep in range(2):                         # the second run reuses the stream after its flush
        out = 0
        for k in range(nb):
            blk = xd[:, k * L:(k + 1) * L]
            dst = rows[:, :, out * L:]
            if st.push_dev(blk.data_ptr(), nb * L, dst.data_ptr(), nb * L + 7, R * (nb * L + 7), exact[out].data_ptr(), s):
                out += 1
        while st.flush_dev(rows[:, :, out * L:].data_ptr(), nb * L + 7, R * (nb * L + 7), exact[out].data_ptr(), s):
            out += 1
        assert out == nb
        torch.cuda.synchronize()
        assert_bits_equal(rows[:, :, :nb * L].cpu().numpy(), ref_rows, "device form, run %d" % rep)
        np.testing.assert_array_equal(exact[:nb].cpu().numpy().T.astype(bool), ref_exact)
    # reset in the middle of a stream: it starts afresh
    for k in range(3):
        st.push(x[:, k * L:(k + 1) * L])
    st.reset()
    assert st.blocks_held == 0
    outs = [r for k in range(nb) if (r := st.push(x[:, k * L:(k + 1) * L])) is not None]
    while (r := st.flush()) is not None:
        outs.append(r)
    assert_bits_equal(np.concatenate([o[0] for o in outs], axis=2), ref_rows, "after reset")
    st.close()


def test_argument_errors_on_a_live_stream(S):
    from pyitd_amd import ITDError, _lib
    import torch
    L, M = 64, 2
    st = S.LevelsStream(L, M, 2)
    blk = torch.zeros(2, L, dtype=torch.float64, device="cuda")
    rows = torch.zeros(2, M + 1, L, dtype=torch.float64, device="cuda")
    lib = _lib.load()
    for _ in range(M + 1):                       # no rows needed: nothing is emitted yet
        assert not st.push_dev(blk.data_ptr(), L, None, 0, 0)
    with pytest.raises(ITDError):                # this push emits: rows are required
        st.push_dev(blk.data_ptr(), L, None, 0, 0)
    with pytest.raises(ITDError):                # row stride below the block
        st.push_dev(blk.data_ptr(), L, rows.data_ptr(), L - 1, (M + 1) * L)
    with pytest.raises(ITDError):                # channel stride overlapping the rows
        st.push_dev(blk.data_ptr(), L, rows.data_ptr(), L, M * L)
    with pytest.raises(ITDError):                # input stride below the block
        st.push_dev(blk.data_ptr(), L - 1, rows.data_ptr(), L, (M + 1) * L)
    assert st.blocks_held == M + 1
    assert st.flush_dev(rows.data_ptr(), L, (M + 1) * L)
    with pytest.raises(ITDError):                # no push while flushing
        st.push_dev(blk.data_ptr(), L, rows.data_ptr(), L, (M + 1) * L)
    # the single-level entries refuse a levels stream
    assert lib.itd_stream_push_f64(st._h, blk.data_ptr(), L, rows.data_ptr(), L, None, 0, None, None) == 1
    st.close()
