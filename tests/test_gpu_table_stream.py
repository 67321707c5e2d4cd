"""The table stream on the GPU (itd_table_stream_*, pyitd_amd.streaming.WaveTableStream / blockwise_single_waves) against the
block-by-block statement tests/table_stream_ref.py and, concatenated, against tests/waves_ref.ref_table of the whole row: positions
integer for integer, value bit for bit (-0.0 told apart from +0.0); what a push may touch of its slots; origins beyond 2^31 and 2^32; a
NaN; flush and reset; the kinds' refusals; pyitd_amd.single_waves on the GPU; behind a LevelsStream on device pointers."""
import ctypes

import numpy as np
import pytest

import table_stream_ref as tsr
import table_stream_runs as runs
from helpers import assert_bits_equal, fuzz_signal
from waves_ref import ref_table

pytestmark = pytest.mark.gpu

BLOCKS = (1, 2, 3, 7)
CASES = [(L, rows) for L in (8, 9, 64, 65, 100, 512, 2048, 2049, 4096) for rows in (1, 3, 9)] + [(8, 700)]


@pytest.fixture(scope="module")
def S():
    from pyitd_amd import streaming
    return streaming


def whole_row(x, ref, what):
    """the reference's events, concatenated, are ref_table of every row"""
    for r in range(x.shape[0]):
        got = tsr.all_events(*ref[r])
        want = ref_table(x[r])
        for k in range(3):
            assert np.array_equal(got[k], want[k].astype(np.int64)), "%s row %d: %s" % (what, r, tsr.NAMES[1 + k])
        assert_bits_equal(got[3], want[3], "%s row %d: value" % (what, r))


@pytest.mark.parametrize("L,rows", CASES)
def test_every_push_and_the_flush_are_the_statement(S, L, rows):
    rng = np.random.default_rng(L * 1009 + rows)
    st = S.WaveTableStream(L, rows)
    rounds = -(-runs.KINDS // rows)                                       # every kind of row at every number of blocks
    cases, shown = [], None
    for i in range(rounds):
        for blocks in BLOCKS:
            x = runs.case_rows(rng, L, rows, blocks, shift=i * rows)
            ref = runs.reference(x, L)
            whole_row(x, ref, "L=%d rows=%d blocks=%d" % (L, rows, blocks))
            cond = tsr.conditions(x, L, ref)
            shown = cond if shown is None else {k: shown[k] or v for k, v in cond.items()}
            cases.append((x, ref, "L=%d rows=%d round %d blocks=%d" % (L, rows, i, blocks)))
    # on the reference alone, before the stream's result is looked at: the cases hold what they are there for
    for name, ok in shown.items():
        assert ok, "L=%d rows=%d: no row shows %s" % (L, rows, name)
    for x, ref, what in cases:                                            # (the stream is reused: it starts afresh after its flush)
        runs.check_stream(st, x, ref, what)
    assert st.status() == 0
    st.close()


def dev_rows(x, L, in_stride):
    """x[rows, blocks L] on the device as [blocks, rows, in_stride], NaN in the gaps"""
    import torch
    R, blocks = x.shape[0], x.shape[1] // L
    h = np.full((blocks, R, in_stride), np.nan)
    h[:, :, :L] = x.reshape(R, blocks, L).transpose(1, 0, 2)
    return torch.from_numpy(h).cuda()


def test_nothing_behind_the_open_entry_and_nothing_between_the_slots_is_touched(S):
    import torch
    for L, rows, blocks in ((100, 3, 3), (8, 5, 2), (2049, 2, 2)):
        rng = np.random.default_rng(L)
        x = runs.case_rows(rng, L, rows, blocks)
        ref = runs.reference(x, L)
        xd = dev_rows(x, L, L + 3)
        dt = runs.DevTables(blocks + 1, rows, L + 5)
        st = S.WaveTableStream(L, rows)
        ts = torch.cuda.Stream()
        torch.cuda.synchronize()
        runs.run_dev(st, xd, L, L + 3, dt, ts.cuda_stream)
        torch.cuda.synchronize()
        runs.same_dev(dt, ref, L, "L=%d strides L + 3, L + 5" % L)
        assert st.status() == 0                                           # (the NaNs of the input's gaps were not read)
        st.close()


def test_a_null_table_pointer_leaves_the_other_three_as_they_are(S):
    import torch
    L, rows, blocks = 65, 3, 3
    x = runs.case_rows(np.random.default_rng(3), L, rows, blocks)
    ref = runs.reference(x, L)
    xd = dev_rows(x, L, L)
    st = S.WaveTableStream(L, rows)
    for skip in range(4):
        dt = runs.DevTables(blocks + 1, rows, L + 1)
        torch.cuda.synchronize()
        runs.run_dev(st, xd, L, L, dt, None, skip)
        torch.cuda.synchronize()
        runs.same_dev(dt, ref, L, "without %s" % tsr.NAMES[1 + skip], skip)
    st.close()


@pytest.mark.parametrize("origin", [2 ** 31 - 3, 2 ** 40])
def test_positions_are_the_streams_indices_plus_the_origin(S, origin):
    L, rows, blocks = 100, 3, 3
    x = runs.case_rows(np.random.default_rng(7), L, rows, blocks)
    ref0, ref = runs.reference(x, L), runs.reference(x, L, origin)
    for r in range(rows):
        a, b = tsr.all_events(*ref0[r]), tsr.all_events(*ref[r])
        assert np.array_equal(a[0] + origin, b[0]) and np.array_equal(a[2] + origin, b[2]) and np.array_equal(a[1], b[1])
    st = S.WaveTableStream(L, rows, origin=origin)
    runs.check_stream(st, x, ref, "origin=%d" % origin)
    st.close()
    got = S.blockwise_single_waves(x, L, origin=origin)
    assert got.start.dtype == np.int64 and got.start.max() > origin


def test_a_nan_sets_the_status_and_leaves_the_other_rows_exact(S):
    import torch
    L, rows, blocks = 64, 3, 4
    rng = np.random.default_rng(5)
    x = runs.case_rows(rng, L, rows, blocks)
    ref = runs.reference(x, L)
    bad = x.copy()
    bad[1, L + 7] = np.nan
    st = S.WaveTableStream(L, rows)
    clean = S.WaveTableStream(L, rows)
    dt, keep = runs.DevTables(blocks + 1, rows, L + 1), runs.DevTables(blocks + 1, rows, L + 1)
    xb, xc = dev_rows(bad, L, L), dev_rows(x, L, L)
    torch.cuda.synchronize()
    runs.run_dev(st, xb, L, L, dt, None)
    assert st.status() == 2
    tabs, count = dt.host()
    assert ((count[:, 1] >= 0) & (count[:, 1] <= L)).all()
    # rows 0 and 2 with everything around their slots, the guard words included, as if row 1 were not there
    runs.run_dev(clean, xc, L, L, keep, None)
    torch.cuda.synchronize()
    runs.same_dev(keep, ref, L, "without the NaN")
    ktabs, kcount = keep.host()
    S1 = L + 1
    for k in range(4):
        a, b = tabs[k].view(np.uint64).copy(), ktabs[k].view(np.uint64).copy()
        a[:, S1:2 * S1] = b[:, S1:2 * S1] = 0
        assert np.array_equal(a, b), tsr.NAMES[1 + k]
    assert np.array_equal(np.delete(count, 1, axis=1), np.delete(kcount, 1, axis=1))
    clean.close()
    st.reset()
    assert st.status() == 0 and st.blocks_held == 0
    runs.check_stream(st, x, ref, "after the reset")                       # the next stream is exact again
    assert st.status() == 0
    st.close()


def test_flush_and_reset(S):
    L, rows = 9, 2
    rng = np.random.default_rng(11)
    st = S.WaveTableStream(L, rows)
    assert st.flush() is None and st.blocks_held == 0                     # a flush of an empty stream
    # a push after a flush starts a new stream: its index 0 is again no crossing
    x = np.stack([tsr.alternating(rng, L, 2), tsr.edges(rng, L, 2)])
    ref = runs.reference(x, L)
    assert len(ref[0][0][0][0]) == L - 2 and len(ref[0][0][1][0]) == L
    for what in ("a new stream", "behind a flush"):
        runs.check_stream(st, x, ref, what)
    # reset in mid-stream discards the open half wave
    y = runs.case_rows(rng, L, rows, 3)
    for p in range(2):
        st.push(y[:, p * L:(p + 1) * L])
    assert st.blocks_held == 2
    st.reset()
    assert st.blocks_held == 0 and st.flush() is None
    runs.check_stream(st, x, ref, "behind a reset")
    # one row, 1-D blocks: what leaves has no row axis
    one = S.WaveTableStream(L)
    w = one.push(x[0, :L])
    assert w.count.shape == () and w.start.shape == (L + 1,) and int(w.count) == L - 2
    f = one.flush()
    assert f.count == 1 and f.value.shape == (1,) and f.start[0] == L - 1
    one.close()
    st.close()


def test_argument_errors_and_the_kinds_refusals(S):
    import torch
    from pyitd_amd import ITDError, _lib
    lib = _lib.load()
    L, rows = 64, 2
    st = S.WaveTableStream(L, rows)
    wf = S.WaveFilterStream(L, rows, L)
    blk = torch.zeros(rows, L, dtype=torch.float64, device="cuda")
    out = torch.zeros(rows, L + 1, dtype=torch.float64, device="cuda")
    tab = torch.zeros(rows, L + 1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(rows, dtype=torch.int32, device="cuda")
    bd = torch.tensor([0.0, np.inf, 0.0, np.inf], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    t = (tab.data_ptr(), tab.data_ptr(), tab.data_ptr(), out.data_ptr())
    with pytest.raises(ITDError):                                        # strides too short
        st.push_dev(blk.data_ptr(), L - 1, *t, L + 1, cnt.data_ptr())
    with pytest.raises(ITDError):
        st.push_dev(blk.data_ptr(), L, *t, L, cnt.data_ptr())
    with pytest.raises(ITDError):
        st.flush_dev(*t, L, cnt.data_ptr())
    with pytest.raises(ITDError):                                        # the count is required, and the block
        st.push_dev(blk.data_ptr(), L, *t, L + 1, None)
    with pytest.raises(ITDError):
        st.push_dev(None, L, *t, L + 1, cnt.data_ptr())
    assert st.blocks_held == 0
    # the wave-filter stream's push refuses a table stream, the table stream's push a wave-filter stream; so do the others
    assert lib.itd_wave_stream_push_f64(st._h, blk.data_ptr(), L, bd.data_ptr(), 0, out.data_ptr(), L + 1, None, None) == 1
    assert lib.itd_wave_stream_flush_f64(st._h, bd.data_ptr(), 0, out.data_ptr(), L + 1, None, None) == 1
    assert lib.itd_wave_stream_latency(st._h) == -1
    em = ctypes.c_int32(0)
    assert lib.itd_table_stream_push_f64(wf._h, blk.data_ptr(), L, *t, L + 1, cnt.data_ptr(), ctypes.byref(em), None) == 1
    assert lib.itd_table_stream_flush_f64(wf._h, *t, L + 1, cnt.data_ptr(), ctypes.byref(em), None) == 1
    assert lib.itd_stream_push_f64(st._h, blk.data_ptr(), L, out.data_ptr(), L + 1, None, 0, None, None) == 1
    assert lib.itd_levels_stream_push_f64(st._h, blk.data_ptr(), L, out.data_ptr(), L, L, None, None, None) == 1
    assert lib.itd_inst_stream_push_f64(st._h, blk.data_ptr(), L, out.data_ptr(), None, None, None, L + 1, None, 0, None, None) == 1
    assert st.blocks_held == 0 and wf.blocks_held == 0
    assert st.push_dev(blk.data_ptr(), L, *t, L + 1, cnt.data_ptr()) and st.blocks_held == 1
    torch.cuda.synchronize()
    st.close()
    wf.close()


@pytest.mark.parametrize("L", [65, 512, 4096])
def test_the_concatenated_events_are_single_waves_on_the_gpu(S, L):
    import pyitd_amd
    x = runs.case_rows(np.random.default_rng(L), L, 12, 8)
    got = S.blockwise_single_waves(x, L)
    want = pyitd_amd.single_waves(x)
    assert got.count.dtype == np.int32 and np.array_equal(got.count, want.count)
    for name in ("start", "length", "peak"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), name
    assert_bits_equal(got.value, want.value, "value")
    one = S.blockwise_single_waves(x[3], L)
    assert one.count == want.count[3] and np.array_equal(one.start, want.start[3, :one.count])


def test_behind_a_levels_stream_on_device_pointers(S):
    """samples in, half-wave events out: the levels stream's emitted rows go into the table stream by pointer, on one stream, with
    no host copy in between"""
    import torch
    L, M, C, nb = 256, 3, 2, 12
    R = C * (M + 1)
    rng = np.random.default_rng(31)
    x = np.stack([fuzz_signal(rng, k, nb * L) for k in (0, 4)])
    lv = S.LevelsStream(L, M, C)
    tb = S.WaveTableStream(L, R)
    xd = torch.from_numpy(x).cuda()
    rows = torch.zeros(nb, C, M + 1, L, dtype=torch.float64, device="cuda")      # what the levels stream emitted, block by block
    dt = runs.DevTables(nb + 1, R, L + 1)
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    torch.cuda.synchronize()
    k = 0
    for p in range(nb):
        if lv.push_dev(xd[:, p * L:].data_ptr(), nb * L, rows[k].data_ptr(), L, (M + 1) * L, None, s):
            assert tb.push_dev(rows[k].data_ptr(), L, *dt.ptrs(k), s)
            k += 1
    while lv.flush_dev(rows[min(k, nb - 1)].data_ptr(), L, (M + 1) * L, None, s):
        assert tb.push_dev(rows[k].data_ptr(), L, *dt.ptrs(k), s)
        k += 1
    assert k == nb and tb.flush_dev(*dt.ptrs(nb), s)
    torch.cuda.synchronize()
    streamed = rows.cpu().numpy().transpose(1, 2, 0, 3).reshape(R, nb * L)       # the concatenated rows the second stage saw
    ref = runs.reference(streamed, L)
    whole_row(streamed, ref, "levels stream -> table stream")
    runs.same_dev(dt, ref, L, "levels stream -> table stream")
    assert sum(len(ev) for ev, _ in ref[0][0]) > nb                             # (events did leave)
    assert lv.status() == 0 and tb.status() == 0
    lv.close()
    tb.close()


@pytest.mark.parametrize("L,rows", [(100, 3), (2049, 2)])
def test_the_device_form_and_the_host_form_give_the_same_tables(S, L, rows):
    import torch
    blocks = 3
    x = runs.case_rows(np.random.default_rng(L + 1), L, rows, blocks)
    ref = runs.reference(x, L)
    st = S.WaveTableStream(L, rows)
    dt = runs.DevTables(blocks + 1, rows, L + 1)
    torch.cuda.synchronize()
    runs.run_dev(st, dev_rows(x, L, L), L, L, dt, None)
    torch.cuda.synchronize()
    tabs, count = dt.host()
    for p in range(blocks):                                               # the same stream, afresh behind its flush
        w = st.push(x[:, p * L:(p + 1) * L])
        runs.same_step(w, count[p, :rows], [t[p, :rows * (L + 1)].reshape(rows, L + 1) for t in tabs], "push %d" % p)
    w = st.flush()
    runs.same_step(w, count[blocks, :rows], [t[blocks, :rows * (L + 1)].reshape(rows, L + 1) for t in tabs], "flush")
    runs.same_dev(dt, ref, L, "device form")
    st.close()
