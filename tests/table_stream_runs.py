"""What the GPU tests of the table stream (test_gpu_table_stream.py, test_gpu_table_stream_order.py) share: the rows they push, the
loops that push and flush them through the host and the device forms, and the comparison with tests/table_stream_ref.py."""
import numpy as np

import table_stream_ref as tsr
from helpers import fuzz_signal
from wave_stream_ref import run_length_signal

KINDS = 12
FILL = (-777, -778, -779, -7.75)                                           # what untouched entries of start, length, peak, value hold


def make_row(rng, kind, L, blocks):
    """row kind 0 .. 11: four run-length signals (H = L // 2 and 2 L + 1, without and with exact zeros), fuzz_signal 0, 1 and 4,
    the five constructed signals"""
    if kind < 4:
        return run_length_signal(rng, L, (L // 2, 2 * L + 1)[kind // 2], blocks, zeros=bool(kind & 1))
    if kind < 7:
        return fuzz_signal(rng, (0, 1, 4)[kind - 4], blocks * L)
    return tsr.CONSTRUCTED[kind - 7](rng, L, blocks)


def case_rows(rng, L, rows, blocks, shift=0):
    """x[rows, blocks L]: row r is of kind (r + shift) mod 12, the constructed ones first"""
    return np.stack([make_row(rng, (7 + r + shift) % KINDS, L, blocks) for r in range(rows)])


def reference(x, L, origin=0):
    """every row's (steps, last) by the block-by-block statement"""
    return [tsr.ref_pushes(x[r], L, origin) for r in range(x.shape[0])]


def same_step(got, want_count, want_tabs, what):
    """a push's or flush's StreamWaves against count and tables of the reference: count, and the entries 0 .. count of every row
    (0 .. count - 1 where the tables have no room for more: a flush)"""
    count = np.asarray(got.count).reshape(-1)
    assert count.dtype == np.int32 and np.array_equal(count, want_count), "%s: count %s, not %s" % (what, count, want_count)
    for k, name in enumerate(tsr.NAMES[1:]):
        g = np.asarray(got[1 + k]).reshape(count.size, -1)
        w = want_tabs[k][:, :g.shape[1]]
        mask = np.arange(g.shape[1])[None, :] <= count[:, None]
        assert g.dtype == w.dtype, (name, g.dtype)
        if k == 3:
            ok = g.view(np.uint64)[mask] == w.view(np.uint64)[mask]
        else:
            ok = g[mask] == w[mask]
        if not ok.all():
            r, e = np.argwhere(mask)[np.flatnonzero(~ok)[0]]
            raise AssertionError("%s: %s of row %d entry %d (count %d): %r, not %r" % (what, name, r, e, count[r], g[r, e], w[r, e]))


def check_stream(st, x, ref, what):
    """push every block of x through the host form and flush: every step against the reference `ref` of x"""
    L, R = st.block, x.shape[0]
    for p in range(x.shape[1] // L):
        got = st.push(x[:, p * L:(p + 1) * L])
        count, tabs = tsr.step_tables([ref[r][0][p] for r in range(R)], L, FILL)
        same_step(got, count, tabs, "%s push %d" % (what, p))
        assert st.blocks_held == p + 1
    got = st.flush()
    count, tabs = tsr.step_tables([([ref[r][1]], ref[r][1]) for r in range(R)], L, FILL)
    assert all(np.asarray(t).shape == (R, 1) for t in got[1:]), what
    same_step(got, count, tabs, "%s flush" % what)
    assert st.blocks_held == 0 and st.flush() is None, what


class DevTables:
    """The tables of a device-form run on the GPU: [steps, rows * event_stride + 8] per table (8 guard words behind the last slot),
    count [steps, rows + 8], everything prefilled with FILL / -9."""

    def __init__(self, steps, rows, event_stride):
        import torch
        self.rows, self.stride = rows, event_stride
        n = rows * event_stride + 8
        self.tabs = [torch.full((steps, n), FILL[k], dtype=torch.float64 if k == 3 else torch.int64, device="cuda") for k in range(4)]
        self.count = torch.full((steps, rows + 8), -9, dtype=torch.int32, device="cuda")

    def ptrs(self, i, skip=None):
        return [None if k == skip else self.tabs[k][i].data_ptr() for k in range(4)] + [self.stride, self.count[i].data_ptr()]

    def host(self):
        return [t.cpu().numpy() for t in self.tabs], self.count.cpu().numpy()


def run_dev(st, xd, L, in_stride, dt, stream, skip=None):
    """push every block of the device rows xd [rows, in_stride-strided blocks] and flush, device forms on `stream`, no host copy:
    step i's tables in dt.tabs[.][i].  xd: [blocks, rows, in_stride]."""
    blocks = xd.shape[0]
    for p in range(blocks):
        assert st.push_dev(xd[p].data_ptr(), in_stride, *dt.ptrs(p, skip), stream)
    assert st.flush_dev(*dt.ptrs(blocks, skip), stream)


def same_dev(dt, ref, L, what, skip=None):
    """a device run's tables against the reference; untouched: everything at or beyond entry count + 1 of a slot (a flush: beyond
    entry 0), everything between and behind the slots, and a skipped table altogether"""
    tabs, count = dt.host()
    R, S = dt.rows, dt.stride
    steps = tabs[0].shape[0]
    for i in range(steps):
        flush = i == steps - 1
        if flush:
            wc, wt = tsr.step_tables([([ref[r][1]], ref[r][1]) for r in range(R)], L, FILL)
        else:
            wc, wt = tsr.step_tables([ref[r][0][i] for r in range(R)], L, FILL)
        assert np.array_equal(count[i, :R], wc), "%s step %d: count %s, not %s" % (what, i, count[i, :R], wc)
        assert (count[i, R:] == -9).all(), what
        for k in range(4):
            want = np.full(R * S + 8, FILL[k], tabs[k].dtype)
            if k != skip:
                for r in range(R):
                    n = 1 if flush else int(wc[r]) + 1
                    want[r * S:r * S + n] = wt[k][r, :n]
            g, w = (tabs[k][i].view(np.uint64), want.view(np.uint64)) if k == 3 else (tabs[k][i], want)
            bad = np.flatnonzero(g != w)
            assert not bad.size, "%s step %d: %s differs at word %d (row %d entry %d): %r, not %r" % (
                what, i, tsr.NAMES[1 + k], bad[0], bad[0] // S, bad[0] % S, tabs[k][i][bad[0]], want[bad[0]])
