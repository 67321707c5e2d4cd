"""Order of calls for the table stream: its results are the same behind a wave_filter call, behind a
WaveFilterStream push, and back to back with other work on a caller's stream — every step against tests/table_stream_ref.py."""
import numpy as np
import pytest

import table_stream_runs as runs

pytestmark = pytest.mark.gpu

L, ROWS, BLOCKS = 100, 3, 3


@pytest.fixture(scope="module")
def S():
    from pyitd_amd import streaming
    return streaming


@pytest.fixture(scope="module")
def case():
    x = runs.case_rows(np.random.default_rng(23), L, ROWS, BLOCKS)
    return x, runs.reference(x, L)


def test_behind_a_wave_filter_call(S, case):
    import pyitd_amd
    x, ref = case
    st = S.WaveTableStream(L, ROWS)
    other = runs.case_rows(np.random.default_rng(1), 512, 4, 2)
    pyitd_amd.wave_filter(other, amplitude=(0.2, 2.0), length=(1.0, 100.0))
    runs.check_stream(st, x, ref, "behind wave_filter")
    for p in range(BLOCKS):                                               # ... and with one between every two pushes
        st.push(x[:, p * L:(p + 1) * L])
        pyitd_amd.wave_filter(other, amplitude=(0.2, 2.0), length=(1.0, 100.0))
    st.reset()
    runs.check_stream(st, x, ref, "behind wave_filter and a reset")
    st.close()


def test_behind_a_wave_filter_stream_push(S, case):
    x, ref = case
    st = S.WaveTableStream(L, ROWS)
    wf = S.WaveFilterStream(L, ROWS, 2 * L)
    bounds = np.array([0.2, 2.0, 0.0, np.inf])
    for p in range(BLOCKS):
        wf.push(x[:, p * L:(p + 1) * L], bounds)
    runs.check_stream(st, x, ref, "behind a wave-filter stream's pushes")
    wf.close()
    st.close()


def test_back_to_back_on_a_callers_stream(S, case):
    """two table streams and a wave-filter stream take the same blocks on one stream of the caller's, with no synchronisation in between"""
    import torch
    x, ref = case
    R, blocks = x.shape[0], x.shape[1] // L
    xd = torch.from_numpy(np.ascontiguousarray(x.reshape(R, blocks, L).transpose(1, 0, 2))).cuda()
    a, b = S.WaveTableStream(L, ROWS), S.WaveTableStream(L, ROWS)
    wf = S.WaveFilterStream(L, ROWS, L)
    da, db = runs.DevTables(blocks + 1, R, L + 1), runs.DevTables(blocks + 1, R, L + 1)
    bd = torch.tensor([0.0, np.inf, 0.0, np.inf], dtype=torch.float64, device="cuda")
    out = torch.zeros(R, L, dtype=torch.float64, device="cuda")
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    torch.cuda.synchronize()
    for p in range(blocks):
        assert a.push_dev(xd[p].data_ptr(), L, *da.ptrs(p), s)
        wf.push_dev(xd[p].data_ptr(), L, bd.data_ptr(), 0, out.data_ptr(), L, s)
        assert b.push_dev(xd[p].data_ptr(), L, *db.ptrs(p), s)
    assert a.flush_dev(*da.ptrs(blocks), s) and b.flush_dev(*db.ptrs(blocks), s)
    torch.cuda.synchronize()
    runs.same_dev(da, ref, L, "the first stream")
    runs.same_dev(db, ref, L, "the second stream")
    for st in (a, b, wf):
        st.close()
