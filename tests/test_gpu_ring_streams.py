"""The contract the four ring streams share (pyitd_amd.streaming.WaveFilterStream, SpectrumStream, InstantaneousStream,
WaveHistogramStream over one host-side body, pyitd_amd/csrc/itd_ring_streams.inc), on the smallest shapes that exercise it: the latency D = ceil((H + reach) / L),
the emission pattern of push, blocks_held after every call, min(pushed, D) emitting flushes, the refusal of a push between two flush
steps, and the restart after a drain.  What each kind computes is held to its reference in its own file."""
import numpy as np
import pytest

from ring_stream_runs import enveloped_signals, latency

pytestmark = pytest.mark.gpu

ROWS = 2
INVALID_ARG = 1                                                           # ITD_ERR_INVALID_ARG (include/pyitd_hip.h)
# kind: (the block L, the reach)
KINDS = {"wave": (8, 0), "spectrum": (64, 1), "inst": (8, 1), "hist": (64, 0)}
EDGES = np.linspace(0.0, 0.6, 6)
LENGTH_EDGES = np.array([1.0, 3.0, 9.0, 27.0, np.inf])                    # (the histogram stream's second axis)


def make(S, kind, H):
    L = KINDS[kind][0]
    if kind == "wave":
        return S.WaveFilterStream(L, ROWS, H)
    if kind == "spectrum":
        return S.SpectrumStream(L, ROWS, H, edges=EDGES)
    if kind == "hist":
        return S.WaveHistogramStream(L, ROWS, H, amplitude_edges=EDGES, length_edges=LENGTH_EDGES)
    return S.InstantaneousStream(L, ROWS, H, want=("amplitude", "phase", "frequency", "length"))


def fields(r):
    """what a push or a flush gave, as a tuple of arrays"""
    return (r,) if isinstance(r, np.ndarray) else tuple(r)


def same_blocks(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        for a, b in zip(fields(g), fields(w)):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            assert a.dtype == b.dtype and a.shape == b.shape, "%s, block %d" % (what, k)
            assert a.tobytes() == b.tobytes(), "%s: block %d differs" % (what, k)


def run(st, x, D, between=None):
    """Every block of x pushed, then flushed to empty, blocks_held checked after every call; between(): called between the first two
    flush steps.  Returns the blocks that left, in order."""
    L, n = st.block, x.shape[1] // st.block
    outs, held = [], 0
    assert st.blocks_held == 0
    for p in range(n):
        r = st.push(x[:, p * L:(p + 1) * L])
        assert (r is None) == (p < D), "push %d of a stream with latency %d" % (p, D)   # None exactly D times
        if r is not None:
            outs.append(r)
        held += r is None
        assert st.blocks_held == held == min(p + 1, D)
    for k in range(min(n, D)):                                            # exactly min(pushed, D) flushes emit
        if k == 1 and between:
            between()
        r = st.flush()
        assert r is not None, "flush %d of %d" % (k, min(n, D))
        outs.append(r)
        held -= 1
        assert st.blocks_held == held
    assert st.flush() is None and st.flush() is None and st.blocks_held == 0
    assert len(outs) == n
    return outs


@pytest.mark.parametrize("hk", range(4))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_latency_emission_flush_refusal_and_restart(kind, hk):
    import torch
    from pyitd_amd import streaming as S
    from pyitd_amd._lib import ITDError
    L, reach = KINDS[kind]
    H = (1, L - 1, L, L + 1)[hk]
    D = latency(L, H, reach)
    assert D == -(-(H + reach) // L) and D == (1 if H + reach <= L else 2)   # both sides of the kind's formula
    rng = np.random.default_rng(100 * hk + len(kind))
    x = enveloped_signals(rng, L, H, ROWS, D + 2)
    fresh = make(S, kind, H)
    assert fresh.latency == D
    assert fresh.flush() is None and fresh.blocks_held == 0              # an empty stream
    want = run(fresh, x, D)
    fresh.close()

    st = make(S, kind, H)
    assert st.latency == D
    for n in (1, D):                                                      # shorter streams first: min(pushed, D) = pushed
        same_blocks(run(st, x[:, :n * L], D), run(make(S, kind, H), x[:, :n * L], D), "%d blocks" % n)

    # a push_dev between two flush steps (there are two where D = 2) is refused and changes nothing
    buf = torch.zeros(ROWS, L, dtype=torch.float64, device="cuda")
    out = torch.zeros(ROWS, L * 8, dtype=torch.float64, device="cuda")
    edges = torch.from_numpy(EDGES).cuda()
    ledges = torch.from_numpy(LENGTH_EDGES).cuda()
    cells = (len(EDGES) - 1) * (len(LENGTH_EDGES) - 1)
    hist = torch.zeros(2, ROWS, cells, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    refused = []

    def push_between():
        held = st.blocks_held
        with pytest.raises(ITDError) as err:
            if kind == "wave":
                st.push_dev(buf.data_ptr(), L, out.data_ptr(), 0, out.data_ptr(), L)
            elif kind == "spectrum":
                st.push_dev(buf.data_ptr(), L, edges.data_ptr(), 0, out.data_ptr(), L * 8)
            elif kind == "hist":
                st.push_dev(buf.data_ptr(), L, edges.data_ptr(), 0, ledges.data_ptr(), 0, hist[0].data_ptr(), hist[1].data_ptr(), cells)
            else:
                st.push_dev(buf.data_ptr(), L, out.data_ptr(), None, None, None, L)
        assert err.value.status == INVALID_ARG
        assert st.blocks_held == held
        refused.append(held)

    same_blocks(run(st, x, D, push_between), want, "with a refused push in the flush")
    assert refused == ([D - 1] if D >= 2 else [])
    # after the drain: the same input through the same object, the same bits as through a fresh one
    same_blocks(run(st, x, D), want, "the same object after its drain")
    st.close()
