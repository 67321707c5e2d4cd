"""What the GPU tests of the ring streams (wave filter, spectrum, instantaneous: test_gpu_wave_stream.py, test_gpu_spectrum_stream.py,
test_gpu_inst_stream.py, test_gpu_ring_streams.py) share: the latency formula, the push-then-flush loop and the rows they push."""
import numpy as np

import spectrum_stream_ref as ssr
from helpers import fuzz_signal
from wave_stream_ref import run_length_signal


def latency(L, H, reach=1):
    """D = ceil((H + reach) / L); reach: the samples a kind reads beyond the horizon, 0 for the wave filter, 1 for the other two"""
    return -(-(H + reach) // L)


def push_and_flush(st, x, push_args=(), flush_args=()):
    """push every block of x[rows, blocks L], flush until empty: (what the calls returned, in order; the pushes' emission pattern; the
    flushes that emitted)"""
    L = st.block
    outs, pattern, flushed = [], [], 0
    for p in range(x.shape[1] // L):
        r = st.push(x[:, p * L:(p + 1) * L], *push_args)
        pattern.append(r is not None)
        if r is not None:
            outs.append(r)
    while (r := st.flush(*flush_args)) is not None:
        flushed += 1
        outs.append(r)
    assert st.blocks_held == 0
    return outs, pattern, flushed


def enveloped_signals(rng, L, H, rows, blocks):
    """x[rows, blocks L]: run-length signals under a smooth envelope (every other one with exact zeros), every third row noise"""
    x = []
    for r in range(rows):
        if r % 3 == 2:
            x.append(fuzz_signal(rng, 0, blocks * L))
        else:
            x.append(run_length_signal(rng, L, H, blocks, zeros=(r % 3 == 1)) * ssr.envelope(blocks * L, rng))
    return np.stack(x)
