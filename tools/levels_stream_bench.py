"""Microseconds per push of the levels stream (pyitd_amd.streaming.LevelsStream, device form) against M+1 hand-chained
single-level linear streams (Stream(kind="linear"), device forms), steady state, for L in {256, 1024, 2048, 4096}, M in {4, 8},
C in {1, 8, 64}.  One line per shape: the path the levels stream takes ("one-launch" up to 2730 samples, "sequence" above),
its time, the hand chain's, and for one-launch shapes the forced launch sequence's too.  usage: python tools/levels_stream_bench.py [--pushes 200]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyitd_amd import streaming  # noqa: E402


def time_pushes(step, pushes, warm):
    for k in range(warm):
        step(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(pushes):
        step(warm + k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / pushes * 1e6


def levels(L, M, C, x, pushes, warm, sequence=False):
    st = streaming.LevelsStream(L, M, C)
    if sequence:
        st.force_sequence()
    path = st.form
    rows = torch.empty(C, M + 1, L, dtype=torch.float64, device="cuda")
    exact = torch.empty(C, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    nb = x.shape[1] // L
    us = time_pushes(lambda k: st.push_dev(x[:, (k % nb) * L:].data_ptr(), x.shape[1], rows.data_ptr(), L, (M + 1) * L,
                                           exact.data_ptr(), s), pushes, warm)
    st.close()
    return path, us


def chain(L, M, C, x, pushes, warm):
    sts = [streaming.Stream(L, C, "linear") for _ in range(M + 1)]
    rot = torch.empty(M + 1, C, L, dtype=torch.float64, device="cuda")
    base = torch.empty(M + 2, C, L, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    nb = x.shape[1] // L

    def step(k):
        src, stride = x[:, (k % nb) * L:].data_ptr(), x.shape[1]
        for i, st in enumerate(sts):
            st.push_dev(src, stride, base[i].data_ptr(), L, rot[i].data_ptr(), L, s)
            src, stride = base[i].data_ptr(), L
    us = time_pushes(step, pushes, warm)
    for st in sts:
        st.close()
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warm", type=int, default=30)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    for L in (256, 1024, 2048, 4096):
        for M in (4, 8):
            for C in (1, 8, 64):
                x = torch.from_numpy(rng.standard_normal((C, 16 * L))).cuda()
                ch = chain(L, M, C, x, a.pushes, a.warm)
                path, lv = levels(L, M, C, x, a.pushes, a.warm)
                line = {"L": L, "M": M, "C": C, "path": path, "levels_us_per_push": round(lv, 1), "chain_us_per_push": round(ch, 1)}
                if path == "one-launch":        # the forced launch sequence beside it
                    line["sequence_us_per_push"] = round(levels(L, M, C, x, a.pushes, a.warm, sequence=True)[1], 1)
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
