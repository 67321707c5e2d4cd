"""The block-wise operators (pyitd_amd.streaming, itd_stream_*) against the CPU statement of the recipe (oracle/stream_oracle.py) on random
streams: block sizes 8 .. 4096 (multiples of the 512-sample tile and others), 1 .. 6 blocks, 1 .. 3 channels, margins 1 .. 11 (1 and 2 in
four of ten trials), shared knots or not, seven signal families — the open-ended
form of tests/test_gpu_stream.py::test_streams_follow_the_oracle_on_seeded_signals.  Tier-1 (linear): bit for bit; cubic: 1e-9 of the scale.
Every trial also runs a levels stream (1 .. 8 levels, both forms, a NaN / an infinity / a leading plateau / clean) against the plain-rules
composition of tests/levels_plain_ref.py: rows bit for bit, flags and status exactly.
usage: python tools/stream_fuzz.py [trials] [seed]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import fuzz_signal, assert_bits_equal
from pyitd_amd import streaming as S
from oracle import stream_oracle as so
import levels_plain_ref as lp

trials = int(sys.argv[1]) if len(sys.argv) > 1 else 500
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
bad = skipped = 0
t0 = time.time()
for trial in range(trials):
    kind = int(rng.integers(0, 7))
    L = int(rng.choice([8, 24, 100, 512, 1000, 1024, 4096]))          # on (L % 512 == 0: the tile bases) and off the evaluation's tile grid
    nb = int(rng.integers(1, 7))
    C = int(rng.integers(1, 4))
    x = np.stack([fuzz_signal(rng, kind if c == 0 else int(rng.integers(0, 7)), L * nb) for c in range(C)])
    if kind == 5:
        x += 1e-3 * rng.standard_normal(x.shape)     # plateaus give 0/0 in the cubic operator's reference too: keep finite
    margin = int(rng.choice([1, 2])) if rng.random() < 0.4 else int(rng.integers(1, 12))   # the recipe's literal margins more often
    shared = bool(rng.integers(0, 2))
    what = "trial %d (kind %d L %d blocks %d channels %d margin %d shared %d)" % (trial, kind, L, nb, C, margin, shared)
    with np.errstate(all="ignore"):
        ref = so.oracle_blockwise_cubic(x, L, margin, shared)
        got = S.blockwise(x, L, "cubic", margin, shared)
        if np.isfinite(ref).all():
            scale = max(1.0, float(np.abs(ref).max()))
            if got.shape != ref.shape or not np.isfinite(got).all() or np.abs(got - ref).max() > 1e-9 * scale:
                bad += 1
                print("cubic MISMATCH " + what)
        else:
            skipped += 1
        rref, bref = so.oracle_blockwise_linear(x, L)
        rot, base = S.blockwise(x, L, "linear")
        try:                                         # (bit for bit, any NaN equal to any NaN: the helper of the suite)
            assert_bits_equal(base, bref, "baseline")
            assert_bits_equal(rot, rref, "rotation")
        except AssertionError as ex:
            bad += 1
            print("linear MISMATCH " + what + ": " + str(ex)[:160])
            if os.environ.get("STREAM_FUZZ_DUMP"):
                np.savez(os.path.join(os.environ["STREAM_FUZZ_DUMP"], "stream_case_%d.npz" % trial), x=x, L=L)
    # the levels leg: the levels stream (both forms where three blocks fit one workgroup) against the plain-rules composition, on the
    # families and modes of the soundness grid (tests/levels_plain_ref.py): rows bit for bit, flags and status exactly
    kind, mode = int(rng.choice(lp.FAMILIES)), str(rng.choice(lp.MODES))
    M, C = int(rng.integers(1, 9)), int(rng.integers(1, 4))
    nb = int(rng.integers(1, M + 8))
    x = np.stack([fuzz_signal(rng, kind, L * nb) for c in range(C)])
    c = int(rng.integers(0, C))
    if mode == "nan":
        x[c, rng.integers(0, L * nb)] = np.nan
    elif mode == "inf":
        x[c, rng.integers(0, L * nb)] = np.inf if rng.random() < 0.5 else -np.inf
    elif mode == "plateau":
        x[c, :rng.integers(2, 6)] = x[c, 0]
    what = "trial %d (kind %d mode %s L %d levels %d blocks %d channels %d)" % (trial, kind, mode, L, M, nb, C)
    ref_rows, ref_exact, ref_status = lp.plain_composition(x, L, M)
    for sequence in ((False, True) if 3 * L <= 8192 else (True,)):
        st = S.LevelsStream(L, M, C)
        st.force_sequence(sequence)
        outs = [r for k in range(nb) if (r := st.push(x[:, k * L:(k + 1) * L])) is not None]
        while (r := st.flush(flat=False)) is not None:
            outs.append(r)
        status = st.status()
        st.close()
        try:
            assert_bits_equal(np.concatenate([o[0] for o in outs], axis=2), ref_rows, "rows")
            assert np.array_equal(np.stack([o[1] for o in outs], axis=1), ref_exact), "flags"
            assert status == ref_status, "status %d, reference %d" % (status, ref_status)
        except AssertionError as ex:
            bad += 1
            print("levels MISMATCH " + what + " sequence=%s: " % sequence + str(ex)[:160])
print("%d trials, %d mismatches (%d cubic comparisons skipped: the reference's 0/0), %.1f s" % (trials, bad, skipped, time.time() - t0))
sys.exit(1 if bad else 0)
