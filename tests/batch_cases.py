"""Inputs, references and comparisons for the tests of the batched single-level entries (itd_baseline_extract_batch_f64,
itd_detect_batch_f64 and their wrappers in pyitd_amd/batch.py).  Nothing here needs a GPU: tests/test_batch_ops_cpu.py holds the
generators to what the GPU tests rely on and the comparisons to being sensitive, tests/test_gpu_batch_ops.py uses them.

A result is read back as the whole flat buffer it was written into: rows (or lists) of n (n - 2) entries at a stride, sentinels in
the stride gaps and in a pad behind the last row.  Every comparison is bit for bit or integer-exact.
"""
import numpy as np

from helpers import assert_bits_equal
from oracle import cpu_oracle, numpy_itd
from test_gpu_device_entries import ISENT, KINDS, PAD, SENT, oracle_detect, signal32

TILE = 512                    # samples per tile (itd_kernels.hpp)
GROUP = 64 * TILE             # samples per group of tiles
RANK_CAP0 = 264               # ITD_RANK_CAP0: knots of a tile beyond which k_extract leaves its by-rank path
CHUNK = 65535                 # signals per launch (gridDim.y)

# every sparse row has a dense row directly before and after it in memory
FAMILIES = ("int16", "sparse_mid", "zigzag", "sparse_ends", "thirds", "const", "tiny", "linspace", "lead_plateau", "trail_plateau",
            "extreme")
SPARSE = ("sparse_mid", "sparse_ends")
EXTRACT_N = (3, 4, 5, 511, 512, 513, 1025, 32767, 32768, 32769, 65 * TILE + 317)
DETECT_N = (3, 4, 5, 511, 512, 513, 1025, 32769)
NAN_N = (5, 513, 1025, 4099)
CHUNK_CASES = ((24, CHUNK + 37), (515, CHUNK + 3))     # (n, batch): one tile and two tiles per signal, two chunks
ASYNC_N = 3 * TILE + 11
MANY_GROUPS_N = 66 * GROUP + 5
MANY_GROUPS_TILE = 65 * 64    # the first tile of group 65: 64 empty tiles follow it, 4160 come before it


def sparse_mid_window(n, knot_tile=None):
    """[a, b): the samples of a sparse-middle row that leave the ramp; its knots lie in [a - 1, b]."""
    tiles = (n + TILE - 1) // TILE
    if knot_tile is None and tiles >= 3:
        knot_tile = tiles // 2
    if knot_tile is not None:
        a = knot_tile * TILE + 8
        return a, min(a + 480, n - 2)
    a = max(1, n // 3)
    return a, min(max(a + 1, 2 * n // 3), n - 1)


def sparse_ends_windows(n):
    w = max(1, min(200, n // 4))
    return (1, 1 + w), (n - 1 - w, n - 1)


def _burst(x, a, b, rng):
    """alternating steps of 3 .. 4 ramp steps on x[:, a:b] (the ramp's step is 1 .. 2: every sample of the window is a knot)"""
    i = np.arange(a, b)
    x[:, a:b] += ((-1.0) ** i) * (6.0 + 2.0 * rng.random((x.shape[0], b - a)))


def family_rows(name, n, count=1, seed=0, knot_tile=None):
    """float64[count, n]: `count` rows of one family (every row its own draw)."""
    rng = np.random.default_rng([seed, n, FAMILIES.index(name)])
    if name in KINDS:                                   # the three float32 kinds of the device entries' tests, widened
        return np.stack([signal32(name, n, seed=seed + r).astype(np.float64) for r in range(count)])
    if name == "zigzag":                                # helpers.fuzz_signal kind 6, a row per draw: every interior sample a knot
        return ((-1.0) ** np.arange(n)) * (1 + rng.random((count, n)))
    if name == "extreme":                               # helpers.fuzz_signal kind 7 (finite by construction: |x| < 1e132)
        return rng.standard_normal((count, n)) * np.exp(rng.uniform(-300, 300, (count, 1)))
    if name == "const":
        return rng.standard_normal((count, 1)) * np.ones(n)
    ramp = np.arange(n) * (1.0 + rng.random((count, 1))) + rng.standard_normal((count, 1))
    if name == "linspace":                              # no knots
        return ramp
    if name == "sparse_mid":                            # knots only inside one tile in the middle of the signal
        _burst(ramp, *sparse_mid_window(n, knot_tile), rng)
        return ramp
    if name == "sparse_ends":                           # knots only next to the two ends
        for a, b in sparse_ends_windows(n):
            _burst(ramp, a, b, rng)
        return ramp
    x = rng.standard_normal((count, n))
    k = max(2, min(n // 3, 130))                        # (130: a plateau longer than two 64-sample wavefront rows)
    if name == "lead_plateau":                          # the baseline's first segment is 0 / 0: NaN rows from finite input
        x[:, :k] = x[:, k - 1:k]
    else:
        assert name == "trail_plateau"
        x[:, n - k:] = x[:, n - k:n - k + 1]
    return x


def mixed_batch(n, batch, seed=0):
    """float64[batch, n]: row b is of family FAMILIES[b % 11]; returns (rows, family name of every row)."""
    x = np.empty((batch, n))
    names = [FAMILIES[b % len(FAMILIES)] for b in range(batch)]
    for k, name in enumerate(FAMILIES):
        cnt = len(range(k, batch, len(FAMILIES)))
        if cnt:
            x[k::len(FAMILIES)] = family_rows(name, n, cnt, seed)
    return x, names


def zero_cross_rows(n, count, seed=0):
    """Rows for the sign-change predicate: +0.0, -0.0, subnormals and values of both signs, with crossings before, across and
    behind every tile seam."""
    rng = np.random.default_rng([seed, n, 99])
    v = np.array([0.0, -0.0, 1.0, -1.0, 2.5, -0.5, 5e-324, -5e-324])
    x = v[rng.integers(0, v.size, (count, n))]
    if n >= 6:
        x[:, 1:5] = (0.0, -0.0, 3.0, -3.0)
    for t in range(TILE, n - 2, TILE):
        x[:, t - 2:t + 2] = (1.0, -1.0, 1.0, -1.0)
    return x


NAN_BATCH = 6
NAN_ROWS = (1, 3)             # between finite rows


def nan_positions(n):
    """The NaN samples of the two NaN rows: the ends and both sides of the first seam; one interior sample and a run of three."""
    ends = sorted({0, n - 1} | ({TILE - 1, TILE} if n > TILE else set()))
    inner = [n // 2] + ([n // 4, n // 4 + 1, n // 4 + 2] if n >= 16 else [])
    return {NAN_ROWS[0]: ends, NAN_ROWS[1]: inner}


def nan_batch(n, seed=0):
    x = family_rows("thirds", n, NAN_BATCH, seed + 50)
    for b, pos in nan_positions(n).items():
        x[b, pos] = np.nan
    return x


# ---- references ---------------------------------------------------------------------------------------------------------------
def extract_reference(x):
    """(rotation[B, n], baseline[B, n], info[B]) of the batched extraction: finite rows by the C oracle, info = the knot count; rows
    that hold a NaN by the plain rules (numpy_itd.baseline_extract(plain_nan=True)), info = -1 - count."""
    x = np.atleast_2d(x)
    rot, base, info = np.empty_like(x), np.empty_like(x), np.empty(x.shape[0], np.int32)
    has_nan = np.isnan(x).any(axis=1)
    for b in range(x.shape[0]):
        if has_nan[b]:
            rot[b], base[b], m, _ = numpy_itd.baseline_extract(x[b], plain_nan=True)
            info[b] = -1 - m
        else:
            rot[b], base[b], kn, _ = cpu_oracle.itd_baseline_extract(x[b], want_knots=True)
            info[b] = len(kn)
    return rot, base, info


def plain_detect(x, mode):
    """The knots of one signal under the plain rules: modes 0-2 the flags of numpy_itd (on finite input = the C oracle, which
    tests/test_batch_ops_cpu.py holds them to), modes 3 and 4 the oracle's C loops, plain IEEE comparisons as they are."""
    if mode <= 2 and np.isnan(x).any():
        f = (numpy_itd.knot_flags, numpy_itd.valley_flags, numpy_itd.peak_flags)[mode]
        return np.flatnonzero(f(x)).astype(np.int64)
    return oracle_detect(x, mode)


def detect_reference(x, mode):
    """(lists, info[B]) of the batched detection."""
    x = np.atleast_2d(x)
    lists = [plain_detect(row, mode) for row in x]
    has_nan = np.isnan(x).any(axis=1)
    info = np.array([-1 - len(k) if h else len(k) for k, h in zip(lists, has_nan)], np.int32)
    return lists, info


# ---- layouts and comparisons --------------------------------------------------------------------------------------------------
def layout(rows, stride, sent=SENT, pad=PAD):
    """rows[B, n] as the flat buffer an entry reads or writes: row b at b * stride, `sent` in the stride gaps and in `pad` entries
    behind the last row.  A single row may have a stride below n (the entries accept that for batch = 1)."""
    rows = np.atleast_2d(rows)
    B, n = rows.shape
    stride = max(stride, n) if B == 1 else stride
    assert stride >= n
    buf = np.full(B * stride + pad, sent, rows.dtype)
    buf[:B * stride].reshape(B, stride)[:, :n] = rows
    return buf


def blank(B, n, stride, sent=SENT, pad=PAD, dtype=np.float64):
    """The sentinel-filled output buffer of B rows of n at `stride`."""
    return np.full(B * (max(stride, n) if B == 1 else stride) + pad, sent, dtype)


def assert_rows(buf, want, stride, what, rows=None, sent=SENT):
    """buf, a flat buffer read back whole, holds want[B, n] at `stride` bit for bit (any NaN = any NaN) with every sentinel of the
    stride gaps and behind the last row untouched."""
    want = np.atleast_2d(want)
    assert_rows_of(buf, want.shape[0], want, np.arange(want.shape[0]), stride, what, sent)


def assert_rows_of(buf, B, want, rows, stride, what, sent=SENT):
    """The same for a batch of B rows of which only `rows` are compared with want[k] = the reference of row rows[k]; the gaps and
    the pad are checked over the whole buffer."""
    n = want.shape[1]
    stride = max(stride, n) if B == 1 else stride
    body = buf[:B * stride].reshape(B, stride)
    assert np.all(body[:, n:] == sent), "%s: a sentinel in a stride gap was overwritten" % what
    assert buf.size > B * stride and np.all(buf[B * stride:] == sent), "%s: a sentinel behind the last row was overwritten" % what
    assert_bits_equal(body[rows, :n], want, what)


def assert_info(buf, want, what):
    B = len(want)
    assert buf.size > B and np.all(buf[B:] == ISENT), "%s: info behind the last signal was written" % what
    bad = np.flatnonzero(buf[:B] != want)
    assert bad.size == 0, "%s: info of %d signals differs; first signal %d: %d, expected %d" % (
        what, bad.size, bad[0], buf[bad[0]], want[bad[0]])


def assert_lists(buf, lists, n, stride, what):
    """buf holds every signal's ascending knot list at the front of its slot of `stride` entries.  Entries [count, n - 2) of a slot
    are unspecified (pyitd_hip.h); everything at or beyond entry n - 2 of a slot and behind the last slot is the sentinel."""
    B = len(lists)
    stride = max(stride, n - 2) if B == 1 else stride
    body = buf[:B * stride].reshape(B, stride)
    assert np.all(body[:, n - 2:] == ISENT), "%s: a sentinel in a list's stride gap was overwritten" % what
    assert buf.size > B * stride and np.all(buf[B * stride:] == ISENT), "%s: a sentinel behind the last list was overwritten" % what
    for b, want in enumerate(lists):
        assert len(want) <= n - 2
        assert np.array_equal(body[b, :len(want)], want), "%s: the list of signal %d differs" % (what, b)


def check_extract(got, x, ref, strides, what, rows=None):
    """got: dict(x, rot, base, info) of flat buffers read back after the call (info None: not passed); x[B, n] the input, ref =
    extract_reference of the compared rows, strides = (x, rot, base)."""
    B = x.shape[0]
    rows = np.arange(B) if rows is None else np.asarray(rows)
    rot, base, info = ref
    assert_rows_of(got["rot"], B, rot, rows, strides[1], what + " rotation")
    assert_rows_of(got["base"], B, base, rows, strides[2], what + " baseline")
    if got.get("info") is not None:
        full = got["info"][:B].copy()
        full[rows] = info
        assert_info(got["info"], full, what)
    assert_rows_of(got["x"], B, x, np.arange(B), strides[0], what + " (the input is left alone)")


def check_detect(got, ref, n, idx_stride, what):
    """got: dict(idx, info) of flat int32 buffers read back (either None: not passed); ref = detect_reference."""
    lists, info = ref
    if got.get("idx") is not None:
        assert_lists(got["idx"], lists, n, idx_stride, what)
    if got.get("info") is not None:
        assert_info(got["info"], info, what)


def chunk_rows_to_check(batch, others=2000, seed=5):
    """Of a batch that runs as two chunks: every row of the last chunk, every row within 64 of the chunk boundary on either side,
    and `others` seeded rows of the rest."""
    rng = np.random.default_rng(seed)
    near = np.arange(CHUNK - 64, batch)
    return np.unique(np.concatenate((near, rng.integers(0, CHUNK - 64, others))))
