"""The numpy statement of the half-wave table stream (include/pyitd_hip.h, itd_table_stream_*), block by block,
with a carried open half wave — a plain helper of the tests, and the constructed signals they push.  Nothing here knows of tiles,
ballots or LDS.

Indices count from the stream's first sample.  i is a crossing index iff i >= 1, x[i + 1] has been pushed and the sign changes
strictly between x[i] and x[i + 1]; it is the last sample of its half wave.  Push p brings x[p L .. (p+1) L): walking its samples in
order, sample j closes the open half wave iff j - 1 is a crossing index, and joins the (then new) open one — a strictly larger |x|
replaces its peak, an equal one does not (the earlier index wins).  What is open when the push ends is reported as the entry behind
the events, and carried.  The flush closes it.  Every reported start and peak is origin + index.
"""
import numpy as np

NAMES = ("count", "start", "length", "peak", "value")


class RefTableStream:
    """One row.  push(block) -> (events, open), flush() -> event or None; an event is (start, length, peak, value)."""

    def __init__(self, L, origin=0):
        self.L, self.origin = int(L), int(origin)
        self.n = 0                      # samples pushed
        self.open = None                # [start, peak, |x| at the peak, value], indices relative to the stream
        self.last = None

    def _event(self, end):
        s, p, _, v = self.open
        return (self.origin + s, end - s + 1, self.origin + p, v)

    def push(self, block):
        block = np.asarray(block, dtype=np.float64)
        assert block.shape == (self.L,)
        events = []
        for v in block:
            j = self.n
            if j >= 2 and ((self.last > 0 and 0 > v) or (self.last < 0 and 0 < v)):      # j - 1 >= 1 is a crossing index
                events.append(self._event(j - 1))
                self.open = None
            if self.open is None:
                self.open = [j, j, abs(v), v]
            elif abs(v) > self.open[2]:
                self.open[1:] = [j, abs(v), v]
            self.last = v
            self.n += 1
        return events, self._event(self.n - 1)

    def flush(self):
        if self.n == 0:
            return None
        e = self._event(self.n - 1)
        self.n, self.open, self.last = 0, None, None
        return e


def ref_pushes(x, L, origin=0):
    """Row x of P L samples: ([(events, open) of push 0 .. P-1], the flush's event)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.ndim == 1 and x.size % L == 0 and x.size >= L
    st = RefTableStream(L, origin)
    steps = [st.push(x[p * L:(p + 1) * L]) for p in range(x.size // L)]
    return steps, st.flush()


def all_events(steps, last):
    """every push's events and the flush's, in order: (start, length, peak int64; value float64)"""
    ev = [e for events, _ in steps for e in events] + [last]
    cols = list(zip(*ev))
    return (np.array(cols[0], np.int64), np.array(cols[1], np.int64), np.array(cols[2], np.int64), np.array(cols[3], np.float64))


def step_tables(rows_steps, L, fill):
    """What a push of the stream gives for these rows' (events, open): count[R], and four tables [R, L + 1] prefilled with `fill`
    (start, length, peak int64; value float64) holding the events and, behind them, the open entry."""
    R = len(rows_steps)
    count = np.zeros(R, np.int32)
    tabs = [np.full((R, L + 1), fill[k], np.float64 if k == 3 else np.int64) for k in range(4)]
    for r, (events, op) in enumerate(rows_steps):
        count[r] = len(events)
        for e, ev in enumerate(events + [op]):
            for k in range(4):
                tabs[k][r, e] = ev[k]
    return count, tabs


# ---- the constructed signals (every one a row of blocks L samples, blocks >= 1) ------------------------------------------------------

def alternating(rng, L, blocks):
    """x[j] = (-1)^j a_j, a_j in {1, 2}: every index from 1 on is a crossing index — pushes of L - 2, L, L, ... events"""
    n = blocks * L
    return ((-1.0) ** np.arange(n)) * rng.integers(1, 3, n)


def long_wave(rng, L, blocks):
    """One sign for 3 L + 5 samples (or the whole row where it is shorter) behind a short opening, its maximum 3.0 attained in two
    different blocks — the earlier index wins across the carry — and twice inside one block; alternating runs behind it."""
    n = blocks * L
    x = np.empty(n)
    sign, pos = 1.0, 0
    for ln in (2, 1):                                                      # index 1 and 2 are crossing indices
        x[pos:pos + ln] = sign * 0.5
        pos, sign = pos + ln, -sign
    ln = min(3 * L + 5, n - pos)
    run = np.full(ln, 0.125)
    for at in (L // 2, L // 2 + 2, L // 2 + L, L // 2 + 2 * L):            # blocks 0, 0, 1, 2 of the run (where it reaches them)
        if at < ln:
            run[at] = 3.0
    x[pos:pos + ln] = sign * run
    pos, sign = pos + ln, -sign
    while pos < n:
        ln = min(int(rng.integers(1, 6)), n - pos)
        x[pos:pos + ln] = sign * rng.choice([0.25, 1.0, 2.0], ln)
        pos, sign = pos + ln, -sign
    return x


def edges(rng, L, blocks):
    """Sign changes placed exactly at i = p L - 1 (between two blocks) and at i = p L in turn, one at i = 0 (no crossing), runs of 1 ..
    4 samples elsewhere only in the first half of every block; the second half of a block is one run up to the placed change."""
    n = blocks * L
    x = np.empty(n)
    cuts = {1}                                                             # a run begins at 1: the sign changes at i = 0
    for p in range(1, blocks + 1):
        cuts.add(p * L if p % 2 else p * L + 1)                            # a run begins at p L (i = p L - 1) or at p L + 1 (i = p L)
    for p in range(blocks):
        pos = p * L + 2
        while pos < p * L + L // 2:
            cuts.add(pos)
            pos += int(rng.integers(1, 5))
    sign, prev = 1.0, 0
    for cpos in sorted(c for c in cuts if c < n) + [n]:
        ln = cpos - prev
        x[prev:cpos] = sign * rng.choice([0.25, 1.0, 2.0], ln)
        prev, sign = cpos, -sign
    return x


def zeros(rng, L, blocks):
    """+, 0, - and +, -0.0, + stretches (a zero in between is no crossing) behind a first block of zeros only that opens with -0.0:
    the half wave open behind the first push (one block: the row's only half wave) is made of zeros and reports -0.0, its first sample"""
    n = blocks * L
    pat = np.array([1.0, 0.0, -1.0, -2.0, 3.0, -0.0, 2.0, -1.0, 0.0, 0.0, 1.0, -0.0, -0.0, -1.5])
    x = np.resize(pat, n)
    x[:L] = np.where(rng.random(L) < 0.5, 0.0, -0.0)
    x[0] = -0.0
    if blocks >= 3:                                                        # zeros on both sides of a block boundary, inside a half wave
        x[2 * L - 2:2 * L + 3] = [-0.0, 0.0, 0.0, -0.0, 0.0]
    return x


def extremes(rng, L, blocks):
    """denormals and +-inf among ordinary samples, in runs of 1 .. 3"""
    n = blocks * L
    vals = np.array([5e-324, 2.5e-320, 1e-310, np.inf, 1.0, 1e308, np.inf, 3.0])
    x = np.empty(n)
    pos, sign = 0, -1.0
    while pos < n:
        ln = min(int(rng.integers(1, 4)), n - pos)
        x[pos:pos + ln] = sign * rng.choice(vals, ln)
        pos, sign = pos + ln, -sign
    return x


CONSTRUCTED = (alternating, long_wave, edges, zeros, extremes)


# ---- conditions on a set of rows' reference results (what a case must show before the stream is looked at) -----------------------------

def conditions(x, L, rows_steps):
    """x[R, P L] and every row's steps: which of the named conditions some row shows"""
    P = x.shape[1] // L
    got = dict.fromkeys(("a push with count == L", "a push with count == 0", "a half wave over three pushes, its peak not in the last",
                         "a tie of the maximum across a block boundary", "a crossing index at a block's last sample",
                         "a crossing index at a block's first sample"), False)
    for r, (steps, last) in enumerate(rows_steps):
        counts = [len(ev) for ev, _ in steps]
        got["a push with count == L"] |= L in counts
        got["a push with count == 0"] |= 0 in counts
        start, length, peak, value = all_events(steps, last)
        end = start + length - 1
        for s, e, pk, v in zip(start, end, peak, value):
            if e // L - s // L >= 2 and pk // L < e // L:
                got["a half wave over three pushes, its peak not in the last"] = True
            at = s + np.flatnonzero(np.abs(x[r, s:e + 1]) == abs(v))
            if at[0] // L != at[-1] // L:
                got["a tie of the maximum across a block boundary"] = True
        cross = end[:-1]                                                   # every half wave but the last ends at a crossing index
        got["a crossing index at a block's last sample"] |= bool(((cross % L == L - 1) & (cross < P * L - 1)).any())
        got["a crossing index at a block's first sample"] |= bool(((cross % L == 0) & (cross > 0)).any())
    return got
