"""CPU model of the "knot-first" form of the sparse levels — TEST INFRASTRUCTURE ONLY (never imported by pyitd_amd).

Idea.  One extraction (ITD.py:79-121) maps every sample through an affine function of ITSELF,
    baseline[i] = B_k + S_k * (x[i] - x[e_k])          for i in [e_k, e_k+1),
so between two consecutive knots the baseline is a monotone image of the (monotone) input and the NEXT level's knots can only
sit at this level's knots — apart from positions where exact ties in the data let rounding make or break a plateau.  Hence the
whole level recursion ITD.py:384-432 can run on the knot list alone:
  * a candidate carries the level's values at (e-1, e, e+1);
  * B_k, S_k come from the knots' values and positions (ITD.py:100-116), the three values move to the next level through the
    affine maps of the segments they lie in, the knot predicate (ITD.py:59 on x and -x) on the new triple decides survival;
  * positions next to an exact tie of the level the recursion starts from (x[i] == x[i+1]) and sample n-2 (its right neighbour
    is forced to 0: baseline[n-1] is never written, ITD.py:112-117) stay candidates for ever ("sticky"), and so does every
    candidate whose triple shows an exact tie at some level.
The samples then need ONE pass over all fused levels (every sample through its segment's map at each level, rotation rows
written, nothing else read or written), which also re-derives every level's knots from the actual samples: any difference
from the knot side's list means the shortcut missed a knot and the result is discarded (the engine repeats level by level).

This file states that algorithm in numpy, and the rules by which the GPU's kernels deliver or refuse a signal (decide(), each rule
with the line of pyitd_amd/csrc/itd_knotfirst.hpp it restates), so that tests can hold (a) the idea to the pinned oracle
(tests/test_oracle_knotfirst.py, tests/test_kf_decisions_cpu.py: baselines and per-level knot lists bit for bit, or an honest
refusal for one stated reason), and (b) the GPU's DECISIONS to this model (tests/test_gpu_kf_decisions.py: delivered exactly where
decide() delivers, refused with decide()'s fail bit, the engine's learned cap at decide()'s fail_lev).  The GPU's intermediate
tables are not compared with the model's: the sample pass verifies them on the device (V0 .. V3) and the delivered rows are held to
the oracle bit for bit.

The constants below are this model's own copies; tests/test_kf_decisions_cpu.py parses the header and compares.

All four capacities have a case on each side of their limit in tests/kf_cases.py — kKfCap too: a pure sine of 0.45 cycles per
sample still has 0.3 knots per sample at level 2 (154 per tile of 512), and a stretch of it shorter than a tile leaves the workgroup
around it far below kKcCapH.  From level 3 on no input of the table comes near kKfCap (the densest, the same sine, has 0.1 knots per
sample there), so its cases hand over at level 2.
"""
import numpy as np

# this model's copies of the kernel's constants (itd_knotfirst.hpp:44,53-59,107-108)
K_KF_CAP = 128          # kKfCap: knots of one tile and level the sample pass holds
K_KC_TILES = 64         # kKcTiles: tiles a knot-side workgroup owns at most
K_KC_CAP = 1024         # kKcCap: candidates of a workgroup from the second fused level on
K_KC_CAP_H = 1720       # kKcCapH: ... at the hand-over level
K_KC_SLAB = 3200        # kKcSlab: table entries of a workgroup, all fused levels
FAIL_VERIFY, FAIL_CAPACITY, FAIL_NONFINITE, FAIL_TIES, FAIL_WAIT = 1, 2, 4, 8, 16      # (8: declared, raised nowhere)
TILE = 512              # samples of a tile
L0_REACH = 128 + 8 * 510    # the fused level-0 launch's reach in front of a tile: the halo group and kReach windows (itd_kernels.hpp:1243)


class NeedFallback(Exception):
    pass


def _predicate(yl, yc, yr):
    with np.errstate(invalid="ignore"):
        dp, dn = yc - yl, yr - yc
        return ((dn > 0) & (dp <= 0)) | ((dn < 0) & (dp >= 0))


NEAR = 2.0 ** -20


def near(a, b):
    """Two neighbouring values that rounding may make (or has made) equal within the levels to come: |a - b| <= 2^-20 max(|a|, |b|)."""
    with np.errstate(invalid="ignore"):
        return np.abs(a - b) <= NEAR * np.maximum(np.abs(a), np.abs(b))


def level_tables(n, pos, xc, ends):
    """Extended knot list, values, B and S of one level (ITD.py:93-116).  pos / xc: interior knots; ends = x[0], x[1], x[n-2], x[n-1]."""
    m = len(pos)
    e = np.concatenate(([0], pos, [n - 1])).astype(np.int64)
    X = np.concatenate(([ends[0]], xc, [ends[3]]))
    B = np.empty(m + 2)
    B[0] = (ends[0] + ends[1]) / 2.0
    B[m + 1] = (ends[2] + ends[3]) / 2.0
    if m:
        k = np.arange(1, m + 1)
        frac = (e[k] - e[k - 1]).astype(np.float64) / (e[k + 1] - e[k - 1]).astype(np.float64)
        B[k] = 0.5 * (X[k - 1] + frac * (X[k + 1] - X[k - 1])) + 0.5 * X[k]
    with np.errstate(all="ignore"):
        S = (B[1:] - B[:-1]) / (X[1:] - X[:-1])           # segments 0 .. m
    return e, X, B, S


def apply_map(n, e, X, B, S, i, xi):
    """baseline at positions i (values xi) through this level's segments; baseline[n-1] = 0."""
    k = np.searchsorted(e[1:-1], i, side="right")         # knots at or before i
    with np.errstate(all="ignore"):
        b = B[k] + S[k] * (xi - X[k])
    return np.where(i == n - 1, 0.0, b)


def _sticky_of(x_level):
    """The hand-over's sticky candidates (itd_knotfirst.hpp:414-437): both samples of every near tie of the first fused level's input
    (positions 1 .. n-2 only) and sample n-2."""
    n = len(x_level)
    # near ties of the level the recursion starts from — NOT the exact ties of the original signal: quantised input grows ties of its
    # own at the first levels (adjacent knots: B_k = x[k-1]/4 + x[k]/2 + x[k+1]/4 is exact on a grid and two neighbours can
    # coincide), a level may break a tie by one ulp and the next one restore it, and neighbours a few thousand ulps apart can
    # collapse a few levels on (differences shrink geometrically from level to level)
    x64 = np.asarray(x_level, dtype=np.float64)
    ties = np.flatnonzero(near(x64[:-1], x64[1:]))
    sticky = np.unique(np.concatenate((ties, ties + 1, [n - 2])))
    return sticky[(sticky >= 1) & (sticky <= n - 2)]


def _per_workgroup(pos, n, tiles):
    """How many of the positions `pos` each knot-side workgroup owns: workgroup w owns tiles [w * tiles, (w + 1) * tiles) of TILE samples,
    the last one of a signal whatever is left (itd_knotfirst.hpp:322).  Halo knots are not counted: the kernel's c and ck are sums over
    the workgroup's own tiles' flag words (itd_knotfirst.hpp:447-448) and over its own survivors (itd_knotfirst.hpp:776-787)."""
    span = tiles * TILE
    return np.bincount(np.asarray(pos, dtype=np.int64) // span, minlength=(n + span - 1) // span)


def knot_trace(x_level, n_extract, knots_fn):
    """The recursion on the knot list, level after level, never giving up (the GPU's workgroups that have not failed run on to the last
    level too): `n_extract` extractions starting from the level whose input x_level is given in full.  One record per level: the
    tables (pos, e, X, B, S, ends), `cand` the candidates at the top of the level, `surv` the candidates it leaves for the next one
    (knots and sticky ones), `nonfinite` whether the level's B, S or mapped triples hold a non-finite value (itd_knotfirst.hpp:717,749).
    Returns the records and the knot list of the last pending baseline."""
    n = len(x_level)
    sticky = _sticky_of(x_level)
    pos = np.asarray(knots_fn(x_level), dtype=np.int64)
    cand = np.unique(np.concatenate((pos, sticky)))
    is_knot = np.isin(cand, pos)
    tri = np.stack([x_level[cand - 1], x_level[cand], x_level[cand + 1]], axis=1).astype(np.float64)
    ends = np.array([x_level[0], x_level[1], x_level[n - 2], x_level[n - 1]], dtype=np.float64)
    sticky_set = set(sticky.tolist())
    levels = []
    for _ in range(n_extract):
        kp, kx = cand[is_knot], tri[is_knot, 1]
        e, X, B, S = level_tables(n, kp, kx, ends)
        # the three samples of every candidate, and the four end samples, through this level's maps
        idx = np.stack([cand - 1, cand, cand + 1], axis=1)
        new = apply_map(n, e, X, B, S, idx.ravel(), tri.ravel()).reshape(-1, 3)
        nonfinite = not (np.all(np.isfinite(B)) and np.all(np.isfinite(S)) and np.all(np.isfinite(new)))
        new_ends = apply_map(n, e, X, B, S, np.array([0, 1, n - 2, n - 1]), ends)
        flag = _predicate(new[:, 0], new[:, 1], new[:, 2])
        tie = near(new[:, 0], new[:, 1]) | near(new[:, 1], new[:, 2])
        sticky_set.update(cand[tie].tolist())
        keep = flag | np.isin(cand, np.fromiter(sticky_set, dtype=np.int64, count=len(sticky_set)))
        levels.append({"pos": kp, "e": e, "X": X, "B": B, "S": S, "ends": ends.copy(), "cand": cand, "surv": cand[keep],
                       "nonfinite": nonfinite})
        cand, tri, is_knot, ends = cand[keep], new[keep], flag[keep], new_ends
    return levels, cand[is_knot]


def knot_side_loads(n, levels, tiles):
    """What the knot side's three capacities are compared with, as the kernel counts it, the maximum over the workgroups of `tiles`
    tiles (the last one of a signal ragged) — per level where the limit is one:
      "kKcCapH"  candidates (knots or sticky) of a workgroup's own tiles at the hand-over: c <= kKcCapH       itd_knotfirst.hpp:451,475
      "kKcCap"   [level] the candidates a level leaves (knots or sticky, the workgroup's own): <= kKcCap     itd_knotfirst.hpp:787
      "kKcSlab"  [level] table entries at the top of a level: toff + ck + 2 <= kKcSlab, ck the workgroup's own knots of the level,
                 toff the sum of ck + 2 over the levels before (the two halo entries of every level ARE counted)   itd_knotfirst.hpp:523,838
    Every workgroup runs every level up to max_iteration + 1, also behind a natural stop, so all levels given are counted."""
    toff = np.zeros((n + tiles * TILE - 1) // (tiles * TILE), dtype=np.int64)
    cap, slab = [], []
    for L in levels:
        ck = _per_workgroup(L["pos"], n, tiles)
        slab.append(int(np.max(toff + ck + 2)))
        cap.append(int(np.max(_per_workgroup(L["surv"], n, tiles))))
        toff += ck + 2
    return {"kKcCapH": int(np.max(_per_workgroup(levels[0]["cand"], n, tiles))), "kKcCap": cap, "kKcSlab": slab}


def knot_side_capacity(n, levels, tiles):
    """(index of the first level at which some workgroup outgrows a capacity, which one) in the kernel's order of checks, or None."""
    loads = knot_side_loads(n, levels, tiles)
    if loads["kKcCapH"] > K_KC_CAP_H:
        return 0, "kKcCapH"
    for q in range(len(levels)):
        if loads["kKcSlab"][q] > K_KC_SLAB:
            return q, "kKcSlab"
        if loads["kKcCap"][q] > K_KC_CAP:
            return q, "kKcCap"
    return None


def knot_side(x_level, x0, n_extract, knots_fn, tiles=None):
    """knot_trace for callers that want the tables or an honest refusal: raises NeedFallback on non-finite knot data and, given the
    `tiles` per knot-side workgroup (16, 32 or 64), where a workgroup outgrows one of the knot side's capacities.  x0: the original signal (unused since round 4: the sticky
    candidates come from the near ties of x_level).  Returns the per-level tables and the knot list of the last pending baseline."""
    levels, last = knot_trace(x_level, n_extract, knots_fn)
    full = knot_side_capacity(len(x_level), levels, tiles) if tiles else None
    bad = [q for q, L in enumerate(levels) if L["nonfinite"]]
    if full is not None and (not bad or full[0] <= bad[0]):
        raise NeedFallback("a workgroup of %d tiles outgrows %s at fused level index %d" % (tiles, full[1], full[0]))
    if bad:
        raise NeedFallback("non-finite knot data at fused level index %d" % bad[0])
    return levels, last


def sample_pass(x_level, levels, next_knots):
    """Every sample through the fused levels; returns the list of baselines and the per-level knot lists re-derived from the
    samples themselves (the verification)."""
    n = len(x_level)
    i = np.arange(n)
    cur = np.asarray(x_level, dtype=np.float64)
    bases, found = [], []
    for L in levels:
        b = apply_map(n, L["e"], L["X"], L["B"], L["S"], i, cur)
        bases.append(b)
        f = np.zeros(n, bool)
        f[1:-1] = _predicate(b[:-2], b[1:-1], b[2:])
        found.append(np.flatnonzero(f))
        cur = b
    return bases, found


def level0_in_reach(x, knots0):
    """The fused level-0 launch (itd_kernels.hpp:1618-1676, kReach = 8) takes a tile's two halo knots in front and three behind from the
    128 samples next to the tile and, where those hold too few, from at most 8 windows of 510 new samples per side: positions
    [s - 4207, s - 1] in front of a tile starting at s, [s + 512, s + 4718] behind it.  Fewer than 2 / 3 knots there, with the walk not
    at the signal's end (s - 4208 > 0 / s + 4719 < n - 1), raise SigState::l0_fail: level 0 is then not finished by this launch and the
    fused levels hand the signal back (odd_input, itd_knotfirst.hpp:351,392-396)."""
    n = len(x)
    k = np.asarray(knots0, dtype=np.int64)
    s = np.arange(0, n, TILE, dtype=np.int64)
    front = np.searchsorted(k, s, side="left") - np.searchsorted(k, s - L0_REACH, side="right")      # knots in (s - 4208, s)
    rear = np.searchsorted(k, s + TILE + L0_REACH - 1, side="left") - np.searchsorted(k, s + TILE, side="left")   # [s + 512, s + 4719)
    bad = ((front < 2) & (s - L0_REACH > 0)) | ((rear < 3) & (s + TILE + L0_REACH - 1 < n - 1))
    return not np.any(bad)


def decide(x, max_iteration, first_fused_level, tiles, oracle=None):
    """What the fused sparse levels do with signal x (float32 or float64, as the caller hands it over) in a call of `max_iteration`
    whose levels first_fused_level .. max_iteration + 1 run fused with `tiles` tiles per knot-side workgroup and no cap.  Returns a dict:
      outcome   "delivered" or "refused"
      bits      the kernel's fail bits, 0 when delivered: 1 verification, 2 capacity, 4 non-finite (every reason that applies)
      level     the lowest level at which the model meets a reason (the first fused level for the hand-over's rules), None: delivered
      fail_lev  what KfSig::fail_lev records: that level for a verification failure of the sample pass (itd_knotfirst.hpp:1245-1247)
                and for non-finite knot data (:875); 99 for everything else — the hand-over's rules (:397), capacities (:412), a
                non-finite sample (:1233), the last pending baseline's count (:154): only the first two teach the engine a cap
      fused     False: the signal stopped before the first fused level (:359-365,392), nothing runs fused and nothing can fail
      lend      the last fused level (KfSig::lend), `natural` its stop; mlev: {level: knots of the level's input} as the knot side
                counts them, first_fused_level .. lend + 1; what: the reasons in words
      levels / bases / last   the knot side's tables, the sample pass's baselines and the last pending baseline's knots (delivered or
                refused by the sample pass), for the comparison with the pinned oracle.
    `oracle`: the pinned oracle's module (oracle.cpu_oracle: knots, itd_baseline_extract) for the levels in front of the fused ones."""
    if oracle is None:
        from oracle import cpu_oracle as oracle
    M, L0 = int(max_iteration), int(first_fused_level)
    if not (2 <= L0 <= M) or tiles not in (16, 32, 64):
        raise ValueError("fused levels: 2 <= first fused level <= max_iteration, 16 / 32 / 64 tiles per workgroup")
    x = np.asarray(x)
    n = len(x)
    out = {"outcome": "delivered", "bits": 0, "level": None, "fail_lev": 99, "fused": False, "lend": -1, "natural": 0, "mlev": {}, "what": []}

    def refuse(bit, level, fail_lev, what):
        out["outcome"] = "refused"
        out["bits"] |= bit
        out["level"] = level if out["level"] is None else min(out["level"], level)
        out["fail_lev"] = min(out["fail_lev"], fail_lev)
        out["what"].append(what)

    # ---- hand-over eligibility (itd_knotfirst.hpp:351,359-365,392-403).  An unfinished level 0 comes first: the levels behind it ran on
    #      that launch's incomplete baseline, so whether the knot side then sees a stop (which would take precedence, :396) is not the
    #      signal's property — the GPU refuses every such case of the table, also one that really stops before the first fused level
    cur = np.asarray(x, dtype=np.float64)
    knots0 = oracle.knots(cur)
    odd = []
    if np.any(np.isnan(cur)):
        odd.append("a NaN in the input (SigState::in_nan)")
    if len(knots0) >= 2 and not level0_in_reach(x, knots0):
        refuse(FAIL_NONFINITE, L0, 99, "level 0 not finished inside the fused launch's reach (SigState::l0_fail)")
        return out
    stopped = len(knots0) < 2
    for j in range(L0):
        if stopped:
            break
        _, cur = oracle.itd_baseline_extract(cur)
        if np.any(np.isnan(cur)):
            odd.append("a NaN in the baseline behind level %d (SigState::nan_mask)" % j)
        stopped = len(oracle.knots(cur)) < 2
    if stopped:
        return out
    if odd:
        refuse(FAIL_NONFINITE, L0, 99, "; ".join(odd))
        return out
    out["fused"] = True
    # ---- the knot side: every level L0 .. M + 1, the stop rules from the list sizes (itd_knotfirst.hpp:860-863)
    levels, last = knot_trace(cur, M + 2 - L0, oracle.knots)
    counts = [len(L["pos"]) for L in levels] + [len(last)]
    lend, natural = M + 1, 0
    for q in range(M + 2 - L0):
        if counts[q + 1] < 2:
            lend, natural = L0 + q, 1
            break
    out.update(lend=lend, natural=natural, mlev={L0 + q: counts[q] for q in range(lend - L0 + 2)})
    out["loads"] = knot_side_loads(n, levels, tiles)
    out["loads"]["kKfCap"] = [int(np.max(np.bincount(L["pos"] // TILE, minlength=1))) for L in levels[: lend - L0 + 1]]
    full = knot_side_capacity(n, levels, tiles)
    if full is not None:
        refuse(FAIL_CAPACITY, L0 + full[0], 99, "a workgroup outgrows %s at level %d" % (full[1], L0 + full[0]))
    bad = [L0 + q for q, L in enumerate(levels) if L["nonfinite"]]
    if bad and bad[0] <= lend:          # (itd_knotfirst.hpp:866: non-finite knot data behind the stop is nobody's)
        refuse(FAIL_NONFINITE, bad[0], bad[0], "non-finite knot data at level %d" % bad[0])
    if out["bits"]:
        return out                      # (itd_knotfirst.hpp:1052: the sample pass does not run for a signal the knot side refused)
    # ---- the sample pass: levels L0 .. lend, then the count of the pending baseline's knots
    used = levels[: lend - L0 + 1]
    bases, found = sample_pass(cur, used, last)
    out.update(levels=used, bases=bases, last=found[-1])
    for q, L in enumerate(used):
        if np.any(np.bincount(L["pos"] // TILE, minlength=1) > K_KF_CAP):          # itd_knotfirst.hpp:1146
            refuse(FAIL_CAPACITY, L0 + q, 99, "a tile holds more than kKfCap knots at level %d" % (L0 + q))
        if not np.all(np.isfinite(bases[q])):                                      # itd_knotfirst.hpp:1233
            refuse(FAIL_NONFINITE, L0 + q, 99, "a non-finite sample at level %d" % (L0 + q))
        if q >= 1 and not np.array_equal(found[q - 1], L["pos"]):                  # V0, itd_knotfirst.hpp:1133-1138,1245-1247
            refuse(FAIL_VERIFY, L0 + q, L0 + q, "the samples' knots of level %d differ from the knot side's" % (L0 + q))
    if not out["bits"]:                 # kf_sig_verdict's own checks, itd_knotfirst.hpp:154,157
        m_exact = len(found[-1])
        if (m_exact >= 2) if natural else (m_exact < 2):
            refuse(FAIL_VERIFY, lend + 1, 99, "the last pending baseline's exact knot count (%d) falls on the other side of 2" % m_exact)
        if any(counts[q] < 2 for q in range(1, lend - L0 + 1)):
            refuse(FAIL_VERIFY, L0 + 1, 99, "a decomposed level with fewer than 2 knots")
    return out
