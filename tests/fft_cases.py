"""Reference, yardsticks and case lists for the FFT and the Fourier mode selectors (itd_fft.hpp, itd_fourier.inc).  No GPU here.

Reference: numpy.fft on numpy.clongdouble input (pocketfft computes in long double: eps 2^-63 on x86-64).
Units: forward u = 2^-53 ||x||2 per row, inverse u = 2^-53 ||x||2 / n; an error is max_k |got_k - ref_k| of a row in units.
Yardsticks on the same input:
  yard_fft   the error of float64 numpy.fft
  yard_seq   where the kernel takes stage_generic (a prime factor > 7 in a tier-1 or four-step sub-transform): the error of a
             float64 direct DFT, twiddles from the exact index (j k) mod n, terms added one by one in index order, on at most 512
             seeded output indices.  A sequential O(p) sum has a larger error constant than pocketfft's Bluestein.
Bound: err <= K max(yard_fft, yard_seq) + F, K = 4, F = 8 units.  K: both sides are backward-stable transforms of different
factorisations (radix-8 butterflies as 8-term sums, sincospi against libm); F: the yardstick is exactly 0 on some structured
inputs.  K and F are the margin, not a measurement (the measured ratios: tools/fft_accuracy.py).

The selector cases are rows synthesised from a designed half spectrum through numpy.fft.irfft, so every magnitude the rules compare
is chosen (gaps of at least 1 per cent), and seeded noisy rows; the expected record of every case is the rules' logic on the
long-double spectrum, and a case counts only when every comparison the rule makes is decided by a relative margin above 2^-40.
"""
import numpy as np

K, F = 4.0, 8.0
EPS = 2.0 ** -53
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)
LONGDOUBLE_WHY = "numpy.longdouble has eps %.3g > 2^-63 here: no long-double reference" % float(np.finfo(np.longdouble).eps)
K_MAX_GRID_Y = 65535          # itd_engine.hip: kMaxGridY
LDS_MAX = 8192                # itd_fft.hpp: kLdsMax
CHUNK_BYTES = 256 << 20       # itd_fourier.inc: kFftChunkBytes
SEQ_INDICES = 512
SEQ_TERMS = 1 << 22           # output indices * n of one direct DFT (memory: 64 MiB of complex128 per row)
MARGIN = 2.0 ** -40


# ---- the host side's choices, restated (itd_fourier.inc, itd_fft.hpp) -------------------------------------------------------
def fft_threads(n):
    t = 64
    while t < 1024 and 8 * t < n:
        t *= 2
    return t


def next_radix(m):
    if m % 8 == 0:
        return 8
    if m % 4 == 0:
        return 4
    if m % 2 == 0:
        return 2
    p = 3
    while m % p:
        p += 2
    return p


def radices(n):
    out, ns = [], 1
    while ns < n:
        out.append(next_radix(n // ns))
        ns *= out[-1]
    return out


def four_step_split(n):
    if n > LDS_MAX * LDS_MAX:
        return 0
    best, d = 0, (n + LDS_MAX - 1) // LDS_MAX
    while d <= LDS_MAX and d * d <= n:
        if n % d == 0:
            best = d
        d += 1
    return best


def bluestein_m(n):
    m = 1
    while m < 2 * n - 1:
        m <<= 1
    return m


def path_of(n):
    """(tier, path): tier 1 'unrolled' / 'generic' (some stage of a prime radix above 7), tier 2 the same over both sub-transforms,
    tier 3 'bluestein'."""
    if n <= LDS_MAX:
        return 1, "generic" if any(r > 8 for r in radices(n)) else "unrolled"
    n1 = four_step_split(n)
    if n1:
        return 2, "generic" if any(r > 8 for r in radices(n1) + radices(n // n1)) else "unrolled"
    return 3, "bluestein"


# (2310 = 2 3 5 7 11 was first listed with the unrolled radices; its factor 11 takes the generic stage, and 210 stands in there)
TIER1_UNROLLED = (1, 2, 8, 64, 512, 4096, 8192, 105, 210, 6720)
TIER1_GENERIC = (11, 13, 121, 88, 1001, 2310, 4099, 8191, 8186)
TIER1_SEAMS = (512, 513, 1024, 1025, 2048, 2049, 4096, 4097)
TIER2 = (8193, 8194, 16382, 16384, 24576, 240240, 1 << 20)
TIER3 = (8209, 10007, 16418, 24627, 65537)
LENGTHS = tuple(dict.fromkeys(TIER1_UNROLLED + TIER1_GENERIC + TIER1_SEAMS + TIER2 + TIER3))


# ---- reference, units, yardsticks -------------------------------------------------------------------------------------------
def ref_fft(x, inverse=False):
    z = np.asarray(x).astype(np.clongdouble)
    return np.fft.ifft(z, axis=-1) if inverse else np.fft.fft(z, axis=-1)


def unit(x, inverse=False):
    """The unit of every row of x[B, n]."""
    x = np.atleast_2d(x)
    u = EPS * np.linalg.norm(x, axis=1)
    return u / x.shape[1] if inverse else u


def err_units(got, ref, u, idx=None):
    """max_k |got_k - ref_k| per row in units (over the output indices idx, if given).  A row of norm 0 has unit 0: its error
    counts as 0 when it is exactly 0, else as infinite."""
    d = np.asarray(got).astype(np.clongdouble) - ref
    if idx is not None:
        d = d[:, idx]
    e = np.max(np.abs(d), axis=1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(u > 0, e / u, np.where(e == 0, 0.0, np.inf))


def seq_indices(n):
    """The seeded output indices of yard_seq: all of them up to 512 points, fewer for long transforms (SEQ_TERMS)."""
    count = max(8, min(SEQ_INDICES, n, SEQ_TERMS // n))
    if count >= n:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.random.default_rng(1000003 * n + 17).choice(n, size=count, replace=False)).astype(np.int64)


def seq_dft(x, inverse, idx):
    """The float64 direct DFT of the rows of x at the output indices idx, the terms added one by one in index order."""
    x = np.atleast_2d(np.asarray(x, dtype=np.complex128))
    n = x.shape[1]
    e = (idx[:, None] * np.arange(n, dtype=np.int64)[None, :]) % n          # exact: idx, j < 2^31
    ang = 2.0 * np.pi * (e / float(n))
    w = np.cos(ang) + (1j if inverse else -1j) * np.sin(ang)
    out = np.empty((x.shape[0], idx.shape[0]), np.complex128)
    for b in range(x.shape[0]):
        out[b] = np.cumsum(x[b][None, :] * w, axis=1)[:, -1]
    return out / n if inverse else out


def takes_generic(n):
    return path_of(n)[1] == "generic"


def yardsticks(x, inverse, ref=None):
    """(ref, unit, yard_fft, yard_seq or None, idx or None) of the rows x[B, n]."""
    x = np.atleast_2d(np.asarray(x, dtype=np.complex128))
    n = x.shape[1]
    ref = ref_fft(x, inverse) if ref is None else ref
    u = unit(x, inverse)
    y_fft = err_units(np.fft.ifft(x, axis=1) if inverse else np.fft.fft(x, axis=1), ref, u)
    if not takes_generic(n):
        return ref, u, y_fft, None, None
    idx = seq_indices(n)
    return ref, u, y_fft, err_units(seq_dft(x, inverse, idx), ref[:, idx], u), idx


def bound(y_fft, y_seq=None):
    return K * (y_fft if y_seq is None else np.maximum(y_fft, y_seq)) + F


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def families(n, light=False):
    """[(family name, row)] of one length: two seeded complex and two real Gaussian rows, unit impulses at 0, 1, n // 2, n - 1,
    pure tones exp(2 pi i k0 j / n) for k0 = 1, n - 1 (index reduced exactly) and a constant.  light: one row per random family
    and one impulse and tone (the 2^20-point case: one pass of that length)."""
    rng = np.random.default_rng(7919 * n + 1)
    out = []
    for r in range(1 if light else 2):
        out.append(("complex%d" % r, rng.standard_normal(n) + 1j * rng.standard_normal(n)))
    for r in range(1 if light else 2):
        out.append(("real%d" % r, rng.standard_normal(n) + 0j))
    for j0 in dict.fromkeys((n - 1,) if light else (0, 1 % n, n // 2, n - 1)):
        z = np.zeros(n, np.complex128)
        z[j0] = 1.0
        out.append(("impulse%d" % j0, z))
    j = np.arange(n, dtype=np.int64)
    for k0 in dict.fromkeys((1 % n,) if light else (1 % n, n - 1)):
        ang = 2.0 * np.pi * (((k0 * j) % n) / float(n))
        out.append(("tone%d" % k0, np.cos(ang) + 1j * np.sin(ang)))
    out.append(("constant", np.full(n, 0.75 + 0j)))
    return out


def family_rows(n):
    fam = families(n, light=n >= 1 << 20)
    return [f[0] for f in fam], np.stack([f[1] for f in fam])


_length_cache = {}


def length_case(n):
    """(names, x[B, n], {inverse: (ref, unit, yard_fft, yard_seq or None, idx or None)}) of one listed length, computed once per
    process for all but the longest transforms and never changed by the tests that share it."""
    if n in _length_cache:
        return _length_cache[n]
    names, x = family_rows(n)
    case = (names, x, {inv: yardsticks(x, inv) for inv in (False, True)})
    if n <= 1 << 17:
        x.setflags(write=False)
        _length_cache[n] = case
    return case


def is_random(name):
    return name.startswith("complex") or name.startswith("real")


# ---- the selectors: the rules with their margins ------------------------------------------------------------------------------
class _Margin:
    def __init__(self):
        self.m = np.inf

    def gap(self, hi, lo):
        """hi > lo was decided: by how much, relative to hi."""
        hi, lo = float(hi), float(lo)
        self.m = min(self.m, (hi - lo) / hi if hi > 0 else 0.0)

    def argmax(self, a, lo, hi):
        seg = a[lo:hi]
        i = int(np.argmax(seg))
        if seg.shape[0] > 1:
            self.gap(seg[i], np.max(np.delete(seg, i)))
        return lo + i

    def argmin(self, a, lo, hi):
        seg = a[lo:hi]
        i = int(np.argmin(seg))
        if seg.shape[0] > 1:
            self.gap(np.min(np.delete(seg, i)), seg[i])
        return lo + i


def decide(a, rule):
    """restate()'s logic (tests/test_fourier_cpu.py) on the magnitudes a = |X| of a whole spectrum: (rec int32[6], the smallest
    relative margin of the comparisons the rule made)."""
    n = a.shape[0]
    half = n // 2
    pm = fp = lp = mina = minb = -1
    ok = False
    mg = _Margin()
    if rule == "any":
        pm = mg.argmax(a, 1, half)
        if pm != 1 and pm != half - 1:
            fp = mg.argmax(a, 0, pm)
            lp = mg.argmax(a, pm + 1, half)
            ok = not (fp == pm - 1 or lp == pm + 1)
    else:
        if half - 1 > 1:
            c, l, r = a[1:half - 1], a[0:half - 2], a[2:half]
            for p, q in ((c, l), (c, r)):
                hi, lo = np.maximum(p, q), np.minimum(p, q)
                with np.errstate(divide="ignore", invalid="ignore"):
                    rel = np.where(hi > 0, (hi - lo) / hi, 0.0)
                mg.m = min(mg.m, float(np.min(rel)))
            peaks = np.flatnonzero((c > l) & (c > r)) + 1
        else:
            peaks = np.zeros(0, np.int64)
        if peaks.shape[0] >= 3:
            k = int(np.argmax(a[peaks]))
            if peaks.shape[0] > 1:
                mg.gap(a[peaks[k]], np.max(np.delete(a[peaks], k)))
            pm = int(peaks[k])
            below, above = peaks[peaks < pm - 1], peaks[peaks > pm + 1]
            if below.shape[0] and above.shape[0]:
                fp, lp, ok = int(below.max()), int(above.min()), True
    if ok:
        mina = mg.argmin(a, fp, pm + 1)
        minb = mg.argmin(a, pm, lp + 1)
    return np.array([int(ok), pm, fp, lp, mina, minb], np.int32), mg.m


def expected(x, rule):
    """(rec, margin, mode) of a real row from its long-double spectrum: the mask, complex64 rounding, the full complex inverse
    and its real part, as the reference builds its mode."""
    X = ref_fft(np.asarray(x, dtype=np.float64))
    rec, margin = decide(np.abs(X), rule)
    n = X.shape[0]
    xn = np.zeros(n, np.complex64)
    if rec[0]:
        mina, minb = int(rec[4]), int(rec[5])
        xn[mina:minb] = X[mina:minb]
        xn[-minb:-mina] = X[-minb:-mina]
    return rec, margin, ref_fft(xn, True).real.astype(np.float64)


SELECTOR_NS = (4, 5, 6, 7, 64, 65, 1000, 1001, 8192, 8193, 10007)
NOISY_NS = (600, 2000, 8193)
NOISY_ROWS = 200


def _row_of(mags, seed):
    """The real row whose spectrum has the magnitudes mags[0 .. n // 2] (seeded phases; bins 0 and, for an even n, n / 2 real)."""
    n = mags["n"]
    m = mags["a"]
    rng = np.random.default_rng(seed)
    H = m * np.exp(2j * np.pi * rng.random(m.shape[0]))
    H[0] = m[0]
    if n % 2 == 0:
        H[-1] = m[-1]
    return np.fft.irfft(H, n)


def _flat(n, seed, **spikes):
    """A seeded background in [1, 2] over bins 0 .. n // 2 with chosen magnitudes at chosen bins."""
    a = 1.0 + np.random.default_rng(seed).random(n // 2 + 1)
    for k, v in spikes.items():
        a[int(k[1:])] = v
    return {"n": n, "a": a}


def _tents(n, peaks):
    """Magnitudes over bins 0 .. n // 2 whose only strict maxima are `peaks` [(bin, log height)]: straight lines in the logarithm
    between each peak and a valley halfway to the next, every step at least 1.2 per cent."""
    m = n // 2 + 1
    s = 0.012
    peaks = sorted(peaks)
    L = np.empty(m)
    p0, h0 = peaks[0]
    L[:p0 + 1] = h0 - s * (p0 - np.arange(p0 + 1))
    for (p, hp), (q, hq) in zip(peaks[:-1], peaks[1:]):
        v = (p + q) // 2
        hv = min(hp - s * (v - p), hq - s * (q - v)) - s
        L[p:v + 1] = np.linspace(hp, hv, v - p + 1)
        L[v:q + 1] = np.linspace(hv, hq, q - v + 1)
    p, hp = peaks[-1]
    L[p:] = hp - s * (np.arange(p, m) - p)
    return {"n": n, "a": np.exp(L)}


def designed_cases():
    """[(name, rule, row, intended rec)]: the record the design aims at (every one is also decided by the rules on the long-double
    spectrum, tests/test_fft_cases_cpu.py).  For n < 8 every `any` row is rejected at peak_max (1 or half - 1) and `valid` has
    fewer than three bins to hold a peak.

    Two cases of the first list of this work cannot exist with decided margins and are replaced by their nearest neighbours:
      first_peak == 0 with mina == 0: mina == 0 needs a[0] <= a[1 .. pm] while first_peak == 0 needs a[0] >= a[1 .. pm - 1]: exact
        ties (the goldens' tie_* cases hold those); here first_peak == 0 with mina > 0.
      mina == minb == peak_max: a[pm] is the largest of bins 1 .. half - 1 (`any`) or exceeds a[pm - 1] (`valid`), so an argmin
        over a range that holds pm and another such bin never lands on pm; here the narrowest mask, mina == pm - 1 and
        minb == pm + 1."""
    out = []
    for n in SELECTOR_NS:
        half = n // 2
        sd = 31 * n

        def add(name, rule, mags, rec, seed=0):
            out.append(("%s_n%d_%s" % (name, n, rule), rule, _row_of(mags, sd + seed), np.array(rec, np.int32)))

        if half < 8:
            add("pm1", "any", _flat(n, sd, k1=9.0), [0, 1, -1, -1, -1, -1])
            if half - 1 > 1:
                add("pmlast", "any", _flat(n, sd + 1, **{"k%d" % (half - 1): 9.0}), [0, half - 1, -1, -1, -1, -1])
            add("nopeaks", "valid", _flat(n, sd + 2, k1=9.0), [0, -1, -1, -1, -1, -1])
            continue
        c = half // 2                 # a bin well inside
        add("pm1", "any", _flat(n, sd, k1=9.0), [0, 1, -1, -1, -1, -1])
        add("pm2", "any", _flat(n, sd + 1, k0=5.0, k1=0.5, k2=9.0, **{"k%d" % c: 0.4, "k%d" % (c + 3): 4.0}), [1, 2, 0, c + 3, 1, c])
        add("pmhalf2", "any", _flat(n, sd + 2, **{"k%d" % (half - 2): 9.0, "k%d" % c: 5.0}), [0, half - 2, c, half - 1, -1, -1])
        add("pmhalf1", "any", _flat(n, sd + 3, **{"k%d" % (half - 1): 9.0}), [0, half - 1, -1, -1, -1, -1])
        add("fp_adjacent", "any", _flat(n, sd + 4, **{"k%d" % c: 9.0, "k%d" % (c - 1): 5.0, "k%d" % (c + 4): 4.0}),
            [0, c, c - 1, c + 4, -1, -1])
        add("lp_adjacent", "any", _flat(n, sd + 5, **{"k%d" % c: 9.0, "k%d" % (c - 4): 5.0, "k%d" % (c + 1): 4.0}),
            [0, c, c - 4, c + 1, -1, -1])
        add("fp0", "any", _flat(n, sd + 6, k0=5.0, k3=0.5, **{"k%d" % c: 9.0, "k%d" % (c + 2): 0.4, "k%d" % (c + 5): 4.0}),
            [1, c, 0, c + 5, 3, c + 2])
        add("narrow", "any", _flat(n, sd + 7, **{"k%d" % c: 9.0, "k%d" % (c - 1): 0.5, "k%d" % (c - 3): 5.0, "k%d" % (c + 1): 0.4,
                                                 "k%d" % (c + 3): 4.0}), [1, c, c - 3, c + 3, c - 1, c + 1])
        add("wide", "any", _flat(n, sd + 8, k2=5.0, k4=0.5, **{"k%d" % c: 9.0, "k%d" % (half - 2): 4.0, "k%d" % (half - 3): 0.4}),
            [1, c, 2, half - 2, 4, half - 3])
        # valid: the strict maxima are the tents' tips; the valley between two tips lies halfway ((p + q) // 2)
        lo, hi = max(3, half // 4), half - max(4, half // 4)
        add("two_peaks", "valid", _tents(n, [(lo, 2.0), (hi, 1.0)]), [0, -1, -1, -1, -1, -1])
        add("three_peaks", "valid", _tents(n, [(lo, 1.0), (c, 3.0), (hi, 2.0)]), [1, c, lo, hi, (lo + c) // 2, (c + hi) // 2])
        add("three_peaks_shifted", "valid", _tents(n, [(lo, 2.5), (c + 1, 3.0), (hi, 1.0)]),
            [1, c + 1, lo, hi, (lo + c + 1) // 2, (c + 1 + hi) // 2])
        add("none_below", "valid", _tents(n, [(lo, 3.0), (c, 1.0), (hi, 2.0)]), [0, lo, -1, -1, -1, -1])
        add("none_above", "valid", _tents(n, [(lo, 1.0), (c, 2.0), (hi, 3.0)]), [0, hi, -1, -1, -1, -1])
        add("below_at_pm_minus_2", "valid", _tents(n, [(lo, 0.5), (c - 2, 2.0), (c, 3.0), (c + 2, 2.5), (hi, 1.0)]),
            [1, c, c - 2, c + 2, c - 1, c + 1])
    return out


def noisy_rows(rule):
    """NOISY_ROWS seeded rows per rule over NOISY_NS: a few sinusoids of random frequency (on and off the bins) and amplitude, an
    offset and white noise of a random level."""
    out = []
    for i in range(NOISY_ROWS):
        n = NOISY_NS[i % len(NOISY_NS)]
        rng = np.random.default_rng(100000 * (1 + (rule == "valid")) + i)
        t = np.arange(n)
        x = rng.uniform(-1, 1) * rng.integers(0, 2) + 10.0 ** rng.uniform(-3, 0) * rng.standard_normal(n)
        for _ in range(int(rng.integers(1, 5))):
            f = rng.uniform(2, n // 2 - 2)
            if rng.random() < 0.5:
                f = round(f)
            x = x + rng.uniform(0.2, 1.0) * np.sin(2 * np.pi * f * t / n + rng.uniform(0, 2 * np.pi))
        out.append(("noisy%03d_n%d_%s" % (i, n, rule), rule, x))
    return out


_selector_cache = {}


def selector_cases(rule):
    """(decided [(name, rule, row, rec, mode)], the share of the noisy rows left out as undecided): designed and noisy rows of
    one rule whose every comparison has a relative margin above 2^-40 on the long-double spectrum.  Computed once."""
    if rule not in _selector_cache:
        decided, left = [], 0
        for name, r, x, _ in designed_cases():
            if r == rule:
                rec, margin, mode = expected(x, rule)
                if margin > MARGIN:
                    decided.append((name, rule, x, rec, mode))
        for name, r, x in noisy_rows(rule):
            rec, margin, mode = expected(x, rule)
            if margin > MARGIN:
                decided.append((name, rule, x, rec, mode))
            else:
                left += 1
        _selector_cache[rule] = (decided, left / float(NOISY_ROWS))
    return _selector_cache[rule]
