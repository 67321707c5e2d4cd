// itd_fft.hpp — a batched complex float64 FFT for gfx950 and the Fourier mode selectors of itd_fourier_decomposition.py.
//
// Tier 1 (k_fft_lds): one workgroup per transform of n <= 8192 points, the whole transform in LDS (16 B per point: 128 KiB at
// 8192, within the 160 KiB of a CU).  Stockham auto-sort stages over the factors of n: radices 8 / 4 / 2 / 3 / 5 / 7 as unrolled
// butterflies held in registers (butterfly<R>), any other prime p as a generic O(p)-per-output stage with a compensated sum.
// A stage reads all of its inputs into registers, synchronises and writes its outputs back over them: one LDS buffer, not two.
// Twiddles come from the exact index (j * k) mod n in int64, folded into the first octant, and sincospi of that ratio — never
// from an accumulated angle.
// Inputs may be real or complex, outputs complex or their real part, both strided; a workgroup may multiply its input by
// W_m^{(x * i) mod m} first (x = blockIdx.x), the twiddle step of the four-step form.
//
// Tiers 2 and 3 (host side, itd_fourier.inc): n = n1 * n2 with n1, n2 <= 8192 as four steps (columns, twiddle, rows) of k_fft_lds;
// every other n by Bluestein's chirp over a power-of-two length M >= 2n - 1 (itself one tier-1 or four-step transform).
//
// k_fourier_select<VALID>: fourier_mode_decomposition_any (:171-209) / _valid (:131-168) on a row's forward spectrum, in place:
// the decision, then the masked spectrum xn (complex64-rounded, the reference's dtype) ready for the full complex inverse.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fft {

constexpr int kLdsMax = 8192;        // largest tier-1 transform
constexpr int kSelThreads = 256;

// transform t of a launch (t = blockIdx.y + t0) starts at (t / per) * ss + (t % per) * bs + blockIdx.x * xs; element i at i * es.
// Units: elements of the array (double for a real side, double2 for a complex one).
struct Side {
    double *p;
    int64_t es, xs, bs, ss, t0;
    int per, real;
};

struct LdsArgs {
    Side in, out;
    int n, inverse;
    int64_t tw_m;        // != 0: input i of the workgroup times W_{tw_m}^{(blockIdx.x * i) mod tw_m}
    double scale;
};

// the next Stockham radix of what is left of n (m = n / Ns): 8s first, then 4, 2, then the smallest odd prime factor
__device__ inline int next_radix(int m)
{
    if (m % 8 == 0) return 8;
    if (m % 4 == 0) return 4;
    if (m % 2 == 0) return 2;
    int p = 3;
    while (m % p) p += 2;
    return p;
}

__device__ inline double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ inline double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }

// exp(-+ 2 pi i e / m): e reduced mod m exactly, then the angle folded into the first octant in integers (t / 8m of a turn,
// t <= m), so the one rounding in the ratio moves the angle by at most 2^-54 * pi / 4 and the quarter turns come out exact
// (the ratio over (-1, 1] cost the radix-5 / 7 factors an ulp, which a constant row showed as 60 units in its empty outputs)
__device__ inline double2 twiddle(int64_t e, int64_t m, int inverse)
{
    e %= m;
    if (e < 0) e += m;
    int64_t t = 8 * e;
    const bool neg_s = t > 4 * m;
    if (neg_s) t = 8 * m - t;
    const bool neg_c = t > 2 * m;
    if (neg_c) t = 4 * m - t;
    const bool swap = t > m;
    if (swap) t = 2 * m - t;
    double s, c;
    sincospi((double)t / (double)(4 * m), &s, &c);
    if (swap) { const double x = s; s = c; c = x; }
    if (neg_c) c = -c;
    if (neg_s) s = -s;
    return make_double2(c, inverse ? s : -s);
}

__device__ inline int64_t side_off(const Side &s, int64_t t)
{
    return (t / s.per) * s.ss + (t % s.per) * s.bs + (int64_t)blockIdx.x * s.xs;
}

// a * W_4 = a * (-+ i)
__device__ inline double2 crot(double2 a, int inverse) { return inverse ? make_double2(-a.y, a.x) : make_double2(a.y, -a.x); }

// the 4-point transform of a0 .. a3 by sums and differences alone
__device__ inline void dft4(double2 a0, double2 a1, double2 a2, double2 a3, int inverse, double2 *X)
{
    const double2 t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = crot(csub(a1, a3), inverse);
    X[0] = cadd(t0, t2); X[1] = cadd(t1, t3); X[2] = csub(t0, t2); X[3] = csub(t1, t3);
}

// out_k = sum_r v_r W_R^{r k}, wR[k] = W_R^k.  Equal inputs must cancel as well as they can (a constant or a pure tone puts a whole
// row into one output; what the other outputs keep of it is their error):
//   R = 8: the 4-point transforms of the even and of the odd inputs joined by W_8^k: sums and differences first, equal inputs cancel
//          exactly (the plain 8-term sum left an ulp of the inputs in every output)
//   odd R: the inputs r and R - r share a cosine and a sine; cos(2 pi / 3) is -1/2 exactly, so radix 3 cancels exactly too
//   R = 2, 4: the plain sum (its factors are 0 and +-1: exact)
template <int R>
__device__ inline void butterfly(const double2 *v, const double2 *wR, int inverse, double2 *out)
{
    if constexpr (R == 8) {
        double2 E[4], O[4];
        dft4(v[0], v[2], v[4], v[6], inverse, E);
        dft4(v[1], v[3], v[5], v[7], inverse, O);
        O[1] = cmul(O[1], wR[1]); O[2] = crot(O[2], inverse); O[3] = cmul(O[3], wR[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) { out[k] = cadd(E[k], O[k]); out[k + 4] = csub(E[k], O[k]); }
    } else if constexpr (R % 2 == 1) {
        constexpr int H = (R - 1) / 2;
        double2 p[H], m[H];
#pragma unroll
        for (int r = 1; r <= H; ++r) { p[r - 1] = cadd(v[r], v[R - r]); m[r - 1] = csub(v[r], v[R - r]); }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            double2 acc = v[0];
#pragma unroll
            for (int r = 1; r <= H; ++r) {
                const double2 w = wR[(r * k) % R];
                const double c = (R == 3 && k) ? -0.5 : w.x;
                acc = cadd(acc, make_double2(p[r - 1].x * c - m[r - 1].y * w.y, p[r - 1].y * c + m[r - 1].x * w.y));
            }
            out[k] = acc;
        }
    } else {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            double2 acc = v[0];
#pragma unroll
            for (int r = 1; r < R; ++r) acc = cadd(acc, cmul(v[r], wR[(r * k) % R]));
            out[k] = acc;
        }
    }
}

// one Stockham stage of radix R (2..8) over n points in LDS: butterfly j reads j + r n/R, writes (j / Ns) Ns R + j % Ns + k Ns
template <int R>
__device__ inline void stage_small(double2 *sb, int n, int Ns, int inverse)
{
    constexpr int Q = (8 + R - 1) / R;      // butterflies per thread: n <= 8 * blockDim.x
    const int nR = n / R, tid = threadIdx.x, nt = blockDim.x;
    double2 wR[R];
#pragma unroll
    for (int k = 0; k < R; ++k) wR[k] = twiddle(k, R, inverse);
    double2 reg[Q][R];
    const int64_t span = n / (Ns * R);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int j = tid + q * nt;
        if (j < nR) {
            const int jm = j % Ns;
            double2 v[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                v[r] = sb[j + r * nR];
                if (r && jm) v[r] = cmul(v[r], twiddle((int64_t)r * jm * span, n, inverse));
            }
            butterfly<R>(v, wR, inverse, reg[q]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int j = tid + q * nt;
        if (j < nR) {
            const int base = (j / Ns) * Ns * R + j % Ns;
#pragma unroll
            for (int k = 0; k < R; ++k) sb[base + k * Ns] = reg[q][k];
        }
    }
    __syncthreads();
}

// a stage of any radix R: every output as its own O(R) sum (Kahan's)
__device__ inline void stage_generic(double2 *sb, int n, int Ns, int R, int inverse)
{
    const int nR = n / R, tid = threadIdx.x, nt = blockDim.x;
    const int64_t span = n / (Ns * R);
    double2 reg[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int o = tid + q * nt;
        if (o < n) {
            const int j = o % nR, k = o / nR;
            const int64_t step = (int64_t)(j % Ns + k * Ns) * span;
            // a compensated sum: R terms of one phase (a tone, a constant) round the same way at every step, and the plain sum
            // drifted by up to R / 2 ulps of the output (1e-13 of the peak at R = 8191)
            double2 acc = sb[j], lost = make_double2(0.0, 0.0);
            for (int r = 1; r < R; ++r) {
                const double2 y = csub(cmul(sb[j + r * nR], twiddle(r * step, n, inverse)), lost);
                const double2 t = cadd(acc, y);
                lost = csub(csub(t, acc), y);
                acc = t;
            }
            reg[q] = acc;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int o = tid + q * nt;
        if (o < n) {
            const int j = o % nR, k = o / nR;
            sb[(j / Ns) * Ns * R + j % Ns + k * Ns] = reg[q];
        }
    }
    __syncthreads();
}

// one transform of n <= 8192 points per workgroup (n / 8 <= blockDim.x <= MAXT), dynamic LDS n * 16 bytes.  MAXT sets the register
// budget: 1024 threads leave 128 VGPRs a lane, 256 leave 512 (the short transforms take that instance)
template <int MAXT>
__global__ void __launch_bounds__(MAXT) k_fft_lds(LdsArgs a)
{
    extern __shared__ double2 sb[];
    const int n = a.n, tid = threadIdx.x, nt = blockDim.x;
    const int64_t ti = (int64_t)blockIdx.y + a.in.t0, to = (int64_t)blockIdx.y + a.out.t0;
    const int64_t io = side_off(a.in, ti), oo = side_off(a.out, to);
    for (int i = tid; i < n; i += nt) {
        const int64_t at = io + (int64_t)i * a.in.es;
        double2 v = a.in.real ? make_double2(a.in.p[at], 0.0) : reinterpret_cast<const double2 *>(a.in.p)[at];
        if (a.tw_m) v = cmul(v, twiddle((int64_t)blockIdx.x * i, a.tw_m, a.inverse));
        sb[i] = v;
    }
    __syncthreads();
    // (the radices are derived here, not read from an array in the arguments: indexing one would copy the arguments to scratch)
    for (int Ns = 1; Ns < n;) {
        const int R = next_radix(n / Ns);
        switch (R) {
        case 2: stage_small<2>(sb, n, Ns, a.inverse); break;
        case 3: stage_small<3>(sb, n, Ns, a.inverse); break;
        case 4: stage_small<4>(sb, n, Ns, a.inverse); break;
        case 5: stage_small<5>(sb, n, Ns, a.inverse); break;
        case 7: stage_small<7>(sb, n, Ns, a.inverse); break;
        case 8: stage_small<8>(sb, n, Ns, a.inverse); break;
        default: stage_generic(sb, n, Ns, R, a.inverse); break;
        }
        Ns *= R;
    }
    for (int i = tid; i < n; i += nt) {
        const int64_t at = oo + (int64_t)i * a.out.es;
        const double2 v = sb[i];
        if (a.out.real) a.out.p[at] = v.x * a.scale;
        else reinterpret_cast<double2 *>(a.out.p)[at] = make_double2(v.x * a.scale, v.y * a.scale);
    }
}

// ---- Bluestein: X[k] = c*_k sum_j (x_j c*_j) c_{k-j}, c_j = exp(i pi j^2 / n), j^2 taken mod 2n exactly -------------------
__device__ inline double2 chirp(int64_t j, int64_t n, bool conj_)
{
    int64_t e = (j * j) % (2 * n);       // j < 2^31: j^2 < 2^62
    if (e > n) e -= 2 * n;
    double s, c;
    sincospi((double)e / (double)n, &s, &c);
    return make_double2(c, conj_ ? -s : s);
}

// A[t][j] = (inverse ? conj(x) : x)_j * conj(c_j) for j < n, 0 up to M
__global__ void k_blue_pre(Side in, int64_t n, int64_t M, int inverse, double2 *A)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    const int64_t t = (int64_t)blockIdx.y + in.t0;
    double2 v = make_double2(0.0, 0.0);
    if (j < n) {
        const int64_t at = (t / in.per) * in.ss + (t % in.per) * in.bs + j * in.es;
        v = in.real ? make_double2(in.p[at], 0.0) : reinterpret_cast<const double2 *>(in.p)[at];
        if (inverse) v.y = -v.y;
        v = cmul(v, chirp(j, n, true));
    }
    A[(int64_t)blockIdx.y * M + j] = v;
}

// the chirp's circulant: b[m] = c_m for m < n, b[M - m] = c_m for 0 < m < n, 0 between
__global__ void k_blue_chirp(int64_t n, int64_t M, double2 *b)
{
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    double2 v = make_double2(0.0, 0.0);
    if (m < n) v = chirp(m, n, false);
    else if (M - m < n) v = chirp(M - m, n, false);
    b[m] = v;
}

__global__ void k_cmul_rows(double2 *A, const double2 *__restrict__ B, int64_t M)
{
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m < M) A[(int64_t)blockIdx.y * M + m] = cmul(A[(int64_t)blockIdx.y * M + m], B[m]);
}

// out_k = conj(c_k) * A[t][k] (conjugated and / n for an inverse)
__global__ void k_blue_post(const double2 *__restrict__ A, int64_t n, int64_t M, int inverse, Side out)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t t = (int64_t)blockIdx.y + out.t0;
    double2 v = cmul(A[(int64_t)blockIdx.y * M + k], chirp(k, n, true));
    if (inverse) v = make_double2(v.x / (double)n, -v.y / (double)n);
    const int64_t at = (t / out.per) * out.ss + (t % out.per) * out.bs + k * out.es;
    if (out.real) out.p[at] = v.x;
    else reinterpret_cast<double2 *>(out.p)[at] = v;
}

// ---- the mode selectors ------------------------------------------------------------------------------------------------
// a = |X| over the first half; numpy's argmax / argmin: the first index wins a tie
__device__ inline double mag(const double2 *X, int64_t i) { const double2 v = X[i]; return hypot(v.x, v.y); }

template <bool MAX>
__device__ inline bool better(double v, int64_t i, double bv, int64_t bi)
{
    return MAX ? (v > bv || (v == bv && i < bi)) : (v < bv || (v == bv && i < bi));
}

// the block's best (v, i) pair; i < 0 marks an empty slot
template <bool MAX>
__device__ int64_t block_arg(double v, int64_t i, double *sv, int64_t *si)
{
    const int tid = threadIdx.x;
    sv[tid] = v; si[tid] = i;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (tid < s && si[tid + s] >= 0 && (si[tid] < 0 || better<MAX>(sv[tid + s], si[tid + s], sv[tid], si[tid]))) {
            sv[tid] = sv[tid + s]; si[tid] = si[tid + s];
        }
        __syncthreads();
    }
    const int64_t r = si[0];
    __syncthreads();
    return r;
}

// argmax / argmin of a over [lo, hi); -1 if empty
template <bool MAX>
__device__ int64_t range_arg(const double2 *X, int64_t lo, int64_t hi, double *sv, int64_t *si)
{
    double bv = 0.0;
    int64_t bi = -1;
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const double v = mag(X, i);
        if (bi < 0 || better<MAX>(v, i, bv, bi)) { bv = v; bi = i; }
    }
    return block_arg<MAX>(bv, bi, sv, si);
}

__device__ inline bool strict_peak(const double2 *X, int64_t i)
{
    const double c = mag(X, i);
    return c > mag(X, i - 1) && c > mag(X, i + 1);
}

// one workgroup per row of n points (Xall: rows of n complex, the forward spectra; overwritten with xn).
// rec[8] per row: status (1 = a mode was built, 0 = rejected), peak_max, first_peak, last_peak, mina, minb, 0, 0 (-1: not reached)
template <bool VALID>
__global__ void __launch_bounds__(kSelThreads) k_fourier_select(double2 *Xall, int64_t n, int32_t *rec_all)
{
    __shared__ double sv[kSelThreads];
    __shared__ int64_t si[kSelThreads];
    __shared__ unsigned long long s_cnt;
    double2 *X = Xall + (int64_t)blockIdx.x * n;
    const int64_t half = n / 2;
    int64_t pm = -1, fp = -1, lp = -1, mina = -1, minb = -1;
    bool ok = false;
    if (!VALID) {
        // :183-197
        pm = range_arg<true>(X, 1, half, sv, si);
        if (pm >= 0 && pm != 1 && pm != half - 1) {
            fp = range_arg<true>(X, 0, pm, sv, si);
            lp = range_arg<true>(X, pm + 1, half, sv, si);
            ok = !(fp == pm - 1 || lp == pm + 1);
        }
    } else {
        // :137-158: the strict maxima in 1 .. half-2; the highest (the stable descending sort: the first wins a tie); the
        // closest one below pm - 1 and the closest above pm + 1
        if (threadIdx.x == 0) s_cnt = 0;
        __syncthreads();
        double bv = 0.0;
        int64_t bi = -1;
        unsigned long long cnt = 0;
        for (int64_t i = 1 + threadIdx.x; i < half - 1; i += blockDim.x)
            if (strict_peak(X, i)) {
                ++cnt;
                const double v = mag(X, i);
                if (bi < 0 || better<true>(v, i, bv, bi)) { bv = v; bi = i; }
            }
        if (cnt) atomicAdd(&s_cnt, cnt);
        pm = block_arg<true>(bv, bi, sv, si);     // (its barriers order the count too)
        if (s_cnt >= 3) {
            int64_t below = -1, above = -1;
            for (int64_t i = 1 + threadIdx.x; i < half - 1; i += blockDim.x)
                if (strict_peak(X, i)) {
                    if (i < pm - 1 && i > below) below = i;
                    if (i > pm + 1 && (above < 0 || i < above)) above = i;
                }
            // the largest `below`, the smallest `above` (an index is its own value)
            fp = block_arg<true>((double)below, below, sv, si);
            lp = block_arg<false>((double)above, above, sv, si);
            ok = fp >= 0 && lp >= 0;
            if (!ok) fp = lp = -1;      // (:153-154: neither is drawn unless both exist)
        } else {
            pm = -1;
        }
    }
    if (ok) {
        // :200-203
        mina = range_arg<false>(X, fp, pm + 1, sv, si);
        minb = range_arg<false>(X, pm, lp + 1, sv, si);
    }
    __syncthreads();
    // xn[mina:minb] = X[mina:minb]; xn[-minb:-mina] = X[-minb:-mina] (empty when mina == 0), in complex64
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const bool keep = ok && ((i >= mina && i < minb) || (mina > 0 && i >= n - minb && i < n - mina));
        const double2 v = X[i];
        X[i] = keep ? make_double2((double)(float)v.x, (double)(float)v.y) : make_double2(0.0, 0.0);
    }
    if (threadIdx.x == 0) {
        int32_t *r = rec_all + (int64_t)blockIdx.x * 8;
        r[0] = ok ? 1 : 0; r[1] = (int32_t)pm; r[2] = (int32_t)fp; r[3] = (int32_t)lp; r[4] = (int32_t)mina; r[5] = (int32_t)minb;
        r[6] = 0; r[7] = 0;
    }
}

// ---- the cascade's elementwise steps (itd_fourier_decomposition.py:39-45, :230-241) -----------------------------------------
// rotation = problem - baseline -> row k; problem = problem - rotation (literally: not the baseline bit for bit); the last band
// also writes the residual row
__global__ void k_band_step(double *__restrict__ prob, const double *__restrict__ base, double *__restrict__ rows, int64_t n, int64_t R,
                            int k, int last)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (i >= n) return;
    const double p = prob[s * n + i], rot = p - base[s * n + i], q = p - rot;
    rows[(s * R + k) * n + i] = rot;
    prob[s * n + i] = q;
    if (last) rows[(s * R + R - 1) * n + i] = q;
}

// one workgroup per (slot, row): not np.allclose(mode, 0) (:232) = some |mode| > 1e-8 (atol; rtol * 0 = 0); then row -= mode
// (:237) and, in the lean form, acc[signal][row] += mode (:285)
__global__ void __launch_bounds__(kSelThreads) k_fourier_apply(const double *__restrict__ modes, double *__restrict__ rows, int64_t n,
                                                               int K, const int32_t *__restrict__ slot_sig, double *__restrict__ acc,
                                                               int32_t *__restrict__ hits, int32_t *__restrict__ any)
{
    __shared__ double sm[kSelThreads];
    const int64_t s = blockIdx.x / K, k = blockIdx.x % K;
    const double *m = modes + (int64_t)blockIdx.x * n;
    double mx = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) mx = fmax(mx, fabs(m[i]));
    sm[threadIdx.x] = mx;
    __syncthreads();
    for (int h = blockDim.x / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + h]);
        __syncthreads();
    }
    const bool hit = sm[0] > 1e-8;
    if (hit) {
        double *r = rows + (s * (K + 1) + k) * n;
        double *a = acc ? acc + ((int64_t)slot_sig[s] * K + k) * n : nullptr;
        for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
            r[i] = r[i] - m[i];
            if (a) a[i] = a[i] + m[i];
        }
    }
    if (threadIdx.x == 0) {
        hits[blockIdx.x] = hit ? 1 : 0;
        if (hit) atomicOr(&any[s], 1);
    }
}

// the next signal: np.sum(rows, axis=0) (:241) — numpy reduces axis 0 row after row in row order
__global__ void k_fourier_sum(const double *__restrict__ rows, int64_t n, int64_t R, const int32_t *__restrict__ any, double *__restrict__ sig)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (i >= n || !any[s]) return;
    const double *r = rows + s * R * n + i;
    double v = r[0];
    for (int64_t k = 1; k < R; ++k) v = v + r[k * n];
    sig[s * n + i] = v;
}

__global__ void k_copy_rows(const double *__restrict__ x, int64_t x_stride, int64_t n, double *__restrict__ out, int32_t *__restrict__ nan_flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (i >= n) return;
    const double v = x[s * x_stride + i];
    out[s * n + i] = v;
    if (v != v) nan_flag[s] = 1;
}

}  // namespace fft
