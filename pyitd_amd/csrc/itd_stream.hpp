// itd_stream.hpp — device side of the block-wise (streaming) operators, itd_stream_* in include/pyitd_hip.h.
//
// The reference describes block-wise operation in a comment only (itd.cpp:31-38: "use a circular buffer with modulous
// tracking ... re-assess extrema in the entire buffer every iteration ... use from the last extrema in the first buffer to the
// first extrema in the last buffer ... compute only the baseline[i] array for the inner third ... rotate buffers") and the
// reuse of retained extrema along channels (itd.cpp:40-44).  The recipe as built here: include/pyitd_hip.h, DESIGN.md section 7.
//
// The ring: per channel 5 slots of `block` samples.  Block k lives in slot k % 3 and — slots 0 and 1 — a second time in slot
// 3 + k % 3, so the three most recent blocks are always one CONTIGUOUS window (first slot (k - 2) % 3) and every kernel of the
// whole-signal operators runs on it unchanged: modulus tracking without a modulus in the kernels' addressing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itd_cubic.hpp"
#include "itd_resident.hpp"

namespace itd {

// one incoming block of every channel into its slot (and the slot's mirror).  status (optional): |= 2 when a stored sample is a
// NaN — the one place that sees every sample of EVERY channel: under shared knots only channel 0's window is scanned for knots,
// so a NaN in another channel would otherwise go unreported.  (The levels stream keeps its own NaN rule and passes nullptr.)
__global__ void k_stream_store(const double *__restrict__ blk, int64_t in_stride, double *__restrict__ ring, int64_t ring_stride,
                               int64_t L, int slot, int32_t *__restrict__ status)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    const int c = blockIdx.y;
    const double v = blk[(int64_t)c * in_stride + i];
    if (status && v != v) atomicOr(status, 2);
    double *r = ring + (int64_t)c * ring_stride;
    r[(int64_t)slot * L + i] = v;
    if (slot < 2) r[(int64_t)(slot + 3) * L + i] = v;
}

// The knots a window's spline is built on: from `margin` extrema in front of the
// emitted part [lo, hi) to margin + 2 behind it; fewer than 4: no spline (the block is emitted unchanged, itd.cpp:170-172).
// kidx[b]: [0, the window's knots (totals[2b] of them), tail] as k_compact leaves them.  One thread per list.
__global__ void k_stream_select(const int32_t *__restrict__ kidx, int64_t kidx_stride, const int32_t *__restrict__ totals, int n_lists,
                                int lo, int hi, int margin, CubicJob *__restrict__ jobs, int32_t *__restrict__ status)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_lists) return;
    const int32_t *k = kidx + (int64_t)b * kidx_stride + 1;
    const int m = totals[2 * b];
    auto lower = [&](int v) {            // first position with k[pos] >= v (numpy.searchsorted, side = "left")
        int l = 0, h = m;
        while (l < h) {
            const int mid = (l + h) >> 1;
            if (k[mid] < v) l = mid + 1; else h = mid;
        }
        return l;
    };
    const int a = lower(lo), bb = lower(hi);
    const int first = max(a - margin, 0), last = min(bb + margin + 2, m);
    const int cnt = last - first;
    CubicJob j;
    j.first = 1 + first;
    j.idx = cnt - 1;
    j.status = totals[2 * b + 1] ? 2 : 0;
    j.valid = cnt >= 4 && j.status == 0;
    jobs[b] = j;
    if (j.status) atomicOr(status, j.status);
}

// the emitted part of the tier-1 operator's window results
__global__ void k_stream_emit2(const double *__restrict__ rot_w, const double *__restrict__ base_w, int64_t w_stride, int64_t lo,
                               int64_t L, double *__restrict__ rot, int64_t rot_stride, double *__restrict__ base, int64_t base_stride)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    const int c = blockIdx.y;
    if (base) base[(int64_t)c * base_stride + i] = base_w[(int64_t)c * w_stride + lo + i];
    if (rot) rot[(int64_t)c * rot_stride + i] = rot_w[(int64_t)c * w_stride + lo + i];
}

// ---- the levels stream (itd_levels_stream_*): M+1 tier-1 stages chained block by block, ONE launch per step --------------
// Stage 0 is the linear stream on the caller's blocks, stage k >= 1 the same operator on the baselines stage k-1 emits.  At step
// t (push t, flush steps continue the count) stage k emits block t-1-k; the rows of block t-1-M leave: rows 0 .. M-1 = the
// rotations of stages 0 .. M-1 (stage k's waits M-k steps in its delay line), row M = stage M's rotation + baseline
// (ITD.py:418-426).  One workgroup per channel runs the stages in order, the window in LDS, the extraction is
// ITD_RES_FLAGS / ITD_RES_PREFIX / ITD_RES_PASSES of k_resident (itd_resident.hpp) without its stop rule and NaN branch: the
// single-level stream's plain rules, and a window holding a NaN sets status bit 2.
//
// The exactness certificate.  E_k(j) = "stage k's rotation and baseline of block j equal level k of the whole-signal
// decomposition of the concatenated blocks (the driver run to level M, ITD.py:384-432) bit for bit".  Locality of level k:
//   * a knot decision (ITD.py:44-59, 87-98, plateaus included: the predicate compares dx[i-1] and dx[i]) at sample i reads
//     samples i-1 .. i+1, so inside a window every decision at window samples 1 .. n-2 is the whole signal's, given the same
//     input there; the window's first / last sample is the window's end knot, which is the whole signal's only at the true
//     stream start / end (there the end rules, numpy.mean(x[:2]) / x[-2:] and baseline[n-1] = 0, ITD.py:96-112, coincide);
//   * the baseline on a segment [tau_k, tau_k+1) reads the knots tau_k-1 .. tau_k+2: positions (as differences), input
//     samples and knot values (ITD.py:100-117).
// So block j (window samples [lo, hi)) is exact at stage k when
//   (a) the window's input is the whole signal's level-k input: k = 0, or E_k-1 holds for every block in the window;
//   (b) every window sample is finite: a NaN makes the reference's detect_peaks take its NaN branch for the whole array and
//       the driver feeds +inf to the next level (ITD.py:46-51, 428-432), and under that branch inf - inf counts as +inf, so
//       a window with an infinity may decide differently from a whole signal that holds a NaN elsewhere;
//   (c) left: the window starts at the stream start, or at least 2 knots lie in window samples 1 .. lo (then tau_k-1 and
//       tau_k of every emitted sample are decided locally);
//   (d) right: the block is the stream's last (its window then ends at the stream end), or at least 2 knots lie in window
//       samples hi .. n-2.  (A window that reaches the last block before the flush cannot know that it is the end.)
// E_k(j) = (a) and (b) and (c) and (d); the block's flag is E_M(j), which implies E_k(j) for every k through (a).  The rule is
// sound and conservative (a segment that needs fewer knots is not looked at).  The flag speaks of the driver run to the end
// ("Out of time"): where the whole signal stops naturally before level M, it has fewer rows.
__host__ __device__ inline bool levels_exact(bool inputs_exact, bool finite, bool at_start, bool at_end, int knots_left, int knots_right)
{
    return inputs_exact && finite && (at_start || knots_left >= 2) && (at_end || knots_right >= 2);
}

struct LevelsArgs {
    const double *in;              // this push's block of every channel (in_stride apart); nullptr on a flush step
    int64_t in_stride;
    double *ring;                  // [C][M+1][5 L]: stage k's mirrored ring (the layout k_stream_store writes)
    double *delay;                 // [C][M (M+1) / 2][L]: stage k < M's rotations, M-k blocks deep
    uint8_t *eflags;               // [C][M+1][4]: E_k of stage k's blocks, by block % 4
    double *rows;                  // the emitted block: rows[c][r][s] at c chan_stride + r row_stride + s (nullptr: none)
    int64_t row_stride, chan_stride;
    uint8_t *exact;                // [C], E_M of the emitted block (optional)
    int32_t *status;               // |= 2: a window held a NaN
    int64_t t, P;                  // the step; P = the blocks in all once flushing began, -1 before
    int L, M, cw;
};

template <int TH, int SPT>
__global__ __launch_bounds__(TH) void k_stream_levels(LevelsArgs a)   // (a workgroup per channel: registers, not occupancy)
{
    static_assert(TH % 64 == 0 && TH * SPT <= kResidentMax, "geometry");
    constexpr int W = TH / 64;
    constexpr int WPL = (TH * SPT / 64 + 63) / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int ch = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = a.L, M = a.M, cw = a.cw;
    // the LDS layout of the largest window (three blocks), as k_resident lays it out
    const int npad = resident_pad(3 * L), cap = resident_cap(cw);
    double *xs = reinterpret_cast<double *>(lds_raw);
    double *Xk = xs + npad;
    double *Bk = Xk + cap;
    double *Sk = Bk + cap;
    double *ends = Sk + cap;
    unsigned long long *bal = reinterpret_cast<unsigned long long *>(ends + 4);
    int *pre = reinterpret_cast<int *>(bal + (npad >> 6));
    int *ctl = pre + (npad >> 6);                  // [1]: the window holds a NaN, [2]: a non-finite sample
    unsigned short *ek = reinterpret_cast<unsigned short *>(ctl + 8);

    const int64_t ring_len = 5 * (int64_t)L;
    double *const ring_c = a.ring + (int64_t)ch * (M + 1) * ring_len;
    double *const delay_c = a.delay + (int64_t)ch * ((int64_t)M * (M + 1) / 2) * L;
    uint8_t *const ef = a.eflags + (int64_t)ch * (M + 1) * 4;
    const int64_t jo = a.t - 1 - M;                                       // the block whose rows leave at this step
    double *const rows_c = (a.rows && jo >= 0 && (a.P < 0 || jo <= a.P - 1)) ? a.rows + (int64_t)ch * a.chan_stride : nullptr;
    int lo_prev = 0;                                                      // the previous stage's emitted block in xs

    for (int k = 0; k <= M; ++k) {
        double *const ring = ring_c + k * ring_len;
        if (tid == 0) ctl[1] = ctl[2] = 0;
        // the block that arrives at stage k: the caller's (stage 0, push), or what stage k-1 emitted just now (still in xs)
        const int64_t arr = a.t - k;
        const bool arrives = k == 0 ? a.in != nullptr : (arr >= 0 && (a.P < 0 || arr <= a.P - 1));
        if (arrives) {
            const int slot = (int)(arr % 3);
            for (int s = tid; s < L; s += TH) {
                const double v = k == 0 ? a.in[(int64_t)ch * a.in_stride + s] : xs[lo_prev + s];
                ring[(int64_t)slot * L + s] = v;
                if (slot < 2) ring[(int64_t)(slot + 3) * L + s] = v;
            }
        }
        __syncthreads();                                                  // (the ring's stores are the workgroup's own)
        const int64_t j = a.t - 1 - k;                                    // the block stage k emits
        const bool active = j >= 0 && (a.P < 0 || j <= a.P - 1);
        const int D = M - k;
        double *const dl = delay_c + ((int64_t)k * M - (int64_t)k * (k - 1) / 2) * L;
        if (!active) {                                                    // drained: its delayed rotation still leaves
            if (k < M && rows_c)
                for (int s = tid; s < L; s += TH) rows_c[(int64_t)k * a.row_stride + s] = dl[(jo % D) * L + s];
            continue;
        }
        const bool succ = a.P < 0 || j + 1 <= a.P - 1;
        const int64_t f = j > 0 ? j - 1 : 0;                              // the window: blocks f .. (succ ? j+1 : j)
        const int n = (int)(j - f + (succ ? 2 : 1)) * L, lo = (int)(j - f) * L, hi = lo + L;
        const int np2 = resident_pad(n), Q = np2 >> 6;
        const double *win = ring + (f % 3) * L;
        double xr[SPT];
        bool nonfinite = false;
#pragma unroll
        for (int jj = 0; jj < SPT; ++jj) {
            const int q = wave + W * jj, i = q * 64 + lane;
            xr[jj] = 0.0;
            if (q < Q) {
                if (i < n) xr[jj] = win[i];
                xs[i] = xr[jj];                                           // the padding is 0 (ITD_RES_FLAGS reads it)
                nonfinite = nonfinite || !(xr[jj] - xr[jj] == 0.0);
            }
        }
        if (__any(nonfinite) && lane == 0) ctl[2] = 1;
        __syncthreads();
        int *cs = ctl;
        ITD_RES_FLAGS;
        __syncthreads();
        ITD_RES_PREFIX;
        const int m = total;
        ITD_RES_PASSES((void)0);
        // the emitted block: rotation into the delay line (its slot's previous block leaves as row k) or row M
#pragma unroll
        for (int jj = 0; jj < SPT; ++jj) {
            const int q = wave + W * jj, i = q * 64 + lane;
            if (q < Q && i >= lo && i < hi) {
                const int s = i - lo;
                const double b = xs[i], r = xr[jj] - b;
                if (k < M) {
                    double *d = dl + (j % D) * L + s;
                    if (rows_c) rows_c[(int64_t)k * a.row_stride + s] = *d;
                    *d = r;
                } else if (rows_c) {
                    rows_c[(int64_t)M * a.row_stride + s] = r + b;
                }
            }
        }
        if (tid == 0) {
            auto at_or_before = [&](int i) { return pre[i >> 6] + __popcll(bal[i >> 6] & ((2ull << (i & 63)) - 1ull)); };
            const int kl = lo > 0 ? at_or_before(lo) : 0, kr = m - at_or_before(hi - 1);
            bool in_ok = true;
            if (k > 0)
                for (int64_t b = f; b < f + n / L; ++b) in_ok = in_ok && ef[(k - 1) * 4 + b % 4] != 0;
            const bool e = levels_exact(in_ok, ctl[2] == 0, f == 0, !succ, kl, kr);
            ef[k * 4 + j % 4] = e ? 1 : 0;
            if (ctl[1]) atomicOr(a.status, 2);
            if (k == M && rows_c && a.exact) a.exact[ch] = e ? 1 : 0;
        }
        lo_prev = lo;
    }
}

// The launch-sequence form of one step (blocks above 2730 samples, or forced: itd_levels_stream_set_sequence): per stage, every
// channel's window goes through extract_batch (the level-0 pair k_detect / k_extract, bit-identical to the resident arithmetic)
// into rw / bw, then this kernel does what k_stream_levels does behind its extraction: the emitted block into the delay line or
// row M, its baseline into stage k+1's ring, and the same exactness rule (levels_exact) over the same knot predicate.  On a flush
// step where stage k has drained it only lets the delayed rotation leave.  One workgroup per channel.
struct LevelsRoute {
    LevelsArgs a;
    const double *rw, *bw;         // stage k's window results, [C][3 L]
    int k;
};

template <int TH>
__global__ __launch_bounds__(TH) void k_levels_route(LevelsRoute r)
{
    __shared__ int cnt[3];         // knots in window samples 1 .. lo, in hi .. n-2; non-finite samples
    const LevelsArgs &a = r.a;
    const int ch = blockIdx.x, tid = threadIdx.x, k = r.k, M = a.M;
    const int64_t L = a.L, ring_len = 5 * L;
    double *const ring_c = a.ring + (int64_t)ch * (M + 1) * ring_len;
    double *const dl = a.delay + ((int64_t)ch * ((int64_t)M * (M + 1) / 2) + (int64_t)k * M - (int64_t)k * (k - 1) / 2) * L;
    uint8_t *const ef = a.eflags + (int64_t)ch * (M + 1) * 4;
    const int64_t jo = a.t - 1 - M;
    double *const rows_c = (a.rows && jo >= 0 && (a.P < 0 || jo <= a.P - 1)) ? a.rows + (int64_t)ch * a.chan_stride : nullptr;
    const int64_t j = a.t - 1 - k;
    const bool active = j >= 0 && (a.P < 0 || j <= a.P - 1);
    const int D = M - k;
    if (!active) {
        if (k < M && rows_c)
            for (int64_t s = tid; s < L; s += TH) rows_c[(int64_t)k * a.row_stride + s] = dl[(jo % D) * L + s];
        return;
    }
    const bool succ = a.P < 0 || j + 1 <= a.P - 1;
    const int64_t f = j > 0 ? j - 1 : 0;
    const int64_t n = (j - f + (succ ? 2 : 1)) * L, lo = (j - f) * L, hi = lo + L;
    if (tid < 3) cnt[tid] = 0;
    __syncthreads();
    const double *win = ring_c + (int64_t)k * ring_len + (f % 3) * L;
    int c0 = 0, c1 = 0, c2 = 0;
#pragma unroll 4
    for (int64_t i = tid; i < n; i += TH) {     // (one workgroup walks the whole window: keep loads in flight)
        const double c = win[i];
        if (!(c - c == 0.0)) ++c2;
        if (i >= 1 && i <= n - 2) {
            const double d0 = c - win[i - 1], d1 = win[i + 1] - c;     // ITD_RES_FLAGS's predicate
            if ((d1 > 0.0 && d0 <= 0.0) || (d1 < 0.0 && d0 >= 0.0)) {
                if (i <= lo) ++c0;
                if (i >= hi) ++c1;
            }
        }
    }
    if (c0) atomicAdd(&cnt[0], c0);
    if (c1) atomicAdd(&cnt[1], c1);
    if (c2) atomicAdd(&cnt[2], c2);
    const double *rw = r.rw + (int64_t)ch * 3 * L + lo, *bw = r.bw + (int64_t)ch * 3 * L + lo;
    double *const next = k < M ? ring_c + (int64_t)(k + 1) * ring_len : nullptr;
    const int slot = (int)(j % 3);
    for (int64_t s = tid; s < L; s += TH) {
        const double b = bw[s], rt = rw[s];
        if (k < M) {
            double *d = dl + (j % D) * L + s;
            if (rows_c) rows_c[(int64_t)k * a.row_stride + s] = *d;
            *d = rt;
            next[(int64_t)slot * L + s] = b;
            if (slot < 2) next[(int64_t)(slot + 3) * L + s] = b;
        } else if (rows_c) {
            rows_c[(int64_t)M * a.row_stride + s] = rt + b;
        }
    }
    __syncthreads();
    if (tid == 0) {
        bool in_ok = true;
        if (k > 0)
            for (int64_t b = f; b < f + n / L; ++b) in_ok = in_ok && ef[(k - 1) * 4 + b % 4] != 0;
        const bool e = levels_exact(in_ok, cnt[2] == 0, f == 0, !succ, cnt[0], cnt[1]);
        ef[k * 4 + j % 4] = e ? 1 : 0;
        if (k == M && rows_c && a.exact) a.exact[ch] = e ? 1 : 0;
    }
}

}  // namespace itd
