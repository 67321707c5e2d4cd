// itd_wave_bounds.hpp — device side of the wave filter's bounds from histogram quantiles (itd_wave_bounds_batch and
// itd_bounds_stream_* in include/pyitd_hip.h): the step between itd_wave_hist_batch_* / the histogram stream
// and itd_wave_filter_batch_* / the wave-filter stream, on the device.
//
// A row has a histogram h[T][na][nl] of non-negative int32 cells, a range of time bins [t0, t1), its edges ae[0..na], le[0..nl] and
// eight float64 parameters q = (aq_lo, aq_hi, lq_lo, lq_hi, as_lo, as_hi, ls_lo, ls_hi).  In int64: ma[i] = sum over t and j,
// ml[j] = sum over t and i, N = sum ma = sum ml.  One axis with marginal m[0..B), edges e[0..B], inclusive prefix sums cum:
//   N == 0      iL = 0, iU = B - 1
//   otherwise   tau_lo = q_lo * (double)N, tau_hi = q_hi * (double)N, one IEEE multiply each;
//               iL = the smallest i with (double)cum[i] > tau_lo; none (q_lo = 1, or a NaN): the smallest i with cum[i] == N
//               iU = max(iL, the smallest i with (double)cum[i] >= tau_hi; none (q_hi above 1, or a NaN): B - 1)
//   lo = e[iL] * s_lo, hi = e[iU + 1] * s_hi, one IEEE multiply each (a scale of 1.0: the edge's own bits)
// so 0 <= iL <= iU < B whatever the parameters hold.  Every decision is an integer sum and a comparison; the sums are integer adds
// (registers, LDS and global integer atomics), so the result is the same bits from run to run and in any batch position.
//
// Many rows (itd_wave_bounds_batch), per chunk of rows three launches:
//   k_wave_bounds_zero    the chunk's slots of the workspace, 128 int64 words per row (ma at 0, ml at 64)
//   k_wave_bounds_part    one workgroup per (row, part of the time range): a part is bounds_part_bins(cells) time bins, 64 KB of
//                         cells.  A thread owns a cell (cells >= 256: up to four of them; fewer cells: 256 / cells time bins abreast)
//                         and sums it over the part's time bins in an int64 register, coalesced over the cells; one LDS atomic per
//                         axis and owned cell, then at most na + nl global atomics per workgroup into the row's slot
//   k_wave_bounds_finish  one wavefront per row: lane i is bin i, a wavefront prefix sum, a ballot for the first lane over the
//                         threshold, lane 0 stores the four bounds and the total
// The stream (k_bounds_stream): one launch per push, one workgroup per row; the push's marginals as above into LDS, the window's
// running sums updated from the ring of per-push marginals (all int64), the finish by the workgroup's first wavefront.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace itd {

constexpr int kBoundsMaxBins = 64;                    // per axis
constexpr int kBoundsMaxCells = 1024;                 // na * nl
constexpr int kBoundsThreads = 256;
constexpr int kBoundsPartCells = 16384;               // the cells one workgroup of the time reduction reads
constexpr int kBoundsSlot = 2 * kBoundsMaxBins;       // int64 words of a row in the workspace and in LDS: ma at 0, ml at kBoundsMaxBins
constexpr int kBoundsStreamMaxCells = 8192;           // the histogram stream's limit on the cells of one push
constexpr int kBoundsStreamMaxWindow = 65536;

// time bins per part of the time reduction
inline int64_t bounds_part_bins(int cells) { return (kBoundsPartCells + cells - 1) / cells; }

// The marginals of the time bins [ta, tb) of one row's cells h[t][na][nl], added into m[kBoundsSlot] in LDS (zeroed by the caller
// in front of a barrier; complete behind the next one).  Called by all kBoundsThreads threads of the workgroup.
__device__ inline void bounds_marginals(const int32_t *__restrict__ h, int64_t ta, int64_t tb, int na, int nl, unsigned long long *m)
{
    const int cells = na * nl;
    const int K = cells >= kBoundsThreads ? 1 : kBoundsThreads / cells;   // time bins abreast
    for (int u = threadIdx.x; u < cells * K; u += kBoundsThreads) {
        const int c = u % cells, k = u / cells;
        long long acc = 0;
#pragma unroll 4
        for (int64_t t = ta + k; t < tb; t += K) acc += h[t * cells + c];
        if (acc != 0) {
            atomicAdd(&m[c / nl], (unsigned long long)acc);
            atomicAdd(&m[kBoundsMaxBins + c % nl], (unsigned long long)acc);
        }
    }
}

// One axis by one wavefront: lane i holds m[i] (0 for i >= B).  Returns the total in N and the two bounds (every lane the same).
__device__ inline void bounds_axis(long long m, int B, const double *__restrict__ e, double q_lo, double q_hi, double s_lo, double s_hi,
                                   double &lo, double &hi, long long &N)
{
    const int lane = threadIdx.x & 63;
    long long cum = m;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(cum, d);
        if (lane >= d) cum += o;
    }
    N = __shfl(cum, 63);
    int iL = 0, iU = B - 1;
    if (N != 0) {                                                         // (the same for the whole wavefront)
        const unsigned long long in = B >= 64 ? ~0ull : (1ull << B) - 1ull;
        const double c = (double)cum, tau_lo = q_lo * (double)N, tau_hi = q_hi * (double)N;
        const unsigned long long above = __ballot(c > tau_lo) & in;
        const unsigned long long full = __ballot(cum == N) & in;          // never empty: lane B - 1
        const unsigned long long reach = __ballot(c >= tau_hi) & in;
        iL = above ? __builtin_ctzll(above) : (full ? __builtin_ctzll(full) : B - 1);
        iU = reach ? __builtin_ctzll(reach) : B - 1;
        if (iU < iL) iU = iL;
    }
    lo = e[iL] * s_lo;
    hi = e[iU + 1] * s_hi;
}

// The finish of one row by one wavefront from its marginals m[kBoundsSlot] (LDS or global): the four bounds and the total
__device__ inline void bounds_finish(const unsigned long long *m, int na, int nl, const double *__restrict__ ae, const double *__restrict__ le,
                                     const double *__restrict__ q, double *__restrict__ bounds, int64_t *total)
{
    const int lane = threadIdx.x & 63;
    const long long ma = lane < na ? (long long)m[lane] : 0, ml = lane < nl ? (long long)m[kBoundsMaxBins + lane] : 0;
    double alo, ahi, llo, lhi;
    long long Na, Nl;
    bounds_axis(ma, na, ae, q[0], q[1], q[4], q[5], alo, ahi, Na);
    bounds_axis(ml, nl, le, q[2], q[3], q[6], q[7], llo, lhi, Nl);
    if (lane == 0) {
        bounds[0] = alo; bounds[1] = ahi; bounds[2] = llo; bounds[3] = lhi;
        if (total) *total = Na;
    }
}

__global__ __launch_bounds__(kBoundsThreads) void k_wave_bounds_zero(unsigned long long *__restrict__ ws, int64_t words)
{
    const int64_t i = (int64_t)blockIdx.x * kBoundsThreads + threadIdx.x;
    if (i < words) ws[i] = 0ull;
}

// grid (parts, rows): the part's time bins [t0 + part per, min(t1, + per)) of the row, into the row's slot of ws
__global__ __launch_bounds__(kBoundsThreads) void k_wave_bounds_part(const int32_t *__restrict__ hist, int64_t hist_stride, int64_t t0, int64_t t1,
                                                                     int64_t per, int na, int nl, unsigned long long *__restrict__ ws)
{
    __shared__ unsigned long long m[kBoundsSlot];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.y;
    if (tid < kBoundsSlot) m[tid] = 0ull;
    __syncthreads();
    const int64_t ta = t0 + (int64_t)blockIdx.x * per, tb = ta + per < t1 ? ta + per : t1;
    bounds_marginals(hist + row * hist_stride, ta, tb, na, nl, m);
    __syncthreads();
    if (tid < kBoundsSlot) {
        const unsigned long long v = m[tid];
        if (v) atomicAdd(&ws[row * kBoundsSlot + tid], v);
    }
}

// grid rows, one wavefront each
__global__ __launch_bounds__(64) void k_wave_bounds_finish(const unsigned long long *__restrict__ ws, int na, int nl, const double *__restrict__ ae,
                                                           int64_t ae_stride, const double *__restrict__ le, int64_t le_stride,
                                                           const double *__restrict__ q, int64_t q_stride, double *__restrict__ bounds,
                                                           int64_t bounds_stride, int64_t *__restrict__ total)
{
    const int64_t row = blockIdx.x;
    bounds_finish(ws + row * kBoundsSlot, na, nl, ae + row * ae_stride, le + row * le_stride, q + row * q_stride, bounds + row * bounds_stride,
                  total ? total + row : nullptr);
}

struct BoundsStreamArgs {
    const int32_t *hist;           // this push's slices of row r at r hist_stride: [C][na][nl]
    int64_t hist_stride;
    const double *ae, *le, *q;     // row r's at r times the stride (0: one set for every row)
    int64_t ae_stride, le_stride, q_stride;
    double *bounds;                // row r's four at r bounds_stride
    int64_t bounds_stride;
    int64_t *total;                // [rows] or nullptr
    unsigned long long *ring;      // [rows][W][na + nl]: the marginals of the pushes in the window
    unsigned long long *run;       // [rows][na + nl]: their sums
    int32_t C, na, nl, W;
    int32_t slot;                  // the ring slot this push goes to: p % W — where push p - W lies, the one it replaces
    int32_t held;                  // the pushes in the window in front of this one: min(p, W); 0: ring and run are not read
};

// grid rows: the push's marginals, the window's sums with the oldest push replaced, the bounds of the window
__global__ __launch_bounds__(kBoundsThreads) void k_bounds_stream(BoundsStreamArgs a)
{
    __shared__ unsigned long long m[kBoundsSlot];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    if (tid < kBoundsSlot) m[tid] = 0ull;
    __syncthreads();
    bounds_marginals(a.hist + row * a.hist_stride, 0, a.C, a.na, a.nl, m);
    __syncthreads();
    const int bins = a.na + a.nl;
    const bool mine = tid < a.na || (tid >= kBoundsMaxBins && tid < kBoundsMaxBins + a.nl);
    if (mine) {
        const int w = tid < kBoundsMaxBins ? tid : a.na + tid - kBoundsMaxBins;
        unsigned long long *const rp = a.run + row * bins + w;
        unsigned long long *const sp = a.ring + (row * a.W + a.slot) * bins + w;
        const unsigned long long fresh = m[tid];
        unsigned long long sum = fresh;
        if (a.held > 0) sum += *rp;
        if (a.held == a.W) sum -= *sp;
        *rp = sum;
        *sp = fresh;
        m[tid] = sum;
    }
    __syncthreads();
    if (tid < 64)
        bounds_finish(m, a.na, a.nl, a.ae + row * a.ae_stride, a.le + row * a.le_stride, a.q + row * a.q_stride, a.bounds + row * a.bounds_stride,
                      a.total ? a.total + row : nullptr);
}

}  // namespace itd
