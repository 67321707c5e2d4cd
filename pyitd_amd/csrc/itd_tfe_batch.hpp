// itd_tfe_batch.hpp — instantaneous amplitude, phase and frequency of MANY rows in one asynchronous call (the batched form of
// itd_tfe.hpp: the same definitions, the same expressions, bit-identical results on NaN-free rows).
//
// The single-row operator numbers a row's half waves globally: an ordered compaction of the zero crossings (whose count the
// host reads to size the amplitude table), a memset and one atomic max per (step, half wave).  Here nothing is numbered.  A half
// wave either begins and ends inside one 512-sample tile — its amplitude is then a segmented maximum of that tile alone — or it
// is the first or the last half wave of a tile, and those two amplitudes follow from three numbers per tile:
//     c      crossings whose index lies in the tile
//     head   max |x| of the tile's samples up to and including its first crossing index (the whole tile if c == 0)
//     tail   max |x| of the samples behind its last crossing index (0 if there are none or c == 0; 0 is neutral for a maximum
//            of magnitudes)
// by a scan along the row (in: what reaches the tile's first half wave from the left, out: what reaches its last one from the
// right):
//     in[0] = 0,       in[t]  = c[t-1] > 0 ? tail[t-1] : max(in[t-1], head[t-1])
//     out[last] = 0,   out[t] = c[t+1] > 0 ? head[t+1] : max(head[t+1], out[t+1])
//     Ahead[t] = max(in[t], head[t], c[t] == 0 ? out[t] : 0)        the tile's first half wave
//     Atail[t] = max(tail[t], out[t])                                its last one (c[t] > 0)
// Three launches per chunk of rows, grid = (tiles, rows) with one wavefront per tile for the two passes over the samples:
//     k_inst_records   reads the row, writes one record per tile
//     k_inst_carry     the scan over a row's records, one workgroup per row; also the row's crossing total / NaN flag (info)
//     k_inst_apply     reads the row again: flags and in-tile segmented maxima anew, the first / last half wave's amplitude from
//                      Ahead / Atail, the amplitude of sample s + 512 (lane 63's successor) from Ahead[t+1]; phase and frequency
//                      exactly as k_tfe_phase writes them; streamed stores, each element rounded once where the output is float32
// No workgroup waits for another, no atomics on global memory, no count on the host.  Nothing outside the first n samples of a
// row is read.  Traffic for float64 in and out: 8 + 8 B read and 24 B written per sample, and per tile 24 B of record and 16 B of
// Ahead / Atail written and read once or twice (about 0.2 B per sample).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itd_tfe.hpp"

#pragma clang fp contract(off)

namespace itd {

struct InstRec {
    int32_t c;          // crossings whose index lies in the tile
    int32_t nan;        // the tile holds a NaN
    double head, tail;
};
static_assert(sizeof(InstRec) == 24, "InstRec layout");

constexpr int kInstSteps = kTfeTile / 64;
constexpr int kInstCarryThreads = 256;                                   // long rows (more than kInstCarrySmall records)
constexpr int kInstCarryPer = 8;                                         // records per thread and pass
constexpr int kInstCarryChunk = kInstCarryThreads * kInstCarryPer;       // K = 2048 records (2^20 samples) per pass
constexpr int kInstCarrySmall = 64 * kInstCarryPer;                      // up to here one wavefront takes the row in one pass

// |x| as an unsigned integer (non-negative doubles order like their bit patterns); a NaN does not count, as in k_tfe_amplitude
__device__ __forceinline__ unsigned long long inst_mag(double x, bool in)
{
    const double a = __builtin_fabs(x);
    return (in && a == a) ? __builtin_bit_cast(unsigned long long, a) : 0ull;
}
__device__ __forceinline__ unsigned long long inst_umax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long inst_wave_max(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = inst_umax(v, __shfl_xor(v, d));
    return v;
}

// The tile's samples (lane + 64 g, zero behind the row's end), every sample's successor, the crossing flags of the tile and
// before[g] = the crossings of the tile in front of the lane's sample of step g.  ext0 = x[s + 512] or 0.  Returns c.
template <typename Tin>
__device__ __forceinline__ int inst_load_tile(const Tin *__restrict__ x, int64_t n, int64_t s, int lane, double ext0,
                                              double (&xr)[kInstSteps], double (&xn)[kInstSteps],
                                              unsigned long long (&cm)[kInstSteps], int (&before)[kInstSteps])
{
#pragma unroll
    for (int g = 0; g < kInstSteps; ++g) {
        const int64_t j = s + g * 64 + lane;
        xr[g] = j < n ? (double)x[j] : 0.0;
    }
    int c = 0;
#pragma unroll
    for (int g = 0; g < kInstSteps; ++g) {
        const int64_t j = s + g * 64 + lane;
        const double nxt = __shfl_down(xr[g], 1);
        const double first_next = g + 1 < kInstSteps ? __shfl(xr[g + 1 < kInstSteps ? g + 1 : g], 0) : ext0;
        xn[g] = lane == 63 ? first_next : nxt;
        cm[g] = __ballot(tfe_crossing(j, n, xr[g], xn[g]));       // (j <= n - 2: xn is a sample of the row)
        before[g] = c + __popcll(cm[g] & ((1ull << lane) - 1ull));
        c += __popcll(cm[g]);
    }
    return c;
}

template <typename Tin>
__global__ __launch_bounds__(64) void k_inst_records(const Tin *__restrict__ rows, int64_t row_stride, int64_t n, int64_t tiles,
                                                     InstRec *__restrict__ rec)
{
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x, s = t * kTfeTile;
    const Tin *x = rows + (int64_t)blockIdx.y * row_stride;
    const double ext0 = s + kTfeTile < n ? (double)x[s + kTfeTile] : 0.0;
    double xr[kInstSteps], xn[kInstSteps];
    unsigned long long cm[kInstSteps];
    int before[kInstSteps];
    const int c = inst_load_tile<Tin>(x, n, s, lane, ext0, xr, xn, cm, before);
    // positions (in the tile) of the first and the last crossing index; none: the head is the whole tile, the tail empty
    int fpos = kTfeTile - 1, lpos = kTfeTile - 1;
    if (c > 0) {
        bool found = false;
#pragma unroll
        for (int g = 0; g < kInstSteps; ++g) {
            if (cm[g]) {
                if (!found) fpos = g * 64 + __builtin_ctzll(cm[g]);
                found = true;
                lpos = g * 64 + 63 - __builtin_clzll(cm[g]);
            }
        }
    }
    unsigned long long hv = 0ull, tv = 0ull;
    bool nan = false;
#pragma unroll
    for (int g = 0; g < kInstSteps; ++g) {
        const int p = g * 64 + lane;
        const bool in = s + p < n;
        const unsigned long long v = inst_mag(xr[g], in);
        nan |= in && xr[g] != xr[g];
        if (p <= fpos) hv = inst_umax(hv, v);
        if (p > lpos) tv = inst_umax(tv, v);
    }
    hv = inst_wave_max(hv);
    tv = inst_wave_max(tv);
    const bool any_nan = __ballot(nan) != 0ull;
    if (lane == 0) {
        InstRec r;
        r.c = c;
        r.nan = any_nan ? 1 : 0;
        r.head = __builtin_bit_cast(double, hv);
        r.tail = __builtin_bit_cast(double, tv);
        rec[(int64_t)blockIdx.y * tiles + t] = r;
    }
}

// An element of the scan: the map s -> reset ? m : max(s, m) on magnitudes (as bit patterns).  then(f, g) is "f, then g";
// the operator is associative and {0, 0} its identity.
struct InstMap {
    int reset;
    unsigned long long m;
};
__device__ __forceinline__ InstMap inst_then(InstMap f, InstMap g)
{
    InstMap r;
    r.reset = f.reset | g.reset;
    r.m = g.reset ? g.m : inst_umax(f.m, g.m);
    return r;
}
__device__ __forceinline__ unsigned long long inst_apply_map(InstMap f, unsigned long long s) { return f.reset ? f.m : inst_umax(s, f.m); }

// One workgroup per row.  Position p counts the records in scan order: record p in the forward pass (which leaves max(in, head)
// in Ahead), record tiles - 1 - p in the backward pass (which completes Ahead and writes Atail).  A pass takes NT * kInstCarryPer
// positions at a time — every thread kInstCarryPer consecutive ones, an exclusive scan of the threads' maps across the workgroup —
// and carries its running value from one such chunk to the next.
template <int NT>
__global__ __launch_bounds__(NT) void k_inst_carry(const InstRec *__restrict__ rec, int64_t tiles, double *__restrict__ Ahead,
                                                   double *__restrict__ Atail, int32_t *__restrict__ info)
{
    constexpr int NW = NT / 64, R = kInstCarryPer;
    __shared__ InstMap wave_tot[NW];
    __shared__ int sh_cnt, sh_nan;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x;
    rec += row * tiles;
    Ahead += row * tiles;
    Atail += row * tiles;
    if (tid == 0) { sh_cnt = 0; sh_nan = 0; }
    int cnt = 0, nan = 0;
    for (int dir = 0; dir < 2; ++dir) {
        unsigned long long run = 0ull;                  // in[] / out[] of the chunk's first position
        for (int64_t base = 0; base < tiles; base += (int64_t)NT * R) {
            InstRec r[R];
            InstMap f[R];
            InstMap mine = {0, 0ull};
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int64_t p = base + (int64_t)tid * R + k;
                const bool in = p < tiles;
                const int64_t t = dir ? tiles - 1 - p : p;
                if (in) r[k] = rec[t];
                else { r[k].c = 0; r[k].nan = 0; r[k].head = 0.0; r[k].tail = 0.0; }
                f[k].reset = r[k].c > 0 ? 1 : 0;
                // forward: a tile with crossings hands on its tail, one without joins its maximum (head); backward: the head either way
                f[k].m = __builtin_bit_cast(unsigned long long, (dir == 0 && r[k].c > 0) ? r[k].tail : r[k].head);
                if (!in) { f[k].reset = 0; f[k].m = 0ull; }
                mine = inst_then(mine, f[k]);
                if (dir == 0) { cnt += r[k].c; nan |= r[k].nan; }
            }
            // inclusive scan of the threads' maps along the wavefront, the wavefronts' totals through LDS
            InstMap inc = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                InstMap o;
                o.reset = __shfl_up(inc.reset, d);
                o.m = __shfl_up(inc.m, d);
                if (lane >= d) inc = inst_then(o, inc);
            }
            __syncthreads();                            // (the previous chunk's reads of wave_tot are done)
            if (lane == 63) wave_tot[wave] = inc;
            __syncthreads();
            InstMap excl;
            excl.reset = __shfl_up(inc.reset, 1);
            excl.m = __shfl_up(inc.m, 1);
            if (lane == 0) { excl.reset = 0; excl.m = 0ull; }
            InstMap front = {0, 0ull}, all = {0, 0ull};
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                if (w < wave) front = inst_then(front, wave_tot[w]);
                all = inst_then(all, wave_tot[w]);
            }
            unsigned long long v = inst_apply_map(inst_then(front, excl), run);   // in[] / out[] of the thread's first position
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int64_t p = base + (int64_t)tid * R + k;
                if (p < tiles) {
                    const int64_t t = dir ? tiles - 1 - p : p;
                    const unsigned long long head = __builtin_bit_cast(unsigned long long, r[k].head);
                    if (dir == 0) {
                        Ahead[t] = __builtin_bit_cast(double, inst_umax(v, head));
                    } else {
                        const unsigned long long tail = __builtin_bit_cast(unsigned long long, r[k].tail);
                        if (r[k].c == 0) {
                            const unsigned long long a = __builtin_bit_cast(unsigned long long, Ahead[t]);
                            Ahead[t] = __builtin_bit_cast(double, inst_umax(a, v));
                        }
                        Atail[t] = __builtin_bit_cast(double, inst_umax(tail, v));
                    }
                }
                v = inst_apply_map(f[k], v);
            }
            run = inst_apply_map(all, run);
        }
        // the backward pass reads the Ahead the forward pass wrote (other threads of this workgroup)
        __threadfence_block();
        __syncthreads();
    }
    if (info) {
        if (cnt) atomicAdd(&sh_cnt, cnt);
        if (nan) atomicOr(&sh_nan, 1);
        __syncthreads();
        if (tid == 0) info[row] = sh_nan ? -1 - sh_cnt : sh_cnt;
    }
}

template <typename Tout>
__device__ __forceinline__ void inst_store(Tout *__restrict__ out, int64_t j, double v)
{
    __builtin_nontemporal_store((Tout)v, &out[j]);
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(64) void k_inst_apply(const Tin *__restrict__ rows, int64_t row_stride, int64_t n, int64_t tiles,
                                                   const double *__restrict__ Ahead, const double *__restrict__ Atail,
                                                   Tout *__restrict__ amp_out, Tout *__restrict__ phase_out,
                                                   Tout *__restrict__ freq_out, int64_t out_stride)
{
    const double pi = 3.14159265358979323846;
    __shared__ unsigned long long seg[kTfeTile + 1];   // max |x| of the tile's half waves, by their number inside the tile
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x, s = t * kTfeTile;
    const Tin *x = rows + (int64_t)blockIdx.y * row_stride;
    const int64_t o = (int64_t)blockIdx.y * out_stride;
    const int64_t rt = (int64_t)blockIdx.y * tiles + t;
    const bool has_ext = s + kTfeTile < n;              // sample s + 512 exists: the tile is not the row's last
    const double ext = (lane < 2 && s + kTfeTile + lane < n) ? (double)x[s + kTfeTile + lane] : 0.0;
    const double ext0 = __shfl(ext, 0), ext1 = __shfl(ext, 1);
    const double A_head = Ahead[rt], A_tail = Atail[rt];
    const double A_ext = has_ext ? Ahead[rt + 1] : 0.0;  // the half wave of sample s + 512 is the next tile's first
    double xr[kInstSteps], xn[kInstSteps];
    unsigned long long cm[kInstSteps];
    int before[kInstSteps];
    const int c = inst_load_tile<Tin>(x, n, s, lane, ext0, xr, xn, cm, before);
    if (c >= 2) {
        // half waves 1 .. c-1 begin and end inside the tile: their maxima by one LDS atomic per sample (a maximum does not depend
        // on the order; lanes of one half wave meet on one word).  (A segmented scan over the lanes of every step — k_tfe_amplitude's,
        // 18 dependent cross-lane moves per step — cost 0.24 ms of the call's 1.53 ms on 9 x 2^24 samples.)
        for (int i = 1 + lane; i < c; i += 64) seg[i] = 0ull;
        __syncthreads();
#pragma unroll
        for (int g = 0; g < kInstSteps; ++g) {
            const int64_t j = s + g * 64 + lane;
            if (before[g] > 0 && before[g] < c && j < n) atomicMax(&seg[before[g]], inst_mag(xr[g], true));
        }
        __syncthreads();
    }
    auto phase_in = [&](double xi, double slope, double Aa) {
        if (!(Aa > 0.0)) return 0.0;                    // an all-zero half wave
        const double r = xi / Aa;
        const double as = asin(r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r));
        if (xi >= 0.0) return slope >= 0.0 ? as : pi - as;
        return slope < 0.0 ? pi - as : 2.0 * pi + as;
    };
    // the row's last sample takes the backward difference, for its slope and for its frequency
    const bool last_tile = !has_ext;
    const int lp = (int)(n - 1 - s);                    // its position in this tile (last_tile)
    double A[kInstSteps], ph[kInstSteps];
#pragma unroll
    for (int g = 0; g < kInstSteps; ++g) {
        const int hw = before[g];
        A[g] = hw == 0 ? A_head : (hw == c ? A_tail : __builtin_bit_cast(double, seg[c >= 2 ? hw : 0]));
        double slope = xn[g] - xr[g];
        if (last_tile) {
            const double up = __shfl_up(xr[g], 1);
            const double prev_last = g > 0 ? __shfl(xr[g > 0 ? g - 1 : 0], 63) : 0.0;   // (n >= 3: sample n-1 is never a row's first)
            const double xprev = lane == 0 ? prev_last : up;
            if (g * 64 + lane == lp) slope = xr[g] - xprev;       // (lp == 0: the tile's lone sample, written below)
        }
        ph[g] = phase_in(xr[g], slope, A[g]);
    }
    double ph_ext = 0.0;
    if (has_ext) {
        const double x_last = __shfl(xr[kInstSteps - 1], 63);
        ph_ext = phase_in(ext0, s + kTfeTile + 1 < n ? ext1 - ext0 : ext0 - x_last, A_ext);
    }
    if (last_tile && lp == 0) {
        // the lone sample of the row's last tile: its predecessor is the tile before's last sample
        const double xprev = (double)x[s - 1];
        if (lane == 0) ph[0] = phase_in(xr[0], xr[0] - xprev, A[0]);
    }
#pragma unroll
    for (int g = 0; g < kInstSteps; ++g) {
        const int64_t j = s + g * 64 + lane;
        const bool in = j < n;
        if (in && amp_out) inst_store<Tout>(amp_out + o, j, A[g]);
        if (in && phase_out) inst_store<Tout>(phase_out + o, j, ph[g]);
        if (freq_out) {
            const double nxt = __shfl_down(ph[g], 1);
            const double first_next = g + 1 < kInstSteps ? __shfl(ph[g + 1 < kInstSteps ? g + 1 : g], 0) : ph_ext;
            double dp = (lane == 63 ? first_next : nxt) - ph[g];
            bool write = in;
            if (last_tile) {
                const double up = __shfl_up(ph[g], 1);
                const double prev_last = g > 0 ? __shfl(ph[g > 0 ? g - 1 : 0], 63) : 0.0;
                if (g * 64 + lane == lp) {
                    dp = ph[g] - (lane == 0 ? prev_last : up);
                    write = lp > 0;                     // the lone sample's frequency comes from the tile before (below)
                }
            }
            if (dp < 0.0) dp += 2.0 * pi;               // the phase wraps once per wave
            if (write) inst_store<Tout>(freq_out + o, j, dp / (2.0 * pi));
        }
    }
    if (freq_out && has_ext && s + kTfeTile == n - 1) {
        // sample s + 512 is the row's last: its backward difference is this tile's last forward one
        const double p_last = __shfl(ph[kInstSteps - 1], 63);
        double dp = ph_ext - p_last;
        if (dp < 0.0) dp += 2.0 * pi;
        if (lane == 0) inst_store<Tout>(freq_out + o, n - 1, dp / (2.0 * pi));
    }
}

}  // namespace itd
