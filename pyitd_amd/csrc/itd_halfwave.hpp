// itd_halfwave.hpp — the half-wave tile pipeline that the instantaneous step (itd_tfe_batch.hpp) and the single-wave analysis
// (itd_waves.hpp, itd_wave_hist.hpp) are built on: what a half wave is, how a 512-sample tile is loaded and cut, and the scan that joins the tiles.
//
// A proper rotation is cut into half waves at its zero crossings (Frei & Osorio 2007, single-wave analysis; README.md:13-21,
// 41-55).  Crossing index i (tfe_crossing): a strict sign change between x[i] and x[i+1], 1 <= i <= n-2; a crossing index is the
// last sample of its half wave.  One wavefront takes one tile, 64 samples per step.  A half wave either begins and ends inside
// one tile — then the tile alone knows it (tile_segment_max) — or it is the first or the last half wave of a tile, and what the
// tile holds of it (the head up to and including the first crossing index, the tail behind the last one: tile_crossing_span)
// goes into one record per tile.  A scan along the row's records, one workgroup per row, joins those (halfwave_carry): forward
// for what reaches a tile from the left, backward for what reaches it from the right.  Three launches per chunk of rows:
//     records   reads the row, writes one record per tile                       grid (tiles, rows), 64 threads
//     carry     halfwave_carry over a row's records; the row's info word        grid rows, 64 or kInstCarryThreads threads
//     consumer  reads the row again: the tile's own half waves anew, the first and last one from the carries
// No workgroup waits for another, no atomics on global memory (but the integer adds of itd_wave_hist.hpp's histogram), no count on
// the host, nothing outside the first n samples of a row read.  The operators differ in what a record, a carry and a consumer hold: a policy each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace itd {

constexpr int kTfeTile = 512;
constexpr int kInstSteps = kTfeTile / 64;
constexpr int kInstCarryThreads = 256;                                   // long rows (more than kInstCarrySmall records)
constexpr int kInstCarryPer = 8;                                         // records per thread and pass
constexpr int kInstCarryChunk = kInstCarryThreads * kInstCarryPer;       // K = 2048 records (2^20 samples) per pass
constexpr int kInstCarrySmall = 64 * kInstCarryPer;                      // up to here one wavefront takes the row in one pass
constexpr int32_t kWaveNone = INT32_MAX;                                 // the index of "no sample"

// crossing index i: a sign change between x[i] and x[i+1] (find_extrema's test, itd_fourier_decomposition.py:23-27), 1 <= i <= n-2
// exactly as k_detect's kZeroCross mode flags it (first and last sample never flag)
__device__ __forceinline__ bool tfe_crossing(int64_t i, int64_t n, double x0, double xp)
{
    return i >= 1 && i <= n - 2 && (((x0 > 0.0) && (0.0 > xp)) || ((x0 < 0.0) && (0.0 < xp)));
}

// |x| as an unsigned integer (non-negative doubles order like their bit patterns); a NaN does not count
__device__ __forceinline__ unsigned long long inst_mag(double x, bool in)
{
    const double a = __builtin_fabs(x);
    return (in && a == a) ? __builtin_bit_cast(unsigned long long, a) : 0ull;
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

// positions (in the tile) of the first and the last crossing index; none: the head is the whole tile, the tail empty
__device__ __forceinline__ void tile_crossing_span(const unsigned long long (&cm)[kInstSteps], int &fpos, int &lpos)
{
    fpos = lpos = kTfeTile - 1;
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

// Half waves 1 .. c-1 begin and end inside the tile: mag[r] = their max |x| (as a bit pattern) by one LDS atomic per sample (a
// maximum does not depend on the order; lanes of one half wave meet on one word), kPeak: peak[r] = the first index that attains
// it, by a second round among the samples that do.  mag / peak: LDS, by the half wave's number inside the tile.  The caller's
// barrier follows.  (A segmented scan over the lanes of every step, 18 dependent cross-lane moves per step, cost 0.24 ms of the
// instantaneous call's 1.53 ms on 9 x 2^24 samples.)
template <bool kPeak>
__device__ __forceinline__ void tile_segment_max(unsigned long long *mag, int32_t *peak, int lane, int64_t s, int64_t n, int c,
                                                 const double (&xr)[kInstSteps], const int (&before)[kInstSteps])
{
    if (c < 2) return;
    for (int i = 1 + lane; i < c; i += 64) {
        mag[i] = 0ull;
        if (kPeak) peak[i] = kWaveNone;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kInstSteps; ++g) {
        const int64_t j = s + g * 64 + lane;
        if (before[g] > 0 && before[g] < c && j < n) atomicMax(&mag[before[g]], inst_mag(xr[g], true));
    }
    if (kPeak) {
        __syncthreads();
#pragma unroll
        for (int g = 0; g < kInstSteps; ++g) {
            const int64_t j = s + g * 64 + lane;
            if (before[g] > 0 && before[g] < c && j < n && inst_mag(xr[g], true) == mag[before[g]]) atomicMin(&peak[before[g]], (int32_t)j);
        }
    }
}

// phase of a sample x in a half wave of amplitude A (the three cases: itd_tfe.hpp): rising or falling from the slope (the forward
// difference; the backward one at the row's last sample)
__device__ __forceinline__ double phase_in(double xi, double slope, double Aa)
{
    const double pi = 3.14159265358979323846;
    if (!(Aa > 0.0)) return 0.0;                    // an all-zero half wave
    const double r = xi / Aa;
    const double as = asin(r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r));
    if (xi >= 0.0) return slope >= 0.0 ? as : pi - as;
    return slope < 0.0 ? pi - as : 2.0 * pi + as;
}

template <typename Tout>
__device__ __forceinline__ void inst_store(Tout *__restrict__ out, int64_t j, double v)
{
    __builtin_nontemporal_store((Tout)v, &out[j]);
}

// The scan over one row's records, called by every thread of the row's workgroup (NT threads).  Position p counts the records in
// scan order: record p in the forward pass (dir 0), record tiles - 1 - p in the backward pass (dir 1).  A pass takes
// NT * kInstCarryPer positions at a time — every thread kInstCarryPer consecutive ones, an exclusive scan of the threads' maps
// across the workgroup — and carries its running state from one such chunk to the next.  The policy P supplies
//     Rec, Map, State                    a tile's record; an element of the scan (a map on states); what a position receives
//     ident(), then(f, g), up(f, d)      the monoid of maps ("f, then g") and a map taken from the lane d below
//     apply(f, s)                        the state behind a map
//     load(t)                            record t of the row
//     map(dir, r)                        the map of a record in a pass (it may also fold what the row reports)
//     start(dir)                         the state in front of the pass's first position
//     emit(dir, t, r, v)                 what record t's position writes, given the state v that reaches it
//     pass_end(dir, run)                 the state behind the pass's last position
//     report(tid)                        the row's count and info, behind a barrier after both passes
template <int NT, typename P>
__device__ __forceinline__ void halfwave_carry(P &pol, int64_t tiles)
{
    using Rec = typename P::Rec;
    using Map = typename P::Map;
    using State = typename P::State;
    constexpr int NW = NT / 64, R = kInstCarryPer;
    __shared__ Map wave_tot[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int dir = 0; dir < 2; ++dir) {
        State run = pol.start(dir);                     // what reaches the chunk's first position
        for (int64_t base = 0; base < tiles; base += (int64_t)NT * R) {
            Rec r[R];
            Map f[R];
            Map mine = P::ident();
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int64_t p = base + (int64_t)tid * R + k;
                // (load and map under one branch: taking every record's map unconditionally and blanking it afterwards
                // costs 20 VGPRs in the instantaneous carry, 128 -> 148, a wave per SIMD)
                f[k] = P::ident();
                if (p < tiles) {
                    r[k] = pol.load(dir ? tiles - 1 - p : p);
                    f[k] = pol.map(dir, r[k]);
                } else {
                    r[k] = Rec{};
                }
                mine = P::then(mine, f[k]);
            }
            // inclusive scan of the threads' maps along the wavefront, the wavefronts' totals through LDS
            Map inc = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const Map o = P::up(inc, d);
                if (lane >= d) inc = P::then(o, inc);
            }
            __syncthreads();                            // (the previous chunk's reads of wave_tot are done)
            if (lane == 63) wave_tot[wave] = inc;
            __syncthreads();
            Map excl = P::up(inc, 1);
            if (lane == 0) excl = P::ident();
            Map front = P::ident(), all = P::ident();
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                if (w < wave) front = P::then(front, wave_tot[w]);
                all = P::then(all, wave_tot[w]);
            }
            State v = P::apply(P::then(front, excl), run);      // what reaches the thread's first position
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int64_t p = base + (int64_t)tid * R + k;
                if (p < tiles) pol.emit(dir, dir ? tiles - 1 - p : p, r[k], v);
                v = P::apply(f[k], v);
            }
            run = P::apply(all, run);
        }
        pol.pass_end(dir, run);
        // a backward pass may read what the forward pass wrote (other threads of this workgroup)
        __threadfence_block();
        __syncthreads();
    }
    pol.report(tid);
}

}  // namespace itd
