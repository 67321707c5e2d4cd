// itd_table_stream.hpp — device side of the half-wave table stream (itd_table_stream_* in include/pyitd_hip.h):
// the half-wave table of itd_waves.hpp block by block, with no horizon and no latency.  Every half wave leaves in the push in which
// its end becomes known, whatever its length; concatenated, the events are the whole-row table integer for integer, value bit for bit.
//
// A stream holds `rows` rows in lock step, blocks of L samples (8 <= L <= 4096, any L).  Indices count from the stream's first sample.
// Crossing index i: i >= 1, x[i + 1] exists, a strict sign change between x[i] and x[i + 1] (tfe_crossing's comparison); it is the
// last sample of its half wave.  Push p brings the samples [p L, (p+1) L) and decides the crossing indices max(1, p L - 1) ..
// (p+1) L - 2: sample j of the block is FLAGGED if j - 1 is a crossing index (the predecessor of the block's first sample is the last
// sample of the push before), and a flagged sample is the first sample of a half wave.  With c flags the block's samples fall into
// the segments 0 .. c: segment 0 continues the half wave that was open when the push began, segments 1 .. c begin at the flagged
// samples; the half waves of the segments 0 .. c-1 end in this push (events), segment c is open behind it.
//
// What is open between two pushes is one TableCarry per row (48 B): where the open half wave began, the pair (magnitude bits, index
// of its first occurrence) of itd_waves.hpp's wave_pick, the signed sample at that index, and the last sample pushed.  Segment 0 is
// joined to it with wave_pick's rule: the larger magnitude, on equal magnitudes the smaller index — the carry's, which lies in front
// of the block.  That is the rule the whole-row scan applies tile after tile, so the join is exact for a half wave of any length.
//
// One launch per push, one workgroup per row (k_table_stream), up to 8 samples per thread in registers:
//   1. the carry and the arriving block from the caller's pointer; a NaN in it: status = 2, a plain store;
//   2. the flags as ballots, their sums per 64-sample group through LDS, a prefix over the groups: every sample's segment number;
//   3. tile_segment_max's two rounds on the whole block: one LDS atomicMax per sample on the magnitude bits, an LDS atomicMin of the
//      position among the samples that attain it;
//   4. event e at entry e of the row's slot: start (the carried one for e = 0, else the e-th flagged sample), length (up to the
//      sample in front of the (e+1)-th flagged one), peak; value by the thread that holds the peak sample in a register (event 0: the
//      carried value where the carry holds the peak).  Segment c goes to entry c — the open half wave so far — and into the carry.
// A flush step reads the carry alone and writes one event.  With block number 0 the carry is not read: it may hold anything.
// No atomics on global memory, no floating-point atomics, no workgroup waits for another, nothing read on the host.  Positions inside
// the block are int32, everything stored is int64.
// Dynamic LDS: 8 (L + 1) (mag) + 8 G (ballots) + 4 (L + 1) (peak) + 4 (L + 2) (first) + 4 G (prefix) + 16 with G = ceil(L / 64);
// L = 4096: 66 340 B.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itd_waves.hpp"

#pragma clang fp contract(off)

namespace itd {

constexpr int kTableStreamMinBlock = 8;
constexpr int kTableStreamMaxBlock = 4096;
constexpr int kTableStreamSpt = 8;             // samples of the block per thread
constexpr int kTableStreamSmall = 256 * kTableStreamSpt;   // up to here 256 threads, 512 above

// the open half wave of one row between two pushes; indices count from the stream's first sample
struct TableCarry {
    int64_t start;                 // its first sample
    unsigned long long m;          // max |x| so far, as a bit pattern
    int64_t peak;                  // the smallest index that attains it
    double value;                  // x[peak]
    double last;                   // the last sample pushed
    int64_t pad;
};
static_assert(sizeof(TableCarry) == 48, "TableCarry layout");

struct TableStreamArgs {
    const double *in;              // this push's block of row r at r in_stride; nullptr: a flush step
    int64_t in_stride;
    TableCarry *carry;             // [rows]
    int32_t *status;               // = 2: a pushed block held a NaN
    int64_t blk;                   // a push: the block's number p (0: the carry is not read); a flush step: the blocks pushed
    int64_t origin;                // added to every start and peak that is stored
    int64_t *start, *length, *peak;    // entry e of row r at r event_stride + e (each or nullptr)
    double *value;
    int64_t event_stride;
    int32_t *count;                // [rows]
    int32_t L;
};

// dynamic LDS of a launch for blocks of L samples
inline size_t table_stream_lds(int L)
{
    const size_t groups = (size_t)(L + 63) / 64;
    return (size_t)(L + 1) * sizeof(unsigned long long) + groups * sizeof(unsigned long long) + (size_t)(L + 1) * sizeof(int32_t) +
           (size_t)(L + 2) * sizeof(int32_t) + groups * sizeof(int32_t) + 4 * sizeof(int32_t);
}

template <int TH>
__global__ __launch_bounds__(TH) void k_table_stream(TableStreamArgs a)
{
    constexpr int SPT = kTableStreamSpt, W = TH / 64;
    static_assert(TH % 64 == 0 && TH * SPT >= kTableStreamSmall, "geometry");
    extern __shared__ __attribute__((aligned(16))) unsigned char ts_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = a.L;
    const int G = (L + 63) >> 6;                                          // 64-sample groups of the block, the last one ragged (G <= 64)
    const int64_t row = blockIdx.x;
    const int64_t o = row * a.event_stride;
    TableCarry *const cp = a.carry + row;

    if (!a.in) {                                                          // a flush step: the open half wave ends with the stream
        if (tid == 0) {
            const TableCarry cy = *cp;
            if (a.start) a.start[o] = a.origin + cy.start;
            if (a.length) a.length[o] = a.blk * L - cy.start;
            if (a.peak) a.peak[o] = a.origin + cy.peak;
            if (a.value) a.value[o] = cy.value;
            a.count[row] = 1;
        }
        return;
    }

    unsigned long long *const mag = reinterpret_cast<unsigned long long *>(ts_lds);    // [L + 1] by segment
    unsigned long long *const bal = mag + (L + 1);                                     // [G] the flags of a group
    int32_t *const peak = reinterpret_cast<int32_t *>(bal + G);                        // [L + 1] by segment, position in the block
    int32_t *const first = peak + (L + 1);                                             // [L + 2] first[r]: segment r's first position (r >= 1)
    int32_t *const pre = first + (L + 2);                                              // [G] the flags in front of a group
    int32_t *const ctl = pre + G;                                                      // [0] c

    // 1. the carry (never read in a stream's first push) and the block
    const bool fresh = a.blk == 0;
    const int64_t base = a.blk * L;                                       // the index of the block's first sample
    TableCarry cy = {0, 0ull, 0, 0.0, 0.0, 0};
    if (!fresh) cy = *cp;
    const double *const blk = a.in + row * a.in_stride;
    double xr[SPT];
    bool fl[SPT];
    bool nan = false;
#pragma unroll
    for (int jj = 0; jj < SPT; ++jj) {
        const int g = jj * W + wave, s = g * 64 + lane;                   // (g is the same for the whole wavefront)
        xr[jj] = 0.0;
        fl[jj] = false;
        if (g < G) {
            if (s < L) xr[jj] = blk[s];
            nan |= xr[jj] != xr[jj];
            // 2. flagged: the sample in front is a crossing index (its own index is at least 1)
            double xp = __shfl_up(xr[jj], 1);
            if (lane == 0) xp = s > 0 ? blk[s - 1] : cy.last;
            fl[jj] = s < L && base + s - 1 >= 1 && (((xp > 0.0) && (0.0 > xr[jj])) || ((xp < 0.0) && (0.0 < xr[jj])));
            const unsigned long long m = __ballot(fl[jj]);
            if (lane == 0) bal[g] = m;
        }
    }
    if (nan) *a.status = 2;                                               // (every writer stores the same word)
    for (int i = tid; i <= L; i += TH) {
        mag[i] = 0ull;
        peak[i] = kWaveNone;
    }
    __syncthreads();
    if (wave == 0) {                                                      // exclusive prefix of the groups' counts
        const int p0 = lane < G ? __popcll(bal[lane]) : 0;
        int i0 = p0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o0 = __shfl_up(i0, d);
            if (lane >= d) i0 += o0;
        }
        if (lane < G) pre[lane] = i0 - p0;
        if (lane == 63) ctl[0] = i0;
    }
    __syncthreads();
    const int c = ctl[0];

    // 3. every segment's maximum, then the first position that attains it
    int seg[SPT];
#pragma unroll
    for (int jj = 0; jj < SPT; ++jj) {
        const int g = jj * W + wave, s = g * 64 + lane;
        seg[jj] = 0;
        if (g < G && s < L) {
            seg[jj] = pre[g] + __popcll(bal[g] & ((2ull << lane) - 1ull));   // the flags up to and including its own
            atomicMax(&mag[seg[jj]], inst_mag(xr[jj], true));
            if (fl[jj]) first[seg[jj]] = s;
        }
    }
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < SPT; ++jj) {
        const int g = jj * W + wave, s = g * 64 + lane;
        if (g < G && s < L && inst_mag(xr[jj], true) == mag[seg[jj]]) atomicMin(&peak[seg[jj]], s);
    }
    __syncthreads();

    // 4. the events 0 .. c-1 and the open half wave, entry c.  Segment 0 joined to the carry: the carry's index is the earlier one
    const bool keep = !fresh && cy.m >= mag[0];                           // the peak of half wave 0 lies in front of the block
    const unsigned long long m0 = keep ? cy.m : mag[0];
    const int64_t p0 = keep ? cy.peak : base + peak[0];
    for (int e = tid; e <= c; e += TH) {
        const int64_t st = e == 0 ? cy.start : base + first[e];
        const int64_t en = e < c ? base + first[e + 1] : base + L;        // one past its last sample (so far)
        if (a.start) a.start[o + e] = a.origin + st;
        if (a.length) a.length[o + e] = en - st;
        if (a.peak) a.peak[o + e] = a.origin + (e == 0 ? p0 : base + peak[e]);
    }
    if (tid == 0) {
        if (keep && a.value) a.value[o] = cy.value;
        a.count[row] = c;
        cp->start = c == 0 ? cy.start : base + first[c];
        cp->m = c == 0 ? m0 : mag[c];
        cp->peak = c == 0 ? p0 : base + peak[c];
        if (c == 0 && keep) cp->value = cy.value;                         // (fresh: keep is false, the peak's thread stores it)
    }
#pragma unroll
    for (int jj = 0; jj < SPT; ++jj) {
        const int g = jj * W + wave, s = g * 64 + lane;
        if (g < G && s < L) {
            const int r = seg[jj];
            if (peak[r] == s && (r > 0 || !keep)) {                       // this thread holds the half wave's extremum
                if (a.value) a.value[o + r] = xr[jj];
                if (r == c) cp->value = xr[jj];
            }
            if (s == L - 1) cp->last = xr[jj];
        }
    }
}

}  // namespace itd
