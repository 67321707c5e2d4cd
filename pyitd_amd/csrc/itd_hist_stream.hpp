// itd_hist_stream.hpp — device side of the histogram stream (itd_hist_stream_* in include/pyitd_hip.h): the half
// waves' joint amplitude-length histogram of itd_wave_hist.hpp block by block, at a fixed latency, integer for integer the whole-row
// histogram's time slices wherever no half wave is longer than the horizon.
//
// A stream holds `rows` rows in lock step, blocks of L samples (64 <= L <= 4096), a horizon of H samples, D = ceil(H / L) (reach 0, the
// wave-filter stream's).  hop is a positive multiple of 64 that divides L, C = L / hop cells per block; the amplitude edges ae[0 .. Na]
// and the length edges le[0 .. Nl] are section 20's (1 <= Na, Nl <= 64, Na Nl <= 1024), and C Na Nl <= 8192 keeps the block's histogram
// in LDS.  After P pushes row r is x[0 .. P L); crossing indices, half waves, length_k, A_k and peak_k (the smallest index with
// |x| == A_k) are itd_waves.hpp's on ABSOLUTE indices; the last half wave ends at the flushed stream's last sample.
//     length_k <= H   counted exactly once, in absolute time bin peak_k / hop, with section 20's comparisons: both bins exist:
//                     count[t][i][j] += 1, samples[t][i][j] += length_k; otherwise outside[t] += 1
//     length_k >  H   in none of the three; each of its samples j adds 1 to overlong[j / hop] — the price of the bounded latency
// Emitted block b writes the cells b C .. (b+1) C - 1: count[C][Na][Nl], samples[C][Na][Nl], outside[C], overlong[C], all int32, every
// cell written, an empty one as 0.  samples <= hop + 2 (H - 1): the half waves whose peaks fall in one cell are disjoint and at most two
// of them reach beyond the cell.
//
// Locality.  Block b is decided from the samples [b L - H, (b+1) L + H) that exist and nothing else (itd_wave_stream.hpp): a half wave
// of at most H samples whose peak lies in the block begins at or after b L - H + 1 and ends at or before (b+1) L + H - 2.  A half wave
// s..e that touches the block has the maxima ML left of the block, MB inside it and MR right of it (magnitudes as bit patterns, as
// wave_pick compares them).  Its peak lies in the block iff
//     the block's part is non-empty,   s >= b L or ML < MB (the earlier index wins a tie),   and MR <= MB.
// wave_ring_search_left / _right return exactly ML and MR; positions outside the block are never needed.
//
// One launch per step, one workgroup per row (k_hist_stream), on the ring and the records of itd_wave_stream.hpp:
//   1. the arriving block into the ring (wave_ring_store); the row's two edge sets into LDS, the block's histogram zeroed in LDS;
//   2. the emitted block cut at its crossings (wave_ring_cut) and the two searches — wave_ring_block's sequence, but with ML and MR
//      kept apart from the block's own maxima (hist_ring_block);
//   3. every half wave's first position of its maximum inside the block: an LDS atomicMin of the index among the samples that attain
//      it (k_wave_table's second round); the overlong samples per cell by ballots;
//   4. one lane per half wave 0 .. c: is its peak here (the rule above; half waves 1 .. c-1 lie inside the block), the length test
//      against H, wave_hist_search over the edges in LDS, one LDS integer atomic each into count and samples, or into outside;
//   5. behind a barrier the block's slices are streamed out whole.
// No atomics on global memory, no floating-point atomics, no workgroup waits for another, nothing read on the host.  Positions inside
// the ring window are int32, the window's absolute origin is int64, as in k_wave_stream.
// Dynamic LDS: 1056 (two edge sets of 65, ML, MR) + 4 (2 F + 2 G + L + 1) (F = C Na Nl: count, samples; outside, overlong; the peaks)
// + k_wave_stream's 12 L + 12 G + 56 with G = L / 64.  L = 4096, F = 8192: 1056 + 82 440 + 49 976 = 133 472 B.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itd_wave_hist.hpp"
#include "itd_wave_stream.hpp"

#pragma clang fp contract(off)

namespace itd {

constexpr int kHistStreamMinBlock = 64;
constexpr int kHistStreamMaxBlock = 4096;
constexpr int kHistStreamMaxCells = 8192;    // C * Na * Nl of one block

struct HistStreamArgs {
    RingStepArgs r;                // the ring's fields (itd_ring_plan.hpp)
    const double *aedges;          // ae[0 .. Na] of row r at r aedges_stride (0: one set for all rows)
    int64_t aedges_stride;
    const double *ledges;          // le[0 .. Nl] of row r at r ledges_stride
    int64_t ledges_stride;
    int32_t *count, *samples;      // the emitted block's cells [C][Na][Nl] of row r at r hist_stride
    int64_t hist_stride;
    int32_t *outside, *overlong;   // [C] of row r at r count_stride (or nullptr)
    int64_t count_stride;
    int32_t Na, Nl, spc;           // bins per axis; 64-sample groups per cell (hop / 64)
};

// int32 words of a launch's LDS behind the edges: count[F], samples[F], outside[G], overlong[G], peak[L + 1], padded to 8 bytes
__host__ __device__ inline int hist_stream_words(int L, int F) { return (2 * F + 2 * (L >> 6) + L + 1 + 1) & ~1; }

// dynamic LDS of a launch for blocks of L samples and F = C Na Nl cells
inline size_t hist_stream_lds(int L, int F, int)
{
    return (size_t)(2 * (kWaveHistMaxBins + 1) + 2) * 8 + (size_t)hist_stream_words(L, F) * 4 + (wave_stream_lds(L) + 7) / 8 * 8;
}

// wave_ring_block's sequence (itd_wave_stream.hpp) with the searches' maxima kept apart: mag[0] and mag[c] stay the maxima of the BLOCK's
// parts of half waves 0 and c, mlr[0] = ML (max |x| of half wave 0 left of the block), mlr[1] = MR (of half wave c right of it).  pk[0 .. L]
// is set to INT32_MAX on the way.  Returns c behind a barrier.
template <int TH>
__device__ __forceinline__ int hist_ring_block(const WaveRing &rg, const RingStepArgs &a, const WaveCutLds &q, unsigned long long *mlr,
                                               int32_t *pk, const double *blk, int tid, int wave, double (&xr)[kWaveStreamSpt],
                                               bool (&cr)[kWaveStreamSpt], int (&seg)[kWaveStreamSpt])
{
    constexpr int U = kWaveStreamUnroll;
    const int L = a.L, H = a.H, b0 = a.D * L;                             // b0: the emitted block's first window position
    for (int i = tid; i <= L; i += TH) { q.mag[i] = 0ull; pk[i] = INT32_MAX; }
    if (tid == 0) { q.ctl[1] = INT32_MIN; q.ctl[2] = INT32_MAX; mlr[0] = mlr[1] = 0ull; }
    double unused[kWaveStreamSpt];
    const int c = wave_ring_cut<TH, false>(rg, blk, q.mag, q.bal, q.edge, q.pre, &q.ctl[0], tid, wave, xr, unused, cr, seg);
    {
        unsigned long long m;
        int found;
        wave_ring_search_left<TH, U>(rg, &q.ctl[1], tid, m, found);
        if (m) atomicMax(&mlr[0], m);
        if (tid == 0) q.edge[0] = found != INT32_MIN ? found - b0 : (a.at_start ? a.rd_lo - 1 - b0 : -H - 2);
    }
    {
        unsigned long long m;
        int found;
        wave_ring_search_right<TH, U>(rg, &q.ctl[2], tid, m, found);
        if (m) atomicMax(&mlr[1], m);
        if (tid == 0) q.edge[c + 1] = found != INT32_MAX ? found - b0 : (a.at_end ? a.rd_hi - 1 - b0 : L + H + 2);
    }
    __syncthreads();
    return c;
}

template <int TH>
__global__ __launch_bounds__(TH) void k_hist_stream(HistStreamArgs a)
{
    constexpr int SPT = kWaveStreamSpt, W = TH / 64;
    static_assert(TH % 64 == 0, "geometry");
    extern __shared__ __attribute__((aligned(16))) unsigned char hs_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = a.r.L, D = a.r.D, H = a.r.H, Na = a.Na, Nl = a.Nl, spc = a.spc;
    const int G = L >> 6;                                                 // 64-sample groups of the block (L is a multiple of 64)
    const int C = G / spc, bins = Na * Nl, F = C * bins;
    double *ae = reinterpret_cast<double *>(hs_lds);                                  // [65]
    double *le = ae + (kWaveHistMaxBins + 1);                                         // [65]
    unsigned long long *mlr = reinterpret_cast<unsigned long long *>(le + (kWaveHistMaxBins + 1));   // ML, MR
    int32_t *cnt = reinterpret_cast<int32_t *>(mlr + 2);                              // [F]
    int32_t *smp = cnt + F;                                                           // [F]
    int32_t *outc = smp + F, *ovlc = outc + G;                                        // [G] each, C of them used
    int32_t *pk = ovlc + G;                                                           // [L + 1]
    const WaveCutLds q = wave_cut_lds(reinterpret_cast<unsigned char *>(cnt + hist_stream_words(L, F)), L);
    const int64_t row = blockIdx.x;
    const WaveRing rg = wave_ring_of(a.r, row, lane);

    // 1. the arriving block into its slot, its record behind it; the edges, the empty histogram
    if (rg.in) wave_ring_store<TH>(rg, a.r.arr, a.r.store_slot, a.r.status, q.amx, &q.ctl[3], tid);
    if (!a.r.emit) return;
    {
        const double *arow = a.aedges + row * a.aedges_stride, *lrow = a.ledges + row * a.ledges_stride;
        for (int i = tid; i <= Na; i += TH) ae[i] = arow[i];
        for (int i = tid; i <= Nl; i += TH) le[i] = lrow[i];
        for (int i = tid; i < 2 * F + 2 * G; i += TH) cnt[i] = 0;          // count, samples, outside, overlong lie in a row
    }

    // 2. the block cut at its crossings, the far ends of its outer half waves, ML and MR
    const double *const blk = rg.ring + (int64_t)((a.r.slot0 + D) % rg.R) * L;    // (window block D: never the arriving one, D >= 1)
    double xr[SPT];
    bool cr[SPT];
    int seg[SPT];
    const int c = hist_ring_block<TH>(rg, a.r, q, mlr, pk, blk, tid, wave, xr, cr, seg);

    // 3. the first position of every half wave's maximum inside the block; the overlong samples per cell
#pragma unroll
    for (int jj = 0; jj < SPT; ++jj) {
        const int g = jj * W + wave, s = g * 64 + lane;
        if (g < G) {
            const int r = seg[jj];
            if (inst_mag(xr[jj], true) == q.mag[r]) atomicMin(&pk[r], s);
            const int n = __popcll(__ballot(q.edge[r + 1] - q.edge[r] > H));
            if (lane == 0 && n) atomicAdd(&ovlc[g / spc], n);
        }
    }
    __syncthreads();

    // 4. one lane per half wave: counted here iff its peak lies in the block and it has at most H samples
    const unsigned long long ML = mlr[0], MR = mlr[1];
    for (int r = tid; r <= c; r += TH) {
        const int32_t e0 = q.edge[r], len = q.edge[r + 1] - e0;
        const unsigned long long MB = q.mag[r];
        bool here = true;
        if (r == 0) here = e0 == -1 || ML < MB;                           // it begins with the block, or the block's maximum is larger
        if (r == c) here = here && e0 < L - 1 && MR <= MB;                // it has samples in the block, and nothing larger follows
        const int32_t p = pk[r];
        if (!here || len > H || p >= L) continue;
        int pa, pl;
        wave_hist_search(ae, Na, __builtin_bit_cast(double, MB), le, Nl, (double)len, pa, pl);
        const int cell = (p >> 6) / spc;
        if (pa >= 1 && pa <= Na && pl >= 1 && pl <= Nl) {
            const int i = cell * bins + (pa - 1) * Nl + (pl - 1);
            atomicAdd(&cnt[i], 1);
            atomicAdd(&smp[i], len);
        } else {
            atomicAdd(&outc[cell], 1);
        }
    }
    __syncthreads();

    // 5. the block's slices, whole
    int32_t *const crow = a.count + row * a.hist_stride, *const srow = a.samples + row * a.hist_stride;
    for (int i = tid; i < F; i += TH) {
        __builtin_nontemporal_store(cnt[i], &crow[i]);
        __builtin_nontemporal_store(smp[i], &srow[i]);
    }
    if (tid < C) {
        if (a.outside) a.outside[row * a.count_stride + tid] = outc[tid];
        if (a.overlong) a.overlong[row * a.count_stride + tid] = ovlc[tid];
    }
}

}  // namespace itd
