// itd_spectrum_stream.hpp — device side of the spectrum stream (itd_spectrum_stream_* in include/pyitd_hip.h):
// the time-frequency-energy spectrum of itd_tfe_spectrum.hpp block by block, at a fixed latency, bit for bit the whole-row spectrum's
// time slices wherever no half wave is longer than the horizon.
//
// A stream holds `rows` rows in lock step, blocks of L samples (a multiple of hop, 64 <= L <= 4096), a horizon of H samples,
// D = ceil((H + 1) / L).  A[j] and f[j] are DESIGN.md section 8's on the concatenated row, from the expressions itd_tfe_batch.hpp
// uses (tfe_crossing on ABSOLUTE indices, inst_mag, phase_in, the forward phase difference with its single wrap; the stream's last
// sample takes the backward difference).  Sample j is OVERLONG if its half wave has more than H samples or sample j + 1 exists and
// its half wave has more than H samples (f[j] needs A[j + 1]) — and the stream's last sample, whose frequency is the backward
// difference, if its predecessor's half wave has; an overlong sample is outside, whatever its frequency would be.  Block
// b gives C = L / hop cells: power[C, F], outside[C], overlong[C] — rows b C .. (b + 1) C - 1 of section 19's definition.
//
// Locality.  Block b is decided from the samples [b L - H, (b+1) L + H] that exist (the READABLE range) and nothing else: the block's
// samples and sample (b+1) L need their half waves' ends, and a half wave of at most H samples that holds one of them lies in
// [b L - H + 1, (b+1) L + H - 1]; the crossing test in front of it reads b L - H, the one at its end (b+1) L + H.  A half wave whose
// end is not found inside the range is longer than H — unless the range begins at the stream's start or ends at the flushed stream's
// end.  Sample (b+1) L is the block's half wave c (the one behind the block's last crossing) whether or not that has samples in the
// block, so k_wave_stream's two searches suffice, with the readable range one sample longer.
//
// One launch per step, one workgroup per row (k_spectrum_stream), on the ring and the records of itd_wave_stream.hpp:
//   1. the arriving block into the ring (wave_ring_store), the row's edges into LDS;
//   2. the emitted block cut at its crossings (wave_ring_cut), the two searches (wave_ring_search_left / _right): every half wave's
//      amplitude and length;
//   3. per sample the phase into LDS, then the frequency from the next sample's phase, the bin by a branch-free search over the
//      edges in LDS (-1 outside, -2 overlong) and the weight: 12 B of LDS per sample;
//   4. one wavefront per cell takes the cell's steps in order: the members of every bin present in a step (k_tfe_bin's way), their
//      step sums by tfe_step_sums, added into the wavefront's acc[F] in LDS; the cell is streamed out, an empty one as +0.0.
// No atomics on global memory, no floating-point atomics, no workgroup waits for another, nothing read on the host.  Positions
// inside the ring window are int32, the window's absolute origin is int64, as in k_wave_stream.
// Dynamic LDS: 8 (L + 1) (phase / weight) + 8 (F + 1) (edges) + 4 L (bins) + max(k_wave_stream's 12 L + 12 G + 56, 16 F W) with
// G = L / 64 and W wavefronts (4 for L <= 2048, 8 above): the cut's arrays are dead when the wavefronts' acc and msk take their
// place.  L = 4096, F = 512: 32 776 + 4104 + 16 384 + 65 536 = 118 800 B.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itd_tfe_spectrum.hpp"
#include "itd_wave_stream.hpp"

#pragma clang fp contract(off)

namespace itd {

constexpr int kSpectrumStreamMinBlock = 64;
constexpr int kSpectrumStreamMaxBlock = 4096;

struct SpectrumStreamArgs {
    RingStepArgs r;                // the ring's fields (itd_ring_plan.hpp); the readable range reaches one sample past the wave filter's
    const double *edges;           // edges[0 .. F] of row r at r edges_stride (0: one set for all rows)
    int64_t edges_stride;
    double *power;                 // the emitted block's cells [C][F] of row r at r power_stride
    int64_t power_stride;
    int32_t *outside, *overlong;   // [C] of row r at r count_stride (or nullptr)
    int64_t count_stride;
    int32_t F, spc, weight;        // bins; 64-sample steps per cell (hop / 64); 0 count, 1 amplitude, 2 energy
};

// dynamic LDS of a launch with TH threads for blocks of L samples and F bins
inline size_t spectrum_stream_lds(int L, int F, int TH)
{
    const size_t cut = wave_stream_lds(L), bins = (size_t)16 * F * (TH / 64);
    return (size_t)(L + 1) * 8 + (size_t)(F + 1) * 8 + (size_t)L * 4 + ((cut > bins ? cut : bins) + 7) / 8 * 8;
}

// (a wavefront's LDS accesses are issued in order; this keeps the compiler from moving them across, where lanes read what other
// lanes of the same wavefront wrote)
__device__ __forceinline__ void spectrum_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int TH>
__global__ __launch_bounds__(TH) void k_spectrum_stream(SpectrumStreamArgs a)
{
    constexpr int SPT = kWaveStreamSpt, W = TH / 64;
    static_assert(TH % 64 == 0, "geometry");
    extern __shared__ __attribute__((aligned(16))) unsigned char ss_lds[];
    const double pi = 3.14159265358979323846;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = a.r.L, D = a.r.D, H = a.r.H, F = a.F;
    const int G = L >> 6;                                                 // 64-sample steps of the block (L is a multiple of 64)
    double *wq = reinterpret_cast<double *>(ss_lds);                                   // [L + 1] phase, then weight
    double *edg = wq + (L + 1);                                                       // [F + 1]
    int32_t *bin = reinterpret_cast<int32_t *>(edg + (F + 1));                         // [L]
    unsigned char *un = reinterpret_cast<unsigned char *>(bin + L);                   // the cut's arrays, then acc / msk
    const WaveCutLds q = wave_cut_lds(un, L);
    unsigned long long *const mag = q.mag;
    int32_t *const edge = q.edge;
    const int64_t row = blockIdx.x;
    const WaveRing rg = wave_ring_of(a.r, row, lane);

    // 1. the arriving block into its slot, its record behind it
    if (rg.in) wave_ring_store<TH>(rg, a.r.arr, a.r.store_slot, a.r.status, q.amx, &q.ctl[3], tid);
    if (!a.r.emit) return;
    const int b0 = D * L;
    const double *erow = a.edges + row * a.edges_stride;
    for (int i = tid; i <= F; i += TH) edg[i] = erow[i];

    // 2. the block cut at its crossings, the far ends of its outer half waves
    const double *const blk = rg.ring + (int64_t)((a.r.slot0 + D) % rg.R) * L;
    double xr[SPT], slope[SPT];
    bool cr[SPT];
    int seg[SPT];
    const int c = wave_ring_block<TH, true>(rg, a.r, q, blk, tid, wave, xr, slope, cr, seg);

    // 3. amplitude, phase, frequency, bin and weight of every sample
    const bool has_ext = b0 + L < a.r.rd_hi;                                // sample (b+1) L exists (and then (b+1) L + 1 too, readable: H >= 1)
    double A[SPT];
    bool ovl[SPT];
#pragma unroll
    for (int jj = 0; jj < SPT; ++jj) {
        const int g = jj * W + wave, s = g * 64 + lane;
        A[jj] = 0.0;
        ovl[jj] = false;
        if (g < G) {
            const int r = seg[jj];
            A[jj] = __builtin_bit_cast(double, mag[r]);
            ovl[jj] = edge[r + 1] - edge[r] > H || (cr[jj] && edge[r + 2] - edge[r + 1] > H);   // (cr: r + 1 <= c)
            // the stream's last sample has no successor; its backward difference needs A of its predecessor (another half wave
            // where L - 2 is a crossing index)
            if (!has_ext && s == L - 1 && r >= 1 && edge[r] == L - 2) ovl[jj] |= edge[r] - edge[r - 1] > H;
            // the stream's last sample takes the backward difference
            const double sl = (!has_ext && s == L - 1) ? xr[jj] - blk[L - 2] : slope[jj];
            wq[s] = phase_in(xr[jj], sl, A[jj]);
        }
    }
    if (tid == 0 && has_ext) {
        const double x0 = rg.ld(b0 + L), x1 = rg.ld(b0 + L + 1);
        wq[L] = phase_in(x0, x1 - x0, __builtin_bit_cast(double, mag[c]));
    }
    __syncthreads();
    double f[SPT];
#pragma unroll
    for (int jj = 0; jj < SPT; ++jj) {
        const int g = jj * W + wave, s = g * 64 + lane;
        f[jj] = 0.0;
        if (g < G) {
            double dp = (!has_ext && s == L - 1) ? wq[s] - wq[s - 1] : wq[s + 1] - wq[s];
            if (dp < 0.0) dp += 2.0 * pi;                                 // the phase wraps once per wave
            f[jj] = dp / (2.0 * pi);
        }
    }
    __syncthreads();                                                      // (the phases are read: the weights take their place)
    {
        // the edges at or below f, pos = searchsorted(edges, f, "right") (k_tfe_bin's search); a NaN has none
        const int top = 1 << (31 - __clz(F + 1));
        int pos[SPT];
#pragma unroll
        for (int jj = 0; jj < SPT; ++jj) pos[jj] = 0;
        for (int jump = top; jump >= 1; jump >>= 1) {
#pragma unroll
            for (int jj = 0; jj < SPT; ++jj) {
                const int p = pos[jj] + jump;
                if (edg[(p <= F + 1 ? p : F + 1) - 1] <= f[jj] && p <= F + 1) pos[jj] = p;
            }
        }
#pragma unroll
        for (int jj = 0; jj < SPT; ++jj) {
            const int g = jj * W + wave, s = g * 64 + lane;
            if (g < G) {
                const bool inside = pos[jj] >= 1 && pos[jj] <= F;
                bin[s] = ovl[jj] ? -2 : (inside ? pos[jj] - 1 : -1);
                wq[s] = a.weight == 0 ? 1.0 : (a.weight == 1 ? A[jj] : A[jj] * A[jj]);
            }
        }
    }
    __syncthreads();                                                      // (the cut's arrays are dead from here on)

    // 4. one wavefront per cell: its steps in order, the step sums of all bins present at once, into the wavefront's acc
    double *acc = reinterpret_cast<double *>(un) + (size_t)wave * F;                   // [W][F]
    unsigned long long *msk = reinterpret_cast<unsigned long long *>(un) + (size_t)W * F + (size_t)wave * F;   // [W][F]
    for (int i = lane; i < F; i += 64) { acc[i] = 0.0; msk[i] = 0ull; }
    spectrum_wave_sync();
    const int spc = a.spc, C = G / spc;
    double *const prow = a.power + row * a.power_stride;
    for (int cell = wave; cell < C; cell += W) {
        int out_cnt = 0, ovl_cnt = 0;
        for (int st = cell * spc; st < (cell + 1) * spc; ++st) {
            const int s = st * 64 + lane;
            const int k = bin[s];
            const bool inside = k >= 0;
            const double w = inside ? wq[s] : 0.0;
            out_cnt += __popcll(__ballot(!inside));
            ovl_cnt += __popcll(__ballot(k == -2));
            unsigned long long todo = __ballot(inside), members = 0ull;
            for (int it = 0; it < kTfeBallots && todo; ++it) {
                const int kb = __builtin_amdgcn_readlane(k, __builtin_ctzll(todo));
                const bool member = inside && k == kb;
                const unsigned long long m = __ballot(member);
                if (member) members = m;
                todo &= ~m;
            }
            if (todo) {
                const bool rest = (todo >> lane) & 1ull;
                if (rest) atomicOr(&msk[k], 1ull << lane);
                spectrum_wave_sync();
                if (rest) members = msk[k];
                spectrum_wave_sync();
                if (rest && lane == __builtin_ctzll(members)) msk[k] = 0ull;
            }
            const double sum = tfe_step_sums(w, members, lane);
            if (inside && lane == __builtin_ctzll(members)) acc[k] = acc[k] + sum;
            spectrum_wave_sync();                                         // (the next step's lanes read what these wrote)
        }
        double *dst = prow + (int64_t)cell * F;
        for (int i = lane; i < F; i += 64) {
            __builtin_nontemporal_store(acc[i], &dst[i]);
            acc[i] = 0.0;
        }
        if (lane == 0) {
            if (a.outside) a.outside[row * a.count_stride + cell] = out_cnt;
            if (a.overlong) a.overlong[row * a.count_stride + cell] = ovl_cnt;
        }
        spectrum_wave_sync();
    }
}

}  // namespace itd
