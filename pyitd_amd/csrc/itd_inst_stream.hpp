// itd_inst_stream.hpp — device side of the instantaneous stream (itd_inst_stream_* in include/pyitd_hip.h): the
// instantaneous amplitude, phase and frequency of itd_tfe_batch.hpp and every sample's half-wave length block by block, at a fixed
// latency, bit for bit the whole-row operator's values wherever they are delivered.
//
// A stream holds `rows` rows in lock step, blocks of L samples (8 <= L <= 4096, any L), a horizon of H samples,
// D = ceil((H + 1) / L).  A[j], phase[j], f[j] and len[j] are DESIGN.md section 8's and section 18's on the concatenated row, from the
// expressions k_spectrum_stream uses (tfe_crossing on ABSOLUTE indices, inst_mag, phase_in, the forward phase difference with its
// single wrap; the stream's last sample takes the backward difference).  Sample j is LONG if len[j] > H and OVERLONG by section
// 22's rule (long, or its successor is; the stream's last sample: or its predecessor is).  Block b gives, per sample,
//     amplitude = A, phase = phase   where the sample is not long      (they need its own half wave and x[j + 1] only)
//     frequency = f                  where it is not overlong
//     length    = len (int32)        where it is not long, else 0
// and kInstStreamNaN in every float64 slot that is not delivered; per row two counts, the long and the overlong samples.
//
// Locality, the ring, the records and the readable range [b L - H, (b+1) L + H] are the spectrum stream's (itd_spectrum_stream.hpp);
// steps 1 to 3 below are its steps 1 to 3, but with every per-sample access guarded by s < L: the block's last 64-sample step is
// ragged where L is no multiple of 64, and L = 8 is less than one wavefront.
//
// One launch per step, one workgroup per row (k_inst_stream):
//   1. the arriving block into the ring (wave_ring_store);
//   2. the emitted block cut at its crossings (wave_ring_cut), the two searches (wave_ring_search_left / _right): every half wave's
//      amplitude and length;
//   3. per sample the amplitude from mag, long / overlong from the edge differences, the phase into LDS; behind a barrier the
//      frequency from the next sample's phase (sample (b+1) L's by one thread);
//   4. the wanted outputs streamed out, 8 (4) bytes per lane, consecutive lanes on consecutive samples; a NULL output is skipped;
//      the two counts: ballots and popcounts per wavefront, two LDS integer adds per wavefront, one plain store per row.
// No atomics on global memory, no floating-point atomics, no workgroup waits for another, nothing read on the host.  Positions
// inside the ring window are int32, the window's absolute origin is int64, as in k_wave_stream.
// Dynamic LDS: 8 (L + 1) (phases) + k_wave_stream's 12 L + 12 G + 56 with G = ceil(L / 64).  L = 4096: 32 776 + 49 976 = 82 752 B —
// one workgroup of 512 threads per CU by LDS; a block of 8192 samples would need 165 KB and does not fit the CU's 160 KB.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itd_wave_stream.hpp"

#pragma clang fp contract(off)

namespace itd {

constexpr int kInstStreamMinBlock = 8;
constexpr int kInstStreamMaxBlock = 4096;
constexpr unsigned long long kInstStreamNaN = 0x7FF8000000000000ull;    // every float64 value that is not delivered

struct InstStreamArgs {
    RingStepArgs r;                // the ring's fields (itd_ring_plan.hpp); the readable range is the spectrum stream's
    double *amp, *phase, *freq;    // the emitted block of row r at r out_stride (each or nullptr)
    int32_t *length;
    int64_t out_stride;
    int32_t *counts;               // (long, overlong) of row r at r counts_stride (or nullptr)
    int64_t counts_stride;
};

// dynamic LDS of a launch for blocks of L samples
inline size_t inst_stream_lds(int L) { return (size_t)(L + 1) * 8 + wave_stream_lds(L); }

template <int TH>
__global__ __launch_bounds__(TH) void k_inst_stream(InstStreamArgs a)
{
    constexpr int SPT = kWaveStreamSpt, W = TH / 64;
    static_assert(TH % 64 == 0, "geometry");
    extern __shared__ __attribute__((aligned(16))) unsigned char is_lds[];
    const double pi = 3.14159265358979323846;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = a.r.L, D = a.r.D, H = a.r.H;
    const int G = (L + 63) >> 6;                                          // 64-sample steps of the block, the last one ragged
    double *ph = reinterpret_cast<double *>(is_lds);                                   // [L + 1] phase
    const WaveCutLds q = wave_cut_lds(reinterpret_cast<unsigned char *>(ph + (L + 1)), L);   // the cut's arrays (wave_stream_lds)
    unsigned long long *const mag = q.mag, *const bal = q.bal;
    int32_t *const edge = q.edge, *const ctl = q.ctl;                     // ctl[4] long, ctl[5] overlong samples
    const int64_t row = blockIdx.x;
    const WaveRing rg = wave_ring_of(a.r, row, lane);

    // 1. the arriving block into its slot, its record behind it
    if (rg.in) wave_ring_store<TH>(rg, a.r.arr, a.r.store_slot, a.r.status, q.amx, &ctl[3], tid);
    if (!a.r.emit) return;
    const int b0 = D * L;

    // 2. the block cut at its crossings, the far ends of its outer half waves
    if (tid == 0) { ctl[4] = 0; ctl[5] = 0; }
    const double *const blk = rg.ring + (int64_t)((a.r.slot0 + D) % rg.R) * L;
    double xr[SPT], slope[SPT];
    bool cr[SPT];
    int seg[SPT];
    const int c = wave_ring_block<TH, true>(rg, a.r, q, blk, tid, wave, xr, slope, cr, seg);

    // 3. amplitude, length and phase of every sample; long and overlong
    const bool has_ext = b0 + L < a.r.rd_hi;                                // sample (b+1) L exists (and then (b+1) L + 1 too, readable: H >= 1)
    // (the block's length once more, through readfirstlane: s < Lq is then compared anew below — against L the compiler keeps the
    // cut's eight lane masks of s < L alive across the searches and spills SGPRs for them)
    const int Lq = __builtin_amdgcn_readfirstlane(L);
    double A[SPT], pv[SPT];
    int len[SPT];                                                         // 0: a long sample
    unsigned ovm = 0;                                                     // bit jj: sample jj is overlong
    int n_long = 0, n_ovl = 0;                                            // this wavefront's counts
#pragma unroll
    for (int jj = 0; jj < SPT; ++jj) {
        const int g = jj * W + wave, s = g * 64 + lane;
        A[jj] = pv[jj] = 0.0;
        len[jj] = 0;
        if (g < G) {
            bool lng = false, ov = false;
            if (s < Lq) {
                const int r = seg[jj];
                const int32_t n = edge[r + 1] - edge[r];
                const bool last = !has_ext && s == L - 1;                 // the stream's last sample: no successor
                A[jj] = __builtin_bit_cast(double, mag[r]);
                lng = n > H;
                // (the crossing flags from the cut's ballots, not from 8 lane masks kept across the searches; a crossing index: r + 1 <= c)
                ov = lng || (((bal[g] >> lane) & 1ull) && edge[r + 2] - edge[r + 1] > H);
                // its backward difference needs A of its predecessor (another half wave where L - 2 is a crossing index)
                if (last && r >= 1 && edge[r] == L - 2) ov |= edge[r] - edge[r - 1] > H;
                pv[jj] = phase_in(xr[jj], last ? xr[jj] - blk[L - 2] : slope[jj], A[jj]);
                ph[s] = pv[jj];
                len[jj] = lng ? 0 : n;
                ovm |= ov ? 1u << jj : 0u;
            }
            n_long += __popcll(__ballot(lng));
            n_ovl += __popcll(__ballot(ov));
        }
    }
    if (tid == 0 && has_ext) {
        const double x0 = rg.ld(b0 + L), x1 = rg.ld(b0 + L + 1);
        ph[L] = phase_in(x0, x1 - x0, __builtin_bit_cast(double, mag[c]));
    }
    if (a.counts && lane == 0 && (n_long | n_ovl)) {
        atomicAdd(&ctl[4], n_long);
        atomicAdd(&ctl[5], n_ovl);
    }
    __syncthreads();

    // 4. the frequency from the next sample's phase; the wanted outputs out
    const double none = __builtin_bit_cast(double, kInstStreamNaN);
    double *const amp = a.amp ? a.amp + row * a.out_stride : nullptr, *const phs = a.phase ? a.phase + row * a.out_stride : nullptr;
    double *const frq = a.freq ? a.freq + row * a.out_stride : nullptr;
    int32_t *const lno = a.length ? a.length + row * a.out_stride : nullptr;
#pragma unroll
    for (int jj = 0; jj < SPT; ++jj) {
        const int g = jj * W + wave, s = g * 64 + lane;
        if (g < G && s < Lq) {
            const bool lng = len[jj] == 0;
            if (amp) __builtin_nontemporal_store(lng ? none : A[jj], &amp[s]);
            if (phs) __builtin_nontemporal_store(lng ? none : pv[jj], &phs[s]);
            if (frq) {
                double dp = (!has_ext && s == L - 1) ? ph[s] - ph[s - 1] : ph[s + 1] - ph[s];
                if (dp < 0.0) dp += 2.0 * pi;                             // the phase wraps once per wave
                __builtin_nontemporal_store(((ovm >> jj) & 1u) ? none : dp / (2.0 * pi), &frq[s]);
            }
            if (lno) __builtin_nontemporal_store(len[jj], &lno[s]);
        }
    }
    if (a.counts && tid == 0) {
        int32_t *const cnt = a.counts + row * a.counts_stride;
        cnt[0] = ctl[4];
        cnt[1] = ctl[5];
    }
}

}  // namespace itd
