// itd_tfe_spectrum.hpp — the time-frequency-energy spectrum of MANY rows in one asynchronous call: every row's instantaneous
// amplitude A and frequency f (itd_tfe_batch.hpp: the same bits itd_instantaneous_batch_* stores in float64) binned over time
// and frequency without ever being stored.  The definition (include/pyitd_hip.h) fixes the bins by IEEE
// comparisons against the edges and the order of every sum, so the result is a function of the row alone:
//     bin of sample j    the k with edges[k] <= f[j] && f[j] < edges[k+1]; none (f below edges[0], at or above edges[F], NaN): outside
//     step sum           step s = samples 64 s .. 64 s + 63 of the row; v[l] = w[64 s + l] where that sample exists and lies in bin
//                        k, else +0.0; the adjacent-pair tree (v0 + v1), (v2 + v3), ... of six levels
//     cell S[t, k]       +0.0, then the step sums of the steps t hop / 64 .. (t + 1) hop / 64 - 1 that exist, in increasing order
//     outside[t]         the outside samples with j / hop == t
// w = 1.0, A or A * A (one float64 multiply).  Launches per chunk of rows: k_inst_records and k_inst_carry as they are, then
// k_tfe_bin in k_inst_apply's place: one wavefront per (row, time bin) where hop >= 512, per (row, tile) below (hop 64, 128, 256:
// a cell never straddles a tile).  The wavefront walks its steps in order, evaluates their tiles with inst_tile_eval — the
// expressions k_inst_apply stores from — and finds every lane's bin by a binary search over the edges in LDS.  It loops over the
// distinct bins present in a step (the lowest remaining lane's bin, its members by a ballot; from the fifth bin on an integer OR
// into the bin's word in LDS) only to hand every lane its bin's member mask.  The step sums of all those bins then come from ONE
// pass over the tree's six levels (tfe_step_sums), and every bin's lowest member lane adds its sum into acc[bin] in LDS.  At a
// cell's end the F sums and the outside count are streamed to their place and acc is cleared.  (One butterfly of
// member ? w : +0.0 per distinct bin gives the same bits; on rows whose frequencies scatter over 30 to 50 bins per step it took
// 12.1 ms at 9 x 2^24 samples where this form takes 3.2 ms: DESIGN.md section 19.)  No atomics on global memory, no
// floating-point atomics at all, no workgroup waits for another, nothing read on the host.
// LDS per wavefront: 4104 B (tile_segment_max) + 8 F (acc) + 8 (F + 1) (edges) + 8 F (msk), dynamic: 16400 B at F = 512.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itd_tfe_batch.hpp"

#pragma clang fp contract(off)

namespace itd {

constexpr int kTfeMaxBins = 512;
constexpr int kTfeBallots = 4;          // distinct bins of a step found by ballots before the rest go through LDS

// k_tfe_bin's sink: a tile's amplitudes and frequencies kept in registers
struct TfeKeep {
    double (&A)[kInstSteps];
    double (&f)[kInstSteps];
    double A_last = 0.0, f_last = 0.0;
    __device__ __forceinline__ void sample(int g, int64_t, bool, double a, double) { A[g] = a; }
    __device__ __forceinline__ void freq(int g, int64_t, bool, double v) { f[g] = v; }
    __device__ __forceinline__ void last(double a, double v) { A_last = a; f_last = v; }
};

// The step sums of ALL bins present in a step at once.  members: the lanes of this lane's bin (0 for a lane outside); v: the
// lane's weight (+0.0 outside).  Level b of the adjacent-pair tree joins the two halves (2^b lanes each) of every aligned group
// of 2^(b+1) lanes; a bin's partial sum of a half stays with the half's lowest member lane.  Where both halves hold members the
// lower half's keeper fetches the upper half's partial and adds it (lower + upper, the tree's order); where one half holds
// none, the tree adds +0.0 to a non-negative value, which changes nothing, and the keeper keeps what it has.  After six levels
// the bin's lowest member lane holds the bin's step sum: bit for bit the tree over member ? w : +0.0.
__device__ __forceinline__ double tfe_step_sums(double v, unsigned long long members, int lane)
{
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        const int half = 1 << b;
        const unsigned long long lower = ((1ull << half) - 1ull) << (lane & ~(2 * half - 1));
        const unsigned long long ml = members & lower, mu = members & (lower << half);
        const bool take = ml != 0ull && mu != 0ull && lane == __builtin_ctzll(ml);
        const double up = __shfl(v, take ? __builtin_ctzll(mu) : lane);
        if (take) v = v + up;
    }
    return v;
}

template <typename Tin>
__global__ __launch_bounds__(64) void k_tfe_bin(const Tin *__restrict__ rows, int64_t row_stride, int64_t n, int64_t tiles,
                                                const double *__restrict__ Ahead, const double *__restrict__ Atail,
                                                const double *__restrict__ edges, int F, int64_t hop, int weight, int64_t T,
                                                double *__restrict__ spec, int64_t spec_stride, int32_t *__restrict__ outside)
{
    __shared__ unsigned long long seg[kTfeTile + 1];
    extern __shared__ double tfe_lds[];
    double *acc = tfe_lds, *edg = tfe_lds + F;          // acc[F], edg[F + 1], msk[F]
    unsigned long long *msk = reinterpret_cast<unsigned long long *>(tfe_lds + 2 * F + 1);
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.y;
    const Tin *x = rows + row * row_stride;
    for (int i = lane; i <= F; i += 64) edg[i] = edges[i];
    for (int i = lane; i < F; i += 64) { acc[i] = 0.0; msk[i] = 0ull; }
    __syncthreads();
    // the wavefront's steps [st0, st1): one cell of hop >= 512 samples, or the cells of one tile
    const int64_t spc = hop / 64;                       // steps per cell
    const int64_t steps = (n + 63) / 64;
    const int64_t cell0 = hop >= kTfeTile ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * (kTfeTile / hop);
    const int64_t cells = hop >= kTfeTile ? 1 : kTfeTile / hop;
    const int64_t st0 = cell0 * spc;
    const int64_t st1 = (cell0 + cells) * spc < steps ? (cell0 + cells) * spc : steps;
    const int top = 1 << (31 - __clz(F + 1));           // the largest power of two in F + 1 edges
    int out_cnt = 0;
    for (int64_t tt = st0 / kInstSteps; tt * kInstSteps < st1; ++tt) {
        const int64_t s = tt * kTfeTile;
        // the lone sample of a row's last tile has its frequency from the tile before: evaluate that one and keep its last()
        const bool lone = s == n - 1;
        const int64_t te = lone ? tt - 1 : tt;
        double A[kInstSteps], f[kInstSteps];
        TfeKeep keep = {A, f};
        inst_tile_eval<Tin>(x, n, te * kTfeTile, row * tiles + te, lane, Ahead, Atail, seg, true, keep);
        if (lone) { A[0] = keep.A_last; f[0] = keep.f_last; }
        // the edges at or below f, pos = searchsorted(edges, f, "right"), for the tile's eight steps side by side (independent LDS
        // reads); a NaN has none.  Whatever the edges hold, an index stays inside them.
        int pos[kInstSteps];
#pragma unroll
        for (int g = 0; g < kInstSteps; ++g) pos[g] = 0;
        for (int jump = top; jump >= 1; jump >>= 1) {
#pragma unroll
            for (int g = 0; g < kInstSteps; ++g) {
                const int p = pos[g] + jump;
                if (edg[(p <= F + 1 ? p : F + 1) - 1] <= f[g] && p <= F + 1) pos[g] = p;
            }
        }
#pragma unroll
        for (int g = 0; g < kInstSteps; ++g) {
            const int64_t st = tt * kInstSteps + g;
            if (st < st0 || st >= st1) continue;        // (the same for every lane)
            const bool in = s + g * 64 + lane < n;
            const bool inside = in && pos[g] >= 1 && pos[g] <= F;
            const int k = pos[g] - 1;
            const double w = weight == 0 ? 1.0 : (weight == 1 ? A[g] : A[g] * A[g]);
            out_cnt += __popcll(__ballot(in && !inside));
            // the distinct bins present in the step: the lowest remaining lane's bin, its members by a ballot — for up to kTfeBallots
            // bins, which is every bin of a step on a row whose frequency moves slowly; the lanes of a step that holds more bins
            // meet on their bin's word of msk (an integer OR in LDS: the outcome does not depend on the order) and clear it again
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
                __builtin_amdgcn_wave_barrier();
                if (rest) members = msk[k];
                __builtin_amdgcn_wave_barrier();
                if (rest && lane == __builtin_ctzll(members)) msk[k] = 0ull;
            }
            // ... their step sums by one pass over the tree's levels; a bin's lowest member adds its sum into acc (the bins differ)
            const double sum = tfe_step_sums(inside ? w : 0.0, members, lane);
            if (inside && lane == __builtin_ctzll(members)) acc[k] = acc[k] + sum;
            __builtin_amdgcn_wave_barrier();            // (the next step's lanes read what these wrote: one wavefront, LDS in order)
            if ((st + 1) % spc == 0 || st + 1 == st1) {
                // the cell's end: its F sums and its outside count to their place, acc cleared for the next one
                const int64_t cell = st / spc;
                __syncthreads();
                double *dst = spec + row * spec_stride + cell * F;
                for (int i = lane; i < F; i += 64) {
                    __builtin_nontemporal_store(acc[i], &dst[i]);
                    acc[i] = 0.0;
                }
                if (outside && lane == 0) outside[row * T + cell] = out_cnt;
                out_cnt = 0;
                __syncthreads();
            }
        }
    }
}

}  // namespace itd
