// itd_wave_hist.hpp — the joint amplitude-length histogram of MANY rows' half waves in one asynchronous call: how a row's half
// waves (itd_waves.hpp: start_k, end_k, length_k, A_k, peak_k) are distributed over amplitude, length and time, without the table
// of 20 bytes per half wave that itd_waves_batch_* writes.  The definition (include/pyitd_hip.h):
//     amplitude bin of half wave k   the i with ae[i] <= A_k && A_k < ae[i+1]                     (IEEE comparisons on float64)
//     length bin                     the j with le[j] <= (double)length_k && (double)length_k < le[j+1]
//     time bin                       t = peak_k / hop, T = ceil(n / hop)
//     both i and j exist             count[t][i][j] += 1, samples[t][i][j] += length_k
//     otherwise                      outside[t] += 1
// Every output is an int32 and every update an integer add: the result does not depend on the order of the updates, so it is the
// same bits from run to run and in any batch position.  No floating-point atomics anywhere.
// Launches per chunk of rows: k_wave_hist_zero (the rows' slots, not the gaps between them), k_wave_records and k_wave_carry as
// they are, then k_wave_hist in k_wave_table's place: one wavefront per 512-sample tile bins the half waves that END in the tile
// (the row's last tile also the row's last one), the set k_wave_table emits.  hop is a multiple of 512, so the half waves
// 1 .. c-1 of a tile — they begin and end in it, and so does their peak, which therefore need not be found — share the tile's
// time bin: they meet in a per-tile histogram in LDS (one integer atomic per half wave on a word that packs count << 16 |
// samples; a tile holds at most 511 of them with at most 512 samples), and the lane that finds a cell's word at zero hands that
// cell on to the global histograms behind a barrier: one integer atomic per touched cell and output.  Half wave 0 reaches the
// tile from the left and its peak may lie many tiles back; it, and the row's last half wave, go to their own time bin directly,
// with the peak the carries hold.
// The tile's histogram takes the place of the half waves' maxima once every half wave knows its cell.
// LDS per wavefront: 6160 B (WaveTileLds<false>) + 8 (Na + Nl + 2) B dynamic for the edges: 6.7 KB at 32 x 32 bins.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itd_waves.hpp"

#pragma clang fp contract(off)

namespace itd {

constexpr int kWaveHistMaxBins = 64;        // per axis
constexpr int kWaveHistMaxCells = 1024;     // abins * lbins
constexpr int kWaveHistZeroThreads = 256;

// bytes of k_wave_hist's dynamic LDS: ae[Na + 1] and le[Nl + 1]
inline size_t wave_hist_lds(int abins, int lbins)
{
    return (size_t)(abins + lbins + 2) * sizeof(double);
}

// Every cell of the rows' slots and every entry of outside to zero; the gaps between the rows' slots are not written.
__global__ __launch_bounds__(kWaveHistZeroThreads) void k_wave_hist_zero(int32_t *__restrict__ count, int32_t *__restrict__ samples,
                                                                         int64_t hist_stride, int64_t slot, int32_t *__restrict__ outside,
                                                                         int64_t T)
{
    const int64_t i = (int64_t)blockIdx.x * kWaveHistZeroThreads + threadIdx.x;
    const int64_t row = blockIdx.y;
    if (i < slot) {
        if (count) count[row * hist_stride + i] = 0;
        if (samples) samples[row * hist_stride + i] = 0;
    }
    if (outside && i < T) outside[row * T + i] = 0;
}

// pos = the number of edges at or below v (searchsorted(edges, v, "right")) for ordered edges e[0 .. N]; v lies in bin pos - 1 iff
// 1 <= pos <= N.  Whatever the edges hold, an index stays inside them.  Two searches side by side: independent LDS reads.
__device__ __forceinline__ void wave_hist_search(const double *ae, int Na, double va, const double *le, int Nl, double vl, int &pa, int &pl)
{
    pa = pl = 0;
#pragma unroll
    for (int jump = kWaveHistMaxBins; jump >= 1; jump >>= 1) {
        const int qa = pa + jump, ql = pl + jump;
        const double ea = ae[(qa <= Na + 1 ? qa : Na + 1) - 1], el = le[(ql <= Nl + 1 ? ql : Nl + 1) - 1];
        if (qa <= Na + 1 && ea <= va) pa = qa;
        if (ql <= Nl + 1 && el <= vl) pl = ql;
    }
}

template <typename Tin>
__global__ __launch_bounds__(64) void k_wave_hist(const Tin *__restrict__ rows, int64_t row_stride, int64_t n, int64_t tiles,
                                                  const WaveFwd *__restrict__ fwd, const WaveBwd *__restrict__ bwd,
                                                  const double *__restrict__ aedges, int64_t aedges_stride, int Na,
                                                  const double *__restrict__ ledges, int64_t ledges_stride, int Nl, int64_t hop, int64_t T,
                                                  int32_t *__restrict__ count, int32_t *__restrict__ samples, int64_t hist_stride,
                                                  int32_t *__restrict__ outside)
{
    __shared__ WaveTileLds<false> L;                                // (no peak but the carries' is needed: see below)
    extern __shared__ double wave_hist_edges[];
    static_assert(sizeof(L.mag) >= kWaveHistMaxCells * sizeof(uint32_t), "the tile's histogram takes the maxima's place");
    const int cells = Na * Nl;
    double *ae = wave_hist_edges, *le = ae + Na + 1;
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.y;
    const int64_t t = blockIdx.x, s = t * kTfeTile;
    const Tin *x = rows + row * row_stride;
    const int64_t rt = row * tiles + t;
    for (int i = lane; i <= Na; i += 64) ae[i] = aedges[row * aedges_stride + i];
    for (int i = lane; i <= Nl; i += 64) le[i] = ledges[row * ledges_stride + i];
    const double ext0 = s + kTfeTile < n ? (double)x[s + kTfeTile] : 0.0;
    const WaveFwd F = fwd[rt];
    const WaveBwd B = bwd[rt];
    double xr[kInstSteps], xn[kInstSteps];
    unsigned long long cm[kInstSteps];
    int before[kInstSteps];
    const int c = inst_load_tile<Tin>(x, n, s, lane, ext0, xr, xn, cm, before);
    wave_tile_segments<false>(L, lane, s, n, c, xr, cm, before, F, B);                 // (its barrier also stands behind the stores above)
    // the peaks of the two half waves that are not the tile's own, from the carries (as wave_tile_segments<true> would leave them)
    const WavePair pf = {F.m, F.i}, pb = {B.m, B.i};
    const int32_t pk_first = c == 0 ? wave_pick(pf, pb).i : F.i, pk_last = B.i;
    count = count ? count + row * hist_stride : nullptr;
    samples = samples ? samples + row * hist_stride : nullptr;
    outside = outside ? outside + row * T : nullptr;
    const int64_t tb = s / hop;                                     // the time bin of every peak inside this tile
    // 1. the cell of every half wave that ends here: 0 .. c-1, and c in the row's last tile.  The two that are not the tile's own
    //    go to their time bin at once; one of the tile's own leaves cell << 10 | length (or -1: outside) in the place of its first
    //    edge — an entry that only its own lane still needs (its neighbour below has read it as its last edge in the same step)
    const int ends = c + (t == tiles - 1 ? 1 : 0);
    int out_here = 0;
    for (int r0 = 0; r0 < ends; r0 += 64) {
        const int r = r0 + lane;
        const bool have = r < ends;
        const int rr = have ? r : 0;
        const int32_t len = L.edge[rr + 1] - L.edge[rr];
        const int32_t pk = r == 0 ? pk_first : pk_last;              // (used for r = 0 and r = c alone)
        int pa, pl;
        wave_hist_search(ae, Na, __builtin_bit_cast(double, L.mag[rr]), le, Nl, (double)len, pa, pl);
        const bool inside = pa >= 1 && pa <= Na && pl >= 1 && pl <= Nl;
        const int cell = (pa - 1) * Nl + (pl - 1);
        const bool own = have && r >= 1 && r < c;                   // begins and ends in the tile: the tile's time bin
        out_here += __popcll(__ballot(own && !inside));
        if (have && !own) {
            // the half wave from the left, or the row's last one: its own time bin (a finite row's peak lies inside the row)
            const int64_t tk = (int64_t)pk / hop;
            if (pk >= 0 && tk < T) {
                if (inside) {
                    if (count) atomicAdd(&count[tk * cells + cell], 1);
                    if (samples) atomicAdd(&samples[tk * cells + cell], len);
                } else if (outside) {
                    atomicAdd(&outside[tk], 1);
                }
            }
        }
        if (have) L.edge[rr] = own && inside ? (cell << 10) | len : -1;     // (an own half wave has at most 511 samples)
    }
    if (c < 2) return;                                              // no half wave of the tile's own
    __syncthreads();
    // 2. the tile's histogram where the maxima stood: count << 16 | samples per cell
    uint32_t *hist = reinterpret_cast<uint32_t *>(L.mag);
    for (int i = lane; i < cells; i += 64) hist[i] = 0u;
    __syncthreads();
    // 3. one integer atomic per half wave; the lane that finds a cell's word at zero hands the cell on
    for (int r = 1 + lane; r < c; r += 64) {
        const int32_t p = L.edge[r];
        if (p >= 0) L.edge[r] = atomicAdd(&hist[p >> 10], (1u << 16) | (uint32_t)(p & 1023)) == 0u ? (p >> 10) : -1;
    }
    __syncthreads();
    // 4. every touched cell once
    for (int r = 1 + lane; r < c; r += 64) {
        const int cell = L.edge[r];
        if (cell < 0) continue;
        const uint32_t v = hist[cell];
        if (count) atomicAdd(&count[tb * cells + cell], (int32_t)(v >> 16));
        if (samples) atomicAdd(&samples[tb * cells + cell], (int32_t)(v & 0xffffu));
    }
    if (outside && lane == 0 && out_here) atomicAdd(&outside[tb], out_here);
}

}  // namespace itd
