// itd_tfe_batch.hpp — instantaneous amplitude, phase and frequency of MANY rows in one asynchronous call (the batched form of
// itd_tfe.hpp: the same definitions, the same phase expression (phase_in), bit-identical results on NaN-free rows).
//
// The single-row operator numbers a row's half waves globally: an ordered compaction of the zero crossings (whose count the
// host reads to size the amplitude table), a memset and one atomic max per (step, half wave).  Here nothing is numbered: the
// tile pipeline of itd_halfwave.hpp with the smallest records.  A half wave either begins and ends inside one 512-sample tile
// — its amplitude is then a segmented maximum of that tile alone — or it is the first or the last half wave of a tile, and
// those two amplitudes follow from three numbers per tile:
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
//                      Ahead / Atail, the amplitude of sample s + 512 (lane 63's successor) from Ahead[t+1]; one arcsine per
//                      sample, the neighbour's phase from the next lane; streamed stores, each element rounded once where the
//                      output is float32
// Traffic for float64 in and out: 8 + 8 B read and 24 B written per sample, and per tile 24 B of record and 16 B of Ahead / Atail
// written and read once or twice (about 0.2 B per sample).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itd_halfwave.hpp"

#pragma clang fp contract(off)

namespace itd {

struct InstRec {
    int32_t c;          // crossings whose index lies in the tile
    int32_t nan;        // the tile holds a NaN
    double head, tail;
};
static_assert(sizeof(InstRec) == 24, "InstRec layout");

__device__ __forceinline__ unsigned long long inst_umax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long inst_wave_max(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = inst_umax(v, __shfl_xor(v, d));
    return v;
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
    int fpos, lpos;
    tile_crossing_span(cm, fpos, lpos);
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

// halfwave_carry's policy: the state is in[] / out[] of a position; the forward pass leaves max(in, head) in Ahead, the backward
// pass completes Ahead and writes Atail.  The row's crossing total is a per-thread sum and one LDS atomic (sh: two words, zeroed
// by the kernel in front of the scan).
struct InstCarry {
    using Rec = InstRec;
    using Map = InstMap;
    using State = unsigned long long;
    const InstRec *rec;
    double *Ahead, *Atail;
    int32_t *info;          // the row's word (or NULL)
    int *sh;
    int cnt = 0, nan = 0;

    static __device__ __forceinline__ Map ident() { return {0, 0ull}; }
    static __device__ __forceinline__ Map then(Map f, Map g) { return {f.reset | g.reset, g.reset ? g.m : inst_umax(f.m, g.m)}; }
    static __device__ __forceinline__ State apply(Map f, State s) { return f.reset ? f.m : inst_umax(s, f.m); }
    static __device__ __forceinline__ Map up(Map v, int d) { return {__shfl_up(v.reset, d), __shfl_up(v.m, d)}; }
    __device__ __forceinline__ Rec load(int64_t t) const { return rec[t]; }
    // forward: a tile with crossings hands on its tail, one without joins its maximum (head); backward: the head either way
    __device__ __forceinline__ Map map(int dir, const Rec &r)
    {
        if (dir == 0) { cnt += r.c; nan |= r.nan; }
        return {r.c > 0 ? 1 : 0, __builtin_bit_cast(unsigned long long, (dir == 0 && r.c > 0) ? r.tail : r.head)};
    }
    __device__ __forceinline__ State start(int) const { return 0ull; }
    __device__ __forceinline__ void emit(int dir, int64_t t, const Rec &r, State v) const
    {
        if (dir == 0) {
            Ahead[t] = __builtin_bit_cast(double, inst_umax(v, __builtin_bit_cast(unsigned long long, r.head)));
        } else {
            if (r.c == 0) {
                const unsigned long long a = __builtin_bit_cast(unsigned long long, Ahead[t]);
                Ahead[t] = __builtin_bit_cast(double, inst_umax(a, v));
            }
            Atail[t] = __builtin_bit_cast(double, inst_umax(__builtin_bit_cast(unsigned long long, r.tail), v));
        }
    }
    __device__ __forceinline__ void pass_end(int, State) const {}
    __device__ __forceinline__ void report(int tid) const
    {
        if (!info) return;
        if (cnt) atomicAdd(&sh[0], cnt);
        if (nan) atomicOr(&sh[1], 1);
        __syncthreads();
        if (tid == 0) *info = sh[1] ? -1 - sh[0] : sh[0];
    }
};

// One workgroup per row: halfwave_carry over the row's records; also the row's crossing total / NaN flag (info).
template <int NT>
__global__ __launch_bounds__(NT) void k_inst_carry(const InstRec *__restrict__ rec, int64_t tiles, double *__restrict__ Ahead,
                                                   double *__restrict__ Atail, int32_t *__restrict__ info)
{
    __shared__ int sh[2];
    if (threadIdx.x == 0) { sh[0] = 0; sh[1] = 0; }     // (the scan's barriers stand between this and report's atomics)
    const int64_t row = blockIdx.x;
    InstCarry pol = {rec + row * tiles, Ahead + row * tiles, Atail + row * tiles, info ? info + row : nullptr, sh};
    halfwave_carry<NT>(pol, tiles);
}

// One tile's amplitudes, phases and frequencies, handed to a sink sample by sample: what k_inst_apply stores and what k_tfe_bin
// (itd_tfe_spectrum.hpp) bins, from the same expressions.  Called by the tile's wavefront (one wavefront per workgroup); seg:
// kTfeTile + 1 words of LDS; rt: the tile's index into Ahead / Atail (row * tiles + t).  The sink receives
//     sample(g, j, in, A, ph)    the lane's sample j = s + 64 g + lane (in: j < n): amplitude and phase
//     freq(g, j, write, f)       its frequency (asked for by want_f); write is false behind the row's end and for the lone sample
//                                of a row's last tile, whose frequency comes from the tile before:
//     last(A, f)                 sample n - 1 = s + 512, where that is the row's last: its amplitude and frequency (all lanes)
template <typename Tin, typename Sink>
__device__ __forceinline__ void inst_tile_eval(const Tin *__restrict__ x, int64_t n, int64_t s, int64_t rt, int lane,
                                               const double *__restrict__ Ahead, const double *__restrict__ Atail,
                                               unsigned long long *seg, bool want_f, Sink &sink)
{
    const double pi = 3.14159265358979323846;
    const bool has_ext = s + kTfeTile < n;              // sample s + 512 exists: the tile is not the row's last
    const double ext = (lane < 2 && s + kTfeTile + lane < n) ? (double)x[s + kTfeTile + lane] : 0.0;
    const double ext0 = __shfl(ext, 0), ext1 = __shfl(ext, 1);
    const double A_head = Ahead[rt], A_tail = Atail[rt];
    const double A_ext = has_ext ? Ahead[rt + 1] : 0.0;  // the half wave of sample s + 512 is the next tile's first
    double xr[kInstSteps], xn[kInstSteps];
    unsigned long long cm[kInstSteps];
    int before[kInstSteps];
    const int c = inst_load_tile<Tin>(x, n, s, lane, ext0, xr, xn, cm, before);
    tile_segment_max<false>(seg, nullptr, lane, s, n, c, xr, before);
    __syncthreads();
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
        sink.sample(g, j, in, A[g], ph[g]);
        if (want_f) {
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
            sink.freq(g, j, write, dp / (2.0 * pi));
        }
    }
    if (want_f && has_ext && s + kTfeTile == n - 1) {
        // sample s + 512 is the row's last: its backward difference is this tile's last forward one
        const double p_last = __shfl(ph[kInstSteps - 1], 63);
        double dp = ph_ext - p_last;
        if (dp < 0.0) dp += 2.0 * pi;
        sink.last(A_ext, dp / (2.0 * pi));
    }
}

// k_inst_apply's sink: streamed stores of the outputs asked for
template <typename Tout>
struct InstStore {
    Tout *amp_out, *phase_out, *freq_out;       // the row's outputs (or NULL)
    int64_t n;
    int lane;
    __device__ __forceinline__ void sample(int, int64_t j, bool in, double A, double ph) const
    {
        if (in && amp_out) inst_store<Tout>(amp_out, j, A);
        if (in && phase_out) inst_store<Tout>(phase_out, j, ph);
    }
    __device__ __forceinline__ void freq(int, int64_t j, bool write, double f) const
    {
        if (write) inst_store<Tout>(freq_out, j, f);
    }
    __device__ __forceinline__ void last(double, double f) const
    {
        if (lane == 0) inst_store<Tout>(freq_out, n - 1, f);
    }
};

template <typename Tin, typename Tout>
__global__ __launch_bounds__(64) void k_inst_apply(const Tin *__restrict__ rows, int64_t row_stride, int64_t n, int64_t tiles,
                                                   const double *__restrict__ Ahead, const double *__restrict__ Atail,
                                                   Tout *__restrict__ amp_out, Tout *__restrict__ phase_out,
                                                   Tout *__restrict__ freq_out, int64_t out_stride)
{
    __shared__ unsigned long long seg[kTfeTile + 1];   // max |x| of the tile's half waves, by their number inside the tile
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x, s = t * kTfeTile;
    const Tin *x = rows + (int64_t)blockIdx.y * row_stride;
    const int64_t o = (int64_t)blockIdx.y * out_stride;
    InstStore<Tout> sink = {amp_out ? amp_out + o : nullptr, phase_out ? phase_out + o : nullptr, freq_out ? freq_out + o : nullptr, n, lane};
    inst_tile_eval<Tin>(x, n, s, (int64_t)blockIdx.y * tiles + t, lane, Ahead, Atail, seg, freq_out != nullptr, sink);
}

}  // namespace itd
