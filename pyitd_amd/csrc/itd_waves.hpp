// itd_waves.hpp — single-wave analysis of MANY rows in one asynchronous call: the table of a row's half waves (start, length, peak,
// signed extremum) and the row filtered by its half waves' amplitude and length.  The tile pipeline of itd_halfwave.hpp with records
// that hold, beyond "the maximum of a half wave" (itd_tfe_batch.hpp), where it first occurs, where the half wave begins and ends.
//
// A half wave is the run of samples between two crossing indices (tfe_crossing): half wave k holds start_k .. end_k with
// start_0 = 0, start_k = c_{k-1} + 1, end_k = c_k, end_m = n - 1.  A_k = max |x| over it, peak_k the smallest index that attains
// A_k, value_k = x[peak_k].  Every result is an integer, a copy of an input sample or a zero.
//
// A maximum with its first position is a pair (m, i) — m the magnitude as a bit pattern, i the absolute index — under
//     wave_pick(a, b) = the one with the larger m; on equal m the one with the smaller i
// That is the maximum of a total order (m ascending, then i descending): associative, commutative, identity (0, INT32_MAX).  The
// earlier index wins a tie whichever operand holds it: the left one in the forward pass, the right one in the backward pass.
//
// One record per 512-sample tile (WaveRec): c, the NaN flag, the pair of the tile's head (the samples up to and including its
// first crossing index, the whole tile if c == 0), the pair of its tail (the samples behind its last crossing index; the identity
// if there are none or c == 0) and the first and the last crossing index.  A scan along the row, one workgroup per row:
//     forward   in[0]  = ((0, MAX), start 0, prefix 0)
//               in[t+1] = c[t] > 0 ? (tail[t], last[t] + 1, prefix + c[t]) : (pick(in[t], head[t]), start, prefix)
//               Fwd[t] = (pick(in[t], head[t]), start, prefix)      the half wave that reaches tile t from the left, with the
//                                                                   tile's head; prefix = the tile's first half-wave number
//     backward  out[last] = ((0, MAX), end n - 1)
//               out[t-1] = c[t] > 0 ? (head[t], first[t]) : (pick(head[t], out[t]), end)
//               Bwd[t] = (pick(tail[t], out[t]), end)               the half wave that leaves tile t to the right, with its tail
// The tile's first half wave is (Fwd.pair, Fwd.start, first) if c > 0 and (pick(Fwd.pair, Bwd.pair), Fwd.start, Bwd.end) if not;
// its last one (c > 0) is (Bwd.pair, last + 1, Bwd.end); half waves 1 .. c-1 begin and end inside the tile.
// Launches per chunk of rows, grid = (tiles, rows), one wavefront per tile for the passes over the samples:
//     k_wave_records   reads the row, writes one record per tile                                              40 B per tile
//     k_wave_carry     the two scans, one workgroup per row; also the row's count and info                    24 + 16 B per tile
//     k_wave_table     every tile writes the half waves that END in it (the row's last tile the row's last one) at prefix + rank
//     k_wave_filter    reads the row again, stores keep ? x : +0.0 (streamed; rounded once where the output is float32)
// Traffic of the filter for float64 in and out: 8 + 8 B read and 8 B written per sample, 80 B per tile written and
// read (0.3 B per sample).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itd_halfwave.hpp"

#pragma clang fp contract(off)

namespace itd {

struct WavePair {
    unsigned long long m;   // |x| as a bit pattern
    int32_t i;              // the absolute index of its first occurrence
};
__device__ __forceinline__ WavePair wave_pick(WavePair a, WavePair b)
{
    return (a.m > b.m || (a.m == b.m && a.i <= b.i)) ? a : b;
}

struct WaveRec {
    unsigned long long hm, tm;  // head / tail magnitude
    int32_t c, nan;
    int32_t hi, ti;             // head / tail first-maximum index (tail: kWaveNone if empty)
    int32_t first, last;        // first / last crossing index of the tile (c > 0)
};
static_assert(sizeof(WaveRec) == 40, "WaveRec layout");
struct WaveFwd {
    unsigned long long m;
    int32_t i, start, prefix, pad;
};
static_assert(sizeof(WaveFwd) == 24, "WaveFwd layout");
struct WaveBwd {
    unsigned long long m;
    int32_t i, end;
};
static_assert(sizeof(WaveBwd) == 16, "WaveBwd layout");

__device__ __forceinline__ WavePair wave_reduce(WavePair v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        WavePair o;
        o.m = __shfl_xor(v.m, d);
        o.i = __shfl_xor(v.i, d);
        v = wave_pick(v, o);
    }
    return v;
}

template <typename Tin>
__global__ __launch_bounds__(64) void k_wave_records(const Tin *__restrict__ rows, int64_t row_stride, int64_t n, int64_t tiles,
                                                     WaveRec *__restrict__ rec)
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
    WavePair hv = {0ull, kWaveNone}, tv = {0ull, kWaveNone};
    bool nan = false;
#pragma unroll
    for (int g = 0; g < kInstSteps; ++g) {          // positions ascend with g: a strict comparison keeps the lane's earliest
        const int p = g * 64 + lane;
        const bool in = s + p < n;
        const WavePair v = {inst_mag(xr[g], in), in ? (int32_t)(s + p) : kWaveNone};
        nan |= in && xr[g] != xr[g];
        if (p <= fpos) hv = wave_pick(hv, v);
        if (p > lpos) tv = wave_pick(tv, v);
    }
    hv = wave_reduce(hv);
    tv = wave_reduce(tv);
    const bool any_nan = __ballot(nan) != 0ull;
    if (lane == 0) {
        WaveRec r;
        r.hm = hv.m; r.tm = tv.m;
        r.c = c;
        r.nan = any_nan ? 1 : 0;
        r.hi = hv.i; r.ti = tv.i;
        r.first = (int32_t)(s + fpos); r.last = (int32_t)(s + lpos);
        rec[(int64_t)blockIdx.y * tiles + t] = r;
    }
}

// An element of the scan: the map on a state (pair, pos, cnt)
//     reset ? (p, pos, s.cnt + cnt) : (pick(s.pair, p), s.pos, s.cnt + cnt)
// — InstMap with the position of the maximum, the half wave's own begin (forward) or end (backward) and the crossing count riding
// along.  then(f, g) is "f, then g".  It is associative with the identity {0, (0, MAX), 0, 0}: pick is the maximum of a total
// order (associative, commutative, (0, MAX) its least element), a reset on the right discards what is on its left, pos follows
// the last reset (a map without one carries pos = 0 and never uses it) and cnt is a plain sum.
struct WaveMap {
    int reset;
    WavePair p;
    int32_t pos, cnt;
};
struct WaveState {
    WavePair p;
    int32_t pos, cnt;
};

// halfwave_carry's policy: the forward pass writes Fwd, the backward pass Bwd (neither reads the other's); the row's crossing
// total rides in the map and is what the forward pass ends with.
struct WaveCarry {
    using Rec = WaveRec;
    using Map = WaveMap;
    using State = WaveState;
    const WaveRec *rec;
    WaveFwd *fwd;
    WaveBwd *bwd;
    int32_t n;
    int32_t *count, *info;  // the row's words (or NULL)
    int *sh_nan;            // one word, zeroed by the kernel in front of the scan
    int nan = 0;
    int32_t total = 0;      // the row's crossings (every thread holds it after the forward pass)

    static __device__ __forceinline__ Map ident() { return {0, {0ull, kWaveNone}, 0, 0}; }
    static __device__ __forceinline__ Map then(Map f, Map g)
    {
        return {f.reset | g.reset, g.reset ? g.p : wave_pick(f.p, g.p), g.reset ? g.pos : f.pos, f.cnt + g.cnt};
    }
    static __device__ __forceinline__ State apply(Map f, State s)
    {
        return {f.reset ? f.p : wave_pick(s.p, f.p), f.reset ? f.pos : s.pos, s.cnt + f.cnt};
    }
    static __device__ __forceinline__ Map up(Map v, int d)
    {
        return {__shfl_up(v.reset, d), {__shfl_up(v.p.m, d), __shfl_up(v.p.i, d)}, __shfl_up(v.pos, d), __shfl_up(v.cnt, d)};
    }
    __device__ __forceinline__ Rec load(int64_t t) const { return rec[t]; }
    // forward: a tile with crossings hands on its tail and where it begins, one without joins its head; backward: the head
    // either way, and with crossings where the half wave ends
    __device__ __forceinline__ Map map(int dir, const Rec &r)
    {
        const bool cut = r.c > 0;
        if (dir == 0) {
            nan |= r.nan;
            return {cut ? 1 : 0, {cut ? r.tm : r.hm, cut ? r.ti : r.hi}, cut ? r.last + 1 : 0, r.c};
        }
        return {cut ? 1 : 0, {r.hm, r.hi}, cut ? r.first : 0, 0};
    }
    __device__ __forceinline__ State start(int dir) const { return {{0ull, kWaveNone}, dir ? n - 1 : 0, 0}; }
    __device__ __forceinline__ void emit(int dir, int64_t t, const Rec &r, State v) const
    {
        if (dir == 0) {
            const WavePair a = wave_pick(v.p, WavePair{r.hm, r.hi});
            fwd[t] = {a.m, a.i, v.pos, v.cnt, 0};
        } else {
            const WavePair a = wave_pick(WavePair{r.tm, r.ti}, v.p);
            bwd[t] = {a.m, a.i, v.pos};
        }
    }
    __device__ __forceinline__ void pass_end(int dir, State run)
    {
        if (dir == 0) total = run.cnt;
    }
    __device__ __forceinline__ void report(int tid) const
    {
        if (nan) atomicOr(sh_nan, 1);
        __syncthreads();
        if (tid == 0) {
            if (count) *count = total + 1;
            if (info) *info = *sh_nan ? -1 - total : total;
        }
    }
};

// One workgroup per row: halfwave_carry over the row's records; also the row's count and info.
template <int NT>
__global__ __launch_bounds__(NT) void k_wave_carry(const WaveRec *__restrict__ rec, int64_t tiles, int64_t n, WaveFwd *__restrict__ fwd,
                                                   WaveBwd *__restrict__ bwd, int32_t *__restrict__ count, int32_t *__restrict__ info)
{
    __shared__ int sh_nan;
    if (threadIdx.x == 0) sh_nan = 0;                   // (the scan's barriers stand between this and report's atomic)
    const int64_t row = blockIdx.x;
    WaveCarry pol = {rec + row * tiles, fwd + row * tiles, bwd + row * tiles, (int32_t)n, count ? count + row : nullptr,
                     info ? info + row : nullptr, &sh_nan};
    halfwave_carry<NT>(pol, tiles);
}

// What the table and the filter need of a tile's half waves, by their number r = 0 .. c inside the tile, in LDS:
//     edge[r]      the index in front of half wave r's first sample (start_r - 1): edge[r + 1] is its last sample
//     mag[r]       A_r as a bit pattern
//     peak[r]      peak_r (kPeak)
// Half waves 1 .. c-1 from the tile's own flags and samples (one LDS atomic per sample, as in k_inst_apply; the first position by
// a second round among the samples that attain the maximum), half waves 0 and c from the carries.
template <bool kPeak>
struct WaveTileLds {
    unsigned long long mag[kTfeTile + 1];
    int32_t edge[kTfeTile + 2];
    int32_t peak[kPeak ? kTfeTile + 1 : 1];
};

template <bool kPeak>
__device__ __forceinline__ void wave_tile_segments(WaveTileLds<kPeak> &L, int lane, int64_t s, int64_t n, int c, const double (&xr)[kInstSteps],
                                                   const unsigned long long (&cm)[kInstSteps], const int (&before)[kInstSteps],
                                                   const WaveFwd F, const WaveBwd B)
{
    tile_segment_max<kPeak>(L.mag, L.peak, lane, s, n, c, xr, before);
    // a crossing index is the last sample of the half wave it belongs to
#pragma unroll
    for (int g = 0; g < kInstSteps; ++g)
        if ((cm[g] >> lane) & 1ull) L.edge[before[g] + 1] = (int32_t)(s + g * 64 + lane);
    if (lane == 0) {
        const WavePair f = {F.m, F.i}, b = {B.m, B.i};
        const WavePair head = c == 0 ? wave_pick(f, b) : f;
        L.edge[0] = F.start - 1;
        L.edge[c + 1] = B.end;
        L.mag[0] = head.m;
        if (kPeak) L.peak[0] = head.i;
        if (c > 0) {
            L.mag[c] = B.m;
            if (kPeak) L.peak[c] = B.i;
        }
    }
    __syncthreads();
}

template <typename Tin>
__global__ __launch_bounds__(64) void k_wave_table(const Tin *__restrict__ rows, int64_t row_stride, int64_t n, int64_t tiles,
                                                   const WaveFwd *__restrict__ fwd, const WaveBwd *__restrict__ bwd,
                                                   int32_t *__restrict__ start_out, int32_t *__restrict__ length_out,
                                                   int32_t *__restrict__ peak_out, double *__restrict__ value_out, int64_t wave_stride,
                                                   int32_t cap)
{
    __shared__ WaveTileLds<true> L;
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x, s = t * kTfeTile;
    const Tin *x = rows + (int64_t)blockIdx.y * row_stride;
    const int64_t o = (int64_t)blockIdx.y * wave_stride;
    const int64_t rt = (int64_t)blockIdx.y * tiles + t;
    const double ext0 = s + kTfeTile < n ? (double)x[s + kTfeTile] : 0.0;
    const WaveFwd F = fwd[rt];
    const WaveBwd B = bwd[rt];
    double xr[kInstSteps], xn[kInstSteps];
    unsigned long long cm[kInstSteps];
    int before[kInstSteps];
    const int c = inst_load_tile<Tin>(x, n, s, lane, ext0, xr, xn, cm, before);
    wave_tile_segments<true>(L, lane, s, n, c, xr, cm, before, F, B);
    auto emit = [&](int r) {
        const int64_t k = (int64_t)F.prefix + r;
        if (k >= cap) return;
        const int32_t st = L.edge[r] + 1, en = L.edge[r + 1], pk = L.peak[r];
        if (start_out) start_out[o + k] = st;
        if (length_out) length_out[o + k] = en - st + 1;
        if (peak_out) peak_out[o + k] = pk;
        if (value_out) value_out[o + k] = (pk >= 0 && pk < n) ? (double)x[pk] : 0.0;    // (always inside the row)
    };
#pragma unroll
    for (int g = 0; g < kInstSteps; ++g)
        if ((cm[g] >> lane) & 1ull) emit(before[g]);
    if (lane == 0 && t == tiles - 1) emit(c);           // the row's last half wave ends with the row
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(64) void k_wave_filter(const Tin *__restrict__ rows, int64_t row_stride, int64_t n, int64_t tiles,
                                                    const WaveFwd *__restrict__ fwd, const WaveBwd *__restrict__ bwd,
                                                    const double *__restrict__ bounds, int64_t bounds_stride, Tout *__restrict__ out,
                                                    int64_t out_stride)
{
    __shared__ WaveTileLds<false> L;
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x, s = t * kTfeTile;
    const Tin *x = rows + (int64_t)blockIdx.y * row_stride;
    out += (int64_t)blockIdx.y * out_stride;
    const int64_t rt = (int64_t)blockIdx.y * tiles + t;
    const double ext0 = s + kTfeTile < n ? (double)x[s + kTfeTile] : 0.0;
    const double bnd = lane < 4 ? bounds[(int64_t)blockIdx.y * bounds_stride + lane] : 0.0;      // once per wavefront
    const double amp_lo = __shfl(bnd, 0), amp_hi = __shfl(bnd, 1), len_lo = __shfl(bnd, 2), len_hi = __shfl(bnd, 3);
    const WaveFwd F = fwd[rt];
    const WaveBwd B = bwd[rt];
    double xr[kInstSteps], xn[kInstSteps];
    unsigned long long cm[kInstSteps];
    int before[kInstSteps];
    const int c = inst_load_tile<Tin>(x, n, s, lane, ext0, xr, xn, cm, before);
    wave_tile_segments<false>(L, lane, s, n, c, xr, cm, before, F, B);
#pragma unroll
    for (int g = 0; g < kInstSteps; ++g) {
        const int64_t j = s + g * 64 + lane;
        const int r = before[g];
        const double A = __builtin_bit_cast(double, L.mag[r]);
        const double len = (double)(L.edge[r + 1] - L.edge[r]);
        const bool keep = amp_lo <= A && A <= amp_hi && len_lo <= len && len <= len_hi;
        if (j < n) inst_store<Tout>(out, j, keep ? xr[g] : 0.0);
    }
}

}  // namespace itd
