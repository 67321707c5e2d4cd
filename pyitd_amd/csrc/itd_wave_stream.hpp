// itd_wave_stream.hpp — device side of the wave-filter stream (itd_wave_stream_* in include/pyitd_hip.h): the
// single-wave feature filter of itd_waves.hpp block by block, at a fixed latency, bit for bit the whole-row filter with len_hi
// capped at the horizon.
//
// A stream holds `rows` rows in lock step, blocks of L samples, a horizon of H samples, D = ceil(H / L).  Crossing indices, half
// waves, A_k and length_k are those of itd_halfwave.hpp / itd_waves.hpp on ABSOLUTE indices (tfe_crossing refuses index 0: it is
// handed the index counted from the stream's start, never a window's).  The output is
//     y[j] = x[j]  if the half wave k of sample j has length_k <= H and amp_lo <= A_k <= amp_hi and len_lo <= length_k <= len_hi
//            +0.0  otherwise
// i.e. itd_wave_filter_batch_* with len_hi replaced by min(len_hi, H): a half wave longer than the horizon is never kept — the
// price of a bounded latency.
//
// Locality.  Block b is decided from the samples [b L - H, (b+1) L + H) clipped to what exists (the READABLE range) and nothing
// else.  For a sample j of block b:
//   * no crossing index c with b L - H <= c < j: the half wave began at or before b L - H — it is longer than H (+0.0) — unless the
//     readable range begins at the stream's start: then it begins at 0;
//   * no crossing index c with j <= c and c + 1 < (b+1) L + H: it is longer than H (+0.0), unless the readable range ends at the
//     flushed stream's end: then it ends at the last sample.
// H <= D L, so the readable range lies in the blocks b - D .. b + D: a ring of R = 2 D + 1 blocks per row, block q in slot q % R.
// Push p stores block p and (p >= D) emits block p - D; the flush steps emit the blocks still held.
//
// One launch per step, one workgroup per row (k_wave_stream; steps 1 to 3 are device functions — WaveRing, wave_ring_store, and
// wave_ring_block over wave_ring_cut and wave_ring_search_left / _right — that k_spectrum_stream of itd_spectrum_stream.hpp and
// k_inst_stream of itd_inst_stream.hpp call too; the launch's ring fields, RingStepArgs, and the host's arithmetic for them are in
// itd_ring_plan.hpp):
//   1. the arriving block into the row's ring (a NaN in it: status = 2, a plain store); the launch itself reads the arriving block
//      from the caller's pointer, so no fence stands between the store and the searches;
//   2. the emitted block's samples in registers, their crossing flags as ballots and a prefix over them in LDS: every sample's
//      half-wave number r = 0 .. c inside the block; edge[r + 1] = the r-th crossing's position, mag[r] = max |x| of the block's
//      part of half wave r by one LDS atomic per sample (tile_segment_max's way, on the whole block);
//   3. to the left, chunk by chunk from the block's first sample down to the readable range's begin: the last crossing index and
//      max |x| behind it; to the right, chunk by chunk up to the readable range's end: the first crossing index and max |x| up to
//      it.  Both stop at the first chunk that holds a crossing: a push reads 8 (L + 2 H) B at the most, far less where the row
//      crosses zero often.  Where it does not — a half wave that spans many blocks — the searches first step over whole blocks:
//      every block left a 16-byte record when it arrived (WaveBlockRec: does a crossing index lie among its first L - 1 samples,
//      its max |x|), and a block that lies inside the readable range with its successor sample, holds no such crossing and has
//      none at its last sample either adds its maximum and is passed, 64 blocks per step; the samples are read from the first
//      block that cannot be passed on.  The same maxima and the same crossings, so the same bits: O(L + D) per push;
//   4. every half wave of the block decided, keep ? x : +0.0 stored.
// No atomics on global memory, no floating-point atomics, no workgroup waits for another, nothing read on the host.  Positions
// inside the ring window are int32 (R L < 2 H + 3 L <= 2^23 + 2^15; the searches look at most 64 blocks past it before they are
// refused: + 2^19), the window's absolute origin is int64 (a stream is unbounded).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "itd_halfwave.hpp"
#include "itd_ring_plan.hpp"

#pragma clang fp contract(off)

namespace itd {

constexpr int kWaveStreamSpt = 8;            // samples of the emitted block per thread
constexpr int kWaveStreamUnroll = 4;         // samples per thread and chunk of the outer searches
constexpr int kWaveStreamMaxBlock = 8192;    // = kResidentMax
constexpr int64_t kWaveStreamMaxHorizon = (int64_t)1 << 22;

struct WaveStreamArgs {
    RingStepArgs r;                // the ring's fields (itd_ring_plan.hpp)
    const double *bounds;          // (amp_lo, amp_hi, len_lo, len_hi) of row r at r bounds_stride
    int64_t bounds_stride;
    double *out;                   // the emitted block of row r at r out_stride (emit = 1)
    int64_t out_stride;
};

// dynamic LDS of a launch for blocks of L samples
inline size_t wave_stream_lds(int L)
{
    const size_t groups = (size_t)(L + 63) / 64;
    return (size_t)(L + 1) * sizeof(unsigned long long) + groups * sizeof(unsigned long long) + (size_t)(L + 2) * sizeof(int32_t) +
           groups * sizeof(int32_t) + 8 * sizeof(int32_t) + sizeof(unsigned long long);
}

// ---- what the stream kernels share (k_wave_stream here, k_spectrum_stream, k_inst_stream in their own headers): one row's ring as a launch
// sees it, the arriving block's record, and the two searches that pass whole blocks by their records ---------------------------------

// One row's ring window: window position w (0 <= w < R L) is the sample base + w of the stream; window block k sits in ring slot
// (slot0 + k) % R, but the arriving block (k = 2 D of a push), which is read from the caller's pointer.
struct WaveRing {
    const double *in;              // the arriving block of this row (nullptr on a flush step)
    double *ring;                  // [R][L]
    WaveBlockRec *rec;             // [R]
    int64_t base, n_abs;           // the absolute index of window position 0; of the readable range's end (a crossing index's successor lies inside it)
    int32_t L, D, R, slot0, rd_lo, rd_hi, lane;

    __device__ __forceinline__ double ld(int w) const
    {
        const int k = (int)((unsigned)w / (unsigned)L), s = w - k * L;
        if (in && k == 2 * D) return in[s];
        int slot = slot0 + k;
        if (slot >= R) slot -= R;
        return ring[(int64_t)slot * L + s];
    }
    // Window block k (never the arriving one) can be passed whole: no crossing index among its samples, its last one included
    // (whose successor, block k + 1's first sample, the caller has checked to be readable).  mx: its max |x|.
    __device__ __forceinline__ bool passable(int k, unsigned long long &mx) const
    {
        int slot = slot0 + k;
        if (slot >= R) slot -= R;
        const WaveBlockRec r = rec[slot];
        mx = r.mx;
        const int w = (k + 1) * L - 1;
        return r.cross == 0 && !tfe_crossing(base + w, n_abs, ld(w), ld(w + 1));
    }
    // the lanes' verdicts on 64 blocks in search order: how many can be passed before the first that cannot, their max |x| into m
    __device__ __forceinline__ int pass_blocks(bool ok, unsigned long long mx, unsigned long long &m) const
    {
        const unsigned long long no = ~__ballot(ok);
        const int f = no ? __builtin_ctzll(no) : 64;
        unsigned long long part = lane < f ? mx : 0ull;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) part = max(part, (unsigned long long)__shfl_xor(part, d));
        m = max(m, part);
        return f;
    }
};

// the ring of row `row` under a launch's ring fields
__device__ __forceinline__ WaveRing wave_ring_of(const RingStepArgs &a, int64_t row, int lane)
{
    const int R = 2 * a.D + 1;
    return {a.in ? a.in + row * a.in_stride : nullptr, a.ring + row * (int64_t)R * a.L, a.rec + row * (int64_t)R, a.base, a.base + a.rd_hi,
            a.L, a.D, R, a.slot0, a.rd_lo, a.rd_hi, lane};
}

// The arriving block (absolute index of its first sample: arr) into its slot, its record behind it; a NaN in it: *status = 2, a plain
// store.  amx (one word) and flag (one word): LDS.  Called by every thread of the row's workgroup; ends behind a barrier.
template <int TH>
__device__ __forceinline__ void wave_ring_store(const WaveRing &rg, int64_t arr, int store_slot, int32_t *status, unsigned long long *amx,
                                                int32_t *flag, int tid)
{
    const int L = rg.L, lane = rg.lane;
    const double *const in = rg.in;
    if (tid == 0) { *amx = 0ull; *flag = 0; }
    __syncthreads();
    double *dst = rg.ring + (int64_t)store_slot * L;
    bool nan = false, cross = false;
    unsigned long long mx = 0ull;
    for (int s = tid; s < L; s += TH) {
        const double v = in[s];
        nan |= v != v;
        dst[s] = v;
        mx = max(mx, inst_mag(v, true));
        if (s + 1 < L) cross |= tfe_crossing(arr + s, arr + L, v, in[s + 1]);
    }
    if (nan) *status = 2;                                                 // (every writer stores the same word)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (unsigned long long)__shfl_xor(mx, d));
    if (lane == 0 && mx) atomicMax(amx, mx);
    if (__any(cross) && lane == 0) *flag = 1;
    __syncthreads();
    if (tid == 0) rg.rec[store_slot] = {*amx, *flag, 0};
}

// To the left of the emitted block (window block D): the last crossing index in [rd_lo, D L) — found, INT32_MIN if none — and max |x|
// behind it (m).  Whole blocks are passed by their records first, every wavefront on its own (no barrier); then chunk by chunk, ending
// at the first chunk that holds a crossing.  slot: a word of LDS that holds INT32_MIN.
template <int TH, int U>
__device__ __forceinline__ void wave_ring_search_left(const WaveRing &rg, int32_t *slot, int tid, unsigned long long &m, int &found)
{
    const int L = rg.L, lane = rg.lane;
    m = 0ull;
    found = INT32_MIN;
    int k = rg.D - 1;
    for (int f = 64; f == 64;) {
        const int kk = k - lane;
        unsigned long long mx = 0ull;
        const bool ok = kk >= 0 && kk * L >= rg.rd_lo && rg.passable(kk, mx);
        f = rg.pass_blocks(ok, mx, m);
        k -= f;
    }
    for (int hi = (k + 1) * L; hi > rg.rd_lo && found == INT32_MIN; hi -= TH * U) {
        double v[U];
        int pos = INT32_MIN;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int w = hi - (u + 1) * TH + tid;
            const bool on = w >= rg.rd_lo;
            v[u] = on ? rg.ld(w) : 0.0;
            double nx = __shfl_down(v[u], 1);
            if (on && (lane == 63 || w + 1 >= hi - u * TH)) nx = rg.ld(w + 1);     // (w + 1 <= D L < rd_hi: it exists)
            if (on && tfe_crossing(rg.base + w, rg.n_abs, v[u], nx)) pos = max(pos, w);
        }
        if (pos != INT32_MIN) atomicMax(slot, pos);
        __syncthreads();
        found = *slot;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int w = hi - (u + 1) * TH + tid;
            if (w >= rg.rd_lo && w > found) m = max(m, inst_mag(v[u], true));
        }
        __syncthreads();                                                  // (nobody is a chunk ahead of a reader of *slot)
    }
}

// To the right: the first crossing index in [(D + 1) L, rd_hi - 1) — found, INT32_MAX if none — and max |x| up to it (m).  slot: a
// word of LDS that holds INT32_MAX.
template <int TH, int U>
__device__ __forceinline__ void wave_ring_search_right(const WaveRing &rg, int32_t *slot, int tid, unsigned long long &m, int &found)
{
    const int L = rg.L, lane = rg.lane;
    m = 0ull;
    found = INT32_MAX;
    int k = rg.D + 1;
    for (int f = 64; f == 64;) {
        const int kk = k + lane;
        unsigned long long mx = 0ull;
        const bool ok = (kk + 1) * L < rg.rd_hi && rg.passable(kk, mx);     // (block kk + 1's first sample is readable)
        f = rg.pass_blocks(ok, mx, m);
        k += f;
    }
    for (int lo = k * L; lo < rg.rd_hi && found == INT32_MAX; lo += TH * U) {
        double v[U];
        int pos = INT32_MAX;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int w = lo + u * TH + tid;
            const bool on = w < rg.rd_hi;
            v[u] = on ? rg.ld(w) : 0.0;
            double nx = __shfl_down(v[u], 1);
            if (on && lane == 63) nx = w + 1 < rg.rd_hi ? rg.ld(w + 1) : 0.0;
            if (on && tfe_crossing(rg.base + w, rg.n_abs, v[u], nx)) pos = min(pos, w);    // (w + 1 = rd_hi: refused by n_abs)
        }
        if (pos != INT32_MAX) atomicMin(slot, pos);
        __syncthreads();
        found = *slot;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int w = lo + u * TH + tid;
            if (w < rg.rd_hi && w <= found) m = max(m, inst_mag(v[u], true));
        }
        __syncthreads();
    }
}

// The emitted block (window block D, blk) cut at its crossings, called by every thread of the row's workgroup: the thread's samples
// xr (s = (jj W + wave) 64 + lane, 0.0 behind the block), their successors' difference where asked for (slope), their crossing flags
// cr and half-wave numbers seg = 0 .. c inside the block; in LDS edge[r + 1] = the r-th crossing's position, mag[r] = max |x| of the
// block's part of half wave r (one LDS atomic per sample), bal / pre: the flags' ballots and their prefix, *cnt = c.  The caller's
// searches complete mag[0], edge[0], mag[c] and edge[c + 1]; its barrier follows them.
template <int TH, bool kSlope>
__device__ __forceinline__ int wave_ring_cut(const WaveRing &rg, const double *blk, unsigned long long *mag, unsigned long long *bal,
                                             int32_t *edge, int32_t *pre, int32_t *cnt, int tid, int wave, double (&xr)[kWaveStreamSpt],
                                             double (&slope)[kWaveStreamSpt], bool (&cr)[kWaveStreamSpt], int (&seg)[kWaveStreamSpt])
{
    constexpr int SPT = kWaveStreamSpt, W = TH / 64;
    const int L = rg.L, lane = rg.lane, G = (L + 63) >> 6, b0 = rg.D * L;
#pragma unroll
    for (int jj = 0; jj < SPT; ++jj) {
        const int g = jj * W + wave, s = g * 64 + lane;                   // (g is the same for the whole wavefront)
        xr[jj] = 0.0;
        cr[jj] = false;
        if (kSlope) slope[jj] = 0.0;
        if (g < G) {
            double xn = 0.0;
            if (s < L) {
                xr[jj] = blk[s];
                if (s + 1 < L) xn = blk[s + 1];
                else if (b0 + L < rg.rd_hi) xn = rg.ld(b0 + L);
                cr[jj] = tfe_crossing(rg.base + b0 + s, rg.n_abs, xr[jj], xn);
                if (kSlope) slope[jj] = xn - xr[jj];
            }
            const unsigned long long m = __ballot(cr[jj]);
            if (lane == 0) bal[g] = m;
        }
    }
    __syncthreads();
    if (wave == 0) {                                                      // exclusive prefix of the groups' counts (G <= 128)
        const int p0 = lane < G ? __popcll(bal[lane]) : 0, p1 = lane + 64 < G ? __popcll(bal[lane + 64]) : 0;
        int i0 = p0, i1 = p1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o0 = __shfl_up(i0, d), o1 = __shfl_up(i1, d);
            if (lane >= d) { i0 += o0; i1 += o1; }
        }
        const int t0 = __shfl(i0, 63), t1 = __shfl(i1, 63);
        if (lane < G) pre[lane] = i0 - p0;
        if (lane + 64 < G) pre[lane + 64] = t0 + i1 - p1;
        if (lane == 0) *cnt = t0 + t1;
    }
    __syncthreads();
    const int c = *cnt;
#pragma unroll
    for (int jj = 0; jj < SPT; ++jj) {
        const int g = jj * W + wave, s = g * 64 + lane;
        seg[jj] = 0;
        if (g < G && s < L) {
            seg[jj] = pre[g] + __popcll(bal[g] & ((1ull << lane) - 1ull));
            atomicMax(&mag[seg[jj]], inst_mag(xr[jj], true));
            if (cr[jj]) edge[seg[jj] + 1] = s;                            // a crossing index is the last sample of its half wave
        }
    }
    return c;
}

// The cut's arrays in LDS, wave_stream_lds(L) bytes from `base` on (8-byte aligned).  ctl: [0] c, [1] the left search's crossing,
// [2] the right search's, [3] the arriving block's flag, [4 .. 7] the caller's.
struct WaveCutLds {
    unsigned long long *mag, *bal, *amx;         // [L + 1]; [G]; [1] the arriving block's max |x|
    int32_t *edge, *pre, *ctl;                   // [L + 2], positions relative to the block; [G]; [8]
};
__device__ __forceinline__ WaveCutLds wave_cut_lds(unsigned char *base, int L)
{
    const int G = (L + 63) >> 6;                                          // 64-sample groups of the block
    WaveCutLds q;
    q.mag = reinterpret_cast<unsigned long long *>(base);
    q.bal = q.mag + (L + 1);
    q.amx = q.bal + G;
    q.edge = reinterpret_cast<int32_t *>(q.amx + 1);
    q.pre = q.edge + (L + 2);
    q.ctl = q.pre + G;
    return q;
}

// Steps 2 and 3 of an emitting launch, called by every thread of the row's workgroup behind step 1: the emitted block (window block
// D, blk) cut at its crossings (wave_ring_cut: xr, slope, cr, seg and the LDS arrays), then the outer searches, chunk by chunk, each
// ending at the first chunk that holds a crossing, which complete mag[0], edge[0], mag[c] and edge[c + 1].  Returns c behind a barrier.
template <int TH, bool kSlope>
__device__ __forceinline__ int wave_ring_block(const WaveRing &rg, const RingStepArgs &a, const WaveCutLds &q, const double *blk, int tid,
                                               int wave, double (&xr)[kWaveStreamSpt], double (&slope)[kWaveStreamSpt],
                                               bool (&cr)[kWaveStreamSpt], int (&seg)[kWaveStreamSpt])
{
    constexpr int U = kWaveStreamUnroll;
    const int L = a.L, H = a.H, b0 = a.D * L;                             // b0: the emitted block's first window position
    for (int i = tid; i <= L; i += TH) q.mag[i] = 0ull;
    if (tid == 0) { q.ctl[1] = INT32_MIN; q.ctl[2] = INT32_MAX; }
    const int c = wave_ring_cut<TH, kSlope>(rg, blk, q.mag, q.bal, q.edge, q.pre, &q.ctl[0], tid, wave, xr, slope, cr, seg);
    {
        unsigned long long m;
        int found;
        wave_ring_search_left<TH, U>(rg, &q.ctl[1], tid, m, found);
        if (m) atomicMax(&q.mag[0], m);
        // half wave 0 begins behind the crossing; without one at the stream's start (if the range reaches it), else out of reach
        if (tid == 0) q.edge[0] = found != INT32_MIN ? found - b0 : (a.at_start ? a.rd_lo - 1 - b0 : -H - 2);
    }
    {
        unsigned long long m;
        int found;
        wave_ring_search_right<TH, U>(rg, &q.ctl[2], tid, m, found);
        if (m) atomicMax(&q.mag[c], m);
        // half wave c ends at the crossing; without one at the flushed stream's last sample (if the range reaches it), else out of reach
        if (tid == 0) q.edge[c + 1] = found != INT32_MAX ? found - b0 : (a.at_end ? a.rd_hi - 1 - b0 : L + H + 2);
    }
    __syncthreads();
    return c;
}

template <int TH>
__global__ __launch_bounds__(TH) void k_wave_stream(WaveStreamArgs a)
{
    constexpr int SPT = kWaveStreamSpt, W = TH / 64;
    static_assert(TH % 64 == 0 && TH * SPT >= 64, "geometry");
    extern __shared__ __attribute__((aligned(16))) unsigned char ws_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = a.r.L, D = a.r.D, H = a.r.H;
    const int G = (L + 63) >> 6;                                          // 64-sample groups of the block
    const WaveCutLds q = wave_cut_lds(ws_lds, L);
    unsigned long long *const mag = q.mag;
    int32_t *const edge = q.edge;
    const int64_t row = blockIdx.x;
    const WaveRing rg = wave_ring_of(a.r, row, lane);

    // 1. the arriving block into its slot, its record behind it
    if (rg.in) wave_ring_store<TH>(rg, a.r.arr, a.r.store_slot, a.r.status, q.amx, &q.ctl[3], tid);
    if (!a.r.emit) return;

    // 2., 3. the block: samples, flags, half-wave numbers, inner maxima; the outer searches
    const double *const blk = rg.ring + (int64_t)((a.r.slot0 + D) % rg.R) * L;    // (window block D: never the arriving one, D >= 1)
    double xr[SPT], unused[SPT];
    bool cr[SPT];
    int seg[SPT];
    wave_ring_block<TH, false>(rg, a.r, q, blk, tid, wave, xr, unused, cr, seg);

    // 4. every half wave of the block decided
    const double *bnd = a.bounds + row * a.bounds_stride;
    const double amp_lo = bnd[0], amp_hi = bnd[1], len_lo = bnd[2], len_hi = bnd[3];
    double *const out = a.out + row * a.out_stride;
#pragma unroll
    for (int jj = 0; jj < SPT; ++jj) {
        const int g = jj * W + wave, s = g * 64 + lane;
        if (g < G && s < L) {
            const int r = seg[jj];
            const double A = __builtin_bit_cast(double, mag[r]);
            const int32_t n = edge[r + 1] - edge[r];
            const double len = (double)n;
            const bool keep = n <= H && amp_lo <= A && A <= amp_hi && len_lo <= len && len <= len_hi;
            out[s] = keep ? xr[jj] : 0.0;
        }
    }
}

}  // namespace itd
