// itd_ring_plan.hpp — what the ring streams (wave filter, spectrum, instantaneous: itd_wave_stream.hpp, itd_spectrum_stream.hpp,
// itd_inst_stream.hpp) share that needs no HIP: the ring fields of a step's launch arguments, the window arithmetic that fills them,
// and the block counting of push and flush.  Plain C++, so that a host compiler can build it alone (tests/c_client/ring_plan_host.cpp).
//
// A stream holds blocks of L samples, a horizon of H samples and a reach of 0 (wave filter) or 1 (spectrum, instantaneous) samples
// beyond it; D = ceil((H + reach) / L) is its latency in blocks.  Block b is decided from the samples [b L - H, (b+1) L + H + reach)
// that exist; they lie in the blocks b - D .. b + D: a ring of R = 2 D + 1 blocks per row, block q in slot q % R.  Push p stores block
// p and (p >= D) emits block p - D; the flush steps emit the blocks still held, one per step.
#pragma once
#include <stdint.h>

namespace itd {

// what a block leaves behind when it arrives: cross = a crossing index among its samples 0 .. L-2 (their successors are the
// block's own; whether its last sample is one is known from the next block's first), mx = max |x| of the block as a bit pattern
struct WaveBlockRec {
    unsigned long long mx;
    int32_t cross, pad;
};
static_assert(sizeof(WaveBlockRec) == 16, "WaveBlockRec layout");

// The ring fields of one step's launch arguments: the first member of every ring kernel's argument struct (WaveStreamArgs,
// SpectrumStreamArgs, InstStreamArgs), its own fields behind it.
struct RingStepArgs {
    const double *in;              // this push's block of every row (in_stride apart); nullptr on a flush step
    int64_t in_stride;
    double *ring;                  // [rows][R][L]
    WaveBlockRec *rec;             // [rows][R]: the record of the block in every ring slot
    int64_t arr;                   // the absolute index of the arriving block's first sample
    int32_t *status;               // = 2: a pushed block held a NaN
    int64_t base;                  // the absolute index of window position 0: (b - D) L (negative in a stream's first D blocks)
    int32_t L, D, H;
    int32_t slot0;                 // the ring slot of window block 0: (b - D) mod R; window block k sits in slot (slot0 + k) % R
    int32_t store_slot;            // the ring slot the arriving block goes to (in != nullptr)
    int32_t emit;                  // 0: a push that only stores
    int32_t rd_lo, rd_hi;          // the readable range in window positions: max(D L - H, -base) .. min((D+1) L + H + reach, what exists)
    int32_t at_start, at_end;      // it begins at the stream's start; it ends at the flushed stream's end
};

// The block counting of one stream.  t: the blocks pushed; P: the blocks in all once flushing began (-1: pushing); sent: the blocks
// emitted, all since create / reset / the last flush's end.
struct RingCount {
    int64_t t, P, sent;
};
constexpr RingCount kRingCountFresh = {0, -1, 0};

inline int64_t ring_held(const RingCount &c) { return (c.P < 0 ? c.t : c.P) - c.sent; }
inline bool ring_flushing(const RingCount &c) { return c.P >= 0; }

// The plan of one step: the arriving block (stores: there is one; none on a flush step) goes into the ring, block b (b < 0: none)
// is emitted from the samples [b L - H, (b+1) L + H + reach) that exist.  Fills every field of `a` that is no pointer or stride.
inline void ring_plan(RingStepArgs &a, int64_t t, int64_t P, int64_t L, int64_t D, int64_t H, int64_t reach, int64_t b, bool stores)
{
    const int64_t R = 2 * D + 1;
    a.arr = t * L;
    a.L = (int32_t)L; a.D = (int32_t)D; a.H = (int32_t)H;
    a.store_slot = stores ? (int32_t)(t % R) : 0;
    a.emit = b >= 0 ? 1 : 0;
    a.base = 0;
    a.slot0 = a.rd_lo = a.rd_hi = a.at_start = a.at_end = 0;
    if (b < 0) return;
    const int64_t exists = (P < 0 ? t + 1 : P) * L;                       // (a push: the arriving block included)
    const int64_t lo = b * L - H > 0 ? b * L - H : 0, want = (b + 1) * L + H + reach, hi = want < exists ? want : exists;
    a.base = (b - D) * L;
    a.slot0 = (int32_t)((((b - D) % R) + R) % R);
    a.rd_lo = (int32_t)(lo - a.base);
    a.rd_hi = (int32_t)(hi - a.base);
    a.at_start = lo == 0 ? 1 : 0;
    a.at_end = P >= 0 && hi == exists ? 1 : 0;
}

// push p stores block p and (p >= D) emits block p - D; step(b) runs the launch (b < 0: it only stores) and returns 0 or an error,
// after which nothing has changed
template <typename Step>
int ring_push(RingCount &c, int64_t D, int32_t *emitted, Step step)
{
    const bool emits = c.t >= D;
    const int rc = step(emits ? c.t - D : -1);
    if (rc) return rc;
    ++c.t;
    if (emits) ++c.sent;
    if (emitted) *emitted = emits ? 1 : 0;
    return 0;
}

// one block per call: the next block still held.  step(b) as above; it sees the count with the stream's length fixed (P >= 0)
template <typename Step>
int ring_flush(RingCount &c, int32_t *emitted, Step step)
{
    if (emitted) *emitted = 0;
    if (c.P < 0 && c.t == 0) return 0;             // empty: nothing to run
    const bool begins = c.P < 0;                   // the first flush step: the stream's length is fixed from here on
    if (begins) c.P = c.t;
    const int rc = step(c.sent);
    if (rc) {                                      // nothing was emitted: the stream is as it was, pushes are still taken
        if (begins) c.P = -1;
        return rc;
    }
    if (emitted) *emitted = 1;
    if (++c.sent == c.P) c = kRingCountFresh;      // the last block: the stream starts afresh
    return 0;
}

}  // namespace itd
