// itd_policy.hpp — which form a decomposition takes and what the engine learns when a form falls short (DESIGN.md sections 10, 11,
// 13), and which form a spline extraction takes (section 9).  Plain C++17: itd_engine.hip holds one FormPolicy,
// tests/test_policy_host.py drives one on the host.
#pragma once

#include <algorithm>
#include <cstdint>

#include "../../include/pyitd_hip.h"

struct FormPolicy {
    static constexpr int32_t kBackOff = 16, kBackOffMax = 1024;   // calls in a plainer form after a fail; a refused probe doubles a span
    static int32_t doubled(int32_t span) { return std::min(span * 2, kBackOffMax); }
    static constexpr int kRangeTiles = 64, kRangeMinTiles = 16;   // tiles per knot-side workgroup (itd_knotfirst.hpp's kKcTiles)
    static constexpr int kFailCapacity = 2, kFailWait = 16;        // KfSig::fail bits (itd_knotfirst.hpp)
    static constexpr int64_t kFusedMinN = 65536;                   // automatic: shorter signals never run the fused sparse levels

    // ---- modes and overrides: what the itd_set_* of the same names set ----
    int32_t resident_mode = ITD_RESIDENT_AUTO, l0_mode = ITD_LEVEL0_AUTO, fuse_mode = ITD_FUSE_AUTO;
    int32_t fuse_level = 0, fuse_range = 0;   // first fused level, tiles per knot-side workgroup (0: automatic)
    int32_t fuse_cap = 0;                     // the first level NOT fused (0: whatever was learned; -1: never)
    int64_t fuse_min_samples = (int64_t)2 << 20;   // samples per launch sequence from which the fused form pays
    // ---- learned state ----
    int32_t resident_off_left = 0;      // calls still to skip the resident form (a resident call met a non-finite value)
    int32_t l0_records_left = 0;        // calls still to run level 0 record-driven (a fused level-0 launch fell short)
    int32_t fuse_off_left = 0;          // calls still to run level by level (the fused levels refused a whole call): a pause
    int32_t fuse_off_span = kBackOff;   // ... the next pause: doubled by a refused probe, reset by a delivered call
    bool fuse_probe = false;            // the next fused call is the first attempt after a pause
    int32_t fuse_cap_auto = 0;          // learned cap: the lowest KfSig::fail_lev of a refusal (0: none)
    int32_t fuse_cap_calls = 0;         // delivered calls under it since it was learned ...
    int32_t fuse_cap_span = kBackOff;   // ... after this many the next call tries all levels (a probe)
    bool kf_force_tickets = false;      // a halo wait was given up: workgroup ids are tickets from then on
    bool fuse_level2_off = false;       // a level-2 list outgrew its workgroup: automatic first fused level 3 from then on
    int32_t kf_shrink = 0;              // automatic range: halved this many times
    bool fuse_no_memory = false;        // no fused levels' workspace: level by level from then on
    // ---- counters: what the itd_get_* of the same names report ----
    int32_t resident_repeats = 0, fuse_repeats = 0;
    int64_t fuse_signal_repairs = 0, device_repairs = 0;

    // ---- setters: each clears the learned state that belongs to what it sets ----
    void set_resident_mode(int32_t m) { resident_mode = m; resident_off_left = 0; }
    void set_level0_mode(int32_t m) { l0_mode = m; l0_records_left = 0; }
    void set_fuse_mode(int32_t m) { fuse_mode = m; fuse_off_left = 0; fuse_off_span = kBackOff; fuse_probe = false; }
    void set_fuse_level(int32_t level) { fuse_level = level; fuse_level2_off = false; }
    void set_fuse_range(int32_t tiles) { fuse_range = tiles; kf_shrink = 0; }
    void set_fuse_cap(int32_t level) { fuse_cap = level; fuse_cap_auto = 0; fuse_cap_calls = 0; fuse_cap_span = kBackOff; }
    void set_fuse_min_samples(int64_t samples) { fuse_min_samples = samples; }

    // ---- decisions for the call being enqueued (those that are not const count a pause down) ----
    // resident form?  `fits`: n <= kResidentMax; a level-0 mode or launch timing means level by level
    bool resident(bool fits, bool timing)
    {
        if (!fits || resident_mode == ITD_RESIDENT_OFF) return false;
        if (resident_mode == ITD_RESIDENT_ONLY) return true;
        if (l0_mode != ITD_LEVEL0_AUTO || timing) return false;
        if (resident_off_left > 0) { --resident_off_left; return false; }
        return true;
    }
    void resident_unavailable() { resident_mode = ITD_RESIDENT_OFF; }   // (the runtime refused the resident kernel its LDS)
    bool level0_fused()   // else record-driven
    {
        if (l0_mode != ITD_LEVEL0_AUTO) return l0_mode == ITD_LEVEL0_FUSED;
        if (l0_records_left > 0) { --l0_records_left; return false; }
        return true;
    }
    // fused sparse levels?  `seq`: samples per launch sequence.  The call that ends a pause runs level by level, the next one probes.
    bool fused_levels(int64_t n, int64_t seq, int32_t M, bool fuse0)
    {
        if (fuse_mode == ITD_FUSE_OFF || !fuse0 || M < 2 || (fuse_level && fuse_level > M)) return false;
        if (fuse_mode == ITD_FUSE_ONLY) return true;
        if (n < kFusedMinN || l0_mode != ITD_LEVEL0_AUTO || fuse_no_memory || seq < fuse_min_samples) return false;
        if (fuse_off_left > 0) { if (--fuse_off_left == 0) fuse_probe = true; return false; }
        return true;
    }
    int first_level(int64_t seq, int32_t M) const   // automatic: 2 from 2^22 samples per sequence, else 3 (2 if M is below that)
    {
        if (fuse_level) return fuse_level;
        const int L0 = (seq >= ((int64_t)1 << 22) && !fuse_level2_off) ? 2 : 3;
        return L0 > M ? 2 : L0;
    }
    int tiles_per_wg() const { return fuse_range ? fuse_range : std::max(kRangeMinTiles, kRangeTiles >> kf_shrink); }
    // levels cap .. M + 1 one launch each behind the fused ones (0: none); a learned cap is left off now and then (a probe)
    int cap(int L0, int32_t M) const
    {
        int c = fuse_cap ? fuse_cap : fuse_cap_auto;            // (fuse_cap -1 = never: falls out below)
        if (c > 0 && !fuse_cap && fuse_cap_calls >= fuse_cap_span) c = 0;
        return (c < L0 + 2 || c > M + 1) ? 0 : c;               // (two fused levels at least, within the call's)
    }
    // `wgs`: the knot side's workgroups over every stream in flight; blockIdx only where all of them are resident at once
    bool tickets(int64_t wgs, int64_t resident_wgs) const { return wgs > resident_wgs || kf_force_tickets; }

    // ---- learning: what the summary (or the enqueue) found.  Those returning bool: false = the mode forbids the repeat ----
    static bool many(int failed, int batch) { return batch < 8 || failed * 8 > batch; }   // else: repair the few signals one by one
    bool workspace_unavailable() { if (fuse_mode == ITD_FUSE_ONLY) return false; fuse_no_memory = true; return true; }
    bool resident_failed() { if (resident_mode == ITD_RESIDENT_ONLY) return false; ++resident_repeats; resident_off_left = kBackOff; return true; }
    bool level0_fell_short() { if (l0_mode == ITD_LEVEL0_FUSED) return false; l0_records_left = kBackOff; return true; }
    // a delivered probe that reached the learned cap's level drops the cap (the workload has changed)
    void fused_levels_delivered(bool capped, int32_t M)
    {
        fuse_off_span = kBackOff; fuse_probe = false;
        if (fuse_cap || !fuse_cap_auto) return;
        if (capped) ++fuse_cap_calls;
        else if (M + 1 >= fuse_cap_auto) { fuse_cap_auto = 0; fuse_cap_calls = 0; fuse_cap_span = kBackOff; }
    }
    enum class Refusal { Fail, RepairSignals, RepeatCall };
    // `bits`: the OR of the failed signals' fail bits, `fail_lev`: the lowest level any of them failed at; the call's L0, cap and M
    Refusal fused_levels_refused(int bits, int fail_lev, int L0, int cap_of_call, int32_t M, bool many_failed)
    {
        if (fuse_mode == ITD_FUSE_ONLY) return Refusal::Fail;
        const bool stays_fused = back_off(bits, L0);
        if (!many_failed) return Refusal::RepairSignals;   // (a few signals: back_off only — no pause, no cap, no fuse_repeats)
        ++fuse_repeats;
        // input failing at one level every time keeps the levels in front of it fused: the next calls are capped there (only this
        // path learns a cap); a refused probe puts the next one further off
        bool capped_next = false;
        if (!fuse_cap && !(bits & (kFailCapacity | kFailWait))) {
            if (fail_lev >= L0 + 2 && fail_lev <= M + 1 && (cap_of_call == 0 || fail_lev < cap_of_call)) {
                fuse_cap_span = (fuse_cap_auto && !cap_of_call) ? doubled(fuse_cap_span) : kBackOff;
                fuse_cap_auto = fail_lev; fuse_cap_calls = 0; capped_next = true;
            } else { fuse_cap_auto = 0; fuse_cap_span = kBackOff; }
        }
        if (!stays_fused && !capped_next) levels_off();
        return Refusal::RepeatCall;
    }
    // the device-side repair re-ran `fixed` signals for `why` (1: fused levels, their fail bits from bit 3; 2: level 0; 4: resident).
    // Unlike the host path: a few signals learn nothing (not even back_off), no cap, no pause reset, no *_repeats counted.
    void device_repaired(int fixed, int why, bool many_failed, int L0)
    {
        device_repairs += fixed;
        if (!fixed || !many_failed) return;
        if ((why & 1) && !back_off((why >> 3) & 31, L0)) levels_off();
        if (why & 2) l0_records_left = kBackOff;
        if (why & 4) resident_off_left = kBackOff;
    }
    // capacity: first level 2 -> 3, then halve the range; a wait-only fail: tickets.  True: the next calls stay fused that way
    bool back_off(int bits, int level)
    {
        if (bits & kFailCapacity) {
            if (!fuse_level && level == 2 && !fuse_level2_off) { fuse_level2_off = true; return true; }
            if (!fuse_range && tiles_per_wg() > kRangeMinTiles) { ++kf_shrink; return true; }
            return false;
        }
        if (bits == kFailWait && !kf_force_tickets) { kf_force_tickets = true; return true; }
        return false;
    }
    void levels_off() { if (fuse_probe) fuse_off_span = doubled(fuse_off_span); fuse_off_left = fuse_off_span; fuse_probe = false; }
};

// ---- which form a spline extraction takes: nothing is learned, so plain functions of the call's shape ----
// Few long signals: parallel in the knots; many short rows: one thread per signal, FITPACK's own sweep (bit-level).  One signal that
// one workgroup can hold: the parallel form as one launch.
constexpr int64_t kSplineParallelMinN = 1024;      // automatic: parallel in the knots from this many samples ...
constexpr int32_t kSplineParallelMaxBatch = 256;   // ... for fewer signals than this
constexpr int64_t kSplineSmallMax = 8192;          // samples one workgroup holds (itd_nak.hpp's kNakSmallMax)
enum class SplineForm { Serial, Parallel, Small };
inline SplineForm spline_form(int32_t solver, int64_t n, int32_t batch)
{
    const bool par = solver == ITD_SPLINE_PARALLEL || (solver == ITD_SPLINE_AUTO && batch < kSplineParallelMaxBatch && n >= kSplineParallelMinN);
    if (!par) return SplineForm::Serial;
    return batch == 1 && n <= kSplineSmallMax ? SplineForm::Small : SplineForm::Parallel;
}
// MEITD's selection loop as one launch: where every extraction of the host-driven loop on this signal would take the small form
inline bool meitd_one_launch(int32_t solver, int64_t n) { return n >= 3 && spline_form(solver, n, 1) == SplineForm::Small; }
