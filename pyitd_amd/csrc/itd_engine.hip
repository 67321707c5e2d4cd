// itd_engine.hip — host side of libpyitd_hip.so: the C ABI declared in include/pyitd_hip.h.
//
// The level loop of the reference driver (ITD.itd, ITD.py:384-432) is enqueued here as a fixed
// sequence of launches on one HIP stream with NO host synchronisation between levels: the stop rule
// (`num_extrema < 2`, ITD.py:404) is evaluated on the device by block 0 of k_extract and later launches of a
// stopped signal return at once; k_finalize performs the row fix-up.  The host reads one small
// per-signal summary at the end (itd_get_summary).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <atomic>
#include <chrono>
#include <dlfcn.h>
#include <memory>
#include <new>
#include <thread>
#include <vector>

#include "../../include/pyitd_hip.h"
#include "itd_kernels.hpp"
#include "itd_resident.hpp"
#include "itd_knotfirst.hpp"
#include "itd_cubic.hpp"
#include "itd_detect_fast.hpp"
#include "itd_stream.hpp"
#include "itd_tfe.hpp"
#include "itd_tfe_batch.hpp"
#include "itd_tfe_spectrum.hpp"
#include "itd_waves.hpp"
#include "itd_wave_hist.hpp"
#include "itd_wave_stream.hpp"
#include "itd_spectrum_stream.hpp"
#include "itd_inst_stream.hpp"
#include "itd_hist_stream.hpp"
#include "itd_table_stream.hpp"
#include "itd_wave_bounds.hpp"
#include "itd_spline.hpp"
#include "itd_nak.hpp"
#include "itd_wpe.hpp"
#include "itd_meitd.hpp"
#include "itd_policy.hpp"
#include "itd_memory.hpp"
#include "itd_fft.hpp"

#ifndef ITD_TILE
#define ITD_TILE 512
#endif

using namespace itd;

namespace {
constexpr int T = ITD_TILE;
#ifndef ITD_SLOT_PAD
#define ITD_SLOT_PAD 0
#endif
constexpr int64_t kSlotPad = ITD_SLOT_PAD;   // elements (multiple of 2 keeps the slots 16-byte aligned)
static_assert(T % 128 == 0 && T / 64 <= kMaxGroups, "tile geometry: whole 8/16-byte loads per lane, <= 8 flag words per record");

// per-signal state + the (padded) group sums of all three rotating buffers, one launch
__global__ void k_init_state(SigState *st, int batch, int32_t *gsum, int64_t gsum_elems, int keep_in_nan = 0)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < gsum_elems; i += (int64_t)gridDim.x * blockDim.x)
        gsum[i] = 0;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const int in_nan = st[b].in_nan;
    sig_state_reset(st + b);
    if (keep_in_nan) st[b].in_nan = in_nan;   // the NaN-input repeat needs to know which signals hold one (k_nan_level0)
}

// ---- device-visible validity and the device-side repair (itd_set_valid_flags, itd_set_device_repair) ----
// One thread per signal, behind the last launch of a decomposition: the fused levels' verdict merged into the signal's state (what
// read_states does on the host when the summary is read), then valid[b] = 1 if the rows in the caller's buffer are final; need[b] = 1
// if the optimistic forms fell short for this signal (fused levels refused, fused level 0 out of reach, resident form met a
// non-finite value) and a level-by-level run would repair it.  A NaN in the caller's signal is neither (the host repeats such a
// call the way the reference runs it): valid = 0, need = 0.
__global__ void k_verdict(SigState *__restrict__ state, int batch, const KfSig *__restrict__ kf, int L0, int nan_follow,
                          int32_t *__restrict__ valid, int32_t *__restrict__ need)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    SigState &st = state[b];
    if (kf) kf_sig_verdict(kf[b], L0, st);
    const int nan_in = st.in_nan != 0;
    const int short_fall = !nan_in && (st.kf_fail != 0 || st.l0_fail != 0 || st.res_fail != 0);
    if (need) need[b] = short_fall;
    if (valid) valid[b] = (!short_fall && !(nan_in && nan_follow)) ? 1 : 0;
}

// in front of the repair's launches: the set of states they work on — a signal that needs the repair starts from the initial
// state, every other one carries a copy of its final state and the skip flag (the repair's launches return at once for it); the
// set's group sums cleared
__global__ void k_repair_init(const SigState *__restrict__ from, SigState *__restrict__ to, const int32_t *__restrict__ need, int batch,
                              int32_t *gsum, int64_t gsum_elems)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < gsum_elems; i += (int64_t)gridDim.x * blockDim.x)
        gsum[i] = 0;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    if (need[b]) {
        // (bits 0 .. 2: which optimistic form fell short; from bit 3 on the fused levels' own failure bits, so that the host's back-offs
        //  — smaller ranges only for a list that outgrew its workgroup — see the reason as they do without the device-side repair)
        const int why = (from[b].kf_fail ? 1 : 0) | (from[b].l0_fail ? 2 : 0) | (from[b].res_fail ? 4 : 0) | ((from[b].kf_fail & 31) << 3);
        sig_state_reset(to + b);
        to[b].skip = -why;
    } else { to[b] = from[b]; to[b].skip = 1; }
}

// behind the repair: what it repaired is final now (a level-by-level run cannot fall short; a NaN it met in the signal stays the host's)
__global__ void k_verdict_repaired(const SigState *__restrict__ state, int batch, const int32_t *__restrict__ need, int nan_follow,
                                   int32_t *__restrict__ valid)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch || !need[b]) return;
    valid[b] = (state[b].in_nan && nan_follow) ? 0 : 1;
}

// itd_debug_int_ratio_check: int_ratio(a, b) against the compiler's full division for every pair 0 <= a <= b <= max_den (b >= 1) and
// for pseudo-random pairs up to 2^31 - 1: the number of pairs whose bit patterns differ
__global__ void k_int_ratio_check(int max_den, unsigned long long *bad)
{
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (long long)gridDim.x * blockDim.x;
    unsigned long long mine = 0;
    for (long long b = 1 + tid; b <= max_den; b += nthreads)
        for (int a = 0; a <= (int)b; ++a) {
            volatile double x = (double)a, y = (double)(int)b;          // (volatile: the reference stays the emitted division)
            mine += dbits(int_ratio(a, (int)b)) != dbits(x / y);
        }
    unsigned long long h = 0x9e3779b97f4a7c15ull * (unsigned long long)(tid + 1);
    for (int k = 0; k < 4096; ++k) {
        h ^= h << 13; h ^= h >> 7; h ^= h << 17;
        const int b = (int)((h >> 1) & 0x7fffffff) | 1, a = (int)((h >> 33) & 0x7fffffff) % b;
        volatile double x = (double)a, y = (double)b;
        mine += dbits(int_ratio(a, b)) != dbits(x / y);
    }
    if (mine) atomicAdd(bad, mine);
}

// totals[2b + 1] = signal b holds a NaN (k_compact): OR them into one flag
__global__ void k_or_nan_flags(const int32_t *__restrict__ totals, int batch, int32_t *__restrict__ flag)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch && totals[2 * b + 1]) atomicOr(flag, 1);
}

// up to 32 counts for a polling host: self-validating words (itd_kernels.hpp: small_put)
__global__ void k_copy_words(const int32_t *__restrict__ src, unsigned long long *__restrict__ words, int cnt, int32_t seq)
{
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) small_put(words, i, (uint32_t)src[i], (uint32_t)seq);
}

__global__ void k_widen_idx(const int32_t *__restrict__ src, int64_t *__restrict__ dst, int64_t cnt)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) dst[i] = src[i];
}
static_assert(FormPolicy::kRangeTiles == kKcTiles && FormPolicy::kFailCapacity == kKfFailCapacity && FormPolicy::kFailWait == kKfFailWait,
              "itd_policy.hpp restates the fused levels' geometry and fail bits");
static_assert(kSplineSmallMax == kNakSmallMax && kSplineParallelMinN <= kSplineSmallMax && kSplineParallelMaxBatch > 1,
              "itd_policy.hpp restates what one workgroup of itd_nak.hpp holds; the automatic solver reaches the one-workgroup form");
}  // namespace

// A call's result rows: the caller's buffer and its element type (float64, or float32 for the itd_decompose_rows32_* entries).  The
// type is a property of the call: it travels with the pointer through every form and every repeat, which therefore writes the same
// type into the same buffer as the first attempt.  Strides and offsets count elements.
// So does a selection (itd_decompose_select_*): sel set, the buffer holds count() packed rows per signal — the rotations of which.mask
// in ascending order, then the residual if which.res >= 0 — and a row that is not among them is stored nowhere.  Without a selection
// the map is the identity (row r in slot r, the residual in the row of the stop) and every launch is the one it always was.
struct Rows {
    void *p = nullptr; bool f32 = false;
    bool sel = false; RowSel which{0u, -1};
    Rows() {}
    Rows(double *d) : p(d) {}
    Rows(float *f) : p(f), f32(true) {}
    Rows(void *q, bool is32, uint32_t mask, bool residual) : p(q), f32(is32), sel(true), which{mask, residual ? __builtin_popcount(mask) : -1} {}
    size_t esz() const { return f32 ? sizeof(float) : sizeof(double); }
    Rows at(int64_t elems) const { Rows r = *this; r.p = static_cast<char *>(p) + elems * (int64_t)esz(); return r; }
    int count(int M) const { return sel ? __builtin_popcount(which.mask) + (which.res >= 0 ? 1 : 0) : M + 2; }   // rows per signal
    int64_t stride(int M, int64_t n) const { return (int64_t)count(M) * (n + ITD_ROW_PAD); }   // elements from one signal's rows to the next's
    // the slot of the row a level launch writes (rotation j, or behind the last requested level the "Out of time!" residual); < 0: none
    int slot(int j, bool residual) const { return !sel ? j : residual ? which.res : sel_slot(which, j); }
};

// A Rows as the kernels see it: every kernel that stores rows is a template on the element type (Trow) and on whether the rows are a
// selection's packed ones (SEL).  with_row_form is the one place where a call's runtime description becomes those template arguments:
// it hands f the form as a tag value, and what f launches names each kernel once, as k<..., typename Form::Trow, Form::SEL>.
template <typename TROW, bool SELECT>
struct RowForm { using Trow = TROW; static constexpr bool SEL = SELECT; };
template <typename F>
int with_row_form(const Rows &rows, F &&f)
{
    if (rows.sel) return rows.f32 ? f(RowForm<float, true>{}) : f(RowForm<double, true>{});
    return rows.f32 ? f(RowForm<float, false>{}) : f(RowForm<double, false>{});
}

// The record of the last decomposition enqueued: what itd_get_summary reads back, repeats or repairs, and itd_get_timing, ... refer to
struct LastCall {
    int32_t batch = 0, m = 0; int64_t n = 0; hipStream_t stream = nullptr;                              // the call's arguments
    const void *x = nullptr; bool x_f32 = false; int64_t x_stride = 0; Rows rows; double *bases = nullptr;
    bool fused = false, resident = false;   // fused level 0; the one-workgroup form (k_resident)
    bool nan_input = false;        // the NaN-input repeat (k_nan_level0): its results follow the reference
    bool kf = false;               // fused sparse levels whose verdict is still to be drawn
    int kf_level = 0, kf_cap = 0;  // their first level and cap (0: all levels fused)
    int kf_form = 0, kf_cap_form = 0;   // ... as enqueued (itd_get_last_fuse_level / _cap): stay when a summary has drawn the verdict
};

struct itd_engine {
    int device = 0;
    int64_t max_n = 0;
    int32_t max_batch = 0;
    int64_t max_tiles = 0;
    hipStream_t own_stream = nullptr;
    // workspace
    Buf<int32_t> d_lists;          // [tiles][T]  per-tile knot lists, written only for the API helpers (k_compact)
    Buf<int32_t> d_counts;         // [2][batch][tiles]  knots per tile, double buffered by level parity
    Buf<TileRec> d_recs;           // [2][batch][tiles]  head/tail knot records, double buffered by level parity
    int64_t tiles_half = 0;        // elements per counts/recs buffer
    Buf<int32_t> d_gsum;           // [2][3][batch][groups*pitch]: per-64-tile knot totals, rotating by level % 3; two sets (below)
    int64_t gsum_third = 0;        // elements per buffer
    Buf<int32_t> d_kidx;           // [max_n + 2]  ordered knot indices for the API helpers (single signal)
    Buf<int32_t> d_total;          // [1] knot total written by k_compact
    Buf<double> d_pp;              // [batch][3][pp_pitch] rotating baselines (slot = level % 3)
    int64_t pp_pitch = 0;          // elements between consecutive slots: max_n + kSlotPad (breaks the power-of-two distance)
    Buf<SigState> d_state;         // [2][batch]
    Pinned<SigState> h_state;      // [batch]
    Pinned<char> h_kf;             // the heads of the fused levels' KfSig (kKfSigHead bytes per signal), on demand
    // Per-signal states and group sums exist twice.  A decomposition works on the set the previous one did not use, and its last
    // launch (k_finalize) re-initialises the other set for the call after it: no initialising launch in front of a decomposition,
    // and the summary of the last call stays readable.  dirty_*: the leading part of a set that may not be in its initial state
    // (signals / group-sum elements per buffer); a call that finds its set dirty initialises it with a launch of its own.
    int cur_set = 0;
    int32_t dirty_sig[2] = {0, 0};
    int64_t dirty_gs[2] = {0, 0};
    // workspace of the single-level helpers (itd_detect_*, itd_baseline_extract_*): one signal, apart from the
    // decomposition's, so a helper call never disturbs a decomposition that is still in flight or not yet summarised;
    // with d_lists, d_kidx and d_total the fixed buffers that helper_ws() presents as a KnotWs (no allocation after create)
    Buf<int32_t> d_hcounts;        // [2][tiles]
    Buf<TileRec> d_hrecs;          // [2][tiles]
    Buf<int32_t> d_hgsum;          // [3][groups*pitch]
    int64_t hgsum_third = 0;
    Buf<SigState> d_hstate;        // [1]
    int32_t chunk = 0;             // signals per launch sequence of a batched decomposition (0 = automatic, see enqueue_decompose)
    int32_t batch_streams = 2;     // chunks of a batch rotate over this many streams (itd_set_batch_streams): 1 .. kMaxBatchStreams
    hipStream_t aux_stream[3] = {nullptr, nullptr, nullptr};   // the others besides the caller's, created on demand
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};

    FormPolicy policy;              // which form each call takes, what the summaries have taught (itd_policy.hpp)
    const void *lds_fn[24] = {}; int lds_fns = 0;   // the kernel instances granted their dynamic LDS on this engine (allow_lds)
    // a few scalars per call come back to the host in MEITD's operators (counts, six sums): 256 bytes of pinned host memory that the
    // GPU writes directly (mapped, coherent) — no copy behind the launch, just the stream's synchronisation (a pageable destination
    // cost ~15 us per call: 110 calls per MEITD run)
    Pinned<void> h_small; void *d_small = nullptr;   // (d_small: its device address)
    int32_t small_seq = 0;          // the number of the call whose scalars are awaited: every word of a result carries it in its high half (small_put)
    int32_t resident_window = 0;    // segments per pass over a level's ranks (itd_set_resident_window; 0 = automatic)
    // the fused sparse levels (itd_knotfirst.hpp): workspace (allocated at first use), mode, first fused level
    Buf<void> d_kf;
    std::vector<Buf<void>> kf_retired;   // earlier, smaller workspaces: a captured graph may still hold their pointers — kept until the engine is destroyed
    KfWs kf{};                       // pointers into d_kf, for signal 0
    // device-visible validity / device-side repair (itd_set_valid_flags, itd_set_device_repair)
    int32_t *valid_dev = nullptr;                    // the caller's [batch] words, written behind every decomposition; NULL = none
    bool device_repair = false;
    Buf<int32_t> d_need;                             // [max_batch] which signals the repair's launches work on
    Buf<int32_t> d_valid_own;                        // [max_batch] (the repair needs the words even if the caller gave none)
    bool last_device_repair = false;                 // the last call carried its repair: the summary has nothing to repeat
    int64_t kf_resident_wgs = 0;                     // knot-side workgroups the device holds at once (occupancy query at creation of the workspace)
    // fault injection into the fused levels' workspace (itd_debug_kf_fault; tests only): kind < 0 = none
    int32_t fault_kind = -1, fault_level = 0, fault_where = 0, fault_slot = 0, fault_delta = 0;
    int32_t fault_sig = 0;         // the signal of the batch the fault lands in (itd_debug_kf_fault_signal)
    int32_t spline_solver = ITD_SPLINE_AUTO;   // FITPACK flavour: serial bit-level sweep or the parallel moment form (itd_set_spline_solver)
    int64_t ws_total = 0;          // itd_engine_workspace_bytes: the create-time buffers and every fused-levels workspace, retired ones included
    // host-convenience staging (grow only)
    Buf<void> d_cub;                                      // cubic variant: per-signal jobs + K, bf, b (3 arrays of idx+2 doubles each);
                                                          // also staging of the NaN-input helper path and the instantaneous step
    Buf<int32_t> d_cub_e;                                 // cubic variant: the caller's knots narrowed to int32 (host form)
    Buf<int32_t> d_flag;                                  // [1] device-side argument check
    // three arenas a KnotWs is carved from (knot_workspace), apart so that operators used in one call do not share one
    Buf<void> d_dw;                                       // batched knot detection: cubic batch, detect batch, counts, streams
    Buf<void> d_bw;                                       // batched single-level tier-1 extraction (a k_extract behind the scan)
    Buf<void> d_sp;                                       // spline flavour (batched): the scan's parts, fit arrays, metadata
    Buf<double> d_sp2;                                    // 2-D consumers: three planes of scratch
    Buf<void> d_ib;                                       // batched instantaneous step (itd_instantaneous_batch_*): tile records, Ahead / Atail
    Buf<void> d_wv;                                       // single-wave analysis (itd_waves_batch_*, itd_wave_filter_batch_*, itd_wave_hist_batch_*): tile records, forward / backward carries
    Buf<void> d_ts;                                       // time-frequency-energy spectrum (itd_tfe_spectrum_*): tile records, Ahead / Atail
    Buf<void> d_mb;                                       // MEITD over a batch (itd_meitd_batch_f64): per-signal results, solver arrays, logs, XITD sums
    Buf<int64_t> d_rowtab;                                // itd_gather_rows_f64: the row table
    Buf<char> d_wpe;                                      // weighted permutation entropy: the segments' sums
    Buf<void> d_io_x;
    Buf<void> d_iq_avg;                                  // the I/Q form of the cubic operator: the components' mean series
    Buf<double> d_io_rows;
    Buf<double> d_io_bases;
    Pinned<void> h_pin[2];                 // host-form calls: pinned bounce buffers of the pipelined device -> host copy (copy_to_host)
    bool host_keep_bases = false;      // itd_set_host_keep_baselines: host-form calls leave their baselines in d_io_bases
    int64_t kept_n = 0; int32_t kept_nb = -1;   // what itd_get_last_baselines_host can still deliver (-1: nothing)
    // the FFT and the ITD-Fourier cascade (itd_fft.hpp, itd_fourier.inc), all grown on demand
    Buf<void> d_fft_x;                                    // the selectors' spectra
    Buf<void> d_fft_y;                                    // four-step: the column transforms
    Buf<void> d_fft_a;                                    // Bluestein: the padded chirped rows
    Buf<void> d_fft_b;                                    // Bluestein: the chirp's spectrum for fft_chirp_n
    int64_t fft_chirp_n = 0;
    Buf<void> d_fft_rec;                                  // selector records when the caller wants none
    Buf<void> d_fc;                                       // cascade: signals, band scratch, rows, modes, records, flags
    Buf<void> d_fio;                                      // cascade host form: its input, rows and accumulators (not d_io_*)
    Buf<double> d_fmodes;                                 // cascade: the mode arena of the last call (non-lean)
    int64_t fmodes_count = 0, fmodes_n = 0; bool fmodes_lean = false;
    std::vector<int32_t> frec;                            // cascade: [fmodes_count][8] records of the last call
    Buf<int32_t> d_fplan;                                 // cascade: the band plan's knot lists (int32), for fplan_n / fplan_sr
    int64_t fplan_n = 0; double fplan_sr = 0.0;
    std::vector<int64_t> fplan_host, fplan_idx;
    // last run
    bool ran = false;
    LastCall last;
    int32_t nan_input_mode = ITD_NAN_INPUT_FOLLOW;   // itd_set_nan_input_mode
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev;   // event pairs: [2k] start, [2k+1] stop
    std::vector<int> ev_tag;      // what pair k brackets (ITD_TIME_*)
    std::vector<int> ev_from, ev_to;   // the pair's two events (normally 2k, 2k+1; a span borrows the events of the launches at its ends)
    int span_first = -1, span_last = -1;   // of the decomposition being enqueued: its first / last instrumented launch
    int n_timed = 0;              // pairs recorded since timing was (re)enabled
    bool timing_overflow = false;
    int timing_mode = 0;          // 0: every launch class; 1: the level-0 launch only (itd_get_step_periods)
    int timing_stride = 1;        // instrument every stride-th decomposition only (event records cost ~5 us each)
    int timing_seq = 0;
    bool timing_now = false;
    char err[512] = {0};
};

namespace {

int fail_hip(itd_engine *e, hipError_t rc, const char *what)
{
    if (e) snprintf(e->err, sizeof(e->err), "%s: %s (%d)", what, hipGetErrorString(rc), (int)rc);
    return ITD_ERR_HIP;
}

#define HIP_TRY(e, call)                                         \
    do {                                                         \
        hipError_t rc__ = (call);                                \
        if (rc__ != hipSuccess) return fail_hip((e), rc__, #call); \
    } while (0)

struct DevGuard {
    int prev = -1;
    explicit DevGuard(int dev) { (void)hipGetDevice(&prev); if (prev != dev) (void)hipSetDevice(dev); else prev = -1; }
    ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

inline int64_t tiles_of(int64_t n) { return (n + T - 1) / T; }

// the stream a call works on: the caller's, or the engine's own
inline hipStream_t stream_of(const itd_engine *e, void *stream) { return stream ? (hipStream_t)stream : e->own_stream; }

// hipEvent pairs on the launch stream around selected launches (bench instrumentation, off by default)
// a pair of events for a launch that records them itself (hipExtLaunchKernel)
int time_slot(itd_engine *e, int tag)
{
    if (!e->timing || !e->timing_now) return -1;
    if (e->timing_mode == 1 && tag != ITD_TIME_EXTRACT_L0) return -1;   // step periods: only the level-0 launch carries events
    if (2 * (size_t)e->n_timed + 1 >= e->ev.size()) { e->timing_overflow = true; return -1; }
    const int k = e->n_timed++;
    e->ev_tag[(size_t)k] = tag;
    e->ev_from[(size_t)k] = 2 * k; e->ev_to[(size_t)k] = 2 * k + 1;
    if (tag != ITD_TIME_DECOMPOSE && tag != ITD_TIME_KF_KNOTS) {      // a launch of its own: the ends of the decomposition's span
        if (e->span_first < 0) e->span_first = k;
        e->span_last = k;
    }
    return k;
}

// signals per launch sequence of a batched decomposition.  All levels of a chunk run before the next chunk starts, so
// the baseline a level writes (8 B per sample per signal) is still in the 256 MiB Infinity Cache when the next level reads it
// — the state the single 2^24-sample signal is in.  Automatic: about 2^24 samples per chunk.
constexpr int32_t kMaxGridY = 65535;   // HIP's limit on gridDim.y
int chunk_of(const itd_engine *e, int64_t n, int32_t batch)
{
    if (e->chunk > 0) return std::min<int32_t>(std::min<int32_t>(e->chunk, kMaxGridY), batch);
    // one stream: 2^24 samples per chunk; two or more (the default): half of that per chunk — two chunks in flight, measured best
    // on 512 x 2^20 with the fused levels' knot side as one launch (chunks of 8 signals over 2 streams: 12.3 ms against 12.7 with 12
    // and 13.0 with 16 over one stream; round 2, level by level: 10-12 signals over 2 streams, profiles/r02/session2_batch_streams.txt)
    // a batch of up to 2^24 samples in all is ONE sequence (64 signals of 2^18 samples: 393 us as one sequence against 466 as two chunks
    // of 32 over two streams; 256 x 2^16: 416 against 436 — profiles/r05/bench_default_form.json, many_mid_size_signals)
    if ((int64_t)batch * n <= ((int64_t)1 << 24) && batch <= kMaxGridY) return batch;
    const int64_t per = e->batch_streams > 1 ? ((int64_t)1 << 23) : ((int64_t)1 << 24);
    const int64_t c = std::max<int64_t>(1, per / n);
    return (int)std::min<int64_t>(std::min<int64_t>(c, kMaxGridY), batch);   // a chunk's signals are the launches' grid.y
}

// samples per launch sequence: what the policy's automatic choices of the fused levels go by
inline int64_t seq_samples(const itd_engine *e, int64_t n, int32_t batch) { return (int64_t)std::min<int32_t>(chunk_of(e, n, batch), batch) * n; }

// The workspace of the fused sparse levels (itd_knotfirst.hpp), allocated at the first call that takes that path.  Per signal and
// knot-side workgroup (kKcTiles tiles): a slab of table entries (32 B per knot and level: kKcSlab of them) and one 256-byte
// boundary record per level; per level and tile the knots' flag words and the tile's first table index; per tile the near-tie flag words.
constexpr int kKfLevels = ITD_MAX_ITERATION + 3;
int ensure_kf_ws(itd_engine *e, int tpw, bool may_allocate)
{
    const size_t wgs = (size_t)(e->max_tiles + tpw - 1) / tpw;
    if (e->d_kf && (size_t)e->kf.wgs_max >= wgs) return ITD_OK;
    if (!may_allocate) return ITD_ERR_NOMEM;
    if (e->d_kf) {
        // smaller ranges (a list outgrew its workgroup, itd_set_fuse_range, a lower first fused level): more workgroups per signal need
        // a larger workspace.  The old one is NOT freed: a hipGraph captured on this engine has its pointers baked into the fused
        // levels' launches and may be replayed at any time (its launches stay self-consistent: geometry and pointers travel
        // together as kernel arguments) — it is retired until itd_engine_destroy; its bytes stay counted
        e->kf_retired.push_back(std::move(e->d_kf));
    }
    const size_t B = (size_t)e->max_batch;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_sig = al(B * sizeof(KfSig)), b_pool = al(B * wgs * kKcSlab * sizeof(KfEntry));
    const size_t b_first = al(B * kKfLevels * (size_t)e->max_tiles * 4), b_tf = al(B * kKfLevels * (size_t)e->max_tiles * 64);
    const size_t b_tie = al(B * (size_t)e->max_tiles * 64), b_rec = al(B * kKfLevels * wgs * kKcRecGran * 8);
    const size_t total = b_sig + b_pool + b_first + b_tf + b_tie + b_rec;
    const hipError_t rc = e->d_kf.alloc(total, &e->ws_total);
    if (rc != hipSuccess) { fail_hip(e, rc, "hipMalloc(fused levels' workspace)"); return rc == hipErrorOutOfMemory ? ITD_ERR_NOMEM : ITD_ERR_HIP; }
    char *p = (char *)e->d_kf;
    KfWs &w = e->kf;
    w.sig = (KfSig *)p; p += b_sig;
    w.pool = (KfEntry *)p; p += b_pool;
    w.first = (int32_t *)p; p += b_first;
    w.tflags = (unsigned long long *)p; p += b_tf;
    w.nearw = (unsigned long long *)p; p += b_tie;
    w.rec = (unsigned long long *)p;
    // the signals' generation counters start at 0 and no record carries a tag yet
    // (hipMemset runs on the null stream; the launches that use the workspace on non-blocking streams: the fills have to be over first)
    if (hipMemset(w.sig, 0, b_sig) != hipSuccess || hipMemset(w.rec, 0, b_rec) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ITD_ERR_HIP;
    w.wgs_max = (int32_t)wgs; w.rec_levels = kKfLevels;
    {   // how many knot-side workgroups are resident at once: a grid within that takes its ids from blockIdx (itd_knotfirst.hpp)
        int per_cu = 0, cus = 0;
        hipDeviceProp_t prop;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(&k_kf_knots<T>), kKcThreads, 0) != hipSuccess ||
            hipGetDeviceProperties(&prop, e->device) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
        else cus = prop.multiProcessorCount;
        // (Should the hardware admit fewer than the API says, the surplus workgroups
        //  start in blockIdx order as others finish — observed, not promised; a wait that can never end is given up after
        //  ITD_KC_TIMEOUT and the call repeated level by level)
        e->kf_resident_wgs = (int64_t)per_cu * cus;
    }
    return ITD_OK;
}

// a launch through hipExtLaunchKernel that carries the timed pair `pair` (time_slot; -1: none): its two events take the dispatch's own
// begin / end timestamps (no marker packets in the stream: nothing is added to the timed region)
hipError_t launch_timed(itd_engine *e, const void *fn, dim3 grid, dim3 block, void **args, hipStream_t st, int pair)
{
    return hipExtLaunchKernel(fn, grid, block, args, 0, st, pair >= 0 ? e->ev[2 * (size_t)pair] : nullptr,
                              pair >= 0 ? e->ev[2 * (size_t)pair + 1] : nullptr, 0);
}

// What every chunk of one decomposition shares, computed once per call by enqueue_decompose
template <typename Tin>
struct DecomposePlan {
    const Tin *x; int64_t x_stride, n, rows_stride; int32_t M;
    Rows rows; double *bases;         // bases: the caller's baselines buffer, or NULL (the baselines live in the engine's rotating slots)
    bool fuse0, nan_input, kf;        // fused level 0; the NaN-input repeat (k_nan_level0); fused sparse levels
    int L0, cap, Mk;                  // fused levels L0 .. Mk + 1; cap != 0: levels cap .. M + 1 one launch each behind them
    int n_tiles, n_groups;
    int kf_tpw, kf_wgs;               // the knot side's tiles per workgroup, its workgroups per signal
    SigState *state, *other_state;    // the call's set of states / group sums, and the other set (left initialised for the next call)
    int32_t *gsum, *other_gsum;
    int chunk, S;                     // signals per chunk; streams the chunks rotate over
};

// One chunk's buffers: signals b0 .. b0 + nb - 1 of the call (grid.y of its launches), every per-signal pointer offset by b0
struct ChunkBufs {
    const itd_engine *e;
    int nb, n_tiles; int64_t n, rows_stride;
    hipStream_t st;
    SigState *state; Rows rows; double *bases, *pp; int32_t *gsum, *counts; TileRec *recs; unsigned long long *near;
    int32_t *gs(int level) const { return gsum + (int64_t)(level % 3) * e->gsum_third; }      // group sums rotate by level % 3,
    int32_t *cnt(int level) const { return counts + (int64_t)(level & 1) * e->tiles_half; }   // counts and records by level parity
    TileRec *rec(int level) const { return recs + (int64_t)(level & 1) * e->tiles_half; }
    // level j's baseline: row j of the caller's buffer, or slot j % 3 of the engine's rotating slots
    double *base(int j) const { return bases ? bases + (int64_t)j * n : pp + (int64_t)(j % 3) * e->pp_pitch; }
    int64_t base_stride() const { return bases ? rows_stride : 3 * e->pp_pitch; }
};

// one level launch of a chunk (k_extract): level j's input xin -> rotation rows[j] and baseline j; level j's counts, records and group
// sums -> level j + 1's (TIES: the launch in front of the fused sparse levels also flags the tiles of its baseline that hold a near tie)
// (slot: Rows::slot.  < 0, a level whose row the selection drops: the form without a row store, TROW = NoRow — its pointer is the buffer's
// own base, a valid address that is never used)
template <typename Trow, typename TIN, bool FIN, int CAPK, int KTW = kTilesPerWave, bool FUSE = false, bool TIES = false>
hipError_t launch_extract(itd_engine *e, const ChunkBufs &c, const TIN *xin, int64_t xs, int j, int pair, int slot)
{
    const TIN *a_x = xin; int64_t a_xs = xs, a_n = c.n, a_rs = c.rows_stride, a_bs = c.base_stride();
    int a_nt = c.n_tiles, a_b = c.nb, a_lvl = j, a_keep = 0;
    const int32_t *a_ci = c.cnt(j), *a_gi = c.gs(j); int32_t *a_co = c.cnt(j + 1), *a_go = c.gs(j + 1), *a_gc = c.gs(j + 2);
    const TileRec *a_ri = c.rec(j); TileRec *a_ro = c.rec(j + 1);
    void *a_rot = c.rows.at((int64_t)std::max(slot, 0) * (c.n + ITD_ROW_PAD)).p; double *a_bas = c.base(j);
    SigState *a_st = c.state; unsigned long long *a_tie = TIES ? c.near : nullptr;
    void *args[] = {&a_x, &a_xs, &a_n, &a_nt, &a_b, &a_ci, &a_co, &a_ri, &a_ro, &a_gi, &a_go, &a_gc, &a_rot, &a_rs,
                    &a_bas, &a_bs, &a_st, &a_lvl, &a_keep, &a_tie};
    const auto launch = [&](auto form) {
        return launch_timed(e, reinterpret_cast<const void *>(&k_extract<TIN, T, FIN, CAPK, KTW, FUSE, TIES, typename decltype(form)::Trow>),
                            dim3((c.n_tiles + KTW - 1) / KTW, c.nb), dim3(kWave), args, c.st, pair);
    };
    return slot < 0 ? launch(RowForm<NoRow, false>{}) : launch(RowForm<Trow, false>{});
}

// the fused levels' workspace as one chunk's launches see it: this call's geometry, every pointer offset to the chunk's first signal
template <typename Tin>
KfWs kf_chunk_ws(const itd_engine *e, const DecomposePlan<Tin> &p, const int b0, const int nb)
{
    KfWs w = e->kf;
    w.n_tiles = p.n_tiles; w.L0 = p.L0; w.nlev = p.Mk + 3 - p.L0;
    w.cap = p.cap;
    w.xnext = p.cap ? e->d_pp + (int64_t)b0 * 3 * e->pp_pitch + (int64_t)((p.cap - 1) % 3) * e->pp_pitch : nullptr; w.xnext_stride = 3 * e->pp_pitch;
    w.tpw = p.kf_tpw; w.wgs = p.kf_wgs; w.nb = nb;
    // (ids from blockIdx only where the whole grid is resident at once — with S streams in flight each launch may count on its share
    //  of the device only)
    w.ticketed = e->policy.tickets((int64_t)w.wgs * nb * p.S, e->kf_resident_wgs) ? 1 : 0;
    w.dbg_kind = e->fault_kind; w.dbg_lev = e->fault_level; w.dbg_wg = e->fault_where; w.dbg_slot = e->fault_slot; w.dbg_delta = e->fault_delta;
    w.dbg_sig = e->fault_sig - b0;               // (relative to this launch's first signal; outside it: no workgroup matches)
    const size_t B0 = (size_t)b0;
    w.sig += B0; w.pool += B0 * (size_t)w.wgs_max * kKcSlab; w.rec += B0 * (size_t)w.rec_levels * w.wgs_max * kKcRecGran;
    // (the per-signal strides of `first` / `tflags` follow this call's geometry: nlev levels x n_tiles tiles per signal)
    w.first += B0 * (size_t)w.nlev * p.n_tiles; w.tflags += B0 * (size_t)w.nlev * p.n_tiles * 8; w.nearw += B0 * (size_t)p.n_tiles * 8;
    return w;
}

// One chunk's launches, all on stream cst, in this order:
//   1. level 0's knots: k_scan0 from the signal (record-driven level 0), or k_nan_level0 (the NaN-input repeat); none for the fused
//      level-0 launch, which finds its own;
//   2. the level launches up to j_last (M + 1, or the one in front of the first fused level);
//   3. without fused levels: k_finalize.  With them: the knot side (k_kf_knots, which does k_finalize's work for the first fused level),
//      the test-only k_kf_fault and the sample pass (k_kf_apply); behind capped fused levels a scan of the baseline the sample pass
//      stored (k_clear_gsum, k_scan0), the remaining level launches and k_finalize.
// Form: the rows' RowForm (with_row_form): every launch that stores rows is the instance of that form.
template <typename Form, typename Tin>
int run_chunk(itd_engine *e, const DecomposePlan<Tin> &p, const int b0, const int nb, const hipStream_t cst)
{
    using Trow = typename Form::Trow;
    constexpr bool SEL = Form::SEL;
    const int64_t n = p.n, pp3 = 3 * e->pp_pitch;
    const ChunkBufs c{e, nb, p.n_tiles, n, p.rows_stride, cst, p.state + b0, p.rows.at((int64_t)b0 * p.rows_stride),
                      p.bases ? p.bases + (int64_t)b0 * p.rows_stride : nullptr, e->d_pp + (int64_t)b0 * pp3,
                      p.gsum + (int64_t)b0 * p.n_groups * kGsumPitch, e->d_counts + (int64_t)b0 * p.n_tiles,
                      e->d_recs + (int64_t)b0 * p.n_tiles, p.kf ? e->kf.nearw + (size_t)b0 * p.n_tiles * 8 : nullptr};
    const Tin *xc = p.x + (int64_t)b0 * p.x_stride;
    double *xm_c = c.pp + 2 * e->pp_pitch;   // NaN-input repeat: the mutated signal, one per signal at the slots' stride
    const dim3 blk(kWave);
    // what k_finalize needs (the knot side as well, for the first fused level: its gsum is set there): the rows, the baselines, the other set
    KfFin fin{c.rows.p, p.rows_stride, c.bases ? c.bases : c.pp, c.base_stride(), c.bases ? n : e->pp_pitch, c.bases ? 0 : 3, nullptr,
              p.other_state + b0, p.other_gsum + (int64_t)b0 * p.n_groups * kGsumPitch, e->gsum_third, c.rows.which.res};
    // the level launches ja .. jb: extraction j + 1, input = the level-j signal, rotation -> rows[j], baseline -> baseline j
    auto levels = [&](const int ja, const int jb) -> int {
        for (int j = ja; j <= jb; ++j) {
            const bool final_level = j == p.M + 1;        // (with fused levels: only behind capped ones)
            const int pair = time_slot(e, final_level ? ITD_TIME_EXTRACT_FINAL : (j == 0 ? ITD_TIME_EXTRACT_L0 : ITD_TIME_EXTRACT));
            const double *in = j ? c.base(j - 1) : nullptr;
            const int64_t is = c.base_stride();
            hipError_t rc;
            const int slot = c.rows.slot(j, final_level);
            if (j == 0) {   // never the last level: M >= 0
                if (p.nan_input) rc = launch_extract<Trow, double, false, kRankCap0>(e, c, xm_c, pp3, 0, pair, slot);
                else if (p.fuse0) rc = launch_extract<Trow, Tin, false, kRankCap0, kFuse0TilesPerWave, true>(e, c, xc, p.x_stride, 0, pair, slot);
                else rc = launch_extract<Trow, Tin, false, kRankCap0>(e, c, xc, p.x_stride, 0, pair, slot);
            } else if (final_level) rc = launch_extract<Trow, double, true, kRankCap>(e, c, in, is, j, pair, slot);
            else if (p.kf && j == p.L0 - 1) rc = launch_extract<Trow, double, false, kRankCap, kTilesPerWave, false, true>(e, c, in, is, j, pair, slot);
            else rc = launch_extract<Trow, double, false, kRankCap>(e, c, in, is, j, pair, slot);
            if (rc != hipSuccess) return fail_hip(e, rc, "hipExtLaunchKernel(k_extract)");
        }
        return ITD_OK;
    };
    // stop test on the last pending baseline (ITD.py:400-404 takes priority over the timeout branch) and the residual row
    auto finalize = [&]() {
        // blocks per signal: a thread of the row fix-up moves 8 samples (four 16-byte accesses) before the grid is widened
        const int fb = (int)std::min<int64_t>(std::max<int64_t>((n + 8 * kFinalizeThreads - 1) / (8 * kFinalizeThreads), 1), 1024);
        const int jf = p.M + 2;      // the level whose input is pending
        k_finalize<Trow, SEL><<<dim3(fb, nb), kFinalizeThreads, 0, cst>>>(static_cast<Trow *>(fin.rows), fin.rows_stride, n, fin.bases, fin.bases_stride,
                                                                          fin.bases_row_pitch, fin.bases_rotate, c.gs(jf), p.n_tiles, jf, c.state,
                                                                          fin.other_state, fin.other_gsum, fin.other_third, fin.res_slot);
    };

    if (p.nan_input) {
        k_nan_level0<Tin, T><<<dim3(p.n_tiles, nb), blk, 0, cst>>>(xc, p.x_stride, n, p.n_tiles, xm_c, pp3, c.cnt(0), c.rec(0), c.gs(0), c.state);
    } else if (!p.fuse0) {
        const Tin *a_x = xc; int64_t a_xs = p.x_stride, a_n = n; int a_nt = p.n_tiles;
        int32_t *a_c = c.cnt(0), *a_g = c.gs(0); TileRec *a_r = c.rec(0); SigState *a_st = c.state; int a_lv = 0;
        void *args[] = {&a_x, &a_xs, &a_n, &a_nt, &a_c, &a_r, &a_g, &a_st, &a_lv};
        HIP_TRY(e, launch_timed(e, reinterpret_cast<const void *>(&k_scan0<Tin, T, kScanTilesPerWave>),
                                dim3((p.n_tiles + kScanTilesPerWave - 1) / kScanTilesPerWave, nb), blk, args, cst, time_slot(e, ITD_TIME_SCAN0)));
    }
    if (const int rc = levels(0, p.kf ? p.L0 - 1 : p.M + 1)) return rc;
    if (!p.kf) {
        finalize();
        return ITD_OK;
    }

    // ---- levels L0 .. Mk + 1 fused: ONE knot-side launch (hand-over and every fused level), ONE pass over the samples ----
    const KfWs w = kf_chunk_ws(e, p, b0, nb);
    const double *xl = c.base(p.L0 - 1);
    const int64_t xl_stride = c.base_stride();
    {   // the knot side: k_finalize's work for the first fused level (the stop test of its input, the other state set) included
        KfWs a_w = w; int64_t a_ls = xl_stride, a_n = n; const double *a_xl = xl; int a_m = p.Mk;
        const int32_t *a_c = c.cnt(p.L0); const TileRec *a_r = c.rec(p.L0); SigState *a_st = c.state;
        KfFin a_f = fin;
        a_f.gsum = c.gs(p.L0);
        void *args[] = {&a_w, &a_f, &a_xl, &a_ls, &a_n, &a_m, &a_c, &a_r, &a_st};
        HIP_TRY(e, launch_timed(e, reinterpret_cast<const void *>(&k_kf_knots<T, Trow, SEL>), dim3((unsigned)w.wgs * (unsigned)nb), dim3(kKcThreads),
                                args, cst, time_slot(e, ITD_TIME_KF_KNOTS)));
    }
    if (e->fault_kind >= 0 && (e->fault_kind <= 5 || e->fault_kind == 8) && e->fault_level >= p.L0 && e->fault_level - p.L0 < w.nlev &&
        e->fault_where >= 0 && e->fault_where < p.n_tiles && e->fault_sig >= b0 && e->fault_sig < b0 + nb)   // (tests only) one field of what the sample pass is about to read, perturbed
        k_kf_fault<<<1, 64, 0, cst>>>(w, e->fault_sig - b0, e->fault_kind, e->fault_level - p.L0, e->fault_where, e->fault_slot & 0xffff, e->fault_delta);
    {   // the sample pass: verifies the knot side's tables and writes the rows
        KfWs a_w = w; const double *a_xl = xl; int64_t a_xs = xl_stride, a_n = n, a_rs = p.rows_stride, a_bs = p.rows_stride;
        const TileRec *a_rec = c.rec(p.L0); void *a_rows = c.rows.p; double *a_bases = c.bases;
        RowSel a_sel = c.rows.which;
        void *args[] = {&a_w, &a_xl, &a_xs, &a_n, &a_rec, &a_rows, &a_rs, &a_bases, &a_bs, &a_sel};
        const auto apply_of = [&](auto with_bases) {
            const auto fn = [](auto part) {
                return reinterpret_cast<const void *>(&k_kf_apply<T, kKfCap, decltype(with_bases)::value, decltype(part)::value, Trow, SEL>);
            };
            return p.cap ? fn(std::true_type{}) : fn(std::false_type{});    // (PART: capped fused levels)
        };
        const void *apply_fn = apply_of(std::false_type{});
        // (the caller's baselines come with all the rows in float64 only: the other forms have no BASES instance)
        if constexpr (std::is_same<Trow, double>::value && !SEL) { if (c.bases) apply_fn = apply_of(std::true_type{}); }
        HIP_TRY(e, launch_timed(e, apply_fn, dim3(p.n_tiles + kf_check_blocks(w.wgs), nb), blk, args, cst, time_slot(e, ITD_TIME_KF_APPLY)));
    }
    if (!p.cap) return ITD_OK;

    // ---- capped: levels cap .. M + 1 one launch each, from a scan of the baseline the sample pass has stored (the input of level cap:
    //      its knots' records, counts and group sums, the level's end samples).  A signal that stopped inside the fused levels carries
    //      SigState::skip: these launches return at once for it.  Should the fused levels refuse, the whole call is repeated anyway:
    //      what runs here then is discarded.
    const int64_t ge = (int64_t)nb * p.n_groups * kGsumPitch;
    k_clear_gsum<<<(int)std::min<int64_t>((ge + 255) / 256, 1024), 256, 0, cst>>>(c.gs(p.cap), c.gs(p.cap + 1), ge);
    k_scan0<double, T, kScanTilesPerWave><<<dim3((p.n_tiles + kScanTilesPerWave - 1) / kScanTilesPerWave, nb), blk, 0, cst>>>(
        c.base(p.cap - 1), c.base_stride(), n, p.n_tiles, c.cnt(p.cap), c.rec(p.cap), c.gs(p.cap), c.state, p.cap);
    if (const int rc = levels(p.cap, p.M + 1)) return rc;
    finalize();
    return ITD_OK;
}

// The set of states / group sums a decomposition works on: the one the previous call did not use (the NaN-input repeat: the same
// again, its states carry the in_nan flags), initialised by that call's k_finalize unless the bookkeeping says otherwise — a launch of
// its own initialises it then (the device-side repair's k_repair_init: from the other set's final states).  Returns the set.
int claim_state_set(itd_engine *e, int32_t batch, int64_t gs_extent, bool nan_input, bool capturing, const int32_t *repair_need, hipStream_t st)
{
    const int set = nan_input ? e->cur_set : (e->cur_set ^ 1);
    SigState *const state = e->d_state + (size_t)set * e->max_batch;
    int32_t *const gsum = e->d_gsum + (size_t)set * 3 * e->gsum_third;
    if (repair_need || nan_input || capturing || e->dirty_sig[set] > 0 || e->dirty_gs[set] > 0) {
        const int64_t ge = 3 * e->gsum_third;   // the buffers are small: clear all of them
        const int gb = (int)std::min<int64_t>(std::max<int64_t>((ge + 255) / 256, (batch + 255) / 256), 2048);
        if (repair_need) k_repair_init<<<gb, 256, 0, st>>>(e->d_state + (size_t)(set ^ 1) * e->max_batch, state, repair_need, batch, gsum, ge);
        else k_init_state<<<gb, 256, 0, st>>>(state, batch, gsum, ge, nan_input ? 1 : 0);
        e->dirty_sig[set] = std::max(e->dirty_sig[set], batch);
    } else {
        e->dirty_sig[set] = batch;
    }
    e->dirty_gs[set] = gs_extent;
    e->cur_set = set;
    return set;
}

// The record of the call just enqueued (e->last): its arguments, every form off; the caller sets what its form adds
template <typename Tin>
LastCall &record_call(itd_engine *e, const Tin *x, int64_t n, int32_t batch, int64_t x_stride, int32_t M, Rows rows, double *bases,
                      hipStream_t st)
{
    LastCall &c = e->last;
    e->ran = true;
    c.batch = batch; c.m = M; c.n = n; c.stream = st;
    c.x = x; c.x_f32 = sizeof(Tin) == 4; c.x_stride = x_stride; c.rows = rows; c.bases = bases;
    c.fused = c.resident = c.nan_input = c.kf = false;
    return c;
}

template <typename Tin>
int enqueue_decompose(itd_engine *e, const Tin *x, int64_t n, int32_t batch, int64_t x_stride, int32_t M,
                      Rows rows, double *bases_user, hipStream_t st, bool fuse0, bool nan_input = false, bool kf = false,
                      const int32_t *repair_need = nullptr)
{
    // repair_need: the device-side repair of the call just enqueued (itd_set_device_repair): the same call again, level by level,
    // whose launches return at once for every signal that is not flagged (SigState::skip, set by k_repair_init)
    // nan_input: the caller's signal holds a NaN (found by the previous, rejected run of this call): level 0 the way the
    // reference runs it — k_nan_level0 writes the mutated signal (NaN -> +inf, ITD.py:50) into the third baseline slot, which
    // nothing touches before level 2, and the level-0 records; the record-driven level-0 extraction then reads that copy
    if (nan_input) fuse0 = false;
    DecomposePlan<Tin> p;
    p.x = x; p.x_stride = x_stride; p.n = n; p.M = M; p.rows = rows; p.bases = bases_user; p.fuse0 = fuse0; p.nan_input = nan_input;
    // kf: levels L0 .. max_iteration + 1 run fused (itd_knotfirst.hpp): one launch per level only for levels 0 .. L0 - 1
    p.L0 = e->policy.first_level(seq_samples(e, n, batch), M);
    kf = kf && fuse0 && p.L0 >= 2 && p.L0 <= M && n < ((int64_t)1 << 31) - 65536;
    // a call that is being captured into a graph must be complete in itself (the graph may be replayed any number of times) and
    // cannot allocate: a captured call on an engine whose fused workspace does not exist yet runs level by level
    hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap_status);
    const bool capturing = cap_status != hipStreamCaptureStatusNone;
    p.kf_tpw = e->policy.tiles_per_wg();
    if (kf && capturing && ensure_kf_ws(e, p.kf_tpw, false) != ITD_OK) kf = false;
    if (kf) {
        const int rc = ensure_kf_ws(e, p.kf_tpw, true);
        if (rc == ITD_ERR_NOMEM && e->policy.workspace_unavailable()) {
            // no room for the fused levels' workspace (136 B x max_n / 8 + 136 B per tile and level, per signal): this engine stays
            // level by level — the result is the same
            (void)hipGetLastError();
            kf = false;
        } else if (rc) return rc;
    }
    p.kf = kf;
    // capped fused levels: levels L0 .. cap - 1 fused, cap .. M + 1 one launch each behind a scan of the baseline the sample pass leaves
    p.cap = kf ? e->policy.cap(p.L0, M) : 0;
    p.Mk = p.cap ? p.cap - 2 : M;               // the knot side's "max_iteration": its levels are L0 .. Mk + 1
    p.n_tiles = (int)tiles_of(n);
    p.n_groups = groups_of(p.n_tiles);
    p.kf_wgs = (p.n_tiles + p.kf_tpw - 1) / p.kf_tpw;
    p.rows_stride = rows.stride(M, n);

    // instrument every timing_stride-th decomposition only: a launch that carries events needs a completion signal of its own
    // (~2 us per launch, measured), the whole-decomposition span two marker records (~5 us each)
    e->timing_now = e->timing && (e->timing_seq++ % e->timing_stride == 0);
    // the whole-decomposition span: from the first instrumented launch's begin to the last one's end — their dispatches' own
    // timestamps, no marker packets in the stream (two markers cost ~10 us of the instrumented step; k_finalize, not instrumented,
    // lies outside the span of a level-by-level call)
    const int span_pair = time_slot(e, ITD_TIME_DECOMPOSE);
    e->span_first = e->span_last = -1;
    const int64_t gs_extent = (int64_t)batch * p.n_groups * kGsumPitch;
    const int set = claim_state_set(e, batch, gs_extent, nan_input, capturing, repair_need, st);
    p.state = e->d_state + (size_t)set * e->max_batch; p.other_state = e->d_state + (size_t)(set ^ 1) * e->max_batch;
    p.gsum = e->d_gsum + (size_t)set * 3 * e->gsum_third; p.other_gsum = e->d_gsum + (size_t)(set ^ 1) * 3 * e->gsum_third;
    if (bases_user)  // the reference's timeout result keeps an all-zero last baselines row (ITD.py:385,424)
        HIP_TRY(e, hipMemset2DAsync(bases_user + ((int64_t)M + 1) * n, (size_t)p.rows_stride * sizeof(double), 0,
                                    (size_t)n * sizeof(double), (size_t)batch, st));

    // chunks are independent (per-signal state, counts, records, group sums, slots): with two streams they alternate, so that one
    // chunk's launch boundaries and tails overlap the other's work (fork after the init, join before the caller's stream goes on).
    // Streams in use: the caller's and S - 1 of the engine's; signals too long for two of them to share the Infinity Cache (more than
    // 3 * 2^22 samples per chunk) keep to one stream
    p.chunk = chunk_of(e, n, batch);
    const int n_chunks = (batch + p.chunk - 1) / p.chunk;
    p.S = (e->chunk == 0 && (int64_t)p.chunk * n > ((int64_t)3 << 22)) ? 1 : std::min<int>(e->batch_streams, n_chunks);
    if (p.S > 1) {
        if (!e->ev_fork) HIP_TRY(e, hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
        HIP_TRY(e, hipEventRecord(e->ev_fork, st));
        for (int k = 0; k < p.S - 1; ++k) {
            if (!e->aux_stream[k]) {
                HIP_TRY(e, hipStreamCreateWithFlags(&e->aux_stream[k], hipStreamNonBlocking));
                HIP_TRY(e, hipEventCreateWithFlags(&e->ev_join[k], hipEventDisableTiming));
            }
            HIP_TRY(e, hipStreamWaitEvent(e->aux_stream[k], e->ev_fork, 0));
        }
    }
    for (int k = 0; k < n_chunks; ++k) {
        const int b0 = k * p.chunk, lane = k % p.S;
        const int rc = with_row_form(rows, [&](auto form) {
            return run_chunk<decltype(form)>(e, p, b0, std::min(p.chunk, batch - b0), lane == 0 ? st : e->aux_stream[lane - 1]);
        });
        if (rc) return rc;
    }
    for (int k = 0; k < p.S - 1; ++k) {
        HIP_TRY(e, hipEventRecord(e->ev_join[k], e->aux_stream[k]));
        HIP_TRY(e, hipStreamWaitEvent(st, e->ev_join[k], 0));
    }
    // what this call's k_finalize launches leave initialised in the other set
    if (!capturing && batch >= e->dirty_sig[set ^ 1] && gs_extent >= e->dirty_gs[set ^ 1]) {
        e->dirty_sig[set ^ 1] = 0;
        e->dirty_gs[set ^ 1] = 0;
    }
    if (span_pair >= 0) {
        if (e->span_first >= 0) { e->ev_from[(size_t)span_pair] = 2 * e->span_first; e->ev_to[(size_t)span_pair] = 2 * e->span_last + 1; }
        else e->ev_tag[(size_t)span_pair] = -1;           // nothing instrumented in this call
    }
    HIP_TRY(e, hipGetLastError());
    LastCall &c = record_call(e, x, n, batch, x_stride, M, rows, bases_user, st);
    c.fused = fuse0; c.nan_input = nan_input; c.kf = kf; c.kf_level = p.L0; c.kf_cap = kf ? p.cap : 0;
    if (!repair_need) { c.kf_form = kf ? p.L0 : 0; c.kf_cap_form = c.kf_cap; }   // (what itd_get_last_fuse_level / _cap report)
    return ITD_OK;
}

// More than 64 KB of dynamic LDS has to be asked for, per kernel instance: asked once per engine, which remembers the grant
hipError_t allow_lds(itd_engine *e, const void *fn, size_t bytes)
{
    if (std::find(e->lds_fn, e->lds_fn + e->lds_fns, fn) != e->lds_fn + e->lds_fns) return hipSuccess;
    const hipError_t rc = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc == hipSuccess && e->lds_fns < (int)(sizeof(e->lds_fn) / sizeof(e->lds_fn[0]))) e->lds_fn[e->lds_fns++] = fn;
    return rc;
}

// The geometry of the one-workgroup kernels (k_resident, k_stream_levels) for n samples.  cls: four samples per thread, 64 threads up
// to 256 samples ... 1024 threads up to 4096, eight per thread up to 8192 (the per-thread sample loops are unrolled over registers; the
// wider workgroups hide the phases' latencies better).  cw: the window of by-rank knot slots, automatic (0.4 knots per sample) or
// what the caller was told, cut to what fits the LDS
struct WgClass { int cls, threads, cw; size_t lds; };
inline WgClass wg_class(int n, int window = 0)
{
    const int cls = n <= 256 ? 0 : n <= 512 ? 1 : n <= 1024 ? 2 : n <= 2048 ? 3 : n <= 4096 ? 4 : 5;
    int cw = std::min(window > 0 ? window : resident_auto_window(n), resident_pad(n));
    while (resident_lds_bytes(n, cw) > kResidentLdsMax) cw -= 64;
    return {cls, cls == 5 ? 1024 : 64 << cls, cw, resident_lds_bytes(n, cw)};
}

// Short signals (n <= kResidentMax): the whole decomposition as ONE launch, one workgroup per signal, the signal resident
// in LDS (itd_resident.hpp).  Optimistic: the kernel handles finite data only and raises SigState::res_fail
// otherwise; itd_get_summary then repeats the call level by level.  The kernel initialises the states it works on itself
// and leaves the other set's states as k_finalize would (the group sums are not touched).
template <typename Tin>
int enqueue_resident(itd_engine *e, const Tin *x, int64_t n, int32_t batch, int64_t x_stride, int32_t M, Rows rows,
                     double *bases_user, hipStream_t st)
{
    const int64_t R = (int64_t)M + 2;
    const int64_t rows_stride = rows.stride(M, n);      // (the caller's baselines, full calls only, lie R rows apart as well)
    const int set = e->cur_set ^ 1;
    SigState *const set_state = e->d_state + (size_t)set * e->max_batch;
    SigState *const other_state = e->d_state + (size_t)(set ^ 1) * e->max_batch;
    if (bases_user)  // the reference's timeout result keeps an all-zero last baselines row (ITD.py:385,424)
        HIP_TRY(e, hipMemset2DAsync(bases_user + (R - 1) * n, (size_t)rows_stride * sizeof(double), 0,
                                    (size_t)n * sizeof(double), (size_t)batch, st));
    const WgClass wc = wg_class((int)n, e->resident_window);
    const void *fn = nullptr;
    (void)with_row_form(rows, [&](auto form) {
        using Trow = typename decltype(form)::Trow;
        constexpr bool SEL = decltype(form)::SEL;
        const void *const by_class[6] = {
            reinterpret_cast<const void *>(&k_resident<Tin, 64, 4, Trow, SEL>),   reinterpret_cast<const void *>(&k_resident<Tin, 128, 4, Trow, SEL>),
            reinterpret_cast<const void *>(&k_resident<Tin, 256, 4, Trow, SEL>),  reinterpret_cast<const void *>(&k_resident<Tin, 512, 4, Trow, SEL>),
            reinterpret_cast<const void *>(&k_resident<Tin, 1024, 4, Trow, SEL>), reinterpret_cast<const void *>(&k_resident<Tin, 1024, 8, Trow, SEL>)};
        fn = by_class[wc.cls];
        return ITD_OK;
    });
    const hipError_t arc = allow_lds(e, fn, kResidentLdsMax);
    if (arc != hipSuccess) {     // a device / runtime that does not grant it: this engine runs level by level from now on
        (void)hipGetLastError();
        if (e->policy.resident_mode == ITD_RESIDENT_ONLY) return fail_hip(e, arc, "hipFuncSetAttribute(k_resident, MaxDynamicSharedMemorySize)");
        e->policy.resident_unavailable();
        return enqueue_decompose<Tin>(e, x, n, batch, x_stride, M, rows, bases_user, st, e->policy.level0_fused());
    }
    const Tin *a_x = x; int64_t a_xs = x_stride, a_rs = rows_stride, a_bs = rows_stride;
    int a_n = (int)n, a_m = M, a_cw = wc.cw, a_nf = e->nan_input_mode == ITD_NAN_INPUT_FOLLOW ? 1 : 0;
    void *a_rows = rows.p; double *a_bases = bases_user;
    SigState *a_st = set_state, *a_ot = other_state; RowSel a_sel = rows.which;
    void *args[] = {&a_x, &a_xs, &a_n, &a_m, &a_cw, &a_nf, &a_rows, &a_rs, &a_bases, &a_bs, &a_st, &a_ot, &a_sel};
    HIP_TRY(e, hipLaunchKernel(fn, dim3((unsigned)batch), dim3((unsigned)wc.threads), args, wc.lds, st));
    HIP_TRY(e, hipGetLastError());
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap);
    e->dirty_sig[set] = std::max(e->dirty_sig[set], batch);
    if (cap == hipStreamCaptureStatusNone && batch >= e->dirty_sig[set ^ 1]) e->dirty_sig[set ^ 1] = 0;
    e->cur_set = set;
    record_call(e, x, n, batch, x_stride, M, rows, bases_user, st).resident = true;
    e->last.kf_form = 0;
    return ITD_OK;
}

template <typename Tin>
int enqueue_any(itd_engine *e, const Tin *x, int64_t n, int32_t batch, int64_t x_stride, int32_t M, Rows rows,
                double *bases_user, hipStream_t st)
{
    int rc;
    if (e->policy.resident(n <= kResidentMax, e->timing)) rc = enqueue_resident<Tin>(e, x, n, batch, x_stride, M, rows, bases_user, st);
    else {
        const bool f0 = e->policy.level0_fused();
        rc = enqueue_decompose<Tin>(e, x, n, batch, x_stride, M, rows, bases_user, st, f0, false,
                                    e->policy.fused_levels(n, seq_samples(e, n, batch), M, f0));
    }
    e->last_device_repair = false;
    if (rc || (!e->valid_dev && !e->device_repair)) return rc;
    // ---- behind the call's last launch: the verdict on the device (and, if asked for, the repair) ----
    const int vb = (batch + 63) / 64;
    SigState *state_a = e->d_state + (size_t)e->cur_set * e->max_batch;
    int32_t *valid = e->valid_dev ? e->valid_dev : e->d_valid_own;
    const int follow = e->nan_input_mode == ITD_NAN_INPUT_FOLLOW ? 1 : 0;
    k_verdict<<<vb, 64, 0, st>>>(state_a, batch, e->last.kf ? e->kf.sig : nullptr, e->last.kf_level, follow, valid, e->device_repair ? e->d_need : nullptr);
    if (e->device_repair) {
        // the same call level by level (record-driven level 0: any knot spacing), guarded per signal by d_need: rows_dev is final
        // when the stream has drained, with no host synchronisation in between
        rc = enqueue_decompose<Tin>(e, x, n, batch, x_stride, M, rows, bases_user, st, false, false, false, e->d_need);
        if (rc) return rc;
        k_verdict_repaired<<<vb, 64, 0, st>>>(e->d_state + (size_t)e->cur_set * e->max_batch, batch, e->d_need, follow, valid);
        e->last_device_repair = true;
    }
    HIP_TRY(e, hipGetLastError());
    return ITD_OK;
}

int check_args(itd_engine *e, const void *x, int64_t n, int32_t batch, int64_t x_stride, int32_t M, const void *rows)
{
    if (!e || !x || !rows) return ITD_ERR_INVALID_ARG;
    if (n < 3 || n > e->max_n || n >= (int64_t)INT32_MAX) return ITD_ERR_INVALID_ARG;  // N < 3: ITD.py:42-43 is garbage
    if (batch < 1 || batch > e->max_batch) return ITD_ERR_INVALID_ARG;   // any size: batches run in chunks of <= 65535 signals
    if (batch > 1 && x_stride < n) return ITD_ERR_INVALID_ARG;
    if (M < 0 || M > ITD_MAX_ITERATION) return ITD_ERR_INVALID_ARG;  // row M+1 must fit in 22 rows (ITD.py:384,421)
    return ITD_OK;
}

// a selection of rows (itd_decompose_select_*): rotation bits within 0 .. M, the residual flag 0 or 1, one row at least
// and the row type 0 (float64) or 1 (float32).  What the select entries, device and host, test before they look at anything else
bool selection_ok(int32_t M, uint32_t mask, int32_t want_residual, int32_t rows_f32)
{
    if (M < 0 || M > ITD_MAX_ITERATION || (mask >> (M + 1)) != 0 || (rows_f32 != 0 && rows_f32 != 1)) return false;
    return (want_residual == 0 || want_residual == 1) && (mask != 0 || want_residual == 1);
}

// The body of the six device entries (itd_decompose_*_f32 / _f64): they differ in the Rows they describe
template <typename Tin>
int decompose_dev(itd_engine *e, const Tin *x_dev, int64_t n, int32_t batch, int64_t x_stride, int32_t M, Rows rows, double *bases_dev,
                  void *stream)
{
    const int rc = check_args(e, x_dev, n, batch, x_stride, M, rows.p);
    if (rc) return rc;
    DevGuard g(e->device);
    return enqueue_any<Tin>(e, x_dev, n, batch, x_stride, M, rows, bases_dev, stream_of(e, stream));
}

// a grow-only buffer of the engine made to hold `want` bytes (Buf::reserve), the engine's error text set when that fails
template <typename Tp>
int grow(itd_engine *e, Buf<Tp> &b, size_t want)
{
    hipError_t why = hipSuccess;
    if (b.reserve(want, &why)) { fail_hip(e, why, "hipMalloc(io)"); return ITD_ERR_NOMEM; }
    return ITD_OK;
}

// Device -> pageable host memory for the host-form calls (numpy in, numpy out).  hipMemcpy into pageable memory stages through
// the runtime's own pinned buffer and one host thread moves the bytes on (~12 GB/s measured: the 1.2 GB of rows of a 2^24-sample
// decomposition took 100 ms for 0.56 ms of compute).  Here: DMA into one of two pinned bounce buffers while a few host threads copy
// the other one into the caller's array (and take its first-touch page faults in parallel).
constexpr size_t kPinBytes = (size_t)16 << 20;
constexpr int kCopyThreads = 4;
int copy_to_host(itd_engine *e, void *dst_host, const void *src_dev, size_t bytes, hipStream_t st)
{
    if (bytes < 4 * kPinBytes) {   // small: the plain path
        HIP_TRY(e, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(e, hipStreamSynchronize(st));
        return ITD_OK;
    }
    for (int k = 0; k < 2; ++k)
        if (!e->h_pin[k] && e->h_pin[k].alloc(kPinBytes) != hipSuccess) {   // no pinned memory to be had: the plain path
            HIP_TRY(e, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, st));
            HIP_TRY(e, hipStreamSynchronize(st));
            return ITD_OK;
        }
    const size_t n_chunks = (bytes + kPinBytes - 1) / kPinBytes;
    std::atomic<size_t> ready{0};                       // chunks whose DMA has completed
    std::unique_ptr<std::atomic<int>[]> done(new (std::nothrow) std::atomic<int>[n_chunks]);   // host threads done with chunk k
    if (!done) {
        HIP_TRY(e, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(e, hipStreamSynchronize(st));
        return ITD_OK;
    }
    for (size_t k = 0; k < n_chunks; ++k) done[k].store(0, std::memory_order_relaxed);
    std::atomic<bool> abort_copy{false};
    auto worker = [&](int tix) {
        for (size_t k = 0; k < n_chunks; ++k) {
            while (ready.load(std::memory_order_acquire) <= k) {
                if (abort_copy.load(std::memory_order_relaxed)) return;
                std::this_thread::yield();
            }
            const size_t len = std::min(kPinBytes, bytes - k * kPinBytes);
            const size_t per = ((len + kCopyThreads - 1) / kCopyThreads + 63) & ~(size_t)63;
            const size_t lo = std::min(len, per * (size_t)tix), hi = std::min(len, lo + per);
            if (hi > lo) memcpy((char *)dst_host + k * kPinBytes + lo, (const char *)e->h_pin[k & 1] + lo, hi - lo);
            done[k].fetch_add(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> pool;
    try {   // nothing may be thrown across the C ABI: without its host threads the copy takes the plain path
        pool.reserve(kCopyThreads);
        for (int t = 0; t < kCopyThreads; ++t) pool.emplace_back(worker, t);
    } catch (...) {
        abort_copy.store(true);
        for (auto &t : pool) t.join();
        HIP_TRY(e, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(e, hipStreamSynchronize(st));
        return ITD_OK;
    }
    hipError_t rc = hipSuccess;
    for (size_t k = 0; k < n_chunks && rc == hipSuccess; ++k) {
        if (k >= 2)   // the bounce buffer is free again once every host thread has copied chunk k-2 out of it
            while (done[k - 2].load(std::memory_order_acquire) < kCopyThreads) std::this_thread::yield();
        const size_t len = std::min(kPinBytes, bytes - k * kPinBytes);
        rc = hipMemcpyAsync(e->h_pin[k & 1], (const char *)src_dev + k * kPinBytes, len, hipMemcpyDeviceToHost, st);
        if (rc == hipSuccess) rc = hipStreamSynchronize(st);
        if (rc == hipSuccess) ready.store(k + 1, std::memory_order_release);
    }
    if (rc != hipSuccess) abort_copy.store(true);
    for (auto &t : pool) t.join();
    if (rc != hipSuccess) return fail_hip(e, rc, "copy_to_host");
    return ITD_OK;
}

}  // namespace

extern "C" {

int itd_abi_version(void) { return ITD_ABI_VERSION; }

const char *itd_status_string(int s)
{
    switch (s) {
        case ITD_OK: return "ok";
        case ITD_ERR_INVALID_ARG: return "invalid argument";
        case ITD_ERR_NO_DEVICE: return "no HIP device";
        case ITD_ERR_HIP: return "HIP runtime error";
        case ITD_ERR_NOMEM: return "out of memory";
        case ITD_ERR_NOT_RUN: return "no decomposition has been run";
        case ITD_ERR_NONFINITE: return "NaN in the input (rejected by this operator / mode)";
        default: return "unknown status";
    }
}

const char *itd_last_error(const itd_engine *e) { return e ? e->err : "null engine"; }

int itd_engine_create(itd_engine **out, int device_id, int64_t max_n, int32_t max_batch)
{
    if (!out || max_n < 3 || max_batch < 1 || max_n >= (int64_t)INT32_MAX) return ITD_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) return ITD_ERR_NO_DEVICE;
    itd_engine *e = new (std::nothrow) itd_engine();
    if (!e) return ITD_ERR_NOMEM;
    e->device = device_id;
    e->max_n = max_n;
    e->max_batch = max_batch;
    e->max_tiles = tiles_of(max_n);
    DevGuard g(device_id);
    const size_t B = (size_t)max_batch;
    const int max_groups = groups_of((int)e->max_tiles);
    e->tiles_half = (int64_t)B * e->max_tiles;
    e->gsum_third = (int64_t)B * max_groups * kGsumPitch;
    hipError_t rc = hipSuccess;
    auto alloc = [&](auto &buf, size_t bytes) { if (rc == hipSuccess) rc = buf.alloc(bytes, &e->ws_total); };   // counted
    alloc(e->d_lists, (size_t)e->max_tiles * T * sizeof(int32_t));   // API helpers only (one signal)
    alloc(e->d_counts, 2 * (size_t)e->tiles_half * sizeof(int32_t));
    alloc(e->d_recs, 2 * (size_t)e->tiles_half * sizeof(TileRec));
    alloc(e->d_gsum, 2 * 3 * (size_t)e->gsum_third * sizeof(int32_t));
    alloc(e->d_kidx, (size_t)(max_n + 2) * sizeof(int32_t));
    alloc(e->d_total, 64);
    e->pp_pitch = max_n + kSlotPad;
    alloc(e->d_pp, B * 3 * (size_t)e->pp_pitch * sizeof(double));
    alloc(e->d_state, 2 * B * sizeof(SigState));
    e->dirty_sig[0] = e->dirty_sig[1] = max_batch;       // nothing is initialised yet
    e->dirty_gs[0] = e->dirty_gs[1] = e->gsum_third;
    e->hgsum_third = (int64_t)max_groups * kGsumPitch;
    alloc(e->d_hcounts, 2 * (size_t)e->max_tiles * sizeof(int32_t));
    alloc(e->d_hrecs, 2 * (size_t)e->max_tiles * sizeof(TileRec));
    alloc(e->d_hgsum, 3 * (size_t)e->hgsum_third * sizeof(int32_t));
    alloc(e->d_hstate, sizeof(SigState));
    alloc(e->d_flag, 64);
    alloc(e->d_need, sizeof(int32_t) * (size_t)max_batch);
    alloc(e->d_valid_own, sizeof(int32_t) * (size_t)max_batch);
    if (rc == hipSuccess) rc = e->h_state.alloc(B * sizeof(SigState));
    if (rc == hipSuccess) rc = hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking);
    if (rc != hipSuccess) {
        const bool oom = (rc == hipErrorOutOfMemory);
        itd_engine_destroy(e);
        return oom ? ITD_ERR_NOMEM : ITD_ERR_HIP;
    }
    *out = e;
    return ITD_OK;
}

void itd_engine_destroy(itd_engine *e)
{
    if (!e) return;
    DevGuard g(e->device);
    if (e->own_stream) (void)hipStreamSynchronize(e->own_stream);
    for (auto ev : e->ev) if (ev) (void)hipEventDestroy(ev);
    if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
    for (int k = 0; k < 3; ++k) {
        if (e->aux_stream[k]) { (void)hipStreamSynchronize(e->aux_stream[k]); (void)hipStreamDestroy(e->aux_stream[k]); }
        if (e->ev_join[k]) (void)hipEventDestroy(e->ev_join[k]);
    }
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    delete e;   // (its buffers free themselves: here, with the engine's device current and its streams drained)
}

int64_t itd_engine_workspace_bytes(const itd_engine *e) { return e ? e->ws_total : 0; }

// ---- plain device-memory helpers: a host binding that owns no GPU allocator of its own (numpy callers, the C client) ----
int itd_dev_alloc(int device_id, int64_t bytes, void **out)
{
    if (!out || bytes <= 0) return ITD_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return ITD_ERR_NO_DEVICE;
    DevGuard g(device_id);
    const hipError_t rc = hipMalloc(out, (size_t)bytes);
    if (rc == hipErrorOutOfMemory) return ITD_ERR_NOMEM;
    return rc == hipSuccess ? ITD_OK : ITD_ERR_HIP;
}

int itd_dev_free(int device_id, void *p)
{
    if (!p) return ITD_OK;
    DevGuard g(device_id);
    return hipFree(p) == hipSuccess ? ITD_OK : ITD_ERR_HIP;
}

int itd_dev_copy(int device_id, void *dst, const void *src, int64_t bytes, int32_t to_device)
{
    if (!dst || !src || bytes < 0) return ITD_ERR_INVALID_ARG;
    DevGuard g(device_id);
    // Ordered against EVERYTHING on the device, whatever stream it was enqueued on: the engines' own streams are non-blocking
    // (no implicit ordering with the null stream this copy uses), and a caller of this plain helper expects "after what I
    // launched, before what I launch next"
    if (hipDeviceSynchronize() != hipSuccess) return ITD_ERR_HIP;
    return hipMemcpy(dst, src, (size_t)bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost) == hipSuccess
               ? ITD_OK : ITD_ERR_HIP;
}
int itd_engine_device(const itd_engine *e) { return e ? e->device : -1; }

// ---- sharding a batch of independent signals over the GPUs of a node, for hosts without torch.distributed ----
int itd_shard_range(int64_t batch, int32_t world, int32_t rank, int64_t *lo, int64_t *hi)
{
    if (batch < 0 || world < 1 || rank < 0 || rank >= world || !lo || !hi) return ITD_ERR_INVALID_ARG;
    const int64_t q = batch / world, r = batch % world;
    *lo = (int64_t)rank * q + std::min<int64_t>(rank, r);
    *hi = *lo + q + (rank < r ? 1 : 0);
    return ITD_OK;
}

namespace {
// RCCL's point-to-point entry points, resolved at the first scatter (the library does not link against librccl: a single-GPU
// host never needs it)
struct RcclApi {
    int (*send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*group_start)() = nullptr;
    int (*group_end)() = nullptr;
    bool tried = false, ok = false;
};
RcclApi g_rccl;
bool rccl_load()
{
    if (g_rccl.tried) return g_rccl.ok;
    g_rccl.tried = true;
    void *h = nullptr;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
        h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
    }
    if (!h) return false;
    g_rccl.send = reinterpret_cast<decltype(g_rccl.send)>(dlsym(h, "ncclSend"));
    g_rccl.recv = reinterpret_cast<decltype(g_rccl.recv)>(dlsym(h, "ncclRecv"));
    g_rccl.group_start = reinterpret_cast<decltype(g_rccl.group_start)>(dlsym(h, "ncclGroupStart"));
    g_rccl.group_end = reinterpret_cast<decltype(g_rccl.group_end)>(dlsym(h, "ncclGroupEnd"));
    g_rccl.ok = g_rccl.send && g_rccl.recv && g_rccl.group_start && g_rccl.group_end;
    return g_rccl.ok;
}
}  // namespace

int itd_shard_scatter(const void *x_root_dev, void *x_local_dev, int64_t n, int64_t batch, int32_t elem_bytes, int32_t world,
                      int32_t rank, int32_t root, void *nccl_comm, void *stream)
{
    int64_t lo = 0, hi = 0;
    if (n < 1 || (elem_bytes != 4 && elem_bytes != 8) || root < 0 || root >= world || itd_shard_range(batch, world, rank, &lo, &hi)) return ITD_ERR_INVALID_ARG;
    if ((rank == root && !x_root_dev) || (hi > lo && !x_local_dev)) return ITD_ERR_INVALID_ARG;
    const hipStream_t st = (hipStream_t)stream;
    const size_t row = (size_t)n * (size_t)elem_bytes;
    if (rank == root && hi > lo && x_local_dev != static_cast<const char *>(x_root_dev) + (size_t)lo * row)      // the root's own shard: a local copy
        if (hipMemcpyAsync(x_local_dev, static_cast<const char *>(x_root_dev) + (size_t)lo * row, (size_t)(hi - lo) * row, hipMemcpyDeviceToDevice, st) != hipSuccess)
            return ITD_ERR_HIP;
    if (world == 1) return ITD_OK;
    if (!nccl_comm) return ITD_ERR_INVALID_ARG;
    if (!rccl_load()) return ITD_ERR_NO_DEVICE;            // no RCCL library on this host
    // one group of point-to-point transfers: every link of the root busy at once (xGMI is point to point), bytes as ncclChar (= 0)
    if (g_rccl.group_start()) return ITD_ERR_HIP;
    int rc = 0;
    if (rank == root) {
        for (int r = 0; r < world && !rc; ++r) {
            int64_t l = 0, h = 0;
            (void)itd_shard_range(batch, world, r, &l, &h);
            if (r != root && h > l) rc = g_rccl.send(static_cast<const char *>(x_root_dev) + (size_t)l * row, (size_t)(h - l) * row, 0, r, nccl_comm, st);
        }
    } else if (hi > lo) {
        rc = g_rccl.recv(x_local_dev, (size_t)(hi - lo) * row, 0, root, nccl_comm, st);
    }
    const int rc_end = g_rccl.group_end();
    return (rc || rc_end) ? ITD_ERR_HIP : ITD_OK;
}

int itd_decompose_f32(itd_engine *e, const float *x_dev, int64_t n, int32_t batch, int64_t x_stride,
                      int32_t max_iteration, double *rows_dev, double *baselines_dev, void *stream)
{
    return decompose_dev(e, x_dev, n, batch, x_stride, max_iteration, Rows(rows_dev), baselines_dev, stream);
}

int itd_decompose_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride,
                      int32_t max_iteration, double *rows_dev, double *baselines_dev, void *stream)
{
    return decompose_dev(e, x_dev, n, batch, x_stride, max_iteration, Rows(rows_dev), baselines_dev, stream);
}

// float32 rows: the same call in every respect, each row element the float64 one rounded once at its store; no caller's baselines
int itd_decompose_rows32_f32(itd_engine *e, const float *x_dev, int64_t n, int32_t batch, int64_t x_stride,
                             int32_t max_iteration, float *rows_dev, void *stream)
{
    return decompose_dev(e, x_dev, n, batch, x_stride, max_iteration, Rows(rows_dev), nullptr, stream);
}

int itd_decompose_rows32_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride,
                             int32_t max_iteration, float *rows_dev, void *stream)
{
    return decompose_dev(e, x_dev, n, batch, x_stride, max_iteration, Rows(rows_dev), nullptr, stream);
}

// selected rows: the same call in every respect, each selected row's elements those of the full call; the rest is stored nowhere
int itd_decompose_select_f32(itd_engine *e, const float *x_dev, int64_t n, int32_t batch, int64_t x_stride, int32_t max_iteration,
                             uint32_t rotation_mask, int32_t want_residual, void *rows_dev, int32_t rows_f32, void *stream)
{
    if (!selection_ok(max_iteration, rotation_mask, want_residual, rows_f32)) return ITD_ERR_INVALID_ARG;
    return decompose_dev(e, x_dev, n, batch, x_stride, max_iteration, Rows(rows_dev, rows_f32 != 0, rotation_mask, want_residual != 0), nullptr, stream);
}

int itd_decompose_select_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride, int32_t max_iteration,
                             uint32_t rotation_mask, int32_t want_residual, void *rows_dev, int32_t rows_f32, void *stream)
{
    if (!selection_ok(max_iteration, rotation_mask, want_residual, rows_f32)) return ITD_ERR_INVALID_ARG;
    return decompose_dev(e, x_dev, n, batch, x_stride, max_iteration, Rows(rows_dev, rows_f32 != 0, rotation_mask, want_residual != 0), nullptr, stream);
}

namespace {
// The recorded call `c` again, level by level unless fuse0, on its signals b0 .. b0 + batch - 1 into their rows (and baselines)
int enqueue_again(itd_engine *e, const LastCall c, int b0, int32_t batch, bool fuse0, bool nan_input)
{
    const int64_t rs = c.rows.stride(c.m, c.n);      // (the caller's baselines come with full calls only: the same stride)
    const Rows rows = c.rows.at((int64_t)b0 * rs); double *bases = c.bases ? c.bases + (int64_t)b0 * rs : nullptr;
    return c.x_f32 ? enqueue_decompose<float>(e, (const float *)c.x + (int64_t)b0 * c.x_stride, c.n, batch, c.x_stride, c.m, rows, bases, c.stream, fuse0, nan_input)
                   : enqueue_decompose<double>(e, (const double *)c.x + (int64_t)b0 * c.x_stride, c.n, batch, c.x_stride, c.m, rows, bases, c.stream, fuse0, nan_input);
}

// The signals of the last call whose fused levels reported a failure (h_state[b].kf_fail), each run again on its own: level by level,
// record-driven level 0, into its own rows (and baselines) of the caller's buffers; its state replaces h_state[b].  The engine's
// record of the last call (what a later itd_get_summary, itd_get_timing, ... refer to) is put back afterwards.
int repair_signals(itd_engine *e, int B)
{
    const LastCall keep = e->last;
    const bool keep_timing = e->timing;
    const int main_set = e->cur_set;
    const int64_t main_gs = e->dirty_gs[main_set];
    e->timing = false;                       // (the repairs are not part of any timed launch class)
    int rc = ITD_OK;
    for (int b = 0; b < B && rc == ITD_OK; ++b) {
        if (!e->h_state[b].kf_fail) continue;
        rc = enqueue_again(e, keep, b, 1, false, false);
        if (rc) break;
        // (stream ordered: the copy leaves before the next repair's last launch puts this state set back into its initial state)
        if (hipMemcpyAsync(&e->h_state[b], e->d_state + (size_t)e->cur_set * e->max_batch, sizeof(SigState), hipMemcpyDeviceToHost, keep.stream) != hipSuccess) { rc = ITD_ERR_HIP; break; }
        ++e->policy.fuse_signal_repairs;
    }
    if (hipStreamSynchronize(keep.stream) != hipSuccess && rc == ITD_OK) rc = ITD_ERR_HIP;
    e->timing = keep_timing;
    // The call's state set on the device becomes what the host now knows (fused verdicts and repaired signals merged), and the
    // engine's current set again: a later itd_get_summary of this call reads it as it stands (last.kf = false: nothing left to
    // draw or repair); the other set was last used by a one-signal repair.
    if (rc == ITD_OK) {
        for (int b = 0; b < B; ++b) e->h_state[b].kf_fail = 0;
        if (hipMemcpyAsync(e->d_state + (size_t)main_set * e->max_batch, e->h_state, sizeof(SigState) * (size_t)B, hipMemcpyHostToDevice, keep.stream) != hipSuccess ||
            hipStreamSynchronize(keep.stream) != hipSuccess) rc = ITD_ERR_HIP;
    }
    e->cur_set = main_set;
    e->dirty_sig[main_set] = std::max(e->dirty_sig[main_set], keep.batch);
    e->dirty_sig[main_set ^ 1] = std::max(e->dirty_sig[main_set ^ 1], 1);
    e->dirty_gs[main_set] = std::max(e->dirty_gs[main_set], main_gs);
    e->dirty_gs[main_set ^ 1] = std::max<int64_t>(e->dirty_gs[main_set ^ 1], (int64_t)groups_of((int)tiles_of(keep.n)) * kGsumPitch);
    e->last = keep;            // (kf_cap keeps the fused call's cap: unread once kf is false)
    e->last.kf = false;
    e->last.kf_cap_form = 0;   // (as the repairs left it: itd_get_last_fuse_cap reports 0 after a summary that repaired signals)
    return rc;
}

// ---- the steps of itd_get_summary, in its order; each returns ITD_OK or the error that ends the summary ----

// The signals' states of the last call, and the verdict of its fused sparse levels drawn from the heads of their KfSig into the
// states as the host sees them (no launch of its own behind the sample pass)
int read_states(itd_engine *e, int B)
{
    HIP_TRY(e, hipMemcpyAsync(e->h_state, e->d_state + (size_t)e->cur_set * e->max_batch, sizeof(SigState) * (size_t)B, hipMemcpyDeviceToHost, e->last.stream));
    if (e->last.kf) {
        if (!e->h_kf) HIP_TRY(e, e->h_kf.alloc(kKfSigHead * (size_t)e->max_batch));
        HIP_TRY(e, hipMemcpy2DAsync(e->h_kf, kKfSigHead, e->kf.sig, sizeof(KfSig), kKfSigHead, (size_t)B, hipMemcpyDeviceToHost, e->last.stream));
    }
    HIP_TRY(e, hipStreamSynchronize(e->last.stream));
    KfSig ks;
    for (int b = 0; e->last.kf && b < B; ++b) { memcpy(&ks, e->h_kf + (size_t)b * kKfSigHead, kKfSigHead); kf_sig_verdict(ks, e->last.kf_level, e->h_state[b]); }
    return ITD_OK;
}

// The call carried its own repair (itd_set_device_repair): nothing to repeat here; count what it re-ran and let the policy learn
void count_device_repairs(itd_engine *e, int B)
{
    if (!e->last_device_repair) return;
    int fixed = 0, why = 0;
    for (int b = 0; b < B; ++b) if (e->h_state[b].skip < 0) { ++fixed; why |= -e->h_state[b].skip; }
    e->last_device_repair = false;      // (a second summary of the same call counts nothing)
    e->policy.device_repaired(fixed, why, FormPolicy::many(fixed, B), e->last.kf_level);
}

// the same call again, whole, and its states read back
int repeat_call(itd_engine *e, int B, bool fuse0, bool nan_input)
{
    const int rc = enqueue_again(e, e->last, 0, B, fuse0, nan_input);
    if (rc) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->h_state, e->d_state + (size_t)e->cur_set * e->max_batch, sizeof(SigState) * (size_t)B, hipMemcpyDeviceToHost, e->last.stream));
    HIP_TRY(e, hipStreamSynchronize(e->last.stream));
    return ITD_OK;
}

// The one-workgroup form handles finite data only: a NaN / infinity in the input or in a baseline (a leading or trailing plateau,
// ITD.py:115-116) raised res_fail.  Repeat the call level by level — those kernels carry the reference's NaN rules.
int repeat_resident(itd_engine *e, int B)
{
    if (!e->last.resident) return ITD_OK;
    if (!std::any_of(e->h_state.get(), e->h_state + B, [](const SigState &s) { return s.res_fail != 0; })) return ITD_OK;
    if (!e->policy.resident_failed()) {
        snprintf(e->err, sizeof(e->err), "resident form: a non-finite sample or baseline (ITD_RESIDENT_ONLY forbids the level-by-level repeat)");
        return ITD_ERR_HIP;
    }
    return repeat_call(e, B, e->policy.level0_fused(), false);
}

// A signal of the call holds a NaN.  The reference runs such input through detect_peaks' NaN branch and overwrites the NaNs with
// +inf (ITD.py:46-51, 64-68); the launches so far evaluated plain rules.  Repeat the call with the level 0 that follows the
// reference (k_nan_level0); SigState::in_nan stays set and tells it which signals are concerned.
int repeat_nan_input(itd_engine *e, int B)
{
    if (e->last.nan_input || e->nan_input_mode != ITD_NAN_INPUT_FOLLOW) return ITD_OK;
    const bool any = std::any_of(e->h_state.get(), e->h_state + B, [](const SigState &s) { return s.in_nan != 0; });
    return any ? repeat_call(e, B, false, true) : ITD_OK;
}

// The fused sparse levels deliver the reference's result or report that they cannot (SigState::kf_fail: the sample pass found a
// knot the knot side had missed, a list / table outgrew its workspace, non-finite knot data, too many exact ties).  A few signals of
// a batch: each of them is run again on its own, level by level (record-driven level 0: any knot spacing), into its rows — the rest
// of the batch keeps its fused result.  Many, or a single signal: the whole call is repeated level by level.
int settle_fused_levels(itd_engine *e, int B)
{
    if (!e->last.kf) return ITD_OK;
    int nfail = 0, bits = 0, fail_lev = 99;
    for (int b = 0; b < B; ++b) {
        if (!e->h_state[b].kf_fail) continue;
        ++nfail;
        bits |= e->h_state[b].kf_fail;
        fail_lev = std::min<int>(fail_lev, reinterpret_cast<const KfSig *>(e->h_kf + (size_t)b * kKfSigHead)->fail_lev);
    }
    if (!nfail) { e->policy.fused_levels_delivered(e->last.kf_cap != 0, e->last.m); return ITD_OK; }
    const auto what = e->policy.fused_levels_refused(bits, fail_lev, e->last.kf_level, e->last.kf_cap, e->last.m, FormPolicy::many(nfail, B));
    if (what == FormPolicy::Refusal::Fail) {
        snprintf(e->err, sizeof(e->err), "fused sparse levels: not the reference's result (fail bits 0x%x: 1 verification, 2 capacity, 4 non-finite, 16 halo wait); ITD_FUSE_ONLY forbids the level-by-level repeat", bits);
        return ITD_ERR_HIP;
    }
    return what == FormPolicy::Refusal::RepairSignals ? repair_signals(e, B) : repeat_call(e, B, e->policy.level0_fused(), false);
}

// The fused level-0 launch reaches kReach windows beyond a tile for its halo knots; a signal smoother than that (knots more than
// ~4000 samples apart at level 0) raised l0_fail: repeat the call record-driven (k_scan0 + records)
int repeat_level0(itd_engine *e, int B)
{
    if (!e->last.fused) return ITD_OK;
    if (!std::any_of(e->h_state.get(), e->h_state + B, [](const SigState &s) { return s.l0_fail && !s.in_nan; })) return ITD_OK;
    if (!e->policy.level0_fell_short()) {
        snprintf(e->err, sizeof(e->err), "fused level 0: a tile's halo knots lie beyond its reach (ITD_LEVEL0_FUSED forbids the record-driven repeat)");
        return ITD_ERR_HIP;
    }
    return repeat_call(e, B, false, false);
}

void fill_summary(const itd_engine *e, int B, int32_t *n_rows, int32_t *n_baselines, int32_t *stop_reason, int64_t *knot_counts,
                  int32_t *nan_levels)
{
    for (int b = 0; b < B; ++b) {
        const SigState &s = e->h_state[b];
        // ITD.py:404-416, counter = stop_level-1: rows[0:counter+1], baselines[0:counter-1] after the increment;
        // ITD.py:418-426, counter = max_iteration+1: rows and baselines[0:counter] (last row zero)
        const int rows = s.fin_stopped ? s.fin_stop_level : e->last.m + 2;
        if (n_rows) n_rows[b] = rows;
        if (n_baselines) n_baselines[b] = s.fin_stopped ? rows - 1 : rows;
        if (stop_reason) stop_reason[b] = s.fin_stopped ? ITD_STOP_NATURAL : ITD_STOP_TIMEOUT;
        if (knot_counts)
            for (int j = 0; j <= ITD_MAX_ROWS; ++j) knot_counts[(size_t)b * (ITD_MAX_ROWS + 1) + j] = s.m[j];
        if (nan_levels) nan_levels[b] = (s.in_nan && !e->last.nan_input) ? -2 : -1;
    }
}
}  // namespace

int itd_get_summary(itd_engine *e, int32_t *n_rows, int32_t *n_baselines, int32_t *stop_reason,
                    int64_t *knot_counts, int32_t *nan_levels)
{
    if (!e) return ITD_ERR_INVALID_ARG;
    if (!e->ran) return ITD_ERR_NOT_RUN;
    DevGuard g(e->device);
    const int B = e->last.batch;
    int rc = read_states(e, B);
    if (rc) return rc;
    count_device_repairs(e, B);
    // each repeat also lets the engine's next calls start the way it runs: workloads tend to be homogeneous
    if ((rc = repeat_resident(e, B)) || (rc = repeat_nan_input(e, B)) || (rc = settle_fused_levels(e, B)) || (rc = repeat_level0(e, B)))
        return rc;
    fill_summary(e, B, n_rows, n_baselines, stop_reason, knot_counts, nan_levels);
    return ITD_OK;
}

int itd_set_level0_mode(itd_engine *e, int32_t mode)
{
    if (!e || mode < ITD_LEVEL0_AUTO || mode > ITD_LEVEL0_FUSED) return ITD_ERR_INVALID_ARG;
    e->policy.set_level0_mode(mode);
    return ITD_OK;
}

int itd_set_nan_input_mode(itd_engine *e, int32_t mode)
{
    if (!e || (mode != ITD_NAN_INPUT_FOLLOW && mode != ITD_NAN_INPUT_REJECT)) return ITD_ERR_INVALID_ARG;
    e->nan_input_mode = mode;
    return ITD_OK;
}

int itd_set_host_keep_baselines(itd_engine *e, int32_t enable)
{
    if (!e) return ITD_ERR_INVALID_ARG;
    e->host_keep_bases = enable != 0;
    if (!enable) e->kept_nb = -1;
    return ITD_OK;
}

int itd_get_last_baselines_host(itd_engine *e, double *baselines_host, int64_t n, int32_t n_baselines)
{
    if (!e || (!baselines_host && n_baselines > 0)) return ITD_ERR_INVALID_ARG;
    if (e->kept_nb < 0) return ITD_ERR_NOT_RUN;
    if (n != e->kept_n || n_baselines != e->kept_nb) return ITD_ERR_INVALID_ARG;
    if (n_baselines == 0) return ITD_OK;
    DevGuard g(e->device);
    return copy_to_host(e, baselines_host, e->d_io_bases, (size_t)n_baselines * (size_t)n * sizeof(double), e->own_stream);
}

int itd_set_resident_mode(itd_engine *e, int32_t mode)
{
    if (!e || mode < ITD_RESIDENT_AUTO || mode > ITD_RESIDENT_ONLY) return ITD_ERR_INVALID_ARG;
    e->policy.set_resident_mode(mode);
    return ITD_OK;
}

int itd_get_resident_repeats(const itd_engine *e) { return e ? e->policy.resident_repeats : -1; }

int itd_set_valid_flags(itd_engine *e, int32_t *valid_dev)
{
    if (!e) return ITD_ERR_INVALID_ARG;
    e->valid_dev = valid_dev;
    return ITD_OK;
}

int itd_set_device_repair(itd_engine *e, int32_t on)
{
    if (!e) return ITD_ERR_INVALID_ARG;
    e->device_repair = on != 0;
    return ITD_OK;
}

int64_t itd_get_device_repairs(const itd_engine *e) { return e ? e->policy.device_repairs : -1; }

int itd_set_fuse_range(itd_engine *e, int32_t tiles)
{
    if (!e || (tiles != 0 && tiles != 16 && tiles != 32 && tiles != 64)) return ITD_ERR_INVALID_ARG;
    e->policy.set_fuse_range(tiles);
    return ITD_OK;
}

int itd_set_fuse_mode(itd_engine *e, int32_t mode)
{
    if (!e || mode < ITD_FUSE_AUTO || mode > ITD_FUSE_ONLY) return ITD_ERR_INVALID_ARG;
    e->policy.set_fuse_mode(mode);
    return ITD_OK;
}

int itd_set_fuse_level(itd_engine *e, int32_t first_fused_level)
{
    // (level 1's launch completes the signal's own knot count, and a level-1 list would not fit the workspace: 2 at least)
    if (!e || (first_fused_level != 0 && (first_fused_level < 2 || first_fused_level > ITD_MAX_ITERATION))) return ITD_ERR_INVALID_ARG;
    e->policy.set_fuse_level(first_fused_level);
    return ITD_OK;
}

int itd_set_fuse_min_samples(itd_engine *e, int64_t samples)
{
    if (!e || samples < 0) return ITD_ERR_INVALID_ARG;
    e->policy.set_fuse_min_samples(samples);
    return ITD_OK;
}

int itd_debug_int_ratio_check(int device, int32_t max_den, int64_t *mismatches)
{
    if (!mismatches || max_den < 1) return ITD_ERR_INVALID_ARG;
    DevGuard g(device);
    Buf<unsigned long long> d;
    unsigned long long h = 0;
    if (d.alloc(8) != hipSuccess || hipMemset(d, 0, 8) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ITD_ERR_HIP;
    k_int_ratio_check<<<1024, 256>>>(max_den, d);
    const bool ok = hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost) == hipSuccess;
    *mismatches = (int64_t)h;
    return ok ? ITD_OK : ITD_ERR_HIP;
}

int itd_debug_kf_fault(itd_engine *e, int32_t kind, int32_t level, int32_t where, int32_t slot, int32_t delta)
{
    if (!e || kind > 8 || (kind >= 0 && (level < 2 || level > ITD_MAX_ITERATION + 1 || where < 0 || slot < 0))) return ITD_ERR_INVALID_ARG;
    if ((kind == 6 || kind == 7) && slot > 4) return ITD_ERR_INVALID_ARG;
    e->fault_kind = kind < 0 ? -1 : kind;
    e->fault_level = level; e->fault_where = where; e->fault_slot = slot; e->fault_delta = delta;
    return ITD_OK;
}

int itd_debug_kf_fault_signal(itd_engine *e, int32_t signal)
{
    if (!e || signal < 0) return ITD_ERR_INVALID_ARG;
    e->fault_sig = signal;
    return ITD_OK;
}

int itd_set_fuse_cap(itd_engine *e, int32_t first_level_not_fused)
{
    if (!e || first_level_not_fused < -1 || first_level_not_fused > ITD_MAX_ITERATION + 1 || (first_level_not_fused > 0 && first_level_not_fused < 4)) return ITD_ERR_INVALID_ARG;
    e->policy.set_fuse_cap(first_level_not_fused);
    return ITD_OK;
}
int itd_get_last_fuse_cap(const itd_engine *e) { return !e ? -1 : (e->ran && e->last.kf_form ? e->last.kf_cap_form : 0); }

int itd_get_fuse_repeats(const itd_engine *e) { return e ? e->policy.fuse_repeats : -1; }
int itd_get_last_fuse_level(const itd_engine *e) { return !e ? -1 : (e->ran && e->last.kf_form ? e->last.kf_form : 0); }
int64_t itd_get_fuse_signal_repairs(const itd_engine *e) { return e ? e->policy.fuse_signal_repairs : -1; }

int itd_set_resident_window(itd_engine *e, int32_t segments)
{
    if (!e || segments < 0 || (segments > 0 && segments < 8)) return ITD_ERR_INVALID_ARG;
    e->resident_window = segments;
    return ITD_OK;
}

#if ITD_PROF
// diagnostic build only (tools/level0_prof.py): where the fused level-0 launch's wavefronts leave their phase times
extern "C" int itd_debug_prof_buffer(void *dev_buf)
{
    unsigned long long *p = static_cast<unsigned long long *>(dev_buf);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_prof_buf), &p, sizeof(p)) == hipSuccess ? ITD_OK : ITD_ERR_HIP;
}
// (tools/knots_prof.py): the knot side's workgroups' phase marks
extern "C" int itd_debug_knots_prof_buffer(void *dev_buf)
{
    unsigned long long *p = static_cast<unsigned long long *>(dev_buf);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_kc_prof), &p, sizeof(p)) == hipSuccess ? ITD_OK : ITD_ERR_HIP;
}
#endif

int itd_set_batch_streams(itd_engine *e, int32_t streams)
{
    if (!e || streams < 1 || streams > 4) return ITD_ERR_INVALID_ARG;
    e->batch_streams = streams;
    return ITD_OK;
}

int itd_set_batch_chunk(itd_engine *e, int32_t signals_per_chunk)
{
    if (!e || signals_per_chunk < 0) return ITD_ERR_INVALID_ARG;
    e->chunk = signals_per_chunk;
    return ITD_OK;
}

}  // extern "C"

namespace {
// The body of the six host entries.  host: the caller's rows as a Rows (its pointer a host address): float32 rows and selections come
// without baselines, kept or returned; all of a selection's slots are copied back, those of rotations the decomposition did not reach
// with unspecified content
template <typename Tin>
int decompose_host(itd_engine *e, const Tin *x_host, int64_t n, int32_t M, Rows host, double *bases_host,
                   int32_t *n_rows, int32_t *n_baselines, int32_t *stop_reason, int64_t *knot_counts)
{
    if (!e || !x_host || !host.p) return ITD_ERR_INVALID_ARG;
    if (n < 3 || n > e->max_n || M < 0 || M > ITD_MAX_ITERATION) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    int rc = grow(e, e->d_io_x, (size_t)n * sizeof(Tin));
    if (rc) return rc;
    rc = grow(e, e->d_io_rows, (size_t)host.stride(M, n) * host.esz());
    if (rc) return rc;
    const bool dev_bases = !host.f32 && !host.sel && (bases_host || e->host_keep_bases);
    e->kept_nb = -1;
    if (dev_bases) {
        rc = grow(e, e->d_io_bases, (size_t)host.stride(M, n) * sizeof(double));
        if (rc) return rc;
    }
    hipStream_t st = e->own_stream;
    HIP_TRY(e, hipMemcpyAsync(e->d_io_x, x_host, (size_t)n * sizeof(Tin), hipMemcpyHostToDevice, st));
    Rows rows = host;
    rows.p = e->d_io_rows.get();
    rc = enqueue_any<Tin>(e, (const Tin *)e->d_io_x, n, 1, n, M, rows, dev_bases ? e->d_io_bases : nullptr, st);
    if (rc) return rc;
    int32_t nr = 0, nb = 0, why = 0, nanlv = -1;
    int64_t kc[ITD_MAX_ROWS + 1];
    rc = itd_get_summary(e, &nr, &nb, &why, kc, &nanlv);
    if (rc) return rc;
    rc = copy_to_host(e, host.p, e->d_io_rows, (size_t)(host.sel ? host.count(M) : nr) * n * host.esz(), st);
    if (rc) return rc;
    if (bases_host) {
        rc = copy_to_host(e, bases_host, e->d_io_bases, (size_t)nb * n * sizeof(double), st);
        if (rc) return rc;
    }
    if (n_rows) *n_rows = nr;
    if (n_baselines) *n_baselines = nb;
    if (stop_reason) *stop_reason = why;
    if (knot_counts) memcpy(knot_counts, kc, sizeof(kc));
    if (dev_bases && nanlv == -1) { e->kept_n = n; e->kept_nb = nb; }
    return nanlv != -1 ? ITD_ERR_NONFINITE : ITD_OK;
}

// ---------------------------------------------------------------------------------------------
// The knot scan every single-level operator starts with: what it works on (KnotWs: carved from one of the engine's arenas, or
// the fixed one-signal buffers seen as one), its launches (knot_scan), the record-driven level-0 extraction behind it
// (extract_level0) and its totals on the host (fetch_totals).
// ---------------------------------------------------------------------------------------------
struct KnotWs {
    int32_t *lists, *counts, *gsum, *kidx, *totals, *tbase;   // a part that was not asked for is NULL
    TileRec *recs;
    SigState *state;
    int64_t kidx_stride;      // kidx[b] = [lead slot, knots, tail]; totals[b] = {knot count, the signal holds a NaN}
    int64_t half, third;      // elements between the two count / record buffers, between the three group-sum buffers
    int64_t gsum_zero;        // group-sum elements a scan zeroes first: one buffer, or all three (a k_extract behind the scan)
    int n_tiles, n_groups;
    int init_pad;             // blocks the initialising launch has beyond what it needs (the fixed buffers' launch always had one)
};
// the optional parts: per-tile lists (the fast pair keeps its flag words there), ordered lists and totals, the knots in front of
// every tile (k_compact), and the second count / record buffer with group-sum buffers two and three
enum : int { kWsLists = 1, kWsOrdered = 2, kWsTbase = 4, kWsExtract = 8, kWsDetect = kWsLists | kWsOrdered | kWsTbase };

// a KnotWs for `batch` signals of n samples from a grow-only arena, `tail` bytes for the caller behind it (*tail_out)
int knot_workspace(itd_engine *e, Buf<void> &arena, int64_t n, int batch, int parts, KnotWs &w, size_t tail = 0,
                   char **tail_out = nullptr)
{
    w.n_tiles = (int)tiles_of(n);
    w.n_groups = groups_of(w.n_tiles);
    w.kidx_stride = n + 2;
    w.half = (int64_t)batch * w.n_tiles;
    w.third = (int64_t)batch * w.n_groups * kGsumPitch;
    const size_t bufs = parts & kWsExtract ? 2 : 1, gbufs = parts & kWsExtract ? 3 : 1, B = (size_t)batch, tiles = (size_t)w.half;
    w.gsum_zero = (int64_t)gbufs * w.third;
    w.init_pad = 0;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_lists = parts & kWsLists ? al(tiles * T * sizeof(int32_t)) : 0, b_tbase = parts & kWsTbase ? al(tiles * sizeof(int32_t)) : 0;
    const size_t b_counts = al(bufs * tiles * sizeof(int32_t)), b_recs = al(bufs * tiles * sizeof(TileRec));
    const size_t b_gsum = al(gbufs * (size_t)w.third * sizeof(int32_t)), b_state = al(B * sizeof(SigState));
    const size_t b_kidx = parts & kWsOrdered ? al(B * (size_t)w.kidx_stride * sizeof(int32_t)) : 0, b_tot = parts & kWsOrdered ? al(B * 2 * sizeof(int32_t)) : 0;
    const int rc = grow(e, arena, b_lists + b_counts + b_recs + b_gsum + b_state + b_kidx + b_tot + b_tbase + tail);
    if (rc) return rc;
    char *p = (char *)arena;
    auto take = [&p](size_t b) { char *q = b ? p : nullptr; p += b; return q; };
    w.lists = (int32_t *)take(b_lists);
    w.counts = (int32_t *)take(b_counts);
    w.recs = (TileRec *)take(b_recs);
    w.gsum = (int32_t *)take(b_gsum);
    w.state = (SigState *)take(b_state);
    w.kidx = (int32_t *)take(b_kidx);
    w.totals = (int32_t *)take(b_tot);
    w.tbase = (int32_t *)take(b_tbase);
    if (tail_out) *tail_out = p;
    return ITD_OK;
}

// the engine's fixed one-signal buffers as a KnotWs: the helpers' own state, counts, records and group sums (a decomposition's
// workspace is never touched), nothing to allocate.  The second half of the count buffer receives every tile's knot base.
KnotWs helper_ws(const itd_engine *e, int64_t n)
{
    KnotWs w;
    w.n_tiles = (int)tiles_of(n);
    w.n_groups = groups_of(w.n_tiles);
    w.lists = e->d_lists; w.counts = e->d_hcounts; w.recs = e->d_hrecs; w.gsum = e->d_hgsum; w.state = e->d_hstate;
    w.kidx = e->d_kidx; w.kidx_stride = e->max_n + 2; w.totals = e->d_total;
    w.half = e->max_tiles; w.third = e->hgsum_third;
    w.tbase = w.counts + w.half;
    w.gsum_zero = 3 * e->hgsum_third;
    w.init_pad = 1;
    return w;
}

// the scan's first launch: states and group sums (keep_in_nan: the NaN-input repeat needs to know which signals hold one)
void scan_init(const KnotWs &w, int batch, bool keep_in_nan, hipStream_t st)
{
    const int64_t blocks = std::max<int64_t>((w.gsum_zero + 255) / 256 + w.init_pad, (batch + 255) / 256);
    k_init_state<<<(unsigned)std::min<int64_t>(blocks, 2048), 256, 0, st>>>(w.state, batch, w.gsum, w.gsum_zero, keep_in_nan ? 1 : 0);
}

// the scan's last launch when ordered lists are wanted.  kidx_out = NULL: into the workspace's lists with a leading slot (what the
// cubic kernels and the stream's selection read); else the caller's [batch][kidx_out_stride] array without one (itd_detect_batch_*).
// fast: from the flag words of the short pair (itd_detect_fast.hpp)
void scan_compact(const KnotWs &w, int64_t n, int batch, bool fast, int64_t tail_value, int32_t *kidx_out, int64_t kidx_out_stride,
                  hipStream_t st)
{
    const dim3 grid_t(w.n_tiles, batch), blk(kWave);
    int32_t *kidx = kidx_out ? kidx_out : w.kidx;
    const int64_t stride = kidx_out ? kidx_out_stride : w.kidx_stride;
    const int lead = kidx_out ? 0 : 1;
    if (fast)
        k_compact_fast<<<grid_t, blk, 0, st>>>(reinterpret_cast<const unsigned long long *>(w.lists), w.counts, w.gsum, w.n_tiles, n, kidx,
                                               stride, w.totals, w.state, tail_value, w.tbase, lead);
    else
        k_compact<T><<<grid_t, blk, 0, st>>>(w.lists, w.counts, w.gsum, w.n_tiles, n, kidx, stride, w.totals, w.state, tail_value, w.tbase, lead);
}

// Level-0 knots of `batch` signals (batch <= 65535: grid.y) by predicate `mode`, no host synchronisation.  after: what is wanted
// behind the detection — nothing (counts, records and group sums for a k_extract), totals[b] only, or the ordered lists too.
// nan_follow: the scanned signals hold a NaN (found by a first scan, SigState::in_nan kept): the knot set the reference's NaN
// branch gives (k_nan_level0), and — if nan_xm is non-null — the mutated float64 copy of the signal
enum KnotAfter { kScanOnly, kScanTotals, kScanOrdered };
template <typename Tin>
int knot_scan(itd_engine *e, const KnotWs &w, const Tin *x, int64_t x_stride, int64_t n, int batch, int mode, KnotAfter after, hipStream_t st,
              int64_t tail_value = -1, bool nan_follow = false, double *nan_xm = nullptr, int32_t *kidx_out = nullptr, int64_t kidx_out_stride = 0)
{
    const dim3 grid_t(w.n_tiles, batch), blk(kWave);
    int32_t *lists = after == kScanOrdered ? w.lists : nullptr;
    scan_init(w, batch, nan_follow, st);
    bool fast = false;
    if constexpr (std::is_same<Tin, double>::value) {
        // the two predicates without NaN rules and without an extraction behind them: the short pair (itd_detect_fast.hpp); the
        // tiles' flag words live where the general pair keeps its per-tile position lists
        fast = !nan_follow && after == kScanOrdered && (mode == (int)kCpp || mode == (int)kZeroCross);
        unsigned long long *fw = reinterpret_cast<unsigned long long *>(w.lists);
        if (fast && mode == (int)kCpp) k_detect_fast<(int)kCpp><<<grid_t, blk, 0, st>>>(x, x_stride, n, w.n_tiles, w.counts, fw, w.gsum, w.state);
        else if (fast) k_detect_fast<(int)kZeroCross><<<grid_t, blk, 0, st>>>(x, x_stride, n, w.n_tiles, w.counts, fw, w.gsum, w.state);
    }
    if (!fast && nan_follow)
        k_nan_level0<Tin, T><<<grid_t, blk, 0, st>>>(x, x_stride, n, w.n_tiles, nan_xm, n, w.counts, w.recs, w.gsum, w.state, mode, lists);
    else if (!fast)
        k_detect<Tin, T><<<grid_t, blk, 0, st>>>(x, x_stride, n, w.n_tiles, mode, lists, w.counts, w.recs, w.gsum, w.state);
    if (after == kScanOrdered) scan_compact(w, n, batch, fast, tail_value, kidx_out, kidx_out_stride, st);
    else if (after == kScanTotals) k_batch_totals<<<(batch + 3) / 4, 256, 0, st>>>(w.gsum, w.n_groups, batch, w.state, w.totals);
    HIP_TRY(e, hipGetLastError());
    return ITD_OK;
}

// the record-driven level-0 extraction behind a scan (ITD.py:79-121; keep_nan: the baseline as computed): rewrites the per-tile
// lists' counts and records into the workspace's second buffers
template <typename Tin>
void extract_level0(const KnotWs &w, const Tin *x, int64_t x_stride, int64_t n, int batch, double *rot, int64_t rot_stride, double *base,
                    int64_t base_stride, hipStream_t st)
{
    k_extract<Tin, T, false, kRankCap0, kTilesPerWave><<<dim3((w.n_tiles + kTilesPerWave - 1) / kTilesPerWave, batch), kWave, 0, st>>>(
        x, x_stride, n, w.n_tiles, batch, w.counts, w.counts + w.half, w.recs, w.recs + w.half, w.gsum, w.gsum + w.third, w.gsum + 2 * w.third,
        rot, rot_stride, base, base_stride, w.state, 0, 1);
}

// totals[b] = {knot count, the signal held a NaN} of `batch` signals: synchronises, fills counts_out (optional).  A NaN: the
// reference's detect_peaks would take its NaN branch and write +inf into the caller's array — rejected, like NaN input of a
// decomposition, unless the caller follows that branch itself (nan_is_error = false).  read_totals: the same from totals that are on
// the host already (a copy taken earlier on the stream, the mapped reply's words)
int read_totals(const int32_t *tot, int batch, int32_t *counts_out, bool nan_is_error = true)
{
    bool nan_in = false;
    for (int b = 0; b < batch; ++b) {
        if (counts_out) counts_out[b] = tot[2 * (size_t)b];
        nan_in = nan_in || tot[2 * (size_t)b + 1] != 0;
    }
    return nan_in && nan_is_error ? ITD_ERR_NONFINITE : ITD_OK;
}
int copy_totals(itd_engine *e, const int32_t *totals, int batch, int32_t *tot_host, hipStream_t st)
{
    HIP_TRY(e, hipMemcpyAsync(tot_host, totals, (size_t)batch * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    return ITD_OK;
}
int fetch_totals(itd_engine *e, const int32_t *totals, int batch, int32_t *counts_out, hipStream_t st, bool nan_is_error = true)
{
    std::vector<int32_t> tot((size_t)batch * 2);
    const int rc = copy_totals(e, totals, batch, tot.data(), st);
    return rc ? rc : read_totals(tot.data(), batch, counts_out, nan_is_error);
}
// the knot total of the last one-signal scan and whether the signal holds a NaN, both from one copy (nothing is written where the
// copy fails)
int fetch_total(itd_engine *e, const KnotWs &w, hipStream_t st, int64_t *m_host, bool nan_is_error = true, bool *has_nan = nullptr)
{
    int32_t tot[2] = {0, 0};
    const int rc = copy_totals(e, w.totals, 1, tot, st);
    if (rc) return rc;
    *m_host = tot[0];
    if (has_nan) *has_nan = tot[1] != 0;
    return read_totals(tot, 1, nullptr, nan_is_error);
}

// the three knot sets of the reference's own detect functions follow its NaN branch when the signal holds a NaN
inline bool nan_follows(const itd_engine *e, int mode)
{
    return e->nan_input_mode == ITD_NAN_INPUT_FOLLOW && (mode == (int)kKnots || mode == (int)kValleys || mode == (int)kPeaks);
}

// One signal's knots by predicate `mode` in the engine's fixed buffers, with the level-0 extraction behind the scan if rot / base
// are given.  m = NULL: nothing is read back: one pass under the plain rules, asynchronous.  Else the total is read (*m, written
// like fetch_total's), and a signal that holds a NaN is refused (ITD_ERR_NONFINITE) unless the mode follows the reference's NaN
// branch: then it is scanned again the way the reference runs it (ITD.py:46-51, 64-68; numba_accelerated_itd.py:28-49) and the
// total read again.  An extraction's second pass reads the mutated float64 copy that branch leaves behind (ITD.py:87-88), staged
// in d_cub: *mutated = that copy, or NULL where the signal's own values are its knot values.  knots_out (device, optional): the
// ordered list, synchronised
template <typename Tin>
int scan_one(itd_engine *e, const Tin *x, int64_t n, int mode, double *rot, double *base, int64_t *m, int32_t *knots_out,
             hipStream_t st, const double **mutated = nullptr)
{
    const KnotWs w = helper_ws(e, n);
    double *xm = nullptr;
    bool has_nan = false;
    auto pass = [&](bool follow) -> int {
        const int rc = knot_scan<Tin>(e, w, x, n, n, 1, mode, m ? kScanOrdered : kScanOnly, st, -1, follow, xm);
        if (rc) return rc;
        if (rot) {   // (the scan has taken the ordered list: k_extract rewrites the per-tile lists)
            if (xm) extract_level0<double>(w, xm, n, n, 1, rot, n, base, n, st);
            else extract_level0<Tin>(w, x, n, n, 1, rot, n, base, n, st);
            HIP_TRY(e, hipGetLastError());
        }
        return m ? fetch_total(e, w, st, m, !follow && !nan_follows(e, mode), &has_nan) : (int)ITD_OK;
    };
    int rc = pass(false);
    if (rc || !m) return rc;
    if (has_nan) {
        if (rot) {
            rc = grow(e, e->d_cub, (size_t)n * sizeof(double));
            if (rc) return rc;
            xm = (double *)e->d_cub;
        }
        rc = pass(true);
        if (rc) return rc;
    }
    if (mutated) *mutated = xm;
    if (knots_out && *m > 0) {
        HIP_TRY(e, hipMemcpyAsync(knots_out, w.kidx + 1, sizeof(int32_t) * (size_t)*m, hipMemcpyDeviceToDevice, st));
        HIP_TRY(e, hipStreamSynchronize(st));
    }
    return ITD_OK;
}

template <typename Tin>
int extract_dev(itd_engine *e, const Tin *x, int64_t n, double *rot, double *base, int32_t *knots, int64_t *m_host,
                hipStream_t st, bool want_sync, const double **mutated = nullptr)
{
    if (!e || !x || !rot || !base) return ITD_ERR_INVALID_ARG;
    if (n < 3 || n > e->max_n) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    int64_t m = 0;
    const int rc = scan_one<Tin>(e, x, n, (int)kKnots, rot, base, m_host || knots || want_sync ? &m : nullptr, knots, st, mutated);
    if (rc) return rc;
    if (m_host) *m_host = m;
    return ITD_OK;
}

template <typename Tin>
int detect_dev(itd_engine *e, const Tin *x, int64_t n, int32_t mode, int32_t *idx, int64_t *count, hipStream_t st)
{
    if (!e || !x || !count) return ITD_ERR_INVALID_ARG;
    if (n < 3 || n > e->max_n || mode < 0 || mode > 4) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    return scan_one<Tin>(e, x, n, mode, nullptr, nullptr, count, idx, st);
}

// What a host form of the single-level helpers stages through, on the engine's own stream: the caller's signal in d_io_x, its results
// in regions of d_io_rows handed out in the order they are asked for (every element 8 bytes wide).  Once a copy from or into the
// caller's memory has been enqueued, no return hands that memory back before the stream has drained: the destructor sees to it on
// every path that has not said so itself (sync(); settled() behind a device form that has synchronised)
struct HostStage {
    itd_engine *e;
    hipStream_t st;
    DevGuard g;
    int rc = ITD_OK;          // the first thing that went wrong while staging: no copy is enqueued behind it
    double *x = nullptr;      // d_io_x
    char *next = nullptr;     // d_io_rows: what has not been handed out ...
    size_t left = 0;          // ... of so many elements
    bool pending = false;     // a copy from or into the caller's memory may be in flight

    explicit HostStage(itd_engine *e_) : e(e_), st(e_->own_stream), g(e_->device) {}
    HostStage(const HostStage &) = delete;
    ~HostStage() { if (pending) (void)hipStreamSynchronize(st); }

    // the length of a signal that goes through the engine's fixed one-signal buffers
    int check_n(int64_t n) { return rc = n < 3 || n > e->max_n ? (int)ITD_ERR_INVALID_ARG : rc; }
    int reserve(size_t in_elems, size_t out_elems)
    {
        if (!rc) rc = grow(e, e->d_io_x, in_elems * sizeof(double));
        if (!rc) rc = grow(e, e->d_io_rows, out_elems * sizeof(double));
        if (!rc) { x = (double *)e->d_io_x; next = (char *)e->d_io_rows.get(); left = out_elems; }
        return rc;
    }
    template <typename U> U *take(int64_t count)
    {
        static_assert(sizeof(U) == sizeof(double), "d_io_rows is carved in 8-byte elements");
        if (count < 0 || (size_t)count > left) { rc = ITD_ERR_INVALID_ARG; return nullptr; }   // more than the entry reserved
        U *p = (U *)next;
        next += (size_t)count * sizeof(U); left -= (size_t)count;
        return p;
    }
    template <typename U> int copy(U *dst, const U *src, int64_t count, hipMemcpyKind kind)
    {
        if (rc) return rc;
        pending = true;
        HIP_TRY(e, hipMemcpyAsync(dst, src, (size_t)count * sizeof(U), kind, st));
        return ITD_OK;
    }
    template <typename U> int upload(U *dst_dev, const U *src_host, int64_t count) { return copy(dst_dev, src_host, count, hipMemcpyHostToDevice); }
    template <typename U> int download(U *dst_host, const U *src_dev, int64_t count) { return copy(dst_host, src_dev, count, hipMemcpyDeviceToHost); }
    // a device knot list (int32) widened into `region` and brought home as the int64 the host forms deliver
    int knots_home(int64_t *dst_host, const int32_t *kidx, int64_t count, int64_t *region)
    {
        k_widen_idx<<<(unsigned)((count + 255) / 256), 256, 0, st>>>(kidx, region, count);
        return download(dst_host, region, count);
    }
    int sync()
    {
        HIP_TRY(e, hipStreamSynchronize(st));
        pending = false;
        return ITD_OK;
    }
    void settled() { pending = false; }
};
}  // namespace

extern "C" {

int itd_decompose_host_f64(itd_engine *e, const double *x_host, int64_t n, int32_t max_iteration, double *rows_host,
                           double *baselines_host, int32_t *n_rows, int32_t *n_baselines, int32_t *stop_reason,
                           int64_t *knot_counts)
{
    return decompose_host(e, x_host, n, max_iteration, Rows(rows_host), baselines_host, n_rows, n_baselines, stop_reason, knot_counts);
}

int itd_decompose_host_f32(itd_engine *e, const float *x_host, int64_t n, int32_t max_iteration, double *rows_host,
                           double *baselines_host, int32_t *n_rows, int32_t *n_baselines, int32_t *stop_reason,
                           int64_t *knot_counts)
{
    return decompose_host(e, x_host, n, max_iteration, Rows(rows_host), baselines_host, n_rows, n_baselines, stop_reason, knot_counts);
}

int itd_decompose_rows32_host_f32(itd_engine *e, const float *x_host, int64_t n, int32_t max_iteration, float *rows_host,
                                  int32_t *n_rows, int32_t *stop_reason, int64_t *knot_counts)
{
    return decompose_host(e, x_host, n, max_iteration, Rows(rows_host), nullptr, n_rows, nullptr, stop_reason, knot_counts);
}

int itd_decompose_rows32_host_f64(itd_engine *e, const double *x_host, int64_t n, int32_t max_iteration, float *rows_host,
                                  int32_t *n_rows, int32_t *stop_reason, int64_t *knot_counts)
{
    return decompose_host(e, x_host, n, max_iteration, Rows(rows_host), nullptr, n_rows, nullptr, stop_reason, knot_counts);
}

int itd_decompose_select_host_f32(itd_engine *e, const float *x_host, int64_t n, int32_t max_iteration, uint32_t rotation_mask,
                                  int32_t want_residual, void *rows_host, int32_t rows_f32, int32_t *n_rows, int32_t *stop_reason,
                                  int64_t *knot_counts)
{
    if (!selection_ok(max_iteration, rotation_mask, want_residual, rows_f32)) return ITD_ERR_INVALID_ARG;
    return decompose_host(e, x_host, n, max_iteration, Rows(rows_host, rows_f32 != 0, rotation_mask, want_residual != 0), nullptr, n_rows, nullptr,
                          stop_reason, knot_counts);
}

int itd_decompose_select_host_f64(itd_engine *e, const double *x_host, int64_t n, int32_t max_iteration, uint32_t rotation_mask,
                                  int32_t want_residual, void *rows_host, int32_t rows_f32, int32_t *n_rows, int32_t *stop_reason,
                                  int64_t *knot_counts)
{
    if (!selection_ok(max_iteration, rotation_mask, want_residual, rows_f32)) return ITD_ERR_INVALID_ARG;
    return decompose_host(e, x_host, n, max_iteration, Rows(rows_host, rows_f32 != 0, rotation_mask, want_residual != 0), nullptr, n_rows, nullptr,
                          stop_reason, knot_counts);
}

int itd_baseline_extract_f64(itd_engine *e, const double *x_dev, int64_t n, double *rot_dev, double *base_dev,
                             int32_t *knots_dev, int64_t *m_host, void *stream)
{
    if (!e) return ITD_ERR_INVALID_ARG;
    return extract_dev<double>(e, x_dev, n, rot_dev, base_dev, knots_dev, m_host, stream_of(e, stream), false);
}

int itd_baseline_extract_f32(itd_engine *e, const float *x_dev, int64_t n, double *rot_dev, double *base_dev,
                             int32_t *knots_dev, int64_t *m_host, void *stream)
{
    if (!e) return ITD_ERR_INVALID_ARG;
    return extract_dev<float>(e, x_dev, n, rot_dev, base_dev, knots_dev, m_host, stream_of(e, stream), false);
}

int itd_baseline_extract_host_f64(itd_engine *e, const double *x_host, int64_t n, double *rot_host, double *base_host,
                                  int64_t *knots_host, int64_t *m_host, double *bk_host)
{
    if (!e || !x_host || !rot_host || !base_host) return ITD_ERR_INVALID_ARG;
    HostStage S(e);
    if (S.check_n(n) || S.reserve(n, 4 * n + 2)) return S.rc;
    double *d_rot = S.take<double>(n), *d_base = S.take<double>(n), *d_bk = S.take<double>(n + 2);
    int64_t *d_k64 = S.take<int64_t>(n);
    int rc = S.upload(S.x, x_host, n);
    if (rc) return rc;
    int64_t m = 0;
    const double *mutated = nullptr;
    rc = extract_dev<double>(e, S.x, n, d_rot, d_base, nullptr, &m, S.st, true, &mutated);
    if (!rc) rc = S.download(rot_host, d_rot, n);
    if (!rc) rc = S.download(base_host, d_base, n);
    if (!rc && knots_host && m > 0) rc = S.knots_home(knots_host, helper_ws(e, n).kidx + 1, m, d_k64);
    if (!rc && bk_host) {
        // (a signal that holds NaNs: the knot values of the mutated copy, as the reference computes them after detect_peaks' write)
        k_knot_values<double><<<(unsigned)((m + 2 + 255) / 256), 256, 0, S.st>>>(mutated ? mutated : S.x, n, helper_ws(e, n).kidx, (int)m, d_bk);
        rc = S.download(bk_host, d_bk, m + 2);
    }
    if (!rc) rc = S.sync();
    if (rc) return rc;
    if (m_host) *m_host = m;
    return ITD_OK;
}

int itd_detect_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t mode, int32_t *idx_dev, int64_t *count_host,
                   void *stream)
{
    if (!e) return ITD_ERR_INVALID_ARG;
    return detect_dev<double>(e, x_dev, n, mode, idx_dev, count_host, stream_of(e, stream));
}

int itd_detect_f32(itd_engine *e, const float *x_dev, int64_t n, int32_t mode, int32_t *idx_dev, int64_t *count_host,
                   void *stream)
{
    if (!e) return ITD_ERR_INVALID_ARG;
    return detect_dev<float>(e, x_dev, n, mode, idx_dev, count_host, stream_of(e, stream));
}

int itd_detect_host_f64(itd_engine *e, const double *x_host, int64_t n, int32_t mode, int64_t *idx_host,
                        int64_t *count_host)
{
    if (!e || !x_host || !count_host || mode < 0 || mode > 4) return ITD_ERR_INVALID_ARG;
    HostStage S(e);
    if (S.check_n(n) || S.reserve(n, n)) return S.rc;
    int64_t *d_k64 = S.take<int64_t>(n);
    int rc = S.upload(S.x, x_host, n);
    if (rc) return rc;
    int64_t m = 0;
    rc = detect_dev<double>(e, S.x, n, mode, nullptr, &m, S.st);
    if (rc) return rc;
    S.settled();      // (detect_dev has read its total)
    if (idx_host && m > 0) {
        rc = S.knots_home(idx_host, helper_ws(e, n).kidx + 1, m, d_k64);
        if (!rc) rc = S.sync();
        if (rc) return rc;
    }
    *count_host = m;
    return ITD_OK;
}

int itd_knot_values_host_f64(itd_engine *e, const double *x_host, int64_t n, const int64_t *extrema_host, int64_t m,
                             double *bk_host)
{
    if (!e || !x_host || !extrema_host || !bk_host) return ITD_ERR_INVALID_ARG;
    if (n < 2 || n > e->max_n || m < 0 || m + 2 > e->max_n + 2) return ITD_ERR_INVALID_ARG;
    for (int64_t k = 0; k < m + 2; ++k)
        if (extrema_host[k] < 0 || extrema_host[k] >= n) return ITD_ERR_INVALID_ARG;
    if (m == 0) return ITD_OK;
    std::vector<int32_t> e32((size_t)m + 2);      // (ahead of the stage: it is uploaded from)
    for (int64_t k = 0; k < m + 2; ++k) e32[(size_t)k] = (int32_t)extrema_host[k];
    HostStage S(e);
    if (S.reserve(n, m + 2)) return S.rc;
    double *d_bk = S.take<double>(m + 2);
    int rc = S.upload(S.x, x_host, n);
    if (!rc) rc = S.upload(e->d_kidx.get(), (const int32_t *)e32.data(), m + 2);
    if (rc) return rc;
    k_knot_values<double><<<(unsigned)((m + 2 + 255) / 256), 256, 0, S.st>>>(S.x, n, e->d_kidx, (int)m, d_bk);
    // interior values only: bk[0] and bk[m+1] are the caller's (numba_accelerated_itd.py:171)
    rc = S.download(bk_host + 1, d_bk + 1, m);
    return rc ? rc : S.sync();
}

int itd_knot_values_f64(itd_engine *e, const double *x_dev, int64_t n, const int32_t *extrema_dev, int64_t m, double *bk_dev,
                        void *stream)
{
    if (!e || !x_dev || !extrema_dev || !bk_dev) return ITD_ERR_INVALID_ARG;
    if (n < 2 || n >= (int64_t)INT32_MAX || m < 0 || m > n) return ITD_ERR_INVALID_ARG;
    if (m == 0) return ITD_OK;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    k_knot_values<double><<<(unsigned)((m + 2 + 255) / 256), 256, 0, st>>>(x_dev, n, extrema_dev, (int)m, bk_dev, 1);
    HIP_TRY(e, hipGetLastError());
    return ITD_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// The cubic-spline baseline variant (itd_cubic.hpp): itd_baseline_extract_fast(I, extrema_input, idx),
// itd_fourier_decomposition.py:49-122 = itd.cpp:156-239.  Single-level operator; synchronous like the other helpers.
// ---------------------------------------------------------------------------------------------
namespace {
// What the cubic kernels work on, carved from d_cub for `batch` signals with knot arrays of L entries: the jobs in front, then K, bf
// and b, then `extra` more arrays of [batch][L] doubles for the caller, from A.b + batch * L on.  The knot lists (A.e, A.e_stride,
// A.job_stride) are the caller's to fill in.
int cubic_args(itd_engine *e, const double *x, int64_t x_stride, int64_t n, int batch, int64_t L, int extra, CubicArgs &A)
{
    const size_t jobs_b = (((size_t)batch * sizeof(CubicJob)) + 255) & ~(size_t)255, arr_n = (size_t)batch * (size_t)L;
    const int rc = grow(e, e->d_cub, jobs_b + (3 + (size_t)extra) * arr_n * sizeof(double));
    if (rc) return rc;
    double *arr = (double *)((char *)e->d_cub + jobs_b);
    A.x = x; A.x_stride = x_stride; A.n = n;
    A.jobs = (const CubicJob *)e->d_cub;
    A.K = arr; A.bf = arr + arr_n; A.b = arr + 2 * arr_n; A.a_stride = L;
    return ITD_OK;
}

// The cubic operator over `batch` signals, asynchronous on st.  extrema = NULL: every signal's own knots (itd.cpp:159-169);
// else the caller's list(s) of idx + 1 entries (e_stride = 0: one list for every signal, itd.cpp:40-44).  *jobs_out: the
// per-signal jobs on the device (idx used, valid, status) for callers that synchronise afterwards; *knots_out: the detected
// knots' ordered lists (lead slot in front).
int cubic_batch(itd_engine *e, const double *x, int64_t n, int batch, int64_t x_stride, const int32_t *extrema, int64_t e_stride,
                int64_t idx, double *baseline, int64_t b_stride, hipStream_t st, const CubicJob **jobs_out, int *n_jobs_out,
                const int32_t **knots_out = nullptr)
{
    CubicArgs A;
    int rc = cubic_args(e, x, x_stride, n, batch, (extrema ? idx : n) + 2, 0, A);
    if (rc) return rc;
    CubicJob *jobs = (CubicJob *)e->d_cub;
    int n_jobs;
    int64_t max_count;
    if (!extrema) {
        KnotWs w;
        rc = knot_workspace(e, e->d_dw, n, batch, kWsDetect, w);
        // (tail 0: e[idx] = 0, the file's static array at first call)
        if (!rc) rc = knot_scan<double>(e, w, x, x_stride, n, batch, (int)kCpp, kScanOrdered, st, 0);
        if (rc) return rc;
        if (knots_out) *knots_out = w.kidx;
        n_jobs = batch;
        k_cubic_jobs<<<(batch + 255) / 256, 256, 0, st>>>(jobs, batch, 1, 0, w.totals);
        A.e = w.kidx; A.e_stride = w.kidx_stride; A.job_stride = 1;
        A.tbase = w.tbase; A.tb_stride = w.n_tiles;
        max_count = n;
    } else {
        n_jobs = e_stride ? batch : 1;
        k_cubic_jobs<<<(n_jobs + 255) / 256, 256, 0, st>>>(jobs, n_jobs, 0, idx, nullptr);
        k_cubic_validate<<<dim3((unsigned)((idx + 1 + 255) / 256), n_jobs), 256, 0, st>>>(extrema, e_stride, idx, n, jobs);
        A.e = extrema; A.e_stride = e_stride; A.job_stride = e_stride ? 1 : 0;
        max_count = idx - 1;
    }
    const unsigned nblk = (unsigned)std::max<int64_t>(1, (max_count + kScanBlockElems - 1) / kScanBlockElems);
    k_cubic_sweep<true><<<dim3(nblk, batch), kScanThreads, 0, st>>>(A);
    k_cubic_sweep<false><<<dim3(nblk, batch), kScanThreads, 0, st>>>(A);
    k_cubic_eval<T><<<dim3((unsigned)tiles_of(n), batch), kWave, 0, st>>>(A, 0, n, baseline, b_stride, 0);
    HIP_TRY(e, hipGetLastError());
    if (jobs_out) *jobs_out = jobs;
    if (n_jobs_out) *n_jobs_out = n_jobs;
    return ITD_OK;
}

// knots of x by one of the cubic variant's predicates into d_kidx+1 (d_kidx[0] = 0 in front of them), *idx_out = their
// count (find_extrema: including the leading 0 and the extrapolated tail, like the reference's return value)
int cubic_detect(itd_engine *e, const double *x, int64_t n, int mode, int64_t *count, hipStream_t st)
{
    const KnotWs w = helper_ws(e, n);
    int rc = knot_scan<double>(e, w, x, n, n, 1, mode, kScanOrdered, st, mode == (int)kCpp ? 0 : -1);
    if (rc) return rc;
    if (mode == (int)kZeroCross) k_zero_cross_tail<<<1, 1, 0, st>>>(w.kidx, w.totals);
    return fetch_total(e, w, st, count);
}

// one signal, synchronous: ONE host synchronisation, at the end (the job: knot count, validity)
int cubic_dev(itd_engine *e, const double *x, int64_t n, const int32_t *extrema, int64_t idx, double *baseline,
              int64_t *idx_out, hipStream_t st, const int32_t **knots_dev_out = nullptr)
{
    if (!e || !x || !baseline) return ITD_ERR_INVALID_ARG;
    if (n < 3 || n > e->max_n) return ITD_ERR_INVALID_ARG;
    if (extrema && (idx < 2 || idx > n - 1)) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    const CubicJob *jobs = nullptr;
    const int32_t *kidx = nullptr;
    int rc = cubic_batch(e, x, n, 1, n, extrema, 0, idx, baseline, n, st, &jobs, nullptr, &kidx);
    if (rc) return rc;
    CubicJob job;
    HIP_TRY(e, hipMemcpyAsync(&job, jobs, sizeof(job), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    if (job.status == 1) return ITD_ERR_INVALID_ARG;
    if (job.status == 2) return ITD_ERR_NONFINITE;
    if (idx_out) *idx_out = job.idx;
    if (knots_dev_out) *knots_dev_out = kidx + 1;    // the detected knots (behind the workspace list's leading slot)
    return ITD_OK;
}

// the caller's knot list (host, int64, `count` entries) for the kernels: range-checked on the host copy first (narrowing to int32
// must not wrap; nothing has been enqueued where that fails), uploaded into `scratch`, narrowed into d_cub_e
int stage_extrema(HostStage &S, const int64_t *extrema_host, int64_t count, int64_t n, int64_t *scratch, const int32_t **dev_out)
{
    for (int64_t k = 0; k < count; ++k)
        if (extrema_host[k] < 0 || extrema_host[k] >= n) return ITD_ERR_INVALID_ARG;
    int rc = grow(S.e, S.e->d_cub_e, (size_t)count * sizeof(int32_t));
    if (!rc) rc = S.upload(scratch, extrema_host, count);
    if (rc) return rc;
    k_narrow_idx<<<(unsigned)((count + 255) / 256), 256, 0, S.st>>>(scratch, S.e->d_cub_e, count);
    *dev_out = S.e->d_cub_e;
    return ITD_OK;
}

// The host form of the natural-cubic operator and of its I/Q form: `comps` values per sample, body(x, list, baseline, &idx, st,
// &knots) the device form (knots: where it leaves the knots it detected, asked for when the caller hands in no list)
template <typename Body>
int cubic_host(itd_engine *e, const double *x_host, int comps, int64_t n, const int64_t *extrema_host, int64_t idx,
               double *baseline_host, int64_t *idx_out, int64_t *extrema_out_host, Body body)
{
    if (!e || !x_host || !baseline_host || (extrema_host && (idx < 2 || idx > n - 1))) return ITD_ERR_INVALID_ARG;
    HostStage S(e);
    if (S.check_n(n) || S.reserve((size_t)comps * n, 2 * n)) return S.rc;
    double *d_base = S.take<double>(n);
    int64_t *d_e64 = S.take<int64_t>(n);          // the caller's list on its way in, or the detected knots on their way out
    const int32_t *ek = nullptr, *knots_dev = nullptr;
    int rc = extrema_host ? stage_extrema(S, extrema_host, idx + 1, n, d_e64, &ek) : (int)ITD_OK;
    if (!rc) rc = S.upload(S.x, x_host, comps * n);
    if (rc) return rc;
    int64_t got = 0;
    rc = body(S.x, ek, d_base, &got, S.st, extrema_host ? nullptr : &knots_dev);
    if (rc) return rc;
    if (idx_out) *idx_out = got;
    if (got >= 2) rc = S.download(baseline_host, d_base, n);     // itd.cpp:85-87: fewer than 2 knots, the caller's buffer is left alone
    if (!rc && extrema_out_host && !extrema_host && got > 0) rc = S.knots_home(extrema_out_host, knots_dev, got, d_e64);
    return rc ? rc : S.sync();
}
}  // namespace

extern "C" {

int itd_baseline_extract_cubic_f64(itd_engine *e, const double *x_dev, int64_t n, const int32_t *extrema_dev, int64_t idx,
                                   double *baseline_dev, int64_t *idx_host, void *stream)
{
    if (!e) return ITD_ERR_INVALID_ARG;
    return cubic_dev(e, x_dev, n, extrema_dev, idx, baseline_dev, idx_host, stream_of(e, stream));
}

int itd_baseline_extract_cubic_f32(itd_engine *e, const float *x_dev, int64_t n, const int32_t *extrema_dev, int64_t idx,
                                   double *baseline_dev, int64_t *idx_host, void *stream)
{
    if (!e || !x_dev) return ITD_ERR_INVALID_ARG;
    if (n < 3 || n > e->max_n) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    int rc = grow(e, e->d_io_x, (size_t)n * sizeof(double));
    if (rc) return rc;
    k_widen_f32<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(x_dev, (double *)e->d_io_x, n);   // float64 arithmetic on the widened signal
    return cubic_dev(e, (const double *)e->d_io_x, n, extrema_dev, idx, baseline_dev, idx_host, st);
}

int itd_baseline_extract_cubic_host_f64(itd_engine *e, const double *x_host, int64_t n, const int64_t *extrema_host,
                                        int64_t idx, double *baseline_host, int64_t *idx_out, int64_t *extrema_out_host)
{
    return cubic_host(e, x_host, 1, n, extrema_host, idx, baseline_host, idx_out, extrema_out_host,
                      [=](const double *x, const int32_t *ek, double *base, int64_t *got, hipStream_t st, const int32_t **knots) {
                          return cubic_dev(e, x, n, ek, idx, base, got, st, knots);
                      });
}

// The common-baseline form on complex (I/Q) data, itd.cpp:58-154 (itd_detect_fast.hpp: k_detect_fast_iq): knots where both
// components have an extremum, the natural-cubic operator of itd_baseline_extract_cubic_* on the components' mean.
int itd_baseline_extract_iq_f64(itd_engine *e, const double *iq_dev, int64_t n, const int32_t *extrema_dev, int64_t idx,
                                double *baseline_dev, int64_t *idx_host, void *stream)
{
    if (!e || !iq_dev || !baseline_dev) return ITD_ERR_INVALID_ARG;
    if (n < 3 || n > e->max_n || (reinterpret_cast<uintptr_t>(iq_dev) & 15)) return ITD_ERR_INVALID_ARG;
    if (extrema_dev && (idx < 2 || idx > n - 1)) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    int rc = grow(e, e->d_iq_avg, (size_t)n * sizeof(double));
    if (rc) return rc;
    double *avg = (double *)e->d_iq_avg;
    if (extrema_dev) {
        k_iq_mean<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(iq_dev, n, avg);
        return cubic_dev(e, avg, n, extrema_dev, idx, baseline_dev, idx_host, st);
    }
    // the shared scan around a detection kernel of its own (k_detect_fast_iq also writes the mean series)
    const KnotWs w = helper_ws(e, n);
    scan_init(w, 1, false, st);
    k_detect_fast_iq<<<w.n_tiles, kWave, 0, st>>>(iq_dev, n, w.n_tiles, w.counts, reinterpret_cast<unsigned long long *>(w.lists), w.gsum, w.state, avg);
    // the ordered list [lead slot, knots, e[idx] = 0 (itd.cpp's static array at first call)]
    scan_compact(w, n, 1, true, 0, nullptr, 0, st);
    int64_t m = 0;
    rc = fetch_total(e, w, st, &m);
    if (rc) return rc;
    if (idx_host) *idx_host = m;
    if (m < 2) return ITD_OK;                      // itd.cpp:85-87: the caller's buffer is left alone
    return cubic_dev(e, avg, n, w.kidx + 1, m, baseline_dev, nullptr, st);
}

int itd_baseline_extract_iq_host_f64(itd_engine *e, const double *iq_host, int64_t n, const int64_t *extrema_host, int64_t idx,
                                     double *baseline_host, int64_t *idx_out, int64_t *extrema_out_host)
{
    return cubic_host(e, iq_host, 2, n, extrema_host, idx, baseline_host, idx_out, extrema_out_host,
                      [=](const double *iq, const int32_t *ek, double *base, int64_t *got, hipStream_t st, const int32_t **knots) {
                          if (knots) *knots = helper_ws(e, n).kidx + 1;      // (its scan runs in the engine's fixed buffers)
                          return itd_baseline_extract_iq_f64(e, iq, n, ek, idx, base, got, st);
                      });
}

int itd_find_extrema_host_f64(itd_engine *e, const double *s_host, int64_t n, int64_t *extrema_host, int64_t *idx_out)
{
    if (!e || !s_host || !extrema_host || !idx_out) return ITD_ERR_INVALID_ARG;
    HostStage S(e);
    if (S.check_n(n) || S.reserve(n, n + 2)) return S.rc;
    int64_t *d_e64 = S.take<int64_t>(n + 2);
    int rc = S.upload(S.x, s_host, n);
    if (rc) return rc;
    int64_t m = 0;
    rc = cubic_detect(e, S.x, n, (int)kZeroCross, &m, S.st);
    if (rc) return rc;
    // d_kidx = [0, crossings (m of them), extrapolated tail]: idx = m + 2 entries, the rest of the caller's array is zero
    const int64_t idx = m + 2;
    if (idx > n) return ITD_ERR_INVALID_ARG;   // the reference's own array would overflow (every interior sample a crossing)
    memset(extrema_host, 0, (size_t)n * sizeof(int64_t));
    rc = S.knots_home(extrema_host, helper_ws(e, n).kidx, idx, d_e64);
    if (!rc) rc = S.sync();
    if (rc) return rc;
    *idx_out = idx;
    return ITD_OK;
}

// ---------------------------------------------------------------------------------------------
// The FITPACK flavour of the baseline, batched (itd_spline.hpp): itd_baseline_extract_modified,
// numba_accelerated_itd.py:182-211 (= siftED2D.ipynb cell 1); MEITD.py:303-338 with min_extrema = 0.
// ---------------------------------------------------------------------------------------------
}  // extern "C"
namespace {
// baseline (and optionally rotation) of `batch` contiguous-sample signals; all device pointers; asynchronous on st; *totals_out = the
// device array of {knot count, NaN flag} per signal.  The fit's arrays lie behind the knot scan's workspace in the same arena.
int spline_enqueue(itd_engine *e, const double *x, int64_t n, int batch, int64_t x_stride, int min_extrema, double *base,
                   int64_t base_stride, double *rot, int64_t rot_stride, hipStream_t st, const int32_t **totals_out)
{
    const int64_t lda = n + 3;                       // m <= n + ... data sites: knots <= n - 2, m <= n; 1-based arrays
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t B = (size_t)batch, b_a = al(B * 4 * (size_t)lda * sizeof(double)), b_c = al(B * (size_t)lda * sizeof(double));
    char *p = nullptr;
    KnotWs k;
    int rc = knot_workspace(e, e->d_sp, n, batch, kWsLists | kWsOrdered, k, b_a + b_c + al(B * sizeof(SplineMeta)), &p);
    if (!rc) rc = knot_scan<double>(e, k, x, x_stride, n, batch, (int)kKnots, kScanOrdered, st);
    if (rc) return rc;
    double *a = (double *)p, *c = (double *)(p + b_a);
    SplineMeta *meta = (SplineMeta *)(p + b_a + b_c);
    k_spline_fit<<<(batch + 63) / 64, 64, 0, st>>>(x, x_stride, n, batch, k.kidx, k.kidx_stride, k.totals, min_extrema, a, c, lda, meta);
    k_spline_eval<<<dim3((unsigned)((n + 255) / 256), batch), 256, 0, st>>>(x, x_stride, n, batch, k.kidx, k.kidx_stride, c, meta, base,
                                                                            base_stride, rot, rot_stride);
    HIP_TRY(e, hipGetLastError());
    *totals_out = k.totals;
    return ITD_OK;
}

// The same operator, parallel in the knots (itd_nak.hpp): the interpolating not-a-knot spline from its second derivatives.
// Asynchronous on st; *totals_out = the device array of {knot count, NaN flag} per signal.
int nak_enqueue(itd_engine *e, const double *x, int64_t n, int batch, int64_t x_stride, int min_extrema, double *base,
                int64_t base_stride, double *rot, int64_t rot_stride, hipStream_t st, const int32_t **totals_out)
{
    KnotWs w;
    int rc = knot_workspace(e, e->d_dw, n, batch, kWsDetect, w);
    if (!rc) rc = knot_scan<double>(e, w, x, x_stride, n, batch, (int)kKnots, kScanOrdered, st);     // kidx[b] = [0, knots, n-1]
    if (rc) return rc;
    CubicArgs A;
    rc = cubic_args(e, x, x_stride, n, batch, n + 2, 3, A);
    if (rc) return rc;
    CubicJob *jobs = (CubicJob *)e->d_cub;
    A.e = w.kidx; A.e_stride = w.kidx_stride; A.job_stride = 1;
    const size_t arr_n = (size_t)batch * (size_t)A.a_stride;
    double *cp = A.b + arr_n, *sub = cp + arr_n, *rhs = sub + arr_n;     // the sweeps' three arrays behind the cubic ones
    k_nak_jobs<<<(batch + 255) / 256, 256, 0, st>>>(jobs, batch, w.totals, min_extrema);
    k_nak_values<<<dim3((unsigned)((n + 255) / 256), batch), 256, 0, st>>>(A);
    k_nak_rows<<<dim3((unsigned)((n + 255) / 256), batch), 256, 0, st>>>(A, sub, rhs);
    const unsigned runs = (unsigned)((n + kNakRun - 1) / kNakRun);
    k_nak_forward<<<dim3((runs + 63) / 64, batch), 64, 0, st>>>(A, cp, sub, rhs);
    k_nak_backward<<<dim3((runs + 63) / 64, batch), 64, 0, st>>>(A, cp);
    k_cubic_eval<T, true><<<dim3((unsigned)tiles_of(n), batch), kWave, 0, st>>>(A, 0, n, base, base_stride, 1, rot, rot_stride);
    HIP_TRY(e, hipGetLastError());
    *totals_out = w.totals;
    return ITD_OK;
}

// The scalars an operator hands back, in the engine's 256 bytes of mapped pinned host memory (h_small / its device address d_small)
// that the launch fills itself: 8-byte words, the value in the low half and the call's number in the high half (small_put), each
// written whole.  Made for a call that wants its scalars this way: takes the call's number, or is false where the memory cannot be
// mapped — the caller then copies through its own buffers.
constexpr int kSmallWords = 32;
struct SmallReply {
    itd_engine *e;
    int32_t seq = 0;          // 0: no reply (not wanted, not mapped); the kernel gets (words(), seq)
    explicit SmallReply(itd_engine *eng, bool wanted = true) : e(eng)
    {
        if (!wanted) return;
        if (!e->h_small) {
            if (e->h_small.alloc(kSmallWords * 8, nullptr, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); return; }
            if (hipHostGetDevicePointer(&e->d_small, e->h_small, 0) != hipSuccess) { (void)hipGetLastError(); e->d_small = nullptr; return; }
            memset(e->h_small, 0, kSmallWords * 8);
        }
        if (e->d_small) seq = e->small_seq = e->small_seq == INT32_MAX ? 1 : e->small_seq + 1;
    }
    explicit operator bool() const { return seq != 0; }
    unsigned long long *words() const { return seq ? (unsigned long long *)e->d_small : nullptr; }
    // Wait for the launch that fills the first `nwords` words: whatever order the stores reach the host in, a result is taken only
    // when all of its words are this call's.  The host polls: a few microseconds behind the kernel's end instead of the ~25 us
    // hipStreamSynchronize takes to come back from an interrupt on a busy host.  Falls back to the synchronisation if the words do
    // not turn up within 2 ms (a long kernel, a fault).
    int wait(int nwords, hipStream_t st) const
    {
        volatile unsigned long long *w = (volatile unsigned long long *)e->h_small;
        auto all_here = [&]() {
            for (int i = 0; i < nwords; ++i) if ((uint32_t)(w[i] >> 32) != (uint32_t)seq) return false;
            return true;
        };
        const auto t0 = std::chrono::steady_clock::now();
        bool synced = false;
        for (int spin = 0; !all_here(); ++spin) {
            if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(synced ? 2000 : 2)) {
                if (synced) { snprintf(e->err, sizeof(e->err), "the launch's result words did not arrive"); return ITD_ERR_HIP; }
                HIP_TRY(e, hipStreamSynchronize(st));
                synced = true;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        return ITD_OK;
    }
    // the value at word i: 32 bits in one word, 64 bits in two (low half first)
    uint32_t u32(int i) const { return (uint32_t)((const volatile unsigned long long *)e->h_small)[i]; }
    uint64_t u64(int i) const { return (uint64_t)u32(i) | ((uint64_t)u32(i + 1) << 32); }
};

// What the one-workgroup solver works on (k_nak_small, k_meitd_small, k_meitd_batch), per signal: the knot indices, then six arrays
// of L = n + 2 doubles (K, dpg, M, cpg, subg, rhsg), each part 256-byte aligned.  The sweeps' four arrays live in dynamic LDS where
// they fit (more than 64 KB of it has to be asked for).
struct NakSmallWs {
    int32_t *idx;                    // signal 0's block starts here; signal g's: sig_bytes further each
    double *arr;
    int64_t L;
    size_t idx_bytes, sig_bytes;
    bool in_lds;
    size_t lds;                      // the launch's dynamic LDS
    double *a(int k) const { return arr + k * L; }
};
// `count` signals' blocks at `offset` bytes of a grow-only arena, `tail` bytes for the caller behind the last one.  lds_floor: dynamic LDS the
// kernel takes whatever the sweeps need (MEITD's entropy pass takes turns with them in the same bytes)
int nak_small_ws(itd_engine *e, Buf<void> &arena, size_t offset, int64_t n, int count, size_t tail, size_t lds_floor, NakSmallWs &w)
{
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    w.L = n + 2;
    w.idx_bytes = al((size_t)w.L * sizeof(int32_t));
    w.sig_bytes = w.idx_bytes + al(6 * (size_t)w.L * sizeof(double));
    const size_t sweeps = 4 * (size_t)w.L * sizeof(double);
    w.in_lds = sweeps <= kNakSmallLdsMax;
    w.lds = std::max(w.in_lds ? sweeps : (size_t)0, lds_floor);
    const int rc = grow(e, arena, offset + (size_t)count * w.sig_bytes + tail);
    if (rc) return rc;
    w.idx = (int32_t *)((char *)arena + offset);
    w.arr = (double *)((char *)arena + offset + w.idx_bytes);
    return ITD_OK;
}
// launches the instance of a one-workgroup kernel that matches the workspace, granted its LDS
template <typename... P, typename... A>
int nak_small_launch(itd_engine *e, const NakSmallWs &w, void (*in_lds)(P...), void (*in_memory)(P...), unsigned grid, hipStream_t st, A... args)
{
    void (*const fn)(P...) = w.in_lds ? in_lds : in_memory;
    const size_t grant = w.in_lds ? kNakSmallLdsMax : w.lds;      // (arrays in memory: the floor alone, if any)
    if (grant) HIP_TRY(e, allow_lds(e, reinterpret_cast<const void *>(fn), grant));
    fn<<<grid, kNakSmallThreads, w.lds, st>>>(args...);
    HIP_TRY(e, hipGetLastError());
    return ITD_OK;
}

// ONE signal of at most kNakSmallMax samples through the parallel-in-knots form: one launch, one workgroup (itd_nak.hpp: k_nak_small),
// four words back — knots, NaN flag, validity, and (baseline_knots_host) the knot count of the produced baseline.  Synchronous.
int nak_small(itd_engine *e, const double *x, int64_t n, int min_extrema, double *base, double *rot, hipStream_t st,
              int32_t *knots_host, int32_t *baseline_knots_host)
{
    NakSmallWs w;
    int rc = nak_small_ws(e, e->d_cub, 256, n, 1, 0, 0, w);     // (in front: the kernel's four words where nothing is mapped)
    if (rc) return rc;
    int32_t *out = (int32_t *)e->d_cub;
    const SmallReply reply(e);
    rc = nak_small_launch(e, w, k_nak_small<true>, k_nak_small<false>, 1, st, x, (int)n, min_extrema, w.idx, w.a(0), w.a(1), w.a(2), w.a(3),
                          w.a(4), w.a(5), base, rot, baseline_knots_host ? 1 : 0, out, reply.words(), reply.seq);
    if (rc) return rc;
    int32_t h[4] = {0, 0, 0, 0};
    if (reply) {
        rc = reply.wait(4, st);
        if (rc) return rc;
        for (int q = 0; q < 4; ++q) h[q] = (int32_t)reply.u32(q);
    } else {
        HIP_TRY(e, hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_TRY(e, hipStreamSynchronize(st));
    }
    if (knots_host) knots_host[0] = h[0];
    if (baseline_knots_host) baseline_knots_host[0] = h[3];
    return h[1] ? ITD_ERR_NONFINITE : ITD_OK;
}

// The extraction behind every entry below: device pointers, `batch` contiguous-sample signals; st NULL = the engine's own stream.
// The form is the policy's (itd_policy.hpp: spline_form).  baseline_knots_host: also the knot count of every PRODUCED baseline — what
// MEITD's loops ask for right after an extraction (MEITD.py:362-363, :497-505) — in the same synchronisation.  Synchronous; a NaN in
// a signal is ITD_ERR_NONFINITE, a NaN in a produced baseline is not an error of its own.
int spline_extract(itd_engine *e, const double *x, int64_t n, int32_t batch, int64_t x_stride, int32_t min_extrema, double *base,
                   int64_t base_stride, double *rot, int64_t rot_stride, int32_t *knots_host, int32_t *baseline_knots_host, hipStream_t st)
{
    if (!e || !x || !base) return ITD_ERR_INVALID_ARG;
    if (n < 3 || n >= (int64_t)INT32_MAX - 8 || batch < 1 || batch > kMaxGridY || min_extrema < 0) return ITD_ERR_INVALID_ARG;
    if (batch > 1 && (x_stride < n || base_stride < n || (rot && rot_stride < n))) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    st = stream_of(e, st);
    const SplineForm form = spline_form(e->spline_solver, n, batch);
    if (form == SplineForm::Small) return nak_small(e, x, n, min_extrema, base, rot, st, knots_host, baseline_knots_host);
    const int32_t *totals = nullptr;
    int rc = (form == SplineForm::Parallel ? nak_enqueue : spline_enqueue)(e, x, n, batch, x_stride, min_extrema, base, base_stride, rot,
                                                                           rot_stride, st, &totals);
    if (rc) return rc;
    if (!baseline_knots_host) return fetch_totals(e, totals, batch, knots_host, st);
    // (the extraction's totals are read before the counting launches reuse the detection workspace)
    std::vector<int32_t> tot((size_t)batch * 2);
    HIP_TRY(e, hipMemcpyAsync(tot.data(), totals, tot.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    KnotWs dw;
    rc = knot_workspace(e, e->d_dw, n, batch, kWsDetect, dw);
    if (!rc) rc = knot_scan<double>(e, dw, base, base_stride, n, batch, (int)kKnots, kScanTotals, st);
    if (!rc) rc = fetch_totals(e, dw.totals, batch, baseline_knots_host, st, false);   // (one synchronisation for both)
    return rc ? rc : read_totals(tot.data(), batch, knots_host);                        // (the NaN flags that count are the extraction's)
}

}  // namespace
extern "C" {

int itd_baseline_extract_spline_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride,
                                    int32_t min_extrema, double *baseline_dev, int64_t baseline_stride, double *rot_dev,
                                    int64_t rot_stride, int32_t *knots_host, void *stream)
{
    return spline_extract(e, x_dev, n, batch, x_stride, min_extrema, baseline_dev, baseline_stride, rot_dev, rot_stride, knots_host, nullptr,
                          (hipStream_t)stream);
}

// the same plus the knot count of every PRODUCED baseline, one synchronisation for both
int itd_baseline_extract_spline2_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride,
                                     int32_t min_extrema, double *baseline_dev, int64_t baseline_stride, double *rot_dev,
                                     int64_t rot_stride, int32_t *knots_host, int32_t *baseline_knots_host, void *stream)
{
    return spline_extract(e, x_dev, n, batch, x_stride, min_extrema, baseline_dev, baseline_stride, rot_dev, rot_stride, knots_host,
                          baseline_knots_host, (hipStream_t)stream);
}

int itd_set_spline_solver(itd_engine *e, int32_t solver)
{
    if (!e || solver < ITD_SPLINE_AUTO || solver > ITD_SPLINE_PARALLEL) return ITD_ERR_INVALID_ARG;
    e->spline_solver = solver;
    return ITD_OK;
}

int itd_baseline_extract_spline_host_f64(itd_engine *e, const double *x_host, int64_t n, int32_t batch, int32_t min_extrema,
                                         double *baseline_host, double *rot_host, int32_t *knots_host)
{
    return itd_baseline_extract_spline_host2_f64(e, x_host, n, batch, min_extrema, baseline_host, rot_host, knots_host, nullptr);
}

// host arrays in and out: upload, the extraction (with the produced baselines' knot counts if asked for: counted on the data already
// on the device instead of another upload / list download), download
int itd_baseline_extract_spline_host2_f64(itd_engine *e, const double *x_host, int64_t n, int32_t batch, int32_t min_extrema,
                                          double *baseline_host, double *rot_host, int32_t *knots_host, int32_t *baseline_knots_host)
{
    if (!e || !x_host || !baseline_host) return ITD_ERR_INVALID_ARG;
    if (n < 3 || batch < 1) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = e->own_stream;
    const size_t cnt = (size_t)n * (size_t)batch;
    int rc = grow(e, e->d_sp2, 3 * cnt * sizeof(double));
    if (rc) return rc;
    double *d_x = e->d_sp2, *d_b = d_x + cnt, *d_r = d_b + cnt;
    HIP_TRY(e, hipMemcpyAsync(d_x, x_host, cnt * sizeof(double), hipMemcpyHostToDevice, st));
    rc = spline_extract(e, d_x, n, batch, n, min_extrema, d_b, n, rot_host ? d_r : nullptr, n, knots_host, baseline_knots_host, st);
    if (rc) return rc;
    HIP_TRY(e, hipMemcpyAsync(baseline_host, d_b, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
    if (rot_host) HIP_TRY(e, hipMemcpyAsync(rot_host, d_r, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    return ITD_OK;
}

// knot counts of host signals without any index list (matlab_detect_peaks(x).size + matlab_detect_peaks(-x).size for mode
// ITD_DETECT_KNOTS, MEITD.py:350, :376, :409): upload, one counting launch pair, 4 bytes per signal back
int itd_count_knots_host_f64(itd_engine *e, const double *x_host, int64_t n, int32_t batch, int32_t mode, int32_t *counts_host)
{
    if (!e || !x_host || !counts_host || n < 3 || batch < 1 || batch > kMaxGridY || mode < 0 || mode > 4) return ITD_ERR_INVALID_ARG;
    const size_t cnt = (size_t)n * (size_t)batch;
    HostStage S(e);
    if (S.reserve(cnt, 0)) return S.rc;
    int rc = S.upload(S.x, x_host, (int64_t)cnt);
    if (rc) return rc;
    KnotWs w;
    rc = knot_workspace(e, e->d_dw, n, batch, kWsDetect, w);
    if (!rc) rc = knot_scan<double>(e, w, S.x, n, n, batch, mode, kScanTotals, S.st);
    if (rc) return rc;
    rc = fetch_totals(e, w.totals, batch, counts_host, S.st);     // counted under the plain rules: see itd_detect_* for detect_peaks' NaN branch
    if (rc != ITD_ERR_HIP) S.settled();                            // (the totals' copy has synchronised)
    return rc;
}

// ---- MEITD's operators on device-resident signals (MEITD.py:344-534 keeps one signal and its rotations / baselines in a loop:
//      nothing but a few scalars has to cross PCIe per pass) -----------------------------------------------------------------
int itd_count_knots_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride, int32_t mode,
                        int32_t *counts_host, void *stream)
{
    if (!e || !x_dev || !counts_host || n < 3 || batch < 1 || batch > kMaxGridY || mode < 0 || mode > 4) return ITD_ERR_INVALID_ARG;
    if (batch > 1 && x_stride < n) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    KnotWs w;
    int rc = knot_workspace(e, e->d_dw, n, batch, kWsDetect, w);
    if (!rc) rc = knot_scan<double>(e, w, x_dev, x_stride, n, batch, mode, kScanTotals, st);
    if (rc) return rc;
    const SmallReply reply(e, 2 * batch <= kSmallWords);
    if (reply) {                  // a few counts: the GPU copies them into the mapped words itself
        k_copy_words<<<1, 64, 0, st>>>(w.totals, reply.words(), 2 * batch, reply.seq);
        HIP_TRY(e, hipGetLastError());
        rc = reply.wait(2 * batch, st);
        if (rc) return rc;
        int32_t tot[kSmallWords];
        for (int i = 0; i < 2 * batch; ++i) tot[i] = (int32_t)reply.u32(i);
        return read_totals(tot, batch, counts_host);
    } else
        return fetch_totals(e, w.totals, batch, counts_host, st);
}

// the weighted sums and window counts of the six order-3 permutation patterns of x (itd_wpe.hpp; MEITD.py:79-128), and —
// optionally, in the same synchronisation — x's knot count: MEITD.py:346-351 and :373-378 ask for both of the same signal
int itd_wpe3_f64(itd_engine *e, const double *x_dev, int64_t n, double *bin_weights_host, int64_t *bin_windows_host,
                 int32_t *knots_host, void *stream)
{
    if (!e || !x_dev || !bin_weights_host || !bin_windows_host || n < 3) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    const int64_t nw = n - 2;
    const bool exact = nw <= kWpeExactWindows;
    const int64_t seg_len = exact ? nw : kWpeSeg;
    const int64_t nseg = (nw + seg_len - 1) / seg_len;
    if (nseg > INT32_MAX / 8) return ITD_ERR_INVALID_ARG;
    const size_t out_off = (size_t)nseg * (6 * (sizeof(double) + sizeof(long long)) + 2 * sizeof(int));    // the segments' sums, then the totals
    int rc = grow(e, e->d_wpe, out_off + 6 * (sizeof(double) + sizeof(long long)) + 2 * sizeof(int));
    if (rc) return rc;
    double *part_s = reinterpret_cast<double *>(e->d_wpe.get());
    long long *part_c = reinterpret_cast<long long *>(part_s + (size_t)nseg * 6);
    int *part_k = reinterpret_cast<int *>(part_c + (size_t)nseg * 6);
    double *out_s = reinterpret_cast<double *>(e->d_wpe + out_off);
    long long *out_c = reinterpret_cast<long long *>(out_s + 6);
    int *out_k = reinterpret_cast<int *>(out_c + 6);
    // (one segment — MEITD's signals —: the sums land in the engine's mapped host words, no copy behind the launch.  The knot count
    // of x rides along: a window's middle sample is a knot or not — MEITD.py:346-351, :373-378 ask for both)
    const SmallReply reply(e, nseg == 1);
    k_wpe3<<<(unsigned)nseg, kWpeThreads, 0, st>>>(x_dev, nw, seg_len, part_s, part_c, knots_host ? part_k : nullptr, reply.words(), reply.seq);
    if (nseg > 1) k_wpe3_combine<<<1, 64, 0, st>>>(part_s, part_c, (int)nseg, out_s, out_c, knots_host ? part_k : nullptr, out_k);
    HIP_TRY(e, hipGetLastError());
    struct { double s[6]; long long c[6]; int k[2]; } res;
    res.k[0] = res.k[1] = 0;
    if (reply) {                  // words 0..11: the six sums, 12..17: the six window counts, 18: the knots, 19: the NaN flag
        rc = reply.wait(20, st);
        if (rc) return rc;
        for (int b = 0; b < 6; ++b) {
            const uint64_t bits = reply.u64(2 * b);
            memcpy(&res.s[b], &bits, sizeof(double));
            res.c[b] = (long long)reply.u32(12 + b);
        }
        res.k[0] = (int)reply.u32(18); res.k[1] = (int)reply.u32(19);
    } else {
        const size_t res_b = 6 * (sizeof(double) + sizeof(long long)) + (knots_host ? 2 * sizeof(int) : 0);
        HIP_TRY(e, hipMemcpyAsync(&res, nseg > 1 ? out_s : part_s, res_b, hipMemcpyDeviceToHost, st));
        HIP_TRY(e, hipStreamSynchronize(st));
    }
    for (int b = 0; b < 6; ++b) { bin_weights_host[b] = res.s[b]; bin_windows_host[b] = (int64_t)res.c[b]; }
    if (knots_host) *knots_host = res.k[0];
    return knots_host && res.k[1] ? ITD_ERR_NONFINITE : ITD_OK;
}

// MEITD's whole selection loop on one short device-resident signal as one launch (itd_meitd.hpp: k_meitd_small).  Synchronous.
int itd_meitd_small_f64(itd_engine *e, double *rows_dev, int64_t n, double wpemax, int32_t *result_host, void *probe_log_host,
                        int32_t log_cap, void *stream)
{
    if (!e || !rows_dev || !result_host || log_cap < 0 || (log_cap > 0 && !probe_log_host)) return ITD_ERR_INVALID_ARG;
    // (only where the host-driven loop's extractions take the same operator: the parallel-in-knots form of one signal)
    if (!meitd_one_launch(e->spline_solver, n)) return ITD_ERR_INVALID_ARG;     // (bounds n too: 3 .. kNakSmallMax, so (int)n below is safe)
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    NakSmallWs w;               // (the two operators take turns in the same LDS; in front of the workspace: the result, behind it: the log)
    int rc = nak_small_ws(e, e->d_cub, 256, n, 1, kMeitdLogCap * sizeof(MeitdProbe), kMeitdWpeLds, w);
    if (rc) return rc;
    MeitdOut *dout = (MeitdOut *)e->d_cub;
    MeitdProbe *dlog = (MeitdProbe *)((char *)w.idx + w.sig_bytes);
    rc = nak_small_launch(e, w, k_meitd_small<true>, k_meitd_small<false>, 1, st, rows_dev, (int)n, wpemax, w.idx, w.a(0), w.a(1), w.a(2), w.a(3),
                          w.a(4), w.a(5), dlog, dout);
    if (rc) return rc;
    // (a whole loop: milliseconds — the header and the log are plain copies behind it)
    MeitdOut ho;
    HIP_TRY(e, hipMemcpyAsync(&ho, dout, sizeof(ho), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    memcpy(result_host, &ho, sizeof(MeitdOut));
    const int32_t got = result_host[4] < log_cap ? result_host[4] : log_cap;
    if (got > 0) HIP_TRY(e, hipMemcpy(probe_log_host, dlog, (size_t)(got < kMeitdLogCap ? got : kMeitdLogCap) * sizeof(MeitdProbe), hipMemcpyDeviceToHost));
    return ITD_OK;
}

// MEITD's selection loop on a batch of short device-resident signals, one workgroup per signal (itd_meitd.hpp: k_meitd_batch).
// Synchronous; launches of at most kMaxGridY signals.  The per-signal scratch is the engine's d_mb, apart from every other workspace;
// above kMeitdBatchKeepBytes it is freed when the call returns.
constexpr size_t kMeitdBatchKeepBytes = (size_t)64 << 20;
int itd_meitd_batch_f64(itd_engine *e, double *rows_dev, int64_t n, int32_t batch, int64_t rows_stride, const double *x_host, double wpemax,
                        int32_t *result_host, void *probe_logs_host, int32_t log_cap, double *xitd_sums_host, int64_t *xitd_windows_host,
                        void *stream)
{
    if (!e || !rows_dev || !result_host || batch < 1 || log_cap < 0 || (log_cap > 0 && !probe_logs_host)) return ITD_ERR_INVALID_ARG;
    // (the same rule as itd_meitd_small_f64: where the host-driven loop's extractions take the parallel-in-knots form)
    if (!meitd_one_launch(e->spline_solver, n)) return ITD_ERR_INVALID_ARG;     // (bounds n too: 3 .. kNakSmallMax, so (int)n below is safe)
    if (rows_stride < (int64_t)(kMeitdWork + 2 * kMeitdKept) * n || (!xitd_sums_host) != (!xitd_windows_host)) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    const int grid_max = batch < kMaxGridY ? batch : kMaxGridY;
    const bool xitd = xitd_sums_host != nullptr;
    const size_t out_b = (((size_t)grid_max * sizeof(MeitdOut)) + 255) & ~(size_t)255;
    const size_t log_b = (size_t)grid_max * kMeitdLogCap * sizeof(MeitdProbe);
    const size_t xs_b = xitd ? (size_t)grid_max * kMeitdKept * 6 * (sizeof(double) + sizeof(long long)) : 0;
    const size_t x_b = x_host ? (((size_t)grid_max * (size_t)n * sizeof(double)) + 255) & ~(size_t)255 : 0;
    // results, logs, XITD's sums, the signals' solver workspaces, the staged signals; the logs are packed, as far as the longest
    // reaches, behind everything else before they go to the host: log_b more
    NakSmallWs w;
    int rc = nak_small_ws(e, e->d_mb, out_b + log_b + xs_b, n, grid_max, x_b + log_b, kMeitdWpeLds, w);
    if (rc) return rc;
    MeitdOut *dout = (MeitdOut *)e->d_mb;
    MeitdProbe *dlog = (MeitdProbe *)((char *)e->d_mb + out_b);
    double *dxw = xitd ? (double *)((char *)e->d_mb + out_b + log_b) : nullptr;
    long long *dxc = xitd ? (long long *)(dxw + (size_t)grid_max * kMeitdKept * 6) : nullptr;
    char *tail = (char *)w.idx + (size_t)grid_max * w.sig_bytes;
    double *dx = x_host ? (double *)tail : nullptr;
    MeitdProbe *dpack = (MeitdProbe *)(tail + x_b);
    const int32_t cap = log_cap < kMeitdLogCap ? log_cap : kMeitdLogCap;
    std::vector<MeitdOut> ho((size_t)grid_max);
    std::vector<MeitdProbe> hlog;
    for (int32_t b0 = 0; b0 < batch; b0 += grid_max) {
        const int32_t G = batch - b0 < grid_max ? batch - b0 : grid_max;
        double *rows = rows_dev + (size_t)b0 * (size_t)rows_stride;
        // (the signals as one contiguous copy; each workgroup moves its own into row 5 of its block)
        if (x_host) HIP_TRY(e, hipMemcpyAsync(dx, x_host + (size_t)b0 * (size_t)n, (size_t)G * (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        rc = nak_small_launch(e, w, k_meitd_batch<true>, k_meitd_batch<false>, (unsigned)G, st, dx, rows, rows_stride, (int)n, wpemax, (char *)w.idx,
                              (int64_t)w.sig_bytes, (int64_t)w.idx_bytes, w.L, dlog, dout, dxw, dxc);
        if (rc) return rc;
        HIP_TRY(e, hipMemcpyAsync(ho.data(), dout, (size_t)G * sizeof(MeitdOut), hipMemcpyDeviceToHost, st));
        HIP_TRY(e, hipStreamSynchronize(st));
        int32_t most = 0;
        for (int32_t b = 0; b < G; ++b) {
            memcpy(result_host + ((size_t)b0 + b) * 24, &ho[(size_t)b], sizeof(MeitdOut));
            most = ho[(size_t)b].probes > most ? ho[(size_t)b].probes : most;
        }
        most = most < cap ? most : cap;
        // (every signal's log as far as the longest one reaches: packed on the device, then one copy)
        if (most > 0) {
            HIP_TRY(e, hipMemcpy2DAsync(dpack, (size_t)most * sizeof(MeitdProbe), dlog, kMeitdLogCap * sizeof(MeitdProbe), (size_t)most * sizeof(MeitdProbe),
                                        (size_t)G, hipMemcpyDeviceToDevice, st));
            hlog.resize((size_t)G * (size_t)most);
            HIP_TRY(e, hipMemcpyAsync(hlog.data(), dpack, hlog.size() * sizeof(MeitdProbe), hipMemcpyDeviceToHost, st));
        }
        if (xitd) {
            static_assert(sizeof(long long) == sizeof(int64_t), "XITD's window counts are 64-bit on both sides");
            HIP_TRY(e, hipMemcpyAsync(xitd_sums_host + (size_t)b0 * kMeitdKept * 6, dxw, (size_t)G * kMeitdKept * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_TRY(e, hipMemcpyAsync(xitd_windows_host + (size_t)b0 * kMeitdKept * 6, dxc, (size_t)G * kMeitdKept * 6 * sizeof(long long), hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(e, hipStreamSynchronize(st));
        for (int32_t b = 0; most > 0 && b < G; ++b)
            memcpy((char *)probe_logs_host + ((size_t)b0 + b) * log_cap * sizeof(MeitdProbe), hlog.data() + (size_t)b * most, (size_t)most * sizeof(MeitdProbe));
    }
    if (e->d_mb.bytes() > kMeitdBatchKeepBytes) e->d_mb.release();   // (a large batch's workspace does not stay allocated behind the call)
    return ITD_OK;
}

__global__ void k_gather_rows(const double *__restrict__ src, const int64_t *__restrict__ tab, int64_t rows, int64_t n, double *__restrict__ dst)
{
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const double *s = src + tab[r];
        double *d = dst + r * n;
        for (int64_t i = threadIdx.x; i < n; i += blockDim.x) d[i] = s[i];
    }
}

// rows of n float64 at element offsets of src_dev, one after the other into dst_dev: one upload of the table, one launch; then (dst_host)
// one download through the pinned bounce buffers.  Synchronous.
int itd_gather_rows_f64(itd_engine *e, const double *src_dev, int64_t src_elems, const int64_t *offsets_host, int64_t rows, int64_t n,
                        double *dst_dev, double *dst_host, void *stream)
{
    if (!e || !src_dev || !offsets_host || !dst_dev || rows < 0 || rows > INT32_MAX || n < 1 || src_elems < n) return ITD_ERR_INVALID_ARG;
    for (int64_t r = 0; r < rows; ++r)
        if (offsets_host[r] < 0 || offsets_host[r] > src_elems - n) return ITD_ERR_INVALID_ARG;
    if (rows == 0) return ITD_OK;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    int rc = grow(e, e->d_rowtab, (size_t)rows * sizeof(int64_t));
    if (rc) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->d_rowtab, offsets_host, (size_t)rows * sizeof(int64_t), hipMemcpyHostToDevice, st));
    k_gather_rows<<<(unsigned)(rows < 65536 ? rows : 65536), 256, 0, st>>>(src_dev, e->d_rowtab, rows, n, dst_dev);
    HIP_TRY(e, hipGetLastError());
    if (dst_host) return copy_to_host(e, dst_host, dst_dev, (size_t)rows * (size_t)n * sizeof(double), st);
    HIP_TRY(e, hipStreamSynchronize(st));
    return ITD_OK;
}

// weighted_permutation_entropy's pass over the samples for any order 2 .. 5: sums_host / windows_host [order^order], indexed by the
// reference's hash value (a hash without windows is absent from its list)
int itd_wpe_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t order, double *sums_host, int64_t *windows_host, void *stream)
{
    if (!e || !x_dev || !sums_host || !windows_host || order < 2 || order > kWpeMaxOrder || n < order) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    const int64_t nw = n - order + 1;
    int nh = 1;
    for (int k = 0; k < order; ++k) nh *= order;
    const int64_t seg_len = nw <= kWpeExactWindows ? nw : kWpeSeg * 4;
    const int64_t nseg = (nw + seg_len - 1) / seg_len;
    if (nseg > 65535) return ITD_ERR_INVALID_ARG;
    const size_t wts_off = ((size_t)nw * sizeof(unsigned short) + 255) / 256 * 256;
    const size_t part_off = wts_off + (size_t)nw * sizeof(double);
    const size_t out_off = part_off + (size_t)nseg * nh * (sizeof(double) + sizeof(long long));
    int rc = grow(e, e->d_wpe, out_off + (size_t)nh * (sizeof(double) + sizeof(long long)));
    if (rc) return rc;
    unsigned short *hashes = reinterpret_cast<unsigned short *>(e->d_wpe.get());
    double *wts = reinterpret_cast<double *>(e->d_wpe + wts_off);
    double *part_s = reinterpret_cast<double *>(e->d_wpe + part_off);
    long long *part_c = reinterpret_cast<long long *>(part_s + (size_t)nseg * nh);
    double *out_s = reinterpret_cast<double *>(e->d_wpe + out_off);
    long long *out_c = reinterpret_cast<long long *>(out_s + nh);
    const unsigned gb = (unsigned)((nw + 255) / 256);
    switch (order) {
    case 2: k_wpe_eval<2><<<gb, 256, 0, st>>>(x_dev, nw, hashes, wts); break;
    case 3: k_wpe_eval<3><<<gb, 256, 0, st>>>(x_dev, nw, hashes, wts); break;
    case 4: k_wpe_eval<4><<<gb, 256, 0, st>>>(x_dev, nw, hashes, wts); break;
    default: k_wpe_eval<5><<<gb, 256, 0, st>>>(x_dev, nw, hashes, wts); break;
    }
    k_wpe_sum<<<dim3((unsigned)((nh + 255) / 256), (unsigned)nseg), 256, 0, st>>>(hashes, wts, nw, seg_len, nh, part_s, part_c);
    if (nseg > 1) k_wpe_combine<<<(unsigned)((nh + 255) / 256), 256, 0, st>>>(part_s, part_c, (int)nseg, nh, out_s, out_c);
    HIP_TRY(e, hipGetLastError());
    std::vector<long long> cnt((size_t)nh);
    HIP_TRY(e, hipMemcpyAsync(sums_host, nseg > 1 ? out_s : part_s, (size_t)nh * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipMemcpyAsync(cnt.data(), nseg > 1 ? out_c : part_c, (size_t)nh * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    for (int h = 0; h < nh; ++h) windows_host[h] = (int64_t)cnt[(size_t)h];
    return ITD_OK;
}

int itd_subtract_f64(itd_engine *e, const double *a_dev, const double *b_dev, double *out_dev, int64_t count, void *stream)
{
    if (!e || !a_dev || !b_dev || !out_dev || count < 0) return ITD_ERR_INVALID_ARG;
    if (!count) return ITD_OK;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    k_subtract<<<(unsigned)((count + 255) / 256), 256, 0, st>>>(a_dev, b_dev, out_dev, count);
    HIP_TRY(e, hipGetLastError());
    return ITD_OK;
}

// copies ordered on the engine's stream (or `stream`): kind 0 device -> host, 1 host -> device, 2 device -> device,
// 3 zero bytes (src ignored); wait != 0: return when it is done
int itd_copy(itd_engine *e, void *dst, const void *src, int64_t bytes, int32_t kind, int32_t wait, void *stream)
{
    if (!e || !dst || (!src && kind != 3) || bytes < 0 || kind < 0 || kind > 3) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    if (bytes) {
        if (kind == 3) HIP_TRY(e, hipMemsetAsync(dst, 0, (size_t)bytes, st));
        else HIP_TRY(e, hipMemcpyAsync(dst, src, (size_t)bytes, kind == 0 ? hipMemcpyDeviceToHost : (kind == 1 ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice), st));
    }
    if (wait) HIP_TRY(e, hipStreamSynchronize(st));
    return ITD_OK;
}

// crossways_itd_baseline_extract(data), siftED2D.ipynb cell 1, for `planes` images of rows x cols (device, contiguous):
// rows then columns of the rows' result, columns then rows of the columns' result, averaged.
int itd_crossways_f64(itd_engine *e, const double *img_dev, int32_t planes, int32_t rows, int32_t cols, int32_t min_extrema,
                      double *out_dev, void *stream)
{
    if (!e || !img_dev || !out_dev || planes < 1 || rows < 3 || cols < 3) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    const size_t cnt = (size_t)planes * rows * cols;
    int rc = grow(e, e->d_sp2, 3 * cnt * sizeof(double));
    if (rc) return rc;
    double *A = e->d_sp2, *Bq = A + cnt, *C = Bq + cnt;       // scratch planes
    auto tr = [&](const double *in, int r, int c, double *out) {
        k_transpose<<<dim3((c + 31) / 32, (r + 31) / 32, planes), 256, 0, st>>>(in, r, c, out);
    };
    HIP_TRY(e, hipMemsetAsync(e->d_flag, 0, sizeof(int32_t), st));
    // every row of `sigs` x `len`, in chunks of at most 65535 signals (they are the launches' grid.y: 20 ensemble planes of a
    // 3840 x 2160 image are 76 800 rows per stage); the NaN-input flags of every chunk of every stage are OR-ed into d_flag
    auto ext = [&](const double *in, int64_t sigs, int len, double *out) {
        for (int64_t s0 = 0; s0 < sigs; s0 += kMaxGridY) {
            const int nb = (int)std::min<int64_t>(kMaxGridY, sigs - s0);
            const int32_t *totals = nullptr;
            const int rc2 = spline_enqueue(e, in + s0 * len, len, nb, len, min_extrema, out + s0 * len, len, nullptr, 0, st, &totals);
            if (rc2) return rc2;
            k_or_nan_flags<<<(nb + 255) / 256, 256, 0, st>>>(totals, nb, e->d_flag);
        }
        return (int)ITD_OK;
    };
    // lengthwise = rows(data); then its columns
    if ((rc = ext(img_dev, (int64_t)planes * rows, cols, A))) return rc;    // A = lengthwise (rows done)
    tr(A, rows, cols, Bq);                                                  // Bq = lengthwise^T  [cols][rows]
    if ((rc = ext(Bq, (int64_t)planes * cols, rows, A))) return rc;         // A = columns of lengthwise, transposed layout
    tr(A, cols, rows, C);                                                   // C = lengthwise, final [rows][cols]
    // crosswise = columns(data); then its rows
    tr(img_dev, rows, cols, A);                                             // A = data^T
    if ((rc = ext(A, (int64_t)planes * cols, rows, Bq))) return rc;         // Bq = columns of data (transposed layout)
    tr(Bq, cols, rows, A);                                                  // A = crosswise [rows][cols]
    if ((rc = ext(A, (int64_t)planes * rows, cols, Bq))) return rc;         // Bq = rows of crosswise
    k_mean2<<<(unsigned)((cnt + 255) / 256), 256, 0, st>>>(C, Bq, (int64_t)cnt, out_dev);
    HIP_TRY(e, hipGetLastError());
    int32_t nan_in = 0;     // a NaN in any row of any of the four stages
    HIP_TRY(e, hipMemcpyAsync(&nan_in, e->d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    return nan_in ? ITD_ERR_NONFINITE : ITD_OK;
}

int itd_crossways_host_f64(itd_engine *e, const double *img_host, int32_t planes, int32_t rows, int32_t cols, int32_t min_extrema,
                           double *out_host)
{
    if (!e || !img_host || !out_host || planes < 1 || rows < 3 || cols < 3) return ITD_ERR_INVALID_ARG;
    const int64_t cnt = (int64_t)planes * rows * cols;
    HostStage S(e);
    if (S.reserve(0, 2 * (size_t)cnt)) return S.rc;        // both sides in d_io_rows
    double *d_in = S.take<double>(cnt), *d_out = S.take<double>(cnt);
    int rc = S.upload(d_in, img_host, cnt);
    if (rc) return rc;
    rc = itd_crossways_f64(e, d_in, planes, rows, cols, min_extrema, d_out, S.st);
    if (!rc) rc = S.download(out_host, d_out, cnt);
    return rc ? rc : S.sync();
}

// ---------------------------------------------------------------------------------------------
// Instantaneous amplitude / phase / frequency of a proper rotation (itd_tfe.hpp; README.md:13-21, 41-55).
// ---------------------------------------------------------------------------------------------
int itd_instantaneous_f64(itd_engine *e, const double *rot_dev, int64_t n, double *amp_dev, double *phase_dev, double *freq_dev,
                          void *stream)
{
    if (!e || !rot_dev || (!amp_dev && !phase_dev && !freq_dev)) return ITD_ERR_INVALID_ARG;
    if (n < 3 || n > e->max_n) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    int64_t m = 0;
    int rc = cubic_detect(e, rot_dev, n, (int)kZeroCross, &m, st);   // ordered zero crossings in d_kidx[1..m]
    if (rc) return rc;
    rc = grow(e, e->d_cub, (size_t)(m + 2) * sizeof(unsigned long long));
    if (rc) return rc;
    unsigned long long *amp_bits = (unsigned long long *)e->d_cub;
    HIP_TRY(e, hipMemsetAsync(amp_bits, 0, (size_t)(m + 1) * sizeof(unsigned long long), st));
    static_assert(kTfeTile == T, "k_compact's per-tile bases are per T samples");
    const unsigned blocks = (unsigned)tiles_of(n);
    const int32_t *tile_base = helper_ws(e, n).tbase;   // crossings in front of every tile (k_compact)
    k_tfe_amplitude<<<blocks, 64, 0, st>>>(rot_dev, n, tile_base, amp_bits);
    k_tfe_phase<<<blocks, 64, 0, st>>>(rot_dev, n, tile_base, amp_bits, amp_dev, phase_dev, freq_dev);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, hipStreamSynchronize(st));
    return ITD_OK;
}

int itd_instantaneous_host_f64(itd_engine *e, const double *rot_host, int64_t n, double *amp_host, double *phase_host,
                               double *freq_host)
{
    if (!e || !rot_host) return ITD_ERR_INVALID_ARG;
    HostStage S(e);
    if (S.check_n(n) || S.reserve(n, 3 * n)) return S.rc;
    double *d_a = S.take<double>(n), *d_p = S.take<double>(n), *d_f = S.take<double>(n);
    int rc = S.upload(S.x, rot_host, n);
    if (rc) return rc;
    rc = itd_instantaneous_f64(e, S.x, n, d_a, d_p, d_f, S.st);
    if (!rc && amp_host) rc = S.download(amp_host, d_a, n);
    if (!rc && phase_host) rc = S.download(phase_host, d_p, n);
    if (!rc && freq_host) rc = S.download(freq_host, d_f, n);
    return rc ? rc : S.sync();
}

int itd_set_kernel_timing(itd_engine *e, int max_decompositions)
{
    if (!e || max_decompositions < 0 || max_decompositions > 4096) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    e->timing = max_decompositions > 0;
    e->timing_seq = 0;
    e->n_timed = 0;
    e->timing_overflow = false;
    const size_t want = 2 * (size_t)max_decompositions * (ITD_MAX_ROWS + 3);
    while (e->ev.size() < want) {
        hipEvent_t ev = nullptr;
        HIP_TRY(e, hipEventCreate(&ev));
        e->ev.push_back(ev);
    }
    e->ev_tag.resize(e->ev.size() / 2, 0);
    e->ev_from.resize(e->ev.size() / 2, 0);
    e->ev_to.resize(e->ev.size() / 2, 0);
    return ITD_OK;
}

int itd_set_kernel_timing_stride(itd_engine *e, int stride)
{
    if (!e || stride < 1) return ITD_ERR_INVALID_ARG;
    e->timing_stride = stride;
    return ITD_OK;
}

int itd_set_kernel_timing_mode(itd_engine *e, int32_t mode)
{
    if (!e || mode < 0 || mode > 1) return ITD_ERR_INVALID_ARG;
    e->timing_mode = mode;
    return ITD_OK;
}

int itd_get_kernel_timing_samples(itd_engine *e, int32_t which, double *ms_out, int32_t cap, int32_t *count)
{
    if (!e || which < 0 || which > ITD_TIME_KF_KNOTS || cap < 0 || (cap > 0 && !ms_out)) return ITD_ERR_INVALID_ARG;
    if (!e->ran || !e->timing) return ITD_ERR_NOT_RUN;
    DevGuard g(e->device);
    HIP_TRY(e, hipStreamSynchronize(e->last.stream));
    int cnt = 0;
    for (int k = 0; k < e->n_timed; ++k) {
        if (e->ev_tag[(size_t)k] != which) continue;
        if (cnt < cap) {
            float ms = 0.f;
            HIP_TRY(e, hipEventElapsedTime(&ms, e->ev[(size_t)e->ev_from[(size_t)k]], e->ev[(size_t)e->ev_to[(size_t)k]]));
            ms_out[cnt] = ms;
        }
        ++cnt;
    }
    if (count) *count = cnt;
    return ITD_OK;
}

int itd_get_step_periods(itd_engine *e, double *ms_out, int32_t cap, int32_t *count)
{
    if (!e || cap < 0 || (cap > 0 && !ms_out)) return ITD_ERR_INVALID_ARG;
    if (!e->ran || !e->timing) return ITD_ERR_NOT_RUN;
    DevGuard g(e->device);
    HIP_TRY(e, hipStreamSynchronize(e->last.stream));
    int cnt = 0, prev = -1;
    for (int k = 0; k < e->n_timed; ++k) {
        if (e->ev_tag[(size_t)k] != ITD_TIME_EXTRACT_L0) continue;
        if (prev >= 0) {
            if (cnt < cap) {
                float ms = 0.f;
                HIP_TRY(e, hipEventElapsedTime(&ms, e->ev[(size_t)e->ev_from[(size_t)prev]], e->ev[(size_t)e->ev_from[(size_t)k]]));
                ms_out[cnt] = ms;
            }
            ++cnt;
        }
        prev = k;
    }
    if (count) *count = cnt;
    return ITD_OK;
}

int itd_get_kernel_timing(itd_engine *e, int32_t which, double *ms_total, int32_t *launches)
{
    if (!e || which < 0 || which > ITD_TIME_KF_KNOTS) return ITD_ERR_INVALID_ARG;
    if (!e->ran || !e->timing) return ITD_ERR_NOT_RUN;
    DevGuard g(e->device);
    HIP_TRY(e, hipStreamSynchronize(e->last.stream));
    double tot = 0.0;
    int cnt = 0;
    for (int k = 0; k < e->n_timed; ++k) {
        if (e->ev_tag[(size_t)k] != which) continue;
        float ms = 0.f;
        HIP_TRY(e, hipEventElapsedTime(&ms, e->ev[(size_t)e->ev_from[(size_t)k]], e->ev[(size_t)e->ev_to[(size_t)k]]));
        tot += ms;
        ++cnt;
    }
    if (ms_total) *ms_total = tot;
    if (launches) *launches = cnt;
    return ITD_OK;
}

}  // extern "C"

#include "itd_engine_batch.inc"
#include "itd_ring_streams.inc"
#include "itd_table_stream.inc"
#include "itd_wave_bounds.inc"
#include "itd_fourier.inc"
