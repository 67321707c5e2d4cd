/*
 * pyitd_hip.h — C ABI of the MI355X (gfx950) ITD engine, libpyitd_hip.so.
 *
 * This is the drop-in boundary for ONE path of falseywinchnet/PyITD:
 *     itd(x, max_iteration) -> rotations[rows, N] (+ baselines)
 * i.e. the reference's   ITD.itd            ITD.py:351-432  (runnable form: PyITD.ipynb cell 1;
 *                                           free-function form ITD_numba.py:100-136)
 *                        itd_baseline_extract  ITD.py:79-121
 *                        detect_peaks          ITD.py:33-76  (twin matlab_detect_peaks,
 *                                              numba_accelerated_itd.py:17-59)
 *                        baseline_knot_estimation  numba_accelerated_itd.py:167-178 (= ITD.py:100-110)
 * The reference is pure Python/numba with no FFI of its own; each entry point below names the
 * reference function a binding would replace.  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - plain C types only; every function returns an itd_status (0 = ok) and never throws.
 *   - "_dev" pointers are device (HBM) pointers on the engine's GPU; "_host" pointers are host memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the engine's own stream).
 *   - all floating-point results are IEEE binary64 computed in the reference's association order
 *     (no FMA contraction), so they are bit-identical to the reference for finite data.
 *   - int32 knot indices on the device (N < 2^31); the host-facing entry points widen to int64
 *     like the reference's numpy.int64 arrays.
 */
#ifndef PYITD_HIP_H
#define PYITD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITD_ABI_VERSION 12

/* rotations/baselines hold at most 22 rows in the reference (ITD.py:384-385): max_iteration <= 20 */
#define ITD_MAX_ROWS 22
#define ITD_MAX_ITERATION 20

typedef enum itd_status {
    ITD_OK = 0,
    ITD_ERR_INVALID_ARG = 1,   /* NULL pointer, N < 3, batch < 1, max_iteration outside [0, 20], sizes beyond the engine's */
    ITD_ERR_NO_DEVICE = 2,     /* no HIP device / wrong device id */
    ITD_ERR_HIP = 3,           /* a HIP runtime call failed: see itd_last_error() */
    ITD_ERR_NOMEM = 4,         /* device or host allocation failed */
    ITD_ERR_NOT_RUN = 5,       /* results requested before a decomposition was enqueued */
    ITD_ERR_NONFINITE = 6      /* the input signal contains a NaN and the operator / the engine's mode rejects such input */
} itd_status;

/* stop reasons of the level loop */
#define ITD_STOP_NATURAL 0 /* "No more decompositions possible", ITD.py:404-416 */
#define ITD_STOP_TIMEOUT 1 /* "Out of time!",                    ITD.py:418-426 */

/* knot-detection modes for itd_detect_* */
#define ITD_DETECT_KNOTS 0  /* union used by the extraction, ITD.py:87-98 */
#define ITD_DETECT_VALLEYS 1 /* detect_peaks(x), ITD.py:33-76 (dx[i]>0 & dx[i-1]<=0) */
#define ITD_DETECT_PEAKS 2   /* detect_peaks(-x) = matlab_detect_peaks(x), numba_accelerated_itd.py:17-59 */
#define ITD_DETECT_CPP 3     /* itd.cpp:161-168: (x[i-1] < x[i] && x[i] >= x[i+1]) || (x[i-1] > x[i] && x[i] <= x[i+1]) */
#define ITD_DETECT_ZERO_CROSS 4 /* find_extrema's test, itd_fourier_decomposition.py:23-27: sign change x[i] -> x[i+1] */

typedef struct itd_engine itd_engine; /* opaque; not thread-safe: one engine per host thread/stream */
/* (Debugging: with PYITD_POISON=1 in the environment every workspace the library allocates is filled with 0xFF bytes before its
 *  first use — reading memory nobody wrote gives NaNs / -1 on every run instead of whatever the allocation happened to hold.) */

int itd_abi_version(void);
const char *itd_status_string(int status);
/* detail of the last ITD_ERR_HIP on this engine (static storage inside the engine) */
const char *itd_last_error(const itd_engine *e);

/* Create an engine on HIP device `device_id` able to decompose up to `max_batch` signals of up to
 * `max_n` samples per call.  Allocates the device workspace once (three rotating float64 baseline slots per signal =
 * 24 B per sample, 0.3 B per sample of per-tile records and counts, and one signal's worth of knot lists for the
 * single-level helpers).  No allocation happens
 * in the decompose calls (they are graph-capturable).  `max_batch` is bounded by memory only: a batch runs in chunks of
 * at most 65535 signals (itd_set_batch_chunk); the batched FITPACK-flavour call takes at most 65535 signals per call. */
int itd_engine_create(itd_engine **out, int device_id, int64_t max_n, int32_t max_batch);
void itd_engine_destroy(itd_engine *e);
int64_t itd_engine_workspace_bytes(const itd_engine *e);
int itd_engine_device(const itd_engine *e);

/* Plain device-memory helpers for bindings that own no GPU allocator (the numpy path of pyitd_amd.itd_batch, the C
 * client of tests/c_client): hipMalloc / hipFree / synchronous hipMemcpy on `device_id`, ordered against all work on the
 * device (itd_dev_copy synchronises the device first: the engines' own streams are non-blocking).  to_device: 1 = host -> device,
 * 0 = device -> host.  Callers that already hold device buffers (torch tensors, their own hipMalloc) never need these. */
int itd_dev_alloc(int device_id, int64_t bytes, void **out);
int itd_dev_free(int device_id, void *p);
int itd_dev_copy(int device_id, void *dst, const void *src, int64_t bytes, int32_t to_device);

/* ---- sharding a batch over the GPUs of a node (one process and one engine per GPU) ----
 * Signals are independent: rank r of `world` owns the contiguous range [lo, hi) of the batch (the first batch % world ranks get one
 * signal more) and decomposes it with its own engine; there is NO data-path collective.  itd_shard_range is that arithmetic
 * (pyitd_amd.distributed.shard_range).  itd_shard_scatter hands every rank its range when the batch lives on ONE rank — the
 * "trivial batch scatter" of the north star — as one group of ncclSend / ncclRecv over xGMI: `nccl_comm` is the caller's ncclComm_t
 * (as void *; RCCL is resolved with dlopen at the first call, the library does not link it), x_root_dev the root's [batch][n]
 * array (ignored elsewhere), x_local_dev this rank's [hi - lo][n] array, elem_bytes 4 or 8; enqueued on `stream`, no host
 * synchronisation.  world = 1 is a local copy and needs no communicator.  ITD_ERR_NO_DEVICE: no RCCL library on this host. */
int itd_shard_range(int64_t batch, int32_t world, int32_t rank, int64_t *lo, int64_t *hi);
int itd_shard_scatter(const void *x_root_dev, void *x_local_dev, int64_t n, int64_t batch, int32_t elem_bytes, int32_t world,
                      int32_t rank, int32_t root, void *nccl_comm, void *stream);

/* ---- full decomposition, device resident: replaces ITD.itd (ITD.py:351-432) -------------------
 * x_dev          [batch] signals, signal b starts at x_dev + b*x_stride (elements), n samples each
 * rows_dev       [batch][max_iteration+2][n] float64.  On return (after the stream has run) rows
 *                0 .. n_rows-1 of each signal are the reference's returned array: proper rotations, then
 *                the residual (natural stop: the previous baseline; timeout: rotation + baseline).
 * baselines_dev  optional [batch][max_iteration+2][n] float64: row j = baseline after extraction j+1
 *                (the reference's `baselines` buffer, ITD.py:385,429); NULL = keep only a ping-pong pair
 *                inside the engine (saves 8 B/sample/level of HBM capacity, same traffic).
 * Everything is enqueued on `stream` with no host synchronisation; call itd_get_summary afterwards — the rows are final once it
 * has returned (or, for stream-ordered consumers, under itd_set_valid_flags / itd_set_device_repair below).
 * Calls of one engine must be ordered with respect to each other (the same stream, or synchronised by the caller): they share
 * the engine's workspace, and a call's last launch leaves part of it initialised for the next call.  A call that is captured
 * into a graph initialises what it needs itself, so the graph can be replayed any number of times. */
int itd_decompose_f32(itd_engine *e, const float *x_dev, int64_t n, int32_t batch, int64_t x_stride,
                      int32_t max_iteration, double *rows_dev, double *baselines_dev, void *stream);
int itd_decompose_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride,
                      int32_t max_iteration, double *rows_dev, double *baselines_dev, void *stream);

/* The same decomposition with its rows delivered in float32: rows_dev is [batch][max_iteration+2][n] float32, densely packed.
 * Every element is the element itd_decompose_f32 / _f64 delivers, converted to float32 (round to nearest even; values below the
 * float32 normal range become subnormals, values beyond it +-inf) — rotation rows, the natural-stop residual (a copied baseline),
 * the "Out of time!" residual (rotation + baseline formed in float64, then rounded) and the all-zero row of a stop at c = 0 alike.
 * The arithmetic is the float64 entries' own: each value is rounded once, where it is stored, and nothing reads a row back (the
 * baselines travel in the engine's float64 ping-pong pair, exactly as with baselines_dev == NULL — these entries offer no
 * baselines).  Row traffic and the result buffer halve.  In every other respect the contract is that of itd_decompose_f32 / _f64:
 * no host synchronisation, itd_get_summary finalises the call (any repeat writes float32 into the same buffer) and reports the same
 * summary as the float64 call, itd_set_valid_flags / itd_set_device_repair, the NaN-input modes and the timing records apply.
 * Calls of either row type may follow each other on one engine in any order. */
int itd_decompose_rows32_f32(itd_engine *e, const float *x_dev, int64_t n, int32_t batch, int64_t x_stride,
                             int32_t max_iteration, float *rows_dev, void *stream);
int itd_decompose_rows32_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride,
                             int32_t max_iteration, float *rows_dev, void *stream);

/* The same decomposition with only the rows the caller names.  rotation_mask: bit r selects rotation row r, 0 <= r <= max_iteration
 * (a bit above max_iteration is ITD_ERR_INVALID_ARG); want_residual: 0 or 1; S = popcount(rotation_mask) + want_residual >= 1.
 * rows_dev is [batch][S][n], densely packed (signal stride S * n), float64 or — rows_f32 = 1 — float32 rounded once at the store as
 * by itd_decompose_rows32_*: the selected rotations in ascending order, the residual's slot last.  With `rows` what
 * itd_decompose_f32 / _f64 delivers for the same input and n_rows as itd_get_summary reports it: the slot of rotation r holds rows[r]
 * if r <= n_rows - 2, otherwise its content is unspecified (as rows past n_rows are); the residual's slot holds rows[n_rows - 1]
 * wherever the stop falls — the copied baseline of a natural stop, the all-zero row of a stop at c = 0, the "Out of time!" row.  A row
 * that is not selected is stored nowhere: the call moves, and the buffer holds, S rows instead of max_iteration + 2.  The arithmetic,
 * the knots and the summary (n_rows, stop_reason, knot_counts, nan_levels: those of the full call) are unchanged, and so is the rest
 * of the contract: no host synchronisation, itd_get_summary finalises the call (every repeat honours the selection and writes into
 * the same buffer), itd_set_valid_flags / itd_set_device_repair and the NaN-input modes apply, calls of any kind may follow each
 * other on one engine.  No baselines. */
int itd_decompose_select_f32(itd_engine *e, const float *x_dev, int64_t n, int32_t batch, int64_t x_stride, int32_t max_iteration,
                             uint32_t rotation_mask, int32_t want_residual, void *rows_dev, int32_t rows_f32, void *stream);
int itd_decompose_select_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride, int32_t max_iteration,
                             uint32_t rotation_mask, int32_t want_residual, void *rows_dev, int32_t rows_f32, void *stream);

/* Stream-ordered consumers (a kernel of the caller's enqueued behind the decomposition, a replayed hipGraph).
 * The engine runs optimistic forms first — the fused sparse levels, the fused level 0, the resident form of short signals — each
 * of which either delivers the reference's result or REPORTS that it cannot (tied / quantised / very smooth input, non-finite
 * values); by default itd_get_summary then repeats the call level by level, so rows_dev is final only once the summary has been
 * read.  Two settings make the result usable without that host round trip:
 *   itd_set_valid_flags(e, valid_dev)   valid_dev[batch] int32, device memory owned by the caller (NULL = off).  Behind the last
 *       launch of every later decomposition the engine writes valid_dev[b] = 1 if signal b's rows (and baselines) are final,
 *       0 if they are not (they will be once itd_get_summary has run).  One short launch.
 *   itd_set_device_repair(e, 1)          the engine also enqueues the level-by-level repeat itself, guarded on the device: its
 *       launches return at once for every signal whose first result stands and re-run the others, so that rows_dev is final —
 *       and valid_dev[b] = 1 — when the stream has drained, with no host synchronisation (graph-capturable).  A call whose
 *       optimistic forms all delivered pays the guarded launches' boundaries (a dozen empty launches, ~25 us).  The one case left
 *       to the host is a NaN in the caller's signal under ITD_NAN_INPUT_FOLLOW (valid_dev[b] = 0; itd_get_summary repeats such a
 *       call the way the reference runs it).  itd_get_summary stays valid after either setting and repeats nothing twice.
 * Reference behaviour: ITD.itd returns final arrays, ITD.py:404-432. */
int itd_set_valid_flags(itd_engine *e, int32_t *valid_dev);
int itd_set_device_repair(itd_engine *e, int32_t on);
int64_t itd_get_device_repairs(const itd_engine *e);   /* signals the device-side repair has re-run (counted when a summary is read) */

/* Synchronise with the last decomposition and fetch its per-signal summary (any pointer may be NULL):
 *   n_rows       [batch]      rows valid in rows_dev (= shape[0] of the reference's result)
 *   n_baselines  [batch]      rows valid in get_baselines() (ITD.py:414 / :424)
 *   stop_reason  [batch]      ITD_STOP_NATURAL / ITD_STOP_TIMEOUT
 *   knot_counts  [batch][ITD_MAX_ROWS+1]  knot_counts[j] = interior knots of the input of extraction j+1
 *                (j = 0: the signal itself; j >= 1: the number the reference prints at ITD.py:403);
 *                entries past the last evaluated level are -1
 *   nan_levels   [batch]      -1 = results follow the reference; -2 = the input signal itself contains a NaN and the engine
 *                was told to reject such input (itd_set_nan_input_mode: rows undefined)
 * NaNs that arise inside a decomposition are followed exactly: a baseline acquires NaNs when the signal starts with a
 * plateau (ITD.py:115-116 divides by x[e_1]-x[0] = 0); the reference's stop test then counts knots under detect_peaks'
 * NaN rules (ITD.py:46-51,64-68) and overwrites NaN with +inf in place (ITD.py:50).  Since ABI revision 2 the extraction
 * kernel applies these rules itself, tile by tile, in the same launch (no re-run, no extra pass over the signal). */
int itd_get_summary(itd_engine *e, int32_t *n_rows, int32_t *n_baselines, int32_t *stop_reason,
                    int64_t *knot_counts, int32_t *nan_levels);
/* NaN in the INPUT.  The reference runs it through detect_peaks' NaN branch at level 0 — NaN differences count as +inf, NaN
 * samples and their neighbours cannot be peaks — and overwrites the NaNs of the caller's array with +inf (ITD.py:46-51, 64-68;
 * there is no copy at ITD.py:41, 82, 389); everything after that sees the mutated array.
 *   ITD_NAN_INPUT_FOLLOW (default)  the decomposition found a NaN in a signal: itd_get_summary repeats the call with a level 0
 *                                   that follows those rules on a mutated float64 copy of the signal (inside the engine: x_dev is
 *                                   never written); rows / baselines / knot counts are the reference's, bit for bit.  As with the
 *                                   other repeats x_dev / rows_dev / baselines_dev must stay valid until itd_get_summary.
 *   ITD_NAN_INPUT_REJECT            ABI revision 2's behaviour: nan_levels = -2, host forms return ITD_ERR_NONFINITE.
 * The reference's own single-level functions follow the same mode: itd_detect_* in the modes KNOTS / VALLEYS (detect_peaks) /
 * PEAKS (matlab_detect_peaks: the NaN branch on the negated differences, numba_accelerated_itd.py:28-49) and
 * itd_baseline_extract_* repeat their scan under the NaN rules when they find a NaN (the device forms only when they
 * synchronise anyway, i.e. when m_host / count_host is given).  The cubic / spline / instantaneous operators, whose reference
 * code has no NaN branch, reject NaN input (ITD_ERR_NONFINITE). */
#define ITD_NAN_INPUT_FOLLOW 0
#define ITD_NAN_INPUT_REJECT 1
int itd_set_nan_input_mode(itd_engine *e, int32_t mode);
/* Level 0 of a decomposition (the caller's signal) finds its knots in one of two ways:
 *   fused    the level-0 extraction launch evaluates the knot predicate itself and takes each tile's neighbouring knots from
 *            the 128 samples either side of the tile (walking on through up to ~4000 samples where those hold too few): the
 *            signal is read once, there is no separate scan pass;
 *   records  a scan pass (k_scan0) leaves per-tile knot records, the extraction launch reads them (any knot spacing).
 * ITD_LEVEL0_AUTO (default): fused; if a tile's knots lie beyond the fused launch's reach (input smoother than ~4000
 * samples between extrema), itd_get_summary repeats the call record-driven before it returns — so, as before, x_dev /
 * rows_dev / baselines_dev must stay valid until itd_get_summary — and the engine's next 16 decompositions start
 * record-driven.  Results are identical in every mode. */
#define ITD_LEVEL0_AUTO 0
#define ITD_LEVEL0_RECORDS 1
#define ITD_LEVEL0_FUSED 2   /* never repeat: itd_get_summary fails with ITD_ERR_HIP if the reach was exceeded (benchmarks) */
int itd_set_level0_mode(itd_engine *e, int32_t mode);
/* The sparse levels fused ("knot first", pyitd_amd/csrc/itd_knotfirst.hpp; ABI revision 6, one knot-side launch since revision 7).
 * An extraction maps every sample through an affine function of itself inside its segment (ITD.py:114-117), so the next level's
 * knots sit at this level's knots (apart from places where near ties let rounding make or break a plateau: both samples of every
 * near tie of the first fused level's input stay candidates): from level `first_fused_level` on the level recursion runs on the
 * knot list alone — ONE launch, the lists resident in LDS — and the samples take ONE pass for all remaining levels: 8 B read + 8 B
 * per row written per sample instead of 24 B per sample and level.  The sample pass re-derives every level's knots from the values
 * it computes; where they differ from the knot side's (or a list outgrows its workgroup, or knot data go non-finite: coarsely
 * quantised, plateau-ridden or very smooth signals) itd_get_summary repeats the call level by level before it returns (x_dev /
 * rows_dev / baselines_dev must stay valid until then, as before; or on the device: itd_set_device_repair) and the engine's next 16
 * decompositions start level by level (32, 64, ... 1024 when the fused attempt that follows such a pause refuses again: a workload
 * the fused form cannot deliver pays one wasted attempt in ever more calls; a delivered call starts over at 16) — after a list
 * outgrew its workgroup they stay fused, handing over a level later or with half the tiles per workgroup (itd_set_fuse_range); when
 * only a few signals of a batch are concerned (at most one in eight) just those are run again, each on its own, and the engine stays
 * in the fused form.
 * Results are bit-identical in every mode: what the fused form cannot deliver it reports.  The fused levels' workspace is allocated
 * by the first call that takes this path; a call being captured into a graph cannot allocate: on an engine that has not fused yet it is
 * captured level by level (run one decomposition before the capture to get the fused form into the graph).  A graph that holds a fused
 * call stays replayable whatever the engine does afterwards: when later calls need a larger workspace (smaller ranges after a capacity
 * refusal, itd_set_fuse_range, itd_set_fuse_level) the one the graph refers to is kept until itd_engine_destroy, never freed.
 * ITD_FUSE_AUTO (default): calls whose launch sequences cover at least itd_set_fuse_min_samples samples (signals per chunk x n; default
 * 2 * 2^20: one signal of 2^20 / 2^21 / 2^22 / 2^23 samples takes 89 / 115 / 183 / 305 us level by level and 90 / 104 / 149 / 227 us
 * fused), signals of >= 65536 samples; ITD_FUSE_OFF: never; ITD_FUSE_ONLY: always, never repeat (itd_get_summary fails with
 * ITD_ERR_HIP instead: tests, benchmarks).  itd_set_fuse_level: the first fused level, 2 .. max_iteration, or 0 (default) = automatic:
 * level 2 where a launch sequence covers at least 2^22 samples (levels 0 and 1 as one launch each; 377 against 404 us at 2^24), else
 * level 3; a level-2 candidate list that outgrows its workgroup moves the engine's later calls to level 3 before the ranges are halved. */
#define ITD_FUSE_AUTO 0
#define ITD_FUSE_OFF 1
#define ITD_FUSE_ONLY 2
int itd_set_fuse_mode(itd_engine *e, int32_t mode);
int itd_set_fuse_level(itd_engine *e, int32_t first_fused_level);
/* Tiles (of 512 samples) a knot-side workgroup of the fused levels owns: 64, 32 or 16; 0 (default) = automatic: 64, halved for the
 * calls after one in which a workgroup's candidate list (1720 entries at the first fused level, 1024 from the next on: knots and
 * near-tie samples) outgrew its LDS — dense knots at the first fused level (white noise from level 2, alternating data).  Smaller
 * ranges hold denser lists and cost more workgroups. */
int itd_set_fuse_range(itd_engine *e, int32_t tiles);
int itd_set_fuse_min_samples(itd_engine *e, int64_t samples);
/* ABI revision 11: capped fused levels.  A workload whose fused form is refused at the same level every time — exactly periodic input
 * whose baseline collapses to a handful of knots at some level (BASELINE configs[4]'s substitute clip: 1049 knots, then 3, at level 8):
 * every sample a near tie there — keeps the fused form for the levels in front of that one: levels first_fused .. cap - 1 run fused
 * (the sample pass also stores the baseline behind level cap - 1), levels cap .. max_iteration + 1 one launch each from a scan of that
 * baseline.  first_level_not_fused = 0 (default): automatic — a whole-call refusal records the lowest level at which anything failed
 * (verification, non-finite knot data) and the engine's next calls are capped there instead of running level by level (after 16
 * delivered capped calls one call tries all levels again; a probe refused at the learned level doubles that span, up to 1024; a
 * delivered probe drops the cap); -1: never; 4 .. max_iteration + 1: always this cap (tests).  A cap leaves at least two fused levels or
 * is ignored.  Results are bit-identical either way. */
int itd_set_fuse_cap(itd_engine *e, int32_t first_level_not_fused);
/* the cap of the last decomposition as it was enqueued (0: none — every level from the first fused one on ran fused, or no fused levels) */
int itd_get_last_fuse_cap(const itd_engine *e);
/* Tests only (ABI revision 9): arm ONE fault in what the fused levels' knot side hands to their sample pass, applied to signal 0 of
 * every following fused call of this engine until disarmed (kind < 0).  The sample pass verifies everything it takes from the knot
 * side (itd_knotfirst.hpp: V0 .. V3); a fault in a field it uses must end in a refusal (ITD_FUSE_ONLY: itd_get_summary fails;
 * otherwise the call is repeated level by level, itd_get_fuse_repeats counts it) — tests/test_gpu_fused.py holds that for thousands.
 *   kind 0 / 1 / 2  delta ulps added to X / B / S of table entry `slot` (mod the run's length) of tile `where`'s run at `level`;
 *   kind 3          delta added to that entry's knot position;     kind 4   delta added to the run's start index first[level][where];
 *   kind 5          bit (delta & 63) of flag word (slot & 7) of tile `where` at `level` flipped;
 *   kind 6 / 7      the value (delta ulps) / position (delta) of halo knot `slot` (0, 1: the two in front, 2 .. 4: the three behind) as
 *                   knot-side workgroup `where` receives it from its neighbours at `level`;
 *   kind 8          delta added to the knot side's count of `level`'s knots (what its stop rules read): the sample pass's check
 *                   wavefronts count the verified flag words themselves, the verdict compares.
 * `level` is the absolute level (first fused level .. max_iteration + 1). */
int itd_debug_kf_fault(itd_engine *e, int32_t kind, int32_t level, int32_t where, int32_t slot, int32_t delta);
/* Tests only (ABI revision 11): the armed fault lands in signal `signal` of the batch instead of signal 0 (kinds 6 / 7: in that signal's
 * knot-side workgroup `where`) — the fused levels of a batch run many signals per launch, and what is verified for signal 0 has to hold
 * for every other one. */
int itd_debug_kf_fault_signal(itd_engine *e, int32_t signal);
/* Tests only (ABI revision 9): the kernels form the knot spacings' ratio (k1 - k0) / (k2 - k0) of ITD.py:107 with the division's own
 * instruction sequence minus its range scaling and special-case fix-up, which do nothing for exact small integers (itd_kernels.hpp:
 * int_ratio).  This runs that sequence against the compiler's full float64 division on the device for EVERY pair 0 <= a <= b <= max_den
 * and for 2^30 pseudo-random pairs below 2^31: *mismatches = pairs whose results differ in any bit (must be 0). */
int itd_debug_int_ratio_check(int device, int32_t max_den, int64_t *mismatches);
/* how many whole calls of this engine itd_get_summary has had to repeat level by level because the fused levels reported a failure */
int itd_get_fuse_repeats(const itd_engine *e);
/* the first fused level of the last decomposition as it was enqueued (2, 3, ...), 0 if it ran one launch per level throughout
 * (too short, ITD_FUSE_OFF, a back-off) or in the resident form: what a benchmark's byte model needs (ABI revision 9) */
int itd_get_last_fuse_level(const itd_engine *e);
/* ... and how many single signals of batches it has re-run on their own (the rest of their batch kept the fused result) */
int64_t itd_get_fuse_signal_repairs(const itd_engine *e);
/* Short signals (n <= 8192 samples): the resident form — ONE launch, one workgroup per signal, the signal and its knot arrays
 * in LDS through all levels of the driver loop (ITD.py:384-432): the signal is read once and every result row written once
 * (4 + 8 rows bytes per sample; the level-by-level form is launch bound there: 10 dependent launches).  Baselines that go NaN
 * (a leading or trailing plateau, ITD.py:115-116) and NaNs in the caller's signal follow the reference's NaN rules inside the kernel;
 * only under ITD_NAN_INPUT_REJECT does a NaN input make itd_get_summary repeat the call level by level before it returns (x_dev /
 * rows_dev / baselines_dev must stay valid until then, as before; the engine's next 16 decompositions then start level by level).
 * Rows past n_rows are not written in this form.
 * ITD_RESIDENT_AUTO (default): resident for n <= 8192 unless the engine was given a level-0 mode or kernel timing;
 * ITD_RESIDENT_OFF: never; ITD_RESIDENT_ONLY: always for n <= 8192, never repeat (itd_get_summary fails with ITD_ERR_HIP
 * instead; tests, benchmarks).  Results are identical in every mode. */
#define ITD_RESIDENT_AUTO 0
#define ITD_RESIDENT_OFF 1
#define ITD_RESIDENT_ONLY 2
int itd_set_resident_mode(itd_engine *e, int32_t mode);
/* how many resident calls of this engine itd_get_summary has had to repeat level by level so far */
int itd_get_resident_repeats(const itd_engine *e);
/* The resident form holds a window of `segments` consecutive knot-to-knot segments of a level in LDS at a time; a level with more
 * knots takes several passes.  0 = automatic (0.4 knots per sample: one pass for ordinary signals), otherwise >= 8 (cut to what
 * fits the LDS).  Results do not depend on it (tests run tiny windows to exercise the passes). */
int itd_set_resident_window(itd_engine *e, int32_t segments);
/* Batched decompositions run as launch sequences over chunks of `signals_per_chunk` signals, all levels of a chunk before
 * the next chunk (0 = automatic: about 2^24 samples in flight — per chunk over one stream, 3/4 of that per chunk over two —, so a
 * level's baseline is still in the 256 MiB Infinity Cache when the next level reads it).  Results do not depend on the chunk size. */
int itd_set_batch_chunk(itd_engine *e, int32_t signals_per_chunk);
/* The chunks of a batch are independent: they rotate over `streams` streams (the caller's and streams - 1 of the engine's, forked
 * from / joined to the caller's stream by events), each chunk's launches in order on its stream — its own knot side of the fused levels
 * included —, so that one chunk's launch boundaries and tails overlap another's work.
 * 1 .. 4; default 2 (with automatic chunks of about 1.2e7 samples: 32.5 ms against 35.9 ms over one stream for 1024 x 2^20). */
int itd_set_batch_streams(itd_engine *e, int32_t streams);

/* Per-level knot lists are not retained by a decomposition (each level's list is consumed by the next
 * launch); to inspect them run itd_detect_* on the input or on a stored baseline row.  The single-level operators
 * below work in a workspace of their own: calling them between itd_decompose_* and itd_get_summary (on any stream)
 * does not disturb the decomposition.  A signal that contains a NaN: see itd_set_nan_input_mode. */

/* ---- one-call host convenience (numpy in -> numpy out, what the reference's callers see) -------
 * Copies x to the GPU, decomposes, copies rows (and baselines if non-NULL) back.
 * rows_host / baselines_host: [max_iteration+2][n] float64, caller allocated. */
int itd_decompose_host_f64(itd_engine *e, const double *x_host, int64_t n, int32_t max_iteration,
                           double *rows_host, double *baselines_host, int32_t *n_rows, int32_t *n_baselines,
                           int32_t *stop_reason, int64_t *knot_counts /* [ITD_MAX_ROWS+1] */);
int itd_decompose_host_f32(itd_engine *e, const float *x_host, int64_t n, int32_t max_iteration,
                           double *rows_host, double *baselines_host, int32_t *n_rows, int32_t *n_baselines,
                           int32_t *stop_reason, int64_t *knot_counts);
/* ... with float32 rows (itd_decompose_rows32_*): rows_host is [max_iteration+2][n] float32, the copy back is half as long.  No
 * baselines: itd_set_host_keep_baselines is ignored by these calls (itd_get_last_baselines_host returns ITD_ERR_NOT_RUN after one). */
int itd_decompose_rows32_host_f32(itd_engine *e, const float *x_host, int64_t n, int32_t max_iteration, float *rows_host,
                                  int32_t *n_rows, int32_t *stop_reason, int64_t *knot_counts);
int itd_decompose_rows32_host_f64(itd_engine *e, const double *x_host, int64_t n, int32_t max_iteration, float *rows_host,
                                  int32_t *n_rows, int32_t *stop_reason, int64_t *knot_counts);
/* ... with selected rows (itd_decompose_select_*): rows_host is [S][n] float64 or (rows_f32 = 1) float32; all S slots are copied
 * back, n_rows is the full call's.  No baselines, as with the rows32 forms. */
int itd_decompose_select_host_f32(itd_engine *e, const float *x_host, int64_t n, int32_t max_iteration, uint32_t rotation_mask,
                                  int32_t want_residual, void *rows_host, int32_t rows_f32, int32_t *n_rows, int32_t *stop_reason,
                                  int64_t *knot_counts);
int itd_decompose_select_host_f64(itd_engine *e, const double *x_host, int64_t n, int32_t max_iteration, uint32_t rotation_mask,
                                  int32_t want_residual, void *rows_host, int32_t rows_f32, int32_t *n_rows, int32_t *stop_reason,
                                  int64_t *knot_counts);

/* The reference keeps the baselines of the last run on the instance (ITD.py:413-414,423-424) but most callers only look at
 * the returned rows: with itd_set_host_keep_baselines(e, 1) a host-form call with baselines_host == NULL still computes the
 * baselines buffer and leaves it on the device (half the PCIe traffic of the call); itd_get_last_baselines_host copies its
 * first n_baselines rows ([n_baselines][n] float64; n and n_baselines as the call reported them) out later — until the next
 * host-form call on this engine, after which it returns ITD_ERR_NOT_RUN. */
int itd_set_host_keep_baselines(itd_engine *e, int32_t enable);
int itd_get_last_baselines_host(itd_engine *e, double *baselines_host, int64_t n, int32_t n_baselines);

/* ---- single-level operators ---------------------------------------------------------------------
 * itd_baseline_extract (ITD.py:79-121): rotation/baseline of ONE extraction of a device signal.
 * knots_dev (optional, capacity n int32) receives the interior knot indices, *m_host their count. */
int itd_baseline_extract_f64(itd_engine *e, const double *x_dev, int64_t n, double *rot_dev, double *base_dev,
                             int32_t *knots_dev, int64_t *m_host, void *stream);
int itd_baseline_extract_f32(itd_engine *e, const float *x_dev, int64_t n, double *rot_dev, double *base_dev,
                             int32_t *knots_dev, int64_t *m_host, void *stream);
/* host convenience: rot/base [n] float64, knots_host (optional) [n] int64, bk_host (optional) [n+2] knot values */
int itd_baseline_extract_host_f64(itd_engine *e, const double *x_host, int64_t n, double *rot_host,
                                  double *base_host, int64_t *knots_host, int64_t *m_host, double *bk_host);

/* detect_peaks / matlab_detect_peaks / knot union (ITD.py:33-76, :87-98): ordered indices of a device
 * signal.  idx_dev capacity n int32; the count is returned through *count_host (synchronises). */
int itd_detect_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t mode, int32_t *idx_dev,
                   int64_t *count_host, void *stream);
int itd_detect_f32(itd_engine *e, const float *x_dev, int64_t n, int32_t mode, int32_t *idx_dev,
                   int64_t *count_host, void *stream);
int itd_detect_host_f64(itd_engine *e, const double *x_host, int64_t n, int32_t mode, int64_t *idx_host,
                        int64_t *count_host);

/* baseline_knot_estimation (numba_accelerated_itd.py:167-178 = ITD.py:106-110): fills bk[1..m] for the
 * caller's extended knot list e[0..m+1] (bk[0], bk[m+1] are left as given, like the reference).
 * All host pointers; x [n], extrema [m+2] int64, bk [m+2]. */
int itd_knot_values_host_f64(itd_engine *e, const double *x_host, int64_t n, const int64_t *extrema_host,
                             int64_t m, double *bk_host);
/* The same on device buffers, enqueued on `stream` (no synchronisation, no validation: the caller guarantees
 * 0 <= extrema_dev[k] < n): x_dev [n] float64, extrema_dev [m+2] int32 (what itd_detect_* delivers, with the end knots
 * 0 and n-1 around it), bk_dev [m+2] float64 of which bk_dev[1..m] are written. */
int itd_knot_values_f64(itd_engine *e, const double *x_dev, int64_t n, const int32_t *extrema_dev, int64_t m,
                        double *bk_dev, void *stream);

/* ---- cubic-spline baseline variant with externally supplied knots ---------------------------
 * itd_baseline_extract_fast(I, extrema_input, idx), itd_fourier_decomposition.py:49-122 — the Python twin of
 * itd_baseline_extract(data, baseline, length, &idx, compute_extrema), itd.cpp:156-239.  Restated literally in float64,
 * quirks included (knot values for k = 1..idx-2 only, K[idx-1] = 0, K[idx] = I[e[idx]], the sweep as written, natural ends,
 * the segment idx-2 evaluated linearly).  Float results agree with the reference to rounding (the reference's numpy form
 * uses libm pow for t**3, numba multiplies, the knot recurrences run here as scans): tests hold them to 1e-9 of the
 * signal's scale; knot indices are exact.
 *   extrema_dev   idx+1 knots (int32, device): e[0..idx-1] strictly increasing sample indices, e[idx] any sample index
 *                 (find_extrema leaves 0 there); 2 <= idx <= n-1.  Invalid lists return ITD_ERR_INVALID_ARG.
 *                 NULL = compute_extrema (itd.cpp:159-169): the knots are the samples with
 *                 (x[i-1] < x[i] && x[i] >= x[i+1]) || (x[i-1] > x[i] && x[i] <= x[i+1]), e[idx] = 0 (the file's static
 *                 array at first call); *idx_host receives their count; fewer than 2 leave baseline_dev untouched (:170).
 *   the float32 form widens the signal first: itd.cpp's all-float32 arithmetic has no compilable reference to pin. */
int itd_baseline_extract_cubic_f64(itd_engine *e, const double *x_dev, int64_t n, const int32_t *extrema_dev, int64_t idx,
                                   double *baseline_dev, int64_t *idx_host, void *stream);
int itd_baseline_extract_cubic_f32(itd_engine *e, const float *x_dev, int64_t n, const int32_t *extrema_dev, int64_t idx,
                                   double *baseline_dev, int64_t *idx_host, void *stream);
/* host form: extrema_host int64 [idx+1] or NULL (detect); extrema_out_host (optional, capacity n) receives detected knots */
int itd_baseline_extract_cubic_host_f64(itd_engine *e, const double *x_host, int64_t n, const int64_t *extrema_host,
                                        int64_t idx, double *baseline_host, int64_t *idx_out, int64_t *extrema_out_host);
/* ABI revision 11: the common-baseline form of the same operator on COMPLEX (I/Q) data, itd_baseline_extract_iq, itd.cpp:58-154 (a
 * non-compilable float32 fragment like the 1-D form below it: restated in float64 the way its Python twin restates the 1-D form; no
 * upstream test or Python twin pins the I/Q form: "recipe unpinned").  iq: n complex samples, interleaved (re, im), 16-byte aligned.
 *   knots      the samples at which BOTH components have an extremum under the file's 3-point predicate (itd.cpp:74-80), or the
 *              caller's list (extrema_dev / extrema_host with idx as in itd_baseline_extract_cubic_f64: "retain the extrema and reuse
 *              them ... along multiple channels", itd.cpp:40-44)
 *   baseline   ONE real baseline [n]: the natural-cubic operator above on the components' mean (I + Q) / 2 (itd.cpp:96-108)
 * Fewer than 2 knots leave the baseline buffer untouched (itd.cpp:85-87); *idx_host / *idx_out = the knot count.  Synchronous (one host
 * synchronisation for the knot count when the knots are detected, one at the end for the operator's validity). */
int itd_baseline_extract_iq_f64(itd_engine *e, const double *iq_dev, int64_t n, const int32_t *extrema_dev, int64_t idx,
                                double *baseline_dev, int64_t *idx_host, void *stream);
int itd_baseline_extract_iq_host_f64(itd_engine *e, const double *iq_host, int64_t n, const int64_t *extrema_host, int64_t idx,
                                     double *baseline_host, int64_t *idx_out, int64_t *extrema_out_host);
/* find_extrema(signal), itd_fourier_decomposition.py:17-31: [0, the sign changes s[i] -> s[i+1], one extrapolated index],
 * zero padded to n entries like the reference's numpy.zeros array; *idx_out = the reference's returned idx. */
int itd_find_extrema_host_f64(itd_engine *e, const double *s_host, int64_t n, int64_t *extrema_host, int64_t *idx_out);

/* ---- the FITPACK flavour of the baseline and its 2-D consumers -----------------------------
 * itd_baseline_extract_modified(x), numba_accelerated_itd.py:182-211 (= itd_baseline_extract, siftED2D.ipynb cell 1; MEITD.py:
 * 303-338 is the same operator without the early-out): knots = the tier-1 set, baseline knot values with odd-reflected ends
 * (:196-206), the INTERPOLATING cubic B-spline through them — custom_splrep -> scipy.interpolate.splrep(x, y, k=3), whose
 * default without weights is s = 0; SciPy's FITPACK curfit, restated in pyitd_amd/csrc/itd_fitpack.hpp and held bit for bit to
 * scipy's splrep (tests/test_fitpack_host.py) — evaluated at every sample like numba_splev (:89-164, its equi_spaced interval
 * formula included).  Batched: signal b at x_dev + b*x_stride, n samples each; one GPU thread per signal computes the
 * coefficients (the sweep over the knots is serial), one thread per sample evaluates.
 *   min_extrema   signals with fewer knots are returned unchanged (baseline = x): 10 for numba_accelerated_itd.py:188-190 and
 *                 siftED2D, 0 for MEITD's form; fewer than 2 knots are always returned unchanged (splrep needs m > k)
 *   rot_dev       optional: x - baseline (MEITD.py:335)
 *   knots_host    optional [batch]: the knot count of every signal
 * Returns ITD_ERR_NONFINITE if a signal holds a NaN.  Synchronous. */
int itd_baseline_extract_spline_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride,
                                    int32_t min_extrema, double *baseline_dev, int64_t baseline_stride, double *rot_dev,
                                    int64_t rot_stride, int32_t *knots_host, void *stream);
int itd_baseline_extract_spline_host_f64(itd_engine *e, const double *x_host, int64_t n, int32_t batch, int32_t min_extrema,
                                         double *baseline_host, double *rot_host, int32_t *knots_host);
/* How the spline's coefficients are obtained (ABI revision 6):
 *   ITD_SPLINE_SERIAL    FITPACK's own row-by-row sweep, one GPU thread per signal, bit-level against scipy's splrep: right for
 *                        thousands of short rows (the image sweeps always use it)
 *   ITD_SPLINE_PARALLEL  the same interpolating not-a-knot spline from its second derivatives, parallel in the knots
 *                        (pyitd_amd/csrc/itd_nak.hpp): equal to FITPACK's result to rounding (~1e-14 of the signal's scale; the
 *                        north star allows 1e-6), not bit for bit; right for ONE long signal (MEITD.py:344-549 calls the operator on
 *                        single 1-D signals in a loop)
 *   ITD_SPLINE_AUTO      (default) parallel for calls of fewer than 256 signals of at least 1024 samples, serial otherwise */
#define ITD_SPLINE_AUTO 0
#define ITD_SPLINE_SERIAL 1
#define ITD_SPLINE_PARALLEL 2
int itd_set_spline_solver(itd_engine *e, int32_t solver);
/* the host form with one more optional output (ABI revision 6): baseline_knots_host [batch] = the knot count (ITD_DETECT_KNOTS) of
 * every PRODUCED baseline — MEITD's loops ask for it right after an extraction (MEITD.py:362-363, :497-505); it is counted on the
 * device from the result that is already there (no second upload, no index list) */
int itd_baseline_extract_spline_host2_f64(itd_engine *e, const double *x_host, int64_t n, int32_t batch, int32_t min_extrema,
                                          double *baseline_host, double *rot_host, int32_t *knots_host, int32_t *baseline_knots_host);
/* Knot counts of `batch` contiguous host signals under predicate `mode` (ITD_DETECT_*) without building or copying any index
 * list — `matlab_detect_peaks(x).size + matlab_detect_peaks(-x).size` (MEITD.py:350, :376, :409) is mode ITD_DETECT_KNOTS.
 * Plain rules; returns ITD_ERR_NONFINITE (counts filled in) if a signal holds a NaN.  batch <= 65535. */
int itd_count_knots_host_f64(itd_engine *e, const double *x_host, int64_t n, int32_t batch, int32_t mode, int32_t *counts_host);
/* ---- MEITD's operators on device-resident signals (ABI revision 8) --------------------------------
 * MEITD.py:344-534 keeps one signal, its rotation and its baseline in a loop of extractions, knot counts and entropy tests: with
 * these entries the arrays stay on the device for the whole loop and only scalars come back (pyitd_amd/meitd.py).
 *
 * itd_count_knots_f64: itd_count_knots_host_f64 for signals that are on the device already (signal b at x_dev + b*x_stride).
 *
 * itd_wpe3_f64: weighted_permutation_entropy(x, order=3), MEITD.py:79-128, as far as it touches the samples — for each of the six
 * permutation patterns of the windows (x[i], x[i+1], x[i+2]), in numpy.unique's order of the reference's hash values
 * (5, 7, 11, 15, 19, 21 = argsort (2,1,0), (1,2,0), (2,0,1), (0,2,1), (1,0,2), (0,1,2)): bin_weights_host[6] the sum of the
 * windows' variances, bin_windows_host[6] the number of windows (a pattern without windows is absent from the reference's list).
 * The argsort is numpy's (insertion on three values, NaNs last, ties in index order), the variance numpy.var's expression; up to
 * 65536 windows the sums are taken one by one in index order like the reference's cumsum, longer signals in segments of 4096
 * windows added in order (deterministic, equal to rounding).  The entropy itself is six logarithms on the host:
 * p = w / sum(w); -sum(p log2 p) [/ log2(6)].  knots_host (optional): x's knot count (ITD_DETECT_KNOTS, plain rules) from the same
 * launch — a window's middle sample is a knot or not; MEITD.py:346-351, :373-378 ask for both; then ITD_ERR_NONFINITE (count filled
 * in) if x holds a NaN.
 *
 * itd_wpe_f64: the same pass for any `order` 2 .. 5 (MEITD.py:79 takes the order; MEITD itself only passes 3): sums_host and
 * windows_host have order^order entries, indexed by the reference's hash value sum(argsort[k] * order^k); the entropy is drawn from
 * the entries with windows, in ascending hash order (numpy.unique's).  Sums in index order per hash up to 65536 windows, in
 * segments of 16384 beyond.  A side path: its work grows with order^order x windows.
 *
 * itd_baseline_extract_spline2_f64: itd_baseline_extract_spline_f64 plus baseline_knots_host [batch], the knot count of every
 * PRODUCED baseline, one synchronisation for both (the device form of itd_baseline_extract_spline_host2_f64).
 *
 * itd_subtract_f64: out = a - b, elementwise (MEITD.py:453), enqueued.   itd_copy: a copy ordered on the engine's stream (or
 * `stream`): kind 0 device -> host, 1 host -> device, 2 device -> device, 3 zero fill (src ignored); wait != 0 returns when done. */
int itd_count_knots_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride, int32_t mode,
                        int32_t *counts_host, void *stream);
int itd_wpe3_f64(itd_engine *e, const double *x_dev, int64_t n, double *bin_weights_host, int64_t *bin_windows_host,
                 int32_t *knots_host, void *stream);
int itd_wpe_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t order, double *sums_host, int64_t *windows_host, void *stream);
int itd_baseline_extract_spline2_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride,
                                     int32_t min_extrema, double *baseline_dev, int64_t baseline_stride, double *rot_dev,
                                     int64_t rot_stride, int32_t *knots_host, int32_t *baseline_knots_host, void *stream);
int itd_subtract_f64(itd_engine *e, const double *a_dev, const double *b_dev, double *out_dev, int64_t count, void *stream);
int itd_copy(itd_engine *e, void *dst, const void *src, int64_t bytes, int32_t kind, int32_t wait, void *stream);
/* MEITD's whole selection loop (MEITD.py:395-534 with retrieve_proper_rotation :344-368 and determine_if_first_is_proper_rotation
 * :371-392) on ONE device-resident signal of 3 .. 8192 samples as one launch of one workgroup (ABI revision 10): the extractions,
 * extrema counts and entropy tests above run behind one another on the device and the branch is taken there — no host round trip
 * per operator (the host-driven loop: ~107 of them for a 3000-sample signal).  Only where the engine's solver setting gives the
 * parallel-in-knots form for such a signal (ITD_SPLINE_PARALLEL, or ITD_SPLINE_AUTO and n >= 1024); otherwise ITD_ERR_INVALID_ARG.
 * rows_dev: (6 + 2 * 22) rows of n float64 in one allocation — rows 0..5 working rows (the signal in row 5 on entry), rows 6..27
 * the kept rotations taken off the signal ("high", MEITD.py:447), rows 28..49 those taken off its baselines ("low", :450).
 * wpemax: MEITD's WPEMAX.  result_host[24]: status, number of high rows, number of low rows, the working row that holds the
 * residual, entropy probes taken, extractions run, turns of the loop, 0, then sixteen diagnostic words — the launch's time in
 * units of 10 ns spent in the probes, the extractions, the extrema counts, the row copies / subtractions, the probes' ordered sums,
 * their entropies, two zeros, the extractions' phases (knots, knot values, rows, forward sweep, backward sweep, evaluation), two
 * zeros.  status 0: delivered; 1: the signal has fewer than four
 * extrema (MEITD.py:411-413 returns zeros and the data); 2 (a NaN in a row), 3 (an extraction met fewer than two knots: scipy
 * raises there), 4 (more than 1024 probes): NOT delivered — run the loop from the host, which reproduces the reference's behaviour
 * for those.  probe_log_host (log_cap entries of 88 bytes: double w[6]; int32 c[6]; int32 count; int32 0; double entropy): every
 * entropy probe's six weighted sums, window counts, extrema count and the normalised entropy the device drew from them with its
 * own log2 — the caller re-draws each with the reference's numpy expression and compares the threshold test
 * (wpe < WPEMAX and not wpe < 0.2, MEITD.py:364 / :387), the only use an entropy has: selections identical to the reference's by
 * construction, not by the two log2 agreeing.  Synchronous. */
int itd_meitd_small_f64(itd_engine *e, double *rows_dev, int64_t n, double wpemax, int32_t *result_host, void *probe_log_host,
                        int32_t log_cap, void *stream);
/* The same loop on a BATCH of signals of one length, one workgroup per signal, all of them in one launch (up to 65535 signals per
 * launch; more: one launch per 65535), under the same eligibility rule (3 <= n <= 8192 and the parallel-in-knots solver setting;
 * otherwise ITD_ERR_INVALID_ARG).  Signal b's rows are the 50 rows above at rows_dev + b * rows_stride (rows_stride >= 50 * n
 * elements).  x_host (optional): batch signals of n float64, copied into row 5 of their blocks first (one copy per launch); NULL: the
 * rows already hold them.  result_host [batch][24]: each signal's words as itd_meitd_small_f64's result_host.  probe_logs_host
 * [batch][log_cap] entries: each signal's log as itd_meitd_small_f64's, filled up to min(its probes, log_cap, 1024).
 * xitd_sums_host / xitd_windows_host [batch][22][6] (both or neither): for a signal with status 0, XITD's entropy sums (MEITD.py:536-549)
 * of its kept high rows, its kept low rows and its residual, in that order — row by row what itd_wpe3_f64 returns for that row; the
 * other signals' entries and the rows behind the residual are undefined.  The per-signal workspace is the engine's own, apart from a pending decomposition's.  Synchronous. */
int itd_meitd_batch_f64(itd_engine *e, double *rows_dev, int64_t n, int32_t batch, int64_t rows_stride, const double *x_host, double wpemax,
                        int32_t *result_host, void *probe_logs_host, int32_t log_cap, double *xitd_sums_host, int64_t *xitd_windows_host,
                        void *stream);
/* rows of n float64, row r at src_dev + offsets_host[r] (0 <= offset <= src_elems - n, checked), one after the other into dst_dev
 * [rows][n]: one upload of the table, one launch; dst_host (optional, [rows][n]): then one download of dst_dev — how the batch's
 * components leave the device.  Synchronous. */
int itd_gather_rows_f64(itd_engine *e, const double *src_dev, int64_t src_elems, const int64_t *offsets_host, int64_t rows, int64_t n,
                        double *dst_dev, double *dst_host, void *stream);
/* crossways_itd_baseline_extract(data), siftED2D.ipynb cell 1, for `planes` images of rows x cols float64 (the ensemble
 * members of retrieve_statistical_image_component go through in one call): the operator over every row, then over every
 * column of that; over every column, then every row of that; the mean of the two.  Transposes and the mean run on the GPU. */
int itd_crossways_f64(itd_engine *e, const double *img_dev, int32_t planes, int32_t rows, int32_t cols, int32_t min_extrema,
                      double *out_dev, void *stream);
int itd_crossways_host_f64(itd_engine *e, const double *img_host, int32_t planes, int32_t rows, int32_t cols, int32_t min_extrema,
                           double *out_host);

/* ---- instantaneous amplitude / phase / frequency of a proper rotation --------------------------
 * The time-frequency-energy step the reference describes (README.md:13-21, 41-55) but does not implement; definitions of the
 * paper it quotes (Frei & Osorio 2007, single-wave analysis): half waves between zero crossings, amplitude = the half wave's
 * largest |x|, phase by arcsin(x / amplitude) placed in the wave's quadrant, frequency = forward phase difference / 2 pi in
 * cycles per sample.  rot_dev: one row of the decomposition (or any oscillation about zero); any output may be NULL. */
int itd_instantaneous_f64(itd_engine *e, const double *rot_dev, int64_t n, double *amp_dev, double *phase_dev, double *freq_dev,
                          void *stream);
int itd_instantaneous_host_f64(itd_engine *e, const double *rot_host, int64_t n, double *amp_host, double *phase_host,
                               double *freq_host);

/* ---- batched single-level operators (ABI revision 6): asynchronous on `stream`, no host synchronisation, graph-capturable ---
 * The reference applies its single-level functions row by row (siftED2D.ipynb cell 1: itd_baseline_extract over the rows of an
 * image under numba.prange) and along channels (itd.cpp:40-44).  Signal b starts at x_dev + b * x_stride.  These calls work in
 * workspaces of their own (grown on demand: the first call of a size allocates — so capture a call only after one of its size has
 * run), apart from the decomposition's.  Growing frees the old block and allocates a larger one: a captured call keeps the
 * addresses of the block it was captured in, so its graph is valid only while no larger call of its kind (the extraction has one
 * workspace; the batched detection, knot counts and cubic batch share another) follows on the engine — after one, capture again.
 * A later smaller call works in the front of the grown block and is no such call.
 *
 * itd_baseline_extract_batch_f64: itd_baseline_extract (ITD.py:79-121) of every signal: rot_dev / base_dev [batch] rows of n.
 *   info_dev (optional) [batch]: the signal's interior knot count; -1 - count if the signal holds a NaN — its rows then follow
 *   the plain rules, not detect_peaks' NaN branch (ITD.py:46-51): run that signal through itd_baseline_extract_* .
 *   The plain rules of the extraction: the knots are the samples flagged by dx[i] > 0 & dx[i-1] <= 0 or dx[i] < 0 & dx[i-1] >= 0
 *   as IEEE comparisons (one with a NaN is false: a NaN sample and both its neighbours are never knots), nothing is overwritten
 *   with +inf, and the arithmetic of ITD.py:100-117 runs on those knots as written, NaNs propagating (oracle/numpy_itd.py:
 *   baseline_extract(plain_nan=True) is the statement the tests compare with).  Any batch >= 1: above 65535 signals in chunks.
 * itd_detect_batch_f64: the knots of every signal by predicate `mode` (ITD_DETECT_*): idx_dev (optional) [batch] lists at
 *   idx_stride >= n - 2 (the knots alone, ascending); info_dev (optional) as above.  idx_dev == NULL: counts only (no list is
 *   built).  batch <= 65535.  The plain rules of the detection: every mode's predicate as IEEE comparisons on the samples as they
 *   are — for ITD_DETECT_KNOTS, _VALLEYS and _PEAKS the flags above and their two halves, for the other two modes the loops of
 *   itd.cpp:161-168 and itd_fourier_decomposition.py:17-31, which have no NaN rule to leave out.  Of a signal's list slot the entries
 *   [0, count) are written with its knots; what the entries [count, n - 2) hold afterwards is unspecified (they may be written),
 *   and nothing at or beyond entry n - 2 of a slot is touched.
 * itd_baseline_extract_cubic_batch_f64: itd_baseline_extract_fast (itd_fourier_decomposition.py:49-122) of every signal.
 *   extrema_dev: idx + 1 knots as in itd_baseline_extract_cubic_f64 — ONE list for every signal (extrema_stride = 0: "retain the
 *   extrema and reuse them ... along multiple channels", itd.cpp:40-44) or one per signal (extrema_stride >= idx + 1);
 *   NULL = every signal's own knots by itd.cpp:159-169.  A signal with fewer than 2 knots or an invalid list keeps its
 *   baseline row untouched.  info_dev (optional) [batch]: the idx used; -1 = invalid list, -2 = NaN in the signal.  batch <= 65535. */
int itd_baseline_extract_batch_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride, double *rot_dev,
                                   int64_t rot_stride, double *base_dev, int64_t base_stride, int32_t *info_dev, void *stream);
int itd_detect_batch_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride, int32_t mode, int32_t *idx_dev,
                         int64_t idx_stride, int32_t *info_dev, void *stream);
int itd_baseline_extract_cubic_batch_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride,
                                         const int32_t *extrema_dev, int64_t extrema_stride, int64_t idx, double *baseline_dev,
                                         int64_t baseline_stride, int32_t *info_dev, void *stream);

/* ---- instantaneous amplitude / phase / frequency of many rows: asynchronous on `stream`, no host synchronisation, no host read,
 * graph-capturable.  The definitions and the arithmetic of itd_instantaneous_f64 (on a row without a NaN the results are bit for bit
 * that call's), for float64 or float32 rows — a float32 sample is widened exactly — as they come from itd_decompose_* and
 * itd_decompose_rows32_*.  Row r starts at rows_dev + r * row_stride; its outputs at r * out_stride ELEMENTS of the output type
 * behind amp_dev / phase_dev / freq_dev: float64 (out_f32 = 0) or float32 (out_f32 = 1: each element the float64 one rounded once
 * at its store, as itd_decompose_rows32_* rounds).  Any output may be NULL, not all three.  3 <= n < 2^31 - 65537 as for the other
 * batched entries; rows >= 1, above 65535 rows in chunks; both strides >= n when rows > 1; the outputs must not overlap the input.
 * info_dev (optional) [rows]: the row's zero-crossing count; -1 - count if the row holds a NaN — its outputs are then
 * unspecified, but nothing outside its n elements of each output is written.  Nothing outside the first n samples of a row is read.
 * The workspace (40 bytes per 512 samples of min(rows, 65535) rows) is the engine's, grown on demand: the capture rule of the batched
 * single-level operators above holds — capture a call only after one of its size has run, capture again after a larger one. */
int itd_instantaneous_batch_f64(itd_engine *e, const double *rows_dev, int64_t n, int32_t rows, int64_t row_stride, void *amp_dev,
                                void *phase_dev, void *freq_dev, int64_t out_stride, int32_t out_f32, int32_t *info_dev, void *stream);
int itd_instantaneous_batch_f32(itd_engine *e, const float *rows_dev, int64_t n, int32_t rows, int64_t row_stride, void *amp_dev,
                                void *phase_dev, void *freq_dev, int64_t out_stride, int32_t out_f32, int32_t *info_dev, void *stream);

/* ---- the time-frequency-energy spectrum of many rows: every row's energy binned over time and frequency:
 * asynchronous on `stream`, no host synchronisation, no host read, graph-capturable.  For a row x[0..n) that holds no NaN, A[j] and
 * f[j] are the instantaneous amplitude and frequency (cycles per sample) — the same bits itd_instantaneous_batch_* stores in
 * float64 — and never leave the GPU's registers.
 *   edges_dev [bins + 1] float64, finite and strictly increasing, 1 <= bins <= 512: device memory, read when the call runs — a
 *     captured call bins with whatever they hold at its replay.  Their order cannot be checked without reading device memory:
 *     unordered edges give unspecified bins (nothing outside the outputs is written).
 *   hop: a positive multiple of 64; below 512 only 64, 128 or 256.  T = ceil(n / hop) time bins.
 *   weight: 0 = count (w = 1.0), 1 = amplitude (w = A), 2 = energy (w = A * A, one float64 multiply).
 * The frequency bin of sample j is the k with edges[k] <= f[j] && f[j] < edges[k+1] as IEEE comparisons; a sample with no such k
 * (f below edges[0], at or above edges[bins], NaN) is OUTSIDE.  The order of every sum is part of the definition:
 *   step sum   step s covers samples 64 s .. 64 s + 63, counted from the row's first sample.  v[l] = w[64 s + l] if that sample
 *              exists and lies in bin k, else +0.0; the 64 values are reduced by the adjacent-pair tree (v0 + v1), (v2 + v3), ...,
 *              then pairs of those, six levels.  All weights are non-negative, so the +0.0 entries change nothing.
 *   cell       S[t, k] starts at +0.0; the step sums of the steps t * hop / 64 .. (t + 1) * hop / 64 - 1 that exist are added one
 *              after the other, in increasing step order.
 *   outside    outside[t] = the number of outside samples with j / hop == t.
 * Row r's spectrum [T][bins] float64 (also for float32 rows) sits at spec_dev + r * spec_stride, spec_stride >= T * bins when
 * rows > 1; outside_dev (optional) [rows][T] int32, dense.  Every cell and every entry is written, an empty cell as +0.0: the
 * buffers need no clearing, and nothing else is written.  No atomics on global memory and no floating-point atomics: the result
 * is the same bits from run to run and in any batch position.  Rows, n, row_stride, chunking and info_dev as for
 * itd_instantaneous_batch_* (info: the zero-crossing count, -1 - count if the row holds a NaN — that row's spectrum is then not to
 * be used).  ITD_ERR_INVALID_ARG before any launch for bins, hop or weight out of range, n < 3 or a stride too small.  The parallel
 * grain is (row, time bin) — (row, 512 samples) where hop < 512: a caller who wants a marginal spectrum sums a spectrum of many
 * time bins rather than asking for hop >= n.  The workspace (40 bytes per 512 samples of min(rows, 65535) rows) is the engine's
 * own, apart from the instantaneous step's, grown on demand: the capture rule of the batched single-level operators above holds. */
int itd_tfe_spectrum_f64(itd_engine *e, const double *rows_dev, int64_t n, int32_t rows, int64_t row_stride, const double *edges_dev,
                         int32_t bins, int64_t hop, int32_t weight, double *spec_dev, int64_t spec_stride, int32_t *outside_dev,
                         int32_t *info_dev, void *stream);
int itd_tfe_spectrum_f32(itd_engine *e, const float *rows_dev, int64_t n, int32_t rows, int64_t row_stride, const double *edges_dev,
                         int32_t bins, int64_t hop, int32_t weight, double *spec_dev, int64_t spec_stride, int32_t *outside_dev,
                         int32_t *info_dev, void *stream);

/* ---- single-wave analysis of many rows (README.md:18-21, 47-53: "feature-based filtering" on the half waves): asynchronous on
 * `stream`, no host synchronisation, no host read, graph-capturable.  A row's crossing indices c_0 < ... < c_{m-1} are those of
 * itd_instantaneous_* (1 <= i <= n - 2 with a strict sign change x[i] -> x[i+1]); half wave k (0 <= k <= m) holds the samples
 * start_k .. end_k with start_0 = 0, start_k = c_{k-1} + 1, end_k = c_k, end_m = n - 1; length_k = end_k - start_k + 1;
 * A_k = max |x| over it (what itd_instantaneous_batch_* delivers per sample); peak_k = the smallest index of the half wave with
 * |x| == A_k; value_k = x[peak_k], the signed extremum.  All decisions are exact on the sample as float64 (a float32 sample is
 * widened exactly).  count = m + 1 <= n - 1.  Rows, strides, n, chunking and info_dev as for itd_instantaneous_batch_*: row r at
 * rows_dev + r * row_stride; 3 <= n < 2^31 - 65537; rows >= 1, above 65535 rows in chunks; row_stride >= n when rows > 1;
 * info_dev (optional) [rows]: the row's zero-crossing count, -1 - count if the row holds a NaN — its table entries and its
 * filtered row are then unspecified, but nothing outside that row's own slots is written.  Nothing outside the first n samples of
 * a row is read.
 * itd_waves_batch_f64 / _f32: the table.  Row r's entries sit at r * wave_stride elements behind start_dev / length_dev / peak_dev
 *   (int32) and value_dev (double, also for float32 rows: the widened sample); wave_stride >= cap when rows > 1.  The first
 *   min(count, cap) entries of a slot are written, in the half waves' order; nothing at or beyond entry cap of a slot is touched, and
 *   the entries from count on are left as they were.  count_dev (optional) [rows]: always the true count, so count > cap shows an
 *   overflow.  Any table pointer may be NULL; if all four are, cap and wave_stride are ignored and the call only counts (no table
 *   pass runs); count_dev or at least one table must be given.  cap >= 1 with a table.
 * itd_wave_filter_batch_f64 / _f32: out[j] = x[j] if the half wave k of sample j has amp_lo <= A_k && A_k <= amp_hi &&
 *   len_lo <= (double)length_k && (double)length_k <= len_hi as IEEE comparisons (a NaN bound keeps nothing), else +0.0.  The four
 *   float64 bounds (amp_lo, amp_hi, len_lo, len_hi) of row r are read from bounds_dev + r * bounds_stride: bounds_stride = 0 is
 *   one set for every row, bounds_stride >= 4 one set per row (as extrema_stride of the cubic batch); they are device memory, read
 *   when the call runs — a captured call filters with whatever they hold at its replay.  Row r's output at r * out_stride ELEMENTS
 *   of the output type behind out_dev: float64 (out_f32 = 0) or float32 (out_f32 = 1: the kept sample rounded once at its store);
 *   out_stride >= n when rows > 1; out_dev must not overlap the input.  Bounds (0, +inf, 0, +inf) make a float64 output a
 *   bit-exact copy of the row.
 * The workspace (80 bytes per 512 samples of min(rows, 65535) rows: a 40-byte tile record, a 24-byte forward and a 16-byte
 * backward carry) is the engine's own, apart from the instantaneous step's, grown on demand: the capture rule of the batched
 * single-level operators above holds — capture a call only after one of its size has run, capture again after a larger one. */
int itd_waves_batch_f64(itd_engine *e, const double *rows_dev, int64_t n, int32_t rows, int64_t row_stride, int32_t *start_dev,
                        int32_t *length_dev, int32_t *peak_dev, double *value_dev, int64_t wave_stride, int32_t cap, int32_t *count_dev,
                        int32_t *info_dev, void *stream);
int itd_waves_batch_f32(itd_engine *e, const float *rows_dev, int64_t n, int32_t rows, int64_t row_stride, int32_t *start_dev,
                        int32_t *length_dev, int32_t *peak_dev, double *value_dev, int64_t wave_stride, int32_t cap, int32_t *count_dev,
                        int32_t *info_dev, void *stream);
int itd_wave_filter_batch_f64(itd_engine *e, const double *rows_dev, int64_t n, int32_t rows, int64_t row_stride, const double *bounds_dev,
                              int64_t bounds_stride, void *out_dev, int64_t out_stride, int32_t out_f32, int32_t *info_dev, void *stream);
int itd_wave_filter_batch_f32(itd_engine *e, const float *rows_dev, int64_t n, int32_t rows, int64_t row_stride, const double *bounds_dev,
                              int64_t bounds_stride, void *out_dev, int64_t out_stride, int32_t out_f32, int32_t *info_dev, void *stream);

/* ---- the joint amplitude-length histogram of many rows' half waves: how a row's half waves are distributed
 * over amplitude, length and time, without the table — what a caller looks at to choose itd_wave_filter_batch_*'s bounds.
 * Asynchronous on `stream`, no host synchronisation, no host read, graph-capturable.  For a row x[0..n) that holds no NaN, its half
 * waves k = 0 .. m have start_k, end_k, length_k, A_k and peak_k exactly as defined for itd_waves_batch_* above.  Given amplitude
 * edges ae[0..abins], length edges le[0..lbins] (float64) and hop, every half wave has
 *   amplitude bin   the i with ae[i] <= A_k && A_k < ae[i+1]
 *   length bin      the j with le[j] <= (double)length_k && (double)length_k < le[j+1]
 *   time bin        t = peak_k / hop (integer division); T = ceil(n / hop)
 * as IEEE comparisons on float64, half-open bins as in itd_tfe_spectrum_*.  If both i and j exist, count[t][i][j] += 1 and
 * samples[t][i][j] += length_k; otherwise outside[t] += 1.  All three outputs are int32 and cannot overflow (a row has at most
 * n - 1 half waves and n samples).  sum(count) + sum(outside) = m + 1, and sum(samples) plus the lengths of the outside half waves
 * is n.  Every cell and every entry is written by the call, an empty cell as 0: the buffers need no clearing, and nothing else is
 * written.  Every update is an integer add (no floating-point atomics): the result is the same bits from run to run and in any
 * batch position.
 *   aedges_dev, ledges_dev: row r's edges at aedges_dev + r * aedges_stride (abins + 1 values) and ledges_dev + r * ledges_stride
 *     (lbins + 1 values); a stride of 0 is one set for every row, otherwise aedges_stride >= abins + 1, ledges_stride >= lbins + 1
 *     (as bounds_stride of the filter).  Strictly increasing, no NaN; -inf as a first and +inf as a last edge are allowed.  They
 *     are device memory, read when the call runs — a captured call bins with whatever they hold at its replay.  Their order cannot
 *     be checked without reading device memory: unordered edges give unspecified bins (nothing outside the outputs is written).
 *   1 <= abins <= 64, 1 <= lbins <= 64, abins * lbins <= 1024.
 *   hop: a positive multiple of 512 (a half wave whose peak lies in a 512-sample tile falls into one time bin); a multiple of 512
 *     that is >= n gives T = 1.
 *   count_dev, samples_dev: row r's [T][abins][lbins] int32 at r * hist_stride elements, hist_stride >= T * abins * lbins when
 *     rows > 1; the gaps between the rows' slots are not written.  Either may be NULL, not both.  outside_dev (optional):
 *     [rows][T] int32, dense.
 * Rows, n, row_stride, chunking and info_dev as for itd_waves_batch_* (info: the zero-crossing count m, -1 - m if the row holds a
 * NaN — that row's histogram is then unspecified, but nothing outside its own slots is written).  ITD_ERR_INVALID_ARG before any
 * launch for bins, hop or a stride out of range, n < 3, missing edges or both histograms NULL.  The workspace is the single-wave
 * analysis's (80 bytes per 512 samples of min(rows, 65535) rows); its capture rule holds. */
int itd_wave_hist_batch_f64(itd_engine *e, const double *rows_dev, int64_t n, int32_t rows, int64_t row_stride, const double *aedges_dev,
                            int64_t aedges_stride, int32_t abins, const double *ledges_dev, int64_t ledges_stride, int32_t lbins,
                            int64_t hop, int32_t *count_dev, int32_t *samples_dev, int64_t hist_stride, int32_t *outside_dev,
                            int32_t *info_dev, void *stream);
int itd_wave_hist_batch_f32(itd_engine *e, const float *rows_dev, int64_t n, int32_t rows, int64_t row_stride, const double *aedges_dev,
                            int64_t aedges_stride, int32_t abins, const double *ledges_dev, int64_t ledges_stride, int32_t lbins,
                            int64_t hop, int32_t *count_dev, int32_t *samples_dev, int64_t hist_stride, int32_t *outside_dev,
                            int32_t *info_dev, void *stream);

/* ---- the wave filter's bounds from histogram quantiles: the step between itd_wave_hist_batch_* and
 * itd_wave_filter_batch_*, on the device.  Asynchronous on `stream`, no host synchronisation, no host read, graph-capturable.
 * A row has a histogram h[T][na][nl] of int32 cells, non-negative (the caller's duty) — `count` or `samples` of itd_wave_hist_batch_*
 * or of the histogram stream's slices: the caller chooses by the pointer it passes —, a range of time bins [t0, t1), its edges
 * ae[0..na], le[0..nl] and eight float64 parameters q = (aq_lo, aq_hi, lq_lo, lq_hi, as_lo, as_hi, ls_lo, ls_hi).  In int64:
 *   ma[i] = sum over t0 <= t < t1 and j of h[t][i][j],  ml[j] = the same over t and i,  N = sum ma = sum ml, below 2^53.
 * One axis with marginal m[0..B), edges e[0..B], inclusive prefix sums cum[i], quantiles q_lo, q_hi and scales s_lo, s_hi:
 *   N == 0      iL = 0, iU = B - 1: the whole edge range.
 *   otherwise   tau_lo = q_lo * (double)N and tau_hi = q_hi * (double)N, one IEEE multiply each;
 *               iL = the smallest i with (double)cum[i] > tau_lo; if there is none (q_lo = 1; a NaN), the smallest i with
 *                    cum[i] == N, the last non-empty bin;
 *               iU = max(iL, the smallest i with (double)cum[i] >= tau_hi; if there is none (q_hi above 1; a NaN), B - 1).
 *   lo = e[iL] * s_lo, hi = e[iU + 1] * s_hi, one IEEE multiply each: a scale of 1.0 gives the edge's own bits; inf * 0 gives a
 *   NaN bound, with which the filter keeps nothing.
 * So 0 <= iL <= iU < B whatever q holds; for 0 <= q_lo <= q_hi <= 1 bin iL is not empty and the bins iL .. iU hold at least
 * (q_hi - q_lo) N of the total.  The filter's intervals are closed while the bins are half-open: a half wave whose amplitude equals
 * the upper edge e[iU + 1] exactly is kept.  Output: bounds (amp_lo, amp_hi, len_lo, len_hi) in itd_wave_filter_batch_*'s layout,
 * and N.  Every decision is an integer sum and a comparison, every sum an integer add (no floating-point atomics): the same bits
 * from run to run and in any batch position.
 *   hist_dev: row r's cells at r * hist_stride elements; hist_stride >= T * na * nl when rows > 1.  0 <= t0 < t1 <= T < 2^31.
 *   1 <= na <= 64, 1 <= nl <= 64, na * nl <= 1024.
 *   aedges_dev, ledges_dev, quant_dev: row r's at r * the stride; a stride of 0 is one set for every row, otherwise
 *     aedges_stride >= na + 1, ledges_stride >= nl + 1, quant_stride >= 8.  Device memory, read when the call runs: a captured call
 *     follows them, and the histogram, from replay to replay.
 *   bounds_dev: row r's four float64 at r * bounds_stride, bounds_stride >= 4.  total_dev (optional): [rows] int64.  Nothing else
 *     is written, whatever the parameters hold.
 * Any rows >= 1; more than 65535 go in chunks.  ITD_ERR_INVALID_ARG before any launch for a NULL handle or required pointer or a
 * value or stride out of range.
 * The call runs on a handle of its own, itd_bounds (itd_bounds_create(out, device) / itd_bounds_destroy; itd_bounds_last_error for
 * the text behind ITD_ERR_HIP), not on an itd_engine: the handle owns the call's stream (used when `stream` is NULL) and its
 * workspace (1 KB per row of min(rows, 65535) rows, grown on demand and zeroed by a kernel of the call), so nothing of this call
 * lies in an engine that other operators work in, and no order of other calls can reach its result.  The batched operators' capture
 * rule holds: capture a call only after one of its row count has run; a captured call stays valid until a call on the same handle
 * with more rows grows the workspace.  Not thread-safe: one handle per host thread. */
typedef struct itd_bounds itd_bounds;   /* opaque */
int itd_bounds_create(itd_bounds **out, int device_id);
void itd_bounds_destroy(itd_bounds *b);
const char *itd_bounds_last_error(const itd_bounds *b);
int itd_wave_bounds_batch(itd_bounds *b, const int32_t *hist_dev, int32_t rows, int64_t hist_stride, int64_t T, int64_t t0, int64_t t1,
                          int32_t na, int32_t nl, const double *aedges_dev, int64_t aedges_stride, const double *ledges_dev,
                          int64_t ledges_stride, const double *quant_dev, int64_t quant_stride, double *bounds_dev, int64_t bounds_stride,
                          int64_t *total_dev, void *stream);

/* ---- the ITD-Fourier cascade (itd_fourier_decomposition.py:131-303) and its FFT ---------------------------------------------
 * itd_debug_fft_f64 (tests): `batch` transforms of n complex float64 points (interleaved re, im; transform b at 2 b n doubles) from
 *   in_dev into out_dev (may be in_dev): inverse 0 = numpy.fft.fft, 1 = numpy.fft.ifft (scaled by 1 / n).  n <= 8192: one
 *   workgroup per transform in LDS; n = n1 n2 with n1, n2 <= 8192: four steps; any other n: Bluestein over a power of two
 *   M >= 2n - 1 (M <= 2^26, else ITD_ERR_INVALID_ARG).  Synchronous.
 * itd_fourier_mode_any_f64 / itd_fourier_mode_valid_f64: fourier_mode_decomposition_any (:171-209) / _valid (:131-168) of `rows` real
 *   rows of n >= 4 samples (row r at rows_dev + r row_stride) as one batched operator: forward FFT, the selector's decision and its
 *   masked spectrum xn in complex64 values (xn[mina:minb] = X[mina:minb], xn[-minb:-mina] = X[-minb:-mina] literally: empty when
 *   mina == 0, not the Hermitian mirror), the full complex inverse of xn; its real part into modes_dev (row r at modes_dev +
 *   r mode_stride; zeros for a rejection).  rec_dev (optional) [rows][8]: status (1 mode, 0 rejected), peak_max, first_peak,
 *   last_peak, mina, minb, 0, 0 (-1: not reached).  Asynchronous on `stream`.
 * itd_fourier_cascade_f64: itd_fourier_decomposition (:212-255; lean = 0) or itd_fourier_decomposition_lean (:258-303; lean = 1) of
 *   `batch` signals of n samples (signal b at x_dev + b x_stride; never written).  The band plan is the caller's: `bands` knot lists
 *   of itd_sine_wrapper (:33-47: find_extrema of the band's sine), back to back in knots_host, list k with idx_host[k] + 1 entries
 *   as for itd_baseline_extract_cubic_f64 (2 <= idx <= n - 1, every entry < n); it is kept on the device per engine while
 *   (n, sample_rate, lists) stay the same.  A round runs the bands, the selector _any on every row but the residual, the mode test
 *   (not np.allclose(mode, 0): some |mode| > 1e-8), row -= mode, and the next signal as the sum of the rows in row order; a
 *   signal whose round finds no mode leaves the loop.  One host synchronisation per round.
 *   rows_dev [batch][bands + 1][n]: the final rows (rotations less their modes, then the residual); at the cap (a round with modes
 *   numbered max_rounds >= 1) the rows of that round.  acc_dev (lean) [batch][bands][n]: the modes accumulated per row.
 *   rounds_host [batch]: rounds that found modes (the reference's iteration - 1); capped_host: stopped at the cap; modes_host:
 *   modes found.  ITD_ERR_NONFINITE if a signal holds a NaN.  Synchronous.
 * itd_fourier_cascade_host_f64: the same on host arrays (x_host [batch][n]).
 * itd_fourier_modes_f64: the last cascade's modes in the order found (round, then signal, then row): modes_dst [count][n] (host if
 *   to_host, else device; NULL: records only; a lean call keeps no modes) and records_host [count][8]: signal, round, source row,
 *   peak_max, first_peak, last_peak, mina, minb. */
int itd_debug_fft_f64(itd_engine *e, const double *in_dev, double *out_dev, int64_t n, int32_t batch, int32_t inverse);
int itd_fourier_mode_any_f64(itd_engine *e, const double *rows_dev, int64_t n, int64_t rows, int64_t row_stride, double *modes_dev,
                             int64_t mode_stride, int32_t *rec_dev, void *stream);
int itd_fourier_mode_valid_f64(itd_engine *e, const double *rows_dev, int64_t n, int64_t rows, int64_t row_stride, double *modes_dev,
                               int64_t mode_stride, int32_t *rec_dev, void *stream);
int itd_fourier_cascade_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride, double sample_rate,
                            int32_t bands, const int64_t *knots_host, const int64_t *idx_host, int32_t lean, int32_t max_rounds,
                            double *rows_dev, double *acc_dev, int32_t *rounds_host, int32_t *capped_host, int64_t *modes_host);
int itd_fourier_cascade_host_f64(itd_engine *e, const double *x_host, int64_t n, int32_t batch, double sample_rate, int32_t bands,
                                 const int64_t *knots_host, const int64_t *idx_host, int32_t lean, int32_t max_rounds, double *rows_host,
                                 double *acc_host, int32_t *rounds_host, int32_t *capped_host, int64_t *modes_host);
int itd_fourier_modes_f64(itd_engine *e, double *modes_dst, int64_t count, int32_t *records_host, int32_t to_host);

/* ---- block-wise (streaming) operation for unbounded signals (ABI revision 6) ------------------------------
 * The recipe of the comment at itd.cpp:31-38 — "use a circular buffer with modulous tracking to rotate the samples / re-assess
 * extrema in the entire buffer every iteration / use from the last extrema in the first buffer to the first extrema in the last
 * buffer / set the first and last baseline knots manually to said values / update the j array / compute only the baseline[i]
 * array for the inner third of the buffer overall / rotate buffers, rinse and repeat" — and itd.cpp:40-44's retained extrema
 * along channels.  There is no reference code for it; oracle/stream_oracle.py states the recipe the tests hold this to.
 *
 * A stream keeps the last three blocks of `channels` channels in a device-resident ring.  A push stores one block of every
 * channel and, from the second push on, emits the baseline (and rotation) of the PREVIOUS block — latency one block; flush
 * emits the last block and empties the stream.  Window = the previous, the emitted and the next block (two blocks at either
 * end of the stream, one if the stream holds a single block).
 *   ITD_STREAM_CUBIC   itd_baseline_extract_fast (itd_fourier_decomposition.py:49-122) on the window's extrema (itd.cpp:161-168)
 *                      from `margin` extrema in front of the emitted block to margin + 2 behind it (the recipe's literal
 *                      choice is margin 1; the two extra keep the operator's uncomputed second-to-last knot value, K[idx-1]
 *                      = 0, outside the block); the first and last knot value are the data there (itd.cpp:35).  Fewer than 4
 *                      such extrema: the block is emitted unchanged (itd.cpp:170-172).  shared_knots: the extrema of channel
 *                      0's window serve every channel (itd.cpp:40-44).
 *   ITD_STREAM_LINEAR  itd_baseline_extract (ITD.py:79-121) on the window, every channel on its own knots.  The operator is
 *                      local (two knots either side of a sample), so wherever the blocks hold a few knots the emitted stream is
 *                      bit-identical to the whole-signal operator's rows.
 * Ring, knot detection, knot selection and the operator all run on the device: a device-form push / flush enqueues its
 * launches on `stream` and returns (no host synchronisation; `*emitted` is known from the block count alone); the host forms
 * copy through pinned staging and synchronise once per call.
 * A NaN.  ITD_STREAM_LINEAR: the block is emitted under plain comparison rules.  ITD_STREAM_CUBIC: nothing is built on a window
 * that holds a NaN — every block that takes its knots from such a window (the channel's own; channel 0's under shared_knots) is
 * emitted unchanged, rotation 0.  Under shared_knots a channel other than 0 that holds a NaN while channel 0's window is finite
 * gets a spline on channel 0's knots through its NaN: its samples of that block are unspecified (the NaN spreads through the
 * sweeps), the other channels are not touched by it.  Either kind: a NaN in ANY channel's pushed block is recorded when the
 * block is stored — the device forms leave it for itd_stream_status, the host forms return ITD_ERR_NONFINITE (outputs filled in)
 * from the first emitting call on, until itd_stream_reset. */
typedef struct itd_stream itd_stream;   /* opaque; not thread-safe */
#define ITD_STREAM_CUBIC 0
#define ITD_STREAM_LINEAR 1
#define ITD_STREAM_LEVELS 2   /* a levels stream (itd_levels_stream_create); not a kind itd_stream_create takes */
int itd_stream_create(itd_stream **out, int device_id, int64_t block /* samples, >= 8 */, int32_t channels, int32_t kind,
                      int32_t margin /* cubic: >= 1 */, int32_t shared_knots);
void itd_stream_destroy(itd_stream *s);
int itd_stream_reset(itd_stream *s);            /* forget the blocks held and the recorded status */
int64_t itd_stream_blocks(const itd_stream *s); /* blocks held since create / reset / flush */
const char *itd_stream_last_error(const itd_stream *s);
/* block_dev [channels] rows of `block` samples at in_stride; baseline_dev / rot_dev (optional) likewise, written when
 * *emitted = 1 (every push but the first; every flush of a non-empty stream) */
int itd_stream_push_f64(itd_stream *s, const double *block_dev, int64_t in_stride, double *baseline_dev, int64_t baseline_stride,
                        double *rot_dev, int64_t rot_stride, int32_t *emitted, void *stream);
int itd_stream_flush_f64(itd_stream *s, double *baseline_dev, int64_t baseline_stride, double *rot_dev, int64_t rot_stride,
                         int32_t *emitted, void *stream);
/* host forms: contiguous [channels][block] arrays; rot_host optional */
int itd_stream_push_host_f64(itd_stream *s, const double *block_host, double *baseline_host, double *rot_host, int32_t *emitted);
int itd_stream_flush_host_f64(itd_stream *s, double *baseline_host, double *rot_host, int32_t *emitted);
/* synchronises the device; *status = 0, or 2 if some block of some channel pushed since create / reset held a NaN */
int itd_stream_status(itd_stream *s, int32_t *status);

/* ---- the levels stream: the full multi-level ITD block by block -----------------------------------------------------------
 * A chain of levels + 1 (M + 1) ITD_STREAM_LINEAR stages: stage 0 runs on the caller's blocks, stage k >= 1 on the baselines
 * stage k-1 emits.  The rows of block j are the rotations of stages 0 .. M-1 and, as row M, stage M's rotation + baseline
 * (ITD.py:418-426, the driver's "Out of time!" row): where the whole signal runs to max_iteration = M-1 without a natural
 * stop these are block j's columns of ITD().itd(x, M-1).  Block j's rows leave on push j+M+1 (blocks and pushes counted from 0;
 * the minimum: stage k emits block j once it holds block j+1 of its input), so the first M+1 pushes emit nothing; flush emits
 * one block per call (emitted = 0 once empty, and the stream then starts afresh).  A push between flushes is refused.
 * Each emitted block comes with exact[c] = 1 where its M+1 rows are certified bit-identical to the whole-signal rows of the
 * concatenated blocks (a sound, conservative rule; the rule and its argument: itd_stream.hpp, k_stream_levels); a window
 * holding a NaN is never certified and sets itd_stream_status's bit 2 (the block follows the single-level stream's plain rules).
 * block >= 8 samples, channels 1 .. 65535, levels 1 .. 21.  Blocks up to 2730 samples (3 blocks <= 8192) take ONE launch per
 * step (one workgroup per channel holds the window in LDS); longer blocks take a launch sequence (per stage: the batched tier-1
 * extraction of every channel's window, then one routing / certificate kernel), bit-identical to the one-launch form.
 * itd_levels_stream_set_sequence(s, 1) forces the sequence form on a short block (0: back to one launch; refused for a long
 * block); itd_levels_stream_form returns the form in use (0 one launch, 1 sequence, -1 not a levels stream).  The form may be
 * switched between any two steps of a stream that holds blocks (both forms keep the same rings, delay line and flag bytes; the
 * results are those of either form alone).  Everything is
 * allocated at create (or, for a forced sequence form, by the setter; ITD_ERR_NOMEM when it does not fit): M+1 rings of 5
 * blocks and M (M+1) / 2 delayed blocks per channel, plus, for the sequence form, the windows' results (6 blocks per channel).  itd_stream_destroy / reset / status / blocks / last_error apply; the
 * single-level push / flush entries refuse a levels stream.
 * Device forms: block_dev [channels][block] at in_stride; rows_dev[c][r][s] at c chan_stride + r row_stride + s (row_stride >=
 * block, chan_stride >= M row_stride + block when channels > 1), required when the call emits; exact_dev [channels] optional.
 * They enqueue on `stream` and return.  Host forms: contiguous [channels][block] in, [channels][M+1][block] rows and [channels]
 * flags out, one synchronisation per call. */
int itd_levels_stream_create(itd_stream **out, int device_id, int64_t block, int32_t channels, int32_t levels);
int itd_levels_stream_set_sequence(itd_stream *s, int32_t on);
int itd_levels_stream_form(const itd_stream *s);
int itd_levels_stream_push_f64(itd_stream *s, const double *block_dev, int64_t in_stride, double *rows_dev, int64_t row_stride,
                               int64_t chan_stride, uint8_t *exact_dev, int32_t *emitted, void *stream);
int itd_levels_stream_flush_f64(itd_stream *s, double *rows_dev, int64_t row_stride, int64_t chan_stride, uint8_t *exact_dev,
                                int32_t *emitted, void *stream);
int itd_levels_stream_push_host_f64(itd_stream *s, const double *block_host, double *rows_host, uint8_t *exact_host, int32_t *emitted);
int itd_levels_stream_flush_host_f64(itd_stream *s, double *rows_host, uint8_t *exact_host, int32_t *emitted);

/* ---- the wave-filter stream: the single-wave feature filter block by block, at a fixed latency -----
 * itd_wave_filter_batch_* needs the whole row: a half wave's amplitude and length are known only once it has ended.  A wave-filter
 * stream takes blocks of `rows` rows in lock step and gives the same blocks back filtered, a known number of blocks later.  With
 * blocks of L samples and a horizon of H samples, row r after P pushes is x[0 .. P L).  Crossing indices, half waves, A_k and
 * length_k are exactly those of itd_waves_batch_* above on the indices of the whole stream; the last half wave ends at the
 * stream's last sample, known at the flush.  The output is
 *   y[j] = x[j]  if the half wave k of sample j has length_k <= H && amp_lo <= A_k && A_k <= amp_hi &&
 *                len_lo <= (double)length_k && (double)length_k <= len_hi   (IEEE comparisons on float64; a NaN bound keeps nothing)
 *          +0.0  otherwise
 * — itd_wave_filter_batch_f64 of the concatenated blocks with len_hi replaced by min(len_hi, H), bit for bit; with len_hi <= H
 * the whole-row filter itself.  A HALF WAVE LONGER THAN THE HORIZON IS NEVER KEPT: that is the price of a bounded latency.
 * Latency D = ceil(H / L) blocks (itd_wave_stream_latency; -1 if s is not a wave stream): push p (counted from 0) emits block
 * p - D when p >= D; every flush emits the next block still held, so min(P, D) flushes emit, emitted = 0 once the stream is empty,
 * and the stream then starts afresh.  A push between flushes is refused.  Block b is decided from the samples
 * [b L - H, (b+1) L + H) that exist and from nothing else; a ring of 2 D + 1 blocks per row is the stream's whole state.
 *   8 <= block <= 8192, 1 <= rows <= 65535, 1 <= horizon <= 2^22.  Everything is allocated at create: the rings
 *   (rows (2 D + 1) block 8 bytes), one 16-byte record per block in them (rows (2 D + 1) 16 bytes: whether the block holds a crossing
 *   index, its largest magnitude), the host forms' device and pinned staging (two blocks and four bounds per row, each twice) and,
 *   as for the other streams, an engine of the stream's own (its launch stream and error text); ITD_ERR_NOMEM when it does not
 *   fit.  ITD_ERR_INVALID_ARG before any HIP call for a NULL handle, a NULL pointer or a value out of range.  A call that fails
 *   leaves the stream as it was: a flush whose launch fails has emitted nothing and has not begun the flush.
 *   block_dev: row r's block at block_dev + r in_stride (in_stride >= block when rows > 1) — the dense [channels][M+1][block] rows of
 *     itd_levels_stream_push_f64 go in as channels (M+1) rows with in_stride = block.
 *   out_dev: row r's filtered block at out_dev + r out_stride; required whenever the call emits, written only then.
 *   bounds_dev: (amp_lo, amp_hi, len_lo, len_hi) of row r at bounds_dev + r bounds_stride, bounds_stride 0 (one set for every row)
 *     or >= 4; device memory, read when the launch runs, as for itd_wave_filter_batch_*; required whenever the call emits.  A block
 *     is filtered with the bounds that hold when it is emitted: a caller who changes the bounds in mid-stream judges a half wave
 *     that spans two emitted blocks under both sets.
 * Device forms: one launch per call on `stream`, no host synchronisation, no host read; *emitted follows from the block count
 * alone.  Host forms: contiguous [rows][block] in and out, bounds_host [rows][4]; pinned staging, one synchronisation per call.
 * A NaN in any pushed block sets bit 2 of itd_stream_status until itd_stream_reset; that row's emitted samples are unspecified
 * from then on, nothing outside the row's own slots is written.  itd_stream_destroy / reset / blocks / status / last_error apply
 * (blocks: pushed and not yet emitted); the single-level and the levels push / flush entries refuse a wave stream. */
#define ITD_STREAM_WAVES 3    /* a wave-filter stream (itd_wave_stream_create); not a kind itd_stream_create takes */
int itd_wave_stream_create(itd_stream **out, int device_id, int64_t block, int32_t rows, int64_t horizon);
int itd_wave_stream_latency(const itd_stream *s);
int itd_wave_stream_push_f64(itd_stream *s, const double *block_dev, int64_t in_stride, const double *bounds_dev,
                             int64_t bounds_stride, double *out_dev, int64_t out_stride, int32_t *emitted, void *stream);
int itd_wave_stream_flush_f64(itd_stream *s, const double *bounds_dev, int64_t bounds_stride, double *out_dev,
                              int64_t out_stride, int32_t *emitted, void *stream);
int itd_wave_stream_push_host_f64(itd_stream *s, const double *block_host, const double *bounds_host, double *out_host,
                                  int32_t *emitted);
int itd_wave_stream_flush_host_f64(itd_stream *s, const double *bounds_host, double *out_host, int32_t *emitted);

/* ---- the spectrum stream: the time-frequency-energy spectrum block by block, at a fixed latency -----------
 * itd_tfe_spectrum_* needs the whole row: a sample's amplitude is its half wave's largest |x|, known only when the half wave ends.
 * A spectrum stream takes blocks of `rows` rows in lock step and gives finished time slices of their spectra, a known number of
 * blocks later.  With blocks of L samples, a horizon of H samples and hop | L, row r after P pushes is x[0 .. P L).
 *   A[j], f[j]   the instantaneous amplitude and frequency of the concatenated row: the same bits itd_instantaneous_batch_f64 gives for
 *                it (the same expressions; the stream's last sample takes the backward difference, known at the flush).
 *   overlong     sample j is overlong if its half wave has more than H samples, or sample j + 1 exists and ITS half wave has more
 *                than H samples (f[j] needs A[j + 1]); the stream's last sample, which has no successor and whose backward difference
 *                needs A of its predecessor, is overlong as well if that predecessor lies in another half wave of more than H
 *                samples.  An overlong sample is outside, whatever its frequency would be.
 *   emitted block b   C = L / hop cells: power[C][bins] (float64), outside[C], overlong[C] (int32) — exactly rows b C .. (b+1) C - 1 of
 *                itd_tfe_spectrum_f64's definition above applied to the concatenated row with the overlong samples forced outside:
 *                the same bins by the same comparisons, the same 64-sample step sums by the adjacent-pair tree, added into the cell
 *                in increasing step order.  Every cell is written, an empty one as +0.0.  outside counts the overlong samples too,
 *                overlong counts them alone.  Where no sample is overlong the slices are itd_tfe_spectrum_f64(concatenated rows,
 *                edges, hop, weight) bit for bit.
 * Latency D = ceil((H + 1) / L) blocks (itd_spectrum_stream_latency; -1 if s is not a spectrum stream) — one sample more than the
 * wave-filter stream's reach: the last sample of block b needs A of sample (b+1) L, whose half wave, if it has at most H samples,
 * ends at (b+1) L + H - 1 at the latest, and the crossing test reads one sample further.  Block b is decided from the samples
 * [b L - H, (b+1) L + H] that exist and from nothing else.  Push p (counted from 0) emits block p - D when p >= D; every flush emits
 * the next block still held, then emitted = 0 and the stream starts afresh.  A push between flushes is refused.
 *   64 <= block <= 4096, hop a value itd_tfe_spectrum_* accepts (a positive multiple of 64; below 512 only 64, 128, 256) that
 *   divides block, 1 <= rows <= 65535, 1 <= horizon <= 2^22, 1 <= bins <= 512, weight 0 (count), 1 (amplitude), 2 (energy).
 *   Everything is allocated at create: the rings (rows (2 D + 1) block 8 bytes), one 16-byte record per block in them, the host forms'
 *   staging and an engine of the stream's own; ITD_ERR_NOMEM when it does not fit.  ITD_ERR_INVALID_ARG before any HIP call for a
 *   NULL handle, a NULL pointer or a value out of range.  A call that fails leaves the stream as it was.
 *   block_dev: row r's block at block_dev + r in_stride (in_stride >= block when rows > 1).
 *   edges_dev: edges[0 .. bins] of row r at edges_dev + r edges_stride; edges_stride 0 (one set for every row) or >= bins + 1; device
 *     memory, read when the launch runs (finite and strictly increasing: the caller's duty); a caller may move them between pushes;
 *     required whenever the call emits.
 *   power_dev: row r's cells at power_dev + r power_stride (>= C bins when rows > 1); required whenever the call emits, written only then.
 *   outside_dev, overlong_dev: optional; row r's counts at + r count_stride (>= C when rows > 1).
 * Device forms: one launch per call on `stream`, no host synchronisation, no host read; *emitted follows from the block count alone.
 * Host forms: contiguous [rows][block] in, [rows][C][bins] and [rows][C] out, edges_host with edges_stride as above; pinned staging,
 * one synchronisation per call.  A NaN in any pushed block sets bit 2 of itd_stream_status until itd_stream_reset; that row is
 * unspecified from then on, nothing outside the row's own slots is written.  itd_stream_destroy / reset / blocks / status /
 * last_error apply; every other stream kind's push and flush entries refuse a spectrum stream, and these refuse theirs. */
#define ITD_STREAM_SPECTRUM 4 /* a spectrum stream (itd_spectrum_stream_create); not a kind itd_stream_create takes */
int itd_spectrum_stream_create(itd_stream **out, int device_id, int64_t block, int32_t rows, int64_t horizon, int64_t hop, int32_t bins,
                               int32_t weight);
int itd_spectrum_stream_latency(const itd_stream *s);
int itd_spectrum_stream_push_f64(itd_stream *s, const double *block_dev, int64_t in_stride, const double *edges_dev, int64_t edges_stride,
                                 double *power_dev, int64_t power_stride, int32_t *outside_dev, int32_t *overlong_dev,
                                 int64_t count_stride, int32_t *emitted, void *stream);
int itd_spectrum_stream_flush_f64(itd_stream *s, const double *edges_dev, int64_t edges_stride, double *power_dev, int64_t power_stride,
                                  int32_t *outside_dev, int32_t *overlong_dev, int64_t count_stride, int32_t *emitted, void *stream);
int itd_spectrum_stream_push_host_f64(itd_stream *s, const double *block_host, const double *edges_host, int64_t edges_stride,
                                      double *power_host, int32_t *outside_host, int32_t *overlong_host, int32_t *emitted);
int itd_spectrum_stream_flush_host_f64(itd_stream *s, const double *edges_host, int64_t edges_stride, double *power_host,
                                       int32_t *outside_host, int32_t *overlong_host, int32_t *emitted);

/* ---- the instantaneous stream: amplitude, phase, frequency and half-wave length block by block, at a fixed latency (DESIGN.md
 *      section 24) -----------------------------------------------------------------------------------------------------------------
 * The third consumer stage behind a levels stream: blocks of `rows` rows in lock step go in; the per-sample instantaneous amplitude,
 * phase and frequency and the length of every sample's half wave come out, a known number of blocks later — wherever a value is
 * delivered, bit for bit the whole-row operator's.  With blocks of L samples and a horizon of H samples, row r after P pushes is
 * x[0 .. P L).  On the concatenated row:
 *   len[j]       the number of samples of sample j's half wave: the half waves of itd_waves_batch_* on the indices of the whole
 *                stream; the last one ends at the flushed stream's last sample.
 *   A[j], phase[j], f[j]   the bits itd_instantaneous_batch_f64 gives for the concatenated row (the same expressions; the stream's
 *                last sample takes the backward difference, known at the flush).
 *   long[j]      len[j] > H.
 *   overlong[j]  the spectrum stream's rule above, unchanged: long[j], or long[j + 1] where j + 1 exists, or, for the stream's last
 *                sample, long[j - 1].
 *   emitted block b, for each of its L samples:
 *                amplitude[j] = A[j], phase[j] = phase[j]   where !long[j]  (both need only j's own half wave and x[j + 1])
 *                frequency[j] = f[j]                        where !overlong[j]
 *                length[j]    = len[j] (int32)              where !long[j], else 0
 *                every float64 value that is not delivered is the one pattern 0x7FF8000000000000.  A sample in front of a too-long
 *                half wave keeps its amplitude and phase and loses only its frequency.
 *   counts       per row and emitted block two int32: the long samples, the overlong samples (a superset).
 * With a horizon that holds every half wave the three float outputs are itd_instantaneous_batch_f64 of the concatenated rows bit
 * for bit, length is itd_waves_batch_*'s length repeated over each half wave, and both counts are 0.
 * Latency and locality are the spectrum stream's: D = ceil((H + 1) / L) blocks (itd_inst_stream_latency; -1 if s is not an
 * instantaneous stream); block b is decided from the samples [b L - H, (b+1) L + H] that exist and from nothing else.  Push p
 * (counted from 0) emits block p - D when p >= D; every flush emits the next block still held, then emitted = 0 and the stream
 * starts afresh.  A push between flushes is refused.
 *   8 <= block <= 4096 (any value, no multiple of 64 is asked for), 1 <= rows <= 65535, 1 <= horizon <= 2^22.  Everything is
 *   allocated at create: the rings (rows (2 D + 1) block 8 bytes), one 16-byte record per block in them, the host forms' staging
 *   and an engine of the stream's own; ITD_ERR_NOMEM when it does not fit.  ITD_ERR_INVALID_ARG before any HIP call for a NULL
 *   handle, a NULL required pointer or a value out of range.  A call that fails leaves the stream as it was.
 *   block_dev: row r's block at block_dev + r in_stride (in_stride >= block when rows > 1) — the dense [channels][M+1][block] rows of
 *     itd_levels_stream_push_f64 go in as channels (M+1) rows with in_stride = block.
 *   amp_dev, phase_dev, freq_dev (float64), length_dev (int32): each optional, a NULL one is skipped; row r's block at
 *     + r out_stride (one stride for the four, >= block when rows > 1).  At least one is required whenever the call emits; they
 *     are written only then.
 *   counts_dev: optional; row r's two counts at counts_dev + r counts_stride (>= 2 when rows > 1).
 * Device forms: one launch per call on `stream`, no host synchronisation, no host read; *emitted follows from the block count alone.
 * Host forms: contiguous [rows][block] in and out, counts_host [rows][2]; each output optional, at least one required on every
 * call; pinned staging, one synchronisation per call.  A NaN in any pushed block sets bit 2 of itd_stream_status until
 * itd_stream_reset; that row is unspecified from then on, nothing outside the row's own slots is written.  itd_stream_destroy /
 * reset / blocks / status / last_error apply; every other stream kind's push and flush entries refuse an instantaneous stream,
 * and these refuse theirs. */
#define ITD_STREAM_INSTANT 5  /* an instantaneous stream (itd_inst_stream_create); not a kind itd_stream_create takes */
int itd_inst_stream_create(itd_stream **out, int device_id, int64_t block, int32_t rows, int64_t horizon);
int itd_inst_stream_latency(const itd_stream *s);
int itd_inst_stream_push_f64(itd_stream *s, const double *block_dev, int64_t in_stride, double *amp_dev, double *phase_dev,
                             double *freq_dev, int32_t *length_dev, int64_t out_stride, int32_t *counts_dev, int64_t counts_stride,
                             int32_t *emitted, void *stream);
int itd_inst_stream_flush_f64(itd_stream *s, double *amp_dev, double *phase_dev, double *freq_dev, int32_t *length_dev,
                              int64_t out_stride, int32_t *counts_dev, int64_t counts_stride, int32_t *emitted, void *stream);
int itd_inst_stream_push_host_f64(itd_stream *s, const double *block_host, double *amp_host, double *phase_host, double *freq_host,
                                  int32_t *length_host, int32_t *counts_host, int32_t *emitted);
int itd_inst_stream_flush_host_f64(itd_stream *s, double *amp_host, double *phase_host, double *freq_host, int32_t *length_host,
                                   int32_t *counts_host, int32_t *emitted);

/* ---- the histogram stream: the half waves' joint amplitude-length histogram block by block, at a fixed latency (DESIGN.md
 *      section 25) -----------------------------------------------------------------------------------------------------------------
 * itd_wave_hist_batch_* needs the whole row.  A histogram stream takes blocks of `rows` rows in lock step and gives finished time
 * slices of their histograms a known number of blocks later: the distribution a live wave-filter stream's bounds follow.  With
 * blocks of L samples, a horizon of H samples and hop | L (C = L / hop cells per block), row r after P pushes is x[0 .. P L).
 * Crossing indices, half waves, length_k, A_k and peak_k (the smallest index with |x| == A_k) are itd_waves_batch_*'s on the indices
 * of the whole stream; the last half wave ends at the flushed stream's last sample.  ae[0 .. na], le[0 .. nl]: the edges of
 * itd_wave_hist_batch_*, with its comparisons.
 *   length_k <= H   half wave k is counted exactly once, in absolute time bin peak_k / hop: where both its bins exist
 *                   count[t][i][j] += 1 and samples[t][i][j] += length_k, otherwise outside[t] += 1.
 *   length_k >  H   it is in none of the three; each of its samples j adds 1 to overlong[j / hop] — the price of the bounded latency.
 *   emitted block b   the cells b C .. (b+1) C - 1: count[C][na][nl], samples[C][na][nl], outside[C], overlong[C], all int32.  Every
 *                   cell is written, an empty one as 0; gaps beyond the dense extent of a row's slot are not written.  No overflow:
 *                   samples <= hop + 2 (H - 1).  Where no half wave is longer than H the concatenated slices are
 *                   itd_wave_hist_batch_f64(concatenated rows, ae, le, hop) integer for integer (that call wants hop to be a
 *                   multiple of 512; the definition holds for every hop) and overlong is all 0.
 * Latency D = ceil(H / L) blocks (itd_hist_stream_latency; -1 if s is not a histogram stream), the wave-filter stream's.  Block b is
 * decided from the samples [b L - H, (b+1) L + H) that exist and from nothing else: a half wave that touches the block, with the
 * maxima ML left of it, MB inside it and MR right of it, has its peak in the block iff its part of the block is non-empty, it begins
 * in the block or ML < MB (the earlier index wins a tie), and MR <= MB.  Push p (counted from 0) emits block p - D when p >= D; every
 * flush emits the next block still held, then emitted = 0 and the stream starts afresh.  A push between flushes is refused.
 *   64 <= block <= 4096, hop a positive multiple of 64 that divides block, 1 <= rows <= 65535, 1 <= horizon <= 2^22,
 *   1 <= na, nl <= 64, na nl <= 1024 and C na nl <= 8192 (the block's histogram is held in LDS).  Everything is allocated at create:
 *   the rings (rows (2 D + 1) block 8 bytes), one 16-byte record per block in them, the host forms' staging and an engine of the
 *   stream's own; ITD_ERR_NOMEM when it does not fit.  ITD_ERR_INVALID_ARG before any HIP call for a NULL handle, a NULL required
 *   pointer or a value out of range.  A call that fails leaves the stream as it was.
 *   block_dev: row r's block at block_dev + r in_stride (in_stride >= block when rows > 1).
 *   aedges_dev, ledges_dev: row r's edges at + r aedges_stride / ledges_stride; a stride is 0 (one set for every row) or >= na + 1 /
 *     >= nl + 1; device memory, read when the launch runs (strictly increasing, no NaN, +-inf allowed at the ends: the caller's duty);
 *     a caller may move them between pushes; required whenever the call emits.
 *   count_dev, samples_dev: row r's cells at + r hist_stride (one stride for the two, >= C na nl when rows > 1); required whenever
 *     the call emits, written only then.
 *   outside_dev, overlong_dev: optional; row r's counts at + r count_stride (>= C when rows > 1).
 * Device forms: one launch per call on `stream`, no host synchronisation, no host read; *emitted follows from the block count alone.
 * Host forms: contiguous [rows][block] in, [rows][C][na][nl] and [rows][C] out (outside_host and overlong_host optional), the edges
 * with their strides as above; pinned staging, one synchronisation per call.  A NaN in any pushed block sets bit 2 of
 * itd_stream_status until itd_stream_reset; that row is unspecified from then on, nothing outside the row's own slots is written.
 * itd_stream_destroy / reset / blocks / status / last_error apply; every other stream kind's push and flush entries refuse a
 * histogram stream, and these refuse theirs. */
#define ITD_STREAM_HIST 6     /* a histogram stream (itd_hist_stream_create); not a kind itd_stream_create takes */
int itd_hist_stream_create(itd_stream **out, int device_id, int64_t block, int32_t rows, int64_t horizon, int64_t hop, int32_t na,
                           int32_t nl);
int itd_hist_stream_latency(const itd_stream *s);
int itd_hist_stream_push_f64(itd_stream *s, const double *block_dev, int64_t in_stride, const double *aedges_dev, int64_t aedges_stride,
                             const double *ledges_dev, int64_t ledges_stride, int32_t *count_dev, int32_t *samples_dev,
                             int64_t hist_stride, int32_t *outside_dev, int32_t *overlong_dev, int64_t count_stride, int32_t *emitted,
                             void *stream);
int itd_hist_stream_flush_f64(itd_stream *s, const double *aedges_dev, int64_t aedges_stride, const double *ledges_dev,
                              int64_t ledges_stride, int32_t *count_dev, int32_t *samples_dev, int64_t hist_stride,
                              int32_t *outside_dev, int32_t *overlong_dev, int64_t count_stride, int32_t *emitted, void *stream);
int itd_hist_stream_push_host_f64(itd_stream *s, const double *block_host, const double *aedges_host, int64_t aedges_stride,
                                  const double *ledges_host, int64_t ledges_stride, int32_t *count_host, int32_t *samples_host,
                                  int32_t *outside_host, int32_t *overlong_host, int32_t *emitted);
int itd_hist_stream_flush_host_f64(itd_stream *s, const double *aedges_host, int64_t aedges_stride, const double *ledges_host,
                                   int64_t ledges_stride, int32_t *count_host, int32_t *samples_host, int32_t *outside_host,
                                   int32_t *overlong_host, int32_t *emitted);

/* ---- the table stream: the half-wave table block by block, no horizon and no latency ----------------------
 * itd_waves_batch_* needs the whole row; the ring streams above stop at a horizon.  A table stream takes blocks of `rows` rows in lock
 * step and gives every half wave — start, length, peak, signed extremum — in the push in which its end becomes known, whatever its
 * length: the events a real-time detector works on.  With blocks of L samples, row r after P pushes is x[0 .. P L); indices count
 * from the stream's first sample.
 *   crossing index i   i >= 1, x[i + 1] exists, and the sign changes strictly between x[i] and x[i + 1] (x[i] > 0 > x[i + 1] or
 *                   x[i] < 0 < x[i + 1]; a zero in between is no crossing): itd_waves_batch_*'s on the concatenated row.
 *   half wave k     start_k, length_k, A_k, peak_k (the smallest index with |x| == A_k), value_k = x[peak_k] with its sign bit:
 *                   itd_waves_batch_*'s.  It is complete when its last sample c_k is a known crossing index: when sample c_k + 1
 *                   has been pushed.
 *   push p          (counted from 0) brings the samples [p L, (p+1) L), decides exactly the crossing indices max(1, p L - 1) ..
 *                   (p+1) L - 2 and emits the half waves that end there, in order: at most L - 2 events per row in a stream's
 *                   first push, at most L in every later one.  Whether a block's last sample is a crossing index is decided by the
 *                   next push.
 *   flush           emits the one half wave still open, which ends at sample P L - 1; the stream then starts afresh.  A flush of an
 *                   empty stream emits nothing (emitted = 0) and writes nothing.
 * The events of every push and of the flush, concatenated row by row, are itd_waves_batch_f64 of the concatenated row: positions
 * integer for integer, value bit for bit.  No horizon, no `overlong`: exact for half waves of any length.
 *   origin          every reported start and peak is origin + index (a recording's sample clock); the rule i >= 1 stays relative to
 *                   the stream's first sample.
 *   output          row r owns a slot of event_stride entries in each of four arrays: start, length, peak (int64), value
 *                   (float64); count[r] (int32) = the events of this step.  Entries [0, count) are the completed half waves.  After
 *                   a push entry `count` is the half wave still open: its start, its length so far, its peak and value so far.
 *                   After a flush count = 1, entry 0 is the final half wave and no open entry is written.  Nothing at or beyond
 *                   entry count + 1 of a slot (a flush: beyond entry 0) and nothing outside the slots is written.
 *   8 <= block <= 4096 (any value), 1 <= rows <= 65535, any origin.  Everything is allocated at create: 48 bytes per row for the
 *   open half wave, the status word, the host forms' staging and an engine of the stream's own; ITD_ERR_NOMEM when it does not
 *   fit.  ITD_ERR_INVALID_ARG before any HIP call for a NULL handle, a NULL required pointer, a value out of range or a stride that
 *   is too short.  A call that fails leaves the stream as it was.
 *   block_dev: row r's block at block_dev + r in_stride (in_stride >= block when rows > 1) — the dense [channels][M+1][block] rows of
 *     itd_levels_stream_push_f64 go in as channels (M+1) rows with in_stride = block.
 *   start_dev, length_dev, peak_dev (int64), value_dev (float64): each optional, a NULL one is skipped; row r's slot at
 *     + r event_stride (one stride for the four, >= block + 1 when rows > 1).
 *   count_dev: required, [rows] int32.
 * Device forms: one launch per call on `stream`, no host synchronisation, no host read; *emitted is 1 for every push and for a flush
 * of a stream that holds blocks, else 0: it follows from the block count alone.  Host forms: contiguous [rows][block] in,
 * [rows][block + 1] tables (each optional) and count_host [rows] (required) out; pinned staging, one synchronisation per call.  A NaN
 * in any pushed block sets bit 2 of itd_stream_status until itd_stream_reset; that row's entries are unspecified from then on (its
 * count stays within 0 .. block), nothing outside the row's own slots is written, other rows are unaffected.  itd_stream_destroy /
 * reset (back to block 0; the open half wave is dropped) / blocks (the blocks pushed since the stream began) / status / last_error
 * apply; every other stream kind's push and flush entries refuse a table stream, and these refuse theirs. */
#define ITD_STREAM_TABLE 7    /* a table stream (itd_table_stream_create); not a kind itd_stream_create takes */
int itd_table_stream_create(itd_stream **out, int device_id, int64_t block, int32_t rows, int64_t origin);
int itd_table_stream_push_f64(itd_stream *s, const double *block_dev, int64_t in_stride, int64_t *start_dev, int64_t *length_dev,
                              int64_t *peak_dev, double *value_dev, int64_t event_stride, int32_t *count_dev, int32_t *emitted,
                              void *stream);
int itd_table_stream_flush_f64(itd_stream *s, int64_t *start_dev, int64_t *length_dev, int64_t *peak_dev, double *value_dev,
                               int64_t event_stride, int32_t *count_dev, int32_t *emitted, void *stream);
int itd_table_stream_push_host_f64(itd_stream *s, const double *block_host, int64_t *start_host, int64_t *length_host,
                                   int64_t *peak_host, double *value_host, int32_t *count_host, int32_t *emitted);
int itd_table_stream_flush_host_f64(itd_stream *s, int64_t *start_host, int64_t *length_host, int64_t *peak_host, double *value_host,
                                    int32_t *count_host, int32_t *emitted);

/* ---- the bounds stream: the wave filter's bounds of a sliding window over a histogram stream's slices ------
 * itd_wave_bounds_batch needs the whole histogram.  A bounds stream takes, push by push, the `slices` = C time slices [C][na][nl]
 * that a histogram stream emits per block for each of `rows` rows, and after push p (counted from 0) writes the bounds of the last
 * min(W, p + 1) pushes: by definition itd_wave_bounds_batch over the concatenated slices with
 * [t0, t1) = [max(0, p + 1 - W) C, (p + 1) C), with the edges and the parameters of this push, bit for bit.  No latency, no flush.
 * One launch per push: it replaces the window's oldest push by the new one in a device ring of per-push marginals and int64 running
 * sums per row — exact integers — and finishes as the many-row call does.  The ring slot is a launch argument.
 * Built for this order per block, all on one HIP stream through device pointers: the histogram stream's push, this push, the
 * wave-filter stream's push with the same horizon and so the same latency — block p - D is then filtered with bounds that already
 * include its own half waves.
 *   1 <= rows <= 65535, 1 <= na, nl <= 64, na nl <= 1024, slices >= 1 with slices na nl <= 8192 (the histogram stream's limit),
 *   1 <= window <= 65536 pushes.  Everything is allocated at create: rows (window + 1) (na + nl) 8 bytes of sums, the host form's
 *   staging and an engine of the stream's own; ITD_ERR_NOMEM when it does not fit.
 *   hist_dev: row r's cells at + r hist_stride (>= slices na nl when rows > 1), `count` or `samples` as the caller chooses.
 *   edges, parameters, bounds, total: as for itd_wave_bounds_batch, read and written when the launch runs.
 * The host form takes contiguous hist_host [rows][slices][na][nl], edges and parameters with a stride of 0 (one set) or exactly
 * na + 1 / nl + 1 / 8, and gives bounds_host [rows][4] and total_host [rows] (optional); pinned staging, one synchronisation per call.
 * ITD_ERR_INVALID_ARG before any HIP call for a NULL handle, a NULL required pointer or a value out of range; a call that fails
 * leaves the stream as it was.  itd_stream_reset empties the window; itd_stream_destroy / blocks (the pushes since the stream
 * began) / status (always 0) / last_error apply; every other stream kind's push and flush entries refuse a bounds stream, and these
 * refuse theirs. */
#define ITD_STREAM_BOUNDS 8   /* a bounds stream (itd_bounds_stream_create); not a kind itd_stream_create takes */
int itd_bounds_stream_create(itd_stream **out, int device_id, int32_t rows, int32_t na, int32_t nl, int32_t slices, int32_t window);
int itd_bounds_stream_push(itd_stream *s, const int32_t *hist_dev, int64_t hist_stride, const double *aedges_dev, int64_t aedges_stride,
                           const double *ledges_dev, int64_t ledges_stride, const double *quant_dev, int64_t quant_stride,
                           double *bounds_dev, int64_t bounds_stride, int64_t *total_dev, void *stream);
int itd_bounds_stream_push_host(itd_stream *s, const int32_t *hist_host, const double *aedges_host, int64_t aedges_stride,
                                const double *ledges_host, int64_t ledges_stride, const double *quant_host, int64_t quant_stride,
                                double *bounds_host, int64_t *total_host);

/* ---- introspection for benchmarks -------------------------------------------------------------
 * hipEvent pairs on the launch stream.  Extraction launches are dispatched with their own start/stop events
 * (hipExtLaunchKernel: the events take the dispatch's own begin/end timestamps, so they agree with rocprofv3's kernel durations); the
 * whole-decomposition span uses two marker records.  itd_set_kernel_timing(e, K) enables recording for up to K
 * decompositions (K = 0 disables) and resets the tallies; itd_get_kernel_timing sums the elapsed time of every
 * recorded launch of class `which`. */
#define ITD_TIME_EXTRACT 0        /* k_extract<float64 in>: levels >= 1, the dominant kernel (24 B/sample) */
#define ITD_TIME_EXTRACT_L0 1     /* k_extract on the caller's signal (level 0; 20 B/sample for float32) */
#define ITD_TIME_EXTRACT_FINAL 2  /* k_extract of the "Out of time!" level (writes rotation+baseline only) */
#define ITD_TIME_DECOMPOSE 3      /* first launch .. last launch of one whole decomposition */
#define ITD_TIME_SCAN0 4          /* k_scan0: the level-0 knot scan of the caller's signal (4 B/sample for float32) */
#define ITD_TIME_KF_APPLY 5       /* k_kf_apply: the one pass over the samples for all fused levels (8 B read + 8 B per row written) */
#define ITD_TIME_KF_KNOTS 6       /* k_kf_knots: the knot side of the fused levels (hand-over and every level's step), one launch */
int itd_set_kernel_timing(itd_engine *e, int max_decompositions);
/* instrument only every stride-th decomposition (launches with events cost ~2 us more each, the span's marker records ~5 us each) */
int itd_set_kernel_timing_stride(itd_engine *e, int stride);
int itd_get_kernel_timing(itd_engine *e, int32_t which, double *ms_total, int32_t *launches);
/* the individual durations behind that sum (ms), in launch order: at most `cap` are written, *count = how many exist */
int itd_get_kernel_timing_samples(itd_engine *e, int32_t which, double *ms_out, int32_t cap, int32_t *count);
/* mode 1: only the level-0 launch of each decomposition carries events (one completion signal per step instead of one per launch);
 * itd_get_step_periods then gives the time from one decomposition's first launch to the next one's (ms): the per-step period of
 * back-to-back calls, from the dispatches' own timestamps.  mode 0 (default): every launch class. */
int itd_set_kernel_timing_mode(itd_engine *e, int32_t mode);
int itd_get_step_periods(itd_engine *e, double *ms_out, int32_t cap, int32_t *count);

#ifdef __cplusplus
}
#endif
#endif /* PYITD_HIP_H */
