// itd_engine_batch.inc — included at the end of itd_engine.hip (same translation unit: it uses the engine's internals).
//
//   * batched forms of the single-level operators, asynchronous and graph-capturable (no knot count crosses to the host):
//       itd_baseline_extract_batch_f64        ITD.py:79-121 over rows (siftED2D.ipynb cell 1 calls it row by row)
//       itd_detect_batch_f64                  ITD.py:33-76 / :87-98 / numba_accelerated_itd.py:17-59 / itd.cpp:161-168
//       itd_baseline_extract_cubic_batch_f64  itd_fourier_decomposition.py:49-122 with one retained knot list for every
//                                             channel (itd.cpp:40-44) or one list / the detected knots per signal
//       itd_instantaneous_batch_f64 / _f32    amplitude, phase and frequency of every row (itd_tfe_batch.hpp)
//       itd_tfe_spectrum_f64 / _f32           every row's energy binned over time and frequency (itd_tfe_spectrum.hpp)
//       itd_waves_batch_f64 / _f32            the table of every row's half waves (itd_waves.hpp)
//       itd_wave_filter_batch_f64 / _f32      every row filtered by its half waves' amplitude and length (itd_waves.hpp)
//       itd_wave_hist_batch_f64 / _f32        every row's half waves binned over amplitude, length and time (itd_wave_hist.hpp)
//   * block-wise operation (itd.cpp:31-38), itd_stream_*: a device-resident mirrored ring per channel (itd_stream.hpp), the
//     window's knots, their selection and the operator all on the device — a push enqueues launches and returns; the host form
//     synchronises once per push for its copies.  The recipe: include/pyitd_hip.h, DESIGN.md section 7.
//   * struct itd_stream, for the ring streams too (itd_wave_stream_*, itd_spectrum_stream_*, itd_inst_stream_*), whose host code is
//     in itd_ring_streams.inc, included behind this file.

namespace {

__global__ void k_info_from_totals(const int32_t *__restrict__ totals, int batch, int32_t *__restrict__ info)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch) info[b] = totals[2 * b + 1] ? -1 - totals[2 * b] : totals[2 * b];
}
__global__ void k_info_from_states(const SigState *__restrict__ st, int batch, int32_t *__restrict__ info, int32_t *__restrict__ status)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const int nan_in = st[b].in_nan;
    if (info) info[b] = nan_in ? -1 - st[b].m[0] : st[b].m[0];
    if (status && nan_in) atomicOr(status, 2);
}
__global__ void k_info_from_jobs(const CubicJob *__restrict__ jobs, int job_stride, int batch, int32_t *__restrict__ info)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const CubicJob j = jobs[(size_t)b * job_stride];
    info[b] = j.status == 0 ? j.idx : -j.status;
}

// one tier-1 extraction (ITD.py:79-121) of every signal of the batch: the record-driven level-0 pair (k_detect, k_extract with
// keep_nan: the baseline as computed, the NaN -> +inf write belongs to the driver's stop test).  status (optional): |= 2 when a
// signal holds a NaN (its results then follow the plain rules, not detect_peaks' NaN branch)
int extract_batch(itd_engine *e, const double *x, int64_t n, int32_t batch, int64_t x_stride, double *rot, int64_t rot_stride,
                  double *base, int64_t base_stride, int32_t *info, int32_t *status, hipStream_t st)
{
    const int chunk = std::min<int32_t>(batch, kMaxGridY);
    KnotWs w;   // counts / records of two levels, three group-sum buffers, the signals' states
    int rc = knot_workspace(e, e->d_bw, n, chunk, kWsExtract, w);
    if (rc) return rc;
    for (int b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = std::min(chunk, batch - b0);
        const double *xc = x + (int64_t)b0 * x_stride;
        // (group-sum buffers are laid out for `chunk` signals; a shorter last chunk uses the front of each)
        rc = knot_scan<double>(e, w, xc, x_stride, n, nb, (int)kKnots, kScanOnly, st);
        if (rc) return rc;
        extract_level0<double>(w, xc, x_stride, n, nb, rot + (int64_t)b0 * rot_stride, rot_stride, base + (int64_t)b0 * base_stride, base_stride, st);
        if (info || status) k_info_from_states<<<(nb + 255) / 256, 256, 0, st>>>(w.state, nb, info ? info + b0 : nullptr, status);
    }
    HIP_TRY(e, hipGetLastError());
    return ITD_OK;
}

// ---- the half-wave tile pipeline (itd_halfwave.hpp): the instantaneous step (itd_tfe_batch.hpp) and the single-wave analysis
//      (itd_waves.hpp).  Per chunk of rows a scan (records, carry) and a consumer, launches behind one another on the stream,
//      nothing read on the host.

// what every batched call of the family refuses (outs: the call has somewhere to write)
bool tile_args_ok(const itd_engine *e, const void *x, int64_t n, int32_t rows, int64_t x_stride, bool outs)
{
    return e && x && outs && n >= 3 && n < (int64_t)INT32_MAX - 65536 && rows >= 1 && (rows == 1 || x_stride >= n);
}
// ... and where it writes rows of float64 / float32 samples
bool tile_out_ok(int64_t n, int32_t rows, int64_t out_stride, int32_t out_f32)
{
    return (out_f32 == 0 || out_f32 == 1) && (rows == 1 || out_stride >= n);
}

// The pipeline's workspace in one of the engine's grow-only buffers, for chunk = min(rows, 65535) rows (the launches' grid.y):
// per tile a record and what the carry leaves for the tile's first (head) and last (tail) half wave.
template <typename Rec, typename Head, typename Tail>
struct TileWs {
    Rec *rec;
    Head *head;
    Tail *tail;
    int64_t tiles;
    int chunk;
};
using InstWs = TileWs<InstRec, double, double>;         // Ahead, Atail; in d_ib
using WaveWs = TileWs<WaveRec, WaveFwd, WaveBwd>;       // in d_wv (not d_ib: a captured instantaneous call stays valid)
template <typename Rec, typename Head, typename Tail>
int tile_workspace(itd_engine *e, Buf<void> &buf, int64_t n, int32_t rows, TileWs<Rec, Head, Tail> &w)
{
    w.tiles = (n + kTfeTile - 1) / kTfeTile;
    w.chunk = std::min<int32_t>(rows, kMaxGridY);
    const size_t per = (size_t)w.chunk * (size_t)w.tiles;
    const int rc = grow(e, buf, per * (sizeof(Rec) + sizeof(Head) + sizeof(Tail)));
    w.rec = (Rec *)(void *)buf;
    w.head = (Head *)(w.rec + per);
    w.tail = (Tail *)(w.head + per);
    return rc;
}

// f(b0, nb) for every chunk of rows; then what the launches left behind
template <typename F>
int for_row_chunks(itd_engine *e, int32_t rows, int chunk, F f)
{
    for (int b0 = 0; b0 < rows; b0 += chunk) f(b0, std::min(chunk, rows - b0));
    HIP_TRY(e, hipGetLastError());
    return ITD_OK;
}
// an optional array, `off` elements on
template <typename A>
A *at(A *p, int64_t off) { return p ? p + off : nullptr; }
// ... of float64 / float32 samples
void *at(void *p, int64_t off, int32_t f32) { return p ? (char *)p + (size_t)off * (f32 ? sizeof(float) : sizeof(double)) : nullptr; }

// records and carry of nb rows: Ahead / Atail of every tile, the rows' info words
template <typename Tin>
void inst_scan(const InstWs &w, const Tin *x, int64_t x_stride, int64_t n, int nb, int32_t *info, hipStream_t st)
{
    k_inst_records<Tin><<<dim3((unsigned)w.tiles, (unsigned)nb), kWave, 0, st>>>(x, x_stride, n, w.tiles, w.rec);
    if (w.tiles <= kInstCarrySmall) k_inst_carry<64><<<nb, 64, 0, st>>>(w.rec, w.tiles, w.head, w.tail, info);
    else k_inst_carry<kInstCarryThreads><<<nb, kInstCarryThreads, 0, st>>>(w.rec, w.tiles, w.head, w.tail, info);
}

template <typename Tin, typename Tout>
void inst_chunk(const InstWs &w, const Tin *x, int64_t x_stride, int64_t n, int nb, void *amp, void *phase, void *freq, int64_t out_stride,
                int32_t *info, hipStream_t st)
{
    inst_scan<Tin>(w, x, x_stride, n, nb, info, st);
    k_inst_apply<Tin, Tout><<<dim3((unsigned)w.tiles, (unsigned)nb), kWave, 0, st>>>(x, x_stride, n, w.tiles, w.head, w.tail, (Tout *)amp, (Tout *)phase,
                                                                                     (Tout *)freq, out_stride);
}

template <typename Tin>
int inst_batch(itd_engine *e, const Tin *x, int64_t n, int32_t rows, int64_t x_stride, void *amp, void *phase, void *freq,
               int64_t out_stride, int32_t out_f32, int32_t *info, void *stream)
{
    if (!tile_args_ok(e, x, n, rows, x_stride, amp || phase || freq) || !tile_out_ok(n, rows, out_stride, out_f32)) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    InstWs w;
    const int rc = tile_workspace(e, e->d_ib, n, rows, w);
    if (rc) return rc;
    return for_row_chunks(e, rows, w.chunk, [&](int b0, int nb) {
        const Tin *xc = x + (int64_t)b0 * x_stride;
        const int64_t off = (int64_t)b0 * out_stride;
        void *a = at(amp, off, out_f32), *p = at(phase, off, out_f32), *f = at(freq, off, out_f32);
        if (out_f32) inst_chunk<Tin, float>(w, xc, x_stride, n, nb, a, p, f, out_stride, at(info, b0), st);
        else inst_chunk<Tin, double>(w, xc, x_stride, n, nb, a, p, f, out_stride, at(info, b0), st);
    });
}

// The time-frequency-energy spectrum (itd_tfe_spectrum.hpp): the instantaneous step's scan in a workspace of its own (d_ts: a
// captured instantaneous call stays valid), then k_tfe_bin — one wavefront per (row, time bin), per (row, tile) where hop < 512.
template <typename Tin>
int tfe_spectrum(itd_engine *e, const Tin *x, int64_t n, int32_t rows, int64_t x_stride, const double *edges, int32_t bins, int64_t hop,
                 int32_t weight, double *spec, int64_t spec_stride, int32_t *outside, int32_t *info, void *stream)
{
    if (!tile_args_ok(e, x, n, rows, x_stride, edges && spec)) return ITD_ERR_INVALID_ARG;
    if (bins < 1 || bins > kTfeMaxBins || weight < 0 || weight > 2) return ITD_ERR_INVALID_ARG;
    if (hop < 64 || hop % 64 != 0 || (hop < kTfeTile && hop != 64 && hop != 128 && hop != 256)) return ITD_ERR_INVALID_ARG;
    const int64_t T = (n + hop - 1) / hop;
    if (rows > 1 && spec_stride < T * bins) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    InstWs w;
    const int rc = tile_workspace(e, e->d_ts, n, rows, w);
    if (rc) return rc;
    const size_t lds = (3 * (size_t)bins + 1) * sizeof(double);      // acc[bins], edges[bins + 1], msk[bins]
    return for_row_chunks(e, rows, w.chunk, [&](int b0, int nb) {
        const Tin *xc = x + (int64_t)b0 * x_stride;
        inst_scan<Tin>(w, xc, x_stride, n, nb, at(info, b0), st);
        const dim3 grid((unsigned)(hop >= kTfeTile ? T : w.tiles), (unsigned)nb);
        k_tfe_bin<Tin><<<grid, kWave, lds, st>>>(xc, x_stride, n, w.tiles, w.head, w.tail, edges, bins, hop, weight, T,
                                                 spec + (int64_t)b0 * spec_stride, spec_stride, at(outside, (int64_t)b0 * T));
    });
}

template <typename Tin>
void wave_scan(const WaveWs &w, const Tin *x, int64_t x_stride, int64_t n, int nb, int32_t *count, int32_t *info, hipStream_t st)
{
    k_wave_records<Tin><<<dim3((unsigned)w.tiles, (unsigned)nb), kWave, 0, st>>>(x, x_stride, n, w.tiles, w.rec);
    if (w.tiles <= kInstCarrySmall) k_wave_carry<64><<<nb, 64, 0, st>>>(w.rec, w.tiles, n, w.head, w.tail, count, info);
    else k_wave_carry<kInstCarryThreads><<<nb, kInstCarryThreads, 0, st>>>(w.rec, w.tiles, n, w.head, w.tail, count, info);
}

template <typename Tin>
int waves_batch(itd_engine *e, const Tin *x, int64_t n, int32_t rows, int64_t x_stride, int32_t *start, int32_t *length, int32_t *peak,
                double *value, int64_t wave_stride, int32_t cap, int32_t *count, int32_t *info, void *stream)
{
    const bool table = start || length || peak || value;
    if (!tile_args_ok(e, x, n, rows, x_stride, table || count)) return ITD_ERR_INVALID_ARG;
    if (table && (cap < 1 || (rows > 1 && wave_stride < cap))) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    WaveWs w;
    const int rc = tile_workspace(e, e->d_wv, n, rows, w);
    if (rc) return rc;
    return for_row_chunks(e, rows, w.chunk, [&](int b0, int nb) {
        const Tin *xc = x + (int64_t)b0 * x_stride;
        const int64_t off = (int64_t)b0 * wave_stride;
        wave_scan<Tin>(w, xc, x_stride, n, nb, at(count, b0), at(info, b0), st);
        if (table)
            k_wave_table<Tin><<<dim3((unsigned)w.tiles, (unsigned)nb), kWave, 0, st>>>(xc, x_stride, n, w.tiles, w.head, w.tail, at(start, off),
                                                                                      at(length, off), at(peak, off), at(value, off),
                                                                                      wave_stride, cap);
    });
}

template <typename Tin>
int wave_filter_batch(itd_engine *e, const Tin *x, int64_t n, int32_t rows, int64_t x_stride, const double *bounds, int64_t bounds_stride,
                      void *out, int64_t out_stride, int32_t out_f32, int32_t *info, void *stream)
{
    if (!tile_args_ok(e, x, n, rows, x_stride, bounds && out) || !tile_out_ok(n, rows, out_stride, out_f32)) return ITD_ERR_INVALID_ARG;
    if (bounds_stride != 0 && bounds_stride < 4) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    WaveWs w;
    const int rc = tile_workspace(e, e->d_wv, n, rows, w);
    if (rc) return rc;
    return for_row_chunks(e, rows, w.chunk, [&](int b0, int nb) {
        const Tin *xc = x + (int64_t)b0 * x_stride;
        const double *bc = bounds + (int64_t)b0 * bounds_stride;
        void *oc = at(out, (int64_t)b0 * out_stride, out_f32);
        const dim3 grid((unsigned)w.tiles, (unsigned)nb);
        wave_scan<Tin>(w, xc, x_stride, n, nb, nullptr, at(info, b0), st);
        if (out_f32) k_wave_filter<Tin, float><<<grid, kWave, 0, st>>>(xc, x_stride, n, w.tiles, w.head, w.tail, bc, bounds_stride, (float *)oc, out_stride);
        else k_wave_filter<Tin, double><<<grid, kWave, 0, st>>>(xc, x_stride, n, w.tiles, w.head, w.tail, bc, bounds_stride, (double *)oc, out_stride);
    });
}

// The joint amplitude-length histogram of the rows' half waves (itd_wave_hist.hpp): the rows' slots zeroed, the single-wave scan in
// its workspace (d_wv), then k_wave_hist in k_wave_table's place.
template <typename Tin>
int wave_hist_batch(itd_engine *e, const Tin *x, int64_t n, int32_t rows, int64_t x_stride, const double *aedges, int64_t aedges_stride,
                    int32_t abins, const double *ledges, int64_t ledges_stride, int32_t lbins, int64_t hop, int32_t *count, int32_t *samples,
                    int64_t hist_stride, int32_t *outside, int32_t *info, void *stream)
{
    if (!tile_args_ok(e, x, n, rows, x_stride, aedges && ledges && (count || samples))) return ITD_ERR_INVALID_ARG;
    if (abins < 1 || abins > kWaveHistMaxBins || lbins < 1 || lbins > kWaveHistMaxBins || abins * lbins > kWaveHistMaxCells) return ITD_ERR_INVALID_ARG;
    if (hop < kTfeTile || hop % kTfeTile != 0) return ITD_ERR_INVALID_ARG;
    if ((aedges_stride != 0 && aedges_stride < abins + 1) || (ledges_stride != 0 && ledges_stride < lbins + 1)) return ITD_ERR_INVALID_ARG;
    const int64_t T = (n + hop - 1) / hop, slot = T * abins * lbins;
    if (rows > 1 && hist_stride < slot) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    WaveWs w;
    const int rc = tile_workspace(e, e->d_wv, n, rows, w);
    if (rc) return rc;
    const size_t lds = wave_hist_lds(abins, lbins);
    return for_row_chunks(e, rows, w.chunk, [&](int b0, int nb) {
        const Tin *xc = x + (int64_t)b0 * x_stride;
        int32_t *cc = at(count, (int64_t)b0 * hist_stride), *sc = at(samples, (int64_t)b0 * hist_stride), *oc = at(outside, (int64_t)b0 * T);
        k_wave_hist_zero<<<dim3((unsigned)((slot + kWaveHistZeroThreads - 1) / kWaveHistZeroThreads), (unsigned)nb), kWaveHistZeroThreads, 0, st>>>(
            cc, sc, hist_stride, slot, oc, T);
        wave_scan<Tin>(w, xc, x_stride, n, nb, nullptr, at(info, b0), st);
        k_wave_hist<Tin><<<dim3((unsigned)w.tiles, (unsigned)nb), kWave, lds, st>>>(xc, x_stride, n, w.tiles, w.head, w.tail,
                                                                                   aedges + (int64_t)b0 * aedges_stride, aedges_stride, abins,
                                                                                   ledges + (int64_t)b0 * ledges_stride, ledges_stride, lbins,
                                                                                   hop, T, cc, sc, hist_stride, oc);
    });
}

}  // namespace

struct itd_stream {
    itd_engine *eng = nullptr;
    int64_t L = 0;
    int32_t C = 1, kind = ITD_STREAM_CUBIC, margin = 8, shared = 0;
    int64_t pushed = 0;             // blocks stored since create / reset / flush
    Buf<double> ring;               // [C][5 L]
    Buf<double> scr;                // tier-1: rotation and baseline of the window, [2][C][3 L]
    Buf<CubicJob> jobs;             // cubic: [C]
    Buf<double> arr;                // cubic: K, bf, b, [3][C][3 L + 2]
    Buf<int32_t> d_status;          // sticky: |= 2 when a window held a NaN
    Pinned<double> h_in, h_out;     // pinned staging of the host form: [C][L], [2][C][L]
    Buf<double> d_in, d_out;        // device staging of the host form
    // levels stream (ITD_STREAM_LEVELS, k_stream_levels in itd_stream.hpp): ring = [C][M+1][5 L]
    int32_t M = 0, cw = 0, threads = 0;
    int32_t seq = 0;                // 1: the launch-sequence form (blocks above 2730 samples, or itd_levels_stream_set_sequence)
    int64_t t = 0, P = -1;          // the next step; the blocks in all once flushing began (-1: pushing)
    Buf<double> delay;              // [C][M (M+1) / 2][L]
    Buf<uint8_t> eflags;            // [C][M+1][4]
    Buf<uint8_t> d_exact; Pinned<uint8_t> h_exact;   // host form: [C]
    size_t lds = 0;
    const void *fn = nullptr;
    // the ring streams (ITD_STREAM_WAVES, _SPECTRUM, _INSTANT, _HIST; itd_ring_streams.inc): C rows, ring = [C][2 D + 1][L]; they use L, C,
    // kind, ring, d_status, threads, lds, fn and the staging d_in / h_in, d_out / h_out above, and besides
    struct Ring {
        RingCount cnt = kRingCountFresh;                 // blocks pushed, in all, emitted (itd_ring_plan.hpp)
        int64_t H = 0;                                   // the horizon
        int32_t D = 0;                                   // the latency in blocks, ceil((H + the kind's reach) / L)
        Buf<WaveBlockRec> rec;                           // [C][2 D + 1]: what every block in the ring left behind when it arrived
        int32_t F = 0, weight = 0;                       // spectrum: bins; 0 count, 1 amplitude, 2 energy
        int64_t hop = 0;                                 // spectrum, histogram
        int32_t Na = 0, Nl = 0;                          // histogram: bins per axis (F = the cells of a block, L / hop Na Nl)
        // host form, besides d_in / h_in = [C][L] and d_out / h_out: a kind's float64 parameters and int32 results; what each kind
        // keeps where is stated next to its host form (wave_staging, spectrum_staging, inst_staging)
        Buf<double> d_bnd; Pinned<double> h_bnd;
        Buf<int32_t> d_cnt; Pinned<int32_t> h_cnt;
    } rs;
    // the table stream (ITD_STREAM_TABLE; itd_table_stream.inc): C rows, no ring; it uses L, C, kind, d_status, threads, lds, fn, the
    // staging d_in / h_in, d_out / h_out, rs.d_cnt / h_cnt, rs.cnt.t (the blocks pushed) and besides
    struct Table {
        int64_t origin = 0;                              // added to every position that is reported
        Buf<TableCarry> carry;                           // [C]: the half wave that is open between two pushes
    } tb;
    // the bounds stream (ITD_STREAM_BOUNDS; itd_wave_bounds.inc): C rows, rs.Na x rs.Nl bins, rs.F cells per push; it uses kind,
    // d_status, rs.cnt.t (the pushes) and besides
    struct Bounds {
        int32_t slices = 0, W = 0;                       // time slices per push; the window in pushes
        Buf<unsigned long long> ring, run;               // [C][W][Na + Nl] the window's pushes' marginals; [C][Na + Nl] their sums
        Buf<int32_t> d_hist; Pinned<int32_t> h_hist;     // host form: [C][F]
        Buf<double> d_par; Pinned<double> h_par;         // host form: ae [C][Na + 1], le [C][Nl + 1], q [C][8], bounds [C][4], total [C] (int64)
    } bd;
};

namespace {

// baseline (and rotation) of the samples [lo, hi) of the window [w0, w0 + wl) of every channel's ring
int stream_emit(itd_stream *s, int64_t w0, int64_t wl, int64_t lo, int64_t hi, double *base, int64_t base_stride, double *rot,
                int64_t rot_stride, hipStream_t st)
{
    itd_engine *e = s->eng;
    const int64_t ring_stride = 5 * s->L;
    const double *win = s->ring + w0;
    const int C = s->C;
    if (s->kind == ITD_STREAM_LINEAR) {
        double *rw = s->scr, *bw = s->scr + (int64_t)C * 3 * s->L;
        const int rc = extract_batch(e, win, wl, C, ring_stride, rw, 3 * s->L, bw, 3 * s->L, nullptr, s->d_status, st);
        if (rc) return rc;
        k_stream_emit2<<<dim3((unsigned)((s->L + 255) / 256), C), 256, 0, st>>>(rw, bw, 3 * s->L, lo, hi - lo, rot, rot_stride, base, base_stride);
        HIP_TRY(e, hipGetLastError());
        return ITD_OK;
    }
    // the window's extrema (itd.cpp:33 "re-assess extrema in the entire buffer every iteration"): channel 0's for everybody
    // (itd.cpp:40-44) or every channel's own
    const int n_lists = s->shared ? 1 : C;
    KnotWs w;
    int rc = knot_workspace(e, e->d_dw, wl, n_lists, kWsDetect, w);
    if (!rc) rc = knot_scan<double>(e, w, win, ring_stride, wl, n_lists, (int)kCpp, kScanOrdered, st, 0);
    if (rc) return rc;
    k_stream_select<<<(n_lists + 63) / 64, 64, 0, st>>>(w.kidx, w.kidx_stride, w.totals, n_lists, (int)lo, (int)hi, s->margin, s->jobs, s->d_status);
    CubicArgs A;
    const int64_t La = 3 * s->L + 2;
    A.x = win; A.x_stride = ring_stride; A.n = wl;
    A.e = w.kidx; A.e_stride = s->shared ? 0 : w.kidx_stride;
    A.jobs = s->jobs; A.job_stride = s->shared ? 0 : 1;
    A.tbase = w.tbase; A.tb_stride = s->shared ? 0 : w.n_tiles;
    A.K = s->arr; A.bf = s->arr + (int64_t)C * La; A.b = s->arr + 2 * (int64_t)C * La; A.a_stride = La;
    const unsigned nblk = (unsigned)std::max<int64_t>(1, (wl + kScanBlockElems - 1) / kScanBlockElems);
    k_cubic_sweep<true><<<dim3(nblk, C), kScanThreads, 0, st>>>(A);
    k_cubic_sweep<false><<<dim3(nblk, C), kScanThreads, 0, st>>>(A);
    k_cubic_eval<T><<<dim3((unsigned)tiles_of(hi - lo), C), kWave, 0, st>>>(A, lo, hi, base, base_stride, 1, rot, rot_stride);
    HIP_TRY(e, hipGetLastError());
    return ITD_OK;
}

int stream_push(itd_stream *s, const double *blk, int64_t in_stride, double *base, int64_t base_stride, double *rot,
                int64_t rot_stride, int32_t *emitted, hipStream_t st)
{
    const int64_t L = s->L;
    k_stream_store<<<dim3((unsigned)((L + 255) / 256), s->C), 256, 0, st>>>(blk, in_stride, s->ring, 5 * L, L, (int)(s->pushed % 3), s->d_status);
    ++s->pushed;
    if (emitted) *emitted = s->pushed >= 2 ? 1 : 0;
    if (s->pushed < 2) { HIP_TRY(s->eng, hipGetLastError()); return ITD_OK; }
    const int64_t j = s->pushed - 2;                    // the block that now has a successor
    if (j == 0) return stream_emit(s, 0, 2 * L, 0, L, base, base_stride, rot, rot_stride, st);   // no predecessor
    return stream_emit(s, ((j - 1) % 3) * L, 3 * L, L, 2 * L, base, base_stride, rot, rot_stride, st);
}

int stream_flush(itd_stream *s, double *base, int64_t base_stride, double *rot, int64_t rot_stride, int32_t *emitted, hipStream_t st)
{
    const int64_t L = s->L, P = s->pushed;
    if (emitted) *emitted = P >= 1 ? 1 : 0;
    s->pushed = 0;
    if (P == 0) return ITD_OK;
    if (P == 1) return stream_emit(s, 0, L, 0, L, base, base_stride, rot, rot_stride, st);        // one block in all
    return stream_emit(s, ((P - 2) % 3) * L, 2 * L, L, 2 * L, base, base_stride, rot, rot_stride, st);   // no successor
}

}  // namespace

extern "C" {

int itd_baseline_extract_batch_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride, double *rot_dev,
                                   int64_t rot_stride, double *base_dev, int64_t base_stride, int32_t *info_dev, void *stream)
{
    if (!e || !x_dev || !rot_dev || !base_dev) return ITD_ERR_INVALID_ARG;
    if (n < 3 || n >= (int64_t)INT32_MAX - 65536 || batch < 1) return ITD_ERR_INVALID_ARG;
    if (batch > 1 && (x_stride < n || rot_stride < n || base_stride < n)) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    return extract_batch(e, x_dev, n, batch, x_stride, rot_dev, rot_stride, base_dev, base_stride, info_dev, nullptr, stream_of(e, stream));
}

int itd_detect_batch_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride, int32_t mode, int32_t *idx_dev,
                         int64_t idx_stride, int32_t *info_dev, void *stream)
{
    if (!e || !x_dev || (!idx_dev && !info_dev)) return ITD_ERR_INVALID_ARG;
    if (n < 3 || n >= (int64_t)INT32_MAX - 65536 || batch < 1 || batch > kMaxGridY || mode < 0 || mode > 4) return ITD_ERR_INVALID_ARG;
    if (batch > 1 && (x_stride < n || (idx_dev && idx_stride < n - 2))) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    KnotWs w;
    int rc = knot_workspace(e, e->d_dw, n, batch, kWsDetect, w);
    if (!rc) rc = knot_scan<double>(e, w, x_dev, x_stride, n, batch, mode, idx_dev ? kScanOrdered : kScanTotals, st, -1, false, nullptr, idx_dev, idx_stride);
    if (rc) return rc;
    if (info_dev) k_info_from_totals<<<(batch + 255) / 256, 256, 0, st>>>(w.totals, batch, info_dev);
    HIP_TRY(e, hipGetLastError());
    return ITD_OK;
}

int itd_baseline_extract_cubic_batch_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride,
                                         const int32_t *extrema_dev, int64_t extrema_stride, int64_t idx, double *baseline_dev,
                                         int64_t baseline_stride, int32_t *info_dev, void *stream)
{
    if (!e || !x_dev || !baseline_dev) return ITD_ERR_INVALID_ARG;
    if (n < 3 || n >= (int64_t)INT32_MAX - 65536 || batch < 1 || batch > kMaxGridY) return ITD_ERR_INVALID_ARG;
    if (batch > 1 && (x_stride < n || baseline_stride < n)) return ITD_ERR_INVALID_ARG;
    if (extrema_dev && (idx < 2 || idx > n - 1 || (extrema_stride != 0 && extrema_stride < idx + 1))) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    const CubicJob *jobs = nullptr;
    int n_jobs = 0;
    const int rc = cubic_batch(e, x_dev, n, batch, x_stride, extrema_dev, extrema_stride, idx, baseline_dev, baseline_stride, st, &jobs, &n_jobs);
    if (rc) return rc;
    if (info_dev) k_info_from_jobs<<<(batch + 255) / 256, 256, 0, st>>>(jobs, n_jobs == batch ? 1 : 0, batch, info_dev);
    HIP_TRY(e, hipGetLastError());
    return ITD_OK;
}

int itd_instantaneous_batch_f64(itd_engine *e, const double *rows_dev, int64_t n, int32_t rows, int64_t row_stride, void *amp_dev,
                                void *phase_dev, void *freq_dev, int64_t out_stride, int32_t out_f32, int32_t *info_dev, void *stream)
{
    return inst_batch<double>(e, rows_dev, n, rows, row_stride, amp_dev, phase_dev, freq_dev, out_stride, out_f32, info_dev, stream);
}
int itd_instantaneous_batch_f32(itd_engine *e, const float *rows_dev, int64_t n, int32_t rows, int64_t row_stride, void *amp_dev,
                                void *phase_dev, void *freq_dev, int64_t out_stride, int32_t out_f32, int32_t *info_dev, void *stream)
{
    return inst_batch<float>(e, rows_dev, n, rows, row_stride, amp_dev, phase_dev, freq_dev, out_stride, out_f32, info_dev, stream);
}

int itd_tfe_spectrum_f64(itd_engine *e, const double *rows_dev, int64_t n, int32_t rows, int64_t row_stride, const double *edges_dev,
                         int32_t bins, int64_t hop, int32_t weight, double *spec_dev, int64_t spec_stride, int32_t *outside_dev,
                         int32_t *info_dev, void *stream)
{
    return tfe_spectrum<double>(e, rows_dev, n, rows, row_stride, edges_dev, bins, hop, weight, spec_dev, spec_stride, outside_dev, info_dev, stream);
}
int itd_tfe_spectrum_f32(itd_engine *e, const float *rows_dev, int64_t n, int32_t rows, int64_t row_stride, const double *edges_dev,
                         int32_t bins, int64_t hop, int32_t weight, double *spec_dev, int64_t spec_stride, int32_t *outside_dev,
                         int32_t *info_dev, void *stream)
{
    return tfe_spectrum<float>(e, rows_dev, n, rows, row_stride, edges_dev, bins, hop, weight, spec_dev, spec_stride, outside_dev, info_dev, stream);
}

int itd_waves_batch_f64(itd_engine *e, const double *rows_dev, int64_t n, int32_t rows, int64_t row_stride, int32_t *start_dev,
                        int32_t *length_dev, int32_t *peak_dev, double *value_dev, int64_t wave_stride, int32_t cap, int32_t *count_dev,
                        int32_t *info_dev, void *stream)
{
    return waves_batch<double>(e, rows_dev, n, rows, row_stride, start_dev, length_dev, peak_dev, value_dev, wave_stride, cap, count_dev,
                               info_dev, stream);
}
int itd_waves_batch_f32(itd_engine *e, const float *rows_dev, int64_t n, int32_t rows, int64_t row_stride, int32_t *start_dev,
                        int32_t *length_dev, int32_t *peak_dev, double *value_dev, int64_t wave_stride, int32_t cap, int32_t *count_dev,
                        int32_t *info_dev, void *stream)
{
    return waves_batch<float>(e, rows_dev, n, rows, row_stride, start_dev, length_dev, peak_dev, value_dev, wave_stride, cap, count_dev,
                              info_dev, stream);
}
int itd_wave_filter_batch_f64(itd_engine *e, const double *rows_dev, int64_t n, int32_t rows, int64_t row_stride, const double *bounds_dev,
                              int64_t bounds_stride, void *out_dev, int64_t out_stride, int32_t out_f32, int32_t *info_dev, void *stream)
{
    return wave_filter_batch<double>(e, rows_dev, n, rows, row_stride, bounds_dev, bounds_stride, out_dev, out_stride, out_f32, info_dev, stream);
}
int itd_wave_filter_batch_f32(itd_engine *e, const float *rows_dev, int64_t n, int32_t rows, int64_t row_stride, const double *bounds_dev,
                              int64_t bounds_stride, void *out_dev, int64_t out_stride, int32_t out_f32, int32_t *info_dev, void *stream)
{
    return wave_filter_batch<float>(e, rows_dev, n, rows, row_stride, bounds_dev, bounds_stride, out_dev, out_stride, out_f32, info_dev, stream);
}

int itd_wave_hist_batch_f64(itd_engine *e, const double *rows_dev, int64_t n, int32_t rows, int64_t row_stride, const double *aedges_dev,
                            int64_t aedges_stride, int32_t abins, const double *ledges_dev, int64_t ledges_stride, int32_t lbins,
                            int64_t hop, int32_t *count_dev, int32_t *samples_dev, int64_t hist_stride, int32_t *outside_dev,
                            int32_t *info_dev, void *stream)
{
    return wave_hist_batch<double>(e, rows_dev, n, rows, row_stride, aedges_dev, aedges_stride, abins, ledges_dev, ledges_stride, lbins, hop,
                                   count_dev, samples_dev, hist_stride, outside_dev, info_dev, stream);
}
int itd_wave_hist_batch_f32(itd_engine *e, const float *rows_dev, int64_t n, int32_t rows, int64_t row_stride, const double *aedges_dev,
                            int64_t aedges_stride, int32_t abins, const double *ledges_dev, int64_t ledges_stride, int32_t lbins,
                            int64_t hop, int32_t *count_dev, int32_t *samples_dev, int64_t hist_stride, int32_t *outside_dev,
                            int32_t *info_dev, void *stream)
{
    return wave_hist_batch<float>(e, rows_dev, n, rows, row_stride, aedges_dev, aedges_stride, abins, ledges_dev, ledges_stride, lbins, hop,
                                  count_dev, samples_dev, hist_stride, outside_dev, info_dev, stream);
}

int itd_stream_create(itd_stream **out, int device_id, int64_t block, int32_t channels, int32_t kind, int32_t margin, int32_t shared_knots)
{
    if (!out) return ITD_ERR_INVALID_ARG;
    *out = nullptr;
    if (block < 8 || 3 * block >= (int64_t)INT32_MAX - 65536 || channels < 1 || channels > kMaxGridY) return ITD_ERR_INVALID_ARG;
    if (kind != ITD_STREAM_CUBIC && kind != ITD_STREAM_LINEAR) return ITD_ERR_INVALID_ARG;
    if (kind == ITD_STREAM_CUBIC && margin < 1) return ITD_ERR_INVALID_ARG;
    if (kind == ITD_STREAM_LINEAR && shared_knots) return ITD_ERR_INVALID_ARG;   // the tier-1 knots are the signal's own by definition
    itd_stream *s = new (std::nothrow) itd_stream();
    if (!s) return ITD_ERR_NOMEM;
    int rc = itd_engine_create(&s->eng, device_id, 3 * block, 1);
    if (rc) { delete s; return rc; }
    s->L = block; s->C = channels; s->kind = kind; s->margin = margin; s->shared = shared_knots ? 1 : 0;
    DevGuard g(device_id);
    const size_t C = (size_t)channels, L = (size_t)block;
    hipError_t hrc = s->ring.alloc(C * 5 * L * sizeof(double));
    if (hrc == hipSuccess) hrc = hipMemset(s->ring, 0, C * 5 * L * sizeof(double));
    if (hrc == hipSuccess && kind == ITD_STREAM_LINEAR) hrc = s->scr.alloc(2 * C * 3 * L * sizeof(double));
    if (hrc == hipSuccess && kind == ITD_STREAM_CUBIC) hrc = s->jobs.alloc(C * sizeof(CubicJob));
    if (hrc == hipSuccess && kind == ITD_STREAM_CUBIC) hrc = s->arr.alloc(3 * C * (3 * L + 2) * sizeof(double));
    if (hrc == hipSuccess) hrc = s->d_status.alloc(64);
    if (hrc == hipSuccess) hrc = hipMemset(s->d_status, 0, 64);
    if (hrc == hipSuccess) hrc = hipDeviceSynchronize();     // (the fills ran on the null stream, the stream's launches use a non-blocking one)
    if (hrc != hipSuccess) {
        const bool oom = hrc == hipErrorOutOfMemory;
        itd_stream_destroy(s);
        return oom ? ITD_ERR_NOMEM : ITD_ERR_HIP;
    }
    *out = s;
    return ITD_OK;
}

void itd_stream_destroy(itd_stream *s)
{
    if (!s) return;
    itd_engine *const e = s->eng;   // (never null: a stream whose engine could not be created does not get here)
    DevGuard g(e->device);
    (void)hipStreamSynchronize(e->own_stream);
    delete s;                       // the stream's buffers go before its engine does
    itd_engine_destroy(e);
}

int itd_stream_reset(itd_stream *s)
{
    if (!s) return ITD_ERR_INVALID_ARG;
    DevGuard g(s->eng->device);
    s->pushed = 0;
    s->t = 0;
    s->P = -1;
    s->rs.cnt = kRingCountFresh;
    HIP_TRY(s->eng, hipMemsetAsync(s->d_status, 0, sizeof(int32_t), s->eng->own_stream));
    HIP_TRY(s->eng, hipStreamSynchronize(s->eng->own_stream));
    return ITD_OK;
}

int64_t itd_stream_blocks(const itd_stream *s)
{
    if (!s) return -1;
    // (the ring streams: wave filter, spectrum, instantaneous, histogram; the table stream emits nothing late: what it pushed)
    if (s->kind >= ITD_STREAM_WAVES) return ring_held(s->rs.cnt);
    if (s->kind != ITD_STREAM_LEVELS) return s->pushed;
    return (s->P < 0 ? s->t : s->P) - std::max<int64_t>(0, s->t - s->M - 1);   // pushed, less the blocks whose rows have left
}
const char *itd_stream_last_error(const itd_stream *s) { return s && s->eng ? s->eng->err : "null stream"; }

int itd_stream_push_f64(itd_stream *s, const double *block_dev, int64_t in_stride, double *baseline_dev, int64_t baseline_stride,
                        double *rot_dev, int64_t rot_stride, int32_t *emitted, void *stream)
{
    if (!s || !block_dev || s->kind >= ITD_STREAM_LEVELS) return ITD_ERR_INVALID_ARG;   // (a levels stream and every ring stream: their own entries)
    if (s->C > 1 && (in_stride < s->L || (baseline_dev && baseline_stride < s->L) || (rot_dev && rot_stride < s->L))) return ITD_ERR_INVALID_ARG;
    if (s->pushed >= 1 && !baseline_dev) return ITD_ERR_INVALID_ARG;      // this push emits a block
    DevGuard g(s->eng->device);
    return stream_push(s, block_dev, in_stride, baseline_dev, baseline_stride, rot_dev, rot_stride, emitted, stream_of(s->eng, stream));
}

int itd_stream_flush_f64(itd_stream *s, double *baseline_dev, int64_t baseline_stride, double *rot_dev, int64_t rot_stride,
                         int32_t *emitted, void *stream)
{
    if (!s || s->kind >= ITD_STREAM_LEVELS) return ITD_ERR_INVALID_ARG;
    if (s->pushed >= 1 && !baseline_dev) return ITD_ERR_INVALID_ARG;
    if (s->C > 1 && ((baseline_dev && baseline_stride < s->L) || (rot_dev && rot_stride < s->L))) return ITD_ERR_INVALID_ARG;
    DevGuard g(s->eng->device);
    return stream_flush(s, baseline_dev, baseline_stride, rot_dev, rot_stride, emitted, stream_of(s->eng, stream));
}

int itd_stream_status(itd_stream *s, int32_t *status)
{
    if (!s || !status) return ITD_ERR_INVALID_ARG;
    DevGuard g(s->eng->device);
    HIP_TRY(s->eng, hipDeviceSynchronize());
    HIP_TRY(s->eng, hipMemcpy(status, s->d_status, sizeof(int32_t), hipMemcpyDeviceToHost));
    return ITD_OK;
}

}  // extern "C"

namespace {
// host form: pinned staging in and out, ONE synchronisation per call
int stream_host(itd_stream *s, const double *block_host, double *baseline_host, double *rot_host, int32_t *emitted, bool flush)
{
    if (!s || (!flush && !block_host) || !baseline_host || s->kind >= ITD_STREAM_LEVELS) return ITD_ERR_INVALID_ARG;
    itd_engine *e = s->eng;
    DevGuard g(e->device);
    const size_t cnt = (size_t)s->C * (size_t)s->L;
    if (!s->h_in) {   // the staging, at the first host-form call: all four buffers or none
        Pinned<double> h_in, h_out;
        Buf<double> d_in, d_out;
        HIP_TRY(e, h_in.alloc(cnt * sizeof(double)));
        HIP_TRY(e, h_out.alloc(2 * cnt * sizeof(double)));
        HIP_TRY(e, d_in.alloc(cnt * sizeof(double)));
        HIP_TRY(e, d_out.alloc(2 * cnt * sizeof(double)));
        s->h_in = std::move(h_in); s->h_out = std::move(h_out); s->d_in = std::move(d_in); s->d_out = std::move(d_out);
    }
    hipStream_t st = e->own_stream;
    int32_t em = 0;
    int rc;
    double *d_base = s->d_out, *d_rot = rot_host ? s->d_out + cnt : nullptr;
    if (flush) rc = stream_flush(s, d_base, s->L, d_rot, s->L, &em, st);
    else {
        memcpy(s->h_in, block_host, cnt * sizeof(double));
        HIP_TRY(e, hipMemcpyAsync(s->d_in, s->h_in, cnt * sizeof(double), hipMemcpyHostToDevice, st));
        rc = stream_push(s, s->d_in, s->L, d_base, s->L, d_rot, s->L, &em, st);
    }
    if (rc) return rc;
    int32_t status = 0;
    if (em) {
        HIP_TRY(e, hipMemcpyAsync(s->h_out, s->d_out, (rot_host ? 2 : 1) * cnt * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(e, hipMemcpyAsync(&status, s->d_status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(e, hipStreamSynchronize(st));
    if (em) {
        memcpy(baseline_host, s->h_out, cnt * sizeof(double));
        if (rot_host) memcpy(rot_host, s->h_out + cnt, cnt * sizeof(double));
    }
    if (emitted) *emitted = em;
    return status ? ITD_ERR_NONFINITE : ITD_OK;
}
}  // namespace

extern "C" {
int itd_stream_push_host_f64(itd_stream *s, const double *block_host, double *baseline_host, double *rot_host, int32_t *emitted)
{
    return stream_host(s, block_host, baseline_host, rot_host, emitted, false);
}
int itd_stream_flush_host_f64(itd_stream *s, double *baseline_host, double *rot_host, int32_t *emitted)
{
    return stream_host(s, nullptr, baseline_host, rot_host, emitted, true);
}
}  // extern "C"

// ---- the levels stream: itd_levels_stream_* (include/pyitd_hip.h; the kernel, its schedule and the exactness rule:
//      k_stream_levels in itd_stream.hpp) ------------------------------------------------------------------------------
namespace {

// the launch-sequence form of one step: the new block into stage 0's ring, then per stage extract_batch of every channel's
// window and k_levels_route (itd_stream.hpp); a drained stage only lets its delayed rotation leave
int levels_step_seq(itd_stream *s, const LevelsArgs &a, hipStream_t st)
{
    const int64_t L = s->L, ring_stride = (int64_t)(s->M + 1) * 5 * L;
    const int C = s->C;
    if (a.in)
        k_stream_store<<<dim3((unsigned)((L + 255) / 256), C), 256, 0, st>>>(a.in, a.in_stride, s->ring, ring_stride, L, (int)(a.t % 3), nullptr);
    LevelsRoute r;
    r.a = a;
    r.rw = s->scr;
    r.bw = s->scr + (int64_t)C * 3 * L;
    const int64_t jo = a.t - 1 - s->M;
    const bool out = a.rows && jo >= 0 && (a.P < 0 || jo <= a.P - 1);
    for (int k = 0; k <= s->M; ++k) {
        const int64_t j = a.t - 1 - k;
        const bool active = j >= 0 && (a.P < 0 || j <= a.P - 1);
        if (!active && !(out && k < s->M)) continue;
        if (active) {
            const bool succ = a.P < 0 || j + 1 <= a.P - 1;
            const int64_t f = j > 0 ? j - 1 : 0, n = (j - f + (succ ? 2 : 1)) * L;
            const int rc = extract_batch(s->eng, s->ring + (int64_t)k * 5 * L + (f % 3) * L, n, C, ring_stride, s->scr, 3 * L,
                                         s->scr + (int64_t)C * 3 * L, 3 * L, nullptr, s->d_status, st);
            if (rc) return rc;
        }
        r.k = k;
        k_levels_route<1024><<<C, 1024, 0, st>>>(r);
    }
    HIP_TRY(s->eng, hipGetLastError());
    return ITD_OK;
}

// one step of every stage: ONE launch (or the launch sequence).  rows / exact: where the step's emitted block goes (ignored when
// it emits none)
int levels_step(itd_stream *s, const double *blk, int64_t in_stride, double *rows, int64_t row_stride, int64_t chan_stride,
                uint8_t *exact, hipStream_t st)
{
    LevelsArgs a;
    a.in = blk; a.in_stride = in_stride;
    a.ring = s->ring; a.delay = s->delay; a.eflags = s->eflags;
    a.rows = rows; a.row_stride = row_stride; a.chan_stride = chan_stride; a.exact = exact;
    a.status = s->d_status;
    a.t = s->t; a.P = s->P;
    a.L = (int)s->L; a.M = s->M; a.cw = s->cw;
    if (s->seq) {
        const int rc = levels_step_seq(s, a, st);
        if (rc) return rc;
        ++s->t;
        return ITD_OK;
    }
    void *args[] = {&a};
    HIP_TRY(s->eng, hipLaunchKernel(s->fn, dim3((unsigned)s->C), dim3((unsigned)s->threads), args, s->lds, st));
    HIP_TRY(s->eng, hipGetLastError());
    ++s->t;
    return ITD_OK;
}

bool levels_rows_ok(const itd_stream *s, double *rows, int64_t row_stride, int64_t chan_stride)
{
    if (!rows) return true;
    if (row_stride < s->L) return false;
    return s->C == 1 || chan_stride >= (int64_t)s->M * row_stride + s->L;
}

int levels_push(itd_stream *s, const double *blk, int64_t in_stride, double *rows, int64_t row_stride, int64_t chan_stride,
                uint8_t *exact, int32_t *emitted, hipStream_t st)
{
    const bool emits = s->t >= s->M + 1;
    const int rc = levels_step(s, blk, in_stride, emits ? rows : nullptr, row_stride, chan_stride, exact, st);
    if (rc) return rc;
    if (emitted) *emitted = emits ? 1 : 0;
    return ITD_OK;
}

// one block per call: the steps behind the last push until one emits (a stream of fewer than M+1 blocks has emitted none yet)
int levels_flush(itd_stream *s, double *rows, int64_t row_stride, int64_t chan_stride, uint8_t *exact, int32_t *emitted,
                 hipStream_t st)
{
    if (emitted) *emitted = 0;
    if (s->P < 0 && s->t == 0) return ITD_OK;      // empty: nothing to run
    if (s->P < 0) s->P = s->t;
    for (;;) {
        const int64_t jo = s->t - 1 - s->M;
        if (jo > s->P - 1) {            // empty
            s->t = 0;
            s->P = -1;
            return ITD_OK;
        }
        const int rc = levels_step(s, nullptr, 0, jo >= 0 ? rows : nullptr, row_stride, chan_stride, exact, st);
        if (rc) return rc;
        if (jo >= 0) {
            if (emitted) *emitted = 1;
            if (jo == s->P - 1) { s->t = 0; s->P = -1; }   // the last block: the stream starts afresh
            return ITD_OK;
        }
    }
}

// the launch-sequence form's window results [2][C][3 L] and extract_batch's workspace, at create / when the form is forced
int levels_seq_alloc(itd_stream *s)
{
    if (s->scr) return ITD_OK;
    Buf<double> scr;
    const hipError_t hrc = scr.alloc(2 * (size_t)s->C * 3 * (size_t)s->L * sizeof(double));
    if (hrc != hipSuccess) {
        (void)hipGetLastError();
        return hrc == hipErrorOutOfMemory ? ITD_ERR_NOMEM : fail_hip(s->eng, hrc, "hipMalloc(levels stream scratch)");
    }
    KnotWs w;
    const int rc = knot_workspace(s->eng, s->eng->d_bw, 3 * s->L, std::min<int32_t>(s->C, kMaxGridY), kWsExtract, w);
    if (rc) return rc;
    HIP_TRY(s->eng, hipDeviceSynchronize());
    s->scr = std::move(scr);        // the sequence form is ready only now
    return ITD_OK;
}

}  // namespace

extern "C" {

int itd_levels_stream_create(itd_stream **out, int device_id, int64_t block, int32_t channels, int32_t levels)
{
    if (!out) return ITD_ERR_INVALID_ARG;
    *out = nullptr;
    if (block < 8 || 3 * block >= (int64_t)INT32_MAX - 65536 || channels < 1 || channels > kMaxGridY) return ITD_ERR_INVALID_ARG;
    if (levels < 1 || levels > ITD_MAX_ROWS - 1) return ITD_ERR_INVALID_ARG;
    itd_stream *s = new (std::nothrow) itd_stream();
    if (!s) return ITD_ERR_NOMEM;
    int rc = itd_engine_create(&s->eng, device_id, 3 * block, 1);
    if (rc) { delete s; return rc; }
    s->L = block; s->C = channels; s->kind = ITD_STREAM_LEVELS; s->M = levels;
    DevGuard g(device_id);
    hipError_t hrc = hipSuccess;
    if (3 * block <= kResidentMax) {
        // the one-launch geometry of a three-block window (k_resident's classes) and its window of by-rank knot slots
        const WgClass wc = wg_class((int)(3 * block));
        const void *const inst[6] = {   // by size class
            reinterpret_cast<const void *>(&k_stream_levels<64, 4>),   reinterpret_cast<const void *>(&k_stream_levels<128, 4>),
            reinterpret_cast<const void *>(&k_stream_levels<256, 4>),  reinterpret_cast<const void *>(&k_stream_levels<512, 4>),
            reinterpret_cast<const void *>(&k_stream_levels<1024, 4>), reinterpret_cast<const void *>(&k_stream_levels<1024, 8>)};
        s->cw = wc.cw; s->lds = wc.lds; s->threads = wc.threads; s->fn = inst[wc.cls];
        hrc = allow_lds(s->eng, s->fn, kResidentLdsMax);
    } else {
        s->seq = 1;                 // the window does not fit one workgroup's LDS: the launch sequence
    }
    const size_t C = (size_t)channels, L = (size_t)block, R = (size_t)levels + 1;
    const size_t ring_b = C * R * 5 * L * sizeof(double), delay_b = C * ((size_t)levels * R / 2) * L * sizeof(double);
    if (hrc == hipSuccess) hrc = s->ring.alloc(ring_b);
    if (hrc == hipSuccess) hrc = s->delay.alloc(delay_b);
    if (hrc == hipSuccess) hrc = s->eflags.alloc(C * R * 4);
    if (hrc == hipSuccess) hrc = s->d_status.alloc(64);
    if (hrc == hipSuccess) hrc = hipMemset(s->d_status, 0, 64);
    // the host form's staging: [C][L] in, [C][M+1][L] rows and [C] flags out
    if (hrc == hipSuccess) hrc = s->d_in.alloc(C * L * sizeof(double));
    if (hrc == hipSuccess) hrc = s->d_out.alloc(C * R * L * sizeof(double));
    if (hrc == hipSuccess) hrc = s->d_exact.alloc(C);
    if (hrc == hipSuccess) hrc = s->h_in.alloc(C * L * sizeof(double));
    if (hrc == hipSuccess) hrc = s->h_out.alloc(C * R * L * sizeof(double));
    if (hrc == hipSuccess) hrc = s->h_exact.alloc(C);
    if (hrc == hipSuccess) hrc = hipDeviceSynchronize();     // (the fills ran on the null stream)
    if (hrc != hipSuccess) {
        const bool oom = hrc == hipErrorOutOfMemory;
        (void)hipGetLastError();
        itd_stream_destroy(s);
        return oom ? ITD_ERR_NOMEM : ITD_ERR_HIP;
    }
    if (s->seq && (rc = levels_seq_alloc(s)) != ITD_OK) {
        itd_stream_destroy(s);
        return rc;
    }
    *out = s;
    return ITD_OK;
}

int itd_levels_stream_set_sequence(itd_stream *s, int32_t on)
{
    if (!s || s->kind != ITD_STREAM_LEVELS || (on != 0 && on != 1)) return ITD_ERR_INVALID_ARG;
    if (!on && !s->fn) return ITD_ERR_INVALID_ARG;        // the block is too long for the one-launch form
    if (on) {
        DevGuard g(s->eng->device);
        const int rc = levels_seq_alloc(s);
        if (rc) return rc;
    }
    s->seq = on;
    return ITD_OK;
}

int itd_levels_stream_form(const itd_stream *s) { return s && s->kind == ITD_STREAM_LEVELS ? s->seq : -1; }

int itd_levels_stream_push_f64(itd_stream *s, const double *block_dev, int64_t in_stride, double *rows_dev, int64_t row_stride,
                               int64_t chan_stride, uint8_t *exact_dev, int32_t *emitted, void *stream)
{
    if (!s || !block_dev || s->kind != ITD_STREAM_LEVELS) return ITD_ERR_INVALID_ARG;
    if (s->P >= 0) return ITD_ERR_INVALID_ARG;                               // flushing: drain or reset first
    if (s->C > 1 && in_stride < s->L) return ITD_ERR_INVALID_ARG;
    if (s->t >= s->M + 1 && !rows_dev) return ITD_ERR_INVALID_ARG;          // this push emits a block
    if (!levels_rows_ok(s, rows_dev, row_stride, chan_stride)) return ITD_ERR_INVALID_ARG;
    DevGuard g(s->eng->device);
    return levels_push(s, block_dev, in_stride, rows_dev, row_stride, chan_stride, exact_dev, emitted, stream_of(s->eng, stream));
}

int itd_levels_stream_flush_f64(itd_stream *s, double *rows_dev, int64_t row_stride, int64_t chan_stride, uint8_t *exact_dev,
                                int32_t *emitted, void *stream)
{
    if (!s || s->kind != ITD_STREAM_LEVELS) return ITD_ERR_INVALID_ARG;
    if (itd_stream_blocks(s) > 0 && !rows_dev) return ITD_ERR_INVALID_ARG;  // this flush emits a block
    if (!levels_rows_ok(s, rows_dev, row_stride, chan_stride)) return ITD_ERR_INVALID_ARG;
    DevGuard g(s->eng->device);
    return levels_flush(s, rows_dev, row_stride, chan_stride, exact_dev, emitted, stream_of(s->eng, stream));
}

}  // extern "C"

namespace {
// host form: pinned staging in and out, ONE synchronisation per call
int levels_host(itd_stream *s, const double *block_host, double *rows_host, uint8_t *exact_host, int32_t *emitted, bool flush)
{
    if (!s || s->kind != ITD_STREAM_LEVELS || (!flush && !block_host) || !rows_host) return ITD_ERR_INVALID_ARG;
    if (!flush && s->P >= 0) return ITD_ERR_INVALID_ARG;
    itd_engine *e = s->eng;
    DevGuard g(e->device);
    const size_t cnt = (size_t)s->C * (size_t)s->L, R = (size_t)s->M + 1;
    hipStream_t st = e->own_stream;
    int32_t em = 0;
    int rc;
    if (flush) rc = levels_flush(s, s->d_out, s->L, (int64_t)R * s->L, s->d_exact, &em, st);
    else {
        memcpy(s->h_in, block_host, cnt * sizeof(double));
        HIP_TRY(e, hipMemcpyAsync(s->d_in, s->h_in, cnt * sizeof(double), hipMemcpyHostToDevice, st));
        rc = levels_push(s, s->d_in, s->L, s->d_out, s->L, (int64_t)R * s->L, s->d_exact, &em, st);
    }
    if (rc) return rc;
    if (em) {
        HIP_TRY(e, hipMemcpyAsync(s->h_out, s->d_out, R * cnt * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(e, hipMemcpyAsync(s->h_exact, s->d_exact, (size_t)s->C, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(e, hipStreamSynchronize(st));
    if (em) {
        memcpy(rows_host, s->h_out, R * cnt * sizeof(double));
        if (exact_host) memcpy(exact_host, s->h_exact, (size_t)s->C);
    }
    if (emitted) *emitted = em;
    return ITD_OK;
}
}  // namespace

extern "C" {
int itd_levels_stream_push_host_f64(itd_stream *s, const double *block_host, double *rows_host, uint8_t *exact_host, int32_t *emitted)
{
    return levels_host(s, block_host, rows_host, exact_host, emitted, false);
}
int itd_levels_stream_flush_host_f64(itd_stream *s, double *rows_host, uint8_t *exact_host, int32_t *emitted)
{
    return levels_host(s, nullptr, rows_host, exact_host, emitted, true);
}
}  // extern "C"
