// itd_ring_streams.inc — included at the end of itd_engine.hip behind itd_engine_batch.inc (same translation unit: struct itd_stream
// and the engine's internals).  Host side of the ring streams, fixed-latency streams of one launch per step on a ring of 2 D + 1
// blocks per row:
//     the wave-filter stream    itd_wave_stream_*      k_wave_stream      itd_wave_stream.hpp      DESIGN.md section 21
//     the spectrum stream       itd_spectrum_stream_*  k_spectrum_stream  itd_spectrum_stream.hpp  DESIGN.md section 22
//     the instantaneous stream  itd_inst_stream_*      k_inst_stream      itd_inst_stream.hpp      DESIGN.md section 24
//     the histogram stream      itd_hist_stream_*      k_hist_stream      itd_hist_stream.hpp      DESIGN.md section 25
// Written once for all of them: the launch of a step (ring_step; its window arithmetic and the block counting: itd_ring_plan.hpp),
// create, the device entries' guards and the host form (ring_create, ring_entry, ring_host).  A kind supplies
//   * its kernel, whose argument struct begins with a RingStepArgs, and a function that fills the struct's own fields;
//   * io_ok: what a device entry refuses among those fields;
//   * its staging: how many bytes of d_out, d_bnd and d_cnt its host form needs, and the two lists its host form hands ring_host;
//   * its row of constants, a RingKind.

namespace {

// bytes of the host form's staging besides the block ([C][L] float64 in d_in / h_in): d_out / h_out, d_bnd / h_bnd, d_cnt / h_cnt
struct RingStaging {
    size_t out, bnd, cnt;
};

struct RingKind {
    int32_t id;                                  // ITD_STREAM_*
    int32_t reach;                               // samples read beyond the horizon: D = ceil((H + reach) / L)
    int64_t min_block, max_block;
    int32_t big_threads;                         // 256 threads up to 256 kWaveStreamSpt samples, this many above
    const void *fn_small, *fn_big;               // the kernel's two instances
    size_t (*lds)(int L, int F, int TH);         // dynamic LDS of a launch
    int32_t max_bins;                            // the F of the largest request (0: the kernel has no bins)
    bool (*io_ok)(const itd_stream *s, bool emits, const RingStepArgs *a);
    RingStaging (*staging)(const itd_stream *s);
};

// One step's launch, ONE per step: the arriving block (blk, or nullptr on a flush step) goes into the ring, block b (b < 0: none) is
// emitted.  a: the kind's launch arguments (it is their first member) with the kind's own fields filled in.
int ring_step(itd_stream *s, const RingKind &k, RingStepArgs *a, const double *blk, int64_t in_stride, int64_t b, hipStream_t st)
{
    const RingCount &c = s->rs.cnt;
    ring_plan(*a, c.t, c.P, s->L, s->rs.D, s->rs.H, k.reach, b, blk != nullptr);
    a->in = blk; a->in_stride = in_stride;
    a->ring = s->ring;
    a->rec = s->rs.rec;
    a->status = s->d_status;
    void *args[] = {a};
    HIP_TRY(s->eng, hipLaunchKernel(s->fn, dim3((unsigned)s->C), dim3((unsigned)s->threads), args, s->lds, st));
    HIP_TRY(s->eng, hipGetLastError());
    return ITD_OK;
}

// a push (flush = false: blk arrives) or one flush step
int ring_run(itd_stream *s, const RingKind &k, RingStepArgs *a, bool flush, const double *blk, int64_t in_stride, int32_t *emitted,
             hipStream_t st)
{
    if (flush) return ring_flush(s->rs.cnt, emitted, [&](int64_t b) { return ring_step(s, k, a, nullptr, 0, b, st); });
    return ring_push(s->rs.cnt, s->rs.D, emitted, [&](int64_t b) { return ring_step(s, k, a, blk, in_stride, b, st); });
}

// create: the checks, the engine, D, the geometry, the LDS grant, the ring, the records, the status and the host form's staging
int ring_create(itd_stream **out, int device_id, int64_t block, int32_t rows, int64_t horizon, const RingKind &k, int64_t hop = 0,
                int32_t bins = 0, int32_t weight = 0, int32_t na = 0, int32_t nl = 0)
{
    if (!out) return ITD_ERR_INVALID_ARG;
    *out = nullptr;
    if (block < k.min_block || block > k.max_block || rows < 1 || rows > kMaxGridY) return ITD_ERR_INVALID_ARG;
    if (horizon < 1 || horizon > kWaveStreamMaxHorizon) return ITD_ERR_INVALID_ARG;
    itd_stream *s = new (std::nothrow) itd_stream();
    if (!s) return ITD_ERR_NOMEM;
    int rc = itd_engine_create(&s->eng, device_id, 3 * block, 1);
    if (rc) { delete s; return rc; }
    s->L = block; s->C = rows; s->kind = k.id; s->rs.H = horizon;
    s->rs.hop = hop; s->rs.F = bins; s->rs.weight = weight;
    s->rs.Na = na; s->rs.Nl = nl;
    s->rs.D = (int32_t)((horizon + k.reach + block - 1) / block);
    const bool small = block <= 256 * kWaveStreamSpt;
    s->threads = small ? 256 : k.big_threads;
    s->fn = small ? k.fn_small : k.fn_big;
    s->lds = k.lds((int)block, bins, s->threads);
    DevGuard g(device_id);
    const size_t C = (size_t)rows, L = (size_t)block, R = 2 * (size_t)s->rs.D + 1;
    const RingStaging sg = k.staging(s);
    // the grant is the kernel function's, not this stream's: the most its instance ever asks for, so that a later stream with a
    // shorter block does not lower it under a live one
    hipError_t hrc = allow_lds(s->eng, s->fn, k.lds(small ? 256 * kWaveStreamSpt : (int)k.max_block, k.max_bins, s->threads));
    if (hrc == hipSuccess) hrc = s->ring.alloc(C * R * L * sizeof(double));
    if (hrc == hipSuccess) hrc = s->rs.rec.alloc(C * R * sizeof(WaveBlockRec));
    if (hrc == hipSuccess) hrc = s->d_status.alloc(64);
    if (hrc == hipSuccess) hrc = hipMemset(s->d_status, 0, 64);
    if (hrc == hipSuccess) hrc = s->d_in.alloc(C * L * sizeof(double));
    if (hrc == hipSuccess) hrc = s->d_out.alloc(sg.out);
    if (hrc == hipSuccess && sg.bnd) hrc = s->rs.d_bnd.alloc(sg.bnd);
    if (hrc == hipSuccess && sg.cnt) hrc = s->rs.d_cnt.alloc(sg.cnt);
    if (hrc == hipSuccess) hrc = s->h_in.alloc(C * L * sizeof(double));
    if (hrc == hipSuccess) hrc = s->h_out.alloc(sg.out);
    if (hrc == hipSuccess && sg.bnd) hrc = s->rs.h_bnd.alloc(sg.bnd);
    if (hrc == hipSuccess && sg.cnt) hrc = s->rs.h_cnt.alloc(sg.cnt);
    if (hrc == hipSuccess) hrc = hipDeviceSynchronize();     // (the fill ran on the null stream)
    if (hrc != hipSuccess) {
        const bool oom = hrc == hipErrorOutOfMemory;
        (void)hipGetLastError();
        itd_stream_destroy(s);
        return oom ? ITD_ERR_NOMEM : ITD_ERR_HIP;
    }
    *out = s;
    return ITD_OK;
}

int ring_latency(const itd_stream *s, const RingKind &k) { return s && s->kind == k.id ? s->rs.D : -1; }

// a device entry: push (flush = false) or flush step, asynchronous on `stream`
int ring_entry(itd_stream *s, const RingKind &k, RingStepArgs *a, bool flush, const double *blk, int64_t in_stride, int32_t *emitted,
               void *stream)
{
    if (!s || s->kind != k.id || (!flush && !blk)) return ITD_ERR_INVALID_ARG;
    const RingCount &c = s->rs.cnt;
    if (!flush && ring_flushing(c)) return ITD_ERR_INVALID_ARG;              // flushing: drain or reset first
    if (!flush && s->C > 1 && in_stride < s->L) return ITD_ERR_INVALID_ARG;
    if (!k.io_ok(s, flush ? ring_held(c) > 0 : c.t >= s->rs.D, a)) return ITD_ERR_INVALID_ARG;
    DevGuard g(s->eng->device);
    return ring_run(s, k, a, flush, blk, in_stride, emitted, stream_of(s->eng, stream));
}

// The host form's two lists.  A parameter goes host -> pinned -> device before the step, on every call: `rows` rows of row_bytes,
// host_stride bytes apart at the caller's, packed in the staging.  A result comes device -> pinned -> host after an emitting step;
// one whose host pointer is null is skipped.
struct RingParam {
    const void *host;
    void *pinned, *dev;
    size_t rows, row_bytes, host_stride;
};
struct RingResult {
    void *host, *pinned;
    const void *dev;
    size_t bytes;
};

// host form: pinned staging in and out, ONE synchronisation per call.  s is the kind's stream (the caller has looked: it took the
// staging pointers from it); a: the launch arguments on the staging's device side.
int ring_host(itd_stream *s, const RingKind &k, RingStepArgs *a, bool flush, const double *block_host, std::initializer_list<RingParam> params,
              std::initializer_list<RingResult> results, int32_t *emitted)
{
    if (!flush && (!block_host || ring_flushing(s->rs.cnt))) return ITD_ERR_INVALID_ARG;
    itd_engine *e = s->eng;
    DevGuard g(e->device);
    const size_t block_bytes = (size_t)s->C * (size_t)s->L * sizeof(double);
    hipStream_t st = e->own_stream;
    int32_t em = 0;
    for (const RingParam &p : params) {
        for (size_t r = 0; r < p.rows; ++r) memcpy((char *)p.pinned + r * p.row_bytes, (const char *)p.host + r * p.host_stride, p.row_bytes);
        HIP_TRY(e, hipMemcpyAsync(p.dev, p.pinned, p.rows * p.row_bytes, hipMemcpyHostToDevice, st));
    }
    if (!flush) {
        memcpy(s->h_in, block_host, block_bytes);
        HIP_TRY(e, hipMemcpyAsync(s->d_in, s->h_in, block_bytes, hipMemcpyHostToDevice, st));
    }
    const int rc = ring_run(s, k, a, flush, s->d_in, s->L, &em, st);
    if (rc) return rc;
    if (em)
        for (const RingResult &r : results)
            if (r.host) HIP_TRY(e, hipMemcpyAsync(r.pinned, r.dev, r.bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    if (em)
        for (const RingResult &r : results)
            if (r.host) memcpy(r.host, r.pinned, r.bytes);
    if (emitted) *emitted = em;
    return ITD_OK;
}

// ---- the wave-filter stream ----------------------------------------------------------------------------------------------------

WaveStreamArgs wave_args(const double *bounds, int64_t bounds_stride, double *out, int64_t out_stride)
{
    WaveStreamArgs a = {};
    a.bounds = bounds; a.bounds_stride = bounds_stride;
    a.out = out; a.out_stride = out_stride;
    return a;
}

bool wave_io_ok(const itd_stream *s, bool emits, const RingStepArgs *r)
{
    const WaveStreamArgs &a = *reinterpret_cast<const WaveStreamArgs *>(r);
    if (a.bounds_stride != 0 && a.bounds_stride < 4) return false;
    if (emits && (!a.bounds || !a.out)) return false;
    return s->C == 1 || !a.out || a.out_stride >= s->L;
}

// host form: d_out / h_out = the filtered block [C][L], d_bnd / h_bnd = the bounds [C][4]
RingStaging wave_staging(const itd_stream *s)
{
    const size_t C = (size_t)s->C;
    return {C * (size_t)s->L * sizeof(double), C * 4 * sizeof(double), 0};
}

// (a named function, as in every RingKind row: three captureless lambdas of this one signature in the rows' initialisers all came
// out as the first of them under hipcc, and every kind was launched with the wave filter's LDS)
size_t wave_kind_lds(int L, int, int) { return wave_stream_lds(L); }

static_assert(kWaveStreamMaxBlock == kResidentMax, "the stream's largest block is the resident limit");
const RingKind kWaveKind = {ITD_STREAM_WAVES, 0, 8, kWaveStreamMaxBlock, 1024,
                            reinterpret_cast<const void *>(&k_wave_stream<256>), reinterpret_cast<const void *>(&k_wave_stream<1024>),
                            wave_kind_lds, 0, wave_io_ok, wave_staging};

int wave_host(itd_stream *s, const double *block_host, const double *bounds_host, double *out_host, int32_t *emitted, bool flush)
{
    if (!s || s->kind != ITD_STREAM_WAVES || !bounds_host || !out_host) return ITD_ERR_INVALID_ARG;
    const RingStaging sg = wave_staging(s);
    WaveStreamArgs a = wave_args(s->rs.d_bnd, 4, s->d_out, s->L);
    return ring_host(s, kWaveKind, &a.r, flush, block_host, {{bounds_host, s->rs.h_bnd.get(), s->rs.d_bnd.get(), 1, sg.bnd, 0}},
                     {{out_host, s->h_out.get(), s->d_out.get(), sg.out}}, emitted);
}

}  // namespace

extern "C" {

int itd_wave_stream_create(itd_stream **out, int device_id, int64_t block, int32_t rows, int64_t horizon)
{
    return ring_create(out, device_id, block, rows, horizon, kWaveKind);
}

int itd_wave_stream_latency(const itd_stream *s) { return ring_latency(s, kWaveKind); }

int itd_wave_stream_push_f64(itd_stream *s, const double *block_dev, int64_t in_stride, const double *bounds_dev, int64_t bounds_stride,
                             double *out_dev, int64_t out_stride, int32_t *emitted, void *stream)
{
    WaveStreamArgs a = wave_args(bounds_dev, bounds_stride, out_dev, out_stride);
    return ring_entry(s, kWaveKind, &a.r, false, block_dev, in_stride, emitted, stream);
}

int itd_wave_stream_flush_f64(itd_stream *s, const double *bounds_dev, int64_t bounds_stride, double *out_dev, int64_t out_stride,
                              int32_t *emitted, void *stream)
{
    WaveStreamArgs a = wave_args(bounds_dev, bounds_stride, out_dev, out_stride);
    return ring_entry(s, kWaveKind, &a.r, true, nullptr, 0, emitted, stream);
}

int itd_wave_stream_push_host_f64(itd_stream *s, const double *block_host, const double *bounds_host, double *out_host, int32_t *emitted)
{
    return wave_host(s, block_host, bounds_host, out_host, emitted, false);
}
int itd_wave_stream_flush_host_f64(itd_stream *s, const double *bounds_host, double *out_host, int32_t *emitted)
{
    return wave_host(s, nullptr, bounds_host, out_host, emitted, true);
}

}  // extern "C"

// ---- the spectrum stream (its reach: one sample past the wave filter's, A of sample (b+1) L) ------------------------------------------
namespace {

// (s: a spectrum stream, or what the entries refuse)
SpectrumStreamArgs spectrum_args(const itd_stream *s, const double *edges, int64_t edges_stride, double *power, int64_t power_stride,
                                 int32_t *outside, int32_t *overlong, int64_t count_stride)
{
    SpectrumStreamArgs a = {};
    a.edges = edges; a.edges_stride = edges_stride;
    a.power = power; a.power_stride = power_stride;
    a.outside = outside; a.overlong = overlong; a.count_stride = count_stride;
    if (s) { a.F = s->rs.F; a.spc = (int32_t)(s->rs.hop / 64); a.weight = s->rs.weight; }
    return a;
}

bool spectrum_io_ok(const itd_stream *s, bool emits, const RingStepArgs *r)
{
    const SpectrumStreamArgs &a = *reinterpret_cast<const SpectrumStreamArgs *>(r);
    const int64_t cells = s->L / s->rs.hop;
    if (a.edges_stride != 0 && a.edges_stride < s->rs.F + 1) return false;
    if (emits && (!a.edges || !a.power)) return false;
    if (s->C == 1) return true;
    if (a.power && a.power_stride < cells * s->rs.F) return false;
    return !(a.outside || a.overlong) || a.count_stride >= cells;
}

bool spectrum_hop_ok(int64_t hop) { return hop >= 64 && hop % 64 == 0 && (hop >= kTfeTile || hop == 64 || hop == 128 || hop == 256); }

// host form: d_out / h_out = power [C][L / hop][F], d_bnd / h_bnd = edges [C][F + 1] (one row where all rows share a set),
// d_cnt / h_cnt = outside, then overlong: [2][C][L / hop]
RingStaging spectrum_staging(const itd_stream *s)
{
    const size_t C = (size_t)s->C, cells = (size_t)(s->L / s->rs.hop), F = (size_t)s->rs.F;
    return {C * cells * F * sizeof(double), C * (F + 1) * sizeof(double), 2 * C * cells * sizeof(int32_t)};
}

const RingKind kSpectrumKind = {ITD_STREAM_SPECTRUM, 1, kSpectrumStreamMinBlock, kSpectrumStreamMaxBlock, 512,
                                reinterpret_cast<const void *>(&k_spectrum_stream<256>), reinterpret_cast<const void *>(&k_spectrum_stream<512>),
                                spectrum_stream_lds, kTfeMaxBins, spectrum_io_ok, spectrum_staging};

int spectrum_host(itd_stream *s, const double *block_host, const double *edges_host, int64_t edges_stride, double *power_host,
                  int32_t *outside_host, int32_t *overlong_host, int32_t *emitted, bool flush)
{
    if (!s || s->kind != ITD_STREAM_SPECTRUM || !edges_host || !power_host) return ITD_ERR_INVALID_ARG;
    if (edges_stride != 0 && edges_stride < s->rs.F + 1) return ITD_ERR_INVALID_ARG;
    const RingStaging sg = spectrum_staging(s);
    const size_t C = (size_t)s->C, cells = (size_t)(s->L / s->rs.hop), F1 = (size_t)s->rs.F + 1, ccnt = C * cells;
    int32_t *const d_cnt = s->rs.d_cnt, *const h_cnt = s->rs.h_cnt;
    SpectrumStreamArgs a = spectrum_args(s, s->rs.d_bnd, edges_stride ? (int64_t)F1 : 0, s->d_out, (int64_t)(cells * (size_t)s->rs.F), d_cnt,
                                         d_cnt + ccnt, (int64_t)cells);
    return ring_host(s, kSpectrumKind, &a.r, flush, block_host,
                     {{edges_host, s->rs.h_bnd.get(), s->rs.d_bnd.get(), edges_stride ? C : 1, F1 * sizeof(double), (size_t)edges_stride * sizeof(double)}},
                     {{power_host, s->h_out.get(), s->d_out.get(), sg.out},
                      {outside_host, h_cnt, d_cnt, ccnt * sizeof(int32_t)},
                      {overlong_host, h_cnt + ccnt, d_cnt + ccnt, ccnt * sizeof(int32_t)}},
                     emitted);
}

}  // namespace

extern "C" {

int itd_spectrum_stream_create(itd_stream **out, int device_id, int64_t block, int32_t rows, int64_t horizon, int64_t hop, int32_t bins,
                               int32_t weight)
{
    if (!out) return ITD_ERR_INVALID_ARG;
    *out = nullptr;
    if (!spectrum_hop_ok(hop) || block % hop != 0) return ITD_ERR_INVALID_ARG;
    if (bins < 1 || bins > kTfeMaxBins || weight < 0 || weight > 2) return ITD_ERR_INVALID_ARG;
    return ring_create(out, device_id, block, rows, horizon, kSpectrumKind, hop, bins, weight);
}

int itd_spectrum_stream_latency(const itd_stream *s) { return ring_latency(s, kSpectrumKind); }

int itd_spectrum_stream_push_f64(itd_stream *s, const double *block_dev, int64_t in_stride, const double *edges_dev, int64_t edges_stride,
                                 double *power_dev, int64_t power_stride, int32_t *outside_dev, int32_t *overlong_dev, int64_t count_stride,
                                 int32_t *emitted, void *stream)
{
    SpectrumStreamArgs a = spectrum_args(s, edges_dev, edges_stride, power_dev, power_stride, outside_dev, overlong_dev, count_stride);
    return ring_entry(s, kSpectrumKind, &a.r, false, block_dev, in_stride, emitted, stream);
}

int itd_spectrum_stream_flush_f64(itd_stream *s, const double *edges_dev, int64_t edges_stride, double *power_dev, int64_t power_stride,
                                  int32_t *outside_dev, int32_t *overlong_dev, int64_t count_stride, int32_t *emitted, void *stream)
{
    SpectrumStreamArgs a = spectrum_args(s, edges_dev, edges_stride, power_dev, power_stride, outside_dev, overlong_dev, count_stride);
    return ring_entry(s, kSpectrumKind, &a.r, true, nullptr, 0, emitted, stream);
}

int itd_spectrum_stream_push_host_f64(itd_stream *s, const double *block_host, const double *edges_host, int64_t edges_stride,
                                      double *power_host, int32_t *outside_host, int32_t *overlong_host, int32_t *emitted)
{
    return spectrum_host(s, block_host, edges_host, edges_stride, power_host, outside_host, overlong_host, emitted, false);
}
int itd_spectrum_stream_flush_host_f64(itd_stream *s, const double *edges_host, int64_t edges_stride, double *power_host,
                                       int32_t *outside_host, int32_t *overlong_host, int32_t *emitted)
{
    return spectrum_host(s, nullptr, edges_host, edges_stride, power_host, outside_host, overlong_host, emitted, true);
}

}  // extern "C"

// ---- the instantaneous stream (locality and latency are the spectrum stream's) -----------------------------------------------------
namespace {

InstStreamArgs inst_args(double *amp, double *phase, double *freq, int32_t *length, int64_t out_stride, int32_t *counts, int64_t counts_stride)
{
    InstStreamArgs a = {};
    a.amp = amp; a.phase = phase; a.freq = freq; a.length = length; a.out_stride = out_stride;
    a.counts = counts; a.counts_stride = counts_stride;
    return a;
}

bool inst_io_ok(const itd_stream *s, bool emits, const RingStepArgs *r)
{
    const InstStreamArgs &a = *reinterpret_cast<const InstStreamArgs *>(r);
    const bool any = a.amp || a.phase || a.freq || a.length;
    if (emits && !any) return false;
    if (s->C == 1) return true;
    if (any && a.out_stride < s->L) return false;
    return !a.counts || a.counts_stride >= 2;
}

// host form: d_out / h_out = amplitude, phase, frequency [3][C][L]; d_cnt / h_cnt = length [C][L], then the counts [C][2]
RingStaging inst_staging(const itd_stream *s)
{
    const size_t C = (size_t)s->C, L = (size_t)s->L;
    return {3 * C * L * sizeof(double), 0, C * (L + 2) * sizeof(int32_t)};
}

size_t inst_kind_lds(int L, int, int) { return inst_stream_lds(L); }

const RingKind kInstKind = {ITD_STREAM_INSTANT, 1, kInstStreamMinBlock, kInstStreamMaxBlock, 512,
                            reinterpret_cast<const void *>(&k_inst_stream<256>), reinterpret_cast<const void *>(&k_inst_stream<512>),
                            inst_kind_lds, 0, inst_io_ok, inst_staging};

// only the outputs asked for are computed and copied
int inst_host(itd_stream *s, const double *block_host, double *amp_host, double *phase_host, double *freq_host, int32_t *length_host,
              int32_t *counts_host, int32_t *emitted, bool flush)
{
    if (!s || s->kind != ITD_STREAM_INSTANT) return ITD_ERR_INVALID_ARG;
    if (!amp_host && !phase_host && !freq_host && !length_host) return ITD_ERR_INVALID_ARG;
    const size_t cnt = (size_t)s->C * (size_t)s->L;
    double *const d_out = s->d_out, *const h_out = s->h_out;
    int32_t *const d_cnt = s->rs.d_cnt, *const h_cnt = s->rs.h_cnt;
    InstStreamArgs a = inst_args(amp_host ? d_out : nullptr, phase_host ? d_out + cnt : nullptr, freq_host ? d_out + 2 * cnt : nullptr,
                                 length_host ? d_cnt : nullptr, s->L, counts_host ? d_cnt + cnt : nullptr, 2);
    return ring_host(s, kInstKind, &a.r, flush, block_host, {},
                     {{amp_host, h_out, d_out, cnt * sizeof(double)},
                      {phase_host, h_out + cnt, d_out + cnt, cnt * sizeof(double)},
                      {freq_host, h_out + 2 * cnt, d_out + 2 * cnt, cnt * sizeof(double)},
                      {length_host, h_cnt, d_cnt, cnt * sizeof(int32_t)},
                      {counts_host, h_cnt + cnt, d_cnt + cnt, (size_t)s->C * 2 * sizeof(int32_t)}},
                     emitted);
}

}  // namespace

extern "C" {

int itd_inst_stream_create(itd_stream **out, int device_id, int64_t block, int32_t rows, int64_t horizon)
{
    return ring_create(out, device_id, block, rows, horizon, kInstKind);
}

int itd_inst_stream_latency(const itd_stream *s) { return ring_latency(s, kInstKind); }

int itd_inst_stream_push_f64(itd_stream *s, const double *block_dev, int64_t in_stride, double *amp_dev, double *phase_dev, double *freq_dev,
                             int32_t *length_dev, int64_t out_stride, int32_t *counts_dev, int64_t counts_stride, int32_t *emitted,
                             void *stream)
{
    InstStreamArgs a = inst_args(amp_dev, phase_dev, freq_dev, length_dev, out_stride, counts_dev, counts_stride);
    return ring_entry(s, kInstKind, &a.r, false, block_dev, in_stride, emitted, stream);
}

int itd_inst_stream_flush_f64(itd_stream *s, double *amp_dev, double *phase_dev, double *freq_dev, int32_t *length_dev, int64_t out_stride,
                              int32_t *counts_dev, int64_t counts_stride, int32_t *emitted, void *stream)
{
    InstStreamArgs a = inst_args(amp_dev, phase_dev, freq_dev, length_dev, out_stride, counts_dev, counts_stride);
    return ring_entry(s, kInstKind, &a.r, true, nullptr, 0, emitted, stream);
}

int itd_inst_stream_push_host_f64(itd_stream *s, const double *block_host, double *amp_host, double *phase_host, double *freq_host,
                                  int32_t *length_host, int32_t *counts_host, int32_t *emitted)
{
    return inst_host(s, block_host, amp_host, phase_host, freq_host, length_host, counts_host, emitted, false);
}
int itd_inst_stream_flush_host_f64(itd_stream *s, double *amp_host, double *phase_host, double *freq_host, int32_t *length_host,
                                   int32_t *counts_host, int32_t *emitted)
{
    return inst_host(s, nullptr, amp_host, phase_host, freq_host, length_host, counts_host, emitted, true);
}

}  // extern "C"

// ---- the histogram stream (latency and locality are the wave filter's: reach 0) ------------------------------------------------------
namespace {

// (s: a histogram stream, or what the entries refuse)
HistStreamArgs hist_args(const itd_stream *s, const double *aedges, int64_t aedges_stride, const double *ledges, int64_t ledges_stride,
                         int32_t *count, int32_t *samples, int64_t hist_stride, int32_t *outside, int32_t *overlong, int64_t count_stride)
{
    HistStreamArgs a = {};
    a.aedges = aedges; a.aedges_stride = aedges_stride;
    a.ledges = ledges; a.ledges_stride = ledges_stride;
    a.count = count; a.samples = samples; a.hist_stride = hist_stride;
    a.outside = outside; a.overlong = overlong; a.count_stride = count_stride;
    if (s) { a.Na = s->rs.Na; a.Nl = s->rs.Nl; a.spc = (int32_t)(s->rs.hop / 64); }
    return a;
}

bool hist_io_ok(const itd_stream *s, bool emits, const RingStepArgs *r)
{
    const HistStreamArgs &a = *reinterpret_cast<const HistStreamArgs *>(r);
    const int64_t cells = s->L / s->rs.hop;
    if (a.aedges_stride != 0 && a.aedges_stride < s->rs.Na + 1) return false;
    if (a.ledges_stride != 0 && a.ledges_stride < s->rs.Nl + 1) return false;
    if (emits && (!a.aedges || !a.ledges || !a.count || !a.samples)) return false;
    if (s->C == 1) return true;
    if ((a.count || a.samples) && a.hist_stride < s->rs.F) return false;
    return !(a.outside || a.overlong) || a.count_stride >= cells;
}

// host form: d_out / h_out = count, then samples: [2][C][F] int32 (F = the cells of a block: L / hop Na Nl); d_bnd / h_bnd = the
// amplitude edges [C][Na + 1], then the length edges [C][Nl + 1] (one row each where all rows share a set); d_cnt / h_cnt = outside,
// then overlong: [2][C][L / hop]
RingStaging hist_staging(const itd_stream *s)
{
    const size_t C = (size_t)s->C, cells = (size_t)(s->L / s->rs.hop), F = (size_t)s->rs.F;
    return {2 * C * F * sizeof(int32_t), C * (size_t)(s->rs.Na + s->rs.Nl + 2) * sizeof(double), 2 * C * cells * sizeof(int32_t)};
}

const RingKind kHistKind = {ITD_STREAM_HIST, 0, kHistStreamMinBlock, kHistStreamMaxBlock, 512,
                            reinterpret_cast<const void *>(&k_hist_stream<256>), reinterpret_cast<const void *>(&k_hist_stream<512>),
                            hist_stream_lds, kHistStreamMaxCells, hist_io_ok, hist_staging};

int hist_host(itd_stream *s, const double *block_host, const double *aedges_host, int64_t aedges_stride, const double *ledges_host,
              int64_t ledges_stride, int32_t *count_host, int32_t *samples_host, int32_t *outside_host, int32_t *overlong_host,
              int32_t *emitted, bool flush)
{
    if (!s || s->kind != ITD_STREAM_HIST || !aedges_host || !ledges_host || !count_host || !samples_host) return ITD_ERR_INVALID_ARG;
    if (aedges_stride != 0 && aedges_stride < s->rs.Na + 1) return ITD_ERR_INVALID_ARG;
    if (ledges_stride != 0 && ledges_stride < s->rs.Nl + 1) return ITD_ERR_INVALID_ARG;
    const size_t C = (size_t)s->C, cells = (size_t)(s->L / s->rs.hop), F = (size_t)s->rs.F, ccnt = C * cells;
    const size_t A1 = (size_t)s->rs.Na + 1, L1 = (size_t)s->rs.Nl + 1;
    int32_t *const d_hist = reinterpret_cast<int32_t *>(s->d_out.get()), *const h_hist = reinterpret_cast<int32_t *>(s->h_out.get());
    int32_t *const d_cnt = s->rs.d_cnt, *const h_cnt = s->rs.h_cnt;
    double *const d_ae = s->rs.d_bnd, *const h_ae = s->rs.h_bnd;
    double *const d_le = d_ae + C * A1, *const h_le = h_ae + C * A1;
    HistStreamArgs a = hist_args(s, d_ae, aedges_stride ? (int64_t)A1 : 0, d_le, ledges_stride ? (int64_t)L1 : 0, d_hist, d_hist + C * F,
                                 (int64_t)F, d_cnt, d_cnt + ccnt, (int64_t)cells);
    return ring_host(s, kHistKind, &a.r, flush, block_host,
                     {{aedges_host, h_ae, d_ae, aedges_stride ? C : 1, A1 * sizeof(double), (size_t)aedges_stride * sizeof(double)},
                      {ledges_host, h_le, d_le, ledges_stride ? C : 1, L1 * sizeof(double), (size_t)ledges_stride * sizeof(double)}},
                     {{count_host, h_hist, d_hist, C * F * sizeof(int32_t)},
                      {samples_host, h_hist + C * F, d_hist + C * F, C * F * sizeof(int32_t)},
                      {outside_host, h_cnt, d_cnt, ccnt * sizeof(int32_t)},
                      {overlong_host, h_cnt + ccnt, d_cnt + ccnt, ccnt * sizeof(int32_t)}},
                     emitted);
}

}  // namespace

extern "C" {

int itd_hist_stream_create(itd_stream **out, int device_id, int64_t block, int32_t rows, int64_t horizon, int64_t hop, int32_t na, int32_t nl)
{
    if (!out) return ITD_ERR_INVALID_ARG;
    *out = nullptr;
    if (hop < 64 || hop % 64 != 0 || block < hop || block % hop != 0) return ITD_ERR_INVALID_ARG;
    if (na < 1 || na > kWaveHistMaxBins || nl < 1 || nl > kWaveHistMaxBins || na * nl > kWaveHistMaxCells) return ITD_ERR_INVALID_ARG;
    if (block > kHistStreamMaxBlock || (block / hop) * na * nl > kHistStreamMaxCells) return ITD_ERR_INVALID_ARG;
    return ring_create(out, device_id, block, rows, horizon, kHistKind, hop, (int32_t)(block / hop) * na * nl, 0, na, nl);
}

int itd_hist_stream_latency(const itd_stream *s) { return ring_latency(s, kHistKind); }

int itd_hist_stream_push_f64(itd_stream *s, const double *block_dev, int64_t in_stride, const double *aedges_dev, int64_t aedges_stride,
                             const double *ledges_dev, int64_t ledges_stride, int32_t *count_dev, int32_t *samples_dev, int64_t hist_stride,
                             int32_t *outside_dev, int32_t *overlong_dev, int64_t count_stride, int32_t *emitted, void *stream)
{
    HistStreamArgs a = hist_args(s, aedges_dev, aedges_stride, ledges_dev, ledges_stride, count_dev, samples_dev, hist_stride, outside_dev,
                                 overlong_dev, count_stride);
    return ring_entry(s, kHistKind, &a.r, false, block_dev, in_stride, emitted, stream);
}

int itd_hist_stream_flush_f64(itd_stream *s, const double *aedges_dev, int64_t aedges_stride, const double *ledges_dev, int64_t ledges_stride,
                              int32_t *count_dev, int32_t *samples_dev, int64_t hist_stride, int32_t *outside_dev, int32_t *overlong_dev,
                              int64_t count_stride, int32_t *emitted, void *stream)
{
    HistStreamArgs a = hist_args(s, aedges_dev, aedges_stride, ledges_dev, ledges_stride, count_dev, samples_dev, hist_stride, outside_dev,
                                 overlong_dev, count_stride);
    return ring_entry(s, kHistKind, &a.r, true, nullptr, 0, emitted, stream);
}

int itd_hist_stream_push_host_f64(itd_stream *s, const double *block_host, const double *aedges_host, int64_t aedges_stride,
                                  const double *ledges_host, int64_t ledges_stride, int32_t *count_host, int32_t *samples_host,
                                  int32_t *outside_host, int32_t *overlong_host, int32_t *emitted)
{
    return hist_host(s, block_host, aedges_host, aedges_stride, ledges_host, ledges_stride, count_host, samples_host, outside_host,
                     overlong_host, emitted, false);
}
int itd_hist_stream_flush_host_f64(itd_stream *s, const double *aedges_host, int64_t aedges_stride, const double *ledges_host,
                                   int64_t ledges_stride, int32_t *count_host, int32_t *samples_host, int32_t *outside_host,
                                   int32_t *overlong_host, int32_t *emitted)
{
    return hist_host(s, nullptr, aedges_host, aedges_stride, ledges_host, ledges_stride, count_host, samples_host, outside_host, overlong_host,
                     emitted, true);
}

}  // extern "C"
