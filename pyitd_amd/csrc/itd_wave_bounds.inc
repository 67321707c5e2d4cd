// itd_wave_bounds.inc — included at the end of itd_engine.hip behind itd_table_stream.inc (same translation unit: struct itd_stream and
// the engine's internals).  Host side of the wave filter's bounds from histogram quantiles (itd_wave_bounds.hpp, DESIGN.md section 28):
// the many-row call itd_wave_bounds_batch on a handle of its own (itd_bounds_*) and the bounds stream itd_bounds_stream_*, the bounds
// of a sliding window over a histogram stream's slices, one launch per push.  The pushes are counted in rs.cnt.t (itd_stream_reset and itd_stream_blocks know that field).

// The many-row call's handle: an engine of its own (device, stream, error text) and the call's workspace, 128 int64 sums per row of a
// chunk.  Nothing of it lies in an engine a caller shares with other operators, so no other call can stand in front of or behind it
// there (DESIGN.md section 23's question does not arise).
struct itd_bounds {
    itd_engine *eng = nullptr;
    Buf<unsigned long long> ws;
};

namespace {

bool bounds_bins_ok(int32_t na, int32_t nl)
{
    return na >= 1 && na <= kBoundsMaxBins && nl >= 1 && nl <= kBoundsMaxBins && na * nl <= kBoundsMaxCells;
}
// the strides of the edges, the parameters and the bounds: 0 (where allowed) is one set for every row
bool bounds_strides_ok(int32_t na, int32_t nl, int64_t ae_stride, int64_t le_stride, int64_t q_stride, int64_t bounds_stride)
{
    return (ae_stride == 0 || ae_stride >= na + 1) && (le_stride == 0 || le_stride >= nl + 1) && (q_stride == 0 || q_stride >= 8) &&
           bounds_stride >= 4;
}

bool bounds_is(const itd_stream *s) { return s && s->kind == ITD_STREAM_BOUNDS; }

// what a push reads and writes besides the histogram, as a device entry or the host form's staging names it
struct BoundsIo {
    const double *ae; int64_t ae_stride;
    const double *le; int64_t le_stride;
    const double *q; int64_t q_stride;
    double *bounds; int64_t bounds_stride;
    int64_t *total;
};

// One push's launch, ONE per push; the count moves only behind a launch that was made
int bounds_push(itd_stream *s, const int32_t *hist, int64_t hist_stride, const BoundsIo &io, hipStream_t st)
{
    const int64_t p = s->rs.cnt.t, W = s->bd.W;
    BoundsStreamArgs a = {};
    a.hist = hist; a.hist_stride = hist_stride;
    a.ae = io.ae; a.le = io.le; a.q = io.q;
    a.ae_stride = io.ae_stride; a.le_stride = io.le_stride; a.q_stride = io.q_stride;
    a.bounds = io.bounds; a.bounds_stride = io.bounds_stride;
    a.total = io.total;
    a.ring = s->bd.ring; a.run = s->bd.run;
    a.C = s->bd.slices; a.na = s->rs.Na; a.nl = s->rs.Nl; a.W = s->bd.W;
    a.slot = (int32_t)(p % W);
    a.held = (int32_t)std::min<int64_t>(p, W);
    k_bounds_stream<<<dim3((unsigned)s->C), kBoundsThreads, 0, st>>>(a);
    HIP_TRY(s->eng, hipGetLastError());
    ++s->rs.cnt.t;
    return ITD_OK;
}

}  // namespace

extern "C" {

int itd_bounds_create(itd_bounds **out, int device_id)
{
    if (!out) return ITD_ERR_INVALID_ARG;
    *out = nullptr;
    itd_bounds *b = new (std::nothrow) itd_bounds();
    if (!b) return ITD_ERR_NOMEM;
    const int rc = itd_engine_create(&b->eng, device_id, 4096, 1);
    if (rc) { delete b; return rc; }
    *out = b;
    return ITD_OK;
}

void itd_bounds_destroy(itd_bounds *b)
{
    if (!b) return;
    itd_engine *const e = b->eng;
    DevGuard g(e->device);
    (void)hipStreamSynchronize(e->own_stream);
    delete b;                       // the workspace goes before its engine does
    itd_engine_destroy(e);
}

const char *itd_bounds_last_error(const itd_bounds *b) { return b && b->eng ? b->eng->err : "null handle"; }

int itd_wave_bounds_batch(itd_bounds *b, const int32_t *hist_dev, int32_t rows, int64_t hist_stride, int64_t T, int64_t t0, int64_t t1,
                          int32_t na, int32_t nl, const double *aedges_dev, int64_t aedges_stride, const double *ledges_dev,
                          int64_t ledges_stride, const double *quant_dev, int64_t quant_stride, double *bounds_dev, int64_t bounds_stride,
                          int64_t *total_dev, void *stream)
{
    if (!b || !hist_dev || !aedges_dev || !ledges_dev || !quant_dev || !bounds_dev || rows < 1) return ITD_ERR_INVALID_ARG;
    if (!bounds_bins_ok(na, nl) || !bounds_strides_ok(na, nl, aedges_stride, ledges_stride, quant_stride, bounds_stride)) return ITD_ERR_INVALID_ARG;
    if (T < 1 || T > (int64_t)INT32_MAX || t0 < 0 || t0 >= t1 || t1 > T) return ITD_ERR_INVALID_ARG;
    const int cells = na * nl;
    if (rows > 1 && hist_stride < T * cells) return ITD_ERR_INVALID_ARG;
    itd_engine *const e = b->eng;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    const int chunk = std::min<int32_t>(rows, kMaxGridY);
    const int rc = grow(e, b->ws, (size_t)chunk * kBoundsSlot * sizeof(unsigned long long));
    if (rc) return rc;
    unsigned long long *const ws = b->ws;
    const int64_t per = bounds_part_bins(cells), parts = (t1 - t0 + per - 1) / per;
    return for_row_chunks(e, rows, chunk, [&](int b0, int nb) {
        const int64_t words = (int64_t)nb * kBoundsSlot;
        k_wave_bounds_zero<<<(unsigned)((words + kBoundsThreads - 1) / kBoundsThreads), kBoundsThreads, 0, st>>>(ws, words);
        k_wave_bounds_part<<<dim3((unsigned)parts, (unsigned)nb), kBoundsThreads, 0, st>>>(hist_dev + (int64_t)b0 * hist_stride, hist_stride, t0, t1,
                                                                                          per, na, nl, ws);
        k_wave_bounds_finish<<<(unsigned)nb, 64, 0, st>>>(ws, na, nl, aedges_dev + (int64_t)b0 * aedges_stride, aedges_stride,
                                                          ledges_dev + (int64_t)b0 * ledges_stride, ledges_stride,
                                                          quant_dev + (int64_t)b0 * quant_stride, quant_stride,
                                                          bounds_dev + (int64_t)b0 * bounds_stride, bounds_stride, at(total_dev, b0));
    });
}

int itd_bounds_stream_create(itd_stream **out, int device_id, int32_t rows, int32_t na, int32_t nl, int32_t slices, int32_t window)
{
    if (!out) return ITD_ERR_INVALID_ARG;
    *out = nullptr;
    if (rows < 1 || rows > kMaxGridY || !bounds_bins_ok(na, nl) || slices < 1 || (int64_t)slices * na * nl > kBoundsStreamMaxCells) return ITD_ERR_INVALID_ARG;
    if (window < 1 || window > kBoundsStreamMaxWindow) return ITD_ERR_INVALID_ARG;
    itd_stream *s = new (std::nothrow) itd_stream();
    if (!s) return ITD_ERR_NOMEM;
    int rc = itd_engine_create(&s->eng, device_id, 4096, 1);
    if (rc) { delete s; return rc; }
    s->C = rows; s->kind = ITD_STREAM_BOUNDS;
    s->rs.Na = na; s->rs.Nl = nl; s->rs.F = slices * na * nl;
    s->bd.slices = slices; s->bd.W = window;
    DevGuard g(device_id);
    const size_t C = (size_t)rows, bins = (size_t)(na + nl), par = C * (size_t)(na + 1 + nl + 1 + 8 + 4 + 1);
    hipError_t hrc = s->bd.ring.alloc(C * (size_t)window * bins * sizeof(unsigned long long));
    if (hrc == hipSuccess) hrc = s->bd.run.alloc(C * bins * sizeof(unsigned long long));
    if (hrc == hipSuccess) hrc = s->d_status.alloc(64);
    if (hrc == hipSuccess) hrc = hipMemset(s->d_status, 0, 64);
    if (hrc == hipSuccess) hrc = s->bd.d_hist.alloc(C * (size_t)s->rs.F * sizeof(int32_t));
    if (hrc == hipSuccess) hrc = s->bd.h_hist.alloc(C * (size_t)s->rs.F * sizeof(int32_t));
    if (hrc == hipSuccess) hrc = s->bd.d_par.alloc(par * sizeof(double));
    if (hrc == hipSuccess) hrc = s->bd.h_par.alloc(par * sizeof(double));
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

int itd_bounds_stream_push(itd_stream *s, const int32_t *hist_dev, int64_t hist_stride, const double *aedges_dev, int64_t aedges_stride,
                           const double *ledges_dev, int64_t ledges_stride, const double *quant_dev, int64_t quant_stride, double *bounds_dev,
                           int64_t bounds_stride, int64_t *total_dev, void *stream)
{
    if (!bounds_is(s) || !hist_dev || !aedges_dev || !ledges_dev || !quant_dev || !bounds_dev) return ITD_ERR_INVALID_ARG;
    if (!bounds_strides_ok(s->rs.Na, s->rs.Nl, aedges_stride, ledges_stride, quant_stride, bounds_stride)) return ITD_ERR_INVALID_ARG;
    if (s->C > 1 && hist_stride < s->rs.F) return ITD_ERR_INVALID_ARG;
    DevGuard g(s->eng->device);
    return bounds_push(s, hist_dev, hist_stride, {aedges_dev, aedges_stride, ledges_dev, ledges_stride, quant_dev, quant_stride, bounds_dev,
                                                  bounds_stride, total_dev}, stream_of(s->eng, stream));
}

// host form: contiguous hist_host [rows][slices][na][nl] in, bounds_host [rows][4] and total_host [rows] (optional) out; the edges
// and the parameters with a stride of 0 (one set) or na + 1 / nl + 1 / 8 (dense rows).  Pinned staging, ONE synchronisation per call.
int itd_bounds_stream_push_host(itd_stream *s, const int32_t *hist_host, const double *aedges_host, int64_t aedges_stride,
                                const double *ledges_host, int64_t ledges_stride, const double *quant_host, int64_t quant_stride,
                                double *bounds_host, int64_t *total_host)
{
    if (!bounds_is(s) || !hist_host || !aedges_host || !ledges_host || !quant_host || !bounds_host) return ITD_ERR_INVALID_ARG;
    const int32_t na = s->rs.Na, nl = s->rs.Nl;
    if ((aedges_stride != 0 && aedges_stride != na + 1) || (ledges_stride != 0 && ledges_stride != nl + 1) ||
        (quant_stride != 0 && quant_stride != 8))
        return ITD_ERR_INVALID_ARG;
    itd_engine *e = s->eng;
    DevGuard g(e->device);
    hipStream_t st = e->own_stream;
    const size_t C = (size_t)s->C, F = (size_t)s->rs.F;
    // the staging's parts, in doubles: ae, le, q in; bounds, total out
    const size_t n_ae = aedges_stride ? C * (na + 1) : (size_t)(na + 1), n_le = ledges_stride ? C * (nl + 1) : (size_t)(nl + 1);
    const size_t n_q = quant_stride ? C * 8 : 8, o_le = C * (na + 1), o_q = o_le + C * (nl + 1), o_b = o_q + C * 8, o_t = o_b + C * 4;
    double *const hp = s->bd.h_par, *const dp = s->bd.d_par;
    memcpy(s->bd.h_hist, hist_host, C * F * sizeof(int32_t));
    memcpy(hp, aedges_host, n_ae * sizeof(double));
    memcpy(hp + o_le, ledges_host, n_le * sizeof(double));
    memcpy(hp + o_q, quant_host, n_q * sizeof(double));
    HIP_TRY(e, hipMemcpyAsync(s->bd.d_hist, s->bd.h_hist, C * F * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(e, hipMemcpyAsync(dp, hp, o_b * sizeof(double), hipMemcpyHostToDevice, st));
    const int rc = bounds_push(s, s->bd.d_hist, (int64_t)F, {dp, aedges_stride, dp + o_le, ledges_stride, dp + o_q, quant_stride, dp + o_b, 4,
                                                            reinterpret_cast<int64_t *>(dp + o_t)}, st);
    if (rc) return rc;
    HIP_TRY(e, hipMemcpyAsync(hp + o_b, dp + o_b, C * 5 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    memcpy(bounds_host, hp + o_b, C * 4 * sizeof(double));
    if (total_host) memcpy(total_host, hp + o_t, C * sizeof(int64_t));
    return ITD_OK;
}

}  // extern "C"
