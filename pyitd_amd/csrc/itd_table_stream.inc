// itd_table_stream.inc — included at the end of itd_engine.hip behind itd_ring_streams.inc (same translation unit: struct itd_stream and
// the engine's internals).  Host side of the half-wave table stream, itd_table_stream_* (k_table_stream, itd_table_stream.hpp, DESIGN.md
// section 27): one launch per push or flush step, no ring, no latency — what is open between two pushes is one TableCarry per row.
// The blocks pushed are counted in rs.cnt.t (itd_stream_reset and itd_stream_blocks know that field); everything else a step needs is
// in the stream's own fields.

namespace {

// the four tables and the count of one step, as a device entry or the host form's staging names them
struct TableOut {
    int64_t *start, *length, *peak;
    double *value;
    int64_t event_stride;
    int32_t *count;
};

// One step's launch, ONE per step: a push of blk, or (blk == nullptr) the flush step of a stream that holds blocks
int table_step(itd_stream *s, const double *blk, int64_t in_stride, const TableOut &t, hipStream_t st)
{
    TableStreamArgs a = {};
    a.in = blk; a.in_stride = in_stride;
    a.carry = s->tb.carry;
    a.status = s->d_status;
    a.blk = s->rs.cnt.t;
    a.origin = s->tb.origin;
    a.start = t.start; a.length = t.length; a.peak = t.peak; a.value = t.value;
    a.event_stride = t.event_stride;
    a.count = t.count;
    a.L = (int32_t)s->L;
    void *args[] = {&a};
    HIP_TRY(s->eng, hipLaunchKernel(s->fn, dim3((unsigned)s->C), dim3((unsigned)s->threads), args, blk ? s->lds : 0, st));
    HIP_TRY(s->eng, hipGetLastError());
    return ITD_OK;
}

// a push, or a flush (one step if the stream holds blocks, none if not); the block count moves only behind a launch that was made
int table_run(itd_stream *s, bool flush, const double *blk, int64_t in_stride, const TableOut &t, int32_t *emitted, hipStream_t st)
{
    RingCount &c = s->rs.cnt;
    if (emitted) *emitted = 0;
    if (flush && c.t == 0) return ITD_OK;                                 // empty: nothing to run
    const int rc = table_step(s, flush ? nullptr : blk, in_stride, t, st);
    if (rc) return rc;
    if (flush) c = kRingCountFresh;                                       // the stream starts afresh
    else ++c.t;
    if (emitted) *emitted = 1;
    return ITD_OK;
}

bool table_is(const itd_stream *s) { return s && s->kind == ITD_STREAM_TABLE; }

// a device entry: push (flush = false) or flush, asynchronous on `stream`
int table_entry(itd_stream *s, bool flush, const double *blk, int64_t in_stride, const TableOut &t, int32_t *emitted, void *stream)
{
    if (!table_is(s) || (!flush && !blk) || !t.count) return ITD_ERR_INVALID_ARG;
    if (s->C > 1 && ((!flush && in_stride < s->L) || t.event_stride < s->L + 1)) return ITD_ERR_INVALID_ARG;
    DevGuard g(s->eng->device);
    return table_run(s, flush, blk, in_stride, t, emitted, stream_of(s->eng, stream));
}

// host form: d_in / h_in = the block [C][L]; d_out / h_out = start, length, peak (int64), value: [4][C][L + 1] words of 8 bytes;
// rs.d_cnt / h_cnt = count [C].  Pinned staging in and out, ONE synchronisation per call.
int table_host(itd_stream *s, bool flush, const double *block_host, int64_t *start_host, int64_t *length_host, int64_t *peak_host,
               double *value_host, int32_t *count_host, int32_t *emitted)
{
    if (!table_is(s) || (!flush && !block_host) || !count_host) return ITD_ERR_INVALID_ARG;
    itd_engine *e = s->eng;
    DevGuard g(e->device);
    const size_t C = (size_t)s->C, L = (size_t)s->L, slot = L + 1, block_bytes = C * L * sizeof(double);
    hipStream_t st = e->own_stream;
    double *const d_out = s->d_out, *const h_out = s->h_out;
    void *const host[4] = {start_host, length_host, peak_host, value_host};
    // only the tables asked for are written and copied
    const TableOut t = {start_host ? reinterpret_cast<int64_t *>(d_out) : nullptr, length_host ? reinterpret_cast<int64_t *>(d_out + C * slot) : nullptr,
                        peak_host ? reinterpret_cast<int64_t *>(d_out + 2 * C * slot) : nullptr, value_host ? d_out + 3 * C * slot : nullptr,
                        (int64_t)slot, s->rs.d_cnt};
    if (!flush) {
        memcpy(s->h_in, block_host, block_bytes);
        HIP_TRY(e, hipMemcpyAsync(s->d_in, s->h_in, block_bytes, hipMemcpyHostToDevice, st));
    }
    int32_t em = 0;
    const int rc = table_run(s, flush, s->d_in, s->L, t, &em, st);
    if (rc) return rc;
    if (em) {
        for (int k = 0; k < 4; ++k)
            if (host[k]) HIP_TRY(e, hipMemcpyAsync(h_out + k * C * slot, d_out + k * C * slot, C * slot * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(e, hipMemcpyAsync(s->rs.h_cnt, s->rs.d_cnt, C * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(e, hipStreamSynchronize(st));
    if (em) {
        for (int k = 0; k < 4; ++k)
            if (host[k]) memcpy(host[k], h_out + k * C * slot, C * slot * sizeof(double));
        memcpy(count_host, s->rs.h_cnt, C * sizeof(int32_t));
    }
    if (emitted) *emitted = em;
    return ITD_OK;
}

}  // namespace

extern "C" {

int itd_table_stream_create(itd_stream **out, int device_id, int64_t block, int32_t rows, int64_t origin)
{
    if (!out) return ITD_ERR_INVALID_ARG;
    *out = nullptr;
    if (block < kTableStreamMinBlock || block > kTableStreamMaxBlock || rows < 1 || rows > kMaxGridY) return ITD_ERR_INVALID_ARG;
    itd_stream *s = new (std::nothrow) itd_stream();
    if (!s) return ITD_ERR_NOMEM;
    int rc = itd_engine_create(&s->eng, device_id, 3 * block, 1);
    if (rc) { delete s; return rc; }
    s->L = block; s->C = rows; s->kind = ITD_STREAM_TABLE; s->tb.origin = origin;
    const bool small = block <= kTableStreamSmall;
    s->threads = small ? 256 : 512;
    s->fn = small ? reinterpret_cast<const void *>(&k_table_stream<256>) : reinterpret_cast<const void *>(&k_table_stream<512>);
    s->lds = table_stream_lds((int)block);
    DevGuard g(device_id);
    const size_t C = (size_t)rows, L = (size_t)block;
    // the grant is the kernel function's, not this stream's: the most its instance ever asks for (ring_create)
    hipError_t hrc = allow_lds(s->eng, s->fn, table_stream_lds(small ? kTableStreamSmall : kTableStreamMaxBlock));
    if (hrc == hipSuccess) hrc = s->tb.carry.alloc(C * sizeof(TableCarry));
    if (hrc == hipSuccess) hrc = s->d_status.alloc(64);
    if (hrc == hipSuccess) hrc = hipMemset(s->d_status, 0, 64);
    if (hrc == hipSuccess) hrc = s->d_in.alloc(C * L * sizeof(double));
    if (hrc == hipSuccess) hrc = s->d_out.alloc(4 * C * (L + 1) * sizeof(double));
    if (hrc == hipSuccess) hrc = s->rs.d_cnt.alloc(C * sizeof(int32_t));
    if (hrc == hipSuccess) hrc = s->h_in.alloc(C * L * sizeof(double));
    if (hrc == hipSuccess) hrc = s->h_out.alloc(4 * C * (L + 1) * sizeof(double));
    if (hrc == hipSuccess) hrc = s->rs.h_cnt.alloc(C * sizeof(int32_t));
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

int itd_table_stream_push_f64(itd_stream *s, const double *block_dev, int64_t in_stride, int64_t *start_dev, int64_t *length_dev,
                              int64_t *peak_dev, double *value_dev, int64_t event_stride, int32_t *count_dev, int32_t *emitted, void *stream)
{
    return table_entry(s, false, block_dev, in_stride, {start_dev, length_dev, peak_dev, value_dev, event_stride, count_dev}, emitted, stream);
}

int itd_table_stream_flush_f64(itd_stream *s, int64_t *start_dev, int64_t *length_dev, int64_t *peak_dev, double *value_dev,
                               int64_t event_stride, int32_t *count_dev, int32_t *emitted, void *stream)
{
    return table_entry(s, true, nullptr, 0, {start_dev, length_dev, peak_dev, value_dev, event_stride, count_dev}, emitted, stream);
}

int itd_table_stream_push_host_f64(itd_stream *s, const double *block_host, int64_t *start_host, int64_t *length_host, int64_t *peak_host,
                                   double *value_host, int32_t *count_host, int32_t *emitted)
{
    return table_host(s, false, block_host, start_host, length_host, peak_host, value_host, count_host, emitted);
}

int itd_table_stream_flush_host_f64(itd_stream *s, int64_t *start_host, int64_t *length_host, int64_t *peak_host, double *value_host,
                                    int32_t *count_host, int32_t *emitted)
{
    return table_host(s, true, nullptr, start_host, length_host, peak_host, value_host, count_host, emitted);
}

}  // extern "C"
