// itd_fourier.inc — included at the end of itd_engine.hip (same translation unit: it uses the engine's internals).
//
//   * the FFT's host side (kernels: itd_fft.hpp): tier 1 for n <= 8192, four-step for n = n1 n2 with n1, n2 <= 8192, Bluestein
//     over a power of two otherwise; itd_debug_fft_f64 runs it on device data for the tests
//   * the mode selectors of itd_fourier_decomposition.py (:131-168, :171-209) as batched row operators
//   * the ITD-Fourier cascade (:212-255, :258-303): per band the cubic operator of itd_engine.hip (cubic_batch) on every live
//     signal with the band's retained knot list, then forward FFT, selection and inverse over all rows, the mode test and the next
//     signal on the device; ONE host synchronisation per iteration (the per-row hits and records)

namespace {

// threads per tier-1 workgroup: n <= 8 * threads (the stages' register budget)
int fft_threads(int n)
{
    int t = 64;
    while (t < 1024 && 8 * t < n) t *= 2;
    return t;
}

fft::Side side(double *p, int64_t es, int64_t bs, int64_t ss, int per, int real)
{
    fft::Side s;
    s.p = p; s.es = es; s.xs = 0; s.bs = bs; s.ss = ss; s.t0 = 0; s.per = per; s.real = real;
    return s;
}

// T transforms of n <= 8192 points, nx sub-transforms per transform (blockIdx.x: the four-step's column / row index)
int fft_lds(itd_engine *e, fft::Side in, fft::Side out, int n, int nx, int64_t T, int inverse, int64_t tw_m, double scale, hipStream_t st)
{
    HIP_TRY(e, allow_lds(e, reinterpret_cast<const void *>(&fft::k_fft_lds<1024>), fft::kLdsMax * sizeof(double2)));
    fft::LdsArgs a;
    a.in = in; a.out = out; a.n = n; a.inverse = inverse; a.tw_m = tw_m; a.scale = scale;
    for (int64_t t0 = 0; t0 < T; t0 += kMaxGridY) {
        a.in.t0 = in.t0 + t0;
        a.out.t0 = out.t0 + t0;
        const unsigned ny = (unsigned)std::min<int64_t>(kMaxGridY, T - t0);
        const int threads = fft_threads(n);
        if (threads <= 256) fft::k_fft_lds<256><<<dim3((unsigned)nx, ny), threads, (size_t)n * sizeof(double2), st>>>(a);   // <= 32 KiB
        else fft::k_fft_lds<1024><<<dim3((unsigned)nx, ny), threads, (size_t)n * sizeof(double2), st>>>(a);
    }
    HIP_TRY(e, hipGetLastError());
    return ITD_OK;
}

// n = n1 * n2 with n1, n2 <= 8192: the largest n1 <= sqrt(n) that divides n (0: none)
int64_t four_step_split(int64_t n)
{
    const int64_t L = fft::kLdsMax;
    if (n > L * L) return 0;
    int64_t best = 0;
    for (int64_t d = (n + L - 1) / L; d <= L && d * d <= n; ++d)
        if (n % d == 0) best = d;
    return best;
}

constexpr int64_t kFftChunkBytes = (int64_t)256 << 20;   // workspace per pass of the four-step and Bluestein forms

int fft_exec(itd_engine *e, fft::Side in, fft::Side out, int64_t n, int64_t T, int inverse, hipStream_t st);

// X[k2 + n2 k1] = sum_j1 W_n1^{j1 k1} W_n^{j1 k2} sum_j2 x[j1 + n1 j2] W_n2^{j2 k2}: columns into Y[t][j1][k2], then the rows with the
// twiddle W_n^{j1 k2} applied on input
int fft_four_step(itd_engine *e, fft::Side in, fft::Side out, int64_t n, int64_t n1, int64_t T, int inverse, hipStream_t st)
{
    const int64_t n2 = n / n1;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(T, kFftChunkBytes / (n * 16)));
    int rc = grow(e, e->d_fft_y, (size_t)chunk * (size_t)n * 16);
    if (rc) return rc;
    for (int64_t t0 = 0; t0 < T; t0 += chunk) {
        const int64_t tc = std::min(chunk, T - t0);
        fft::Side a = in;
        a.t0 = in.t0 + t0; a.xs = in.es; a.es = in.es * n1;
        fft::Side y = side((double *)e->d_fft_y, 1, 0, n, 1, 0);
        y.xs = n2;
        rc = fft_lds(e, a, y, (int)n2, (int)n1, tc, inverse, 0, 1.0, st);
        if (rc) return rc;
        fft::Side y2 = side((double *)e->d_fft_y, n2, 0, n, 1, 0);
        y2.xs = 1;
        fft::Side b = out;
        b.t0 = out.t0 + t0; b.xs = out.es; b.es = out.es * n2;
        rc = fft_lds(e, y2, b, (int)n1, (int)n2, tc, inverse, n, inverse ? 1.0 / (double)n : 1.0, st);
        if (rc) return rc;
    }
    return ITD_OK;
}

// any other n: Bluestein's chirp convolution over M = 2^k >= 2n - 1 (M <= 2^26); an inverse as conj(fft(conj(x))) / n
int fft_bluestein(itd_engine *e, fft::Side in, fft::Side out, int64_t n, int64_t T, int inverse, hipStream_t st)
{
    int64_t M = 1;
    while (M < 2 * n - 1) M <<= 1;
    if (M > (int64_t)fft::kLdsMax * fft::kLdsMax) return ITD_ERR_INVALID_ARG;
    int rc;
    if (e->fft_chirp_n != n) {          // the chirp's spectrum, once per n
        e->fft_chirp_n = 0;
        rc = grow(e, e->d_fft_b, (size_t)M * 16);
        if (rc) return rc;
        fft::k_blue_chirp<<<(unsigned)((M + 255) / 256), 256, 0, st>>>(n, M, (double2 *)e->d_fft_b);
        fft::Side bs = side((double *)e->d_fft_b, 1, 0, M, 1, 0);
        rc = fft_exec(e, bs, bs, M, 1, 0, st);
        if (rc) return rc;
        e->fft_chirp_n = n;
    }
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(T, kFftChunkBytes / (M * 16)));
    rc = grow(e, e->d_fft_a, (size_t)chunk * (size_t)M * 16);
    if (rc) return rc;
    double2 *A = (double2 *)e->d_fft_a;
    for (int64_t t0 = 0; t0 < T; t0 += chunk) {
        const int64_t tc = std::min(chunk, T - t0);
        fft::Side a = in;
        a.t0 = in.t0 + t0;
        fft::k_blue_pre<<<dim3((unsigned)((M + 255) / 256), (unsigned)tc), 256, 0, st>>>(a, n, M, inverse, A);
        fft::Side as = side((double *)A, 1, 0, M, 1, 0);
        rc = fft_exec(e, as, as, M, tc, 0, st);
        if (rc) return rc;
        fft::k_cmul_rows<<<dim3((unsigned)((M + 255) / 256), (unsigned)tc), 256, 0, st>>>(A, (const double2 *)e->d_fft_b, M);
        rc = fft_exec(e, as, as, M, tc, 1, st);
        if (rc) return rc;
        fft::Side b = out;
        b.t0 = out.t0 + t0;
        fft::k_blue_post<<<dim3((unsigned)((n + 255) / 256), (unsigned)tc), 256, 0, st>>>(A, n, M, inverse, b);
    }
    HIP_TRY(e, hipGetLastError());
    return ITD_OK;
}

// T transforms of n points, forward (numpy.fft.fft) or inverse (numpy.fft.ifft: scaled by 1/n); in and out may be the same array
int fft_exec(itd_engine *e, fft::Side in, fft::Side out, int64_t n, int64_t T, int inverse, hipStream_t st)
{
    if (n <= fft::kLdsMax) return fft_lds(e, in, out, (int)n, 1, T, inverse, 0, inverse ? 1.0 / (double)n : 1.0, st);
    const int64_t n1 = four_step_split(n);
    if (n1) return fft_four_step(e, in, out, n, n1, T, inverse, st);
    return fft_bluestein(e, in, out, n, T, inverse, st);
}

// the selector over T rows (in: real rows; out: the real modes): forward FFT, selection and mask in place, full complex inverse
int select_rows(itd_engine *e, fft::Side in, int64_t n, int64_t T, bool valid, fft::Side out, int32_t *rec, hipStream_t st)
{
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(T, kMaxGridY), kFftChunkBytes / (n * 16)));
    int rc = grow(e, e->d_fft_x, (size_t)chunk * (size_t)n * 16);
    if (rc) return rc;
    for (int64_t t0 = 0; t0 < T; t0 += chunk) {
        const int64_t tc = std::min(chunk, T - t0);
        fft::Side a = in, o = out;
        a.t0 = in.t0 + t0;
        o.t0 = out.t0 + t0;
        fft::Side x = side((double *)e->d_fft_x, 1, 0, n, 1, 0);
        rc = fft_exec(e, a, x, n, tc, 0, st);
        if (rc) return rc;
        if (valid) fft::k_fourier_select<true><<<(unsigned)tc, fft::kSelThreads, 0, st>>>((double2 *)e->d_fft_x, n, rec + t0 * 8);
        else fft::k_fourier_select<false><<<(unsigned)tc, fft::kSelThreads, 0, st>>>((double2 *)e->d_fft_x, n, rec + t0 * 8);
        rc = fft_exec(e, x, o, n, tc, 1, st);
        if (rc) return rc;
    }
    HIP_TRY(e, hipGetLastError());
    return ITD_OK;
}

int select_entry(itd_engine *e, const double *rows_dev, int64_t n, int64_t rows, int64_t row_stride, double *modes_dev, int64_t mode_stride,
                 int32_t *rec_dev, void *stream, bool valid)
{
    if (!e || !rows_dev || !modes_dev) return ITD_ERR_INVALID_ARG;
    if (n < 4 || n >= (int64_t)INT32_MAX - 65536 || rows < 1) return ITD_ERR_INVALID_ARG;
    if (rows > 1 && (row_stride < n || mode_stride < n)) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = stream_of(e, stream);
    int32_t *rec = rec_dev;
    if (!rec) {
        const int rc = grow(e, e->d_fft_rec, (size_t)rows * 32);
        if (rc) return rc;
        rec = (int32_t *)e->d_fft_rec;
    }
    return select_rows(e, side(const_cast<double *>(rows_dev), 1, 0, row_stride, 1, 1), n, rows, valid,
                       side(modes_dev, 1, 0, mode_stride, 1, 1), rec, st);
}

// the band plan: every band's retained knot list on the device, kept per engine while (n, sample_rate, lists) stay the same
int fourier_plan(itd_engine *e, int64_t n, double sample_rate, int32_t bands, const int64_t *knots_host, const int64_t *idx_host)
{
    size_t total = 0;
    for (int k = 0; k < bands; ++k) {
        const int64_t idx = idx_host[k];
        if (idx < 2 || idx > n - 1) return ITD_ERR_INVALID_ARG;
        const int64_t *kn = knots_host + total;
        for (int64_t j = 0; j <= idx; ++j)
            if (kn[j] < 0 || kn[j] >= n || (j > 0 && j < idx && kn[j] <= kn[j - 1])) return ITD_ERR_INVALID_ARG;
        total += (size_t)idx + 1;
    }
    if (e->fplan_n == n && e->fplan_sr == sample_rate && e->fplan_idx.size() == (size_t)bands &&
        std::equal(e->fplan_idx.begin(), e->fplan_idx.end(), idx_host) && e->fplan_host.size() == total &&
        std::equal(e->fplan_host.begin(), e->fplan_host.end(), knots_host))
        return ITD_OK;
    e->fplan_n = 0;
    e->fplan_host.assign(knots_host, knots_host + total);
    e->fplan_idx.assign(idx_host, idx_host + bands);
    std::vector<int32_t> narrow(total);
    for (size_t j = 0; j < total; ++j) narrow[j] = (int32_t)knots_host[j];
    int rc = grow(e, e->d_fplan, total * sizeof(int32_t));
    if (rc) return rc;
    HIP_TRY(e, hipMemcpy(e->d_fplan, narrow.data(), total * sizeof(int32_t), hipMemcpyHostToDevice));
    e->fplan_n = n;
    e->fplan_sr = sample_rate;
    return ITD_OK;
}

// grow the mode arena to hold `count` modes of n samples, keeping the ones it holds
int arena_reserve(itd_engine *e, int64_t n, int64_t count, hipStream_t st)
{
    const size_t want = (size_t)count * (size_t)n * sizeof(double);
    if (want <= e->d_fmodes.bytes()) return ITD_OK;
    Buf<double> p;                  // (the new block is the arena only once the live modes are in it)
    const hipError_t hrc = p.alloc(std::max(want, 2 * e->d_fmodes.bytes()));
    if (hrc != hipSuccess) { (void)hipGetLastError(); fail_hip(e, hrc, "hipMalloc(mode arena)"); return ITD_ERR_NOMEM; }
    if (e->fmodes_count) HIP_TRY(e, hipMemcpyAsync(p, e->d_fmodes, (size_t)e->fmodes_count * (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    e->d_fmodes = std::move(p);
    return ITD_OK;
}

int fourier_cascade(itd_engine *e, const double *x, int64_t n, int32_t B, int64_t x_stride, int32_t K, int32_t lean, int32_t max_rounds,
                    double *rows_out, double *acc, int32_t *rounds_h, int32_t *capped_h, int64_t *modes_h, hipStream_t st)
{
    const int64_t R = (int64_t)K + 1;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_sig = al((size_t)B * n * 8), b_rows = al((size_t)B * R * n * 8), b_modes = al((size_t)B * K * n * 8);
    const size_t b_rec = al((size_t)B * K * 32), b_hits = al((size_t)B * K * 4), b_int = al((size_t)B * 4);
    int rc = grow(e, e->d_fc, 3 * b_sig + b_rows + b_modes + b_rec + b_hits + 2 * b_int);
    if (rc) return rc;
    char *p = (char *)e->d_fc;
    double *wsig = (double *)p; p += b_sig;
    double *prob = (double *)p; p += b_sig;
    double *base = (double *)p; p += b_sig;
    double *wrows = (double *)p; p += b_rows;
    double *modes = (double *)p; p += b_modes;
    int32_t *rec = (int32_t *)p; p += b_rec;
    int32_t *hits = (int32_t *)p; p += b_hits;
    int32_t *any = (int32_t *)p; p += b_int;
    int32_t *slot_sig = (int32_t *)p;
    e->fmodes_count = 0;
    e->fmodes_n = n;
    e->fmodes_lean = lean != 0;
    e->frec.clear();
    const unsigned gx = (unsigned)((n + 255) / 256);
    // the signals, and their NaN check (the cubic operator has no NaN branch upstream: refused)
    HIP_TRY(e, hipMemsetAsync(any, 0, (size_t)B * 4, st));
    fft::k_copy_rows<<<dim3(gx, (unsigned)B), 256, 0, st>>>(x, x_stride, n, wsig, any);
    std::vector<int32_t> flags((size_t)B), slots((size_t)B), h_hits, h_rec;
    HIP_TRY(e, hipMemcpyAsync(flags.data(), any, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b) if (flags[(size_t)b]) return ITD_ERR_NONFINITE;
    if (lean) HIP_TRY(e, hipMemsetAsync(acc, 0, (size_t)B * K * n * 8, st));
    for (int b = 0; b < B; ++b) { slots[(size_t)b] = b; rounds_h[b] = 0; capped_h[b] = 0; modes_h[b] = 0; }
    int L = B;
    bool upload = true;
    for (int32_t round = 1; L > 0; ++round) {
        if (upload) HIP_TRY(e, hipMemcpyAsync(slot_sig, slots.data(), (size_t)L * 4, hipMemcpyHostToDevice, st));
        // the bands (:37-45): every live signal, one band after the other
        HIP_TRY(e, hipMemcpyAsync(prob, wsig, (size_t)L * n * 8, hipMemcpyDeviceToDevice, st));
        size_t off = 0;
        for (int k = 0; k < K; ++k) {
            const int64_t idx = e->fplan_idx[(size_t)k];
            rc = cubic_batch(e, prob, n, L, n, e->d_fplan + off, 0, idx, base, n, st, nullptr, nullptr);
            if (rc) return rc;
            fft::k_band_step<<<dim3(gx, (unsigned)L), 256, 0, st>>>(prob, base, wrows, n, R, k, k == K - 1);
            off += (size_t)idx + 1;
        }
        // the selector on every row but the residual (:230-237), the next signal (:241)
        rc = select_rows(e, side(wrows, 1, n, R * n, K, 1), n, (int64_t)L * K, false, side(modes, 1, n, (int64_t)K * n, K, 1), rec, st);
        if (rc) return rc;
        HIP_TRY(e, hipMemsetAsync(any, 0, (size_t)L * 4, st));
        fft::k_fourier_apply<<<(unsigned)((int64_t)L * K), fft::kSelThreads, 0, st>>>(modes, wrows, n, K, slot_sig, lean ? acc : nullptr, hits, any);
        fft::k_fourier_sum<<<dim3(gx, (unsigned)L), 256, 0, st>>>(wrows, n, R, any, wsig);
        h_hits.resize((size_t)L * K);
        h_rec.resize((size_t)L * K * 8);
        HIP_TRY(e, hipMemcpyAsync(h_hits.data(), hits, (size_t)L * K * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(e, hipMemcpyAsync(h_rec.data(), rec, (size_t)L * K * 32, hipMemcpyDeviceToHost, st));
        HIP_TRY(e, hipStreamSynchronize(st));
        int64_t found = 0;
        for (size_t j = 0; j < h_hits.size(); ++j) found += h_hits[j];
        if (!lean && found) { rc = arena_reserve(e, n, e->fmodes_count + found, st); if (rc) return rc; }
        int keep = 0;
        for (int s = 0; s < L; ++s) {
            const int sig = slots[(size_t)s];
            int nh = 0;
            for (int k = 0; k < K; ++k) {
                const size_t j = (size_t)s * K + k;
                if (!h_hits[j]) continue;
                ++nh;
                if (!lean)
                    HIP_TRY(e, hipMemcpyAsync(e->d_fmodes + (size_t)e->fmodes_count * n, modes + j * n, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
                ++e->fmodes_count;
                const int32_t r8[8] = {sig, round, k, h_rec[j * 8 + 1], h_rec[j * 8 + 2], h_rec[j * 8 + 3], h_rec[j * 8 + 4], h_rec[j * 8 + 5]};
                e->frec.insert(e->frec.end(), r8, r8 + 8);
            }
            if (nh) { rounds_h[sig] = round; modes_h[sig] += nh; }
            if (!nh || round >= max_rounds) {
                // final (:243-252), or stopped at the cap with the rows of this round
                capped_h[sig] = nh ? 1 : 0;
                HIP_TRY(e, hipMemcpyAsync(rows_out + (size_t)sig * R * n, wrows + (size_t)s * R * n, (size_t)R * n * 8, hipMemcpyDeviceToDevice, st));
                continue;
            }
            if (keep != s) {
                HIP_TRY(e, hipMemcpyAsync(wsig + (size_t)keep * n, wsig + (size_t)s * n, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
            }
            slots[(size_t)keep++] = sig;
        }
        upload = keep != L;
        L = keep;
    }
    HIP_TRY(e, hipStreamSynchronize(st));
    return ITD_OK;
}

int cascade_args(itd_engine *e, int64_t n, int32_t batch, double sample_rate, int32_t bands, const int64_t *knots_host,
                 const int64_t *idx_host, int32_t lean, int32_t max_rounds, int32_t *rounds_host, int32_t *capped_host, int64_t *modes_host)
{
    if (!e || !knots_host || !idx_host || !rounds_host || !capped_host || !modes_host) return ITD_ERR_INVALID_ARG;
    if (n < 4 || n >= (int64_t)INT32_MAX - 65536 || batch < 1 || batch > kMaxGridY || bands < 1 || max_rounds < 1) return ITD_ERR_INVALID_ARG;
    if (!(sample_rate > 0) || (lean != 0 && lean != 1)) return ITD_ERR_INVALID_ARG;
    return ITD_OK;
}

}  // namespace

extern "C" {

int itd_debug_fft_f64(itd_engine *e, const double *in_dev, double *out_dev, int64_t n, int32_t batch, int32_t inverse)
{
    if (!e || !in_dev || !out_dev || n < 1 || n >= (int64_t)INT32_MAX - 65536 || batch < 1 || (inverse != 0 && inverse != 1))
        return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    hipStream_t st = e->own_stream;
    const int rc = fft_exec(e, side(const_cast<double *>(in_dev), 1, 0, n, 1, 0), side(out_dev, 1, 0, n, 1, 0), n, batch, inverse, st);
    if (rc) return rc;
    HIP_TRY(e, hipStreamSynchronize(st));
    return ITD_OK;
}

int itd_fourier_mode_any_f64(itd_engine *e, const double *rows_dev, int64_t n, int64_t rows, int64_t row_stride, double *modes_dev,
                             int64_t mode_stride, int32_t *rec_dev, void *stream)
{
    return select_entry(e, rows_dev, n, rows, row_stride, modes_dev, mode_stride, rec_dev, stream, false);
}

int itd_fourier_mode_valid_f64(itd_engine *e, const double *rows_dev, int64_t n, int64_t rows, int64_t row_stride, double *modes_dev,
                               int64_t mode_stride, int32_t *rec_dev, void *stream)
{
    return select_entry(e, rows_dev, n, rows, row_stride, modes_dev, mode_stride, rec_dev, stream, true);
}

int itd_fourier_cascade_f64(itd_engine *e, const double *x_dev, int64_t n, int32_t batch, int64_t x_stride, double sample_rate,
                            int32_t bands, const int64_t *knots_host, const int64_t *idx_host, int32_t lean, int32_t max_rounds,
                            double *rows_dev, double *acc_dev, int32_t *rounds_host, int32_t *capped_host, int64_t *modes_host)
{
    int rc = cascade_args(e, n, batch, sample_rate, bands, knots_host, idx_host, lean, max_rounds, rounds_host, capped_host, modes_host);
    if (rc) return rc;
    if (!x_dev || !rows_dev || (lean && !acc_dev) || (batch > 1 && x_stride < n)) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    e->fmodes_count = 0;
    e->frec.clear();
    rc = fourier_plan(e, n, sample_rate, bands, knots_host, idx_host);
    if (rc) return rc;
    return fourier_cascade(e, x_dev, n, batch, x_stride, bands, lean, max_rounds, rows_dev, acc_dev, rounds_host, capped_host, modes_host,
                           e->own_stream);
}

int itd_fourier_cascade_host_f64(itd_engine *e, const double *x_host, int64_t n, int32_t batch, double sample_rate, int32_t bands,
                                 const int64_t *knots_host, const int64_t *idx_host, int32_t lean, int32_t max_rounds, double *rows_host,
                                 double *acc_host, int32_t *rounds_host, int32_t *capped_host, int64_t *modes_host)
{
    int rc = cascade_args(e, n, batch, sample_rate, bands, knots_host, idx_host, lean, max_rounds, rounds_host, capped_host, modes_host);
    if (rc) return rc;
    if (!x_host || !rows_host || (lean && !acc_host)) return ITD_ERR_INVALID_ARG;
    DevGuard g(e->device);
    e->fmodes_count = 0;
    e->frec.clear();
    rc = fourier_plan(e, n, sample_rate, bands, knots_host, idx_host);
    if (rc) return rc;
    const size_t xb = (size_t)batch * n * 8, rb = xb * ((size_t)bands + 1), ab = lean ? xb * (size_t)bands : 0;
    // staging of its own: the engine's d_io_* buffers hold what other host forms leave for later (ITD().itd()'s baselines)
    if ((rc = grow(e, e->d_fio, xb + rb + ab))) return rc;
    double *d_x = (double *)e->d_fio, *d_rows = d_x + xb / 8, *d_acc = lean ? d_rows + rb / 8 : nullptr;
    hipStream_t st = e->own_stream;
    HIP_TRY(e, hipMemcpyAsync(d_x, x_host, xb, hipMemcpyHostToDevice, st));
    rc = fourier_cascade(e, d_x, n, batch, n, bands, lean, max_rounds, d_rows, d_acc, rounds_host, capped_host, modes_host, st);
    if (rc) return rc;
    if ((rc = copy_to_host(e, rows_host, d_rows, rb, st))) return rc;
    if (lean && (rc = copy_to_host(e, acc_host, d_acc, ab, st))) return rc;
    return ITD_OK;
}

int itd_fourier_modes_f64(itd_engine *e, double *modes_dst, int64_t count, int32_t *records_host, int32_t to_host)
{
    if (!e || count < 0 || count > e->fmodes_count || (to_host != 0 && to_host != 1)) return ITD_ERR_INVALID_ARG;
    if (modes_dst && e->fmodes_lean) return ITD_ERR_INVALID_ARG;   // a lean call keeps no modes, only their records
    DevGuard g(e->device);
    if (records_host && count) memcpy(records_host, e->frec.data(), (size_t)count * 32);
    if (modes_dst && count) {
        const size_t bytes = (size_t)count * (size_t)e->fmodes_n * 8;
        if (to_host) { const int rc = copy_to_host(e, modes_dst, e->d_fmodes, bytes, e->own_stream); if (rc) return rc; }
        else {
            HIP_TRY(e, hipMemcpyAsync(modes_dst, e->d_fmodes, bytes, hipMemcpyDeviceToDevice, e->own_stream));
            HIP_TRY(e, hipStreamSynchronize(e->own_stream));
        }
    }
    return ITD_OK;
}

}  // extern "C"
