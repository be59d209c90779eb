// histograms and pair histograms host side (included by mhx_api.hip after mhx_api_hpd.inc): the checks, one launch per call on the
// context's select block, the counters back in one copy (mhx_hist_kernels.h, DESIGN.md section 6.5.3)

__global__ void __launch_bounds__(MHX_SELECT_THREADS)
k_hist1d(const mhx_real* __restrict__ samples, const long N, const int d1, const long C, const int* __restrict__ params,
         const double* __restrict__ edges, const int B, const unsigned long long chunk, unsigned long long* __restrict__ counts,
         unsigned long long* __restrict__ outside)
{
    __shared__ double lds_e[MHX_HIST_MAX_BINS + 1];
    __shared__ unsigned lds_n[MHX_HIST_MAX_BINS + 3];
    mhx_hist1d_body(samples, N, d1, C, params, edges, B, chunk, counts, outside, lds_e, lds_n);
}
// three pre-built sizes (B <= 32, 64, 128): LDS per block 4.6, 17 and 66 KB, so that a coarse pair histogram keeps the CU full
template <int BMAX>
__global__ void __launch_bounds__(MHX_SELECT_THREADS)
k_hist2d(const mhx_real* __restrict__ samples, const long N, const int d1, const long C, const int* __restrict__ params,
         const double* __restrict__ edges, const int B, const int* __restrict__ pairs, const unsigned long long chunk,
         unsigned long long* __restrict__ counts, unsigned long long* __restrict__ outside)
{
    __shared__ double lds_e[2 * (BMAX + 1)];
    __shared__ unsigned lds_n[BMAX * BMAX + 1];
    mhx_hist2d_body(samples, N, d1, C, params, edges, B, pairs, chunk, counts, outside, lds_e, lds_n);
}

#define MHX_HIST_MAX_ROWS 65535                             // rows (pairs) of a call: the grid's second dimension

static int hist_check(const draws_view& v, const int32_t* params, int32_t nparams, const double* edges, int32_t nbins, int32_t limit,
                      const uint64_t* counts)
{
    const char* who = v.who;
    if (!edges || !counts) return mhx_fail(MHX_EINVAL, "%s: bad argument", who);
    int rc = select_check_params(who, params, nparams, v.d1);
    if (rc) return rc;
    if (nparams > MHX_HIST_MAX_ROWS) return mhx_fail(MHX_EINVAL, "%s: %d rows in one call, at most %d", who, (int)nparams, MHX_HIST_MAX_ROWS);
    if (nbins < 1 || nbins > limit) return mhx_fail(MHX_EINVAL, "%s: nbins = %d is not in [1, %d]", who, (int)nbins, (int)limit);
    for (int i = 0; i < nparams; ++i) {
        const double* e = edges + (size_t)i * (nbins + 1);
        for (int k = 0; k <= nbins; ++k) {
            if (!std::isfinite(e[k])) return mhx_fail(MHX_EINVAL, "%s: edge %d of row slot %d is not finite", who, k, i);
            if (k && e[k] < e[k - 1]) return mhx_fail(MHX_EINVAL, "%s: the edges of row slot %d decrease at edge %d (%.17g after %.17g)", who, i, k, e[k], e[k - 1]);
        }
    }
    return MHX_OK;
}

static int hist_check_pairs(const char* who, const int32_t* pairs, int32_t npairs, int32_t nparams)
{
    if (!pairs || npairs <= 0) return mhx_fail(MHX_EINVAL, "%s: no pairs", who);
    if (npairs > MHX_HIST_MAX_ROWS) return mhx_fail(MHX_EINVAL, "%s: %d pairs in one call, at most %d", who, (int)npairs, MHX_HIST_MAX_ROWS);
    for (int q = 0; q < 2 * npairs; ++q)
        if (pairs[q] < 0 || pairs[q] >= nparams)
            return mhx_fail(MHX_EINVAL, "%s: pair %d names slot %d, outside [0, %d)", who, q / 2, (int)pairs[q], (int)nparams);
    return MHX_OK;
}

// the arguments are checked.  pairs NULL: the 1-D form (counts [P][B], outside [P][3]), else counts [Q][B][B] and outside [Q].  The
// caller's arrays are written last, after everything succeeded.
static int hist_compute(const draws_view& v, const int32_t* params, int P, const double* edges, int B, const int32_t* pairs, int Q,
                        uint64_t* counts, uint64_t* outside)
{
    mhx_ctx* ctx = v.ctx;
    const char* who = v.who;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t ncount = pairs ? (size_t)Q * B * B : (size_t)P * B, nout = pairs ? (size_t)Q : (size_t)P * 3;
    const size_t nedge = (size_t)P * (B + 1);
    unsigned long long* d_counts = nullptr;
    double* d_edges = nullptr;
    int *d_par = nullptr, *d_pairs = nullptr;
    int rc = scratch_carve(&ctx->select_scratch, &ctx->select_bytes, who, "histogram scratch", [&](scratch_pieces& c) {
        d_counts = c.take<unsigned long long>(ncount + nout);          // counters, then outside: one memset, one copy back
        d_edges = c.take<double>(nedge);
        d_par = c.take<int>(P);
        d_pairs = c.take<int>(pairs ? 2 * (size_t)Q : 0);
    });
    if (rc) return rc;
    unsigned long long* d_out = d_counts + ncount;
    HIP_TRY(hipMemsetAsync(d_counts, 0, (ncount + nout) * sizeof(uint64_t), ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_edges, edges, nedge * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_par, params, (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (pairs) HIP_TRY(hipMemcpyAsync(d_pairs, pairs, 2 * (size_t)Q * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const mhx_real* tensor = v.tensor;
    const long N = v.N, C = v.C;
    const int d1 = v.d1;
    const unsigned long long S = v.S();
    unsigned long long chunk = 0;
    const unsigned long long nblk = sweep_blocks(S, pairs ? Q : P, &chunk);
    const dim3 grid((unsigned)nblk, (unsigned)(pairs ? Q : P)), block(MHX_SELECT_THREADS);
    if (!pairs)
        hipLaunchKernelGGL(k_hist1d, grid, block, 0, ctx->stream, tensor, N, d1, C, d_par, d_edges, B, chunk, d_counts, d_out);
    else if (B <= 32)
        hipLaunchKernelGGL(k_hist2d<32>, grid, block, 0, ctx->stream, tensor, N, d1, C, d_par, d_edges, B, d_pairs, chunk, d_counts, d_out);
    else if (B <= 64)
        hipLaunchKernelGGL(k_hist2d<64>, grid, block, 0, ctx->stream, tensor, N, d1, C, d_par, d_edges, B, d_pairs, chunk, d_counts, d_out);
    else
        hipLaunchKernelGGL(k_hist2d<MHX_HIST2D_MAX_BINS>, grid, block, 0, ctx->stream, tensor, N, d1, C, d_par, d_edges, B, d_pairs, chunk, d_counts, d_out);
    if (hipGetLastError() != hipSuccess) return mhx_fail(MHX_EHIP, "%s: %s failed to launch", who, pairs ? "k_hist2d" : "k_hist1d");
    std::vector<uint64_t> land(ncount + nout);
    HIP_TRY(hipMemcpyAsync(land.data(), d_counts, (ncount + nout) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // every draw of every row (pair) is in exactly one counter: anything else is a tensor that changed during the call
    const size_t rows = pairs ? (size_t)Q : (size_t)P, per = ncount / rows, oper = nout / rows;
    for (size_t r = 0; r < rows; ++r) {
        uint64_t total = 0;
        for (size_t k = 0; k < per; ++k) total += land[r * per + k];
        for (size_t k = 0; k < oper; ++k) total += land[ncount + r * oper + k];
        if (total != S) return mhx_fail(MHX_EHIP, "%s: the counters of slot %zu hold %llu draws of %llu", who, r, (unsigned long long)total, S);
    }
    memcpy(counts, land.data(), ncount * sizeof(uint64_t));
    if (outside) memcpy(outside, land.data() + ncount, nout * sizeof(uint64_t));
    return MHX_OK;
}

// v is checked, nothing else is
static int hist_checked(const draws_view& v, const int32_t* params, int32_t nparams, const double* edges, int32_t nbins, uint64_t* counts,
                        uint64_t* outside)
{
    int rc = hist_check(v, params, nparams, edges, nbins, MHX_HIST_MAX_BINS, counts);
    return rc ? rc : hist_compute(v, params, nparams, edges, nbins, nullptr, 0, counts, outside);
}
static int hist2d_checked(const draws_view& v, const int32_t* params, int32_t nparams, const double* edges, int32_t nbins,
                          const int32_t* pairs, int32_t npairs, uint64_t* counts, uint64_t* outside)
{
    int rc = hist_check(v, params, nparams, edges, nbins, MHX_HIST2D_MAX_BINS, counts);
    if (!rc) rc = hist_check_pairs(v.who, pairs, npairs, nparams);
    return rc ? rc : hist_compute(v, params, nparams, edges, nbins, pairs, npairs, counts, outside);
}

int api_ctx_histogram(mhx_ctx* ctx, const mhx_real* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const int32_t* params,
                      int32_t nparams, const double* edges, int32_t nbins, uint64_t* counts, uint64_t* outside)
{
    draws_view v;
    int rc = draws_of_ctx("mhx_ctx_histogram", ctx, d_tensor, n_samples, dim1, nchains, &v);
    return rc ? rc : hist_checked(v, params, nparams, edges, nbins, counts, outside);
}

int api_run_histogram(mhx_run* r, const int32_t* params, int32_t nparams, const double* edges, int32_t nbins, uint64_t* counts,
                      uint64_t* outside)
{
    draws_view v;
    int rc = draws_of_run("mhx_run_histogram", r, &v);
    return rc ? rc : hist_checked(v, params, nparams, edges, nbins, counts, outside);
}

int api_ctx_histogram2d(mhx_ctx* ctx, const mhx_real* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const int32_t* params,
                        int32_t nparams, const double* edges, int32_t nbins, const int32_t* pairs, int32_t npairs, uint64_t* counts,
                        uint64_t* outside)
{
    draws_view v;
    int rc = draws_of_ctx("mhx_ctx_histogram2d", ctx, d_tensor, n_samples, dim1, nchains, &v);
    return rc ? rc : hist2d_checked(v, params, nparams, edges, nbins, pairs, npairs, counts, outside);
}

int api_run_histogram2d(mhx_run* r, const int32_t* params, int32_t nparams, const double* edges, int32_t nbins, const int32_t* pairs,
                        int32_t npairs, uint64_t* counts, uint64_t* outside)
{
    draws_view v;
    int rc = draws_of_run("mhx_run_histogram2d", r, &v);
    return rc ? rc : hist2d_checked(v, params, nparams, edges, nbins, pairs, npairs, counts, outside);
}
