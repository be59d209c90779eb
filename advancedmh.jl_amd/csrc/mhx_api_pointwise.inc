// pointwise log-likelihood host side (included by mhx_api.hip after mhx_api_derive.inc): the checks, the run-time module, the scratch
// for rows, shifts and partials, three launches -- shift, sweep, merge -- and one copy back (mhx_pointwise_kernels.h, DESIGN.md 6.5.7)

// data rows per tile where option POINTWISE_ROWS does not say: the fastest measured per width (DESIGN.md section 7; section 6.5.7 has
// the register table) -- fp64: 8 ahead of 4 by 10 % at 2 000 rows, level with it at 30; fp32: 4 ahead of 8 by 2 % and 8 %
#define MHX_POINTWISE_ROWS_DEFAULT (MHX_REAL64 ? 8 : 4)
// blocks the sweep aims at before it stops splitting a chain block's draws over strip slots: a few per compute unit
#define MHX_POINTWISE_TARGET_BLOCKS 2048

static std::string pointwise_source(const char* source)
{
    std::string s = "#include \"mhx_device_math.h\"\n#line 1 \"pointwise.hip\"\n";
    s += source;
    s += "\n#define MHX_HAVE_POINTWISE 1\n#include \"mhx_pointwise_kernels.h\"\n";
    return s;
}

// v is checked, nothing else is.  Nothing is written to shift, out5 or T unless the call succeeds.
static int pointwise_checked(const draws_view& v, const char* source, const mhx_real* rows, int64_t nrows, int32_t rowlen,
                             const mhx_real* data, size_t ndata, int32_t shift_given, double* shift, double* out5, int64_t* T)
{
    const char* who = v.who;
    mhx_ctx* ctx = v.ctx;
    if (!source || !rows || !shift || !out5) return mhx_fail(MHX_EINVAL, "%s: NULL argument", who);
    if (nrows < 1 || rowlen < 1)
        return mhx_fail(MHX_EINVAL, "%s: %lld data rows of %d reals: at least one row of at least one real", who, (long long)nrows, (int)rowlen);
    if (nrows > 0x7fffffffll || (unsigned long long)nrows * (unsigned long long)rowlen > 0x7fffffffull)
        return mhx_fail(MHX_EINVAL, "%s: %lld data rows of %d reals: rows are indexed in 31 bits", who, (long long)nrows, (int)rowlen);
    if (ndata && !data) return mhx_fail(MHX_EINVAL, "%s: data is NULL", who);
    if (ndata > 0x7fffffffull) return mhx_fail(MHX_EINVAL, "%s: the data block is too large", who);
    if (v.C > 0x7fffffffl || v.N > 0x7fffffffl)
        return mhx_fail(MHX_EINVAL, "%s: %ld saved draws of %ld chains: each is counted in 31 bits", who, v.N, v.C);
    HIP_TRY(hipSetDevice(ctx->device));
    const int R = opt_int(ctx, "POINTWISE_ROWS", MHX_POINTWISE_ROWS_DEFAULT);
    if (R != 2 && R != 4 && R != 8 && R != 16) return mhx_fail(MHX_EINVAL, "%s: option POINTWISE_ROWS = %d is not 2, 4, 8 or 16", who, R);
    jit_module* m = nullptr;
    hipFunction_t f_sweep = nullptr, f_shift = nullptr, f_merge = nullptr;
    int rc = jit_compile(ctx, pointwise_source(source), {"MHX_JIT_POINTWISE_ROWS=" + std::to_string(R)}, &m);
    if (rc == MHX_EJIT) {                                   // as derive_checked: a diagnostic on the caller's text is the caller's error
        const std::string log = mhx_last_error();
        if (log.find("pointwise.hip") != std::string::npos) return mhx_fail(MHX_EINVAL, "%s: the function does not compile: %.1900s", who, log.c_str());
        return rc;
    }
    if (rc == MHX_OK) rc = jit_function(m, "mhx_jit_pointwise", &f_sweep);
    if (rc == MHX_OK) rc = jit_function(m, "mhx_jit_pointwise_shift", &f_shift);
    if (rc == MHX_OK) rc = jit_function(m, "mhx_jit_pointwise_merge", &f_merge);
    if (rc) return rc;
    // the grid: chain blocks x strip slots x row tiles.  Slots only while the grid is small, never more than MHX_POINTWISE_MAX_SLOTS:
    // the partials are ncb * slots * nrows * 5 doubles whatever N is
    const long ncb = (v.C + MHX_POINTWISE_THREADS - 1) / MHX_POINTWISE_THREADS;
    const long ntiles = ((long)nrows + R - 1) / R;
    const long nstrips = (v.N + MHX_POINTWISE_STRIP - 1) / MHX_POINTWISE_STRIP;
    if (ntiles > 65535) return mhx_fail(MHX_EINVAL, "%s: %lld data rows are more than %d tiles of %d: fewer rows per call", who, (long long)nrows, 65535, R);
    const long want = (MHX_POINTWISE_TARGET_BLOCKS + ncb * ntiles - 1) / (ncb * ntiles);
    const long slots = std::max(1l, std::min(std::min(want, nstrips), (long)MHX_POINTWISE_MAX_SLOTS));
    const size_t P = (size_t)ncb * (size_t)slots, nr = (size_t)nrows;
    double *d_part = nullptr, *d_out = nullptr, *d_shift = nullptr;
    mhx_real *d_rows = nullptr, *d_data = nullptr;
    rc = scratch_carve(&ctx->select_scratch, &ctx->select_bytes, who, "pointwise scratch", [&](scratch_pieces& c) {
        d_part = c.take<double>(P * nr * 5);
        d_out = c.take<double>(nr * 5);
        d_shift = c.take<double>(nr);
        d_rows = c.take<mhx_real>(nr * (size_t)rowlen);
        d_data = c.take<mhx_real>(ndata ? ndata : 1);       // (one dummy element keeps the pointer valid)
    });
    if (rc) { (void)hipGetLastError(); return rc; }
    HIP_TRY(hipMemcpyAsync(d_rows, rows, nr * (size_t)rowlen * sizeof(mhx_real), hipMemcpyHostToDevice, ctx->stream));
    if (ndata) HIP_TRY(hipMemcpyAsync(d_data, data, ndata * sizeof(mhx_real), hipMemcpyHostToDevice, ctx->stream));
    const mhx_real* src = v.tensor;
    const mhx_real *rr = d_rows, *dd = d_data;
    long N = v.N, C = v.C, PP = (long)P;
    int d = v.d1 - 1, nd = (int)ndata, nrw = (int)nrows, rl = (int)rowlen;
    const double *cpart = d_part, *cshift = d_shift;
    const unsigned row_blocks = (unsigned)((nr + 63) / 64);
    if (shift_given) {
        HIP_TRY(hipMemcpyAsync(d_shift, shift, nr * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    } else {
        void* p0[] = {&src, &C, &d, &rr, &nrw, &rl, &dd, &nd, &d_shift};
        HIP_TRY(hipModuleLaunchKernel(f_shift, row_blocks, 1, 1, 64, 1, 1, 0, ctx->stream, p0, nullptr));
    }
    void* p1[] = {&src, &N, &C, &d, &rr, &nrw, &rl, &dd, &nd, &cshift, &d_part};
    HIP_TRY(hipModuleLaunchKernel(f_sweep, (unsigned)ncb, (unsigned)slots, (unsigned)ntiles, MHX_POINTWISE_THREADS, 1, 1, 0, ctx->stream, p1, nullptr));
    void* p2[] = {&cpart, &PP, &nrw, &d_out};
    HIP_TRY(hipModuleLaunchKernel(f_merge, row_blocks, 1, 1, 64, 1, 1, 0, ctx->stream, p2, nullptr));
    std::vector<double> land(nr * 6);                       // the five arrays, then the shift: written to the caller only after the sync
    HIP_TRY(hipMemcpyAsync(land.data(), d_out, nr * 5 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(land.data() + nr * 5, d_shift, nr * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(out5, land.data(), nr * 5 * sizeof(double));
    if (!shift_given) memcpy(shift, land.data() + nr * 5, nr * sizeof(double));
    if (T) *T = (int64_t)v.N * (int64_t)v.C;
    return MHX_OK;
}

int api_ctx_pointwise(mhx_ctx* ctx, const mhx_real* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const char* source,
                      const mhx_real* rows, int64_t nrows, int32_t rowlen, const mhx_real* data, size_t ndata, int32_t shift_given,
                      double* shift, double* out5, int64_t* T)
{
    draws_view v;
    int rc = draws_of_ctx("mhx_ctx_pointwise", ctx, d_tensor, n_samples, dim1, nchains, &v);
    return rc ? rc : pointwise_checked(v, source, rows, nrows, rowlen, data, ndata, shift_given, shift, out5, T);
}

int api_run_pointwise(const mhx_run* src, const char* source, const mhx_real* rows, int64_t nrows, int32_t rowlen, const mhx_real* data,
                      size_t ndata, int32_t shift_given, double* shift, double* out5, int64_t* T)
{
    draws_view v;
    int rc = draws_of_run("mhx_run_pointwise", src, &v);
    return rc ? rc : pointwise_checked(v, source, rows, nrows, rowlen, data, ndata, shift_given, shift, out5, T);
}
