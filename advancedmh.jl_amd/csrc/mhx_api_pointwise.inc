// pointwise log-likelihood host side (included by mhx_api.hip after mhx_api_derive.inc): the checks (row_blocks_checked), the run-time
// module (user_module), the scratch for rows, shifts and partials, the grid (pointwise_sweep_plan), three launches -- shift, sweep, merge
// -- and one copy back (mhx_pointwise_kernels.h, DESIGN.md 6.5.7)

// data rows per tile where option POINTWISE_ROWS does not say: the fastest measured per width (DESIGN.md section 7; section 6.5.7 has
// the register table) -- fp64: 8 ahead of 4 by 10 % at 2 000 rows, level with it at 30; fp32: 4 ahead of 8 by 2 % and 8 %
#define MHX_POINTWISE_ROWS_DEFAULT (MHX_REAL64 ? 8 : 4)

// v is checked, nothing else is.  Nothing is written to shift, out5 or T unless the call succeeds.
static int pointwise_checked(const draws_view& v, const char* source, const mhx_real* rows, int64_t nrows, int32_t rowlen,
                             const mhx_real* data, size_t ndata, int32_t shift_given, double* shift, double* out5, int64_t* T)
{
    const char* who = v.who;
    mhx_ctx* ctx = v.ctx;
    if (!source || !rows || !shift || !out5) return mhx_fail(MHX_EINVAL, "%s: NULL argument", who);
    if (int rc = row_blocks_checked(v, nrows, rowlen, data, ndata)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const int R = opt_int(ctx, "POINTWISE_ROWS", MHX_POINTWISE_ROWS_DEFAULT);
    if (R != 2 && R != 4 && R != 8 && R != 16) return mhx_fail(MHX_EINVAL, "%s: option POINTWISE_ROWS = %d is not 2, 4, 8 or 16", who, R);
    hipFunction_t f_sweep = nullptr, f_shift = nullptr, f_merge = nullptr;
    int rc = user_module(v, "pointwise.hip", "function", source, {{"MHX_HAVE_POINTWISE", "mhx_pointwise_kernels.h"}},
                         {"MHX_JIT_POINTWISE_ROWS=" + std::to_string(R)},
                         {{"mhx_jit_pointwise", &f_sweep}, {"mhx_jit_pointwise_shift", &f_shift}, {"mhx_jit_pointwise_merge", &f_merge}});
    if (rc) return rc;
    const long ntiles = ((long)nrows + R - 1) / R;
    if (ntiles > 65535) return mhx_fail(MHX_EINVAL, "%s: %lld data rows are more than %d tiles of %d: fewer rows per call", who, (long long)nrows, 65535, R);
    const sweep_plan g = pointwise_sweep_plan(v, ntiles);
    const size_t P = (size_t)g.ncb * (size_t)g.slots, nr = (size_t)nrows;
    double *d_part = nullptr, *d_out = nullptr, *d_shift = nullptr;
    mhx_real *d_rows = nullptr, *d_data = nullptr;
    rc = scratch_carve(&ctx->select_scratch, &ctx->select_bytes, who, "pointwise scratch", [&](scratch_pieces& c) {
        d_part = c.take<double>(P * nr * 5);
        d_out = c.take<double>(nr * 5);
        d_shift = c.take<double>(nr);
        d_rows = c.take<mhx_real>(nr * (size_t)rowlen);
        d_data = c.take<mhx_real>(data_block_reals(ndata));
    });
    if (rc) { (void)hipGetLastError(); return rc; }
    HIP_TRY(hipMemcpyAsync(d_rows, rows, nr * (size_t)rowlen * sizeof(mhx_real), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = data_block_upload(ctx, d_data, data, ndata))) return rc;
    const int d = v.d1 - 1;
    const unsigned row_blocks = (unsigned)((nr + 63) / 64);
    if (shift_given) HIP_TRY(hipMemcpyAsync(d_shift, shift, nr * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    else rc = launch_module(f_shift, row_blocks, 64, ctx->stream, v.tensor, v.C, d, d_rows, (int)nrows, (int)rowlen, d_data, (int)ndata, d_shift);
    if (rc == MHX_OK)
        rc = launch_module(f_sweep, dim3((unsigned)g.ncb, (unsigned)g.slots, (unsigned)ntiles), MHX_POINTWISE_THREADS, ctx->stream, v.tensor, v.N,
                           v.C, d, d_rows, (int)nrows, (int)rowlen, d_data, (int)ndata, d_shift, d_part);
    if (rc == MHX_OK) rc = launch_module(f_merge, row_blocks, 64, ctx->stream, d_part, (long)P, (int)nrows, d_out);
    if (rc) return rc;
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
