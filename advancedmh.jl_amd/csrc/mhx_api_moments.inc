// cross moments host side (included by mhx_api.hip after mhx_api_diag.inc): sum_k y_i and sum_k y_i y_j of chosen rows of the draws
// on the fp64 matrix cores, on the context's cross block (mhx_cross_kernels.h, DESIGN.md section 6.5.1)

template <int G, bool DIAG>
__global__ void __launch_bounds__(64)
k_cross(const mhx_real* __restrict__ samples, const long N, const int d1, const long C, const int* __restrict__ rows,
        const double* __restrict__ shift, const mhx_real* __restrict__ zeros, const int ngroups, double* __restrict__ part,
        double* __restrict__ psum)
{
    mhx_cross_body<G, DIAG>(samples, N, d1, C, rows, shift, zeros, ngroups, part, psum);
}
__global__ void __launch_bounds__(1024)
k_cross_fold(const double* __restrict__ src, const int nsplit, const int W, double* __restrict__ dst)
{
    __shared__ double lds[16 * 64];
    mhx_cross_fold_body(src, nsplit, W, dst, lds);
}
__global__ void __launch_bounds__(256)
k_cross_reduce_tiles(const double* __restrict__ part, const int* __restrict__ tiles, const int nsplit, const int m, double* __restrict__ cross)
{
    mhx_cross_reduce_tiles_body(part, tiles, nsplit, m, cross);
}
__global__ void __launch_bounds__(256)
k_cross_reduce_sums(const double* __restrict__ psum, const int nsplit, const int m, double* __restrict__ sum)
{
    mhx_cross_reduce_sums_body(psum, nsplit, m, sum);
}

#define MHX_CROSS_SCRATCH_BYTES ((size_t)64 << 20)          // bound on the partial tiles of a call: the splits of K shrink to fit

static int cross_check(const draws_view& v, const int32_t* params, int32_t nparams, const double* shift, const double* sum,
                       const double* cross)
{
    const char* who = v.who;
    if (!sum || !cross) return mhx_fail(MHX_EINVAL, "%s: bad argument", who);
    int rc = select_check_params(who, params, nparams, v.d1);
    if (rc) return rc;
    if (shift)
        for (int i = 0; i < nparams; ++i)
            if (!std::isfinite(shift[i])) return mhx_fail(MHX_EINVAL, "%s: shift %d is not finite", who, i);
    return MHX_OK;
}

// the arguments are checked
static int cross_compute(const draws_view& v, const int32_t* params, int m, const double* shift, double* sum, double* cross)
{
    mhx_ctx* ctx = v.ctx;
    const char* who = v.who;
    const mhx_real* tensor = v.tensor;
    const long N = v.N, C = v.C;
    const int d1 = v.d1;
    HIP_TRY(hipSetDevice(ctx->device));
    const int T = (m + 15) / 16;
    const bool one = T <= MHX_CROSS_MAX_G;                  // one group: every tile pair in one wave
    const int G = one ? T : MHX_CROSS_SPLIT_G;
    const int ngroups = (T + G - 1) / G, ntiles = ngroups * G;
    const int npd = G * (G + 1) / 2, npo = G * G;
    const long ngp = (long)ngroups * (ngroups - 1) / 2;     // pairs of groups a < b
    const long nslots = (long)ngroups * npd + ngp * npo;
    // tile pair of every slot, in the order the kernels number them
    std::vector<int> tiles((size_t)nslots);
    {
        size_t k = 0;
        for (int gi = 0; gi < ngroups; ++gi)
            for (int a = 0; a < G; ++a)
                for (int b = a; b < G; ++b) tiles[k++] = ((gi * G + a) << 16) | (gi * G + b);
        for (int ga = 0; ga < ngroups; ++ga)
            for (int gb = ga + 1; gb < ngroups; ++gb)
                for (int a = 0; a < G; ++a)
                    for (int b = 0; b < G; ++b) tiles[k++] = ((ga * G + a) << 16) | (gb * G + b);
    }
    std::vector<int> rows((size_t)ntiles * 16, -1);
    std::vector<double> sh((size_t)ntiles * 16, 0.0);
    for (int i = 0; i < m; ++i) { rows[i] = params[i]; sh[i] = shift ? shift[i] : 0.0; }
    // splits of K: units of CH chains dealt to enough waves for the chip (one wave per SIMD at G = 7, more where the accumulators
    // leave room), within the scratch bound
    const long CH = MHX_CROSS_CH(G), U = (C + CH - 1) / CH, total = N * U;
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    if (cus < 1) cus = 1;
    const long waves = (long)cus * 4 * (G <= 2 ? 4 : G <= 4 ? 2 : 1);
    long nsplit = std::min<long>(total, std::max<long>(1, waves / std::max<long>(1, one ? 1 : ngroups)));
    nsplit = std::min<long>(nsplit, std::max<long>(1, (long)(MHX_CROSS_SCRATCH_BYTES / ((size_t)nslots * 256 * sizeof(double)))));
    nsplit = std::min<long>(nsplit, 65535);
    const size_t n_cross = (size_t)m * m;
    double *d_part = nullptr, *d_psum = nullptr, *d_ft = nullptr, *d_fs = nullptr, *d_cross = nullptr, *d_sh = nullptr, *d_zero = nullptr;
    int *d_rows = nullptr, *d_tiles = nullptr;
    int rc = scratch_carve(&ctx->cross_scratch, &ctx->cross_bytes, who, "partial-tile scratch", [&](scratch_pieces& c) {
        d_part = c.take<double>((size_t)nslots * nsplit * 256);        // partial tiles
        d_psum = c.take<double>((size_t)ntiles * nsplit * 64);         // partial sums
        d_ft = c.take<double>((size_t)nslots * 256);                   // folded tiles
        d_fs = c.take<double>((size_t)ntiles * 64);                    // folded sums
        d_cross = c.take<double>(n_cross + (size_t)m);                 // cross, then sum: one copy back
        d_sh = c.take<double>(sh.size());                              // the rows' shifts
        d_zero = c.take<double>(32);
        d_rows = c.take<int>(rows.size());
        d_tiles = c.take<int>(tiles.size());
    });
    if (rc) return rc;
    double* d_sum = d_cross + n_cross;
    HIP_TRY(hipMemsetAsync(d_zero, 0, 32 * sizeof(double), ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_sh, sh.data(), sh.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // the host vectors are pageable: the copies have read them
#define MHX_CROSS_LAUNCH(GG, DIAG, NY)                                                                                          \
    hipLaunchKernelGGL((k_cross<GG, DIAG>), dim3((unsigned)nsplit, (unsigned)(NY)), dim3(64), 0, ctx->stream, tensor, N, d1, C, d_rows,  \
                       d_sh, (const mhx_real*)d_zero, ngroups, d_part, d_psum)
    if (!one) {
        MHX_CROSS_LAUNCH(MHX_CROSS_SPLIT_G, true, ngroups);
        MHX_CROSS_LAUNCH(MHX_CROSS_SPLIT_G, false, ngp);
    } else switch (G) {
        case 1: MHX_CROSS_LAUNCH(1, true, 1); break;
        case 2: MHX_CROSS_LAUNCH(2, true, 1); break;
        case 3: MHX_CROSS_LAUNCH(3, true, 1); break;
        case 4: MHX_CROSS_LAUNCH(4, true, 1); break;
        case 5: MHX_CROSS_LAUNCH(5, true, 1); break;
        case 6: MHX_CROSS_LAUNCH(6, true, 1); break;
        default: MHX_CROSS_LAUNCH(7, true, 1); break;
    }
#undef MHX_CROSS_LAUNCH
    hipLaunchKernelGGL(k_cross_fold, dim3((unsigned)nslots, 4), dim3(64, 16), 0, ctx->stream, d_part, (int)nsplit, 256, d_ft);
    hipLaunchKernelGGL(k_cross_fold, dim3((unsigned)ntiles, 1), dim3(64, 16), 0, ctx->stream, d_psum, (int)nsplit, 64, d_fs);
    hipLaunchKernelGGL(k_cross_reduce_tiles, dim3((unsigned)nslots), dim3(256), 0, ctx->stream, d_ft, d_tiles, 1, m, d_cross);
    hipLaunchKernelGGL(k_cross_reduce_sums, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, d_fs, 1, m, d_sum);
    if (hipGetLastError() != hipSuccess) return mhx_fail(MHX_EHIP, "%s: k_cross failed to launch", who);
    // nothing reaches the caller's arrays unless the whole call succeeded
    std::vector<double> h(n_cross + (size_t)m);
    if (hipMemcpyAsync(h.data(), d_cross, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
        return mhx_fail(MHX_EHIP, "%s: k_cross failed", who);
    memcpy(cross, h.data(), n_cross * sizeof(double));
    memcpy(sum, h.data() + n_cross, (size_t)m * sizeof(double));
    return MHX_OK;
}

// v is checked, nothing else is
static int cross_checked(const draws_view& v, const int32_t* params, int32_t nparams, const double* shift, double* sum, double* cross)
{
    int rc = cross_check(v, params, nparams, shift, sum, cross);
    return rc ? rc : cross_compute(v, params, nparams, shift, sum, cross);
}

int api_ctx_cross_moments(mhx_ctx* ctx, const mhx_real* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const int32_t* params,
                          int32_t nparams, const double* shift, double* sum, double* cross)
{
    draws_view v;
    int rc = draws_of_ctx("mhx_ctx_cross_moments", ctx, d_tensor, n_samples, dim1, nchains, &v);
    return rc ? rc : cross_checked(v, params, nparams, shift, sum, cross);
}

int api_run_cross_moments(mhx_run* r, const int32_t* params, int32_t nparams, const double* shift, double* sum, double* cross, int64_t* n_draws)
{
    draws_view v;
    int rc = draws_of_run("mhx_run_cross_moments", r, &v);
    if (!rc) rc = cross_checked(v, params, nparams, shift, sum, cross);
    if (!rc && n_draws) *n_draws = (int64_t)v.S();
    return rc;
}
