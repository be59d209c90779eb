// autocovariance sums host side (included by mhx_api.hip after mhx_api_hist.inc): the checks, the tile list, two launches per call on
// the context's select block, the sums back in one copy (mhx_acf_kernels.h, DESIGN.md section 6.5.4)

__global__ void __launch_bounds__(256)
k_acf_centre(const mhx_real* __restrict__ samples, const long N, const int d1, const long C, const int* __restrict__ params, const int P,
             const long c0, const long nc, double* __restrict__ mean, double* __restrict__ ss, unsigned long long* __restrict__ counters)
{
    mhx_acf_centre_body(samples, N, d1, C, params, P, c0, nc, mean, ss, counters);
}
template <int R>
__global__ void __launch_bounds__(64 * MHX_ACF_WAVES)
k_acf_tile(const mhx_real* __restrict__ samples, const long N, const int d1, const long C, const int* __restrict__ params, const long c0,
           const long nc, const int* __restrict__ tiles, const int ntiles, const int ngroups, const long ncb, const int normalise,
           const double* __restrict__ mean, const double* __restrict__ ss, double* __restrict__ out)
{
    mhx_acf_tile_body<R>(samples, N, d1, C, params, c0, nc, tiles, ntiles, ngroups, ncb, normalise, mean, ss, out);
}

// the lags of a tile, per width: the fastest of 8, 16 and 32 on the C2 tensor at lags 0..63 (DESIGN.md section 6.5.4: 16.3 ms against
// 18.7 and 34.9 in fp64, 10.5 ms against 13.4 and 31.0 in fp32); option ACF_R picks another
#if MHX_REAL64
#define MHX_ACF_R 16
#else
#define MHX_ACF_R 8
#endif

static int acf_check(const draws_view& v, const int32_t* params, int32_t nparams, const int32_t* lags, int32_t nlags, int64_t chain_begin,
                     int64_t chain_count, const double* acov)
{
    const char* who = v.who;
    const int64_t N = v.N, C = v.C;
    if (!acov) return mhx_fail(MHX_EINVAL, "%s: acov is NULL", who);
    if (N < 2) return mhx_fail(MHX_ESTATE, "%s: %lld draws per chain, an autocovariance needs at least 2", who, (long long)N);
    int rc = select_check_params(who, params, nparams, v.d1);
    if (rc) return rc;
    if (nparams > MHX_HIST_MAX_ROWS) return mhx_fail(MHX_EINVAL, "%s: %d rows in one call, at most %d", who, (int)nparams, MHX_HIST_MAX_ROWS);
    if (!lags || nlags <= 0) return mhx_fail(MHX_EINVAL, "%s: no lags", who);
    for (int j = 0; j < nlags; ++j) {
        if (lags[j] < 0 || lags[j] >= N)
            return mhx_fail(MHX_EINVAL, "%s: lag %d (entry %d) is not in [0, %lld)", who, (int)lags[j], j, (long long)N);
        if (j && lags[j] <= lags[j - 1])
            return mhx_fail(MHX_EINVAL, "%s: the lags must increase strictly: entry %d is %d after %d", who, j, (int)lags[j], (int)lags[j - 1]);
    }
    if (chain_begin < 0 || chain_begin >= C || chain_count < 0 || chain_count > C - chain_begin)
        return mhx_fail(MHX_EINVAL, "%s: chains [%lld, +%lld) are not within [0, %lld)", who, (long long)chain_begin, (long long)chain_count, (long long)C);
    if ((N + MHX_ACF_CHUNK - 1) / MHX_ACF_CHUNK > 65535)
        return mhx_fail(MHX_EINVAL, "%s: %lld draws per chain, at most %d", who, (long long)N, 65535 * MHX_ACF_CHUNK);
    return MHX_OK;
}

// the arguments are checked.  The caller's arrays are written last, after everything succeeded.
static int acf_compute(const draws_view& v, const int32_t* params, int P, const int32_t* lags, int nlags, long c0, long nc, int normalise,
                       double* acov, int64_t* nvalid)
{
    mhx_ctx* ctx = v.ctx;
    const char* who = v.who;
    const mhx_real* tensor = v.tensor;
    const long N = v.N, C = v.C;
    const int d1 = v.d1;
    HIP_TRY(hipSetDevice(ctx->device));
    if (nc == 0) nc = C - c0;
    int R = opt_int(ctx, "ACF_R", MHX_ACF_R);
    if (R != 8 && R != 16 && R != 32) return mhx_fail(MHX_EINVAL, "%s: option ACF_R = %d is not 8, 16 or 32", who, R);
    // the tiles that hold a listed lag, and where each lag lands in the compact output [P][ntiles][R]
    std::vector<int32_t> tiles;
    std::vector<size_t> where((size_t)nlags);
    for (int j = 0; j < nlags; ++j) {
        const int32_t k0 = lags[j] / R * R;
        if (tiles.empty() || tiles.back() != k0) tiles.push_back(k0);
        where[j] = (tiles.size() - 1) * (size_t)R + (size_t)(lags[j] - k0);
    }
    const size_t ntiles = tiles.size(), nout = (size_t)P * ntiles * R;
    const long ncb = (nc + 63) / 64;
    const long ngroups = ((long)ntiles + MHX_ACF_WAVES - 1) / MHX_ACF_WAVES;
    const long chunks = (N + MHX_ACF_CHUNK - 1) / MHX_ACF_CHUNK;
    if ((double)ncb * (double)ngroups * (double)P > 2147483647.0)
        return mhx_fail(MHX_EINVAL, "%s: %ld chain blocks x %ld tile groups x %d rows exceed one launch: ask for fewer lags or rows per call", who, ncb, ngroups, P);
    const size_t npc = (size_t)P * (size_t)nc;
    double *d_out = nullptr, *d_mean = nullptr, *d_ss = nullptr;
    int *d_par = nullptr, *d_tiles = nullptr;
    int rc = scratch_carve(&ctx->select_scratch, &ctx->select_bytes, who, "autocovariance scratch", [&](scratch_pieces& c) {
        d_out = c.take<double>(nout + 2 * (size_t)P);       // sums, then 2 P counters of the same size: one memset, one copy back
        d_mean = c.take<double>(npc);
        d_ss = c.take<double>(npc);                         // lag-0 sums
        d_par = c.take<int>(P);
        d_tiles = c.take<int>(ntiles);
    });
    if (rc) return rc;
    unsigned long long* d_cnt = (unsigned long long*)(d_out + nout);
    HIP_TRY(hipMemsetAsync(d_out, 0, (nout + 2 * (size_t)P) * sizeof(double), ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_par, params, (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_tiles, tiles.data(), ntiles * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_acf_centre, dim3((unsigned)((nc + 255) / 256), (unsigned)P), dim3(256), 0, ctx->stream, tensor, N, d1, C, d_par, P, c0, nc,
                       d_mean, d_ss, d_cnt);
    if (hipGetLastError() != hipSuccess) return mhx_fail(MHX_EHIP, "%s: k_acf_centre failed to launch", who);
    const dim3 grid((unsigned)(ncb * ngroups * P), (unsigned)chunks), block(64 * MHX_ACF_WAVES);
#define MHX_ACF_LAUNCH(RR)                                                                                                                  \
    hipLaunchKernelGGL(k_acf_tile<RR>, grid, block, 0, ctx->stream, tensor, N, d1, C, d_par, c0, nc, d_tiles, (int)ntiles, (int)ngroups, ncb, \
                       normalise ? 1 : 0, d_mean, d_ss, d_out)
    if (R == 8) MHX_ACF_LAUNCH(8);
    else if (R == 16) MHX_ACF_LAUNCH(16);
    else MHX_ACF_LAUNCH(32);
#undef MHX_ACF_LAUNCH
    if (hipGetLastError() != hipSuccess) return mhx_fail(MHX_EHIP, "%s: k_acf_tile failed to launch", who);
    std::vector<double> land(nout + 2 * (size_t)P);
    HIP_TRY(hipMemcpyAsync(land.data(), d_out, land.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const unsigned long long* cnt = (const unsigned long long*)(land.data() + nout);
    for (int i = 0; i < P; ++i) {
        const bool bad = cnt[P + i] != 0;                   // a non-finite draw among the chains read: the row has no answer
        for (int j = 0; j < nlags; ++j)
            acov[(size_t)i * nlags + j] = bad ? std::nan("") : land[(size_t)i * ntiles * R + where[j]];
        if (nvalid) nvalid[i] = bad ? 0 : (int64_t)cnt[i];
    }
    return MHX_OK;
}

// v is checked, nothing else is
static int acf_checked(const draws_view& v, const int32_t* params, int32_t nparams, const int32_t* lags, int32_t nlags, int64_t chain_begin,
                       int64_t chain_count, int32_t normalise, double* acov, int64_t* nvalid)
{
    int rc = acf_check(v, params, nparams, lags, nlags, chain_begin, chain_count, acov);
    return rc ? rc : acf_compute(v, params, nparams, lags, nlags, (long)chain_begin, (long)chain_count, normalise, acov, nvalid);
}

int api_ctx_autocovariance(mhx_ctx* ctx, const mhx_real* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const int32_t* params,
                           int32_t nparams, const int32_t* lags, int32_t nlags, int64_t chain_begin, int64_t chain_count, int32_t normalise,
                           double* acov, int64_t* nvalid)
{
    draws_view v;
    int rc = draws_of_ctx("mhx_ctx_autocovariance", ctx, d_tensor, n_samples, dim1, nchains, &v);
    return rc ? rc : acf_checked(v, params, nparams, lags, nlags, chain_begin, chain_count, normalise, acov, nvalid);
}

int api_run_autocovariance(mhx_run* r, const int32_t* params, int32_t nparams, const int32_t* lags, int32_t nlags, int64_t chain_begin,
                           int64_t chain_count, int32_t normalise, double* acov, int64_t* nvalid)
{
    draws_view v;
    int rc = draws_of_run("mhx_run_autocovariance", r, &v);
    return rc ? rc : acf_checked(v, params, nparams, lags, nlags, chain_begin, chain_count, normalise, acov, nvalid);
}
