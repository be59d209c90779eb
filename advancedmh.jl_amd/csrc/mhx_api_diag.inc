// diagnostics host side (included by mhx_api.hip after draws_view, scratch_carve, sweep_blocks and dev_array): the moment sums and
// Geyer ESS, the rank-normalised diagnostics (per-call device memory, dev_array), and the exact order statistics, whose passes
// carve the context's select block (DESIGN.md section 6.5)

__global__ void __launch_bounds__(256)
k_diag_moments(const mhx_real* __restrict__ samples, const long N, const int d1, const long C, double* __restrict__ mean,
               double* __restrict__ sums)
{
    __shared__ double red[12];
    mhx_diag_moments_body(samples, N, d1, C, mean, sums, red);
}
__global__ void __launch_bounds__(64)
k_diag_autocov(const mhx_real* __restrict__ samples, const long N, const int d1, const long C, const long nc, const long k0,
               const double* __restrict__ mean, double* __restrict__ acov)
{
    mhx_diag_autocov_body(samples, N, d1, C, nc, k0, mean, acov);
}
__global__ void __launch_bounds__(256)
k_diag_between(const double* __restrict__ mean, const double* __restrict__ sums, const int d1, const long C, const double M,
               double* __restrict__ between)
{
    __shared__ double red[4];
    mhx_diag_between_body(mean, sums, d1, C, M, between, red);
}

__global__ void __launch_bounds__(256)
k_diag_from_moments(const mhx_real* __restrict__ mom_mean, const mhx_real* __restrict__ mom_m2, const long nsamp, const int d1,
                    const long C, double* __restrict__ sums)
{
    __shared__ double red[12];
    mhx_diag_from_moments_body(mom_mean, mom_m2, nsamp, d1, C, sums, red);
}

// Geyer's initial positive (monotone) sequence on the multi-chain autocorrelations
//   rho_t = 1 - (W - A_t) / var+     (A_t: chain-averaged autocovariance, W = A_0; Vehtari et al. 2021, eq. 10)
// which is A_t / A_0 for a single chain (var+ == W)
// A row without variance (a parameter that never moved) or with a non-finite draw has no autocorrelation: NaN, not tau = 1.
static double geyer_tau(const double* acov, long nlag, long stride, double varp, bool* truncated)
{
    const double g0 = acov[0];
    if (!(g0 > 0.0) || !(varp > 0.0)) { *truncated = false; return std::nan(""); }
    *truncated = true;
    double tau = -1.0, prev = 1e300;
    for (long m = 0; 2 * m + 1 < nlag; ++m) {
        double pm = (1.0 - (g0 - acov[(2 * m) * stride]) / varp) + (1.0 - (g0 - acov[(2 * m + 1) * stride]) / varp);
        if (!(pm > 0.0)) { *truncated = false; break; }
        if (pm > prev) pm = prev;
        prev = pm;
        tau += 2.0 * pm;
    }
    return tau < 1e-3 ? 1e-3 : tau;
}

// sums / ESS of the draws v on the device (or of running moments: mom_mean/mom_m2 [d1][C], v.N draws behind them)
static int diag_compute(const draws_view& v, const mhx_diag_cfg* cfg, const mhx_real* mom_mean, const mhx_real* mom_m2, double* sum_m,
                        double* sum_m2, double* sum_v, double* ess)
{
    mhx_ctx* ctx = v.ctx;
    const int d1 = v.d1;
    const long C = v.C;
    const bool moments_mode = mom_mean != nullptr;
    const bool split = cfg->split != 0 && !moments_mode;
    if (split && v.N < 4) return mhx_fail(MHX_ESTATE, "mhx_run_diagnostics: split chains need >= 4 draws");
    const long N = split ? v.N / 2 : v.N;                      // draws per (half-)chain
    const int nparts = split ? 2 : 1;                          // half-chains per chain
    dev_array<double> d_mean, d_sums, d_acov;
    std::vector<double> h(3 * (size_t)d1);
    if (!d_mean.alloc((size_t)nparts * d1 * C) || !d_sums.alloc(3 * (size_t)d1)) return mhx_fail(MHX_ENOMEM, "diagnostics scratch");
    (void)hipMemsetAsync(d_sums.p, 0, 3 * (size_t)d1 * sizeof(double), ctx->stream);
    if (moments_mode)
        hipLaunchKernelGGL(k_diag_from_moments, dim3((unsigned)((C + 255) / 256), d1), dim3(256), 0, ctx->stream,
                           mom_mean, mom_m2, N, d1, C, d_sums.p);
    else
        for (int part = 0; part < nparts; ++part)              // the sums of the half-chains add up
            hipLaunchKernelGGL(k_diag_moments, dim3((unsigned)((C + 255) / 256), d1), dim3(256), 0, ctx->stream,
                               v.tensor + (size_t)part * N * d1 * C, N, d1, C, d_mean.p + (size_t)part * d1 * C, d_sums.p);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return mhx_fail(MHX_EHIP, "k_diag_moments failed");
    if (hipMemcpyAsync(h.data(), d_sums.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return mhx_fail(MHX_EHIP, "D2H");
    for (int p = 0; p < d1; ++p) {
        if (sum_m) sum_m[p] = h[p];
        if (sum_m2) sum_m2[p] = h[d1 + p];
        if (sum_v) sum_v[p] = h[2 * (size_t)d1 + p];
    }
    if (!ess) return MHX_OK;
    long nlag = cfg->max_lag < 1 ? 0 : (long)cfg->max_lag + 1;
    if (nlag > N) nlag = N;
    nlag &= ~1L;                                            // pairs
    if (moments_mode || nlag < 2) {                         // no draws kept, or no pair of lags: autocovariances are not available
        for (int p = 0; p < d1; ++p) ess[p] = std::nan("");
        return MHX_OK;
    }
    const long nc = cfg->ess_chains <= 0 ? C : (cfg->ess_chains < C ? cfg->ess_chains : C);
    // d_acov: nlag rows of autocovariance sums, then one row of sum_c (m_c - mean of the m_c)^2
    if (!d_acov.alloc((size_t)(nlag + 1) * d1)) return mhx_fail(MHX_ENOMEM, "autocov scratch");
    (void)hipMemsetAsync(d_acov.p, 0, (size_t)(nlag + 1) * d1 * sizeof(double), ctx->stream);
    const double M = (double)C * nparts, Mnc = (double)nc * nparts;
    for (int part = 0; part < nparts; ++part)
        hipLaunchKernelGGL(k_diag_between, dim3((unsigned)((C + 255) / 256), d1), dim3(256), 0, ctx->stream,
                           d_mean.p + (size_t)part * d1 * C, d_sums.p, d1, C, M, d_acov.p + (size_t)nlag * d1);
    // grid.z holds the lags: long chains (max_lag of half a chain) need more lags than one launch may have
    int zmax = 0;
    if (hipDeviceGetAttribute(&zmax, hipDeviceAttributeMaxGridDimZ, ctx->device) != hipSuccess || zmax < 1) zmax = 65535;
    for (int part = 0; part < nparts; ++part)
        for (long k0 = 0; k0 < nlag; k0 += zmax)
            hipLaunchKernelGGL(k_diag_autocov, dim3((unsigned)((nc + 63) / 64), d1, (unsigned)std::min<long>(nlag - k0, zmax)), dim3(64),
                               0, ctx->stream, v.tensor + (size_t)part * N * d1 * C, N, d1, C, nc, k0,
                               d_mean.p + (size_t)part * d1 * C, d_acov.p);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return mhx_fail(MHX_EHIP, "k_diag_autocov failed");
    std::vector<double> ac((size_t)(nlag + 1) * d1);
    if (hipMemcpyAsync(ac.data(), d_acov.p, ac.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return mhx_fail(MHX_EHIP, "D2H");
    for (int p = 0; p < d1; ++p) {
        // chain-averaged autocovariances with the N/(N-1) factor that makes lag 0 the within variance
        for (long k = 0; k < nlag; ++k) ac[(size_t)k * d1 + p] /= Mnc * (double)(N - 1);
        const double W = h[2 * (size_t)d1 + p] / M;
        const double Vm = M > 1.0 ? ac[(size_t)nlag * d1 + p] / (M - 1.0) : 0.0;
        const double varp = (double)(N - 1) / (double)N * W + Vm;
        // the subset's own within variance stands in for W, so that rho_0 = 1 - (A_0 - A_0)/var+ = 1
        bool trunc = false;
        const double tau = geyer_tau(ac.data() + p, nlag, d1, M > 1.0 ? varp : ac[p], &trunc);
        // total ESS = M N / tau; negative sign marks a sum that was still positive at max_lag
        // (tau is then a lower bound, ESS an upper bound)
        const double e = M * (double)N / tau;
        ess[p] = trunc ? -e : e;
    }
    return MHX_OK;
}

int api_run_diagnostics(mhx_run* r, const mhx_diag_cfg* cfg, double* sum_m, double* sum_m2,
                                   double* sum_v, double* ess)
{
    if (!r || !cfg) return mhx_fail(MHX_EINVAL, "mhx_run_diagnostics: NULL argument");
    if (r->n_saved < 2) return mhx_fail(MHX_ESTATE, "mhx_run_diagnostics: needs a sample buffer with >= 2 draws");
    HIP_TRY(hipSetDevice(r->ctx->device));
    // (not draws_of_run: a run in moments mode has no tensor and is served from its running moments)
    return diag_compute(draws_view{r->ctx, r->d_samples, (long)r->n_saved, (long)r->n, r->dim + 1, "mhx_run_diagnostics"}, cfg,
                        r->moments_mode ? r->d_mom_mean : nullptr, r->d_mom_m2, sum_m, sum_m2, sum_v, ess);
}

// the one parameter-range check of the post-run statistics: rows [0, d1) of the tensor
static int select_check_params(const char* who, const int32_t* params, int32_t nparams, int d1)
{
    if (!params || nparams <= 0) return mhx_fail(MHX_EINVAL, "%s: no parameters", who);
    for (int i = 0; i < nparams; ++i)
        if (params[i] < 0 || params[i] >= d1) return mhx_fail(MHX_EINVAL, "%s: parameter %d out of range [0, %d)", who, (int)params[i], d1);
    return MHX_OK;
}

// ---- rank-normalised diagnostics (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021, sections 4.1-4.3) ----
// One parameter at a time: its N C draws are sorted on the device (rocPRIM radix sort, keys = values, payload = position), every draw
// is replaced by the normal score of its rank, z = Phi^-1((rank - 3/8) / (S + 1/4)), and by the indicators of the 5 % / 95 %
// quantiles; the multi-chain sums and ESS above then run on those series.  Folded scores (for the tail R-hat) come by search in the
// same sorted array (mhx_diag_fold_rank: no second sort).
__global__ void __launch_bounds__(256)
k_diag_gather_param(const mhx_real* __restrict__ samples, const long N, const int d1, const long C, const int p,
                    mhx_real* __restrict__ keys, unsigned* __restrict__ pos)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N * C) return;
    const long t = e / C, c = e - t * C;
    keys[e] = samples[(t * d1 + p) * C + c];
    pos[e] = (unsigned)e;
}

// The normal score of a tie-averaged rank, z = Phi^-1((rank - 3/8) / (S + 1/4)), to a few ulp of fp64 over the whole range.
// The plain form (k_diag_rank_scores<false>) rounds p in double and inverts it: p carries an ABSOLUTE rounding error of 2^-54 near
// 1/2 and 2^-53 near 1, which Phi^-1 returns magnified by 1 / phi(z) -- thousands of ulp of a score near zero, hundreds at the top
// score.  Here the argument is always a quotient of two exactly representable numbers (rank is a multiple of 1/2, S < 2^32) and
// small where z is small:
//   |p - 1/2| <= 1/4   z = sqrt2 erfinv(2 q),  q = p - 1/2 = (rank - (S + 1) / 2) / (S + 1/4)
//   else               z = -+ sqrt2 erfcinv(2 t), t = the tail probability (rank - 3/8) / (S + 1/4) or (S - rank + 5/8) / (S + 1/4)
// Both inverses are well conditioned on their range (relative condition number below 1.2).
MHX_DEV double diag_normal_score(const double rank, const long S)
{
    const double den = (double)S + 0.25, a = rank - 0.5 * ((double)S + 1.0);
    const double sqrt2 = 1.4142135623730951;
    if (fabs(a) <= 0.25 * den) return sqrt2 * erfinv(2.0 * (a / den));
    const double t = (a < 0.0 ? rank - 0.375 : (double)S - rank + 0.625) / den;
    const double z = sqrt2 * erfcinv(2.0 * t);
    return a < 0.0 ? -z : z;
}

// WC false: the score as mhx_run_ess_bulk_tail has always taken it (its results are pinned bit for bit by its own test, and it is the
// yardstick of tools/bench_rank_diag.py); true: diag_normal_score, for mhx_run_rank_diagnostics and mhx_run_rank_scores
template <bool WC>
__global__ void __launch_bounds__(256)
k_diag_rank_scores(const mhx_real* __restrict__ sorted, const unsigned* __restrict__ pos, const long S, const mhx_real q05,
                   const mhx_real q95, mhx_real* __restrict__ z, mhx_real* __restrict__ lo, mhx_real* __restrict__ hi)
{
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= S) return;
    const unsigned e = pos[r];
    // average rank over the run of equal draws (tiedrank, as MCMCDiagnosticTools / Vehtari et al. do): MH output is
    // mostly ties (a rejected step repeats the state), and ordinal ranks would give them distinct, time-ordered scores
    const mhx_real key = sorted[r];
    long a0 = 0, a1 = r;                                   // first index with sorted[i] == key
    while (a0 < a1) { const long mid = (a0 + a1) >> 1; if (sorted[mid] < key) a0 = mid + 1; else a1 = mid; }
    const long first = a0;
    a0 = r; a1 = S - 1;                                    // last index with sorted[i] == key
    while (a0 < a1) { const long mid = (a0 + a1 + 1) >> 1; if (sorted[mid] > key) a1 = mid - 1; else a0 = mid; }
    const double rank = 0.5 * ((double)first + (double)a0) + 1.0;
    if constexpr (WC) z[e] = (mhx_real)diag_normal_score(rank, S);
    else z[e] = (mhx_real)normcdfinv((rank - 0.375) / ((double)S + 0.25));
    lo[e] = key <= q05 ? MHX_R(1.0) : MHX_R(0.0);
    hi[e] = key <= q95 ? MHX_R(1.0) : MHX_R(0.0);
}

__global__ void __launch_bounds__(256)
k_diag_fold_scores(const mhx_real* __restrict__ sorted, const unsigned* __restrict__ pos, const long S, const mhx_real m,
                   mhx_real* __restrict__ z)
{
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= S) return;
    const double rank = mhx_diag_fold_rank(sorted, S, m, r);
    z[pos[r]] = (mhx_real)diag_normal_score(rank, S);
}

// per-call device memory of the rank path
struct rank_scratch {
    dev_array<mhx_real> k0, k1, series;             // series: bulk scores | 5 % indicator | 95 % indicator [| folded scores]
    dev_array<unsigned> p0, p1;
    dev_array<char> tmp;
    size_t tmp_bytes = 0;
};

// the draws of a run that has at least 4 of them per chain and fewer than 2^32 per row (positions travel as 32-bit payload)
static int rank_check(const mhx_run* r, const char* who, draws_view* v)
{
    if (r->moments_mode || r->n_saved < 4) return mhx_fail(MHX_ESTATE, "%s: needs a sample buffer with >= 4 draws", who);
    if ((long)r->n_saved * (long)r->n >= (1L << 32)) return mhx_fail(MHX_EINVAL, "%s: more than 2^32 draws per parameter", who);
    *v = draws_view{r->ctx, r->d_samples, (long)r->n_saved, (long)r->n, r->dim + 1, who};
    return MHX_OK;
}

static int rank_scratch_alloc(mhx_ctx* ctx, long S, int nseries, rank_scratch* w)
{
    if (!w->k0.alloc(S) || !w->k1.alloc(S) || !w->p0.alloc(S) || !w->p1.alloc(S) || !w->series.alloc((size_t)nseries * S))
        return mhx_fail(MHX_ENOMEM, "rank diagnostics scratch");
    if (rocprim::radix_sort_pairs(nullptr, w->tmp_bytes, w->k0.p, w->k1.p, w->p0.p, w->p1.p, (size_t)S, 0, 8 * (unsigned)sizeof(mhx_real), ctx->stream) != hipSuccess ||
        !w->tmp.alloc(w->tmp_bytes ? w->tmp_bytes : 1)) return mhx_fail(MHX_ENOMEM, "radix sort scratch");
    return MHX_OK;
}

// what the host reads of a sorted row, in ONE synchronisation: the 5 % and 95 % order statistics, the two ends, the middle pair
struct rank_row {
    mhx_real q05, q95, first, last, median;
    bool has_nan;
};

// gather row p, sort it (k1 / p1: ascending keys and their [t][c] positions) and fetch rank_row -- the middle pair only for a caller that
// folds (every copy to pageable memory is a round trip of its own, and mhx_run_ess_bulk_tail never made these two)
static int rank_sort_row(const draws_view& v, rank_scratch* w, int p, bool median, rank_row* out)
{
    mhx_ctx* ctx = v.ctx;
    const long S = (long)v.S();
    hipLaunchKernelGGL(k_diag_gather_param, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, v.tensor, v.N, v.d1, v.C, p,
                       w->k0.p, w->p0.p);
    if (rocprim::radix_sort_pairs(w->tmp.p, w->tmp_bytes, w->k0.p, w->k1.p, w->p0.p, w->p1.p, (size_t)S, 0, 8 * (unsigned)sizeof(mhx_real), ctx->stream) != hipSuccess)
        return mhx_fail(MHX_EHIP, "radix sort failed");
    const long at[6] = {(long)(0.05 * (double)(S - 1)), (long)(0.95 * (double)(S - 1)), 0, S - 1, (S - 1) / 2, S / 2};
    mhx_real q[6] = {};
    for (int j = 0; j < (median ? 6 : 4); ++j)
        if (hipMemcpyAsync(&q[j], w->k1.p + at[j], sizeof(mhx_real), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            return mhx_fail(MHX_EHIP, "quantile copy failed");
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return mhx_fail(MHX_EHIP, "quantile copy failed");
    out->q05 = q[0]; out->q95 = q[1]; out->first = q[2]; out->last = q[3];
    // Julia's middle(): the middle draw of an odd S, else half of each of the middle pair added in the run's width
    out->median = !median ? (mhx_real)std::nan("") : (S & 1) ? q[4] : q[4] / MHX_R(2.0) + q[5] / MHX_R(2.0);
    // the bit order of the sort puts a NaN at an end (sign set: first, sign clear: last): such a row has no ranks, and no search is
    // launched on it
    out->has_nan = q[2] != q[2] || q[3] != q[3];
    return MHX_OK;
}

template <bool WC>
static void rank_launch_bulk(mhx_ctx* ctx, rank_scratch* w, long S, const rank_row& row)
{
    hipLaunchKernelGGL(k_diag_rank_scores<WC>, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, w->k1.p, w->p1.p, S, row.q05,
                       row.q95, w->series.p, w->series.p + S, w->series.p + 2 * S);
}
static void rank_launch_fold(mhx_ctx* ctx, rank_scratch* w, long S, const rank_row& row)
{
    hipLaunchKernelGGL(k_diag_fold_scores, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, w->k1.p, w->p1.p, S, row.median,
                       w->series.p + 3 * S);
}

// series j of the rank scratch as draws [N][1][C]
static draws_view rank_series(const draws_view& v, const rank_scratch& w, int j)
{
    return draws_view{v.ctx, w.series.p + (size_t)j * v.S(), v.N, v.C, 1, v.who};
}

// the smaller of the two quantile ESS values; a truncated (negated) one keeps its sign (an indicator that is constant has no ESS:
// NaN, whichever of the two it is)
static double tail_ess(double e05, double e95)
{
    return e05 != e05 || e95 != e95 ? std::nan("") : std::fabs(e05) < std::fabs(e95) ? e05 : e95;
}

int api_run_ess_bulk_tail(mhx_run* r, const mhx_diag_cfg* cfg, const int32_t* params, int32_t nparams,
                                     double* ess_bulk, double* ess_tail)
{
    const char* who = "mhx_run_ess_bulk_tail";
    if (!r || !cfg || !params || nparams <= 0) return mhx_fail(MHX_EINVAL, "%s: bad argument", who);
    draws_view v;
    int rc = rank_check(r, who, &v);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(v.ctx->device));
    if ((rc = select_check_params(who, params, nparams, v.d1))) return rc;
    const long S = (long)v.S();
    rank_scratch w;
    if ((rc = rank_scratch_alloc(v.ctx, S, 3, &w))) return rc;
    for (int i = 0; i < nparams; ++i) {
        rank_row row;
        if ((rc = rank_sort_row(v, &w, params[i], false, &row))) return rc;
        if (row.has_nan) {
            if (ess_bulk) ess_bulk[i] = std::nan("");
            if (ess_tail) ess_tail[i] = std::nan("");
            continue;
        }
        rank_launch_bulk<false>(v.ctx, &w, S, row);
        if (hipGetLastError() != hipSuccess) return mhx_fail(MHX_EHIP, "k_diag_rank_scores failed");
        double e[3];
        for (int j = 0; j < 3; ++j)
            if ((rc = diag_compute(rank_series(v, w, j), cfg, nullptr, nullptr, nullptr, nullptr, nullptr, &e[j]))) return rc;
        if (ess_bulk) ess_bulk[i] = e[0];
        if (ess_tail) ess_tail[i] = tail_ess(e[1], e[2]);
    }
    return MHX_OK;
}

// R-hat = sqrt(var+ / W) from the three sums over M (half-)chains of n draws (include/mhx.h); W == 0: NaN (Vm == 0) or +inf
static double rhat_from_sums(double sum_m, double sum_m2, double sum_v, double M, double n)
{
    if (!(M > 1.0)) return std::nan("");
    const double W = sum_v / M;
    const double Vm = std::fmax((sum_m2 - sum_m * sum_m / M) / (M - 1.0), 0.0);
    return std::sqrt(((n - 1.0) / n * W + Vm) / W);
}

// rank-normalised split R-hat, bulk and folded (section 4.1), and the bulk / tail ESS, from the same one sort
int api_run_rank_diagnostics(mhx_run* r, const mhx_diag_cfg* cfg, const int32_t* params, int32_t nparams, double* ess_bulk,
                             double* ess_tail, double* rhat_bulk, double* rhat_tail)
{
    const char* who = "mhx_run_rank_diagnostics";
    if (!r || !cfg || !params || nparams <= 0) return mhx_fail(MHX_EINVAL, "%s: bad argument", who);
    draws_view v;
    int rc = rank_check(r, who, &v);
    if (rc) return rc;
    mhx_ctx* ctx = v.ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = select_check_params(who, params, nparams, v.d1))) return rc;
    const long N = v.N, C = v.C, S = (long)v.S();
    const bool want_ess = ess_bulk || ess_tail;
    const double nparts = cfg->split ? 2.0 : 1.0, M = (double)C * nparts, n = (double)(cfg->split ? N / 2 : N);
    const double nan = std::nan("");
    rank_scratch w;
    if ((rc = rank_scratch_alloc(ctx, S, 4, &w))) return rc;
    for (int i = 0; i < nparams; ++i) {
        rank_row row;
        if ((rc = rank_sort_row(v, &w, params[i], true, &row))) return rc;
        if (row.has_nan) {
            if (ess_bulk) ess_bulk[i] = nan;
            if (ess_tail) ess_tail[i] = nan;
            if (rhat_bulk) rhat_bulk[i] = nan;
            if (rhat_tail) rhat_tail[i] = nan;
            continue;
        }
        const bool fold = rhat_tail && std::isfinite(row.median);
        rank_launch_bulk<true>(ctx, &w, S, row);
        if (fold) rank_launch_fold(ctx, &w, S, row);
        if (hipGetLastError() != hipSuccess) return mhx_fail(MHX_EHIP, "%s: the score kernels failed to launch", who);
        // the bulk scores: their moments come with the ESS call (the ESS itself as mhx_run_ess_bulk_tail takes it)
        double e[3] = {nan, nan, nan}, sm = 0.0, sm2 = 0.0, sv = 0.0;
        if (want_ess || rhat_bulk)
            if ((rc = diag_compute(rank_series(v, w, 0), cfg, nullptr, nullptr, &sm, &sm2, &sv, want_ess ? &e[0] : nullptr))) return rc;
        if (rhat_bulk) rhat_bulk[i] = rhat_from_sums(sm, sm2, sv, M, n);
        if (want_ess) {
            for (int j = 1; j < 3; ++j)
                if ((rc = diag_compute(rank_series(v, w, j), cfg, nullptr, nullptr, nullptr, nullptr, nullptr, &e[j]))) return rc;
            if (ess_bulk) ess_bulk[i] = e[0];
            if (ess_tail) ess_tail[i] = tail_ess(e[1], e[2]);
        }
        if (rhat_tail) {
            rhat_tail[i] = nan;                             // a median that is not finite folds nothing
            if (fold) {
                if ((rc = diag_compute(rank_series(v, w, 3), cfg, nullptr, nullptr, &sm, &sm2, &sv, nullptr))) return rc;
                rhat_tail[i] = rhat_from_sums(sm, sm2, sv, M, n);
            }
        }
    }
    return MHX_OK;
}

int api_run_rank_scores(mhx_run* r, int32_t param, int32_t folded, mhx_real* out_host)
{
    const char* who = "mhx_run_rank_scores";
    if (!r || !out_host) return mhx_fail(MHX_EINVAL, "%s: NULL argument", who);
    draws_view v;
    int rc = rank_check(r, who, &v);
    if (rc) return rc;
    if ((rc = select_check_params(who, &param, 1, v.d1))) return rc;
    mhx_ctx* ctx = v.ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const long S = (long)v.S();
    rank_scratch w;
    if ((rc = rank_scratch_alloc(ctx, S, 4, &w))) return rc;
    rank_row row;
    if ((rc = rank_sort_row(v, &w, param, true, &row))) return rc;
    if (row.has_nan || (folded && !std::isfinite(row.median))) {
        const mhx_real nan = (mhx_real)std::nan("");
        for (long e = 0; e < S; ++e) out_host[e] = nan;
        return MHX_OK;
    }
    if (folded) rank_launch_fold(ctx, &w, S, row);
    else rank_launch_bulk<true>(ctx, &w, S, row);
    if (hipGetLastError() != hipSuccess) return mhx_fail(MHX_EHIP, "%s: the score kernel failed to launch", who);
    HIP_TRY(hipMemcpyAsync(out_host, w.series.p + (folded ? 3 * (size_t)S : 0), (size_t)S * sizeof(mhx_real), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MHX_OK;
}

// ---- exact order statistics: histogram radix select on the tensor in place (DESIGN.md section 6.5) ----
// Three pre-built (digit width, groups per launch) forms; a pass of d digit bits runs on the narrowest that holds it.  LDS per
// block: groups << width counters of 4 bytes = 16, 64 and 64 KiB.
template <int BITS, int G>
__global__ void __launch_bounds__(MHX_SELECT_THREADS)
k_select_hist(const mhx_real* __restrict__ samples, const long N, const int d1, const long C, const int* __restrict__ params,
              const unsigned long long* __restrict__ prefixes, const int* __restrict__ ngroups, const int gstride, const int first,
              const int shift, const int digit_bits, const int top, const unsigned long long chunk, unsigned long long* __restrict__ hist)
{
    __shared__ unsigned lds[G << BITS];
    mhx_select_hist_body<BITS, G>(samples, N, d1, C, params, prefixes, ngroups, gstride, first, shift, digit_bits, top, chunk, hist, lds);
}

// what a pass reads: the draws and the rows asked for
struct select_source {
    draws_view v;
    const int32_t* params;
    int32_t nparams;
};

// one pass over one tensor: mhx_select_hist_fn of mhx_select.h (hist is host memory)
static int select_hist_pass(void* user, const uint64_t* prefixes, const int32_t* ngroups, int32_t gstride, int32_t shift,
                            int32_t digit_bits, uint64_t* hist)
{
    const select_source* s = (const select_source*)user;
    const draws_view& v = s->v;
    mhx_ctx* ctx = v.ctx;
    const int P = s->nparams;
    if (digit_bits < 1 || digit_bits > MHX_SELECT_MAX_DIGIT_BITS || shift < 0 || shift + digit_bits > MHX_KEY_BITS || gstride < 1)
        return mhx_fail(MHX_EINVAL, "%s: digit of %d bits at bit %d of a %d-bit key", v.who, (int)digit_bits, (int)shift, MHX_KEY_BITS);
    int gmax = 0;
    for (int i = 0; i < P; ++i) {
        if (ngroups[i] < 0 || ngroups[i] > gstride) return mhx_fail(MHX_EINVAL, "%s: %d groups in a stride of %d", v.who, (int)ngroups[i], (int)gstride);
        gmax = std::max(gmax, (int)ngroups[i]);
    }
    if (!gmax) return MHX_OK;
    if (shift + digit_bits == MHX_KEY_BITS && gmax > 1) return mhx_fail(MHX_EINVAL, "%s: the first pass has one group", v.who);
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t nh = ((size_t)P * gstride) << digit_bits, npf = (size_t)P * gstride;
    unsigned long long *d_hist = nullptr, *d_pf = nullptr;
    int *d_ng = nullptr, *d_par = nullptr;
    int rc = scratch_carve(&ctx->select_scratch, &ctx->select_bytes, v.who, "select scratch", [&](scratch_pieces& c) {
        d_hist = c.take<unsigned long long>(nh);            // histogram
        d_pf = c.take<unsigned long long>(npf);             // prefixes
        d_ng = c.take<int>(P);                              // group counts
        d_par = c.take<int>(P);                             // parameter rows
    });
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d_hist, 0, nh * sizeof(uint64_t), ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_pf, prefixes, npf * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_ng, ngroups, (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_par, s->params, (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    unsigned long long chunk = 0;
    const unsigned long long nblk = sweep_blocks(v.S(), P, &chunk);
    const int top = shift + digit_bits == MHX_KEY_BITS;
    const dim3 grid((unsigned)nblk, (unsigned)P), block(MHX_SELECT_THREADS);
#define MHX_SELECT_LAUNCH(BITS, G)                                                                                        \
    for (int first = 0; first < gmax; first += G)                                                                         \
        hipLaunchKernelGGL((k_select_hist<BITS, G>), grid, block, 0, ctx->stream, v.tensor, v.N, v.d1, v.C, d_par, d_pf, d_ng,    \
                           (int)gstride, first, (int)shift, (int)digit_bits, top, chunk, d_hist)
    if (digit_bits <= 8) { MHX_SELECT_LAUNCH(8, 16); }
    else if (digit_bits <= 10) { MHX_SELECT_LAUNCH(10, 16); }
    else { MHX_SELECT_LAUNCH(11, 8); }
#undef MHX_SELECT_LAUNCH
    if (hipGetLastError() != hipSuccess) return mhx_fail(MHX_EHIP, "%s: k_select_hist failed to launch", v.who);
    // only the groups in use travel: rows of gmax << digit_bits counters out of a pitch of gstride << digit_bits
    const size_t pitch = ((size_t)gstride << digit_bits) * sizeof(uint64_t), width = ((size_t)gmax << digit_bits) * sizeof(uint64_t);
    HIP_TRY(hipMemcpy2DAsync(hist, pitch, d_hist, pitch, width, (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MHX_OK;
}

// the context's page-locked landing buffer for the histograms of a call (they arrive by DMA once per pass): kept from call to
// call, grown on demand.  A host that cannot lock that much leaves the call to pageable memory.
static void select_landing(mhx_ctx* ctx, int digit, int32_t nparams, int32_t nranks)
{
    const size_t words = mhx_select_hist_words(digit, nparams, nranks);
    if (words <= ctx->select_landing_words) return;
    if (ctx->select_landing) (void)hipHostFree(ctx->select_landing);
    ctx->select_landing = nullptr; ctx->select_landing_words = 0;
    void* q = nullptr;
    if (hipSetDevice(ctx->device) == hipSuccess && mhx_host_alloc(words * sizeof(uint64_t), &q) == MHX_OK && q) {
        ctx->select_landing = (uint64_t*)q;
        ctx->select_landing_words = words;
    } else (void)hipGetLastError();
}

// ranks of the chosen rows of the draws v (everything but v is unchecked)
static int select_checked(const draws_view& v, const int32_t* params, int32_t nparams, const int64_t* ranks, int32_t nranks, double* out)
{
    if (!out || !ranks || nranks <= 0) return mhx_fail(MHX_EINVAL, "%s: bad argument", v.who);
    int rc = select_check_params(v.who, params, nparams, v.d1);
    if (rc) return rc;
    select_source src{v, params, nparams};
    const int digit = opt_int(v.ctx, "SELECT_BITS", MHX_SELECT_DIGIT_BITS);
    select_landing(v.ctx, digit, nparams, nranks);
    return mhx_select_drive(v.who, MHX_KEY_BITS, digit, nparams, ranks, nranks, v.S(), select_hist_pass, &src, out, v.ctx->select_landing,
                            v.ctx->select_landing_words);
}

int api_ctx_order_statistics(mhx_ctx* ctx, const mhx_real* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,
                             const int32_t* params, int32_t nparams, const int64_t* ranks, int32_t nranks, double* out)
{
    draws_view v;
    int rc = draws_of_ctx("mhx_ctx_order_statistics", ctx, d_tensor, n_samples, dim1, nchains, &v);
    return rc ? rc : select_checked(v, params, nparams, ranks, nranks, out);
}

int api_run_order_statistics(mhx_run* r, const int32_t* params, int32_t nparams, const int64_t* ranks, int32_t nranks, double* out)
{
    draws_view v;
    int rc = draws_of_run("mhx_run_order_statistics", r, &v);
    return rc ? rc : select_checked(v, params, nparams, ranks, nranks, out);
}

// the per-pass building block of the group form (mhx_group_order_statistics adds the members' histograms and scans once)
int api_run_select_histogram(mhx_run* r, const int32_t* params, int32_t nparams, const uint64_t* prefixes, const int32_t* ngroups,
                             int32_t gstride, int32_t shift, int32_t digit_bits, uint64_t* hist)
{
    draws_view v;
    int rc = draws_of_run("mhx_run_select_histogram", r, &v);
    if (rc) return rc;
    if (!prefixes || !ngroups || !hist) return mhx_fail(MHX_EINVAL, "%s: NULL argument", v.who);
    if ((rc = select_check_params(v.who, params, nparams, v.d1))) return rc;
    select_source src{v, params, nparams};
    return select_hist_pass(&src, prefixes, ngroups, gstride, shift, digit_bits, hist);
}
