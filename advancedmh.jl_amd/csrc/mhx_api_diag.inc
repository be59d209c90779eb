// diagnostics host side (included by mhx_api.hip)

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

// sums / ESS of a sample tensor [Nsaved][d1][C] on the device (or of running moments: mom_mean/mom_m2 [d1][C])
static int diag_compute(mhx_ctx* ctx, const mhx_real* d_samples, long Nsaved, int d1, long C, const mhx_diag_cfg* cfg,
                        const mhx_real* mom_mean, const mhx_real* mom_m2, double* sum_m, double* sum_m2, double* sum_v, double* ess)
{
    const bool moments_mode = mom_mean != nullptr;
    const bool split = cfg->split != 0 && !moments_mode;
    if (split && Nsaved < 4) return mhx_fail(MHX_ESTATE, "mhx_run_diagnostics: split chains need >= 4 draws");
    const long N = split ? Nsaved / 2 : Nsaved;                // draws per (half-)chain
    const int nparts = split ? 2 : 1;                          // half-chains per chain
    double *d_mean = nullptr, *d_sums = nullptr, *d_acov = nullptr;
    int rc = MHX_OK;
    std::vector<double> h(3 * (size_t)d1);
    do {
        if (hipMalloc(&d_mean, (size_t)nparts * d1 * C * sizeof(double)) != hipSuccess ||
            hipMalloc(&d_sums, 3 * (size_t)d1 * sizeof(double)) != hipSuccess) { rc = mhx_fail(MHX_ENOMEM, "diagnostics scratch"); break; }
        (void)hipMemsetAsync(d_sums, 0, 3 * (size_t)d1 * sizeof(double), ctx->stream);
        if (moments_mode)
            hipLaunchKernelGGL(k_diag_from_moments, dim3((unsigned)((C + 255) / 256), d1), dim3(256), 0, ctx->stream,
                               mom_mean, mom_m2, N, d1, C, d_sums);
        else
            for (int part = 0; part < nparts; ++part)          // the sums of the half-chains add up
                hipLaunchKernelGGL(k_diag_moments, dim3((unsigned)((C + 255) / 256), d1), dim3(256), 0, ctx->stream,
                                   d_samples + (size_t)part * N * d1 * C, N, d1, C, d_mean + (size_t)part * d1 * C, d_sums);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = mhx_fail(MHX_EHIP, "k_diag_moments failed"); break; }
        if (hipMemcpyAsync(h.data(), d_sums, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = mhx_fail(MHX_EHIP, "D2H"); break; }
        for (int p = 0; p < d1; ++p) {
            if (sum_m) sum_m[p] = h[p];
            if (sum_m2) sum_m2[p] = h[d1 + p];
            if (sum_v) sum_v[p] = h[2 * (size_t)d1 + p];
        }
        if (ess && moments_mode) {
            for (int p = 0; p < d1; ++p) ess[p] = std::nan("");      // no draws kept: autocovariances are not available
        } else if (ess) {
            long nlag = cfg->max_lag < 1 ? 0 : (long)cfg->max_lag + 1;
            if (nlag > N) nlag = N;
            nlag &= ~1L;                                    // pairs
            long nc = cfg->ess_chains <= 0 ? C : (cfg->ess_chains < C ? cfg->ess_chains : C);
            if (nlag < 2) { for (int p = 0; p < d1; ++p) ess[p] = std::nan(""); break; }
            // d_acov: nlag rows of autocovariance sums, then one row of sum_c (m_c - mean of the m_c)^2
            if (hipMalloc(&d_acov, (size_t)(nlag + 1) * d1 * sizeof(double)) != hipSuccess) { rc = mhx_fail(MHX_ENOMEM, "autocov scratch"); break; }
            (void)hipMemsetAsync(d_acov, 0, (size_t)(nlag + 1) * d1 * sizeof(double), ctx->stream);
            const double M = (double)C * nparts, Mnc = (double)nc * nparts;
            for (int part = 0; part < nparts; ++part)
                hipLaunchKernelGGL(k_diag_between, dim3((unsigned)((C + 255) / 256), d1), dim3(256), 0, ctx->stream,
                                   d_mean + (size_t)part * d1 * C, d_sums, d1, C, M, d_acov + (size_t)nlag * d1);
            // grid.z holds the lags: long chains (max_lag of half a chain) need more lags than one launch may have
            int zmax = 0;
            if (hipDeviceGetAttribute(&zmax, hipDeviceAttributeMaxGridDimZ, ctx->device) != hipSuccess || zmax < 1) zmax = 65535;
            for (int part = 0; part < nparts; ++part)
                for (long k0 = 0; k0 < nlag; k0 += zmax)
                    hipLaunchKernelGGL(k_diag_autocov, dim3((unsigned)((nc + 63) / 64), d1, (unsigned)std::min<long>(nlag - k0, zmax)), dim3(64),
                                       0, ctx->stream, d_samples + (size_t)part * N * d1 * C, N, d1, C, nc, k0,
                                       d_mean + (size_t)part * d1 * C, d_acov);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = mhx_fail(MHX_EHIP, "k_diag_autocov failed"); break; }
            std::vector<double> ac((size_t)(nlag + 1) * d1);
            if (hipMemcpyAsync(ac.data(), d_acov, ac.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = mhx_fail(MHX_EHIP, "D2H"); break; }
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
        }
    } while (0);
    if (d_mean) (void)hipFree(d_mean);
    if (d_sums) (void)hipFree(d_sums);
    if (d_acov) (void)hipFree(d_acov);
    return rc;
}

int api_run_diagnostics(mhx_run* r, const mhx_diag_cfg* cfg, double* sum_m, double* sum_m2,
                                   double* sum_v, double* ess)
{
    if (!r || !cfg) return mhx_fail(MHX_EINVAL, "mhx_run_diagnostics: NULL argument");
    if (r->n_saved < 2) return mhx_fail(MHX_ESTATE, "mhx_run_diagnostics: needs a sample buffer with >= 2 draws");
    HIP_TRY(hipSetDevice(r->ctx->device));
    return diag_compute(r->ctx, r->d_samples, r->n_saved, r->dim + 1, r->n, cfg,
                        r->moments_mode ? r->d_mom_mean : nullptr, r->d_mom_m2, sum_m, sum_m2, sum_v, ess);
}

// ---- rank-normalised bulk ESS and tail ESS (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021, sections 4.1-4.3) ----
// One parameter at a time: its N C draws are sorted on the device (rocPRIM radix sort, keys = values, payload =
// position), every draw is replaced by the normal score of its rank, z = Phi^-1((rank - 3/8) / (S + 1/4)), and by
// the indicators of the 5 % / 95 % quantiles; the multi-chain ESS above then runs on those three series.
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
    z[e] = (mhx_real)normcdfinv((rank - 0.375) / ((double)S + 0.25));
    const mhx_real v = sorted[r];
    lo[e] = v <= q05 ? MHX_R(1.0) : MHX_R(0.0);
    hi[e] = v <= q95 ? MHX_R(1.0) : MHX_R(0.0);
}

int api_run_ess_bulk_tail(mhx_run* r, const mhx_diag_cfg* cfg, const int32_t* params, int32_t nparams,
                                     double* ess_bulk, double* ess_tail)
{
    if (!r || !cfg || !params || nparams <= 0) return mhx_fail(MHX_EINVAL, "mhx_run_ess_bulk_tail: bad argument");
    if (r->moments_mode || r->n_saved < 4) return mhx_fail(MHX_ESTATE, "mhx_run_ess_bulk_tail: needs a sample buffer with >= 4 draws");
    mhx_ctx* ctx = r->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const long N = r->n_saved, C = r->n, S = N * C;
    const int d1 = r->dim + 1;
    if (S >= (1L << 32)) return mhx_fail(MHX_EINVAL, "mhx_run_ess_bulk_tail: more than 2^32 draws per parameter");
    for (int i = 0; i < nparams; ++i)
        if (params[i] < 0 || params[i] >= d1) return mhx_fail(MHX_EINVAL, "mhx_run_ess_bulk_tail: parameter %d out of range", params[i]);
    mhx_real *k0 = nullptr, *k1 = nullptr, *series = nullptr;
    unsigned *p0 = nullptr, *p1 = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    int rc = MHX_OK;
    do {
        if (hipMalloc(&k0, S * sizeof(mhx_real)) != hipSuccess || hipMalloc(&k1, S * sizeof(mhx_real)) != hipSuccess ||
            hipMalloc(&p0, S * sizeof(unsigned)) != hipSuccess || hipMalloc(&p1, S * sizeof(unsigned)) != hipSuccess ||
            hipMalloc(&series, 3 * S * sizeof(mhx_real)) != hipSuccess) { rc = mhx_fail(MHX_ENOMEM, "bulk / tail ESS scratch"); break; }
        if (rocprim::radix_sort_pairs(nullptr, tmp_bytes, k0, k1, p0, p1, (size_t)S, 0, 8 * (unsigned)sizeof(mhx_real), ctx->stream) != hipSuccess ||
            hipMalloc(&tmp, tmp_bytes ? tmp_bytes : 1) != hipSuccess) { rc = mhx_fail(MHX_ENOMEM, "radix sort scratch"); break; }
        const unsigned grid = (unsigned)((S + 255) / 256);
        for (int i = 0; i < nparams && rc == MHX_OK; ++i) {
            hipLaunchKernelGGL(k_diag_gather_param, dim3(grid), dim3(256), 0, ctx->stream, r->d_samples, N, d1, C, params[i], k0, p0);
            if (rocprim::radix_sort_pairs(tmp, tmp_bytes, k0, k1, p0, p1, (size_t)S, 0, 8 * (unsigned)sizeof(mhx_real), ctx->stream) != hipSuccess) { rc = mhx_fail(MHX_EHIP, "radix sort failed"); break; }
            mhx_real q[4];
            const long i05 = (long)(0.05 * (double)(S - 1)), i95 = (long)(0.95 * (double)(S - 1));
            if (hipMemcpyAsync(&q[0], k1 + i05, sizeof(mhx_real), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                hipMemcpyAsync(&q[1], k1 + i95, sizeof(mhx_real), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                hipMemcpyAsync(&q[2], k1, sizeof(mhx_real), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                hipMemcpyAsync(&q[3], k1 + (S - 1), sizeof(mhx_real), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = mhx_fail(MHX_EHIP, "quantile copy failed"); break; }
            // the bit order of the sort puts a NaN at an end (sign set: first, sign clear: last): such a row has no ranks, and the
            // searches of k_diag_rank_scores are not run on it
            if (q[2] != q[2] || q[3] != q[3]) {
                if (ess_bulk) ess_bulk[i] = std::nan("");
                if (ess_tail) ess_tail[i] = std::nan("");
                continue;
            }
            hipLaunchKernelGGL(k_diag_rank_scores, dim3(grid), dim3(256), 0, ctx->stream, k1, p1, S, q[0], q[1],
                               series, series + S, series + 2 * S);
            if (hipGetLastError() != hipSuccess) { rc = mhx_fail(MHX_EHIP, "k_diag_rank_scores failed"); break; }
            double e[3];
            for (int j = 0; j < 3 && rc == MHX_OK; ++j)
                rc = diag_compute(ctx, series + (size_t)j * S, N, 1, C, cfg, nullptr, nullptr, nullptr, nullptr, nullptr, &e[j]);
            if (rc) break;
            if (ess_bulk) ess_bulk[i] = e[0];
            // the smaller of the two quantile ESS values; a truncated (negated) one keeps its sign
            // (an indicator that is constant has no ESS: NaN, whichever of the two it is)
            if (ess_tail) ess_tail[i] = e[1] != e[1] || e[2] != e[2] ? std::nan("") : std::fabs(e[1]) < std::fabs(e[2]) ? e[1] : e[2];
        }
    } while (0);
    void* ptrs[] = {k0, k1, p0, p1, series, tmp};
    for (void* q : ptrs) if (q) (void)hipFree(q);
    return rc;
}

// ---- rank-normalised split R-hat, bulk and folded (Vehtari et al. 2021, section 4.1), from the same one sort ----
// mhx_run_ess_bulk_tail above stays as it is (its results are pinned bit for bit by its own test, and it is the yardstick of
// tools/bench_rank_diag.py); what follows repeats its steps per row -- gather, sort, tie searches and indicators -- scores both
// series with diag_normal_score (a few ulp of fp64 at every rank) and adds the folded scores by search in the sorted array
// (mhx_diag_fold_rank: no second sort).
// The normal score of a tie-averaged rank, z = Phi^-1((rank - 3/8) / (S + 1/4)), to a few ulp of fp64 over the whole range.
// k_diag_rank_scores forms p in double and inverts it: p carries an ABSOLUTE rounding error of 2^-54 near 1/2 and 2^-53 near 1, which
// Phi^-1 returns magnified by 1 / phi(z) -- thousands of ulp of a score near zero, hundreds at the top score.  Here the argument is
// always a quotient of two exactly representable numbers (rank is a multiple of 1/2, S < 2^32) and small where z is small:
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

// k_diag_rank_scores with the score above (that kernel stays as it is: mhx_run_ess_bulk_tail keeps its bits)
__global__ void __launch_bounds__(256)
k_diag_rank_scores_wc(const mhx_real* __restrict__ sorted, const unsigned* __restrict__ pos, const long S, const mhx_real q05,
                      const mhx_real q95, mhx_real* __restrict__ z, mhx_real* __restrict__ lo, mhx_real* __restrict__ hi)
{
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= S) return;
    const unsigned e = pos[r];
    const mhx_real key = sorted[r];
    long a0 = 0, a1 = r;                                   // first index with sorted[i] == key
    while (a0 < a1) { const long mid = (a0 + a1) >> 1; if (sorted[mid] < key) a0 = mid + 1; else a1 = mid; }
    const long first = a0;
    a0 = r; a1 = S - 1;                                    // last index with sorted[i] == key
    while (a0 < a1) { const long mid = (a0 + a1 + 1) >> 1; if (sorted[mid] > key) a1 = mid - 1; else a0 = mid; }
    z[e] = (mhx_real)diag_normal_score(0.5 * ((double)first + (double)a0) + 1.0, S);
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

struct rank_scratch {
    mhx_real *k0 = nullptr, *k1 = nullptr, *series = nullptr;   // series: bulk scores | 5 % indicator | 95 % indicator | folded scores
    unsigned *p0 = nullptr, *p1 = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    ~rank_scratch()
    {
        void* ptrs[] = {k0, k1, p0, p1, series, tmp};
        for (void* q : ptrs) if (q) (void)hipFree(q);
    }
};

static int rank_check(const mhx_run* r, const char* who)
{
    if (r->moments_mode || r->n_saved < 4) return mhx_fail(MHX_ESTATE, "%s: needs a sample buffer with >= 4 draws", who);
    if ((long)r->n_saved * (long)r->n >= (1L << 32)) return mhx_fail(MHX_EINVAL, "%s: more than 2^32 draws per parameter", who);
    return MHX_OK;
}

static int rank_scratch_alloc(mhx_ctx* ctx, long S, rank_scratch* w)
{
    if (hipMalloc(&w->k0, S * sizeof(mhx_real)) != hipSuccess || hipMalloc(&w->k1, S * sizeof(mhx_real)) != hipSuccess ||
        hipMalloc(&w->p0, S * sizeof(unsigned)) != hipSuccess || hipMalloc(&w->p1, S * sizeof(unsigned)) != hipSuccess ||
        hipMalloc(&w->series, 4 * S * sizeof(mhx_real)) != hipSuccess) return mhx_fail(MHX_ENOMEM, "rank diagnostics scratch");
    if (rocprim::radix_sort_pairs(nullptr, w->tmp_bytes, w->k0, w->k1, w->p0, w->p1, (size_t)S, 0, 8 * (unsigned)sizeof(mhx_real), ctx->stream) != hipSuccess ||
        hipMalloc(&w->tmp, w->tmp_bytes ? w->tmp_bytes : 1) != hipSuccess) return mhx_fail(MHX_ENOMEM, "radix sort scratch");
    return MHX_OK;
}

// what the host reads of a sorted row, in ONE synchronisation: the 5 % and 95 % order statistics, the two ends, the middle pair
struct rank_row {
    mhx_real q05, q95, first, last, median;
    bool has_nan;
};

// gather row p, sort it (k1 / p1: ascending keys and their [t][c] positions) and fetch rank_row
static int rank_sort_row(mhx_run* r, rank_scratch* w, int p, rank_row* out)
{
    mhx_ctx* ctx = r->ctx;
    const long N = r->n_saved, C = r->n, S = N * C;
    hipLaunchKernelGGL(k_diag_gather_param, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, r->d_samples, N, r->dim + 1, C, p,
                       w->k0, w->p0);
    if (rocprim::radix_sort_pairs(w->tmp, w->tmp_bytes, w->k0, w->k1, w->p0, w->p1, (size_t)S, 0, 8 * (unsigned)sizeof(mhx_real), ctx->stream) != hipSuccess)
        return mhx_fail(MHX_EHIP, "radix sort failed");
    const long at[6] = {(long)(0.05 * (double)(S - 1)), (long)(0.95 * (double)(S - 1)), 0, S - 1, (S - 1) / 2, S / 2};
    mhx_real q[6];
    for (int j = 0; j < 6; ++j)
        if (hipMemcpyAsync(&q[j], w->k1 + at[j], sizeof(mhx_real), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            return mhx_fail(MHX_EHIP, "quantile copy failed");
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return mhx_fail(MHX_EHIP, "quantile copy failed");
    out->q05 = q[0]; out->q95 = q[1]; out->first = q[2]; out->last = q[3];
    // Julia's middle(): the middle draw of an odd S, else half of each of the middle pair added in the run's width
    out->median = (S & 1) ? q[4] : q[4] / MHX_R(2.0) + q[5] / MHX_R(2.0);
    // the bit order of the sort puts a NaN at an end (sign set: first, sign clear: last)
    out->has_nan = q[2] != q[2] || q[3] != q[3];
    return MHX_OK;
}

static void rank_launch_bulk(mhx_ctx* ctx, rank_scratch* w, long S, const rank_row& row)
{
    hipLaunchKernelGGL(k_diag_rank_scores_wc, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, w->k1, w->p1, S, row.q05, row.q95,
                       w->series, w->series + S, w->series + 2 * S);
}
static void rank_launch_fold(mhx_ctx* ctx, rank_scratch* w, long S, const rank_row& row)
{
    hipLaunchKernelGGL(k_diag_fold_scores, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, w->k1, w->p1, S, row.median,
                       w->series + 3 * S);
}

// R-hat = sqrt(var+ / W) from the three sums over M (half-)chains of n draws (include/mhx.h); W == 0: NaN (Vm == 0) or +inf
static double rhat_from_sums(double sum_m, double sum_m2, double sum_v, double M, double n)
{
    if (!(M > 1.0)) return std::nan("");
    const double W = sum_v / M;
    const double Vm = std::fmax((sum_m2 - sum_m * sum_m / M) / (M - 1.0), 0.0);
    return std::sqrt(((n - 1.0) / n * W + Vm) / W);
}

int api_run_rank_diagnostics(mhx_run* r, const mhx_diag_cfg* cfg, const int32_t* params, int32_t nparams, double* ess_bulk,
                             double* ess_tail, double* rhat_bulk, double* rhat_tail)
{
    const char* who = "mhx_run_rank_diagnostics";
    if (!r || !cfg || !params || nparams <= 0) return mhx_fail(MHX_EINVAL, "%s: bad argument", who);
    int rc = rank_check(r, who);
    if (rc) return rc;
    mhx_ctx* ctx = r->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const long N = r->n_saved, C = r->n, S = N * C;
    for (int i = 0; i < nparams; ++i)
        if (params[i] < 0 || params[i] > r->dim) return mhx_fail(MHX_EINVAL, "%s: parameter %d out of range", who, params[i]);
    const bool want_ess = ess_bulk || ess_tail;
    const double nparts = cfg->split ? 2.0 : 1.0, M = (double)C * nparts, n = (double)(cfg->split ? N / 2 : N);
    const double nan = std::nan("");
    rank_scratch w;
    if ((rc = rank_scratch_alloc(ctx, S, &w))) return rc;
    for (int i = 0; i < nparams; ++i) {
        rank_row row;
        if ((rc = rank_sort_row(r, &w, params[i], &row))) return rc;
        if (row.has_nan) {                                  // no ranks: no search is launched on the row
            if (ess_bulk) ess_bulk[i] = nan;
            if (ess_tail) ess_tail[i] = nan;
            if (rhat_bulk) rhat_bulk[i] = nan;
            if (rhat_tail) rhat_tail[i] = nan;
            continue;
        }
        const bool fold = rhat_tail && std::isfinite(row.median);
        rank_launch_bulk(ctx, &w, S, row);
        if (fold) rank_launch_fold(ctx, &w, S, row);
        if (hipGetLastError() != hipSuccess) return mhx_fail(MHX_EHIP, "%s: the score kernels failed to launch", who);
        // the bulk scores: their moments come with the ESS call (the ESS itself as mhx_run_ess_bulk_tail takes it)
        double e[3] = {nan, nan, nan}, sm = 0.0, sm2 = 0.0, sv = 0.0;
        if (want_ess || rhat_bulk)
            if ((rc = diag_compute(ctx, w.series, N, 1, C, cfg, nullptr, nullptr, &sm, &sm2, &sv, want_ess ? &e[0] : nullptr))) return rc;
        if (rhat_bulk) rhat_bulk[i] = rhat_from_sums(sm, sm2, sv, M, n);
        if (want_ess) {
            for (int j = 1; j < 3; ++j)
                if ((rc = diag_compute(ctx, w.series + (size_t)j * S, N, 1, C, cfg, nullptr, nullptr, nullptr, nullptr, nullptr, &e[j]))) return rc;
            if (ess_bulk) ess_bulk[i] = e[0];
            if (ess_tail) ess_tail[i] = e[1] != e[1] || e[2] != e[2] ? nan : std::fabs(e[1]) < std::fabs(e[2]) ? e[1] : e[2];
        }
        if (rhat_tail) {
            rhat_tail[i] = nan;                             // a median that is not finite folds nothing
            if (fold) {
                if ((rc = diag_compute(ctx, w.series + 3 * (size_t)S, N, 1, C, cfg, nullptr, nullptr, &sm, &sm2, &sv, nullptr))) return rc;
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
    int rc = rank_check(r, who);
    if (rc) return rc;
    if (param < 0 || param > r->dim) return mhx_fail(MHX_EINVAL, "%s: parameter %d out of range", who, (int)param);
    mhx_ctx* ctx = r->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const long S = (long)r->n_saved * (long)r->n;
    rank_scratch w;
    if ((rc = rank_scratch_alloc(ctx, S, &w))) return rc;
    rank_row row;
    if ((rc = rank_sort_row(r, &w, param, &row))) return rc;
    if (row.has_nan || (folded && !std::isfinite(row.median))) {
        const mhx_real nan = (mhx_real)std::nan("");
        for (long e = 0; e < S; ++e) out_host[e] = nan;
        return MHX_OK;
    }
    if (folded) rank_launch_fold(ctx, &w, S, row);
    else rank_launch_bulk(ctx, &w, S, row);
    if (hipGetLastError() != hipSuccess) return mhx_fail(MHX_EHIP, "%s: the score kernel failed to launch", who);
    HIP_TRY(hipMemcpyAsync(out_host, w.series + (folded ? 3 * (size_t)S : 0), (size_t)S * sizeof(mhx_real), hipMemcpyDeviceToHost, ctx->stream));
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

struct select_source {
    mhx_ctx* ctx;
    const mhx_real* tensor;
    long N, C;
    int d1;
    const int32_t* params;
    int32_t nparams;
    const char* who;
};

// one pass over one tensor: mhx_select_hist_fn of mhx_select.h (hist is host memory)
static int select_hist_pass(void* user, const uint64_t* prefixes, const int32_t* ngroups, int32_t gstride, int32_t shift,
                            int32_t digit_bits, uint64_t* hist)
{
    const select_source* s = (const select_source*)user;
    mhx_ctx* ctx = s->ctx;
    const int P = s->nparams;
    if (digit_bits < 1 || digit_bits > MHX_SELECT_MAX_DIGIT_BITS || shift < 0 || shift + digit_bits > MHX_KEY_BITS || gstride < 1)
        return mhx_fail(MHX_EINVAL, "%s: digit of %d bits at bit %d of a %d-bit key", s->who, (int)digit_bits, (int)shift, MHX_KEY_BITS);
    int gmax = 0;
    for (int i = 0; i < P; ++i) {
        if (ngroups[i] < 0 || ngroups[i] > gstride) return mhx_fail(MHX_EINVAL, "%s: %d groups in a stride of %d", s->who, (int)ngroups[i], (int)gstride);
        gmax = std::max(gmax, (int)ngroups[i]);
    }
    if (!gmax) return MHX_OK;
    if (shift + digit_bits == MHX_KEY_BITS && gmax > 1) return mhx_fail(MHX_EINVAL, "%s: the first pass has one group", s->who);
    HIP_TRY(hipSetDevice(ctx->device));
    // scratch of the context, grown on demand: histogram | prefixes | group counts | parameter rows
    const size_t nh = ((size_t)P * gstride) << digit_bits, npf = (size_t)P * gstride;
    const size_t bytes = (nh + npf) * sizeof(uint64_t) + 2 * (size_t)P * sizeof(int32_t);
    if (bytes > ctx->select_bytes) {
        if (ctx->select_scratch) (void)hipFree(ctx->select_scratch);
        ctx->select_scratch = nullptr; ctx->select_bytes = 0;
        if (hipMalloc(&ctx->select_scratch, bytes) != hipSuccess) return mhx_fail(MHX_ENOMEM, "%s: %zu bytes of histogram scratch", s->who, bytes);
        ctx->select_bytes = bytes;
    }
    unsigned long long* d_hist = (unsigned long long*)ctx->select_scratch;
    unsigned long long* d_pf = d_hist + nh;
    int* d_ng = (int*)(d_pf + npf);
    int* d_par = d_ng + P;
    HIP_TRY(hipMemsetAsync(d_hist, 0, nh * sizeof(uint64_t), ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_pf, prefixes, npf * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_ng, ngroups, (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_par, s->params, (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    // blocks per parameter: enough blocks for the whole chip, chunks of at least one unrolled block sweep and below 2^31 draws
    const unsigned long long S = (unsigned long long)s->N * (unsigned long long)s->C;
    const unsigned long long sweep = (unsigned long long)MHX_SELECT_THREADS * MHX_SELECT_UNROLL;
    unsigned long long nblk = std::min<unsigned long long>((2048 + P - 1) / P, (S + sweep - 1) / sweep);
    nblk = std::max<unsigned long long>(std::max<unsigned long long>(nblk, 1), (S + (1ull << 31) - 1) >> 31);
    const unsigned long long chunk = (S + nblk - 1) / nblk;
    const int top = shift + digit_bits == MHX_KEY_BITS;
    const dim3 grid((unsigned)nblk, (unsigned)P), block(MHX_SELECT_THREADS);
#define MHX_SELECT_LAUNCH(BITS, G)                                                                                        \
    for (int first = 0; first < gmax; first += G)                                                                         \
        hipLaunchKernelGGL((k_select_hist<BITS, G>), grid, block, 0, ctx->stream, s->tensor, s->N, s->d1, s->C, d_par, d_pf, d_ng, \
                           (int)gstride, first, (int)shift, (int)digit_bits, top, chunk, d_hist)
    if (digit_bits <= 8) { MHX_SELECT_LAUNCH(8, 16); }
    else if (digit_bits <= 10) { MHX_SELECT_LAUNCH(10, 16); }
    else { MHX_SELECT_LAUNCH(11, 8); }
#undef MHX_SELECT_LAUNCH
    if (hipGetLastError() != hipSuccess) return mhx_fail(MHX_EHIP, "%s: k_select_hist failed to launch", s->who);
    // only the groups in use travel: rows of gmax << digit_bits counters out of a pitch of gstride << digit_bits
    const size_t pitch = ((size_t)gstride << digit_bits) * sizeof(uint64_t), width = ((size_t)gmax << digit_bits) * sizeof(uint64_t);
    HIP_TRY(hipMemcpy2DAsync(hist, pitch, d_hist, pitch, width, (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MHX_OK;
}

static int select_check_params(const char* who, const int32_t* params, int32_t nparams, int d1)
{
    if (!params || nparams <= 0) return mhx_fail(MHX_EINVAL, "%s: no parameters", who);
    for (int i = 0; i < nparams; ++i)
        if (params[i] < 0 || params[i] >= d1) return mhx_fail(MHX_EINVAL, "%s: parameter %d out of range [0, %d)", who, (int)params[i], d1);
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

int api_ctx_order_statistics(mhx_ctx* ctx, const mhx_real* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,
                             const int32_t* params, int32_t nparams, const int64_t* ranks, int32_t nranks, double* out)
{
    const char* who = "mhx_ctx_order_statistics";
    if (!ctx || !d_tensor || !out || !ranks || nranks <= 0) return mhx_fail(MHX_EINVAL, "%s: bad argument", who);
    if (n_samples < 1 || dim1 < 1 || nchains < 1) return mhx_fail(MHX_EINVAL, "%s: tensor of %lld x %d x %lld", who, (long long)n_samples, (int)dim1, (long long)nchains);
    int rc = select_check_params(who, params, nparams, dim1);
    if (rc) return rc;
    select_source src{ctx, d_tensor, (long)n_samples, (long)nchains, dim1, params, nparams, who};
    const int digit = opt_int(ctx, "SELECT_BITS", MHX_SELECT_DIGIT_BITS);
    select_landing(ctx, digit, nparams, nranks);
    return mhx_select_drive(who, MHX_KEY_BITS, digit, nparams, ranks, nranks, (uint64_t)n_samples * (uint64_t)nchains, select_hist_pass,
                            &src, out, ctx->select_landing, ctx->select_landing_words);
}

static int select_need_tensor(const mhx_run* r, const char* who)
{
    if (!r) return mhx_fail(MHX_EINVAL, "%s: run is NULL", who);
    if (r->moments_mode || r->n_saved < 1 || !r->d_samples)
        return mhx_fail(MHX_ESTATE, "%s: the run holds no device sample tensor (moments mode, save_samples = 0 or a host-streamed run)", who);
    return MHX_OK;
}

int api_run_order_statistics(mhx_run* r, const int32_t* params, int32_t nparams, const int64_t* ranks, int32_t nranks, double* out)
{
    const char* who = "mhx_run_order_statistics";
    int rc = select_need_tensor(r, who);
    if (rc) return rc;
    if (!out || !ranks || nranks <= 0) return mhx_fail(MHX_EINVAL, "%s: bad argument", who);
    if ((rc = select_check_params(who, params, nparams, r->dim + 1))) return rc;
    select_source src{r->ctx, r->d_samples, (long)r->n_saved, (long)r->n, r->dim + 1, params, nparams, who};
    const int digit = opt_int(r->ctx, "SELECT_BITS", MHX_SELECT_DIGIT_BITS);
    select_landing(r->ctx, digit, nparams, nranks);
    return mhx_select_drive(who, MHX_KEY_BITS, digit, nparams, ranks, nranks, (uint64_t)r->n_saved * (uint64_t)r->n, select_hist_pass,
                            &src, out, r->ctx->select_landing, r->ctx->select_landing_words);
}

// the per-pass building block of the group form (mhx_group_order_statistics adds the members' histograms and scans once)
int api_run_select_histogram(mhx_run* r, const int32_t* params, int32_t nparams, const uint64_t* prefixes, const int32_t* ngroups,
                             int32_t gstride, int32_t shift, int32_t digit_bits, uint64_t* hist)
{
    const char* who = "mhx_run_select_histogram";
    int rc = select_need_tensor(r, who);
    if (rc) return rc;
    if (!prefixes || !ngroups || !hist) return mhx_fail(MHX_EINVAL, "%s: NULL argument", who);
    if ((rc = select_check_params(who, params, nparams, r->dim + 1))) return rc;
    select_source src{r->ctx, r->d_samples, (long)r->n_saved, (long)r->n, r->dim + 1, params, nparams, who};
    return select_hist_pass(&src, prefixes, ngroups, gstride, shift, digit_bits, hist);
}
