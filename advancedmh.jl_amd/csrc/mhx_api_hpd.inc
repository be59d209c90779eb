// HPD intervals host side (included by mhx_api.hip after mhx_api_diag.inc): thresholds by the radix select (on the context's select
// block), then on the context's HPD block one gather sweep, a sort of the tails only, the first minimum width (mhx_hpd_kernels.h,
// DESIGN.md section 6.5.2)

__global__ void __launch_bounds__(MHX_SELECT_THREADS)
k_hpd_gather(const mhx_real* __restrict__ samples, const long N, const int d1, const long C, const int* __restrict__ params,
             const unsigned long long* __restrict__ keyL, const unsigned long long* __restrict__ keyU, const unsigned long long chunk,
             const unsigned long long cap, unsigned long long* __restrict__ count, mhx_key* __restrict__ tails)
{
    mhx_hpd_gather_body(samples, N, d1, C, params, keyL, keyU, chunk, cap, count, tails);
}
__global__ void __launch_bounds__(MHX_HPD_ARGMIN_THREADS)
k_hpd_argmin(const mhx_hpd_row* __restrict__ rows, const mhx_key* __restrict__ tails, const unsigned long long cap,
             const unsigned long long per, double* __restrict__ part_w, unsigned long long* __restrict__ part_i)
{
    __shared__ double red_w[MHX_HPD_ARGMIN_THREADS / 64];
    __shared__ unsigned long long red_i[MHX_HPD_ARGMIN_THREADS / 64];
    mhx_hpd_argmin_body(rows, tails, cap, per, part_w, part_i, red_w, red_i);
}
__global__ void __launch_bounds__(64)
k_hpd_final(const mhx_hpd_row* __restrict__ rows, const mhx_key* __restrict__ tails, const unsigned long long cap, const int nblk,
            const double* __restrict__ part_w, const unsigned long long* __restrict__ part_i, double* __restrict__ out)
{
    mhx_hpd_final_body(rows, tails, cap, nblk, part_w, part_i, out);
}

#define MHX_HPD_SCRATCH_MB 1024.0                           // option HPD_SCRATCH_MB: bound on the scratch of a call, rows go in batches that fit

static size_t hpd_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }      // (a piece of scratch_carve)

// the arguments are checked.  lower / upper are written last, after everything succeeded.
static int hpd_compute(const draws_view& v, const int32_t* params, int P, double alpha, double* lower, double* upper)
{
    mhx_ctx* ctx = v.ctx;
    const char* who = v.who;
    HIP_TRY(hipSetDevice(ctx->device));
    const unsigned long long S = v.S();
    const double am = std::ceil(alpha * (double)S);
    const unsigned long long m = am < 1.0 ? 1ull : (unsigned long long)(int64_t)am;      // alpha < 1: m <= S
    const unsigned long long cap = m - 1;                   // keys a tail buffer holds: the draws strictly beyond a threshold
    double budget_mb = MHX_HPD_SCRATCH_MB;
    if (const char* v = opt(ctx, "HPD_SCRATCH_MB")) {
        budget_mb = atof(v);
        if (!(budget_mb > 0.0) || !std::isfinite(budget_mb)) return mhx_fail(MHX_EINVAL, "%s: option HPD_SCRATCH_MB = '%s' is not a positive number", who, v);
    }
    // the scratch plan, before any sweep: row_bytes is what a row adds to the pieces carved below, each on its own 256-byte line; a single
    // row that does not fit the budget is refused here
    size_t sort_bytes = 0, part_cap = 0;
    int Rmax = 0;
    if (cap > 0) {
        mhx_key* nokey = nullptr;
        if (rocprim::radix_sort_keys(nullptr, sort_bytes, nokey, nokey, (size_t)cap, 0u, (unsigned)MHX_KEY_BITS, ctx->stream) != hipSuccess)
            return mhx_fail(MHX_EHIP, "%s: radix sort scratch query failed", who);
        sort_bytes = hpd_align(sort_bytes ? sort_bytes : 1);
        const unsigned long long tmax_bound = 2 * cap + 1;
        part_cap = (size_t)std::min<unsigned long long>(2048, (tmax_bound + MHX_HPD_ARGMIN_PER_BLOCK - 1) / MHX_HPD_ARGMIN_PER_BLOCK);
        const double row_bytes = 4.0 * (double)cap * sizeof(mhx_key) + 256.0 * 2 + (double)part_cap * 16.0 +
                                 (double)(2 * MHX_HPD_COUNT_STRIDE + 2 + 2) * sizeof(uint64_t) + sizeof(mhx_hpd_row) + sizeof(int32_t);
        const double room = budget_mb * 1048576.0 - (double)sort_bytes - 16.0 * 256.0;
        if (room < row_bytes)
            return mhx_fail(MHX_EINVAL, "%s: the tails of one row (2 x %llu draws beyond the thresholds, %.1f MB of scratch with their sort) do not fit "
                            "option HPD_SCRATCH_MB = %g", who, cap, (row_bytes + (double)sort_bytes) / 1048576.0, budget_mb);
        Rmax = (int)std::min<double>((double)P, std::floor(room / row_bytes));
    }
    // thresholds and the NaN check: ranks {m - 1, S - m, S - 1} of every row in one batch of the select
    const int64_t ranks[3] = {(int64_t)(m - 1), (int64_t)(S - m), (int64_t)(S - 1)};
    std::vector<double> os((size_t)P * 3);
    select_source src{v, params, P};
    const int digit = opt_int(ctx, "SELECT_BITS", MHX_SELECT_DIGIT_BITS);
    select_landing(ctx, digit, P, 3);
    int rc = mhx_select_drive(who, MHX_KEY_BITS, digit, P, ranks, 3, S, select_hist_pass, &src, os.data(), ctx->select_landing,
                              ctx->select_landing_words);
    if (rc) return rc;
    // phase timing (tools build): return after 1 the select, 2 the gather, 3 the sort, with nothing written to lower / upper
    const char* stop_opt = MHX_PROBE_OPT(ctx, "HPD_STOP_AFTER");
    const int stop_after = stop_opt ? atoi(stop_opt) : 0;
    if (stop_after == 1) return MHX_OK;
    std::vector<double> res((size_t)P * 2);
    std::vector<char> nan_row((size_t)P, 0);
    for (int i = 0; i < P; ++i) {
        nan_row[i] = os[(size_t)i * 3 + 2] != os[(size_t)i * 3 + 2];       // NaNs order last: the row holds one
        res[(size_t)i * 2] = nan_row[i] ? std::nan("") : os[(size_t)i * 3];
        res[(size_t)i * 2 + 1] = nan_row[i] ? std::nan("") : os[(size_t)i * 3 + 1];
    }
    if (cap > 0) {                                          // m = 1: one candidate, [y[0], y[S-1]], which the select gave
        const size_t n_tail = (size_t)Rmax * 2 * (size_t)cap;
        mhx_key *d_tails = nullptr, *d_sorted = nullptr;
        char* d_sort = nullptr;
        unsigned long long *d_count = nullptr, *d_keyL = nullptr, *d_keyU = nullptr, *d_pi = nullptr;
        mhx_hpd_row* d_rows = nullptr;
        double *d_pw = nullptr, *d_out = nullptr;
        int* d_par = nullptr;
        rc = scratch_carve(&ctx->hpd_scratch, &ctx->hpd_bytes, who, "tail scratch", [&](scratch_pieces& c) {
            d_tails = c.take<mhx_key>(n_tail);              // Rmax x 2 x cap keys beyond the thresholds
            d_sorted = c.take<mhx_key>(n_tail);             // ... ascending
            d_sort = c.take<char>(sort_bytes);              // sort space
            d_count = c.take<unsigned long long>((size_t)Rmax * 2 * MHX_HPD_COUNT_STRIDE);
            d_keyL = c.take<unsigned long long>(Rmax);      // thresholds
            d_keyU = c.take<unsigned long long>(Rmax);
            d_rows = c.take<mhx_hpd_row>(Rmax);
            d_pw = c.take<double>((size_t)Rmax * part_cap); // partial minima
            d_pi = c.take<unsigned long long>((size_t)Rmax * part_cap);
            d_out = c.take<double>((size_t)Rmax * 2);       // results
            d_par = c.take<int>(Rmax);                      // tensor rows
        });
        if (rc) return rc;
        std::vector<unsigned long long> hL((size_t)Rmax), hU((size_t)Rmax), hc((size_t)Rmax * 2), hcs((size_t)Rmax * 2 * MHX_HPD_COUNT_STRIDE);
        std::vector<mhx_hpd_row> hrows((size_t)Rmax);
        std::vector<double> hout((size_t)Rmax * 2);
        for (int r0 = 0; r0 < P; r0 += Rmax) {
            const int R = std::min(Rmax, P - r0);
            bool any = false;
            for (int k = 0; k < R; ++k) {
                const int i = r0 + k;
                hL[k] = nan_row[i] ? 0ull : mhx_select_key_of(os[(size_t)i * 3], MHX_KEY_BITS);
                hU[k] = nan_row[i] ? ~0ull : mhx_select_key_of(os[(size_t)i * 3 + 1], MHX_KEY_BITS);
                any = any || !nan_row[i];
            }
            if (!any) continue;
            HIP_TRY(hipMemsetAsync(d_count, 0, (size_t)R * 2 * MHX_HPD_COUNT_STRIDE * sizeof(uint64_t), ctx->stream));
            HIP_TRY(hipMemcpyAsync(d_keyL, hL.data(), (size_t)R * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(d_keyU, hU.data(), (size_t)R * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(d_par, params + r0, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
            unsigned long long chunk = 0;
            const unsigned long long nblk = sweep_blocks(S, R, &chunk);
            hipLaunchKernelGGL(k_hpd_gather, dim3((unsigned)nblk, (unsigned)R), dim3(MHX_SELECT_THREADS), 0, ctx->stream, v.tensor, v.N, v.d1,
                               v.C, d_par, d_keyL, d_keyU, chunk, cap, d_count, d_tails);
            if (hipGetLastError() != hipSuccess) return mhx_fail(MHX_EHIP, "%s: k_hpd_gather failed to launch", who);
            HIP_TRY(hipMemcpyAsync(hcs.data(), d_count, (size_t)R * 2 * MHX_HPD_COUNT_STRIDE * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            for (int k = 0; k < R * 2; ++k) hc[k] = hcs[(size_t)k * MHX_HPD_COUNT_STRIDE];      // (a counter per 256-byte line)
            unsigned long long tmax = 1;
            for (int k = 0; k < R; ++k) {
                const unsigned long long cL = hc[(size_t)k * 2], cU = hc[(size_t)k * 2 + 1];
                if (cL > cap || cU > cap)
                    return mhx_fail(MHX_EHIP, "%s: %llu / %llu draws of row %d lie beyond its thresholds where at most %llu can (tensor changed during the call?)",
                                    who, cL, cU, (int)params[r0 + k], cap);
                hrows[k] = mhx_hpd_row{nan_row[r0 + k] ? 1ull : m, cL, cU, hL[k], hU[k]};
                const unsigned long long edge = hrows[k].m - cU;
                tmax = std::max(tmax, cL + (cL < edge ? 1ull : 0ull) + (hrows[k].m - std::max(edge, cL)));
            }
            if (stop_after == 2) continue;
            // the tails only: every (row, tail) segment on its own, keys ascending into the second buffer
            for (int k = 0; k < R * 2; ++k) {
                const size_t n = (size_t)hc[k];
                mhx_key* in = d_tails + (size_t)k * cap;
                mhx_key* out = d_sorted + (size_t)k * cap;
                if (n == 1) HIP_TRY(hipMemcpyAsync(out, in, sizeof(mhx_key), hipMemcpyDeviceToDevice, ctx->stream));
                if (n < 2) continue;
                size_t need = 0;
                if (rocprim::radix_sort_keys(nullptr, need, in, out, n, 0u, (unsigned)MHX_KEY_BITS, ctx->stream) != hipSuccess || need > sort_bytes)
                    return mhx_fail(MHX_EHIP, "%s: the sort of %zu keys asks for %zu bytes of scratch, %zu were planned", who, n, need, sort_bytes);
                need = sort_bytes;
                if (rocprim::radix_sort_keys(d_sort, need, in, out, n, 0u, (unsigned)MHX_KEY_BITS, ctx->stream) != hipSuccess)
                    return mhx_fail(MHX_EHIP, "%s: radix sort of a tail failed", who);
            }
            if (stop_after == 3) { HIP_TRY(hipStreamSynchronize(ctx->stream)); continue; }
            HIP_TRY(hipMemcpyAsync(d_rows, hrows.data(), (size_t)R * sizeof(mhx_hpd_row), hipMemcpyHostToDevice, ctx->stream));
            const unsigned long long maxblk = std::min<unsigned long long>(part_cap, (2048 + R - 1) / R);
            const unsigned long long per = std::max<unsigned long long>(MHX_HPD_ARGMIN_PER_BLOCK, (tmax + maxblk - 1) / maxblk);
            const int nblk_a = (int)((tmax + per - 1) / per);   // <= maxblk <= part_cap
            hipLaunchKernelGGL(k_hpd_argmin, dim3((unsigned)nblk_a, (unsigned)R), dim3(MHX_HPD_ARGMIN_THREADS), 0, ctx->stream, d_rows,
                               d_sorted, cap, per, d_pw, d_pi);
            hipLaunchKernelGGL(k_hpd_final, dim3((unsigned)R), dim3(64), 0, ctx->stream, d_rows, d_sorted, cap, nblk_a, d_pw, d_pi, d_out);
            if (hipGetLastError() != hipSuccess) return mhx_fail(MHX_EHIP, "%s: k_hpd_argmin failed to launch", who);
            HIP_TRY(hipMemcpyAsync(hout.data(), d_out, (size_t)R * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            for (int k = 0; k < R; ++k)
                if (!nan_row[r0 + k]) { res[(size_t)(r0 + k) * 2] = hout[(size_t)k * 2]; res[(size_t)(r0 + k) * 2 + 1] = hout[(size_t)k * 2 + 1]; }
        }
    }
    if (stop_after) return MHX_OK;
    for (int i = 0; i < P; ++i) { lower[i] = res[(size_t)i * 2]; upper[i] = res[(size_t)i * 2 + 1]; }
    return MHX_OK;
}

// v is checked, nothing else is
static int hpd_checked(const draws_view& v, const int32_t* params, int32_t nparams, double alpha, double* lower, double* upper)
{
    if (!lower || !upper) return mhx_fail(MHX_EINVAL, "%s: bad argument", v.who);
    if (!(alpha > 0.0 && alpha < 1.0)) return mhx_fail(MHX_EINVAL, "%s: alpha = %g is not in (0, 1)", v.who, alpha);
    int rc = select_check_params(v.who, params, nparams, v.d1);
    return rc ? rc : hpd_compute(v, params, nparams, alpha, lower, upper);
}

int api_ctx_hpd(mhx_ctx* ctx, const mhx_real* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const int32_t* params,
                int32_t nparams, double alpha, double* lower, double* upper)
{
    draws_view v;
    int rc = draws_of_ctx("mhx_ctx_hpd", ctx, d_tensor, n_samples, dim1, nchains, &v);
    return rc ? rc : hpd_checked(v, params, nparams, alpha, lower, upper);
}

int api_run_hpd(mhx_run* r, const int32_t* params, int32_t nparams, double alpha, double* lower, double* upper)
{
    draws_view v;
    int rc = draws_of_run("mhx_run_hpd", r, &v);
    return rc ? rc : hpd_checked(v, params, nparams, alpha, lower, upper);
}
