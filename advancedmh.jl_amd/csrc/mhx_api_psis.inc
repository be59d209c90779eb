// PSIS-LOO host side (included by mhx_api.hip after mhx_api_pointwise.inc): the checks (row_blocks_checked), the run-time module
// (user_module) and the grid of the pointwise frame (pointwise_sweep_plan), and per batch of data rows
// the cutoffs by the radix select (mhx_select_drive with a histogram pass that re-evaluates l; on the context's select block), then on
// the context's tail block -- HPD's: it survives the select passes, and a call owns it until it returns -- one gather sweep, one
// segmented sort of the tails, the fit (mhx_psis_kernels.h, DESIGN.md section 6.5.8)

#define MHX_PSIS_SCRATCH_MB 1024.0                          // option PSIS_SCRATCH_MB: as HPD_SCRATCH_MB, rows go in batches that fit
#define MHX_PSIS_ROWS_DEFAULT 4                             // data rows per tile of the two sweeps (LDS: rows x 2^11 counters)
#define MHX_PSIS_MAX_TAIL (1ull << 20)                      // M at most: the fit's grid (30 + sqrt(M) points) lives in LDS
#define MHX_PSIS_DRAWS_PER_SLOT (1l << 23)                  // 256 lanes x 2^23 draws: what a block may count in a 32-bit LDS counter

// M = min(floor(0.2 T), ceil(3 sqrt(T / reff))) in double; below 5: 0 (no smoothing)
static unsigned long long psis_tail_length(unsigned long long T, double reff)
{
    const double a = std::floor(0.2 * (double)T), b = std::ceil(3.0 * std::sqrt((double)T / reff));
    const double m = std::min(a, b);
    return m < 5.0 ? 0ull : (unsigned long long)m;
}

// what a histogram pass of the select reads: the batch's rows on the device and the launch shape
struct psis_pass_source {
    draws_view v;
    hipFunction_t f_hist;
    const mhx_real *d_rows, *d_data;
    int nrows, rowlen, ndata, R;
    long ncb, slots;
};

// mhx_select_hist_fn: one rank per row, so one group per row and gstride == 1
static int psis_hist_pass(void* user, const uint64_t* prefixes, const int32_t* ngroups, int32_t gstride, int32_t shift, int32_t digit_bits,
                          uint64_t* hist)
{
    const psis_pass_source* s = (const psis_pass_source*)user;
    const draws_view& v = s->v;
    mhx_ctx* ctx = v.ctx;
    if (digit_bits < 1 || digit_bits > MHX_SELECT_MAX_DIGIT_BITS || shift < 0 || shift + digit_bits > MHX_KEY_BITS || gstride != 1)
        return mhx_fail(MHX_EINVAL, "%s: digit of %d bits at bit %d of a %d-bit key, stride %d", v.who, (int)digit_bits, (int)shift, MHX_KEY_BITS, (int)gstride);
    for (int i = 0; i < s->nrows; ++i)
        if (ngroups[i] != 1) return mhx_fail(MHX_EINVAL, "%s: %d groups where a row has one rank", v.who, (int)ngroups[i]);
    const size_t nh = (size_t)s->nrows << digit_bits;
    unsigned long long *d_hist = nullptr, *d_pf = nullptr;
    int rc = scratch_carve(&ctx->select_scratch, &ctx->select_bytes, v.who, "select scratch", [&](scratch_pieces& c) {
        d_hist = c.take<unsigned long long>(nh);
        d_pf = c.take<unsigned long long>((size_t)s->nrows);
    });
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d_hist, 0, nh * sizeof(uint64_t), ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_pf, prefixes, (size_t)s->nrows * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    const int top = shift + digit_bits == MHX_KEY_BITS;
    const dim3 grid((unsigned)s->ncb, (unsigned)s->slots, (unsigned)((s->nrows + s->R - 1) / s->R));
    rc = launch_module(s->f_hist, grid, MHX_POINTWISE_THREADS, ctx->stream, v.tensor, v.N, v.C, v.d1 - 1, s->d_rows, s->nrows, s->rowlen,
                       s->d_data, s->ndata, d_pf, (int)shift, (int)digit_bits, top, d_hist);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(hist, d_hist, nh * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MHX_OK;
}

// v is checked, nothing else is.  Nothing is written to out8, tail_out, T or M unless the call succeeds.
static int psis_checked(const draws_view& v, const char* source, const mhx_real* rows, int64_t nrows, int32_t rowlen, const mhx_real* data,
                        size_t ndata, double reff, double* out8, double* tail_out, int64_t* T_out, int64_t* M_out)
{
    const char* who = v.who;
    mhx_ctx* ctx = v.ctx;
    if (!source || !rows || !out8) return mhx_fail(MHX_EINVAL, "%s: NULL argument", who);
    if (int rc = row_blocks_checked(v, nrows, rowlen, data, ndata)) return rc;
    if (!(reff > 0.0) || !std::isfinite(reff)) return mhx_fail(MHX_EINVAL, "%s: reff = %g is not a positive finite number", who, reff);
    const unsigned long long S = v.S();
    const unsigned long long M = psis_tail_length(S, reff);
    if (M > MHX_PSIS_MAX_TAIL)
        return mhx_fail(MHX_EINVAL, "%s: a tail of %llu draws is longer than the %llu the fit holds", who, M, (unsigned long long)MHX_PSIS_MAX_TAIL);
    HIP_TRY(hipSetDevice(ctx->device));
    const int R = opt_int(ctx, "PSIS_ROWS", MHX_PSIS_ROWS_DEFAULT);
    if (R != 1 && R != 2 && R != 4 && R != 8) return mhx_fail(MHX_EINVAL, "%s: option PSIS_ROWS = %d is not 1, 2, 4 or 8", who, R);
    double budget_mb = MHX_PSIS_SCRATCH_MB;
    if (const char* o = opt(ctx, "PSIS_SCRATCH_MB")) {
        budget_mb = atof(o);
        if (!(budget_mb > 0.0) || !std::isfinite(budget_mb)) return mhx_fail(MHX_EINVAL, "%s: option PSIS_SCRATCH_MB = '%s' is not a positive number", who, o);
    }
    const int digit = opt_int(ctx, "SELECT_BITS", MHX_SELECT_DIGIT_BITS);
    if (digit < 1 || digit > MHX_SELECT_MAX_DIGIT_BITS) return mhx_fail(MHX_EINVAL, "%s: option SELECT_BITS = %d outside [1, %d]", who, digit, MHX_SELECT_MAX_DIGIT_BITS);
    // the grid of the two sweeps, without the row-tile term (pointwise_sweep_plan says why); enough strip slots that no block counts
    // 2^32 draws of a row
    const sweep_plan g = pointwise_sweep_plan(v, 1);
    const long ncb = g.ncb, slots = std::max((v.N + MHX_PSIS_DRAWS_PER_SLOT - 1) / MHX_PSIS_DRAWS_PER_SLOT, g.slots);
    const size_t nr = (size_t)nrows, cap = (size_t)M;
    if (slots > 65535) return mhx_fail(MHX_EINVAL, "%s: %ld saved draws need more than 65535 strip slots", who, v.N);
    // the scratch plan, before any compile or sweep: the largest batch of rows whose pieces fit the budget
    auto sort_bytes_of = [&](size_t rb, size_t* bytes) {
        *bytes = 0;
        if (!cap) return true;
        mhx_key* nokey = nullptr;
        unsigned* nooff = nullptr;
        size_t need = 0;
        if (rocprim::segmented_radix_sort_keys(nullptr, need, nokey, nokey, (unsigned)(rb * cap), (unsigned)rb, nooff, nooff, 0u,
                                               (unsigned)MHX_KEY_BITS, ctx->stream) != hipSuccess)
            return false;
        *bytes = need ? need : 1;
        return true;
    };
    auto plan_bytes = [&](size_t rb, size_t sort_bytes) {
        scratch_pieces c{nullptr};
        c.take<mhx_real>(nr * (size_t)rowlen); c.take<mhx_real>(data_block_reals(ndata));
        c.take<mhx_key>(rb * cap); c.take<mhx_key>(rb * cap); c.take<double>(rb * cap); c.take<double>(rb * cap ? rb * cap : 1);
        c.take<char>(sort_bytes ? sort_bytes : 1);
        c.take<double>((size_t)ncb * (size_t)slots * rb * 3);
        c.take<unsigned long long>(rb); c.take<unsigned long long>(rb); c.take<double>(rb); c.take<unsigned>(rb * 2); c.take<double>(rb * 8);
        return c.bytes;
    };
    size_t Rb = std::min<size_t>(nr, (size_t)65535 * (size_t)R), sort_bytes = 0;
    if (cap) Rb = std::min<size_t>(Rb, std::max<size_t>(1, (size_t)0xffffffffull / cap));
    for (;;) {
        if (!sort_bytes_of(Rb, &sort_bytes)) { (void)hipGetLastError(); return mhx_fail(MHX_EHIP, "%s: segmented sort scratch query failed", who); }
        const double need = (double)plan_bytes(Rb, sort_bytes);
        if (need <= budget_mb * 1048576.0) break;
        if (Rb == 1)
            return mhx_fail(MHX_EINVAL, "%s: one data row (a tail of %llu draws, %.3f MB of scratch with the rows and the sort) does not fit option "
                            "PSIS_SCRATCH_MB = %g", who, M, need / 1048576.0, budget_mb);
        Rb = std::max<size_t>(1, std::min<size_t>(Rb - 1, (size_t)((double)Rb * budget_mb * 1048576.0 / need)));
    }
    hipFunction_t f_hist = nullptr, f_gather = nullptr, f_fit = nullptr;
    int rc = user_module(v, "pointwise.hip", "function", source,
                         {{"MHX_HAVE_POINTWISE", "mhx_pointwise_kernels.h"}, {"MHX_HAVE_PSIS", "mhx_psis_kernels.h"}},
                         {"MHX_JIT_PSIS_ROWS=" + std::to_string(R)},
                         {{"mhx_jit_psis_hist", &f_hist}, {"mhx_jit_psis_gather", &f_gather}, {"mhx_jit_psis_fit", &f_fit}});
    if (rc) return rc;
    const size_t P = (size_t)ncb * (size_t)slots;
    mhx_real *d_rows = nullptr, *d_data = nullptr;
    mhx_key *d_tails = nullptr, *d_sorted = nullptr;
    double *d_x = nullptr, *d_tl = nullptr, *d_part = nullptr, *d_tau = nullptr, *d_out = nullptr;
    char* d_sort = nullptr;
    unsigned long long *d_cursor = nullptr, *d_tkey = nullptr;
    unsigned* d_off = nullptr;
    rc = scratch_carve(&ctx->hpd_scratch, &ctx->hpd_bytes, who, "PSIS scratch", [&](scratch_pieces& c) {
        d_rows = c.take<mhx_real>(nr * (size_t)rowlen);     // every data row, once
        d_data = c.take<mhx_real>(data_block_reals(ndata));
        d_tails = c.take<mhx_key>(Rb * cap);                // the keys strictly below the cutoffs, as they arrive
        d_sorted = c.take<mhx_key>(Rb * cap);               // ... ascending
        d_x = c.take<double>(Rb * cap);                     // the abscissae of the fit
        d_tl = c.take<double>(Rb * cap ? Rb * cap : 1);     // the tails as doubles, copies of the cutoff included
        d_sort = c.take<char>(sort_bytes ? sort_bytes : 1);
        d_part = c.take<double>(P * Rb * 3);
        d_cursor = c.take<unsigned long long>(Rb);
        d_tkey = c.take<unsigned long long>(Rb);
        d_tau = c.take<double>(Rb);
        d_off = c.take<unsigned>(Rb * 2);                   // segment begins, then ends
        d_out = c.take<double>(Rb * 8);
    });
    if (rc) { (void)hipGetLastError(); return rc; }
    HIP_TRY(hipMemcpyAsync(d_rows, rows, nr * (size_t)rowlen * sizeof(mhx_real), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = data_block_upload(ctx, d_data, data, ndata))) return rc;
    // phase timing (tools build): return after 1 the select, 2 the gather, 3 the sort, with nothing written to the caller
    const char* stop_opt = MHX_PROBE_OPT(ctx, "PSIS_STOP_AFTER");
    const int stop_after = stop_opt ? atoi(stop_opt) : 0;
    std::vector<double> res(nr * 8), tails(tail_out ? nr * cap : 0), taus(Rb), hout(Rb * 8);
    std::vector<unsigned long long> hkey(Rb), hcur(Rb);
    std::vector<unsigned> hoff(Rb * 2);
    const int64_t rank = (int64_t)M;                        // tau = l_(M), 0-based; M <= 0.2 T < T
    select_landing(ctx, digit, (int32_t)Rb, 1);
    const int d = v.d1 - 1;
    for (size_t r0 = 0; r0 < nr; r0 += Rb) {
        const size_t rb = std::min(Rb, nr - r0);
        const mhx_real* rr = d_rows + r0 * (size_t)rowlen;
        psis_pass_source ps{v, f_hist, rr, d_data, (int)rb, (int)rowlen, (int)ndata, R, ncb, slots};
        rc = mhx_select_drive(who, MHX_KEY_BITS, digit, (int32_t)rb, &rank, 1, S, psis_hist_pass, &ps, taus.data(), ctx->select_landing,
                              ctx->select_landing_words);
        if (rc) return rc;
        if (stop_after == 1) continue;
        for (size_t k = 0; k < rb; ++k) hkey[k] = mhx_select_key_of(taus[k], MHX_KEY_BITS);
        HIP_TRY(hipMemsetAsync(d_cursor, 0, rb * sizeof(uint64_t), ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_tkey, hkey.data(), rb * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_tau, taus.data(), rb * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        const dim3 grid((unsigned)ncb, (unsigned)slots, (unsigned)((rb + (size_t)R - 1) / (size_t)R));
        rc = launch_module(f_gather, grid, MHX_POINTWISE_THREADS, ctx->stream, v.tensor, v.N, v.C, d, rr, (int)rb, (int)rowlen, d_data, (int)ndata,
                           d_tkey, d_tau, M, d_cursor, d_tails, d_part);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(hcur.data(), d_cursor, rb * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        bool any = false;
        for (size_t k = 0; k < rb; ++k) {
            if (hcur[k] > M)
                return mhx_fail(MHX_EHIP, "%s: %llu draws of row %zu lie below its cutoff where at most %llu can (tensor changed during the call?)",
                                who, hcur[k], r0 + k, M);
            hoff[k] = (unsigned)(k * cap);
            hoff[rb + k] = (unsigned)(k * cap + (size_t)hcur[k]);
            any = any || hcur[k] > 0;
        }
        if (stop_after == 2) continue;
        if (any) {                                          // every row's tail on its own, ascending into the second buffer
            HIP_TRY(hipMemcpyAsync(d_off, hoff.data(), rb * 2 * sizeof(unsigned), hipMemcpyHostToDevice, ctx->stream));
            size_t need = sort_bytes;
            if (rocprim::segmented_radix_sort_keys(d_sort, need, d_tails, d_sorted, (unsigned)(rb * cap), (unsigned)rb, d_off, d_off + rb, 0u,
                                                   (unsigned)MHX_KEY_BITS, ctx->stream) != hipSuccess)
                return mhx_fail(MHX_EHIP, "%s: segmented radix sort of the tails failed", who);
        }
        if (stop_after == 3) { HIP_TRY(hipStreamSynchronize(ctx->stream)); continue; }
        rc = launch_module(f_fit, (unsigned)rb, MHX_PSIS_FIT_THREADS, ctx->stream, d_sorted, d_cursor, d_tau, d_part, (long)P, (int)rb, M, (double)S,
                           d_x, d_out, d_tl);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(hout.data(), d_out, rb * 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (tail_out && cap) HIP_TRY(hipMemcpyAsync(tails.data() + r0 * cap, d_tl, rb * cap * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (int c = 0; c < 8; ++c)
            for (size_t k = 0; k < rb; ++k) res[(size_t)c * nr + r0 + k] = hout[(size_t)c * rb + k];
    }
    if (stop_after) return MHX_OK;
    memcpy(out8, res.data(), nr * 8 * sizeof(double));
    if (tail_out && cap) memcpy(tail_out, tails.data(), nr * cap * sizeof(double));
    if (T_out) *T_out = (int64_t)S;
    if (M_out) *M_out = (int64_t)M;
    return MHX_OK;
}

int api_ctx_psis(mhx_ctx* ctx, const mhx_real* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const char* source,
                 const mhx_real* rows, int64_t nrows, int32_t rowlen, const mhx_real* data, size_t ndata, double reff, double* out8,
                 double* tail_out, int64_t* T, int64_t* M)
{
    draws_view v;
    int rc = draws_of_ctx("mhx_ctx_psis", ctx, d_tensor, n_samples, dim1, nchains, &v);
    return rc ? rc : psis_checked(v, source, rows, nrows, rowlen, data, ndata, reff, out8, tail_out, T, M);
}

int api_run_psis(const mhx_run* src, const char* source, const mhx_real* rows, int64_t nrows, int32_t rowlen, const mhx_real* data,
                 size_t ndata, double reff, double* out8, double* tail_out, int64_t* T, int64_t* M)
{
    draws_view v;
    int rc = draws_of_run("mhx_run_psis", src, &v);
    return rc ? rc : psis_checked(v, source, rows, nrows, rowlen, data, ndata, reff, out8, tail_out, T, M);
}
