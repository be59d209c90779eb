// parallel tempering host side (included by mhx_api.hip after mhx_api_derive.inc): the checks, the tempering table, the choice between
// the register form and the state-in-HBM form (mhx_rwmh_tempered_kernels.h, DESIGN.md sections 3.17 and 6.1), the swap statistics and
// the rung snapshot.  A tempered run is a RUN_RWMH run of form KF_TEMPERED: mhx_run_init and mhx_run_sample drive it like any other
// (rwmh_init, rwmh_advance); its step kernel takes the table, the swap counters and the swap period after the per-launch block.

// the state-in-HBM form of the catalogue targets, and the gather of one rung
__global__ void __launch_bounds__(256)
k_tempered_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ tt, mhx_u32* __restrict__ swapc,
                   const int swap_every, const int R)
{
    mhx_tmp_generic_body<MHX_TARGET_DYNAMIC>(a, tparams, tt, swapc, swap_every, R);
}
__global__ void __launch_bounds__(256)
k_tempered_rung(const mhx_real* __restrict__ src, mhx_real* __restrict__ dst, const long rows, const long C, const int R, const int r)
{
    mhx_tmp_rung_body(src, dst, rows, C, R, r);
}

int api_rwmh_create_tempered(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_tempered_cfg* tc, mhx_run** out)
{
    const char* me = "mhx_rwmh_create_tempered";
    if (!ctx || !t || !cfg || !tc || !out) return mhx_fail(MHX_EINVAL, "%s: NULL argument", me);
    if (cfg->dim != t->dim) return mhx_fail(MHX_EINVAL, "%s: proposal dim %d != model dim %d", me, cfg->dim, t->dim);
    if (cfg->nchains <= 0) return mhx_fail(MHX_EINVAL, "%s: nchains must be positive", me);
    const int R = tc->R, d = cfg->dim;
    if (R < 2 || R > 64 || (R & (R - 1)))
        return mhx_fail(MHX_EINVAL, "%s: R = %d -- a ladder has a power of two of rungs, 2 <= R <= 64 (it sits in consecutive lanes of one wave)", me, R);
    if (cfg->nchains % R) return mhx_fail(MHX_EINVAL, "%s: nchains = %d is not a multiple of R = %d (whole ladders only)", me, cfg->nchains, R);
    if (cfg->first_chain % (uint64_t)R)
        return mhx_fail(MHX_EINVAL, "%s: first_chain = %llu is not a multiple of R = %d (a shard begins with a ladder)", me,
                        (unsigned long long)cfg->first_chain, R);
    if (tc->swap_every < 0) return mhx_fail(MHX_EINVAL, "%s: swap_every = %d must not be negative (0: no swap rounds)", me, tc->swap_every);
    if (cfg->flags & MHX_FLAG_ZIGGURAT) return mhx_fail(MHX_EINVAL, "%s: MHX_FLAG_ZIGGURAT -- a tempered run draws its normals by Box-Muller only", me);
    if (cfg->flags & MHX_FLAG_STATIC_PROPOSAL)
        return mhx_fail(MHX_EINVAL, "%s: MHX_FLAG_STATIC_PROPOSAL -- a tempered run is a random walk (a static proposal has no scale to temper)", me);
    if (cfg->proposal_kind == MHX_PROP_DENSE) return mhx_fail(MHX_EINVAL, "%s: MHX_PROP_DENSE -- a tempered run takes an ISO or a DIAG proposal", me);
    if (cfg->proposal_kind != MHX_PROP_ISO && cfg->proposal_kind != MHX_PROP_DIAG)
        return mhx_fail(MHX_EINVAL, "%s: unknown proposal kind %d", me, cfg->proposal_kind);
    if (cfg->reduce_lanes > 1) return mhx_fail(MHX_EINVAL, "%s: reduce_lanes = %d -- a tempered run is one lane per chain (reduce_lanes 0 or 1)", me, cfg->reduce_lanes);
    const mhx_real* cfg_vec = (const mhx_real*)cfg->proposal_vec;
    const mhx_real* cfg_mean = (const mhx_real*)cfg->proposal_mean;
    if (cfg_mean)
        for (int k = 0; k < d; ++k)
            if (cfg_mean[k] != MHX_R(0.0)) return mhx_fail(MHX_EINVAL, "%s: a proposal mean -- a tempered run is the zero-mean random walk", me);
    if ((cfg->flags & MHX_FLAG_NO_JIT) && t->kind == MHX_TARGET_USER)
        return mhx_fail(MHX_EINVAL, "%s: MHX_FLAG_NO_JIT with a user target -- its kernels exist only compiled at run time", me);
    if (cfg->proposal_kind == MHX_PROP_ISO && !(cfg->proposal_scale > 0.0)) return mhx_fail(MHX_EINVAL, "%s: ISO proposal needs a positive scale", me);
    if (cfg->proposal_kind == MHX_PROP_DIAG && !cfg_vec) return mhx_fail(MHX_EINVAL, "%s: proposal_vec is NULL", me);
    const double* beta = (const double*)tc->beta;
    const double* scale = (const double*)tc->scale;
    if (!beta) return mhx_fail(MHX_EINVAL, "%s: beta is NULL", me);
    // ---- the table, in the run's width: beta[R] | dbeta[R] | sig[R] or sig[R][d]
    const bool iso = cfg->proposal_kind == MHX_PROP_ISO;
    std::vector<mhx_real> tt((size_t)2 * R + (size_t)R * (iso ? 1 : (size_t)d), MHX_R(0.0));
    if (beta[0] != 1.0) return mhx_fail(MHX_EINVAL, "%s: beta[0] = %g must be exactly 1 (rung 0 is the chain that is read)", me, beta[0]);
    for (int r = 0; r < R; ++r) {
        tt[(size_t)r] = (mhx_real)beta[r];
        if (!(beta[r] > 0.0) || !(tt[(size_t)r] > MHX_R(0.0)) || !std::isfinite(beta[r]))
            return mhx_fail(MHX_EINVAL, "%s: beta[%d] = %g -- every inverse temperature is positive (in the run's width too)", me, r, beta[r]);
        // (no swap rounds: equal temperatures are allowed, so that the cost of the frame can be timed against the plain run)
        if (r && (tc->swap_every > 0 ? !(tt[(size_t)r] < tt[(size_t)r - 1]) : !(tt[(size_t)r] <= tt[(size_t)r - 1])))
            return mhx_fail(MHX_EINVAL, "%s: beta[%d] = %g after beta[%d] = %g -- the ladder must be strictly decreasing (as rounded to the run's width)",
                            me, r, beta[r], r - 1, beta[r - 1]);
    }
    for (int r = 0; r + 1 < R; ++r) tt[(size_t)R + r] = tt[(size_t)r] - tt[(size_t)r + 1];          // one subtraction of the rounded values
    if (scale && scale[0] != 1.0) return mhx_fail(MHX_EINVAL, "%s: scale[0] = %g must be exactly 1 (rung 0 is the plain chain)", me, scale[0]);
    for (int r = 0; r < R; ++r) {
        const double s = scale ? scale[r] : (r ? 1.0 / std::sqrt((double)beta[r]) : 1.0);
        if (!(s > 0.0) || !std::isfinite(s)) return mhx_fail(MHX_EINVAL, "%s: scale[%d] = %g -- every proposal scale is positive and finite", me, r, s);
        if (iso) tt[(size_t)2 * R + r] = (mhx_real)(s * cfg->proposal_scale);                       // one product in double, rounded once
        else for (int k = 0; k < d; ++k) tt[(size_t)2 * R + (size_t)r * d + k] = (mhx_real)(s * (double)cfg_vec[k]);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<mhx_run> r(new mhx_run);
    r->dtype = ctx->dtype;
    r->ctx = ctx; r->target = t; r->kind = RUN_RWMH;
    r->dim = d; r->n = cfg->nchains; r->seed = cfg->seed; r->first_id = cfg->first_chain;
    r->flags = cfg->flags;
    r->prop_kind = cfg->proposal_kind; r->prop_scale = (mhx_real)cfg->proposal_scale;          // (the initial draw is the plain run's)
    r->variant = KF_TEMPERED;
    r->tmp_R = R; r->tmp_swap_every = tc->swap_every;
    HIP_TRY(hipMalloc(&r->d_pvec, (iso ? 1 : (size_t)d) * sizeof(mhx_real)));
    if (!iso) COPY_SYNC(ctx->stream, r->d_pvec, cfg_vec, (size_t)d * sizeof(mhx_real), hipMemcpyHostToDevice);
    HIP_TRY(hipMalloc(&r->d_ttab, tt.size() * sizeof(mhx_real)));
    COPY_SYNC(ctx->stream, r->d_ttab, tt.data(), tt.size() * sizeof(mhx_real), hipMemcpyHostToDevice);
    HIP_TRY(hipMalloc(&r->d_swapc, 2 * (size_t)r->n * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(r->d_swapc, 0, 2 * (size_t)r->n * sizeof(uint32_t), ctx->stream));
    int rc = run_alloc_state(r.get());
    if (rc) return rc;
    const int tk = t->kind;
    // the register form addresses a [dim+1][nchains] slab with 32-bit byte offsets and holds x and y in VGPRs
    const bool small = ((uint64_t)d + 1) * (uint64_t)r->n * (uint64_t)sizeof(mhx_real) < (1ull << 32);
    if (!(r->flags & (MHX_FLAG_GENERIC | MHX_FLAG_NO_JIT)) && small && d <= MHX_TEMPERED_REG_MAX_DIM &&
        !(tk == MHX_TARGET_CORR_GAUSS && d > (MHX_REAL64 ? 32 : 64)) && !(tk == MHX_TARGET_IID_NORMAL && t->nparams > 4096)) {
        jit_module* m = nullptr;
        const char* ut = opt(ctx, "REG_UNROLL");
        std::vector<std::string> xo = {"-mllvm", "-pragma-unroll-threshold=4000000"};
        if (!ut || atoi(ut) > 0) { xo.push_back("-mllvm"); xo.push_back(std::string("-amdgpu-unroll-threshold-private=") + (ut ? ut : "100000")); }
        rc = jit_compile(ctx, jit_source(t, "mhx_rwmh_tempered_kernels.h"),
                         {"MHX_JIT_TEMPERED_REG=1", "MHX_JIT_DIM=" + std::to_string(d), "MHX_JIT_TK=" + std::to_string(tk),
                          "MHX_JIT_PK=" + std::to_string(r->prop_kind), "MHX_JIT_R=" + std::to_string(R)}, &m, xo);
        // kernel(args, tparams, table, swap counters, swap_every): a lane per chain, one wave per block
        r->step = rec_shape("tempered register kernel", 64, 64, 0, {&r->k_tp, &r->d_ttab, &r->d_swapc, &r->tmp_swap_every});
        if (rc == MHX_OK) rc = rec_bind(&r->step, m, "mhx_jit_tempered_reg");
        if (rc) return rc;
        r->fam_reg = true;                                  // (mhx_stats.register_form)
    }
    // ... else kernel(args, tparams, table, swap counters, swap_every, R): the state in HBM, whole ladders per 256-thread block
    if (!r->fam_reg) r->step = rec_shape("tempered state-in-HBM kernel", 256, 256, 0, {&r->k_tp, &r->d_ttab, &r->d_swapc, &r->tmp_swap_every, &r->tmp_R});
    if (tk == MHX_TARGET_USER) {
        jit_module* m = nullptr;
        if ((rc = jit_generic_rwmh(t, &m))) return rc;
        if ((rc = jit_function(m, "mhx_jit_rwmh_init", &r->jit_init))) return rc;
        if (!r->fam_reg) {
            if ((rc = jit_compile(ctx, jit_source(t, "mhx_rwmh_tempered_kernels.h"), {"MHX_JIT_TEMPERED_GENERIC=1", "MHX_JIT_TK=" + std::to_string(tk)}, &m))) return rc;
            if ((rc = rec_bind(&r->step, m, "mhx_jit_tempered_generic"))) return rc;
        }
    } else if (!r->fam_reg && (rc = rec_bind(&r->step, (const void*)k_tempered_generic))) return rc;
    if (!r->fam_reg) HIP_TRY(hipMalloc(&r->d_ybuf, (size_t)d * (size_t)r->n * sizeof(mhx_real)));
    *out = r.release();
    return MHX_OK;
}

int api_run_swap_stats(mhx_run* r, uint64_t* attempts, uint64_t* swaps)
{
    if (!r) return mhx_fail(MHX_EINVAL, "mhx_run_swap_stats: run is NULL");
    if (!r->tmp_R) return mhx_fail(MHX_ESTATE, "mhx_run_swap_stats: not a tempered run (mhx_rwmh_create_tempered)");
    HIP_TRY(hipSetDevice(r->ctx->device));
    const size_t n = (size_t)r->n;
    std::vector<uint32_t> h(2 * n);
    COPY_SYNC(r->ctx->stream, h.data(), r->d_swapc, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    const int R = r->tmp_R;
    for (int p = 0; p + 1 < R; ++p) {
        uint64_t a = 0, s = 0;
        for (size_t c = (size_t)p; c < n; c += (size_t)R) { a += h[c]; s += h[n + c]; }         // the lower slot of pair (p, p + 1) of every ladder
        if (attempts) attempts[p] = a;
        if (swaps) swaps[p] = s;
    }
    return MHX_OK;
}

int api_run_rung(mhx_run* src, int32_t rung, mhx_run** out)
{
    const char* who = "mhx_run_rung";
    if (!src || !out) return mhx_fail(MHX_EINVAL, "%s: NULL argument", who);
    if (!src->tmp_R) return mhx_fail(MHX_ESTATE, "%s: not a tempered run (mhx_rwmh_create_tempered)", who);
    if (rung < 0 || rung >= src->tmp_R) return mhx_fail(MHX_EINVAL, "%s: rung %d out of range [0, %d)", who, (int)rung, src->tmp_R);
    draws_view v;
    int rc = draws_of_run(who, src, &v);
    if (rc) return rc;
    mhx_ctx* ctx = v.ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const long L = v.C / src->tmp_R, rows = v.N * (long)v.d1;
    std::unique_ptr<mhx_run> r(new mhx_run);
    r->dtype = ctx->dtype;
    r->ctx = ctx;
    r->kind = RUN_DERIVED;
    r->dim = v.d1 - 1;
    r->n = (int)L;
    r->seed = v.seed;
    r->first_id = v.first_id;
    rc = ensure_buffer((void**)&r->d_samples, &r->samples_cap, (size_t)rows * (size_t)L * sizeof(mhx_real), who, "rung sample tensor");
    if (rc) { (void)hipGetLastError(); return rc; }
    const long total = rows * L;
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    hipLaunchKernelGGL(k_tempered_rung, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, v.tensor, r->d_samples, rows, v.C,
                       src->tmp_R, (int)rung);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    r->n_saved = v.N;
    r->stats.kernel_ms = ms;
    r->stats.kernel_variant = -1;                           // none of enum kernel_form: mhx_run_form_name says "derived"
    r->stats.launches = 1;
    r->stats.dtype = r->dtype;
    r->stats.factor_band = -1;
    *out = r.release();
    return MHX_OK;
}
