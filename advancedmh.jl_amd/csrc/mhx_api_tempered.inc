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
// ... of an adaptive ladder (mhx_rwmh_create_tempered_adaptive), and the ladder of every slot from its rho outside a step launch
__global__ void __launch_bounds__(256)
k_tempered_adapt_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_tmp_adapt ad, mhx_u32* __restrict__ swapc,
                         const int swap_every, const int R)
{
    mhx_tmp_generic_body<MHX_TARGET_DYNAMIC, true>(a, tparams, nullptr, swapc, swap_every, R, &ad);
}
// ... of an anchored ladder (mhx_rwmh_create_tempered_anchored)
__global__ void __launch_bounds__(256)
k_tempered_anchored_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ tt,
                            mhx_u32* __restrict__ swapc, const int swap_every, const int R, const mhx_tmp_anchor an)
{
    mhx_tmp_generic_body<MHX_TARGET_DYNAMIC, false, true>(a, tparams, tt, swapc, swap_every, R, nullptr, &an);
}
__global__ void __launch_bounds__(256)
k_tempered_derive(const mhx_tmp_adapt ad, const int nchains, const int R) { mhx_tmp_derive_body(ad, nchains, R); }
__global__ void __launch_bounds__(256)
k_tempered_rung(const mhx_real* __restrict__ src, mhx_real* __restrict__ dst, const long rows, const long C, const int R, const int r)
{
    mhx_tmp_rung_body(src, dst, rows, C, R, r);
}

// an adaptive run: rho and beta of every slot back to the initial ladder (create, mhx_run_init)
static int tempered_reset_ladder(mhx_run* r)
{
    if (!r->tmp_adapt) return MHX_OK;
    const size_t n = (size_t)r->n;
    HIP_TRY(hipMemcpyAsync(r->tmp_ad.rho, r->d_tadapt + 2 * n, n * sizeof(mhx_real), hipMemcpyDeviceToDevice, r->ctx->stream));
    hipLaunchKernelGGL(k_tempered_derive, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, r->ctx->stream, r->tmp_ad, r->n, r->tmp_R);
    HIP_TRY(hipGetLastError());
    return MHX_OK;
}

// `ac` NULL: a fixed ladder (mhx_rwmh_create_tempered); else the ladder adapts (mhx_rwmh_create_tempered_adaptive, DESIGN.md section 3.17.1)
// `ref`: a fixed ladder anchored at a reference density (mhx_rwmh_create_tempered_anchored, DESIGN.md section 3.17.2); never with `ac`
static int tempered_create(const char* me, mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_tempered_cfg* tc,
                           const mhx_ladder_adapt_cfg* ac, const mhx_tempered_reference* ref, mhx_run** out)
{
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
    // ---- an anchored ladder: the reference's tables in the run's width, m[d] | w[d], and lc
    std::vector<mhx_real> ta;
    mhx_real ref_lc = MHX_R(0.0);
    if (ref) {
        const double* rm = (const double*)ref->mean;
        const double* rs = (const double*)ref->sd;
        if (!rm || !rs) return mhx_fail(MHX_EINVAL, "%s: the reference's %s is NULL", me, rm ? "sd" : "mean");
        ta.assign((size_t)R + 2 * (size_t)d, MHX_R(0.0));
        double lc = 0.0;
        for (int k = 0; k < d; ++k) {
            if (!std::isfinite(rm[k])) return mhx_fail(MHX_EINVAL, "%s: reference mean[%d] = %g is not finite", me, k, rm[k]);
            if (!std::isfinite(rs[k])) return mhx_fail(MHX_EINVAL, "%s: reference sd[%d] = %g is not finite", me, k, rs[k]);
            if (!(rs[k] > 0.0)) return mhx_fail(MHX_EINVAL, "%s: reference sd[%d] = %g -- every standard deviation is positive (the reference is a proper density)", me, k, rs[k]);
            ta[(size_t)R + k] = (mhx_real)rm[k];
            ta[(size_t)R + d + k] = (mhx_real)(1.0 / rs[k]);                                     // one division in double, rounded once
            if (!std::isfinite((double)ta[(size_t)R + d + k]) || !(ta[(size_t)R + d + k] > MHX_R(0.0)))
                return mhx_fail(MHX_EINVAL, "%s: 1 / reference sd[%d] = %g leaves the run's width", me, k, 1.0 / rs[k]);
            lc -= std::log(rs[k]);
        }
        lc -= 0.5 * (double)d * std::log(2.0 * 3.14159265358979323846);
        ref_lc = (mhx_real)lc;
    }
    // ---- an adaptive ladder: NaN in a field of the cfg = its default
    double a_target = 0.234, a_c = 1.0, a_kappa = 0.6, a_rmin = -10.0, a_rmax = std::log(16.0 / (double)(R - 1));
    if (ac) {
        if (!std::isnan(ac->target_rate)) a_target = ac->target_rate;
        if (!std::isnan(ac->c)) a_c = ac->c;
        if (!std::isnan(ac->kappa)) a_kappa = ac->kappa;
        if (!std::isnan(ac->rho_min)) a_rmin = ac->rho_min;
        if (!std::isnan(ac->rho_max)) a_rmax = ac->rho_max;
        if (tc->swap_every == 0) return mhx_fail(MHX_EINVAL, "%s: swap_every = 0 -- an adaptive ladder tunes itself from its swap rounds", me);
        if (scale) return mhx_fail(MHX_EINVAL, "%s: scale[] given -- the proposal scales of an adaptive ladder follow its temperatures (beta^(-1/2))", me);
        if (ac->adapt_steps < 0) return mhx_fail(MHX_EINVAL, "%s: adapt_steps = %d must not be negative", me, (int)ac->adapt_steps);
        if (!(a_kappa > 0.5 && a_kappa <= 1.0)) return mhx_fail(MHX_EINVAL, "%s: kappa = %g outside (0.5, 1] (the step sizes c s^(-kappa) must sum to infinity and their squares must not)", me, a_kappa);
        if (!(a_c >= 0.0) || !std::isfinite(a_c)) return mhx_fail(MHX_EINVAL, "%s: c = %g must be finite and not negative", me, a_c);
        if (!(a_target > 0.0 && a_target < 1.0)) return mhx_fail(MHX_EINVAL, "%s: target_rate = %g outside (0, 1)", me, a_target);
        if (!std::isfinite(a_rmin) || !std::isfinite(a_rmax) || !(a_rmin <= a_rmax))
            return mhx_fail(MHX_EINVAL, "%s: rho_min = %g, rho_max = %g -- finite, rho_min <= rho_max", me, a_rmin, a_rmax);
        if ((double)(R - 1) * std::exp(a_rmax) > 80.0)
            return mhx_fail(MHX_EINVAL, "%s: (R - 1) exp(rho_max) = %g > 80 -- the coldest beta, exp(-(R - 1) exp(rho_max)), would leave fp32's normal range",
                            me, (double)(R - 1) * std::exp(a_rmax));
    }
    // ---- the table, in the run's width: beta[R] | dbeta[R] | sig[R] or sig[R][d]
    const bool iso = cfg->proposal_kind == MHX_PROP_ISO;
    std::vector<mhx_real> tt((size_t)2 * R + (size_t)R * (iso ? 1 : (size_t)d), MHX_R(0.0));
    if (beta[0] != 1.0) return mhx_fail(MHX_EINVAL, "%s: beta[0] = %g must be exactly 1 (rung 0 is the chain that is read)", me, beta[0]);
    bool end_zero = false;
    for (int r = 0; r < R; ++r) {
        tt[(size_t)r] = (mhx_real)beta[r];
        if (ref && beta[r] == 0.0) {                                // an anchored ladder may END at the reference itself
            if (r != R - 1)
                return mhx_fail(MHX_EINVAL, "%s: beta[%d] = 0 is not the last rung -- only the last inverse temperature of an anchored ladder may be 0", me, r);
            if (!scale)
                return mhx_fail(MHX_EINVAL, "%s: beta[%d] = 0 without scale[] -- the default proposal scale beta^(-1/2) has no value there: give scale[]", me, r);
            end_zero = true;
        } else if (!(beta[r] > 0.0) || !(tt[(size_t)r] > MHX_R(0.0)) || !std::isfinite(beta[r]))
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
    r->variant = ac ? KF_TEMPERED_ADAPT : (ref ? KF_TEMPERED_ANCHOR : KF_TEMPERED);
    r->tmp_R = R; r->tmp_swap_every = tc->swap_every;
    HIP_TRY(hipMalloc(&r->d_pvec, (iso ? 1 : (size_t)d) * sizeof(mhx_real)));
    if (!iso) COPY_SYNC(ctx->stream, r->d_pvec, cfg_vec, (size_t)d * sizeof(mhx_real), hipMemcpyHostToDevice);
    HIP_TRY(hipMalloc(&r->d_ttab, tt.size() * sizeof(mhx_real)));
    COPY_SYNC(ctx->stream, r->d_ttab, tt.data(), tt.size() * sizeof(mhx_real), hipMemcpyHostToDevice);
    HIP_TRY(hipMalloc(&r->d_swapc, 2 * (size_t)r->n * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(r->d_swapc, 0, 2 * (size_t)r->n * sizeof(uint32_t), ctx->stream));
    int rc = run_alloc_state(r.get());
    if (rc) return rc;
    if (ref) {
        for (int q = 0; q < R; ++q) ta[(size_t)q] = MHX_R(1.0) - tt[(size_t)q];                  // one subtraction of the rounded betas
        HIP_TRY(hipMalloc(&r->d_tanchor, ta.size() * sizeof(mhx_real)));
        COPY_SYNC(ctx->stream, r->d_tanchor, ta.data(), ta.size() * sizeof(mhx_real), hipMemcpyHostToDevice);
        r->tmp_anchor = true;
        r->tmp_beta_end_zero = end_zero;
        r->tmp_an.omb = r->d_tanchor;
        r->tmp_an.m = r->d_tanchor + R;
        r->tmp_an.w = r->d_tanchor + R + d;
        r->tmp_an.lc = ref_lc;
    }
    if (ac) {
        // rho0[r] = log(log(beta[r] / beta[r + 1])) in double, rounded once, clamped in the width; gamma[s] = c s^(-kappa), s = 1 ..
        // adapt_steps / swap_every, one pow and one product in double, rounded once.  d_tadapt: rho[n] | beta[n] | rho0[n] | gamma[nrounds]
        const size_t n = (size_t)r->n, nrounds = (size_t)(ac->adapt_steps / tc->swap_every);
        const mhx_real rmin = (mhx_real)a_rmin, rmax = (mhx_real)a_rmax;
        std::vector<mhx_real> h(n + nrounds, MHX_R(0.0));
        for (int q = 0; q + 1 < R; ++q) {
            mhx_real v = (mhx_real)std::log(std::log(beta[q] / beta[q + 1]));
            v = v < rmin ? rmin : (v > rmax ? rmax : v);
            if (!(v == v)) return mhx_fail(MHX_EINVAL, "%s: beta[%d] / beta[%d] = %g has no log log", me, q, q + 1, beta[q] / beta[q + 1]);
            for (size_t c = (size_t)q; c < n; c += (size_t)R) h[c] = v;
        }
        for (size_t s = 1; s <= nrounds; ++s) h[n + s - 1] = (mhx_real)(a_c * std::pow((double)s, -a_kappa));
        HIP_TRY(hipMalloc(&r->d_tadapt, (3 * n + nrounds) * sizeof(mhx_real)));
        COPY_SYNC(ctx->stream, r->d_tadapt + 2 * n, h.data(), (n + nrounds) * sizeof(mhx_real), hipMemcpyHostToDevice);
        r->tmp_adapt = true;
        r->tmp_ad.rho = r->d_tadapt;
        r->tmp_ad.beta = r->d_tadapt + n;
        r->tmp_ad.gamma = r->d_tadapt + 3 * n;
        r->tmp_ad.sigk = r->d_pvec;
        r->tmp_ad.sigma = r->prop_scale;
        r->tmp_ad.target_rate = (mhx_real)a_target;
        r->tmp_ad.rho_min = rmin;
        r->tmp_ad.rho_max = rmax;
        r->tmp_ad.nrounds = (mhx_u32)nrounds;
        if ((rc = tempered_reset_ladder(r.get()))) return rc;
    }
    // the adaptive kernels take the adaptation block where the fixed ones take the table
    const void* tab = ac ? (const void*)&r->tmp_ad : (const void*)&r->d_ttab;
    const int tk = t->kind;
    // the register form addresses a [dim+1][nchains] slab with 32-bit byte offsets and holds x and y in VGPRs
    const bool small = ((uint64_t)d + 1) * (uint64_t)r->n * (uint64_t)sizeof(mhx_real) < (1ull << 32);
    if (!(r->flags & (MHX_FLAG_GENERIC | MHX_FLAG_NO_JIT)) && small && (ref ? d <= MHX_TEMPERED_ANCHORED_REG_MAX_DIM : d <= MHX_TEMPERED_REG_MAX_DIM) &&
        !(tk == MHX_TARGET_CORR_GAUSS && d > (MHX_REAL64 ? 32 : 64)) && !(tk == MHX_TARGET_IID_NORMAL && t->nparams > 4096)) {
        jit_module* m = nullptr;
        const char* ut = opt(ctx, "REG_UNROLL");
        std::vector<std::string> xo = {"-mllvm", "-pragma-unroll-threshold=4000000"};
        if (!ut || atoi(ut) > 0) { xo.push_back("-mllvm"); xo.push_back(std::string("-amdgpu-unroll-threshold-private=") + (ut ? ut : "100000")); }
        std::vector<std::string> rdefs = {"MHX_JIT_TEMPERED_REG=1", "MHX_JIT_DIM=" + std::to_string(d), "MHX_JIT_TK=" + std::to_string(tk),
                                          "MHX_JIT_PK=" + std::to_string(r->prop_kind), "MHX_JIT_R=" + std::to_string(R)};
        if (ac) rdefs.push_back("MHX_JIT_ADAPT=1");                // (a fixed ladder's defines, and so its kernel key, are what they were)
        if (ref) rdefs.push_back("MHX_JIT_ANCHOR=1");
        rc = jit_compile(ctx, jit_source(t, "mhx_rwmh_tempered_kernels.h"),
                         rdefs, &m, xo);
        // kernel(args, tparams, table, swap counters, swap_every): a lane per chain, one wave per block
        // (an anchored ladder: the reference block after them)
        if (ref) r->step = rec_shape("tempered register kernel", 64, 64, 0, {&r->k_tp, tab, &r->d_swapc, &r->tmp_swap_every, &r->tmp_an});
        else r->step = rec_shape("tempered register kernel", 64, 64, 0, {&r->k_tp, tab, &r->d_swapc, &r->tmp_swap_every});
        if (rc == MHX_OK) rc = rec_bind(&r->step, m, ac ? "mhx_jit_tempered_adapt_reg" : (ref ? "mhx_jit_tempered_anchored_reg" : "mhx_jit_tempered_reg"));
        if (rc) return rc;
        r->fam_reg = true;                                  // (mhx_stats.register_form)
    }
    // ... else kernel(args, tparams, table, swap counters, swap_every, R): the state in HBM, whole ladders per 256-thread block
    if (!r->fam_reg && ref) r->step = rec_shape("tempered state-in-HBM kernel", 256, 256, 0, {&r->k_tp, tab, &r->d_swapc, &r->tmp_swap_every, &r->tmp_R, &r->tmp_an});
    else if (!r->fam_reg) r->step = rec_shape("tempered state-in-HBM kernel", 256, 256, 0, {&r->k_tp, tab, &r->d_swapc, &r->tmp_swap_every, &r->tmp_R});
    if (tk == MHX_TARGET_USER) {
        jit_module* m = nullptr;
        if ((rc = jit_generic_rwmh(t, &m))) return rc;
        if ((rc = jit_function(m, "mhx_jit_rwmh_init", &r->jit_init))) return rc;
        if (!r->fam_reg) {
            std::vector<std::string> gdefs = {"MHX_JIT_TEMPERED_GENERIC=1", "MHX_JIT_TK=" + std::to_string(tk)};
            if (ac) gdefs.push_back("MHX_JIT_ADAPT=1");
            if (ref) gdefs.push_back("MHX_JIT_ANCHOR=1");
            if ((rc = jit_compile(ctx, jit_source(t, "mhx_rwmh_tempered_kernels.h"), gdefs, &m))) return rc;
            if ((rc = rec_bind(&r->step, m, ac ? "mhx_jit_tempered_adapt_generic" : (ref ? "mhx_jit_tempered_anchored_generic" : "mhx_jit_tempered_generic")))) return rc;
        }
    } else if (!r->fam_reg && (rc = rec_bind(&r->step, ac ? (const void*)k_tempered_adapt_generic
                                                          : (ref ? (const void*)k_tempered_anchored_generic : (const void*)k_tempered_generic)))) return rc;
    if (!r->fam_reg) HIP_TRY(hipMalloc(&r->d_ybuf, (size_t)d * (size_t)r->n * sizeof(mhx_real)));
    *out = r.release();
    return MHX_OK;
}

int api_rwmh_create_tempered(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_tempered_cfg* tc, mhx_run** out)
{
    return tempered_create("mhx_rwmh_create_tempered", ctx, t, cfg, tc, nullptr, nullptr, out);
}

int api_rwmh_create_tempered_anchored(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_tempered_cfg* tc,
                                      const mhx_tempered_reference* ref, mhx_run** out)
{
    const char* me = "mhx_rwmh_create_tempered_anchored";
    if (!ref) return mhx_fail(MHX_EINVAL, "%s: NULL argument", me);
    return tempered_create(me, ctx, t, cfg, tc, nullptr, ref, out);
}

int api_rwmh_create_tempered_adaptive(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_tempered_cfg* tc,
                                      const mhx_ladder_adapt_cfg* ac, mhx_run** out)
{
    const char* me = "mhx_rwmh_create_tempered_adaptive";
    if (!ac) return mhx_fail(MHX_EINVAL, "%s: NULL argument", me);
    return tempered_create(me, ctx, t, cfg, tc, ac, nullptr, out);
}

// beta[n]: slot c's current temperature, widened exactly.  A fixed ladder: its table.
int api_run_ladder_betas(mhx_run* r, double* beta)
{
    if (!r || !beta) return mhx_fail(MHX_EINVAL, "mhx_run_ladder_betas: NULL argument");
    if (!r->tmp_R) return mhx_fail(MHX_ESTATE, "mhx_run_ladder_betas: not a tempered run (mhx_rwmh_create_tempered)");
    HIP_TRY(hipSetDevice(r->ctx->device));
    const size_t n = (size_t)r->n, R = (size_t)r->tmp_R;
    std::vector<mhx_real> h(r->tmp_adapt ? n : R);
    COPY_SYNC(r->ctx->stream, h.data(), r->tmp_adapt ? (const mhx_real*)r->tmp_ad.beta : (const mhx_real*)r->d_ttab, h.size() * sizeof(mhx_real),
              hipMemcpyDeviceToHost);
    for (size_t c = 0; c < n; ++c) beta[c] = (double)h[r->tmp_adapt ? c : c % R];
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
