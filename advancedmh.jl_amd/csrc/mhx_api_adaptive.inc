// adaptive random-walk Metropolis host side (included by mhx_api.hip after mhx_api_tempered.inc): the checks, the tables, the choice
// between the register form and the state-in-HBM form of EACH phase (mhx_rwmh_adaptive_kernels.h, DESIGN.md sections 3.18 and 6.1),
// the seam and the proposal state.  An adaptive run is a RUN_RWMH run of form KF_ADAPTIVE: mhx_run_init and mhx_run_sample drive it
// like any other (rwmh_init, rwmh_advance); rwmh_advance never lets a launch straddle adp_steps and launches `step` before the seam,
// `step_frozen` after it.

// the state-in-HBM forms of the catalogue targets, and the reset of every chain's proposal state
__global__ void __launch_bounds__(256)
k_adaptive_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_adp ad, const int perk)
{
    mhx_adp_generic_body<MHX_TARGET_DYNAMIC, false>(a, tparams, ad, perk);
}
__global__ void __launch_bounds__(256)
k_adaptive_shape_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_adp ad, const int perk)
{
    mhx_adp_generic_body<MHX_TARGET_DYNAMIC, true>(a, tparams, ad, perk);
}
__global__ void __launch_bounds__(256)
k_adaptive_frozen_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ eff, const int perk)
{
    mhx_adp_frozen_generic_body<MHX_TARGET_DYNAMIC>(a, tparams, eff, perk);
}
__global__ void __launch_bounds__(256)
k_adaptive_reset(const mhx_adp ad, const mhx_real* __restrict__ x, const int nchains, const long ld, const int d, const int perk, const int shape)
{
    mhx_adp_reset_body(ad, x, nchains, ld, d, perk, shape);
}

// lam = 0, sig = eff = s, m = the state, v = s * s; the counters at the seam back to 0 (create has no state yet: mhx_run_init)
static int adaptive_reset(mhx_run* r)
{
    hipStream_t st = r->ctx->stream;
    HIP_TRY(hipMemsetAsync(r->d_acc_freeze, 0, (size_t)r->n * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_adaptive_reset, dim3((unsigned)((r->n + 255) / 256)), dim3(256), 0, st, r->adp_a, (const mhx_real*)r->d_x, r->n,
                       (long)r->n, r->dim, r->adp_perk, r->adp_shape);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return MHX_OK;
}

// transition adp_steps is done: the accept counters as they stand, copied on the device
static int adaptive_seam(mhx_run* r)
{
    HIP_TRY(hipMemcpyAsync(r->d_acc_freeze, r->d_acc, (size_t)r->n * sizeof(uint32_t), hipMemcpyDeviceToDevice, r->ctx->stream));
    return MHX_OK;
}

int api_rwmh_create_adaptive(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_proposal_adapt_cfg* ac, mhx_run** out)
{
    const char* me = "mhx_rwmh_create_adaptive";
    if (!ctx || !t || !cfg || !ac || !out) return mhx_fail(MHX_EINVAL, "%s: NULL argument", me);
    if (cfg->dim != t->dim) return mhx_fail(MHX_EINVAL, "%s: proposal dim %d != model dim %d", me, cfg->dim, t->dim);
    if (cfg->nchains <= 0) return mhx_fail(MHX_EINVAL, "%s: nchains must be positive", me);
    const int d = cfg->dim;
    if (cfg->flags & MHX_FLAG_ZIGGURAT) return mhx_fail(MHX_EINVAL, "%s: MHX_FLAG_ZIGGURAT -- an adaptive run draws its normals by Box-Muller only", me);
    if (cfg->flags & MHX_FLAG_STATIC_PROPOSAL)
        return mhx_fail(MHX_EINVAL, "%s: MHX_FLAG_STATIC_PROPOSAL -- an adaptive run is a random walk (a static proposal has no acceptance rate to steer by its scale)", me);
    if (cfg->proposal_kind == MHX_PROP_DENSE) return mhx_fail(MHX_EINVAL, "%s: MHX_PROP_DENSE -- an adaptive run takes an ISO or a DIAG proposal", me);
    if (cfg->proposal_kind != MHX_PROP_ISO && cfg->proposal_kind != MHX_PROP_DIAG)
        return mhx_fail(MHX_EINVAL, "%s: unknown proposal kind %d", me, cfg->proposal_kind);
    if (cfg->reduce_lanes > 1) return mhx_fail(MHX_EINVAL, "%s: reduce_lanes = %d -- an adaptive run is one lane per chain (reduce_lanes 0 or 1)", me, cfg->reduce_lanes);
    const mhx_real* cfg_vec = (const mhx_real*)cfg->proposal_vec;
    const mhx_real* cfg_mean = (const mhx_real*)cfg->proposal_mean;
    if (cfg_mean)
        for (int k = 0; k < d; ++k)
            if (cfg_mean[k] != MHX_R(0.0)) return mhx_fail(MHX_EINVAL, "%s: a proposal mean -- an adaptive run is the zero-mean random walk", me);
    if ((cfg->flags & MHX_FLAG_NO_JIT) && t->kind == MHX_TARGET_USER)
        return mhx_fail(MHX_EINVAL, "%s: MHX_FLAG_NO_JIT with a user target -- its kernels exist only compiled at run time", me);
    const bool iso = cfg->proposal_kind == MHX_PROP_ISO;
    if (iso && !(cfg->proposal_scale > 0.0)) return mhx_fail(MHX_EINVAL, "%s: ISO proposal needs a positive scale", me);
    if (!iso && !cfg_vec) return mhx_fail(MHX_EINVAL, "%s: proposal_vec is NULL", me);
    // ---- NaN in a double field of the cfg = its default
    double a_target = 0.234, a_c = 1.0, a_kappa = 0.6, a_lmin = -20.0, a_lmax = 20.0;
    if (!std::isnan(ac->target_rate)) a_target = ac->target_rate;
    if (!std::isnan(ac->c)) a_c = ac->c;
    if (!std::isnan(ac->kappa)) a_kappa = ac->kappa;
    if (!std::isnan(ac->lam_min)) a_lmin = ac->lam_min;
    if (!std::isnan(ac->lam_max)) a_lmax = ac->lam_max;
    if (ac->adapt_steps < 0) return mhx_fail(MHX_EINVAL, "%s: adapt_steps = %d must not be negative", me, (int)ac->adapt_steps);
    if (!(a_kappa > 0.5 && a_kappa <= 1.0)) return mhx_fail(MHX_EINVAL, "%s: kappa = %g outside (0.5, 1] (the step sizes c t^(-kappa) must sum to infinity and their squares must not)", me, a_kappa);
    if (!(a_c >= 0.0) || !std::isfinite(a_c)) return mhx_fail(MHX_EINVAL, "%s: c = %g must be finite and not negative", me, a_c);
    if (!(a_target > 0.0 && a_target < 1.0)) return mhx_fail(MHX_EINVAL, "%s: target_rate = %g outside (0, 1)", me, a_target);
    if (!std::isfinite(a_lmin) || !std::isfinite(a_lmax) || !(a_lmin <= a_lmax))
        return mhx_fail(MHX_EINVAL, "%s: lam_min = %g, lam_max = %g -- finite, lam_min <= lam_max", me, a_lmin, a_lmax);
    const bool shape = ac->shape != 0;
    const bool perk = shape || !iso;
    // ---- the tables, in the run's width: gamma[adapt_steps] | s[d] | vlo[d] | vhi[d]
    const size_t A = (size_t)ac->adapt_steps, n = (size_t)cfg->nchains, D = (size_t)d;
    std::vector<mhx_real> tab(A + 3 * D, MHX_R(0.0));
    for (size_t q = 1; q <= A; ++q) tab[q - 1] = (mhx_real)std::min(1.0, a_c * std::pow((double)q, -a_kappa));   // one pow, one product in double, rounded once
    for (int k = 0; k < d; ++k) {
        const mhx_real s = iso ? (mhx_real)cfg->proposal_scale : cfg_vec[k];
        if (!(s > MHX_R(0.0)) || !std::isfinite((double)s))
            return mhx_fail(MHX_EINVAL, "%s: proposal standard deviation [%d] = %g -- every one is positive and finite (in the run's width too)", me, k, (double)s);
        const mhx_real vlo = (mhx_real)((double)s * (double)s * 0x1p-40), vhi = (mhx_real)((double)s * (double)s * 0x1p40);
        if (shape && !std::isnormal(vlo))
            return mhx_fail(MHX_EINVAL, "%s: s[%d]^2 2^-40 = %g is not a normal number of the run's width (the floor of the adapted variance)", me, k, (double)s * (double)s * 0x1p-40);
        if (shape && !std::isfinite(vhi))
            return mhx_fail(MHX_EINVAL, "%s: s[%d]^2 2^40 = %g is not finite in the run's width (the ceiling of the adapted variance)", me, k, (double)s * (double)s * 0x1p40);
        tab[A + (size_t)k] = s;
        tab[A + D + (size_t)k] = vlo;
        tab[A + 2 * D + (size_t)k] = vhi;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<mhx_run> r(new mhx_run);
    r->dtype = ctx->dtype;
    r->ctx = ctx; r->target = t; r->kind = RUN_RWMH;
    r->dim = d; r->n = cfg->nchains; r->seed = cfg->seed; r->first_id = cfg->first_chain;
    r->flags = cfg->flags;
    r->prop_kind = cfg->proposal_kind; r->prop_scale = (mhx_real)cfg->proposal_scale;          // (the initial draw is the plain run's)
    r->variant = KF_ADAPTIVE;
    r->adp = true; r->adp_steps = (uint64_t)ac->adapt_steps; r->adp_shape = shape ? 1 : 0; r->adp_perk = perk ? 1 : 0;
    HIP_TRY(hipMalloc(&r->d_pvec, (iso ? 1 : D) * sizeof(mhx_real)));
    if (!iso) COPY_SYNC(ctx->stream, r->d_pvec, cfg_vec, D * sizeof(mhx_real), hipMemcpyHostToDevice);
    const size_t erows = perk ? D : 1, state = n * (1 + erows + (shape ? 3 * D : 0));
    HIP_TRY(hipMalloc(&r->d_adp, (state + tab.size()) * sizeof(mhx_real)));
    COPY_SYNC(ctx->stream, r->d_adp + state, tab.data(), tab.size() * sizeof(mhx_real), hipMemcpyHostToDevice);
    HIP_TRY(hipMalloc(&r->d_acc_freeze, n * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(r->d_acc_freeze, 0, n * sizeof(uint32_t), ctx->stream));
    mhx_adp& ad = r->adp_a;
    ad.lam = r->d_adp;
    ad.eff = ad.lam + n;
    ad.m = shape ? ad.eff + erows * n : nullptr;
    ad.v = shape ? ad.m + D * n : nullptr;
    ad.sig = shape ? ad.v + D * n : nullptr;
    ad.gamma = r->d_adp + state;
    ad.s = ad.gamma + A;
    ad.vlo = ad.s + D;
    ad.vhi = ad.vlo + D;
    ad.target = (mhx_real)a_target;
    ad.lam_min = (mhx_real)a_lmin;
    ad.lam_max = (mhx_real)a_lmax;
    int rc = run_alloc_state(r.get());
    if (rc) return rc;
    const int tk = t->kind;
    // the register forms address a [dim+1][nchains] slab with 32-bit byte offsets; each phase has its own dimension limit
    const bool small = ((uint64_t)d + 1) * (uint64_t)r->n * (uint64_t)sizeof(mhx_real) < (1ull << 32);
    const bool may_reg = !(r->flags & (MHX_FLAG_GENERIC | MHX_FLAG_NO_JIT)) && small &&
                         !(tk == MHX_TARGET_CORR_GAUSS && d > (MHX_REAL64 ? 32 : 64)) && !(tk == MHX_TARGET_IID_NORMAL && t->nparams > 4096);
    r->adp_reg = may_reg && (shape ? d <= MHX_ADAPT_SHAPE_REG_MAX_DIM : d <= MHX_ADAPT_REG_MAX_DIM);
    r->adp_frozen_reg = may_reg && d <= MHX_ADAPT_FROZEN_REG_MAX_DIM;
    // kernel(args, tparams, adaptation block[, perk]) and kernel(args, tparams, eff[, perk])
    if (r->adp_reg) r->step = rec_shape("adaptive register kernel", 64, 64, 0, {&r->k_tp, &r->adp_a});
    else r->step = rec_shape("adaptive state-in-HBM kernel", 256, 256, 0, {&r->k_tp, &r->adp_a, &r->adp_perk});
    if (r->adp_frozen_reg) r->step_frozen = rec_shape("adaptive register kernel (frozen)", 64, 64, 0, {&r->k_tp, &r->adp_a.eff});
    else r->step_frozen = rec_shape("adaptive state-in-HBM kernel (frozen)", 256, 256, 0, {&r->k_tp, &r->adp_a.eff, &r->adp_perk});
    if (r->adp_reg || r->adp_frozen_reg) {
        jit_module* m = nullptr;
        const char* ut = opt(ctx, "REG_UNROLL");
        std::vector<std::string> xo = {"-mllvm", "-pragma-unroll-threshold=4000000"};
        if (!ut || atoi(ut) > 0) { xo.push_back("-mllvm"); xo.push_back(std::string("-amdgpu-unroll-threshold-private=") + (ut ? ut : "100000")); }
        std::vector<std::string> rdefs = {"MHX_JIT_DIM=" + std::to_string(d), "MHX_JIT_TK=" + std::to_string(tk),
                                          "MHX_JIT_PERK=" + std::to_string(r->adp_perk), "MHX_JIT_SHAPE=" + std::to_string(r->adp_shape)};
        if (r->adp_reg) rdefs.push_back("MHX_JIT_ADAPTIVE_REG=1");
        if (r->adp_frozen_reg) rdefs.push_back("MHX_JIT_ADAPTIVE_FROZEN_REG=1");
        rc = jit_compile(ctx, jit_source(t, "mhx_rwmh_adaptive_kernels.h"), rdefs, &m, xo);
        if (rc == MHX_OK && r->adp_reg) rc = rec_bind(&r->step, m, "mhx_jit_adaptive_reg");
        if (rc == MHX_OK && r->adp_frozen_reg) rc = rec_bind(&r->step_frozen, m, "mhx_jit_adaptive_frozen_reg");
        if (rc) return rc;
    }
    if (tk == MHX_TARGET_USER) {
        jit_module* m = nullptr;
        if ((rc = jit_generic_rwmh(t, &m))) return rc;
        if ((rc = jit_function(m, "mhx_jit_rwmh_init", &r->jit_init))) return rc;
        if (!r->adp_reg || !r->adp_frozen_reg) {
            if ((rc = jit_compile(ctx, jit_source(t, "mhx_rwmh_adaptive_kernels.h"),
                                  {"MHX_JIT_ADAPTIVE_GENERIC=1", "MHX_JIT_TK=" + std::to_string(tk), "MHX_JIT_SHAPE=" + std::to_string(r->adp_shape)}, &m))) return rc;
            if (!r->adp_reg && (rc = rec_bind(&r->step, m, "mhx_jit_adaptive_generic"))) return rc;
            if (!r->adp_frozen_reg && (rc = rec_bind(&r->step_frozen, m, "mhx_jit_adaptive_frozen_generic"))) return rc;
        }
    } else {
        if (!r->adp_reg && (rc = rec_bind(&r->step, shape ? (const void*)k_adaptive_shape_generic : (const void*)k_adaptive_generic))) return rc;
        if (!r->adp_frozen_reg && (rc = rec_bind(&r->step_frozen, (const void*)k_adaptive_frozen_generic))) return rc;
    }
    if (!r->adp_reg || !r->adp_frozen_reg) HIP_TRY(hipMalloc(&r->d_ybuf, D * n * sizeof(mhx_real)));
    *out = r.release();
    return MHX_OK;
}

// lam[n], sd[dim][n] (eff; an ISO proposal without shape: its one row under every coordinate), mean[dim][n] (NaN without shape),
// widened exactly; acc_at_freeze[n]
int api_run_proposal_state(mhx_run* r, double* lam, double* sd, double* mean, uint32_t* acc_at_freeze)
{
    const char* me = "mhx_run_proposal_state";
    if (!r || !lam || !sd) return mhx_fail(MHX_EINVAL, "%s: NULL argument", me);
    if (!r->adp) return mhx_fail(MHX_ESTATE, "%s: not an adaptive run (mhx_rwmh_create_adaptive)", me);
    HIP_TRY(hipSetDevice(r->ctx->device));
    const size_t n = (size_t)r->n, D = (size_t)r->dim, erows = r->adp_perk ? D : 1;
    std::vector<mhx_real> h(n * (1 + erows + (r->adp_shape ? D : 0)));          // lam | eff | m: contiguous in d_adp
    COPY_SYNC(r->ctx->stream, h.data(), r->d_adp, h.size() * sizeof(mhx_real), hipMemcpyDeviceToHost);
    for (size_t c = 0; c < n; ++c) lam[c] = (double)h[c];
    for (size_t k = 0; k < D; ++k)
        for (size_t c = 0; c < n; ++c) {
            sd[k * n + c] = (double)h[n + (r->adp_perk ? k : 0) * n + c];
            if (mean) mean[k * n + c] = r->adp_shape ? (double)h[n + erows * n + k * n + c] : std::nan("");
        }
    if (acc_at_freeze) COPY_SYNC(r->ctx->stream, acc_at_freeze, r->d_acc_freeze, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    return MHX_OK;
}
