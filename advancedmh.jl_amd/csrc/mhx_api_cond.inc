// mhx_api_cond.inc -- host side of the conditional proposals (include/mhx.h: mhx_rwmh_create_conditional; DESIGN.md section 3.14;
// kernels: mhx_rwmh_cond_kernels.h).  Part of mhx_api.hip.
//
// Everything that steps or checks such a run is compiled at run time: the parameter map is user source.  The module's source is
// the device math, the user's log-density (a user target), the map, the kernels' header; the kernel key (jit_compile) is that text
// and every define, the list of families among them, so two maps or two patterns of families never share a module.

static std::string cond_source(const mhx_run* r)
{
    std::string s = "#include \"mhx_device_math.h\"\n";
    if (r->target->kind == MHX_TARGET_USER) {
        s += "#line 1 \"user_logdensity.hip\"\n";
        s += r->target->user_src;
        s += "\n#define MHX_HAVE_USER_TARGET 1\n";
    }
    s += "#line 1 \"proposal_params.hip\"\n";
    s += r->cond_src;
    s += "\n#define MHX_HAVE_PROPOSAL_PARAMS 1\n#include \"";
    s += r->variant == KF_COMPOSITE ? "mhx_rwmh_composite_kernels.h" : "mhx_rwmh_cond_kernels.h";
    s += "\"\n";
    return s;
}

// p(x) of the current states: MHX_EINVAL when a chain's parameters are not a distribution's
static int cond_check(mhx_run* r)
{
    mhx_ctx* ctx = r->ctx;
    mhx_rwmh_args a = rwmh_args(r);
    const mhx_fam_comp* fam = r->d_fam;
    const mhx_real* cdata = r->d_cond_data;
    int ncdata = r->cond_ndata;
    mhx_real* pbuf = r->d_cond_p;
    int* nbad = r->d_cond_bad;
    HIP_TRY(hipMemsetAsync(nbad, 0, sizeof(int), ctx->stream));
    const int* ctab = r->d_cmp_tab;                         // (the last argument of a composite run's check kernel only)
    int rc = launch_module(r->jit_cond_check, (unsigned)((r->n + 255) / 256), 256, ctx->stream, a, fam, cdata, ncdata, pbuf, nbad, ctab);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    int bad = 0;
    COPY_SYNC(ctx->stream, &bad, nbad, sizeof bad, hipMemcpyDeviceToHost);
    if (bad) {
        r->initialised = false;
        return mhx_fail(MHX_EINVAL, "conditional proposal: at the given state of %d of %d chains the parameter map does not give a "
                                "distribution (sigma, theta > 0, a < b, everything finite); the run needs mhx_run_init with valid states",
                        bad, r->n);
    }
    return MHX_OK;
}

// What mhx_rwmh_create_conditional and mhx_rwmh_create_composite share once the run's tables are on the device: the chain state,
// the module (the register form when `fits` and the shape allows it -- `reg_flag` and `reg_defines` beside the dimension and the
// target kind --, else the state-in-HBM form) and its launch record, the check kernel, the parameter buffer and the initial kernel of a
// user target.
static int cond_build(mhx_run* r, const bool fits, const char* reg_flag, const std::vector<std::string>& reg_defines, const char* reg_name,
                      const char* generic_flag, const char* generic_name, const char* check_name)
{
    mhx_ctx* ctx = r->ctx;
    const mhx_target* t = r->target;
    const int d = r->dim, tk = t->kind;
    int rc = run_alloc_state(r);
    if (rc) return rc;
    const std::string src = cond_source(r);
    // the register form addresses a [dim+1][nchains] slab with 32-bit byte offsets and holds x, y and parameters in VGPRs
    const bool small = ((uint64_t)d + 1) * (uint64_t)r->n * (uint64_t)sizeof(mhx_real) < (1ull << 32);
    jit_module* m = nullptr;
    if (!(r->flags & MHX_FLAG_GENERIC) && small && fits &&
        !(tk == MHX_TARGET_CORR_GAUSS && d > (MHX_REAL64 ? 32 : 64)) && !(tk == MHX_TARGET_IID_NORMAL && t->nparams > 4096)) {
        // (the unrolling options: see api_rwmh_create_components)
        const char* ut = opt(ctx, "REG_UNROLL");
        std::vector<std::string> xo = {"-mllvm", "-pragma-unroll-threshold=4000000"};
        if (!ut || atoi(ut) > 0) { xo.push_back("-mllvm"); xo.push_back(std::string("-amdgpu-unroll-threshold-private=") + (ut ? ut : "100000")); }
        std::vector<std::string> defs = {reg_flag, "MHX_JIT_DIM=" + std::to_string(d), "MHX_JIT_TK=" + std::to_string(tk)};
        defs.insert(defs.end(), reg_defines.begin(), reg_defines.end());
        rc = jit_compile(ctx, src, defs, &m, xo);
        // kernel(args, tparams, fam, cdata, ncdata): a lane per chain, one wave per block
        r->step = rec_shape("conditional register kernel", 64, 64, 0, {&r->k_tp, &r->d_fam, &r->d_cond_data, &r->cond_ndata});
        if (rc == MHX_OK) rc = rec_bind(&r->step, m, reg_name);
        if (rc) return rc;
        r->fam_reg = true;
    } else {
        if ((rc = jit_compile(ctx, src, {generic_flag, "MHX_JIT_TK=" + std::to_string(tk)}, &m))) return rc;
        // kernel(args, tparams, fam, cdata, ncdata, pbuf, ...): then a composite run's table and block count, a conditional run's
        // static and symmetric flags
        r->cond_static = (r->flags & MHX_FLAG_STATIC_PROPOSAL) ? 1 : 0;
        if (r->variant == KF_COMPOSITE)
            r->step = rec_shape("composite state-in-HBM kernel", 256, 256, 0,
                                {&r->k_tp, &r->d_fam, &r->d_cond_data, &r->cond_ndata, &r->d_cond_p, &r->d_cmp_tab, &r->cmp_nblocks});
        else
            r->step = rec_shape("conditional state-in-HBM kernel", 256, 256, 0,
                                {&r->k_tp, &r->d_fam, &r->d_cond_data, &r->cond_ndata, &r->d_cond_p, &r->cond_static, &r->fam_symmetric});
        if ((rc = rec_bind(&r->step, m, generic_name))) return rc;
        HIP_TRY(hipMalloc(&r->d_ybuf, (size_t)d * (size_t)r->n * sizeof(mhx_real)));
    }
    if ((rc = jit_function(m, check_name, &r->jit_cond_check))) return rc;
    HIP_TRY(hipMalloc(&r->d_cond_p, (r->fam_reg ? 2 : 4) * (size_t)d * (size_t)r->n * sizeof(mhx_real)));
    if (tk == MHX_TARGET_USER) {
        jit_module* mu = nullptr;
        if ((rc = jit_generic_rwmh(t, &mu))) return rc;
        if ((rc = jit_function(mu, "mhx_jit_rwmh_init", &r->jit_init))) return rc;
    }
    return MHX_OK;
}

int api_rwmh_create_conditional(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_proposal_component* comps,
                                int32_t ncomps, const char* params_src, const mhx_real* data, size_t ndata, mhx_run** out)
{
    const char* me = "mhx_rwmh_create_conditional";
    if (!ctx || !t || !cfg || !comps || !params_src || !out) return mhx_fail(MHX_EINVAL, "%s: NULL argument", me);
    if (ndata && !data) return mhx_fail(MHX_EINVAL, "%s: data is NULL", me);
    if (ndata > 0x7fffffffull) return mhx_fail(MHX_EINVAL, "%s: the data block is too large", me);
    if (cfg->dim != t->dim) return mhx_fail(MHX_EINVAL, "%s: proposal dim %d != model dim %d", me, cfg->dim, t->dim);
    if (ncomps != cfg->dim) return mhx_fail(MHX_EINVAL, "%s: %d components for dim %d (one component per parameter)", me, ncomps, cfg->dim);
    if (cfg->nchains <= 0) return mhx_fail(MHX_EINVAL, "%s: nchains must be positive", me);
    if (cfg->flags & MHX_FLAG_NO_JIT)
        return mhx_fail(MHX_EINVAL, "%s: MHX_FLAG_NO_JIT -- the parameter map is source: there is no pre-built kernel to run", me);
    if (cfg->flags & MHX_FLAG_ZIGGURAT)
        return mhx_fail(MHX_EINVAL, "%s: MHX_FLAG_ZIGGURAT -- a family run draws its Normal components by Box-Muller only", me);
    if (cfg->reduce_lanes > 1)
        return mhx_fail(MHX_EINVAL, "%s: reduce_lanes = %d -- a conditional run is one lane per chain (reduce_lanes 0 or 1)", me, cfg->reduce_lanes);
    const int d = cfg->dim;
    if (d >= (1 << 20)) return mhx_fail(MHX_EINVAL, "%s: dim must be below 2^20 (the Gamma blocks are numbered component << 8 | attempt)", me);
    const bool stat = (cfg->flags & MHX_FLAG_STATIC_PROPOSAL) != 0;
    std::vector<mhx_fam_comp> tab;
    std::string pattern;
    { const int rct = fam_build_table(me, comps, d, tab, pattern); if (rct) return rct; }
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<mhx_run> r(new mhx_run);
    r->dtype = ctx->dtype;
    r->ctx = ctx; r->target = t; r->kind = RUN_RWMH;
    r->dim = d; r->n = cfg->nchains; r->seed = cfg->seed; r->first_id = cfg->first_chain;
    r->flags = cfg->flags;
    r->prop_kind = 4;                                        // none of mhx_proposal_kind, nor a family run's 3
    r->variant = KF_COND;
    r->fam_symmetric = (cfg->flags & MHX_FLAG_SYMMETRIC_PROPOSAL) ? 1 : 0;       // (here a static proposal may be declared symmetric too)
    r->cond_src = params_src;
    r->cond_ndata = (int)ndata;
    HIP_TRY(hipMalloc(&r->d_fam, tab.size() * sizeof(mhx_fam_comp)));
    COPY_SYNC(ctx->stream, r->d_fam, tab.data(), tab.size() * sizeof(mhx_fam_comp), hipMemcpyHostToDevice);
    HIP_TRY(hipMalloc(&r->d_cond_data, (ndata ? ndata : 1) * sizeof(mhx_real)));      // (one dummy element keeps the pointer valid)
    if (ndata) COPY_SYNC(ctx->stream, r->d_cond_data, data, ndata * sizeof(mhx_real), hipMemcpyHostToDevice);
    HIP_TRY(hipMalloc(&r->d_cond_bad, sizeof(int)));
    int rc = cond_build(r.get(), d <= MHX_COND_REG_MAX_DIM, "MHX_JIT_COND_REG=1",
                        {"MHX_JIT_FAM_LIST=" + pattern, std::string("MHX_JIT_FAM_STATIC=") + (stat ? "1" : "0"),
                         std::string("MHX_JIT_FAM_SYM=") + (r->fam_symmetric ? "1" : "0")},
                        "mhx_jit_cond_reg", "MHX_JIT_COND_GENERIC=1", "mhx_jit_cond_generic", "mhx_jit_cond_check");
    if (rc) return rc;
    *out = r.release();
    return MHX_OK;
}
