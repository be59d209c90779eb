// mhx_api_composite.inc -- host side of the composite proposals (include/mhx.h: mhx_rwmh_create_composite; DESIGN.md section 3.15;
// kernels: mhx_rwmh_composite_kernels.h).  Part of mhx_api.hip.
//
// A composite run is a conditional run (mhx_api_cond.inc) whose kind, symmetric flag and parameter map vary per block of components:
// the table (fam_build_table), the module's source (cond_source), the check of p(x) (cond_check) and the launch (cond_launch) are
// shared.  What is new is the block table: compile-time lists for the register form, a small device table for the state-in-HBM
// form.  The kernel key (jit_compile) holds the source and every define, so two block patterns never share a module.

int api_rwmh_create_composite(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_proposal_component* comps,
                              int32_t ncomps, const mhx_proposal_block* blocks, int32_t nblocks, const int32_t* mapped,
                              const char* params_src, const mhx_real* data, size_t ndata, mhx_run** out)
{
    const char* me = "mhx_rwmh_create_composite";
    if (!ctx || !t || !cfg || !comps || !blocks || !out) return mhx_fail(MHX_EINVAL, "%s: NULL argument", me);
    if (ndata && !data) return mhx_fail(MHX_EINVAL, "%s: data is NULL", me);
    if (ndata > 0x7fffffffull) return mhx_fail(MHX_EINVAL, "%s: the data block is too large", me);
    if (cfg->dim != t->dim) return mhx_fail(MHX_EINVAL, "%s: proposal dim %d != model dim %d", me, cfg->dim, t->dim);
    if (ncomps != cfg->dim) return mhx_fail(MHX_EINVAL, "%s: %d components for dim %d (one component per parameter)", me, ncomps, cfg->dim);
    if (cfg->nchains <= 0) return mhx_fail(MHX_EINVAL, "%s: nchains must be positive", me);
    if (cfg->flags & (MHX_FLAG_STATIC_PROPOSAL | MHX_FLAG_SYMMETRIC_PROPOSAL))
        return mhx_fail(MHX_EINVAL, "%s: MHX_FLAG_STATIC_PROPOSAL / MHX_FLAG_SYMMETRIC_PROPOSAL in cfg->flags -- the blocks carry the kind and the "
                                "symmetric flag (MHX_BLOCK_STATIC, MHX_BLOCK_SYMMETRIC)", me);
    if (cfg->flags & MHX_FLAG_NO_JIT)
        return mhx_fail(MHX_EINVAL, "%s: MHX_FLAG_NO_JIT -- a composite run is compiled at run time: there is no pre-built kernel to run", me);
    if (cfg->flags & MHX_FLAG_ZIGGURAT)
        return mhx_fail(MHX_EINVAL, "%s: MHX_FLAG_ZIGGURAT -- a family run draws its Normal components by Box-Muller only", me);
    if (cfg->reduce_lanes > 1)
        return mhx_fail(MHX_EINVAL, "%s: reduce_lanes = %d -- a composite run is one lane per chain (reduce_lanes 0 or 1)", me, cfg->reduce_lanes);
    const int d = cfg->dim;
    if (d >= (1 << 20)) return mhx_fail(MHX_EINVAL, "%s: dim must be below 2^20 (the Gamma blocks are numbered component << 8 | attempt)", me);
    // the blocks: contiguous, in order, covering 0 .. dim-1 exactly
    if (nblocks < 1 || nblocks > d) return mhx_fail(MHX_EINVAL, "%s: %d blocks for dim %d (between 1 and dim)", me, nblocks, d);
    int next = 0;
    for (int b = 0; b < nblocks; ++b) {
        const mhx_proposal_block& B = blocks[b];
        if (B.first != next || B.count < 1 || B.count > d - next)
            return mhx_fail(MHX_EINVAL, "%s: block %d covers components %d .. %d, expected to start at %d and end below %d (the blocks tile "
                                    "0 .. dim-1 in order)", me, b, B.first, B.first + B.count - 1, next, d);
        if ((B.flags & ~(MHX_BLOCK_STATIC | MHX_BLOCK_SYMMETRIC)) || B.reserved)
            return mhx_fail(MHX_EINVAL, "%s: block %d: unknown flags 0x%x or a non-zero reserved field", me, b, (unsigned)B.flags);
        next += B.count;
    }
    if (next != d) return mhx_fail(MHX_EINVAL, "%s: the blocks cover components 0 .. %d of %d (the blocks tile 0 .. dim-1 in order)", me, next - 1, d);
    const bool have_src = params_src && params_src[0];
    int nmapped = 0;
    if (mapped)
        for (int k = 0; k < d; ++k) {
            if (mapped[k] & ~3) return mhx_fail(MHX_EINVAL, "%s: mapped[%d] = %d (bit 0: parameter 0, bit 1: parameter 1)", me, k, mapped[k]);
            const bool gam = comps[k].family == MHX_FAMILY_GAMMA || comps[k].family == MHX_FAMILY_INVERSE_GAMMA;
            if (gam && (mapped[k] & 1))
                return mhx_fail(MHX_EINVAL, "%s: component %d: the shape alpha of a Gamma / InverseGamma component cannot be mapped (its lgamma "
                                        "would not cancel, and the sampler's constants are derived from it on the host)", me, k);
            if (comps[k].family == MHX_FAMILY_EXPONENTIAL && (mapped[k] & 2))
                return mhx_fail(MHX_EINVAL, "%s: component %d: Exponential has one parameter", me, k);
            nmapped += mapped[k] ? 1 : 0;
        }
    if (nmapped && !have_src) return mhx_fail(MHX_EINVAL, "%s: a mapped mask without params_src", me);
    if (!nmapped && have_src) return mhx_fail(MHX_EINVAL, "%s: params_src without a mapped parameter (mapped is NULL or all zero)", me);
    std::vector<mhx_fam_comp> tab;
    std::string pattern;
    { const int rct = fam_build_table(me, comps, d, tab, pattern); if (rct) return rct; }
    // the lists of the register form and the table of the state-in-HBM form
    std::vector<int> ctab((size_t)(2 * d + 3 * nblocks));
    std::string l_stat, l_blk, l_mask, l_sym;
    int nzblocks = 0;                                        // blocks that carry a Z: not symmetric, some component mapped
    for (int b = 0; b < nblocks; ++b) {
        const int st = (blocks[b].flags & MHX_BLOCK_STATIC) ? 1 : 0, sy = (blocks[b].flags & MHX_BLOCK_SYMMETRIC) ? 1 : 0;
        ctab[(size_t)(2 * d + 3 * b)] = blocks[b].first;
        ctab[(size_t)(2 * d + 3 * b + 1)] = blocks[b].count;
        ctab[(size_t)(2 * d + 3 * b + 2)] = (st ? MHX_CMP_STATIC : 0) | (sy ? MHX_CMP_SYMMETRIC : 0);
        l_sym += (b ? "," : "") + std::to_string(sy);
        bool any_mapped = false;
        for (int k = blocks[b].first; k < blocks[b].first + blocks[b].count; ++k) {
            const int mk = mapped ? mapped[k] : 0;
            ctab[(size_t)(2 * k)] = st ? MHX_CMP_STATIC : 0;
            ctab[(size_t)(2 * k + 1)] = mk;
            l_stat += (k ? "," : "") + std::to_string(st);
            l_blk += (k ? "," : "") + std::to_string(b);
            l_mask += (k ? "," : "") + std::to_string(mk);
            any_mapped = any_mapped || mk != 0;
        }
        nzblocks += (any_mapped && !sy) ? 1 : 0;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<mhx_run> r(new mhx_run);
    r->dtype = ctx->dtype;
    r->ctx = ctx; r->target = t; r->kind = RUN_RWMH;
    r->dim = d; r->n = cfg->nchains; r->seed = cfg->seed; r->first_id = cfg->first_chain;
    r->flags = cfg->flags;
    r->prop_kind = 5;                                        // none of mhx_proposal_kind, nor a family run's 3 or a conditional run's 4
    r->variant = KF_COMPOSITE;
    r->cond_src = have_src ? params_src : "MHX_PROPOSAL_PARAMS(x, p, d, data, ndata) {}\n";     // nothing mapped: the empty map
    r->cond_ndata = (int)ndata;
    r->cmp_nblocks = nblocks;
    r->cmp_mapped = nmapped != 0;
    HIP_TRY(hipMalloc(&r->d_fam, tab.size() * sizeof(mhx_fam_comp)));
    COPY_SYNC(ctx->stream, r->d_fam, tab.data(), tab.size() * sizeof(mhx_fam_comp), hipMemcpyHostToDevice);
    HIP_TRY(hipMalloc(&r->d_cmp_tab, ctab.size() * sizeof(int)));
    COPY_SYNC(ctx->stream, r->d_cmp_tab, ctab.data(), ctab.size() * sizeof(int), hipMemcpyHostToDevice);
    HIP_TRY(hipMalloc(&r->d_cond_data, (ndata ? ndata : 1) * sizeof(mhx_real)));      // (one dummy element keeps the pointer valid)
    if (ndata) COPY_SYNC(ctx->stream, r->d_cond_data, data, ndata * sizeof(mhx_real), hipMemcpyHostToDevice);
    HIP_TRY(hipMalloc(&r->d_cond_bad, sizeof(int)));
    // the register rule: mhx_rwmh_composite_kernels.h
    const bool fits = nmapped ? 2 * d + nmapped + nzblocks / 2 <= MHX_COMPOSITE_REG_COST_MAX : d <= MHX_FAM_REG_MAX_DIM;
    int rc = cond_build(r.get(), fits, "MHX_JIT_COMPOSITE_REG=1",
                        {"MHX_JIT_FAM_LIST=" + pattern, "MHX_JIT_CMP_STATIC_LIST=" + l_stat, "MHX_JIT_CMP_BLOCK_LIST=" + l_blk,
                         "MHX_JIT_CMP_MAPPED_LIST=" + l_mask, "MHX_JIT_CMP_SYM_LIST=" + l_sym},
                        "mhx_jit_composite_reg", "MHX_JIT_COMPOSITE_GENERIC=1", "mhx_jit_composite_generic", "mhx_jit_composite_check");
    if (rc) return rc;
    *out = r.release();
    return MHX_OK;
}
