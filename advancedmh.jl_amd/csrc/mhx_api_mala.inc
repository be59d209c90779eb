// MALA host side (included by mhx_api.hip): src/MALA.jl:1-105

__global__ void __launch_bounds__(256)
k_mala(const mhx_mala_args a, const mhx_real* __restrict__ tparams)
{
    mhx_mala_body<MHX_TARGET_DYNAMIC>(a, tparams);
}
__global__ void __launch_bounds__(256)
k_mala_init(const mhx_mala_args a, const mhx_real* __restrict__ tparams, const int reset_counts)
{
    mhx_mala_init_body<MHX_TARGET_DYNAMIC>(a, tparams, reset_counts);
}

#define MHX_MALA_REG_MAX_DIM (MHX_REAL64 ? 24 : 48)
// above it, up to here: candidate and its gradient in registers, the tails of state / gradient / noise in LDS (mhx_mala_reg_body<.., XR>)
#define MHX_MALA_SPLIT_MAX_DIM (MHX_REAL64 ? 64 : 128)
#define MHX_MALA_REG_MAX_DIM_DENSE (MHX_REAL64 ? 16 : 32)

static mhx_mala_args mala_args(const mhx_run* r)
{
    mhx_mala_args a;
    memset(&a, 0, sizeof a);
    a.x = r->d_x; a.gx = r->d_gx; a.lp = r->d_lp; a.acc_count = r->d_acc; a.acc_total = r->d_acc_total;
    a.samples = r->d_samples; a.accepted = r->d_accepted; a.last_acc = r->d_last;
    a.ybuf = r->d_ybuf; a.gybuf = r->d_gy; a.zbuf = r->d_z;
    a.seed = r->seed; a.first_chain = r->first_id;
    a.nchains = r->n; a.ld = r->n; a.dim = r->dim;
    a.target_kind = r->target->kind; a.ntparams = r->target->nparams; a.tconst = r->target->cst;
    a.sigma = r->mala_sigma; a.h = (r->mala_sigma * r->mala_sigma) * MHX_R(0.5); a.hs = MHX_R(0.5) * r->mala_sigma;
    a.save_next = MHX_NO_SAVE; a.thinning = 1;
    a.reduce_lanes = r->coop_L;
    return a;
}

// the matrix-core MALA kernels that stream their operands: the images of A and of A^T, side by side in global memory, built by
// the module's own fill kernels
static int mala_mfma_images(mhx_run* r, jit_module* m)
{
    hipFunction_t fimg = nullptr, fimgT = nullptr;
    int rc = jit_function(m, "mhx_jit_mfma_image", &fimg);
    if (rc == MHX_OK) rc = jit_function(m, "mhx_jit_mfma_image_T", &fimgT);
    if (rc) return rc;
    const size_t ra = mfma_image_reals(r->dim), rt = mfma_image_reals_T(r->dim);
    HIP_TRY(hipMalloc(&r->d_mfma_img, (ra + rt) * sizeof(mhx_real)));
    const mhx_real* src = r->target->dparams;
    mhx_real* dst = r->d_mfma_img;
    rc = launch_module(fimg, 1, 256, r->ctx->stream, src, dst);
    mhx_real* dstT = r->d_mfma_img2 = r->d_mfma_img + ra;
    if (rc == MHX_OK) rc = launch_module(fimgT, 1, 256, r->ctx->stream, src, dstT);
    if (rc == MHX_OK) HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    return rc;
}

int api_mala_create(mhx_ctx* ctx, const mhx_target* t, const mhx_mala_cfg* cfg, mhx_run** out)
{
    if (!ctx || !t || !cfg || !out) return mhx_fail(MHX_EINVAL, "mhx_mala_create: NULL argument");
    if (cfg->dim != t->dim) return mhx_fail(MHX_EINVAL, "mhx_mala_create: dim %d != model dim %d", cfg->dim, t->dim);
    if (cfg->nchains <= 0) return mhx_fail(MHX_EINVAL, "mhx_mala_create: nchains must be positive");
    if (!(cfg->sigma2 > 0.0)) return mhx_fail(MHX_EINVAL, "mhx_mala_create: sigma2 must be positive");
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<mhx_run> r(new mhx_run);
    r->dtype = ctx->dtype;
    r->ctx = ctx; r->target = t; r->kind = RUN_MALA;
    r->dim = cfg->dim; r->n = cfg->nchains; r->seed = cfg->seed; r->first_id = cfg->first_chain;
    r->flags = cfg->flags; r->mala_sigma = std::sqrt((mhx_real)cfg->sigma2);     // rounded to the engine type first, like the oracle
    // the register / cooperative kernels address a [dim+1][nchains] slab with 32-bit byte offsets (like mhx_rwmh_create)
    if (((uint64_t)r->dim + 1) * (uint64_t)r->n * (uint64_t)sizeof(mhx_real) >= (1ull << 32)) r->flags |= MHX_FLAG_GENERIC;
    int rc = run_alloc_state(r.get());
    if (rc) return rc;
    const size_t slab = (size_t)r->dim * (size_t)r->n * sizeof(mhx_real);
    HIP_TRY(hipMalloc(&r->d_gx, slab));
    HIP_TRY(hipMalloc(&r->d_ybuf, slab));
    HIP_TRY(hipMalloc(&r->d_gy, slab));
    HIP_TRY(hipMalloc(&r->d_z, slab));
    // compile-time dimension: state, gradients, candidate and noise in registers (5 d floats per lane)
    const bool user = t->kind == MHX_TARGET_USER;
    const int regmax = t->kind == MHX_TARGET_CORR_GAUSS ? MHX_MALA_REG_MAX_DIM_DENSE : MHX_MALA_REG_MAX_DIM;
    const bool split = t->kind != MHX_TARGET_CORR_GAUSS && r->dim > regmax && r->dim <= MHX_MALA_SPLIT_MAX_DIM;
    const bool want_reg = !(r->flags & (MHX_FLAG_GENERIC | MHX_FLAG_NO_JIT)) && (r->dim <= regmax || split) &&
                          !(t->kind == MHX_TARGET_IID_NORMAL && t->nparams > 4096);
    r->variant = KF_GENERIC;
    // a launch record of this sampler: kernel(args, tparams)
    auto rec = [&](const char* what, unsigned block, int per_block, size_t lds) { return rec_shape(what, block, per_block, lds, {&r->k_tp}); };
    // MHX_FLAG_ZIGGURAT (round 5): the noise by the table ziggurat -- the lane-per-chain register kernel's form (both widths, any target
    // with a gradient, d within that kernel's reach); the cooperative / matrix-core / state-in-HBM kernels draw Box-Muller
    const bool zig = (cfg->flags & MHX_FLAG_ZIGGURAT) != 0;
    if (zig && (!want_reg || cfg->reduce_lanes > 1))
        return mhx_fail(MHX_EINVAL, "MHX_FLAG_ZIGGURAT: MALA has the ziggurat on its lane-per-chain register kernel only (dim <= %d, reduce_lanes <= 1, "
                        "no MHX_FLAG_GENERIC / MHX_FLAG_NO_JIT)", split ? MHX_MALA_SPLIT_MAX_DIM : regmax);
    // cooperative kernel (L lanes per chain, everything in registers) for the separable catalogue targets: asked for
    // (reduce_lanes > 1), or by default where the lane-per-chain register kernel does not reach (d above its budget)
    const bool separable = t->kind == MHX_TARGET_ISO_GAUSS || t->kind == MHX_TARGET_BANANA || t->kind == MHX_TARGET_FUNNEL;
    // the dense Gaussian target on the matrix cores (mhx_mala_mfma_kernels.h): value and gradient are two triangular GEMMs
    // with the ONE factor all chains share; reduction shape 4.  Asked for (reduce_lanes = 4), or by default above the
    // register kernel's budget, wherever both operand images fit LDS
    const size_t mfma_lds = (mfma_image_reals(r->dim) + mfma_image_reals_T(r->dim)) * sizeof(mhx_real);
    const bool no_mfma = opt_on(ctx, "NO_MFMA");                                  // tuning knob
    const bool mfma = t->kind == MHX_TARGET_CORR_GAUSS && !(r->flags & (MHX_FLAG_GENERIC | MHX_FLAG_NO_JIT)) && r->dim >= 16 &&
                      !zig && (cfg->reduce_lanes == 4 || (cfg->reduce_lanes == 0 && r->dim > regmax)) && mfma_lds <= MHX_LDS_PER_BLOCK &&
                      ((uint64_t)r->dim + 1) * (uint64_t)r->n * sizeof(mhx_real) < (1ull << 32) &&      // 32-bit slab offsets
                      !no_mfma;
    // ... and where they do not: both images in global memory, walked through an LDS ring; x and grad(x) re-read from their slabs
    // (candidate, noise, w and the candidate's gradient are what a lane keeps: 4 ceil(d/4) reals)
    const int mNS = (r->dim + 3) / 4, mNT = (r->dim + 15) / 16;
    // the ring of the A^T image: mhx_mfma_stream_geom<D, pair = true, trans = true>::BUF_BYTES on the device side, which rounds
    // a chunk up to whole rounds of the block's threads (64 * MHX_MFMA_WAVES) -- the same expression here, not a literal 256
    constexpr int ring_threads = 64 * MHX_MFMA_WAVES;
    const size_t ringT = (size_t)2 * (((2 * mNT - 1) * 64 * ((int)(4 * sizeof(mhx_real)) / 16) + ring_threads - 1) / ring_threads) * ring_threads * 16;
    const size_t mala_ring = std::max(mfma_ring_bytes(r->dim, true), ringT);
    const bool mfma_s = !mfma && t->kind == MHX_TARGET_CORR_GAUSS && !(r->flags & (MHX_FLAG_GENERIC | MHX_FLAG_NO_JIT)) && r->dim >= 16 &&
                        (cfg->reduce_lanes == 4 || (cfg->reduce_lanes == 0 && r->dim > regmax)) && mNS <= (MHX_REAL64 ? 50 : 100) &&
                        mala_ring <= MHX_LDS_PER_BLOCK && ((uint64_t)r->dim + 1) * (uint64_t)r->n * sizeof(mhx_real) < (1ull << 32) &&
                        !no_mfma;
    // ... and past that (fp64 d = 201 ... 512, fp32 d = 401 ... 1000): the LEAN form -- one vector per lane, A y and A^T w in place,
    // the noise through the z slab, one tile (or a pair, while the ring holds it) per chunk
    const size_t lean_pair_ring = std::max(mfma_ring_bytes(r->dim, true), ringT);
    const bool lean_pair = lean_pair_ring <= MHX_LDS_PER_BLOCK && mNS <= (MHX_REAL64 ? 80 : 160);
    const size_t lean_ring = lean_pair ? lean_pair_ring : mfma_ring_bytes(r->dim, false);
    const bool mfma_l = !mfma && !mfma_s && t->kind == MHX_TARGET_CORR_GAUSS && !(r->flags & (MHX_FLAG_GENERIC | MHX_FLAG_NO_JIT)) && r->dim >= 16 &&
                        (cfg->reduce_lanes == 4 || (cfg->reduce_lanes == 0 && r->dim > regmax)) && mNS <= (MHX_REAL64 ? 128 : 250) &&
                        lean_ring <= MHX_LDS_PER_BLOCK && ((uint64_t)r->dim + 1) * (uint64_t)r->n * sizeof(mhx_real) < (1ull << 32) &&
                        !no_mfma;
    if (cfg->reduce_lanes > 1 && !mfma && !mfma_s && !mfma_l && (!separable || (r->flags & (MHX_FLAG_GENERIC | MHX_FLAG_NO_JIT))))
        return mhx_fail(MHX_EINVAL, "mhx_mala_create: reduce_lanes > 1 needs a separable catalogue target (iso-Gaussian, banana, funnel) "
                                "or the dense Gaussian target with reduce_lanes = 4 (16 <= dim, both factor images within LDS), and JIT");
    if (mfma_s || mfma_l) {
        // the streamed form and the lean form: one shape on the host -- the step kernel and its ring, the two images
        jit_module* m = nullptr;
        std::vector<std::string> defs = {mfma_s ? "MHX_JIT_MALA_MFMA_STREAM=1" : "MHX_JIT_MALA_MFMA_LEAN=1", "MHX_JIT_DIM=" + std::to_string(r->dim)};
        if (mfma_l) defs.push_back(std::string("MHX_JIT_PAIR=") + (lean_pair ? "1" : "0"));
        rc = jit_compile(ctx, jit_source(t, "mhx_mala_mfma_kernels.h"), defs, &m, {"-mllvm", "-pragma-unroll-threshold=4000000"});
        // 16 chains per wave, the LDS is the ring; kernel(args, tparams, image of A, image of A^T)
        launch_rec k = rec_shape(mfma_s ? "streamed matrix-core MALA kernel" : "lean matrix-core MALA kernel", 64 * MHX_MFMA_WAVES, 16 * MHX_MFMA_WAVES,
                                 mfma_s ? mala_ring : lean_ring, {&r->k_tp, &r->d_mfma_img, &r->d_mfma_img2});
        if (rc == MHX_OK) rc = rec_bind(&k, m, mfma_s ? "mhx_jit_mala_mfma_stream" : "mhx_jit_mala_mfma_lean");
        if (rc == MHX_OK) rc = mala_mfma_images(r.get(), m);
        if (rc == MHX_OK) { r->step = k; r->variant = KF_MFMA; r->coop_L = 4; }
        else if (cfg->reduce_lanes > 1) return rc;
    }
    if (mfma) {
        jit_module* m = nullptr;
        const int NS = (r->dim + 3) / 4;
        const char* wenv = opt(ctx, "MFMA_WAVES");
        const int waves = wenv ? std::max(1, atoi(wenv)) : (MHX_REAL64 ? 1 : (NS <= 16 ? 2 : 1));
        rc = jit_compile(ctx, jit_source(t, "mhx_mala_mfma_kernels.h"),
                         {"MHX_JIT_MALA_MFMA=1", "MHX_JIT_DIM=" + std::to_string(r->dim), "MHX_JIT_WAVES=" + std::to_string(waves)}, &m);
        launch_rec k = rec("matrix-core MALA kernel", 64 * MHX_MFMA_WAVES, 16 * MHX_MFMA_WAVES, mfma_lds);      // both images resident in LDS
        if (rc == MHX_OK) rc = rec_bind(&k, m, "mhx_jit_mala_mfma");
        if (rc == MHX_OK) { r->step = k; r->variant = KF_MFMA; r->coop_L = 4; }
        else if (cfg->reduce_lanes > 1) return rc;
    }
    if (separable && !zig && !(r->flags & (MHX_FLAG_GENERIC | MHX_FLAG_NO_JIT)) && (cfg->reduce_lanes > 1 || (cfg->reduce_lanes == 0 && r->dim > regmax))) {
        const int nblk = (r->dim + 3) / 4;
        const int nbl_auto = MHX_REAL64 ? 3 : 6, nbl_max = MHX_REAL64 ? 4 : 8;       // 5 float4 of state per block and lane
        int L = cfg->reduce_lanes > 1 ? cfg->reduce_lanes : 1;
        if (cfg->reduce_lanes > 1) {
            if (L > 64 || (L & (L - 1))) return mhx_fail(MHX_EINVAL, "mhx_mala_create: reduce_lanes must be a power of two <= 64, got %d", L);
        } else {
            while (L < 64 && (nblk + L - 1) / L > nbl_auto) L *= 2;
            while (L < 64 && 2 * L <= nblk && chains_of_whole_run(ctx, r->n) * L / 64 < 2048) L *= 2;
        }
        const int NBL = (nblk + L - 1) / L;
        if (NBL <= nbl_max) {
            jit_module* m = nullptr;
            const int waves = NBL <= (MHX_REAL64 ? 1 : 3) ? 4 : 2;
            rc = jit_compile(ctx, jit_source(t, "mhx_mala_kernels.h"),
                             {"MHX_JIT_MALA_COOP=1", "MHX_JIT_L=" + std::to_string(L), "MHX_JIT_NBL=" + std::to_string(NBL),
                              "MHX_JIT_TK=" + std::to_string(t->kind), "MHX_JIT_WAVES=" + std::to_string(waves)}, &m);
            launch_rec k = rec("cooperative MALA kernel", 256, 4 * (64 / L), 0);      // whole waves of 64 / L chains
            if (rc == MHX_OK) rc = rec_bind(&k, m, "mhx_jit_mala_coop");
            if (rc == MHX_OK) { r->step = k; r->variant = KF_COOP_JIT; r->coop_L = L; }
            else if (cfg->reduce_lanes > 1) return rc;
        } else if (cfg->reduce_lanes > 1) {
            return mhx_fail(MHX_EINVAL, "mhx_mala_create: reduce_lanes=%d leaves %d blocks per lane (max %d)", L, NBL, nbl_max);
        }
    }
    if (want_reg && r->variant == KF_GENERIC) {
        jit_module* m = nullptr;
        // registers next to the generator's temporaries: 2 D reals of candidate + gradient, 3 XR of state / gradient / noise
        int xr = r->dim;
        if (split) xr = std::max(0, std::min(r->dim, ((MHX_REAL64 ? 200 : 400) - 2 * r->dim) / 3));
        if (const char* xe = opt(ctx, "MALA_XR")) xr = std::max(0, std::min(r->dim, atoi(xe)));          // tuning knob
        std::vector<std::string> defs = {"MHX_JIT_MALA=1", "MHX_JIT_DIM=" + std::to_string(r->dim), "MHX_JIT_TK=" + std::to_string(t->kind),
                                         "MHX_JIT_XR=" + std::to_string(xr)};
        if (zig) defs.push_back("MHX_JIT_GEN=1");
        rc = jit_compile(ctx, jit_source(t, "mhx_mala_kernels.h"), defs, &m, {"-mllvm", "-amdgpu-unroll-threshold-private=100000"});
        // the forms that use LDS -- the split form (the tails of state, gradient and noise) and the ziggurat form (its table) -- run one
        // wave per block, the plain form four
        const size_t lds = zig ? MHX_MALA_ZIG_LDS_BYTES(r->dim, xr) : (xr < r->dim ? (size_t)3 * (r->dim - xr) * 64 * sizeof(mhx_real) : 0);
        if (zig) r->normal_gen = MHX_GEN_ZIGGURAT;
        launch_rec k = lds ? rec("MALA register kernel", 64, 64, lds) : rec("MALA register kernel", 256, 256, 0);
        if (rc == MHX_OK) rc = rec_bind(&k, m, zig ? "mhx_jit_mala_zig" : (xr < r->dim ? "mhx_jit_mala_split" : "mhx_jit_mala"));
        if (rc == MHX_OK && user) rc = jit_function(m, "mhx_jit_mala_init", &r->jit_init);
        if (rc == MHX_OK) { r->step = k; r->variant = KF_REG_JIT; }
        else if (zig) return rc;                                         // (no other kernel of this sampler has the ziggurat)
        else r->jit_init = nullptr;                                      // the run-time-dimension kernel computes the same chain
    }
    if (user && r->variant == KF_GENERIC) {
        // the user source must also define MHX_LOGDENSITY_AND_GRADIENT (the reference's
        // check_capabilities, src/MALA.jl:42-52, throws when no gradient is available)
        jit_module* m = nullptr;
        rc = jit_compile(ctx, jit_source(t, "mhx_mala_kernels.h"),
                         {"MHX_JIT_MALA=1", "MHX_JIT_TK=" + std::to_string(t->kind)}, &m);
        if (rc) return rc;
        r->step = rec("MALA state-in-HBM kernel", 256, 256, 0);
        if ((rc = rec_bind(&r->step, m, "mhx_jit_mala"))) return rc;
        if ((rc = jit_function(m, "mhx_jit_mala_init", &r->jit_init))) return rc;
    } else if (r->variant == KF_GENERIC) {
        r->step = rec("MALA state-in-HBM kernel", 256, 256, 0);
        if ((rc = rec_bind(&r->step, (const void*)k_mala))) return rc;
    }
    *out = r.release();
    return MHX_OK;
}

static int mala_eval_state(mhx_run* r, int reset_counts)
{
    mhx_ctx* ctx = r->ctx;
    mhx_mala_args a = mala_args(r);
    const mhx_real* tp = r->target->dparams;
    const unsigned grid = (unsigned)((r->n + 255) / 256);
    if (r->jit_init) {
        int rc = launch_module(r->jit_init, grid, 256, ctx->stream, a, tp, reset_counts);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(k_mala_init, dim3(grid), dim3(256), 0, ctx->stream, a, tp, reset_counts);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MHX_OK;
}

static int mala_init(mhx_run* r, const mhx_real* init)
{
    if (!init) return mhx_fail(MHX_EINVAL, "please specify initial parameters");      // src/MALA.jl:37
    const size_t nx = (size_t)r->dim * (size_t)r->n;
    HIP_TRY(hipMemcpyAsync(r->d_x, init, nx * sizeof(mhx_real), hipMemcpyHostToDevice, r->ctx->stream));
    return mala_eval_state(r, 1);
}

static int mala_advance(mhx_run* r, uint64_t nsteps, uint32_t save_next, int save_slot, int thinning)
{
    mhx_ctx* ctx = r->ctx;
    uint64_t done = 0;
    while (done < nsteps) {
        const uint64_t chunk = std::min<uint64_t>(nsteps - done, MHX_MAX_STEPS_PER_LAUNCH);
        mhx_mala_args a = mala_args(r);
        a.step0 = (uint32_t)(r->tau + 1);
        a.nsteps = (int)chunk;
        a.save_next = save_next;
        a.save_slot = save_slot;
        a.thinning = thinning;
        int rc = launch(r->step, ctx->stream, r->n, 1, &a);
        if (rc) return rc;
        HIP_TRY(hipGetLastError());
        r->stats.launches++;
        save_cursor_skip(r, chunk, thinning, &save_next, &save_slot);
        r->tau += chunk;
        done += chunk;
    }
    return MHX_OK;
}
