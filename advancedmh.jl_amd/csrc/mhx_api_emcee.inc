// emcee host side (included by mhx_api.hip): Ensemble{StretchProposal}, src/emcee.jl:1-102

#ifndef MHX_EMCEE_FUSED_DEFAULT
#define MHX_EMCEE_FUSED_DEFAULT 1        // the stretch move as one launch per sweep where the kernel has that form (MHX_EMCEE_FUSED=0: two half-step launches)
#endif
// ... for ensembles up to this size: the sweep launch trades a kernel boundary (2.7 us) for half as many row products again, which
// pays while a half-step is a chain of latencies and stops paying when the launch fills the machine (d = 50, moves/s one launch
// against two -- banded factor, fp64: 8 192 walkers +36 %, 16 384 +28 %, 24 576 +4 %, 32 768 -17 %; dense factor, fp64: 8 192
// +57 %, 16 384 +-0, 24 576 +13 %, 32 768 -10 %; fp32 crosses over a size later: profiles/r04u_fused_sizes.log)
#ifndef MHX_EMCEE_FUSED_MAX_W
#define MHX_EMCEE_FUSED_MAX_W 24576
#endif
#ifndef MHX_EMCEE_PRELOAD_DEFAULT
#define MHX_EMCEE_PRELOAD_DEFAULT 0      // kernarg preload of the half-step kernel (see mhx_jit_emcee_half)
#endif
__global__ void __launch_bounds__(64)
k_emcee_half(const mhx_emcee_args a, const mhx_real* __restrict__ tparams)
{
    mhx_emcee_half_body<0, MHX_TARGET_DYNAMIC>(mhx_emcee_pick(a), tparams);
}
__global__ void __launch_bounds__(256)
k_emcee_init(const mhx_emcee_args a, const mhx_real* __restrict__ tparams, const int draw)
{
    mhx_emcee_init_body<MHX_TARGET_DYNAMIC>(mhx_emcee_pick(a), tparams, draw);
}
__global__ void __launch_bounds__(64)
k_emcee_seq(const mhx_emcee_args a, const mhx_real* __restrict__ tparams)
{
    mhx_emcee_seq_body<MHX_TARGET_DYNAMIC>(mhx_emcee_pick(a), tparams);
}

#define MHX_EMCEE_REG_MAX_DIM 160     // the candidate of a walker in ONE lane's registers (the walkers themselves are rows in memory): fp64 320 of the
                                      // 512 VGPRs a one-wave block may use.  Was 32 in fp64 until round 4 -- a d = 50 user log-density in the
                                      // reference's precision ran the state-in-HBM kernel at 41 us per half-step -- then 64, then this
#define MHX_EMCEE_REG_SWEEP_MAX_DIM (MHX_REAL64 ? 64 : 128)   // the sweep launch keeps two candidates in registers

// [dim][W] (ABI) <-> [W][pitch] (walker-major, zero padded), one thread per element of the padded copy
__global__ void __launch_bounds__(256)
k_emcee_transpose(mhx_real* __restrict__ x, mhx_real* __restrict__ xw, const int d, const int pitch, const long W, const int to_abi)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= W * pitch) return;
    const long w = e / pitch;
    const int k = (int)(e - w * pitch);
    if (to_abi) { if (k < d) x[(long)k * W + w] = xw[e]; }
    else xw[e] = k < d ? x[(long)k * W + w] : MHX_R(0.0);
}
// the cooperative kernel's state lives in the walker-major copy: refresh it from / write it back to the ABI layout
static int emcee_sync_state(mhx_run* r, int to_abi)
{
    if (!r->d_xw) return MHX_OK;
    const int pitch = mhx_xw_pitch(r->dim);
    const long total = (long)r->n * pitch;
    hipLaunchKernelGGL(k_emcee_transpose, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, r->ctx->stream,
                       r->d_x, r->d_xw, r->dim, pitch, (long)r->n, to_abi);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    return MHX_OK;
}

static mhx_emcee_args emcee_args(const mhx_run* r)
{
    mhx_emcee_args a;
    memset(&a, 0, sizeof a);
    a.x = r->d_x; a.xw = r->d_xw; a.lp = r->d_lp; a.acc_count = r->d_acc; a.acc_total = r->d_acc_total;
    a.xw_out = r->d_xw2; a.lp_out = r->d_lp2;
    a.samples = r->d_samples; a.accepted = r->d_accepted; a.last_acc = r->d_last; a.ybuf = r->d_ybuf;
    a.seed = r->seed; a.ensemble_id = r->first_id;
    a.nwalkers = r->ens_w; a.dim = r->dim;
    a.ld = r->n;                                          // E ensembles side by side: columns of [..][E W] arrays
    a.ybuf_ens = r->variant == KF_EMCEE_SEQ ? r->dim : r->ens_w;
    a.target_kind = r->target->kind; a.ntparams = r->target->nparams; a.tconst = r->target->cst;
    a.stretch = r->stretch;
    a.save_slot = -1;
    a.rec_other_slot = -1;
    a.reduce_lanes = r->coop_L;
    a.t_begin = 0; a.t_count = r->ens_w;                 // the whole moving half
    a.init_kind = r->prop_kind; a.init_scale = r->prop_scale; a.init_vec = r->d_pvec; a.init_mean = r->d_pmean;
    a.nsweeps = 0; a.save_next = MHX_NO_SAVE; a.thinning = 1;
    return a;
}

#ifndef MHX_EMCEE_MFMA_DEFAULT
#define MHX_EMCEE_MFMA_DEFAULT 1
#endif
// the matrix-core form of the stretch move: the operand image of the packed factor (the layout of mhx_mfma_image_fill, built on
// the host -- d <= 128 -- and kept in global memory for the run), the half-step and the sweep kernel
static int emcee_create_mfma(mhx_run* r, const mhx_target* t, const int d)
{
    mhx_ctx* ctx = r->ctx;
    const int NS = (d + 3) / 4, NT = (d + 15) / 16;
    auto steps = [&](int tt) { return std::min(4 * (tt + 1), NS); };
    auto groups = [&](int tt) { return (steps(tt) + 3) / 4; };
    auto first = [&](int tt) { return 2 * tt * (tt + 1); };
    const int total = first(NT - 1) + 4 * groups(NT - 1);
    std::vector<mhx_real> A((size_t)d * (d + 1) / 2), img((size_t)total * 64, MHX_R(0.0));
    HIP_TRY(hipMemcpy(A.data(), t->dparams, A.size() * sizeof(mhx_real), hipMemcpyDeviceToHost));
    for (int tt = 0; tt < NT; ++tt)
        for (int sg = 0; sg < 4 * groups(tt); ++sg)
            for (int ln = 0; ln < 64; ++ln) {
                const int m = ln & 15;
                const int i = MHX_REAL64 ? 16 * tt + m : 16 * tt + 4 * (m & 3) + (m >> 2);      // mhx_mfma_row
                const int k = 4 * sg + (ln >> 4);
                const bool in = i < d && k <= i && sg < steps(tt);
                img[(size_t)(first(tt) + (sg & ~3)) * 64 + (size_t)ln * 4 + (sg & 3)] = in ? A[(size_t)i * (i + 1) / 2 + k] : MHX_R(0.0);
            }
    HIP_TRY(hipMalloc(&r->d_mfma_img, img.size() * sizeof(mhx_real)));
    HIP_TRY(hipMemcpy(r->d_mfma_img, img.data(), img.size() * sizeof(mhx_real), hipMemcpyHostToDevice));
    jit_module* m = nullptr;
    const char* wv = opt(r->ctx, "EMCEE_MFMA_WAVES");                      // tuning knob
    r->coop_waves = wv ? std::max(1, std::min(8, atoi(wv))) : 1;
    std::vector<std::string> defs = {"MHX_JIT_EMCEE_MFMA=1", "MHX_JIT_DIM=" + std::to_string(d), "MHX_EMCEE_MFMA_WAVES=" + std::to_string(r->coop_waves)};
    if (const char* rs = opt(r->ctx, "EMCEE_REC_STORE")) defs.push_back(std::string("MHX_EMCEE_REC_STORE=") + rs);
    int rc = jit_compile(ctx, "#include \"mhx_emcee_mfma_kernels.h\"\n", defs, &m);
    // kernel(args, image) for the half step and the sweep: 16 walkers per wave.  More than one wave per block: the waves share ONE
    // fetch of the operand image through LDS (mhx_emcee_mfma_kernels.h)
    launch_rec half = rec_shape("matrix-core stretch move", 64 * r->coop_waves, 16 * r->coop_waves, r->coop_waves > 1 ? img.size() * sizeof(mhx_real) : 0,
                                {&r->d_mfma_img});
    launch_rec sweep = half;
    if (rc == MHX_OK) rc = rec_bind(&half, m, "mhx_jit_emcee_mfma_half");
    if (rc) { (void)hipFree(r->d_mfma_img); r->d_mfma_img = nullptr; return rc; }
    r->step = half;
    // (this form's sweep kernel pays up to 20 480 walkers at d = 50: 16 384 1.18 -> 1.48e9 moves/s, 20 480 1.31 -> 1.48e9, 24 576 1.53 ->
    // 1.48e9; further out for smaller dimensions -- d = 24: +16 % at 49 152, d = 10: +13 % at 65 536; d = 64: +11 % at 16 384, -9 % at 24 576)
    if (opt_int(ctx, "EMCEE_FUSED", MHX_EMCEE_FUSED_DEFAULT != 0 && (long)r->n <= std::max(16384L, std::min(61440L, 21000L * 50 / std::max(d, 16)))) != 0)
        if (hipFunction_t f = nullptr; jit_function(m, "mhx_jit_emcee_mfma_sweep", &f) == MHX_OK) {      // (a missing sweep kernel is done without)
            if ((rc = rec_bind(&sweep, m, "mhx_jit_emcee_mfma_sweep"))) return rc;
            r->sweep = sweep;
        }
    r->emcee_band = -1;
    r->variant = KF_EMCEE_MFMA;
    r->coop_L = 4;
    return MHX_OK;
}

int api_emcee_create(mhx_ctx* ctx, const mhx_target* t, const mhx_emcee_cfg* cfg, mhx_run** out)
{
    if (!ctx || !t || !cfg || !out) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: NULL argument");
    if (cfg->dim != t->dim) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: dim %d != model dim %d", cfg->dim, t->dim);
    if (cfg->nwalkers < 2) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: an ensemble needs at least 2 walkers");
    if (!(cfg->stretch > 1.0)) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: stretch length must be > 1");
    // the Philox counter of a walker is (walker, ensemble_id, sweep, stream | block): ONE 32-bit word for the ensemble id
    // (spec 3.1: id = ensemble << 32 | walker) -- ids that differ by a multiple of 2^32 would share their streams
    if (cfg->ensemble_id >> 32) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: ensemble_id must be < 2^32 (it is one word of the RNG counter)");
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<mhx_run> r(new mhx_run);
    r->dtype = ctx->dtype;
    r->ctx = ctx; r->target = t; r->kind = RUN_EMCEE;
    // E independent ensembles in one run (README.md:135-148: `sample(model, Ensemble(...), MCMCThreads(), N, nchains)`): ids
    // ensemble_id .. ensemble_id + E - 1, every launch gets E as its second grid dimension
    const int E = cfg->n_ensembles > 1 ? cfg->n_ensembles : 1;
    if (cfg->n_ensembles < 0 || E > 65535) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: n_ensembles must be in [0, 65535]");
    if ((cfg->ensemble_id + (uint64_t)E - 1) >> 32) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: ensemble ids must stay below 2^32");
    if ((long)cfg->nwalkers * E > 0x7fffffffL) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: %d ensembles of %d walkers exceed 2^31 - 1 walkers", E, cfg->nwalkers);
    r->dim = cfg->dim; r->ens_w = cfg->nwalkers; r->n_ens = E; r->seed = cfg->seed; r->first_id = cfg->ensemble_id;
    r->n = cfg->nwalkers * E;                            // what every buffer is sized by
    r->flags = cfg->flags; r->stretch = (mhx_real)cfg->stretch;
    int rc = run_alloc_state(r.get());
    if (rc) return rc;
    const size_t NT = (size_t)r->n;
    r->n = cfg->nwalkers;                                // ... while the kernel form is chosen for ONE ensemble's shape (restored at the exits)
    auto done = [&]() { r->n = (int)NT; *out = r.release(); return (int)MHX_OK; };
    // a launch record of this sampler: kernel(args, tparams); every launch gets E as its second grid dimension
    auto rec = [&](const char* what, unsigned block, int per_block, size_t lds) { return rec_shape(what, block, per_block, lds, {&r->k_tp}); };
    // the prior of the initial walkers (src/emcee.jl:29-34), kept on the device like a proposal
    r->prop_kind = -1;
    if (cfg->init_kind >= 0) {
        const size_t dd = (size_t)cfg->dim;
        size_t nvec = 0;
        if (cfg->init_kind == MHX_PROP_ISO) { if (!(cfg->init_scale > 0.0)) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: init_scale must be positive"); }
        else if (cfg->init_kind == MHX_PROP_DIAG) nvec = dd;
        else if (cfg->init_kind == MHX_PROP_DENSE) nvec = dd * (dd + 1) / 2;
        else return mhx_fail(MHX_EINVAL, "mhx_emcee_create: unknown init_kind %d", cfg->init_kind);
        if (nvec && !cfg->init_vec) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: init_vec is NULL");
        r->prop_kind = cfg->init_kind;
        r->prop_scale = (mhx_real)cfg->init_scale;
        HIP_TRY(hipMalloc(&r->d_pvec, (nvec ? nvec : 1) * sizeof(mhx_real)));
        if (nvec) COPY_SYNC(ctx->stream, r->d_pvec, cfg->init_vec, nvec * sizeof(mhx_real), hipMemcpyHostToDevice);
        if (cfg->init_mean) {
            HIP_TRY(hipMalloc(&r->d_pmean, dd * sizeof(mhx_real)));
            COPY_SYNC(ctx->stream, r->d_pmean, cfg->init_mean, dd * sizeof(mhx_real), hipMemcpyHostToDevice);
        }
    }
    const bool sequential = (cfg->flags & MHX_FLAG_EMCEE_SEQUENTIAL) != 0;
    if (sequential) {
        // the reference's Gauss-Seidel sweep: one wavefront, run-time dimension, state in the ABI layout
        if (cfg->reduce_lanes > 1) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: the sequential sweep runs on one lane group (reduce_lanes must be 0 or 1)");
        r->variant = KF_EMCEE_SEQ;
        r->coop_L = 1;
        r->step = rec("sequential stretch move", 64, 1, 0);        // one wave per ensemble, launched for ONE item
        if (t->kind == MHX_TARGET_USER) {
            jit_module* m = nullptr;
            rc = jit_compile(ctx, jit_source(t, "mhx_emcee_kernels.h"),
                             {"MHX_JIT_EMCEE=1", "MHX_JIT_DIM=0", "MHX_JIT_TK=" + std::to_string(t->kind), "MHX_JIT_L=1"}, &m);
            if (rc == MHX_OK) rc = rec_bind(&r->step, m, "mhx_jit_emcee_seq");
            if (rc == MHX_OK) rc = jit_function(m, "mhx_jit_emcee_init", &r->jit_init);
            if (rc) return rc;
        } else if ((rc = rec_bind(&r->step, (const void*)k_emcee_seq))) return rc;
        HIP_TRY(hipMalloc(&r->d_ybuf, (size_t)cfg->dim * (size_t)E * sizeof(mhx_real)));
        return done();
    }
    const int tk = t->kind, d = r->dim;
    const bool user = tk == MHX_TARGET_USER;
    const bool want_reg = !(r->flags & MHX_FLAG_GENERIC) && d <= MHX_EMCEE_REG_MAX_DIM &&
                          !(tk == MHX_TARGET_IID_NORMAL && t->nparams > 4096);
    r->variant = KF_GENERIC;
    // lanes per walker: the cooperative kernel exists for the dense-Gaussian target with a compile-time dimension
    int L = 1;
    const bool can_coop = tk == MHX_TARGET_CORR_GAUSS && !(r->flags & (MHX_FLAG_GENERIC | MHX_FLAG_NO_JIT)) && d >= 2 && d <= MHX_DENSE_COOP_MAX_DIM;
    if (cfg->reduce_lanes > 1) {
        if (!can_coop) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: reduce_lanes > 1 needs the CORR_GAUSS target, dim <= 256 and JIT");
        L = cfg->reduce_lanes;
        if (L > 64 || (L & (L - 1)) || L > d) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: reduce_lanes must be a power of two <= min(64, dim)");
    } else if (cfg->reduce_lanes == 0 && can_coop && d >= 8) {
        // enough waves for two per SIMD in a half-step, at most 16 lanes per walker (measured on C3:
        // 4 / 8 / 16 / 32 lanes -> 6.9e8 / 9.1e8 / 9.8e8 / 7.8e8 moves/s)
        L = 2;
        while (L < 16 && 2 * L <= d && (long)(r->n / 2) * L / 64 < 2048) L *= 2;
        if (L < dense_coop_lanes(d)) L = dense_coop_lanes(d);          // at most 12.5 rows of A y per lane
    }
    // A DENSE factor (no band to exploit) runs the scalar-factor form (mhx_emcee_scal_body): a lane owns a walker during the
    // mat-vec, so the factor entry is wave-uniform -- the DPP-broadcast operand of v_fmac (mode 1: each wave's rows in VGPRs) or an
    // SGPR pair streamed through the scalar cache (mode 0) -- no LDS image, no fill.  Its reduction shape is the number of waves
    // per block (row classes).  By default where the engine picks the lanes (reduce_lanes == 0) and the candidate plus the wave's
    // factor pieces fit the registers (2 waves per SIMD at 8 waves per block: 256 VGPRs); MHX_EMCEE_SCALAR=0 keeps the lane-group
    // form, =NW (4, 8, 16) forces the scalar form with NW waves wherever a cooperative kernel would run (tuning / tests).
    const int band_bw = (tk == MHX_TARGET_CORR_GAUSS && !(r->flags & MHX_FLAG_DENSE_FACTOR) && t->bandwidth >= 0 &&
                         t->bandwidth <= MHX_EMCEE_MAX_BAND && t->bandwidth < d - 1) ? t->bandwidth : -1;
    // ... or, while its operands fit a lane's registers, the matrix-core form (mhx_emcee_mfma_kernels.h, KF_EMCEE_MFMA): 4 lanes per
    // walker, the candidate formed in the MFMA's B-operand layout, every lane's A operands fetched once per launch from an image
    // built here, once per run -- no LDS, no barrier.  Reduction shape 4.  MHX_EMCEE_MFMA=0 keeps the scalar-factor form (tuning).
    {
        // by default in fp64 from 12 288 walkers on: one wave carries the whole product of its 16 walkers (37 MFMAs of 66 cycles at
        // d = 50), which is the shorter chain only once the scalar-factor form's 8-cycle DPP products queue up behind each other
        // (rotated C3, moves/s against the scalar-factor form -- fp64: 4 096 walkers -6 %, 8 192 -14 %, 12 288 +24 %, 16 384 +16 %,
        // 32 768 +20 %, 65 536 +25 %, 262 144 +23 %; fp32, whose DPP product issues in 4 cycles: -5 ... -25 %: profiles/r04w_mfma_sizes.log)
        // Smaller dimensions: the chain is a few MFMAs and this form has no barrier -- d <= 32 in fp64 +10 ... +45 % at every size from
        // 2 048 to 16 384 walkers, d = 40 +-0 ... +6 %; fp32 d = 10 +5 ... +14 %, d = 24 +-0, d = 32 +5 / -8 % (tools/emcee_mfma_dims.sh)
        const bool want = opt_int(ctx, "EMCEE_MFMA", MHX_EMCEE_MFMA_DEFAULT != 0 && (MHX_REAL64 ? (d <= 40 || r->n >= 12288) : d <= 16)) != 0;
        if (want && can_coop && band_bw < 0 && d >= 8 && d <= (MHX_REAL64 ? 64 : 128) && (cfg->reduce_lanes == 0 || cfg->reduce_lanes == 4) &&
            !opt(ctx, "EMCEE_SCALAR")) {
            int rcm = emcee_create_mfma(r.get(), t, d);
            if (rcm == MHX_OK) {
                HIP_TRY(hipMalloc(&r->d_xw, NT * (size_t)mhx_xw_pitch(d) * sizeof(mhx_real)));
                if (r->sweep) {
                    HIP_TRY(hipMalloc(&r->d_xw2, NT * (size_t)mhx_xw_pitch(d) * sizeof(mhx_real)));
                    HIP_TRY(hipMalloc(&r->d_lp2, NT * sizeof(mhx_real)));
                }
                return done();
            } else if (cfg->reduce_lanes == 4 && opt(ctx, "EMCEE_MFMA")) return rcm;
        }
    }
    bool scal = false;
    int scal_mode = 1;
    {
        const int forced = opt_int(ctx, "EMCEE_SCALAR", -1);
        const int xp = (d + 3) & ~3, b4 = (int)(sizeof(mhx_real) / 4);
        // registers of a lane in phase 2: the walker's candidate, plus (broadcast form) this wave's pieces of the factor
        auto pieces = [&](int nw) { int p = 0; for (int m = 0; nw * m < d; ++m) p += (std::min(nw * m + nw - 1, d - 1)) / 16 + 1; return p; };
        auto fits = [&](int nw, int mode) { return b4 * (xp + (mode ? pieces(nw) + (d + nw - 1) / nw : 0)) + 56 <= (mode ? 250 : 200); };
        if (can_coop && L > 1 && band_bw < 0 && d >= 8 && forced != 0) {
            int nw = 0;
            if (forced == 4 || forced == 8 || forced == 16) nw = forced;
            else if (cfg->reduce_lanes == 0) nw = 8;
            else if (forced > 0 && (cfg->reduce_lanes == 4 || cfg->reduce_lanes == 8 || cfg->reduce_lanes == 16)) nw = cfg->reduce_lanes;
            if (nw && nw <= d) {
                scal_mode = opt_int(ctx, "EMCEE_SCAL_MODE", fits(nw, 1)) ? 1 : 0;       // tuning knob
                if (fits(nw, scal_mode) || forced > 0) { scal = true; L = nw; }
            }
        }
    }
    if (user || L > 1 || (want_reg && !(r->flags & MHX_FLAG_NO_JIT))) {
        const int jd = (L > 1 || (want_reg && !(r->flags & MHX_FLAG_NO_JIT))) ? d : 0;
        jit_module* m = nullptr;
        // a banded precision factor (exact zeros below the band): the cooperative kernel's band form -- no factor image in LDS,
        // no block barrier, BW + 1 products per row.  MHX_FLAG_DENSE_FACTOR keeps the dense form.
        const int bw = L > 1 ? band_bw : -1;
        r->emcee_band = bw;
        std::vector<std::string> defs = {"MHX_JIT_EMCEE=1", "MHX_JIT_DIM=" + std::to_string(jd), "MHX_JIT_TK=" + std::to_string(tk),
                                         "MHX_JIT_L=" + std::to_string(L)};
        if (const char* rs = opt(ctx, "EMCEE_REC_STORE")) defs.push_back(std::string("MHX_EMCEE_REC_STORE=") + rs);   // tuning knob
        if (const char* rs = opt(ctx, "EMCEE_ROW_STORE")) defs.push_back(std::string("MHX_EMCEE_ROW_STORE=") + rs);   // tuning knob
#ifdef MHX_TOOLS_BUILD
        // timing probe (tools/emcee_probe.sh): MHX_EMCEE_PROBE=n ends the cooperative half-step after its n-th phase -- wrong
        // chains, right latencies
        if (const char* probe = opt(ctx, "EMCEE_PROBE")) {
            defs.push_back(std::string("MHX_EMCEE_PROBE=") + probe);
            fprintf(stderr, "mhx (tools build): EMCEE_PROBE=%s -- timing probe: the half-step ends early, this run's chains are NOT valid (stats.tainted = 1)\n", probe);
        }
#endif
        if (scal) {
            defs.push_back("MHX_JIT_SCAL=1");
            // walkers per block: 64 fill the lanes of phase 2 (the throughput shape: large ensembles), 32 spread a latency-bound
            // half-step over twice the CUs (C3: 8192 moving walkers = 256 blocks, one per CU; 6.4 against 7.4 us in fp64)
            r->emcee_wpb = opt_int(ctx, "EMCEE_SCAL_WPB", (r->n / 2 + 63) / 64 >= 512 ? 64 : 32);      // tuning knob: 64, 32, 16
            if (r->emcee_wpb != 16 && r->emcee_wpb != 32) r->emcee_wpb = 64;
            defs.push_back("MHX_EMCEE_SCAL_WPB=" + std::to_string(r->emcee_wpb));
#ifdef MHX_TOOLS_BUILD
            if (opt(ctx, "EMCEE_STAMPS")) {                                       // timing stamps (tools/c3_stamps.py)
                defs.push_back("MHX_EMCEE_STAMPS=1");
                const size_t nwv = ((size_t)(r->n / 2 + 1) / (size_t)r->emcee_wpb + 2) * (size_t)L;
                HIP_TRY(hipMalloc(&r->d_ybuf, nwv * 16 * sizeof(uint64_t)));
                HIP_TRY(hipMemset(r->d_ybuf, 0, nwv * 16 * sizeof(uint64_t)));
                r->emcee_stamp_words = nwv * 16;
            }
#endif
            defs.push_back(std::string("MHX_EMCEE_SCAL_MODE=") + (scal_mode ? "1" : "0"));
            if (const char* rc_ = opt(ctx, "EMCEE_SCAL_REC")) defs.push_back(std::string("MHX_EMCEE_SCAL_REC=") + (atoi(rc_) ? "1" : "0"));   // tuning knob
            r->coop_waves = L;
        } else if (L > 1) {
            // waves per block of the cooperative kernel: they share one LDS copy of the factor image, and every block fetches
            // the same image lines at the same moment -- 8 waves measured best on C3 (2 / 4 / 8 / 16 waves: 9.0 / 7.8 / 7.5 /
            // 10.3 us per half-step in fp64, 7.7 / 5.8 / 5.5 / 6.6 in fp32); MHX_EMCEE_WAVES overrides (tuning knob)
            const char* wv = opt(ctx, "EMCEE_WAVES");
            r->coop_waves = wv ? std::max(1, std::min(16, atoi(wv))) : 8;
            if (!wv && dense_coop_lds_bytes(d, L, 1, 8) > MHX_LDS_PER_BLOCK) r->coop_waves = MHX_EMCEE_COOP_WAVES;   // large images: 4 waves
            defs.push_back("MHX_EMCEE_COOP_WAVES=" + std::to_string(r->coop_waves));
            defs.push_back("MHX_JIT_BW=" + std::to_string(bw));
            if (const char* cr = opt(ctx, "EMCEE_COOP_REC")) defs.push_back(std::string("MHX_EMCEE_COOP_REC=") + (atoi(cr) ? "1" : "0"));   // tuning knob
        }
        // a small ensemble (<= 1024 walkers) on the lane-per-walker kernel: also its persistent one-block form (see below); the block's
        // thread count is a compile-time launch bound (the registers of a lane: 512 / waves per SIMD)
        int persist_threads = 0;
        {
            const int threads = ((r->n + 63) / 64) * 64;
            const int regs = (int)(sizeof(mhx_real) / 4) * 2 * ((jd + 3) & ~3) + 48;         // walker + candidate + the rest, per lane
            const size_t lds = (size_t)r->n * (size_t)(((jd + 3) & ~3) + 1) * sizeof(mhx_real);
            if (!scal && L == 1 && jd > 0 && r->n <= 1024 && opt_int(ctx, "EMCEE_PERSIST", 1) != 0 && lds <= MHX_LDS_PER_BLOCK &&
                regs <= 512 / ((threads / 64 + 3) / 4)) {
                persist_threads = threads;
                defs.push_back("MHX_JIT_PERSIST_THREADS=" + std::to_string(threads));
            }
        }
        // kernarg preload of the half-step's hot arguments (mhx_jit_emcee_half, MHX_JIT_PRELOAD); MHX_EMCEE_PRELOAD=0|1 tuning knob
        r->emcee_preload = opt_int(ctx, "EMCEE_PRELOAD", MHX_EMCEE_PRELOAD_DEFAULT) != 0;
        std::vector<std::string> xopts;
        if (L == 1) xopts = {"-mllvm", "-amdgpu-unroll-threshold-private=100000"};   // a user's loop over the candidate unrolls whatever it costs (see rwmh_create)
        if (r->emcee_preload) {
            defs.push_back("MHX_JIT_PRELOAD=1");
            xopts.push_back("-mllvm"); xopts.push_back("-amdgpu-kernarg-preload-count=9");
        }
        rc = jit_compile(ctx, jit_source(t, "mhx_emcee_kernels.h"), defs, &m, xopts);
        if (rc == MHX_OK) rc = jit_function(m, "mhx_jit_emcee_init", &r->jit_init);
        const int xp = (d + 3) & ~3, u = 16 / (int)sizeof(mhx_real), ys = ((xp / u) | 1) * u;      // mhx_emcee_sgeom::YS
        // The half step.  Scalar-factor form: wpb walkers per block of L waves, their candidates and a row class per wave in LDS;
        // lane-group form: 64 / L walkers per wave, coop_waves waves, candidate rows and the factor image in LDS; a lane per walker:
        // one wave per block, no LDS.  The sweep kernel runs the same blocks (the scalar-factor form: wpb / 2 walkers of EACH half)
        launch_rec half = scal    ? rec("scalar-factor stretch move", 64 * r->coop_waves, r->emcee_wpb, (size_t)(r->emcee_wpb * ys + L * 64) * sizeof(mhx_real))
                          : L > 1 ? rec("cooperative stretch move", 64 * r->coop_waves, (64 / L) * r->coop_waves, dense_coop_lds_bytes(d, L, 1, r->coop_waves))
                                  : rec("stretch move", 64, 64, 0);
        launch_rec sweep = half, persist;
        sweep.what = "stretch move sweep";
        if (scal) sweep.per_block = r->emcee_wpb / 2;
        if (rc == MHX_OK && !scal && L > 1 && half.lds > MHX_LDS_PER_BLOCK)
            rc = mhx_fail(MHX_EINVAL, "emcee: the factor image of dim %d with %d lanes per walker exceeds the LDS", d, L);
        if (rc == MHX_OK) rc = rec_bind(&half, m, "mhx_jit_emcee_half");
        // one launch per sweep (mhx_emcee_coop_sweep_body): the lane-group form with three candidate rows per walker in LDS.  By
        // default for a banded factor only: with the dense image the second half's three full row products cost more than the
        // launch they save (rotated C3: 16.2 us per sweep against 2 x 7.1); MHX_EMCEE_FUSED=0|1 forces it off / on (tuning knob)
        const bool fused_size = MHX_EMCEE_FUSED_DEFAULT != 0 && r->n <= MHX_EMCEE_FUSED_MAX_W;
        // (the lane-group form's launch fills the machine later the smaller the dimension: one launch against two at d = 10 / 24 is
        // +25 % / +28 % at 32 768 walkers, +18 % / +13 % at 49 152, -1 % / -7 % at 65 536 -- profiles/r04u_fused_sizes.log)
        const bool fused_size_band = MHX_EMCEE_FUSED_DEFAULT != 0 && (long)r->n <= std::min(61440L, (long)MHX_EMCEE_FUSED_MAX_W * 50 / std::max(d, 20));
        // (a sweep kernel that is missing, or refused its LDS, is done without: the half-step launches stay)
        auto try_sweep = [&](size_t lds) {
            sweep.lds = lds;
            if (lds > MHX_LDS_PER_BLOCK || rec_bind(&sweep, m, "mhx_jit_emcee_sweep") != MHX_OK) sweep.mod_fn = nullptr;
        };
        if (rc == MHX_OK && !scal && L > 1 && opt_int(ctx, "EMCEE_FUSED", fused_size_band && bw >= 0) != 0) {
            const size_t rows = (size_t)r->coop_waves * (64 / L) * (size_t)(((d + 3) & ~3) + 4) * sizeof(mhx_real);
            try_sweep(half.lds + 2 * rows);
        }
        // ... and the scalar-factor form (mhx_emcee_scal_sweep_body; DPP operand mode, the latency shape of <= 32 walkers per block)
        if (rc == MHX_OK && scal && scal_mode == 1 && r->emcee_wpb == 32 && L >= 2 && opt_int(ctx, "EMCEE_FUSED", fused_size) != 0)
            try_sweep((size_t)(2 * r->emcee_wpb * ys + L * 64 + 2 * r->emcee_wpb) * sizeof(mhx_real));
        // ... and the lane-per-walker register kernel (any target: the second half evaluates the log-density twice)
        if (rc == MHX_OK && !scal && L == 1 && jd > 0 && jd <= MHX_EMCEE_REG_SWEEP_MAX_DIM && opt_int(ctx, "EMCEE_FUSED", fused_size) != 0)
            try_sweep(0);
        // ... and, for an ensemble of at most 1024 walkers whose rows fit the LDS of one block, the whole call in ONE launch of one
        // persistent block (mhx_emcee_persist_body, KF_EMCEE_PERSIST); MHX_EMCEE_PERSIST=0 keeps the sweep launches (tuning knob).  The 64 KB
        // of registers a 1024-thread block leaves each lane hold the walker and its candidate up to d = 24 in fp64 (48 in fp32)
        // (one block of whole waves per ensemble, launched for ONE item; every walker's row in LDS)
        persist = rec("persistent-block ensemble", (unsigned)persist_threads, 1, (size_t)r->n * (size_t)(((jd + 3) & ~3) + 1) * sizeof(mhx_real));
        if (!(rc == MHX_OK && persist_threads > 0 && rec_bind(&persist, m, "mhx_jit_emcee_persist") == MHX_OK))
            persist.mod_fn = nullptr;
        if (rc == MHX_OK) {
            r->step = half; r->sweep = sweep; r->persist = persist; r->sweep_mixed = scal;
            r->variant = scal ? KF_EMCEE_SCAL : (L > 1 ? KF_COOP_JIT : (jd > 0 ? (persist ? KF_EMCEE_PERSIST : KF_REG_JIT) : KF_GENERIC));
            r->coop_L = L;
        } else if (user || cfg->reduce_lanes > 1) {
            return rc;
        } else {
            r->jit_init = nullptr; r->coop_L = 1;
        }
    }
    if (!r->step) {                      // the pre-built half step: run-time dimension, a lane per walker
        r->step = rec("stretch move", 64, 64, 0);
        if ((rc = rec_bind(&r->step, (const void*)k_emcee_half))) return rc;
    }
    if (r->variant == KF_GENERIC) HIP_TRY(hipMalloc(&r->d_ybuf, (size_t)d * NT * sizeof(mhx_real)));
    // the compile-time-dimension kernels (cooperative, register) keep the walkers walker-major
    if (r->variant == KF_COOP_JIT || r->variant == KF_REG_JIT || r->variant == KF_EMCEE_SCAL || r->variant == KF_EMCEE_PERSIST) HIP_TRY(hipMalloc(&r->d_xw, NT * (size_t)mhx_xw_pitch(d) * sizeof(mhx_real)));
    if (r->sweep) {
        HIP_TRY(hipMalloc(&r->d_xw2, NT * (size_t)mhx_xw_pitch(d) * sizeof(mhx_real)));
        HIP_TRY(hipMalloc(&r->d_lp2, NT * sizeof(mhx_real)));
    }
    if (E > 1 && r->emcee_preload) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: option EMCEE_PRELOAD has no many-ensembles form");
    if (E > 1 && r->emcee_stamp_words) return mhx_fail(MHX_EINVAL, "mhx_emcee_create: option EMCEE_STAMPS has no many-ensembles form");
    return done();
}

static int emcee_init(mhx_run* r, const mhx_real* init)
{
    // src/emcee.jl:29-34: the initial walkers are W draws from the wrapped prior -- on the device when it is the
    // (Mv)Normal of cfg.init_*; any other Distribution is drawn on the host side of the boundary and handed over
    if (!init && r->prop_kind < 0)
        return mhx_fail(MHX_EINVAL, "emcee: initial walkers [dim][nwalkers] are required (no (Mv)Normal prior in cfg.init_*)");
    mhx_ctx* ctx = r->ctx;
    const size_t nx = (size_t)r->dim * (size_t)r->n;
    if (init) HIP_TRY(hipMemcpyAsync(r->d_x, init, nx * sizeof(mhx_real), hipMemcpyHostToDevice, ctx->stream));
    mhx_emcee_args a = emcee_args(r);
    const mhx_real* tp = r->target->dparams;
    const unsigned grid = (unsigned)((r->ens_w + 255) / 256), E = (unsigned)r->n_ens;
    int draw = init ? 0 : 1;
    if (r->jit_init) {
        int rc = launch_module(r->jit_init, dim3(grid, E), 256, ctx->stream, a, tp, draw);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(k_emcee_init, dim3(grid, E), dim3(256), 0, ctx->stream, a, tp, draw);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return emcee_sync_state(r, 0);
}

// one launch: walkers [begin, begin + count) of half `h` move (a.sweep / a.save_slot set by the caller)
static int emcee_launch_half(mhx_run* r, mhx_emcee_args a, int h, int begin, int count)
{
    mhx_ctx* ctx = r->ctx;
    a.half = h;
    a.t_begin = begin;
    a.t_count = count;
    if (count <= 0) return MHX_OK;
    const unsigned E = (unsigned)r->n_ens;
    int rc;
    if (r->emcee_preload && r->step.mod_fn) {
        // MHX_JIT_PRELOAD, the one argument list that differs per launch: the hot arguments first, as scalars of their own (the kernel has
        // them preloaded), then the block and tparams -- a copy of the record with that list
        launch_rec k = r->step;
        k.ntail = 0;
        for (const void* p : std::initializer_list<const void*>{&a.lp, &a.seed, &a.ensemble_id, &a.sweep, &a.half, &a.nwalkers, &a.t_begin, &a.t_count, &a, &r->k_tp})
            k.tail[k.ntail++] = const_cast<void*>(p);
        rc = launch(k, ctx->stream, count, E, &a.xw);
    } else {
        rc = launch(r->step, ctx->stream, count, E, &a);
    }
    if (rc) return rc;
    r->stats.launches += 1;
    return MHX_OK;
}

#ifndef MHX_EMCEE_DEFER_DEFAULT
#define MHX_EMCEE_DEFER_DEFAULT 0
#endif
// record of walkers [lo, lo + cnt) from the walker-major state (the half the last launch of a call moved; see emcee_advance)
__global__ void __launch_bounds__(256)
k_emcee_record_half(const mhx_real* __restrict__ xw, const int pitch, const mhx_real* __restrict__ lp, const unsigned char* __restrict__ last,
                    mhx_real* samples, unsigned char* accepted, const int W, const int d, const long slot, const int lo, const int cnt)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cnt) return;
    const int i = lo + t;
    const long ld = W;
    mhx_real* row = samples + slot * (long)(d + 1) * ld + i;
    const mhx_real* xr = xw + (long)i * pitch;
    for (int k = 0; k < d; ++k) row[(long)k * ld] = xr[k];
    row[(long)d * ld] = lp[i];
    accepted[slot * ld + i] = last[i];
}

static int emcee_advance(mhx_run* r, uint64_t nsteps, uint32_t save_next, int save_slot, int thinning)
{
    const int W = r->ens_w, halfW = W / 2;
    const unsigned E = (unsigned)r->n_ens;                   // ensembles: the second grid dimension of every launch
    if (r->variant == KF_EMCEE_SEQ) {                        // the reference's sequential sweep: one launch, one wave per ensemble
        mhx_emcee_args a = emcee_args(r);
        a.sweep = (uint32_t)(r->tau + 1);
        a.nsweeps = (int)nsteps;
        a.save_next = save_next;
        a.save_slot = save_slot;
        a.thinning = thinning;
        if (int rc = launch(r->step, r->ctx->stream, 1, E, &a)) return rc;
        HIP_TRY(hipGetLastError());
        r->stats.launches += 1;
        r->tau += nsteps;
        return MHX_OK;
    }
    if (r->persist && !opt(r->ctx, "EMCEE_DEFER")) {      // a small ensemble: the whole call in one persistent block
        uint64_t done = 0;
        while (done < nsteps) {
            const uint64_t chunk = std::min<uint64_t>(nsteps - done, MHX_MAX_STEPS_PER_LAUNCH);
            mhx_emcee_args a = emcee_args(r);
            a.sweep = (uint32_t)(r->tau + 1);
            a.nsweeps = (int)chunk;
            a.save_next = save_next;
            a.save_slot = save_slot;
            a.thinning = thinning;
            if (int rc = launch(r->persist, r->ctx->stream, 1, E, &a)) return rc;      // a block (a CU) per ensemble
            r->stats.launches += 1;
            save_cursor_skip(r, chunk, thinning, &save_next, &save_slot);
            r->tau += chunk;
            done += chunk;
        }
        HIP_TRY(hipGetLastError());
        return MHX_OK;
    }
    // The cooperative kernel records a half ONE LAUNCH LATER: a half is at rest -- final for its sweep -- while the other one
    // moves, so the launch that moves half B of sweep k writes the record of half A (moved by the launch before), and the
    // first launch of sweep k + 1 writes the record of half B of sweep k; these stores leave at the START of a launch, off
    // its critical path, where the launch that moved the half would have had to wait for them at its end.  What is still
    // owed when the call ends (half B of the last recorded sweep) is written by k_emcee_record_half.
    const bool deferred = E == 1 && r->variant == KF_COOP_JIT && opt_int(r->ctx, "EMCEE_DEFER", MHX_EMCEE_DEFER_DEFAULT) != 0;      // (tuning knob; one ensemble only)
    long owed_b = -1;                                        // slot whose half B has not been recorded yet
    // MHX_EMCEE_SWEEP_DEFER=1 (tuning knob, off): sweep launches of the lane-group form record a sweep at the top of the NEXT launch, from
    // the rows every group loads anyway (mhx_emcee_coop_sweep_body) -- measured SLOWER, 8.34 against 7.60 us per sweep on one box: 6.7 MB
    // of stores at the head of the launch sit in front of the row loads the whole chain waits for
    const bool sweep_defer = E == 1 && r->sweep && r->variant == KF_COOP_JIT && opt_on(r->ctx, "EMCEE_SWEEP_DEFER");
    for (uint64_t s = 0; s < nsteps; ++s) {
        mhx_emcee_args a = emcee_args(r);
        a.sweep = (uint32_t)(r->tau + 1);
        long slot = -1;
        if (save_next != MHX_NO_SAVE && a.sweep == save_next) {
            slot = save_slot;
            ++save_slot;
            save_next += (uint32_t)thinning;
        }
        if (r->sweep && !deferred) {
            // the whole sweep in one launch: reads (d_xw, d_lp), writes every walker's new row to (d_xw2, d_lp2); then they swap
            a.save_slot = slot;
            if (sweep_defer) {                               // the record of a sweep leaves at the top of the NEXT launch (lane-group form)
                a.save_slot = -1;
                a.rec_other_slot = owed_b;
                owed_b = slot;
            }
            a.all_rows = s == 0 ? 1 : 0;                     // the other buffer holds nothing of this state yet
            // blocks of one half each, the second half's first: each half takes whole blocks; the scalar-factor form: mixed blocks, as
            // many as the larger half needs
            const long pb = r->sweep.per_block;
            const long items = r->sweep_mixed ? W - halfW : ((halfW + pb - 1) / pb + (W - halfW + pb - 1) / pb) * pb;
            if (int rc = launch(r->sweep, r->ctx->stream, items, E, &a)) return rc;
            std::swap(r->d_xw, r->d_xw2);
            std::swap(r->d_lp, r->d_lp2);
            r->stats.launches += 1;
            r->tau += 1;
            continue;
        }
        for (int h = 0; h < 2; ++h) {
            if (deferred) {
                a.save_slot = -1;
                a.rec_other_slot = h == 0 ? owed_b : slot;  // half B of the sweep before / half A of this sweep
                if (h == 0) owed_b = -1;
            } else {
                a.save_slot = slot;
            }
            int rc = emcee_launch_half(r, a, h, 0, h ? W - halfW : halfW);
            if (rc) return rc;
        }
        if (deferred) owed_b = slot;
        r->tau += 1;
    }
    if (deferred && owed_b >= 0) {
        const int cntb = W - halfW;
        hipLaunchKernelGGL(k_emcee_record_half, dim3((unsigned)((cntb + 255) / 256)), dim3(256), 0, r->ctx->stream,
                           (const mhx_real*)r->d_xw, mhx_xw_pitch(r->dim), (const mhx_real*)r->d_lp, (const unsigned char*)r->d_last,
                           r->d_samples, r->d_accepted, W, r->dim, owed_b, halfW, cntb);
        r->stats.launches += 1;
    } else if (sweep_defer && !deferred && owed_b >= 0) {     // the call's last recorded sweep: every walker, from the live state
        hipLaunchKernelGGL(k_emcee_record_half, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, r->ctx->stream,
                           (const mhx_real*)r->d_xw, mhx_xw_pitch(r->dim), (const mhx_real*)r->d_lp, (const unsigned char*)r->d_last,
                           r->d_samples, r->d_accepted, W, r->dim, owed_b, 0, W);
        r->stats.launches += 1;
    }
    HIP_TRY(hipGetLastError());
    if (r->emcee_stamp_words) {                              // tools only: the stamps of the call's last launch
        if (const char* fn = MHX_PROBE_OPT(r->ctx, "EMCEE_STAMPS_FILE")) {
            std::vector<uint64_t> h(r->emcee_stamp_words);
            HIP_TRY(hipStreamSynchronize(r->ctx->stream));
            HIP_TRY(hipMemcpy(h.data(), r->d_ybuf, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
            if (FILE* f = fopen(fn, "wb")) { fwrite(h.data(), sizeof(uint64_t), h.size(), f); fclose(f); }
        }
    }
    return MHX_OK;
}

// ---- building blocks of an ensemble sharded over GPUs (every rank holds the whole ensemble, moves its slice of the
// moving half, then the slices are exchanged; mhx/dist.py drives it with RCCL all-gathers)
int api_emcee_half_step(mhx_run* r, int half, int begin, int count)
{
    if (!r || r->kind != RUN_EMCEE) return mhx_fail(MHX_EINVAL, "mhx_emcee_half_step: not an ensemble run");
    if (!r->initialised) return mhx_fail(MHX_ESTATE, "mhx_emcee_half_step: run is not initialised");
    const int W = r->n, halfW = W / 2, cnt = half ? W - halfW : halfW;
    if (r->n_ens > 1) return mhx_fail(MHX_EINVAL, "mhx_emcee_half_step: a run of %d ensembles is not ONE ensemble to shard", r->n_ens);
    if (r->variant == KF_EMCEE_SEQ) return mhx_fail(MHX_EINVAL, "mhx_emcee_half_step: the sequential sweep has no halves");
    if ((half != 0 && half != 1) || begin < 0 || count < 0 || begin + count > cnt)
        return mhx_fail(MHX_EINVAL, "mhx_emcee_half_step: slice [%d, %d) is outside half %d of %d walkers", begin, begin + count, half, cnt);
    HIP_TRY(hipSetDevice(r->ctx->device));
    mhx_emcee_args a = emcee_args(r);
    a.sweep = (uint32_t)(r->tau + 1);
    int rc = emcee_launch_half(r, a, half, begin, count);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return MHX_OK;                                   // stream-ordered: the exchange and the next half-step queue behind it
}
int api_emcee_end_sweep(mhx_run* r)
{
    if (!r || r->kind != RUN_EMCEE) return mhx_fail(MHX_EINVAL, "mhx_emcee_end_sweep: not an ensemble run");
    r->tau += 1;
    return MHX_OK;
}

// ---- exchange of the moved slices between the ranks that share ONE ensemble (mhx_comm_allgather_walkers).  The slice of
// rank q of a half with `cnt` walkers is [cnt q / world, cnt (q+1) / world).  A rank's part of the staging buffer:
//   [maxc x pitch reals: walker rows][maxc reals: lp][maxc u32: accept counts][maxc u8: last accept flag]   (16-byte aligned sections)
struct emcee_xplan { long cnt, lo, maxc; size_t off_lp, off_acc, off_last, stride; int pitch; };
static emcee_xplan emcee_exchange_layout(const mhx_run* r, int half, int world)
{
    emcee_xplan p;
    const long W = r->n, halfW = W / 2;
    p.cnt = half ? W - halfW : halfW;
    p.lo = half ? halfW : 0;
    p.maxc = (p.cnt + world - 1) / world;
    p.pitch = mhx_xw_pitch(r->dim);
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    p.off_lp = up((size_t)p.maxc * p.pitch * sizeof(mhx_real));
    p.off_acc = p.off_lp + up((size_t)p.maxc * sizeof(mhx_real));
    p.off_last = p.off_acc + up((size_t)p.maxc * sizeof(uint32_t));
    p.stride = p.off_last + up((size_t)p.maxc);
    return p;
}
// dir 0: state -> the staging part of rank blockIdx.y0 (one rank); dir 1: staging parts of every OTHER rank -> state
__global__ void __launch_bounds__(256)
k_emcee_exchange(mhx_real* __restrict__ xw, mhx_real* __restrict__ lp, uint32_t* __restrict__ acc, unsigned char* __restrict__ last,
                 char* __restrict__ stage, const emcee_xplan p, const int world, const int me, const int unpack)
{
    const int q = unpack ? (int)blockIdx.y : me;
    if (unpack && q == me) return;
    const long b = p.cnt * q / world, e = p.cnt * (q + 1) / world, count = e - b;
    char* part = stage + (unpack ? p.stride * (size_t)q : 0);
    mhx_real* srow = (mhx_real*)part;
    mhx_real* slp = (mhx_real*)(part + p.off_lp);
    uint32_t* sacc = (uint32_t*)(part + p.off_acc);
    unsigned char* slast = (unsigned char*)(part + p.off_last);
    const long first = p.lo + b;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < count * p.pitch; t += (long)gridDim.x * blockDim.x) {
        if (unpack) xw[first * p.pitch + t] = srow[t]; else srow[t] = xw[first * p.pitch + t];
    }
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (long)gridDim.x * blockDim.x) {
        if (unpack) { lp[first + t] = slp[t]; acc[first + t] = sacc[t]; last[first + t] = slast[t]; }
        else { slp[t] = lp[first + t]; sacc[t] = acc[first + t]; slast[t] = last[first + t]; }
    }
}
int api_emcee_exchange_plan(mhx_run* r, int half, int world, size_t* stride, void** stream)
{
    if (!r || r->kind != RUN_EMCEE) return mhx_fail(MHX_EINVAL, "mhx_emcee_exchange_plan: not an ensemble run");
    if (r->n_ens > 1) return mhx_fail(MHX_EINVAL, "mhx_emcee_exchange_plan: a run of %d ensembles is not ONE ensemble to shard", r->n_ens);
    if (!r->d_xw) return mhx_fail(MHX_ESTATE, "a sharded ensemble needs the walker-major state (compile-time-dimension kernels)");
    if ((half != 0 && half != 1) || world < 1) return mhx_fail(MHX_EINVAL, "mhx_emcee_exchange_plan: half %d, world %d", half, world);
    const emcee_xplan p = emcee_exchange_layout(r, half, world);
    if (stride) *stride = p.stride;
    if (stream) *stream = (void*)r->ctx->stream;
    return MHX_OK;
}
static int emcee_exchange_launch(mhx_run* r, int half, int rank, int world, void* stage, int unpack)
{
    if (!r || r->kind != RUN_EMCEE || !r->d_xw) return mhx_fail(MHX_EINVAL, "mhx_emcee_exchange: not a walker-major ensemble run");
    if (rank < 0 || rank >= world || !stage) return mhx_fail(MHX_EINVAL, "mhx_emcee_exchange: rank %d of %d", rank, world);
    HIP_TRY(hipSetDevice(r->ctx->device));
    const emcee_xplan p = emcee_exchange_layout(r, half, world);
    const unsigned gx = (unsigned)std::min<long>((p.maxc * p.pitch + 255) / 256, 1024);
    hipLaunchKernelGGL(k_emcee_exchange, dim3(gx ? gx : 1, unpack ? world : 1), dim3(256), 0, r->ctx->stream, r->d_xw, r->d_lp, r->d_acc,
                       r->d_last, (char*)stage, p, world, rank, unpack);
    HIP_TRY(hipGetLastError());
    return MHX_OK;
}
int api_emcee_exchange_pack(mhx_run* r, int half, int rank, int world, void* part) { return emcee_exchange_launch(r, half, rank, world, part, 0); }
int api_emcee_exchange_unpack(mhx_run* r, int half, int rank, int world, const void* stage, size_t stride)
{
    (void)stride;
    return emcee_exchange_launch(r, half, rank, world, const_cast<void*>(stage), 1);
}
int api_emcee_device_state(mhx_run* r, mhx_real** xw, int32_t* pitch, mhx_real** lp, uint32_t** acc_count, uint8_t** last_acc)
{
    if (!r || r->kind != RUN_EMCEE) return mhx_fail(MHX_EINVAL, "mhx_emcee_device_state: not an ensemble run");
    if (!r->d_xw) return mhx_fail(MHX_ESTATE, "mhx_emcee_device_state: this run keeps its walkers in the [dim][W] layout "
                                          "(run-time-dimension kernel); a sharded ensemble needs the walker-major state");
    if (xw) *xw = r->d_xw;
    if (pitch) *pitch = mhx_xw_pitch(r->dim);
    if (lp) *lp = r->d_lp;
    if (acc_count) *acc_count = r->d_acc;
    if (last_acc) *last_acc = r->d_last;
    return MHX_OK;
}
