// RAM host side (included by mhx_api.hip): RobustAdaptiveMetropolis, src/RobustAdaptiveMetropolis.jl:75-278

// (G lanes per chain, R rows per lane) shapes built ahead of time; dim <= G R <= dim + MHX_RAM_SLACK
#ifndef MHX_RAM_WAVES
#if MHX_REAL64
#define MHX_RAM_WAVES(G, R) ((R) <= 2 ? 4 : ((R) <= 4 ? 2 : 1))          // a double takes two VGPRs
#else
#define MHX_RAM_WAVES(G, R) ((R) <= 4 ? 4 : ((R) <= 8 ? 3 : 1))
#endif
#endif
// Waves per SIMD of the variant used with the dense Gaussian target (the factor all chains share is one more stream per step,
// through L2, and one more column sweep): fp64 shapes with 3 or 4 rows per lane run it at 3 waves per SIMD -- 168 registers, the
// per-step vectors spilled -- and hide that stream behind the third wave (d = 200: +8 % adapting, +22 % with a fixed factor; with
// a separable target the same bound costs 3 - 12 %, DESIGN.md 6.3).  LDS admits it since round 3: 11.4 KB per wave at d = 200.
#define MHX_RAM_WAVES_DENSE(G, R) ((MHX_REAL64 && ((R) == 3 || (R) == 4)) ? 3 : MHX_RAM_WAVES(G, R))
template <int G, int R, int W>
__global__ void __launch_bounds__(64, W)
k_ram(const mhx_ram_args a, const mhx_real* __restrict__ tparams)
{
    extern __shared__ mhx_real mhx_ram_lds[];
    mhx_ram_body<G, R, MHX_TARGET_DYNAMIC>(a, tparams, mhx_ram_lds);
}
// the deferred-factor form (MHX_FLAG_RAM_DEFERRED): one chain per wave, R rows per lane, two waves per SIMD
#ifndef MHX_RAM_DEFER_WAVES
#define MHX_RAM_DEFER_WAVES 2
#endif
template <int R, int K>
__global__ void __launch_bounds__(64, MHX_RAM_DEFER_WAVES)
k_ram_defer(const mhx_ram_args a, const mhx_real* __restrict__ tparams)
{
    extern __shared__ mhx_real mhx_ram_lds[];
    mhx_ram_defer_body<R, K, MHX_TARGET_DYNAMIC>(a, tparams, mhx_ram_lds);
}
typedef void (*ram_fn)(const mhx_ram_args, const mhx_real*);
static ram_fn ram_defer_fn(int R)
{
    switch (R) {
    case 1: return k_ram_defer<1, MHX_RAM_DEFER_K>;
    case 2: return k_ram_defer<2, MHX_RAM_DEFER_K>;
    case 3: return k_ram_defer<3, MHX_RAM_DEFER_K>;
    default: return k_ram_defer<4, MHX_RAM_DEFER_K>;
    }
}
struct ram_shape { int G, R; int ring_f; void (*fn)(const mhx_ram_args, const mhx_real*); void (*fn_dense)(const mhx_ram_args, const mhx_real*); };
#define RAM_SHAPE(G, R) {G, R, MHX_RAM_RING(G, R), k_ram<G, R, MHX_RAM_WAVES(G, R)>, k_ram<G, R, MHX_RAM_WAVES_DENSE(G, R)>}
static const ram_shape k_ram_shapes[] = {
    // the kernel is bound by instruction issue and the per-column overhead is shared by the 64/G chains of
    // a wave: narrow groups while the rows fit
    RAM_SHAPE(16, 1), RAM_SHAPE(16, 2), RAM_SHAPE(16, 4),
    RAM_SHAPE(32, 3), RAM_SHAPE(32, 4), RAM_SHAPE(32, 5), RAM_SHAPE(32, 6), RAM_SHAPE(32, 7), RAM_SHAPE(32, 8),
    RAM_SHAPE(64, 4), RAM_SHAPE(64, 5), RAM_SHAPE(64, 6), RAM_SHAPE(64, 7), RAM_SHAPE(64, 8), RAM_SHAPE(64, 12), RAM_SHAPE(64, 16),
};
// smallest pre-built shape that holds `d` rows (the table is ordered by G R)
static const ram_shape* ram_pick_shape(const mhx_ctx* ctx, int d)
{
    const int fg = opt_int(ctx, "RAM_G", 0);           // tuning knob: restrict to one group width
    if (MHX_REAL64 && !fg)                                  // fp64: at most 4 rows per lane while a wider group can hold the chain
        for (const auto& sh : k_ram_shapes)
            if (d <= sh.G * sh.R && sh.R <= 4) return &sh;
    for (const auto& sh : k_ram_shapes)
        if (d <= sh.G * sh.R && (!fg || sh.G == fg)) return &sh;
    for (const auto& sh : k_ram_shapes)
        if (d <= sh.G * sh.R) return &sh;
    return nullptr;
}
__global__ void __launch_bounds__(256)
k_ram_init(const mhx_ram_args a, const mhx_real* __restrict__ tparams, const int draw)
{
    mhx_ram_init_body<MHX_TARGET_DYNAMIC>(a, tparams, draw);
}

// packed lower triangle, row-major (ABI, dense stride) <-> column-major (device: [chain][2][tri_pad], `stride`
// floats between chains; the current buffer of chain c is sel[c]), one thread per element
__global__ void __launch_bounds__(256)
k_ram_repack(const mhx_real* __restrict__ in, mhx_real* __restrict__ out, const unsigned char* __restrict__ sel,
             const int d, const long nchains, const long stride, const int to_colmajor, const int shared_in = 0)
{
    const long tri = (long)d * (d + 1) / 2;
    const long trip = mhx_ram_tri_pad(d);
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= tri * nchains) return;
    const long c = e / tri;
    const long k = e - c * tri;
    // decode k as a ROW-major packed index (i >= j): k = i(i+1)/2 + j
    long i = (long)((__builtin_sqrt(8.0 * (double)k + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= k) ++i;
    while (i * (i + 1) / 2 > k) --i;
    const long j = k - i * (i + 1) / 2;
    const long kc = mhx_ram_col_off((int)j, d) + (i - j);      // column-major packed index of (i, j)
    const long buf = sel ? (long)sel[c] : 0;
    if (to_colmajor) out[c * stride + buf * trip + kc] = in[(shared_in ? 0 : c * tri) + k];     // shared_in: one factor for every chain
    else out[c * tri + k] = in[c * stride + buf * trip + kc];
}

__global__ void __launch_bounds__(256)
k_ram_unit_diag(mhx_real* __restrict__ S, const int d, const long nchains)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)d * nchains) return;
    const long c = e / d;
    const int i = (int)(e - c * d);
    S[c * 2 * mhx_ram_tri_pad(d) + mhx_ram_col_off(i, d)] = MHX_R(1.0);
}

// the current factors of a few WATCHED chains, packed row-major (the ABI format), into out[w][tri]
__global__ void __launch_bounds__(256)
k_ram_repack_watch(const mhx_real* __restrict__ S, mhx_real* __restrict__ out, const unsigned char* __restrict__ sel,
                   const int* __restrict__ chains, const int nwatch, const int d)
{
    const long tri = (long)d * (d + 1) / 2;
    const long trip = mhx_ram_tri_pad(d);
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= tri * nwatch) return;
    const long w = e / tri;
    const long k = e - w * tri;
    long i = (long)((__builtin_sqrt(8.0 * (double)k + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= k) ++i;
    while (i * (i + 1) / 2 > k) --i;
    const long j = k - i * (i + 1) / 2;
    const long c = chains[w];
    out[e] = S[(2 * c + (long)sel[c]) * trip + mhx_ram_col_off((int)j, d) + (i - j)];
}

// dmin = dmax = diag(S) of the current factor, [nchains][d]
__global__ void __launch_bounds__(256)
k_ram_diag(const mhx_real* __restrict__ S, const unsigned char* __restrict__ sel,
           mhx_real* __restrict__ dmin, mhx_real* __restrict__ dmax, const int d, const long nchains)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)d * nchains) return;
    const long c = e / d;
    const int i = (int)(e - c * d);
    const long trip = mhx_ram_tri_pad(d);
    const mhx_real v = S[(2 * c + sel[c]) * trip + mhx_ram_col_off(i, d)];
    dmin[e] = v;
    dmax[e] = v;
}

// [n][d] -> [d][n]
__global__ void __launch_bounds__(256)
k_transpose_nd(const mhx_real* __restrict__ in, mhx_real* __restrict__ out, const int d, const long n)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)d * n) return;
    const long c = e % n;
    const long k = e / n;
    out[e] = in[c * d + k];
}

static mhx_ram_args ram_args(const mhx_run* r)
{
    mhx_ram_args a;
    memset(&a, 0, sizeof a);
    a.x = r->d_x; a.lp = r->d_lp; a.acc_count = r->d_acc; a.acc_total = r->d_acc_total;
    a.samples = r->d_samples; a.accepted = r->d_accepted; a.last_acc = r->d_last;
    a.S = r->d_S; a.sel = r->d_Ssel; a.status = r->d_status;
    a.dmin = r->d_dmin; a.dmax = r->d_dmax; a.eta = r->d_eta; a.acol = r->d_pvec; a.loga = r->d_loga;
    a.rec_loga = r->rec_loga_view;
    a.defer = r->d_defer;
    a.prof = MHX_PROBE_OPT(r->ctx, "RAM_PROF") ? 1 : 0;
    a.seed = r->seed; a.first_chain = r->first_id;
    a.nchains = r->n; a.ld = r->n; a.dim = r->dim;
    a.target_kind = r->target->kind; a.ntparams = r->target->nparams; a.tconst = r->target->cst;
    a.alpha = (mhx_real)r->ramcfg.alpha; a.eig_lo = (mhx_real)r->ramcfg.eig_lo; a.eig_hi = (mhx_real)r->ramcfg.eig_hi;
    a.default_bounds = (r->ramcfg.eig_lo == 0.0 && std::isinf(r->ramcfg.eig_hi) && r->ramcfg.eig_hi > 0) ? 1 : 0;
    a.save_next = MHX_NO_SAVE; a.thinning = 1;
    return a;
}

static unsigned grid1d(long n, int block) { return (unsigned)((n + block - 1) / block); }

// The launch record of a RAM run's step kernel -- kernel(args, tparams): a block is ONE wave of 64 / G chains (the deferred form: one
// chain), the grid whole rounds of 8 blocks, the LDS each chain's ring and mirror.  `m`: the module of a user target, else the kernel
// is pre-built.  ram_pick_shape reads the option RAM_G, and options are read when they are used: api_ram_create fills r->step for
// the shape of that moment, and ram_advance asks again at every call (see there).
static int ram_step_record(mhx_run* r, jit_module* m, launch_rec* out)
{
    const int d = r->dim;
    const ram_shape* sh = ram_pick_shape(r->ctx, d);
    if (!sh) return mhx_fail(MHX_EINVAL, "RAM: dim %d exceeds the largest kernel shape", d);
    const int cpw = r->defer_R ? 1 : 64 / sh->G;                     // chains per wave (= block)
    const ram_fn fn = r->defer_R ? ram_defer_fn(r->defer_R) : (r->target->kind == MHX_TARGET_CORR_GAUSS ? sh->fn_dense : sh->fn);
    const int ring_f = r->defer_R ? MHX_RAM_RING(64, r->defer_R) : sh->ring_f;
    size_t lds = (size_t)cpw * (size_t)(mhx_ram_rings(ring_f, d) + mhx_ram_mirror(d)) * sizeof(mhx_real);
    if (r->defer_R) lds += (size_t)MHX_RAM_DEFER_STAGE * sizeof(mhx_real);       // the fold's coefficient staging
    *out = rec_shape("RAM kernel", 64, cpw, lds, {&r->k_tp}, 8);
    return m ? rec_bind(out, m, "mhx_jit_ram") : rec_bind(out, (const void*)fn);
}

int api_ram_create(mhx_ctx* ctx, const mhx_target* t, const mhx_ram_cfg* cfg, mhx_run** out)
{
    if (!ctx || !t || !cfg || !out) return mhx_fail(MHX_EINVAL, "mhx_ram_create: NULL argument");
    if (cfg->dim != t->dim) return mhx_fail(MHX_EINVAL, "mhx_ram_create: dim %d != model dim %d", cfg->dim, t->dim);
    if (cfg->nchains <= 0) return mhx_fail(MHX_EINVAL, "mhx_ram_create: nchains must be positive");
    if (cfg->dim > 1024) return mhx_fail(MHX_EINVAL, "mhx_ram_create: dim %d > 1024 is not supported by the wave-per-chain kernel", cfg->dim);
    if (!(cfg->alpha > 0.0 && cfg->alpha < 1.0)) return mhx_fail(MHX_EINVAL, "mhx_ram_create: alpha must be in (0,1)");
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<mhx_run> r(new mhx_run);
    r->dtype = ctx->dtype;
    r->ctx = ctx; r->target = t; r->kind = RUN_RAM;
    r->dim = cfg->dim; r->n = cfg->nchains; r->seed = cfg->seed; r->first_id = cfg->first_chain;
    r->flags = cfg->flags; r->ramcfg = *cfg;
    int rc = run_alloc_state(r.get());
    if (rc) return rc;
    const long d = r->dim, n = r->n, tri = d * (d + 1) / 2, trip = mhx_ram_tri_pad((int)d);
    HIP_TRY(hipMalloc(&r->d_S, (size_t)(2 * trip * n) * sizeof(mhx_real)));
    HIP_TRY(hipMemsetAsync(r->d_S, 0, (size_t)(2 * trip * n) * sizeof(mhx_real), ctx->stream));
    HIP_TRY(hipMalloc(&r->d_Ssel, (size_t)n));
    HIP_TRY(hipMalloc(&r->d_status, (size_t)n));
    HIP_TRY(hipMalloc(&r->d_dmin, (size_t)(d * n) * sizeof(mhx_real)));
    HIP_TRY(hipMalloc(&r->d_dmax, (size_t)(d * n) * sizeof(mhx_real)));
    HIP_TRY(hipMalloc(&r->d_loga, (size_t)n * sizeof(mhx_real)));
    HIP_TRY(hipMemsetAsync(r->d_loga, 0, (size_t)n * sizeof(mhx_real), ctx->stream));
    HIP_TRY(hipMemsetAsync(r->d_Ssel, 0, (size_t)n, ctx->stream));
    HIP_TRY(hipMemsetAsync(r->d_status, 0, (size_t)n, ctx->stream));
    // the Gaussian target's factor in the column-major packed layout of the cooperative sweep
    HIP_TRY(hipMalloc(&r->d_pvec, (size_t)(t->kind == MHX_TARGET_CORR_GAUSS ? trip : 4) * sizeof(mhx_real)));
    HIP_TRY(hipMemsetAsync(r->d_pvec, 0, (size_t)(t->kind == MHX_TARGET_CORR_GAUSS ? trip : 4) * sizeof(mhx_real), ctx->stream));
    if (t->kind == MHX_TARGET_CORR_GAUSS) {
        hipLaunchKernelGGL(k_ram_repack, dim3(grid1d(tri, 256)), dim3(256), 0, ctx->stream, t->dparams, r->d_pvec,
                           (const unsigned char*)nullptr, (int)d, 1L, trip, 1);
        HIP_TRY(hipGetLastError());
    }
    if (cfg->flags & MHX_FLAG_RAM_DEFERRED) {
        // the deferred-factor form: its own rounding (spec 3.12), one chain per wave
        if (d > 256) return mhx_fail(MHX_EINVAL, "mhx_ram_create: MHX_FLAG_RAM_DEFERRED holds a chain in one wave: dim %ld > 256", d);
        r->defer_R = (int)((d + 63) / 64);
        r->variant = KF_RAM_DEFER;
        const size_t per = (size_t)MHX_RAM_DEFER_REALS(MHX_RAM_DEFER_K, r->defer_R);
        HIP_TRY(hipMalloc(&r->d_defer, per * (size_t)n * sizeof(mhx_real)));
        HIP_TRY(hipMemsetAsync(r->d_defer, 0, per * (size_t)n * sizeof(mhx_real), ctx->stream));
    }
    jit_module* m = nullptr;
    if (t->kind == MHX_TARGET_USER) {
        const ram_shape* sh = ram_pick_shape(ctx, (int)d);
        const int jg = r->defer_R ? 64 : sh->G, jr = r->defer_R ? r->defer_R : sh->R;
        std::vector<std::string> defs = {"MHX_JIT_RAM=1", "MHX_JIT_G=" + std::to_string(jg), "MHX_JIT_R=" + std::to_string(jr),
                                         "MHX_JIT_TK=" + std::to_string(t->kind)};
        if (r->defer_R) defs.push_back("MHX_JIT_DEFER_K=" + std::to_string(MHX_RAM_DEFER_K));
        rc = jit_compile(ctx, jit_source(t, "mhx_ram_kernels.h"), defs, &m);
        if (rc) return rc;
        if ((rc = jit_function(m, "mhx_jit_ram_init", &r->jit_init))) return rc;
    }
    if ((rc = ram_step_record(r.get(), m, &r->step))) return rc;
    // S0 = I (RAM.jl:198-199) until mhx_ram_set_factor says otherwise
    if ((rc = api_ram_set_factor(r.get(), nullptr))) return rc;
    *out = r.release();
    return MHX_OK;
}

static int ram_set_factor(mhx_run* r, const mhx_real* S, const bool shared);
int api_ram_set_factor(mhx_run* r, const mhx_real* S) { return ram_set_factor(r, S, false); }
// the same factor for every chain (the reference's RobustAdaptiveMetropolis(S = ...), RAM.jl:198-206): [dim(dim+1)/2]
int api_ram_set_factor_all(mhx_run* r, const mhx_real* S) { return ram_set_factor(r, S, true); }
static int ram_set_factor(mhx_run* r, const mhx_real* S, const bool shared)
{
    if (!r || r->kind != RUN_RAM) return mhx_fail(MHX_EINVAL, "mhx_ram_set_factor: not a RAM run");
    mhx_ctx* ctx = r->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const long d = r->dim, n = r->n, tri = d * (d + 1) / 2, trip = mhx_ram_tri_pad((int)d);
    if (!S) {
        HIP_TRY(hipMemsetAsync(r->d_Ssel, 0, (size_t)n, ctx->stream));
        HIP_TRY(hipMemsetAsync(r->d_S, 0, (size_t)(2 * trip * n) * sizeof(mhx_real), ctx->stream));
        hipLaunchKernelGGL(k_ram_unit_diag, dim3(grid1d(d * n, 256)), dim3(256), 0, ctx->stream, r->d_S, (int)d, n);
    } else {
        const long nin = shared ? 1 : n;                    // factors handed over
        for (long c = 0; c < nin; ++c)
            for (long i = 0; i < d; ++i)
                if (!(S[c * tri + i * (i + 1) / 2 + i] > MHX_R(0.0)))
                    return mhx_fail(MHX_ENOTPD, "mhx_ram_set_factor: chain %ld has a non-positive diagonal entry %ld", c, i);
        // validated: only now do the selectors go back to buffer 0 (a refused call leaves the run untouched)
        mhx_real* tmp = nullptr;
        HIP_TRY(hipMalloc(&tmp, (size_t)(tri * nin) * sizeof(mhx_real)));
        hipError_t e = hipMemsetAsync(r->d_Ssel, 0, (size_t)n, ctx->stream);       // (no HIP_TRY from here on: `tmp` is released below)
        if (e == hipSuccess) e = hipMemcpyAsync(tmp, S, (size_t)(tri * nin) * sizeof(mhx_real), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_ram_repack, dim3(grid1d(tri * n, 256)), dim3(256), 0, ctx->stream, tmp, r->d_S,
                               (const unsigned char*)nullptr, (int)d, n, 2 * trip, 1, shared ? 1 : 0);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        }
        (void)hipFree(tmp);
        if (e != hipSuccess) return mhx_fail(MHX_EHIP, "mhx_ram_set_factor: %s", hipGetErrorString(e));
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ram_diag, dim3(grid1d(d * n, 256)), dim3(256), 0, ctx->stream, r->d_S, r->d_Ssel,
                       r->d_dmin, r->d_dmax, (int)d, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MHX_OK;
}

int api_ram_get_factor(mhx_run* r, mhx_real* S, uint8_t* status)
{
    if (!r || r->kind != RUN_RAM) return mhx_fail(MHX_EINVAL, "mhx_ram_get_factor: not a RAM run");
    mhx_ctx* ctx = r->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const long d = r->dim, n = r->n, tri = d * (d + 1) / 2;
    if (S) {
        mhx_real* tmp = nullptr;
        HIP_TRY(hipMalloc(&tmp, (size_t)(tri * n) * sizeof(mhx_real)));
        hipLaunchKernelGGL(k_ram_repack, dim3(grid1d(tri * n, 256)), dim3(256), 0, ctx->stream, r->d_S, tmp, r->d_Ssel,
                           (int)d, n, 2 * mhx_ram_tri_pad((int)d), 0);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(S, tmp, (size_t)(tri * n) * sizeof(mhx_real), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        (void)hipFree(tmp);
        if (e != hipSuccess) return mhx_fail(MHX_EHIP, "mhx_ram_get_factor: %s", hipGetErrorString(e));
    }
    if (status) COPY_SYNC(ctx->stream, status, r->d_status, (size_t)n, hipMemcpyDeviceToHost);
    return MHX_OK;
}

int api_ram_get_diag_range(mhx_run* r, mhx_real* diag_min, mhx_real* diag_max)
{
    if (!r || r->kind != RUN_RAM) return mhx_fail(MHX_EINVAL, "mhx_ram_get_diag_range: not a RAM run");
    mhx_ctx* ctx = r->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const long d = r->dim, n = r->n;
    mhx_real* tmp = nullptr;
    HIP_TRY(hipMalloc(&tmp, (size_t)(d * n) * sizeof(mhx_real)));
    int rc = MHX_OK;
    for (int k = 0; k < 2 && rc == MHX_OK; ++k) {
        mhx_real* host = k ? diag_max : diag_min;
        if (!host) continue;
        hipLaunchKernelGGL(k_transpose_nd, dim3(grid1d(d * n, 256)), dim3(256), 0, ctx->stream,
                           k ? r->d_dmax : r->d_dmin, tmp, (int)d, n);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(host, tmp, (size_t)(d * n) * sizeof(mhx_real), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = mhx_fail(MHX_EHIP, "mhx_ram_get_diag_range: %s", hipGetErrorString(e));
    }
    (void)hipFree(tmp);
    return rc;
}

// RobustAdaptiveMetropolisState beyond x / logprob / S (RAM.jl:99-114): logα of each chain's latest transition (kept as
// min(lp' - lp, 0) so that users can average exp(logα), :141-147), the adaptation step size η of the latest warm-up
// transition (0 before any, :211), the iteration counter (1 + transitions) and isaccept
int api_ram_get_adapt_state(mhx_run* r, mhx_real* log_alpha, double* eta, uint8_t* isaccept, uint64_t* iteration)
{
    if (!r || r->kind != RUN_RAM) return mhx_fail(MHX_EINVAL, "mhx_ram_get_adapt_state: not a RAM run");
    if (!r->initialised) return mhx_fail(MHX_ESTATE, "mhx_ram_get_adapt_state: run is not initialised");
    mhx_ctx* ctx = r->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (log_alpha) COPY_SYNC(ctx->stream, log_alpha, r->d_loga, (size_t)r->n * sizeof(mhx_real), hipMemcpyDeviceToHost);
    if (isaccept) COPY_SYNC(ctx->stream, isaccept, r->d_last, (size_t)r->n, hipMemcpyDeviceToHost);
    if (eta) *eta = r->last_eta;
    if (iteration) *iteration = r->tau + 1;
    return MHX_OK;
}

// Per-recorded-step sampler statistics of a sampling call (what the reference's callback sees in `state` after every saved
// step, test/RobustAdaptiveMetropolis.jl:11-28: state.logα, state.η, state.isaccept): logα of every recorded transition goes to
// d_rec_loga [n_samples][n] on the device (the kernel writes it beside the sample record); η is the same for all chains --
// iteration^-gamma of the latest ADAPTING transition at or before the recorded one -- and follows from the schedule here.
// state.S of the watched chains behind the sample just recorded
static int ram_watch_record(mhx_run* r)
{
    const long tri = (long)r->dim * (r->dim + 1) / 2;
    hipLaunchKernelGGL(k_ram_repack_watch, dim3(grid1d(tri * r->watch_n, 256)), dim3(256), 0, r->ctx->stream, (const mhx_real*)r->d_S,
                       r->d_watch + (size_t)r->watch_count * (size_t)r->watch_n * (size_t)tri, (const unsigned char*)r->d_Ssel,
                       (const int*)r->d_watch_chains, r->watch_n, r->dim);
    HIP_TRY(hipGetLastError());
    r->watch_count += 1;
    return MHX_OK;
}

// Watch the factors of a few chains: after EVERY recorded step of a sampling call the current S of each watched chain is kept
// (what a `callback(rng, model, sampler, sample, state, i)` that stores `state.S` sees: test/RobustAdaptiveMetropolis.jl:11-28,57-69
// checks the eigenvalue bounds on exactly that record).  The kernel is persistent over the transitions of a launch, so a watched run
// ends a launch at every recorded transition -- a cost paid only when chains are watched.
int api_ram_watch_factors(mhx_run* r, const int32_t* chains, int n)
{
    if (!r || r->kind != RUN_RAM) return mhx_fail(MHX_EINVAL, "mhx_ram_watch_factors: not a RAM run");
    if (n < 0 || (n > 0 && !chains)) return mhx_fail(MHX_EINVAL, "mhx_ram_watch_factors: bad chain list");
    if (n > 0 && r->defer_R)
        return mhx_fail(MHX_EINVAL, "mhx_ram_watch_factors: a MHX_FLAG_RAM_DEFERRED run holds its factor whole only between launches (a watched "
                                    "run would end a launch -- and flush -- at every recorded step: the sweep form's traffic, another rounding)");
    for (int i = 0; i < n; ++i)
        if (chains[i] < 0 || chains[i] >= r->n) return mhx_fail(MHX_EINVAL, "mhx_ram_watch_factors: chain %d of %d", chains[i], r->n);
    HIP_TRY(hipSetDevice(r->ctx->device));
    if (r->d_watch_chains) { (void)hipFree(r->d_watch_chains); r->d_watch_chains = nullptr; }
    r->watch_n = 0; r->watch_count = 0;
    if (n == 0) return MHX_OK;
    HIP_TRY(hipMalloc(&r->d_watch_chains, (size_t)n * sizeof(int32_t)));
    COPY_SYNC(r->ctx->stream, r->d_watch_chains, chains, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
    r->watch_n = n;
    return MHX_OK;
}

int api_ram_get_watched_factors(mhx_run* r, mhx_real* S, int64_t capacity, int64_t* n_recorded, int32_t* n_watched)
{
    const bool ram = r && r->kind == RUN_RAM;                       // the counts are written on every path: 0 for a run that is not RAM
    if (n_recorded) *n_recorded = ram ? r->watch_count : 0;
    if (n_watched) *n_watched = ram ? r->watch_n : 0;
    if (!ram) return mhx_fail(MHX_EINVAL, "mhx_ram_get_watched_factors: not a RAM run");
    if (!S) return MHX_OK;                                          // a query
    if (r->watch_n <= 0 || r->watch_count <= 0) return mhx_fail(MHX_ESTATE, "mhx_ram_get_watched_factors: nothing was recorded (mhx_ram_watch_factors, then a sampling call that keeps samples)");
    if (capacity < r->watch_count) return mhx_fail(MHX_EINVAL, "mhx_ram_get_watched_factors: the buffer holds %ld samples, %ld were recorded", (long)capacity, (long)r->watch_count);
    HIP_TRY(hipSetDevice(r->ctx->device));
    const size_t tri = (size_t)r->dim * (size_t)(r->dim + 1) / 2;
    COPY_SYNC(r->ctx->stream, S, r->d_watch, (size_t)r->watch_count * (size_t)r->watch_n * tri * sizeof(mhx_real), hipMemcpyDeviceToHost);
    return MHX_OK;
}

static int ram_prepare_step_stats(mhx_run* r, const mhx_schedule* s, uint64_t n_adapt)
{
    mhx_ctx* ctx = r->ctx;
    const size_t N = (size_t)s->n_samples, n = (size_t)r->n;
    int rc = ensure_buffer((void**)&r->d_rec_loga, &r->rec_loga_cap, N * n * sizeof(mhx_real), "mhx_run_sample", "step-statistics buffer");
    if (rc) return rc;
    r->rec_loga_view = r->d_rec_loga;
    r->rec_n = s->n_samples;
    r->rec_eta.assign(N, r->last_eta);
    for (size_t i = 0; i < N; ++i) {
        const uint64_t t = (uint64_t)s->discard_initial + (uint64_t)i * (uint64_t)s->thinning;   // transitions of this call behind sample i
        const uint64_t na = t < n_adapt ? t : n_adapt;                                            // ... of which adapted
        if (na) r->rec_eta[i] = (double)(mhx_real)std::pow((double)(r->tau + na), -(double)(mhx_real)r->ramcfg.gamma);
    }
    // sample 1 of an un-discarded call is the current state: its statistics are the state's own
    if (s->discard_initial == 0)
        HIP_TRY(hipMemcpyAsync(r->d_rec_loga, r->d_loga, n * sizeof(mhx_real), hipMemcpyDeviceToDevice, ctx->stream));
    // watched chains (mhx_ram_watch_factors): room for their factors after every recorded step of this call
    r->watch_count = 0;
    if (r->watch_n > 0) {
        const size_t tri = (size_t)r->dim * (size_t)(r->dim + 1) / 2;
        rc = ensure_buffer((void**)&r->d_watch, &r->watch_cap, N * (size_t)r->watch_n * tri * sizeof(mhx_real), "mhx_run_sample", "watched-factor buffer");
        if (rc) return rc;
        if (s->discard_initial == 0) { rc = ram_watch_record(r); if (rc) return rc; }
    }
    return MHX_OK;
}

int api_ram_get_step_stats(mhx_run* r, mhx_real* log_alpha, double* eta, int64_t capacity, int64_t* n_recorded)
{
    const bool ram = r && r->kind == RUN_RAM;                    // the count is written on every path: 0 for a run that is not RAM
    if (n_recorded) *n_recorded = ram ? r->rec_n : 0;
    if (!ram) return mhx_fail(MHX_EINVAL, "mhx_ram_get_step_stats: not a RAM run");
    if (!log_alpha && !eta) return MHX_OK;                       // a query of the recorded count
    if (r->rec_n <= 0) return mhx_fail(MHX_ESTATE, "mhx_ram_get_step_stats: the last sampling call recorded no samples");
    if (capacity < r->rec_n)
        return mhx_fail(MHX_EINVAL, "mhx_ram_get_step_stats: the buffers hold %ld samples, the last call recorded %ld", (long)capacity, (long)r->rec_n);
    HIP_TRY(hipSetDevice(r->ctx->device));
    if (log_alpha) COPY_SYNC(r->ctx->stream, log_alpha, r->d_rec_loga, (size_t)r->rec_n * (size_t)r->n * sizeof(mhx_real), hipMemcpyDeviceToHost);
    if (eta) memcpy(eta, r->rec_eta.data(), (size_t)r->rec_n * sizeof(double));
    return MHX_OK;
}

static int ram_init(mhx_run* r, const mhx_real* init)
{
    r->last_eta = 0.0;
    mhx_ctx* ctx = r->ctx;
    const size_t nx = (size_t)r->dim * (size_t)r->n;
    if (init) HIP_TRY(hipMemcpyAsync(r->d_x, init, nx * sizeof(mhx_real), hipMemcpyHostToDevice, ctx->stream));
    mhx_ram_args a = ram_args(r);
    const mhx_real* tp = r->target->dparams;
    int draw = init ? 0 : 1;
    const unsigned grid = grid1d(r->n, 256);
    if (r->jit_init) {
        int rc = launch_module(r->jit_init, grid, 256, ctx->stream, a, tp, draw);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(k_ram_init, dim3(grid), dim3(256), 0, ctx->stream, a, tp, draw);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MHX_OK;
}

#define MHX_RAM_MAX_STEPS_PER_LAUNCH 4096ull

static int ram_advance(mhx_run* r, uint64_t nsteps, uint64_t n_adapt, uint32_t save_next, int save_slot, int thinning)
{
    mhx_ctx* ctx = r->ctx;
    // The record of this call.  ram_pick_shape reads the option RAM_G, a call-time option: a pre-built kernel's record is filled
    // again at every call, from the shape picked NOW (r->step holds the one picked at create); a user target's module was compiled
    // for the shape picked at create and keeps that record.  A pad changes this call's copy alone, and has the kernel allowed the
    // padded size.
    launch_rec k = r->step;
    if (!k.mod_fn)
        if (int rcs = ram_step_record(r, nullptr, &k)) return rcs;
    if (const char* pad = opt(ctx, "RAM_LDS_PAD")) {                  // tuning knob: fewer resident waves per CU (DESIGN.md 6.3)
        k.lds += (size_t)atol(pad);
        if (k.lds > 65536 && !k.mod_fn)
            if (int rcl = kernel_lds_limit(k.fn, k.lds, k.what)) return rcl;
    }
    uint64_t done = 0;
    std::vector<mhx_real> eta;
    while (done < nsteps) {
        uint64_t chunk = std::min<uint64_t>(nsteps - done, MHX_RAM_MAX_STEPS_PER_LAUNCH);
        // watched chains: the launch ends AT the next recorded transition, so that the factors behind that sample can be copied out
        const bool watching = r->watch_n > 0 && save_next != MHX_NO_SAVE && (uint64_t)save_next > r->tau;
        if (watching) chunk = std::min<uint64_t>(chunk, (uint64_t)save_next - r->tau);
        const bool record_after = watching && r->tau + chunk == (uint64_t)save_next;
        const uint64_t adapt_here = done < n_adapt ? std::min<uint64_t>(n_adapt - done, chunk) : 0;
        if (adapt_here) {
            // eta = iteration^(-gamma)  (RAM.jl:162), iteration == RNG step counter of the transition
            eta.resize(adapt_here);
            for (uint64_t i = 0; i < adapt_here; ++i)
                eta[i] = (mhx_real)std::pow((double)(r->tau + 1 + i), -(double)(mhx_real)r->ramcfg.gamma);
            r->last_eta = (double)eta[adapt_here - 1];
            if (r->eta_cap < adapt_here) {
                if (r->d_eta) (void)hipFree(r->d_eta);
                r->d_eta = nullptr;
                HIP_TRY(hipMalloc(&r->d_eta, adapt_here * sizeof(mhx_real)));
                r->eta_cap = adapt_here;
            }
            // the previous launch may still read d_eta: order the copy on the same stream
            HIP_TRY(hipMemcpyAsync(r->d_eta, eta.data(), adapt_here * sizeof(mhx_real), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));   // `eta` (pageable host memory) is reused next chunk
        }
        mhx_ram_args a = ram_args(r);
        a.step0 = (uint32_t)(r->tau + 1);
        a.nsteps = (int)chunk;
        a.n_adapt = (int)adapt_here;
        a.save_next = save_next;
        a.save_slot = save_slot;
        a.thinning = thinning;
        if (int rcl = launch(k, ctx->stream, r->n, 1, &a)) return rcl;
        HIP_TRY(hipGetLastError());
        r->stats.launches++;
        if (record_after) { int rcw = ram_watch_record(r); if (rcw) return rcw; }
        save_cursor_skip(r, chunk, thinning, &save_next, &save_slot);
        r->tau += chunk;
        done += chunk;
    }
    return MHX_OK;
}
