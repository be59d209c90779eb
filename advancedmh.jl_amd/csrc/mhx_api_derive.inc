// derived quantities and predictive draws host side (included by mhx_api.hip after mhx_api_acf.inc): the checks, the run-time module
// of the map (user_module), the derived run and its tensor, one launch (mhx_derive_kernels.h, DESIGN.md sections 6.5.5 and 6.5.6)

// The outputs of the draws a lane maps together stay in registers until they are stored: (nout + 1) reals per draw.  More than this
// many outputs are refused; up to it the draws per lane shrink so that the outputs stay within about a quarter of the register file.
#define MHX_DERIVE_MAX_NOUT 128
// draws a lane maps together where the outputs allow it: DESIGN.md section 7 has the measurement; option DERIVE_DRAWS picks another
#define MHX_DERIVE_DRAWS 4

// Draws a lane of a PREDICTIVE map maps together: 1, from the cross-compiled resource usage (DESIGN.md section 6.5.6 has the table).
// The frame unrolls the map once per draw of the group to have their row loads in flight together; a generator call is some hundred
// dependent VALU instructions per output, which the other waves of the SIMD cover, and each further draw costs registers and a copy
// of every attempt loop: the test map with two Gamma draws is 1788 instructions, 131 VGPRs and 3 waves per SIMD at 1 in fp64, 4901 /
// 155 / 3 at 2, 7823 / 192 / 2 at 4.  Option DERIVE_DRAWS picks another, within the same register cap.
#define MHX_PREDICT_DRAWS 1

// what differs between the two kinds of map: the name the compiler knows the caller's text by, the frame's define and entry, the
// default draws per lane -- and, where `rng`, two more kernel arguments and the limit on n_saved
struct derive_kind {
    const char* file;
    const char* have;
    const char* entry;
    int draws;
    bool rng;
};
static const derive_kind k_derived = {"derived.hip", "MHX_HAVE_DERIVED", "mhx_jit_derive", MHX_DERIVE_DRAWS, false};
static const derive_kind k_predictive = {"predictive.hip", "MHX_HAVE_PREDICTIVE", "mhx_jit_predict", MHX_PREDICT_DRAWS, true};

static int derive_draws_per_lane(const mhx_ctx* ctx, const derive_kind& kind, int nout)
{
    const int asked = opt_int(ctx, "DERIVE_DRAWS", 0);
    const int fit = std::max(1, 128 / ((nout + 1) * (MHX_REAL64 ? 2 : 1)));
    return std::min(asked >= 1 && asked <= 16 ? asked : kind.draws, fit);           // (the option never lifts the register cap)
}

// v is checked, nothing else is.  Nothing is left behind unless the call succeeds: the run and its tensor are owned here until then.
// seed: the predictive streams' (a derived map has none); the run that is made inherits v's seed and first_id either way.
static int derive_checked(const draws_view& v, const derive_kind& kind, const char* source, int32_t nout, const mhx_real* data, size_t ndata,
                          uint64_t seed, mhx_run** out)
{
    const char* who = v.who;
    mhx_ctx* ctx = v.ctx;
    if (!source || !out) return mhx_fail(MHX_EINVAL, "%s: NULL argument", who);
    if (nout < 1) return mhx_fail(MHX_EINVAL, "%s: nout = %d, a map has at least one output", who, (int)nout);
    if (nout > MHX_DERIVE_MAX_NOUT)
        return mhx_fail(MHX_EINVAL, "%s: nout = %d, at most %d outputs per map (they are held in registers): split the map", who, (int)nout,
                        MHX_DERIVE_MAX_NOUT);
    if (int rc = data_block_checked(who, data, ndata)) return rc;
    if (v.C > 0x7fffffffl) return mhx_fail(MHX_EINVAL, "%s: %ld chains, a run holds fewer than 2^31", who, v.C);
    if (kind.rng && (unsigned long long)v.N > (1ull << 32))
        return mhx_fail(MHX_EINVAL, "%s: %ld saved draws, a predictive map numbers them in 32 bits (at most 2^32)", who, v.N);
    HIP_TRY(hipSetDevice(ctx->device));
    const int U = derive_draws_per_lane(ctx, kind, nout);
    hipFunction_t fn = nullptr;
    int rc = user_module(v, kind.file, "map", source, {{kind.have, "mhx_derive_kernels.h"}},
                         {"MHX_JIT_DERIVE_NOUT=" + std::to_string(nout), "MHX_JIT_DERIVE_DRAWS=" + std::to_string(U)}, {{kind.entry, &fn}});
    if (rc) return rc;
    std::unique_ptr<mhx_run> r(new mhx_run);
    r->dtype = ctx->dtype;
    r->ctx = ctx;
    r->kind = RUN_DERIVED;
    r->dim = nout;
    r->n = (int)v.C;
    r->seed = v.seed;
    r->first_id = v.first_id;
    const size_t bytes = (size_t)v.N * ((size_t)nout + 1) * (size_t)v.C * sizeof(mhx_real);
    rc = ensure_buffer((void**)&r->d_samples, &r->samples_cap, bytes, who, "derived sample tensor");
    if (rc) { (void)hipGetLastError(); return rc; }
    dev_array<mhx_real> d_data;
    if (!d_data.alloc(data_block_reals(ndata))) {
        (void)hipGetLastError();
        return mhx_fail(MHX_ENOMEM, "%s: %zu bytes of data block", who, ndata * sizeof(mhx_real));
    }
    if ((rc = data_block_upload(ctx, d_data.p, data, ndata))) return rc;
    const long strip = (long)U * MHX_DERIVE_ROUNDS, nstrips = (v.N + strip - 1) / strip;
    const dim3 grid((unsigned)((v.C + MHX_DERIVE_THREADS - 1) / MHX_DERIVE_THREADS), (unsigned)std::min(nstrips, 65535l));
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    // (mhx_jit_derive takes the first seven arguments, mhx_jit_predict the seed of its streams and the first chain's id as well)
    rc = launch_module(fn, grid, MHX_DERIVE_THREADS, ctx->stream, v.tensor, r->d_samples, v.N, v.C, v.d1 - 1, d_data.p, (int)ndata,
                       (unsigned long long)seed, (unsigned long long)v.first_id);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    r->n_saved = v.N;
    r->stats.kernel_ms = ms;                                // the map's launch; no transitions, no accepts
    r->stats.kernel_variant = -1;                           // none of enum kernel_form: mhx_run_form_name says "derived"
    r->stats.launches = 1;
    r->stats.dtype = r->dtype;
    r->stats.factor_band = -1;
    *out = r.release();
    return MHX_OK;
}

int api_ctx_derive(mhx_ctx* ctx, const mhx_real* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const char* source, int32_t nout,
                   const mhx_real* data, size_t ndata, mhx_run** out)
{
    draws_view v;
    int rc = draws_of_ctx("mhx_ctx_derive", ctx, d_tensor, n_samples, dim1, nchains, &v);
    return rc ? rc : derive_checked(v, k_derived, source, nout, data, ndata, 0, out);
}

int api_run_derive(const mhx_run* src, const char* source, int32_t nout, const mhx_real* data, size_t ndata, mhx_run** out)
{
    draws_view v;
    int rc = draws_of_run("mhx_run_derive", src, &v);
    return rc ? rc : derive_checked(v, k_derived, source, nout, data, ndata, 0, out);
}

int api_ctx_predict(mhx_ctx* ctx, const mhx_real* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, int64_t first_chain,
                    const char* source, int32_t nout, const mhx_real* data, size_t ndata, uint64_t seed, mhx_run** out)
{
    draws_view v;
    int rc = draws_of_ctx("mhx_ctx_predict", ctx, d_tensor, n_samples, dim1, nchains, &v);
    if (rc) return rc;
    v.seed = seed;                                          // (a caller's tensor has no run to inherit from)
    v.first_id = (uint64_t)first_chain;
    return derive_checked(v, k_predictive, source, nout, data, ndata, seed, out);
}

int api_run_predict(const mhx_run* src, const char* source, int32_t nout, const mhx_real* data, size_t ndata, uint64_t seed, mhx_run** out)
{
    draws_view v;
    int rc = draws_of_run("mhx_run_predict", src, &v);
    return rc ? rc : derive_checked(v, k_predictive, source, nout, data, ndata, seed, out);
}
