// the log evidence of an anchored tempered run, host side (included by mhx_api.hip after mhx_api_tempered.inc): the checks, the grid of
// the pointwise frame (pointwise_sweep_plan), the scratch for partials and table, two launches -- sweep, merge -- and one copy back
// (mhx_evidence_kernels.h, DESIGN.md section 6.5.9)

__global__ void __launch_bounds__(MHX_POINTWISE_THREADS)
k_evidence_sweep(const mhx_real* __restrict__ src, const long N, const long C, const int d, const int R, const mhx_tmp_anchor an,
                 const mhx_real* __restrict__ dbeta, double* __restrict__ part)
{
    mhx_evidence_sweep_body(src, N, C, d, R, an, dbeta, part);
}
__global__ void __launch_bounds__(256)
k_evidence_merge(const double* __restrict__ part, const long slots, const long C, double* __restrict__ out)
{
    mhx_evidence_merge_body(part, slots, C, out);
}

// out [nchains][8]: bad, shift, s1, s2, max_f, sumexp_f, max_b, sumexp_b of every chain.  Nothing is written unless the call succeeds.
int api_run_evidence(mhx_run* r, double* out, int64_t* n_saved)
{
    const char* who = "mhx_run_evidence";
    if (!r || !out) return mhx_fail(MHX_EINVAL, "%s: NULL argument", who);
    if (!r->tmp_anchor)
        return mhx_fail(MHX_ESTATE, "%s: not an anchored tempered run (mhx_rwmh_create_tempered_anchored): without a normalised reference "
                                    "the path from beta = 1 ends at a density of unknown normaliser", who);
    draws_view v;
    int rc = draws_of_run(who, r, &v);
    if (rc) return rc;
    if (!r->tmp_beta_end_zero)
        return mhx_fail(MHX_ESTATE, "%s: the ladder's last beta is not 0 -- the path must reach the reference itself for its integral to be the "
                                    "evidence", who);
    if (v.C > 0x7fffffffl || v.N > 0x7fffffffl) return mhx_fail(MHX_EINVAL, "%s: %ld saved draws of %ld chains: each is counted in 31 bits", who, v.N, v.C);
    mhx_ctx* ctx = v.ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const sweep_plan g = pointwise_sweep_plan(v, 1);
    const size_t C = (size_t)v.C, K = MHX_EVIDENCE_FIELDS;
    double *d_part = nullptr, *d_out = nullptr;
    rc = scratch_carve(&ctx->select_scratch, &ctx->select_bytes, who, "evidence scratch", [&](scratch_pieces& c) {
        d_part = c.take<double>((size_t)g.slots * K * C);
        d_out = c.take<double>(C * K);
    });
    if (rc) { (void)hipGetLastError(); return rc; }
    hipLaunchKernelGGL(k_evidence_sweep, dim3((unsigned)g.ncb, (unsigned)g.slots), dim3(MHX_POINTWISE_THREADS), 0, ctx->stream, v.tensor, v.N, v.C,
                       v.d1 - 1, r->tmp_R, r->tmp_an, (const mhx_real*)(r->d_ttab + r->tmp_R), d_part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_evidence_merge, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, ctx->stream, d_part, g.slots, v.C, d_out);
    HIP_TRY(hipGetLastError());
    std::vector<double> land(C * K);                        // written to the caller only after the sync
    HIP_TRY(hipMemcpyAsync(land.data(), d_out, C * K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(out, land.data(), C * K * sizeof(double));
    if (n_saved) *n_saved = (int64_t)v.N;
    return MHX_OK;
}
