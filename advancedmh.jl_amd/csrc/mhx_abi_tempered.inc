// the parallel-tempering entries of the C ABI (included at the end of mhx_abi.cpp; engine side: mhx_api_tempered.inc).  Like the
// pointwise entries they were never part of the hand-written dispatcher whose all-zero answers tests/golden/abi_null_contract.json
// records, so they stand apart from the 73 entries of that record; tests/test_tempered_cpu.py pins their guards.
extern "C" {

int mhx_rwmh_create_tempered(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_tempered_cfg* tcfg, mhx_run** out)
{
    NEED_SAME(rwmh_create_tempered, ctx, t, cfg, tcfg, out);
}

int mhx_rwmh_create_tempered_adaptive(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_tempered_cfg* tcfg,
                                      const mhx_ladder_adapt_cfg* acfg, mhx_run** out)
{
    NEED_SAME(rwmh_create_tempered_adaptive, ctx, t, cfg, tcfg, acfg, out);
}

int mhx_rwmh_create_tempered_anchored(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_tempered_cfg* tcfg,
                                      const mhx_tempered_reference* ref, mhx_run** out)
{
    NEED_SAME(rwmh_create_tempered_anchored, ctx, t, cfg, tcfg, ref, out);
}

int mhx_run_evidence(mhx_run* r, double* out, int64_t* n_saved) { NEED_SAMPLER(run_evidence, r, out, n_saved); }

int mhx_run_ladder_betas(mhx_run* r, double* beta) { NEED_SAMPLER(run_ladder_betas, r, beta); }

int mhx_run_swap_stats(mhx_run* r, uint64_t* attempts, uint64_t* swaps) { NEED_SAMPLER(run_swap_stats, r, attempts, swaps); }

int mhx_run_rung(mhx_run* r, int32_t rung, mhx_run** out) { NEED(run_rung, r, rung, out); }

}
