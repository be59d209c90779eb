// the adaptive random walk's entries of the C ABI (included at the end of mhx_abi.cpp; engine side: mhx_api_adaptive.inc).  Like the
// tempering entries they stand apart from the 73 entries tests/golden/abi_null_contract.json records; tests/test_adaptive_rwmh_cpu.py
// pins their guards.
extern "C" {

int mhx_rwmh_create_adaptive(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_proposal_adapt_cfg* acfg, mhx_run** out)
{
    NEED_SAME(rwmh_create_adaptive, ctx, t, cfg, acfg, out);
}

int mhx_run_proposal_state(mhx_run* r, double* lam, double* sd, double* mean, uint32_t* acc_at_freeze)
{
    NEED_SAMPLER(run_proposal_state, r, lam, sd, mean, acc_at_freeze);
}

}
