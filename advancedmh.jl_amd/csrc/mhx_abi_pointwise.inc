// the pointwise log-likelihood and PSIS-LOO entries of the C ABI (included at the end of mhx_abi.cpp; engine side: mhx_api_pointwise.inc).
// They were never part of the hand-written dispatcher whose all-zero answers tests/golden/abi_null_contract.json records, so they
// stand apart from the 73 entries of that record; tests/test_pointwise_cpu.py pins their guards.
extern "C" {

int mhx_run_pointwise(const mhx_run* src, const char* source, const void* rows, int64_t nrows, int32_t rowlen, const void* data, size_t ndata,
                      int32_t shift_given, double* shift, double* out5, int64_t* T)
{
    NEED(run_pointwise, src, source, rows, nrows, rowlen, data, ndata, shift_given, shift, out5, T);
}

int mhx_ctx_pointwise(mhx_ctx* ctx, const void* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const char* source, const void* rows,
                      int64_t nrows, int32_t rowlen, const void* data, size_t ndata, int32_t shift_given, double* shift, double* out5, int64_t* T)
{
    NEED(ctx_pointwise, ctx, d_tensor, n_samples, dim1, nchains, source, rows, nrows, rowlen, data, ndata, shift_given, shift, out5, T);
}

// PSIS-LOO (engine side: mhx_api_psis.inc); tests/test_psis_cpu.py pins the guards
int mhx_run_psis(const mhx_run* src, const char* source, const void* rows, int64_t nrows, int32_t rowlen, const void* data, size_t ndata,
                 double reff, double* out8, double* tail_out, int64_t* T, int64_t* M)
{
    NEED(run_psis, src, source, rows, nrows, rowlen, data, ndata, reff, out8, tail_out, T, M);
}

int mhx_ctx_psis(mhx_ctx* ctx, const void* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const char* source, const void* rows,
                 int64_t nrows, int32_t rowlen, const void* data, size_t ndata, double reff, double* out8, double* tail_out, int64_t* T, int64_t* M)
{
    NEED(ctx_psis, ctx, d_tensor, n_samples, dim1, nchains, source, rows, nrows, rowlen, data, ndata, reff, out8, tail_out, T, M);
}

}
