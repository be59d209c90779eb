// mhx_impl.h -- the two instantiations of the engine behind the C ABI.
//
// libmhx.so holds the engine twice: namespace mhx_f32 (mhx_real = float) and namespace mhx_f64 (mhx_real = double; the
// reference computes in Float64), both compiled from mhx_api.hip + the kernel headers.  The public entry points of
// include/mhx.h live in mhx_abi.cpp and forward to the instantiation the handle belongs to (the first word of every
// handle is its mhx_dtype).  This header declares the api_* functions of both, so that definitions (mhx_api.hip) and
// calls (mhx_abi.cpp) are checked against ONE set of prototypes by the C++ linker (mangled names carry the types).
// mhx_abi.cpp's forwarder reads each parameter type off these prototypes: an api_* function takes the public entry's
// parameters in order and in the public types (int64_t, not long), handles and real buffers as the namespace's own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mhx.h"

// thread-local error message shared by everything in the library (mhx_last_error); returns `code`
int mhx_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

struct mhx_handle_hdr { int32_t dtype; };

// hiprtc is entered by one thread at a time (the member threads of a group may each need a specialisation): mhx_abi.cpp
void mhx_jit_lock();
void mhx_jit_unlock();

#define MHX_IMPL_DECLARE(NS, REAL)                                                                                     \
    namespace NS {                                                                                                     \
    struct mhx_ctx;                                                                                                    \
    struct mhx_target;                                                                                                 \
    struct mhx_run;                                                                                                    \
    int api_ctx_create(int device, mhx_ctx** out);                                                                     \
    int api_ctx_destroy(mhx_ctx* ctx);                                                                                 \
    int api_ctx_device(const mhx_ctx* ctx);                                                                            \
    int api_ctx_set_option(mhx_ctx* ctx, const char* name, const char* value);                                         \
    int api_ctx_get_option(const mhx_ctx* ctx, const char* name, char* buf, size_t len);                               \
    int api_ctx_pci_bus_id(const mhx_ctx* ctx, char* buf, size_t len);                                                 \
    int api_run_shape(const mhx_run* r, int32_t* dim, int32_t* nchains);                                               \
    int api_ctx_jit_counts(const mhx_ctx* ctx, int64_t* compiles, int64_t* cache_hits);                                \
    int api_ctx_jit_compiler(const mhx_ctx* ctx, char* compiler, size_t len, int64_t* ext_compiles);                   \
    int api_ctx_host_pin_counts(const mhx_ctx* ctx, int64_t* registered, int64_t* released);                           \
    int api_target_builtin(mhx_ctx* ctx, int kind, int dim, const REAL* params, size_t nparams, mhx_target** out);     \
    int api_target_from_hip_source(mhx_ctx* ctx, const char* src, int dim, const REAL* data, size_t ndata,             \
                                   mhx_target** out);                                                                  \
    int api_target_destroy(mhx_target* t);                                                                             \
    int api_target_eval(mhx_ctx* ctx, const mhx_target* t, const REAL* x, int n, REAL* lp);                            \
    int api_rwmh_create(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, mhx_run** out);                    \
    int api_rwmh_create_components(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg,                         \
                                   const mhx_proposal_component* comps, int32_t ncomps, mhx_run** out);                \
    int api_rwmh_create_conditional(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg,                        \
                                    const mhx_proposal_component* comps, int32_t ncomps, const char* params_src,       \
                                    const REAL* data, size_t ndata, mhx_run** out);                                    \
    int api_rwmh_create_composite(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg,                          \
                                  const mhx_proposal_component* comps, int32_t ncomps, const mhx_proposal_block* blocks, \
                                  int32_t nblocks, const int32_t* mapped, const char* params_src, const REAL* data,     \
                                  size_t ndata, mhx_run** out);                                                        \
    int api_emcee_create(mhx_ctx* ctx, const mhx_target* t, const mhx_emcee_cfg* cfg, mhx_run** out);                  \
    int api_ram_create(mhx_ctx* ctx, const mhx_target* t, const mhx_ram_cfg* cfg, mhx_run** out);                      \
    int api_mala_create(mhx_ctx* ctx, const mhx_target* t, const mhx_mala_cfg* cfg, mhx_run** out);                    \
    int api_ram_set_factor(mhx_run* r, const REAL* S);                                                                 \
    int api_ram_set_factor_all(mhx_run* r, const REAL* S);                                                             \
    int api_ram_get_factor(mhx_run* r, REAL* S, uint8_t* status);                                                      \
    int api_ram_get_diag_range(mhx_run* r, REAL* diag_min, REAL* diag_max);                                            \
    int api_ram_get_adapt_state(mhx_run* r, REAL* log_alpha, double* eta, uint8_t* isaccept, uint64_t* iteration);     \
    int api_ram_get_step_stats(mhx_run* r, REAL* log_alpha, double* eta, int64_t capacity, int64_t* n_recorded);       \
    int api_ram_watch_factors(mhx_run* r, const int32_t* chains, int n);                                               \
    int api_ram_get_watched_factors(mhx_run* r, REAL* S, int64_t capacity, int64_t* n_recorded, int32_t* n_watched);   \
    int api_run_init(mhx_run* r, const REAL* initial_params);                                                          \
    int api_run_sample(mhx_run* r, const mhx_schedule* s, int save_samples);                                           \
    int api_run_get_samples(mhx_run* r, REAL* samples, uint8_t* accepted);                                             \
    int api_run_sample_to_host(mhx_run* r, const mhx_schedule* s, REAL* samples, uint8_t* accepted, int slab_samples);  \
    int api_run_device_samples(mhx_run* r, void** samples, void** accepted, int64_t* n_samples);                       \
    int api_run_get_state(mhx_run* r, REAL* x, REAL* lp, uint32_t* accept_counts);                                     \
    int api_run_set_state(mhx_run* r, const REAL* x);                                                                  \
    int api_run_state_size(mhx_run* r, size_t* bytes);                                                                 \
    int api_run_save_state(mhx_run* r, void* blob, size_t bytes);                                                      \
    int api_run_load_state(mhx_run* r, const void* blob, size_t bytes);                                                \
    int api_run_stats(mhx_run* r, mhx_stats* out);                                                                     \
    const char* api_run_form_name(const mhx_run* r);                                                                   \
    int api_run_host_stats(mhx_run* r, mhx_host_stats* out);                                                           \
    int api_run_destroy(mhx_run* r);                                                                                   \
    int api_run_diagnostics(mhx_run* r, const mhx_diag_cfg* cfg, double* sum_m, double* sum_m2, double* sum_v,         \
                            double* ess);                                                                              \
    int api_run_ess_bulk_tail(mhx_run* r, const mhx_diag_cfg* cfg, const int32_t* params, int32_t nparams,             \
                              double* ess_bulk, double* ess_tail);                                                     \
    int api_run_rank_diagnostics(mhx_run* r, const mhx_diag_cfg* cfg, const int32_t* params, int32_t nparams,          \
                                 double* ess_bulk, double* ess_tail, double* rhat_bulk, double* rhat_tail);            \
    int api_run_rank_scores(mhx_run* r, int32_t param, int32_t folded, REAL* out_host);                                \
    int api_ctx_order_statistics(mhx_ctx* ctx, const REAL* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,   \
                                 const int32_t* params, int32_t nparams, const int64_t* ranks, int32_t nranks,         \
                                 double* out);                                                                         \
    int api_run_order_statistics(mhx_run* r, const int32_t* params, int32_t nparams, const int64_t* ranks,             \
                                 int32_t nranks, double* out);                                                         \
    int api_run_select_histogram(mhx_run* r, const int32_t* params, int32_t nparams, const uint64_t* prefixes,         \
                                 const int32_t* ngroups, int32_t gstride, int32_t shift, int32_t digit_bits,           \
                                 uint64_t* hist);                                                                      \
    int api_ctx_cross_moments(mhx_ctx* ctx, const REAL* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,    \
                              const int32_t* params, int32_t nparams, const double* shift, double* sum, double* cross);  \
    int api_run_cross_moments(mhx_run* r, const int32_t* params, int32_t nparams, const double* shift, double* sum,    \
                              double* cross, int64_t* n_draws);                                                        \
    int api_ctx_hpd(mhx_ctx* ctx, const REAL* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,              \
                    const int32_t* params, int32_t nparams, double alpha, double* lower, double* upper);               \
    int api_run_hpd(mhx_run* r, const int32_t* params, int32_t nparams, double alpha, double* lower, double* upper);   \
    int api_ctx_histogram(mhx_ctx* ctx, const REAL* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,        \
                          const int32_t* params, int32_t nparams, const double* edges, int32_t nbins, uint64_t* counts, \
                          uint64_t* outside);                                                                          \
    int api_run_histogram(mhx_run* r, const int32_t* params, int32_t nparams, const double* edges, int32_t nbins,      \
                          uint64_t* counts, uint64_t* outside);                                                        \
    int api_ctx_histogram2d(mhx_ctx* ctx, const REAL* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,      \
                            const int32_t* params, int32_t nparams, const double* edges, int32_t nbins,                \
                            const int32_t* pairs, int32_t npairs, uint64_t* counts, uint64_t* outside);                \
    int api_run_histogram2d(mhx_run* r, const int32_t* params, int32_t nparams, const double* edges, int32_t nbins,    \
                            const int32_t* pairs, int32_t npairs, uint64_t* counts, uint64_t* outside);                \
    int api_ctx_autocovariance(mhx_ctx* ctx, const REAL* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,   \
                               const int32_t* params, int32_t nparams, const int32_t* lags, int32_t nlags,             \
                               int64_t chain_begin, int64_t chain_count, int32_t normalise, double* acov,              \
                               int64_t* nvalid);                                                                       \
    int api_run_autocovariance(mhx_run* r, const int32_t* params, int32_t nparams, const int32_t* lags, int32_t nlags, \
                               int64_t chain_begin, int64_t chain_count, int32_t normalise, double* acov,              \
                               int64_t* nvalid);                                                                       \
    int api_run_derive(const mhx_run* src, const char* source, int32_t nout, const REAL* data, size_t ndata,           \
                       mhx_run** out);                                                                                 \
    int api_ctx_derive(mhx_ctx* ctx, const REAL* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,           \
                       const char* source, int32_t nout, const REAL* data, size_t ndata, mhx_run** out);               \
    int api_run_predict(const mhx_run* src, const char* source, int32_t nout, const REAL* data, size_t ndata,          \
                        uint64_t seed, mhx_run** out);                                                                 \
    int api_ctx_predict(mhx_ctx* ctx, const REAL* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,          \
                        int64_t first_chain, const char* source, int32_t nout, const REAL* data, size_t ndata,         \
                        uint64_t seed, mhx_run** out);                                                                 \
    int api_run_pointwise(const mhx_run* src, const char* source, const REAL* rows, int64_t nrows, int32_t rowlen,     \
                          const REAL* data, size_t ndata, int32_t shift_given, double* shift, double* out5, int64_t* T); \
    int api_ctx_pointwise(mhx_ctx* ctx, const REAL* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,        \
                          const char* source, const REAL* rows, int64_t nrows, int32_t rowlen, const REAL* data,       \
                          size_t ndata, int32_t shift_given, double* shift, double* out5, int64_t* T);                 \
    int api_run_psis(const mhx_run* src, const char* source, const REAL* rows, int64_t nrows, int32_t rowlen,          \
                     const REAL* data, size_t ndata, double reff, double* out8, double* tail_out, int64_t* T,          \
                     int64_t* M);                                                                                      \
    int api_ctx_psis(mhx_ctx* ctx, const REAL* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,             \
                     const char* source, const REAL* rows, int64_t nrows, int32_t rowlen, const REAL* data,            \
                     size_t ndata, double reff, double* out8, double* tail_out, int64_t* T, int64_t* M);               \
    bool api_run_is_derived(const mhx_run* r);                                                                         \
    int api_rwmh_create_tempered(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg,                          \
                                 const mhx_tempered_cfg* tcfg, mhx_run** out);                                        \
    int api_rwmh_create_tempered_adaptive(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg,                 \
                                          const mhx_tempered_cfg* tcfg, const mhx_ladder_adapt_cfg* acfg,             \
                                          mhx_run** out);                                                             \
    int api_rwmh_create_tempered_anchored(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg,                 \
                                          const mhx_tempered_cfg* tcfg, const mhx_tempered_reference* ref,            \
                                          mhx_run** out);                                                             \
    int api_run_evidence(mhx_run* r, double* out, int64_t* n_saved);                                                  \
    int api_run_ladder_betas(mhx_run* r, double* beta);                                                               \
    int api_run_swap_stats(mhx_run* r, uint64_t* attempts, uint64_t* swaps);                                          \
    int api_run_rung(mhx_run* src, int32_t rung, mhx_run** out);                                                      \
    int api_rwmh_create_adaptive(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg,                          \
                                 const mhx_proposal_adapt_cfg* acfg, mhx_run** out);                                  \
    int api_run_proposal_state(mhx_run* r, double* lam, double* sd, double* mean, uint32_t* acc_at_freeze);           \
    int api_emcee_half_step(mhx_run* r, int half, int begin, int count);                                               \
    int api_emcee_end_sweep(mhx_run* r);                                                                               \
    int api_emcee_device_state(mhx_run* r, REAL** xw, int32_t* pitch, REAL** lp, uint32_t** acc_count,                 \
                               uint8_t** last_acc);                                                                    \
    int api_emcee_exchange_plan(mhx_run* r, int half, int world, size_t* stride, void** stream);                       \
    int api_emcee_exchange_pack(mhx_run* r, int half, int rank, int world, void* part);                                \
    int api_emcee_exchange_unpack(mhx_run* r, int half, int rank, int world, const void* stage, size_t stride);        \
    }

MHX_IMPL_DECLARE(mhx_f32, float)
MHX_IMPL_DECLARE(mhx_f64, double)
