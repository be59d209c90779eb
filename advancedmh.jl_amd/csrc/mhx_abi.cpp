// mhx_abi.cpp -- the C ABI of include/mhx.h: every entry point forwards to the instantiation of the engine the handle
// belongs to (namespace mhx_f32: mhx_real = float, namespace mhx_f64: mhx_real = double; mhx_impl.h).  The first word
// of every handle is its mhx_dtype.  No device code here.
#include "mhx_impl.h"
#include "mhx_host_expand.h"    // mhx_numa_*: placement of page-locked result memory

#include <hip/hip_runtime_api.h>   // hipHostMalloc / hipHostFree only (mhx_host_alloc): no device code here

#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <string>
#include <type_traits>

static thread_local std::string g_err;
static std::mutex g_jit_mu;
void mhx_jit_lock() { g_jit_mu.lock(); }
void mhx_jit_unlock() { g_jit_mu.unlock(); }

int mhx_fail(int code, const char* fmt, ...)
{
    char buf[2048];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" int mhx_version(void) { return MHX_VERSION; }
extern "C" const char* mhx_last_error(void) { return g_err.c_str(); }

// ---- the forwarder ------------------------------------------------------------------------------------------------------
// call<W>(engine function, public arguments...) takes the parameter types from the engine function's own type and converts each
// public argument to its parameter by a closed set of rules; anything else does not compile:
//   the same type                                       passed through (scalars, structs of the header, char*, void* blobs, ...)
//   T*, const T*, T** for T = mhx_ctx, mhx_target, mhx_run   the same pointer to the namespace's handle
//   void*, const void*, void**                          REAL*, const REAL*, REAL**: the buffers "of the context's dtype"
struct w32 { using real = float;  using ctx = mhx_f32::mhx_ctx; using target = mhx_f32::mhx_target; using run = mhx_f32::mhx_run; };
struct w64 { using real = double; using ctx = mhx_f64::mhx_ctx; using target = mhx_f64::mhx_target; using run = mhx_f64::mhx_run; };

struct no_rule;
template <class W, class T> struct engine_of { using type = no_rule; };
template <class W> struct engine_of<W, void> { using type = typename W::real; };
template <class W> struct engine_of<W, ::mhx_ctx> { using type = typename W::ctx; };
template <class W> struct engine_of<W, ::mhx_target> { using type = typename W::target; };
template <class W> struct engine_of<W, ::mhx_run> { using type = typename W::run; };

template <class W, class A> struct converted { using type = no_rule; };
template <class W, class T> struct converted<W, T*> { using type = typename engine_of<W, T>::type*; };
template <class W, class T> struct converted<W, const T*> { using type = const typename engine_of<W, T>::type*; };
template <class W, class T> struct converted<W, T**> { using type = typename engine_of<W, T>::type**; };

template <class W, class P, class A> static inline P pass(A a)
{
    if constexpr (std::is_same_v<P, A>) return a;
    else {
        static_assert(std::is_same_v<P, typename converted<W, A>::type>, "mhx_abi: no rule converts this public argument to the engine's parameter");
        return reinterpret_cast<P>(a);
    }
}
template <class W, class R, class... P, class... A> static inline R call(R (*fn)(P...), A... a)
{
    static_assert(sizeof...(P) == sizeof...(A), "mhx_abi: the engine function takes another number of arguments");
    return fn(pass<W, P, A>(a)...);
}

static inline bool is64(const void* h) { return reinterpret_cast<const mhx_handle_hdr*>(h)->dtype == MHX_F64; }
// same dtype for every handle of a call (a target built on an fp32 context cannot serve an fp64 run)
template <class... A> static inline bool same(const void* a, const void* b, A...) { return !a || !b || is64(a) == is64(b); }
template <class H, class... A> static inline H first(H h, A...) { return h; }

// the one place that picks the instantiation: api_<fn> of the namespace, named once; FWD's first argument is the handle that decides
#define DISPATCH(f64, fn, ...) ((f64) ? call<w64>(&mhx_f64::api_##fn, __VA_ARGS__) : call<w32>(&mhx_f32::api_##fn, __VA_ARGS__))
#define FWD(fn, ...) DISPATCH(is64(first(__VA_ARGS__)), fn, __VA_ARGS__)

// The one guard of the entry points that step, initialise, set, save or load state, or read sampler state: a derived run
// (mhx_run_derive) holds a sample tensor and nothing else.  Which entry is on which list: include/mhx.h at mhx_run_derive.
static int refuse_derived(const mhx_run* r, const char* name)
{
    if (!FWD(run_is_derived, r)) return MHX_OK;
    return mhx_fail(MHX_ESTATE, "%s: the run is a derived run (mhx_run_derive): it holds a sample tensor and no sampler state", name);
}

// ---- the guards ---------------------------------------------------------------------------------------------------------
// The body of an entry point is ONE of these: the guard, then mhx_<fn>'s arguments forwarded to api_<fn>, the handle first.
//   NULL_OK       a NULL handle is MHX_OK: the destroys
//   NEED          the handle must not be NULL ("handle is NULL"; NEED_CTX: the same guard where the text reads "ctx is NULL")
//   NEED_SAMPLER  NEED, then a derived run is refused before anything else is looked at: the "refuse" list of include/mhx.h
//   NEED_SAME     NEED, then context and target must be of one dtype
// The few entries that are not of this shape (mhx_ctx_create, _dtype, _device, mhx_run_form_name, mhx_host_*) are written out.
#define REFUSE_NULL(fn, what, ...) if (!first(__VA_ARGS__)) return mhx_fail(MHX_EINVAL, "mhx_" #fn ": " what " is NULL")
#define NULL_OK(fn, ...)      if (!first(__VA_ARGS__)) return MHX_OK; return FWD(fn, __VA_ARGS__)
#define NEED(fn, ...)         REFUSE_NULL(fn, "handle", __VA_ARGS__); return FWD(fn, __VA_ARGS__)
#define NEED_CTX(fn, ...)     REFUSE_NULL(fn, "ctx", __VA_ARGS__); return FWD(fn, __VA_ARGS__)
#define NEED_SAMPLER(fn, ...) REFUSE_NULL(fn, "handle", __VA_ARGS__); if (int rc_ = refuse_derived(first(__VA_ARGS__), "mhx_" #fn)) return rc_; return FWD(fn, __VA_ARGS__)
#define NEED_SAME(fn, ...)    REFUSE_NULL(fn, "handle", __VA_ARGS__); if (!same(__VA_ARGS__)) return mhx_fail(MHX_EINVAL, "mhx_" #fn ": the handles belong to contexts of different dtype"); return FWD(fn, __VA_ARGS__)

extern "C" int mhx_ctx_create(int device, int dtype, mhx_ctx** out)
{
    if (!out) return mhx_fail(MHX_EINVAL, "mhx_ctx_create: out is NULL");
    if (dtype != MHX_F32 && dtype != MHX_F64) return mhx_fail(MHX_EINVAL, "mhx_ctx_create: dtype must be MHX_F32 (0) or MHX_F64 (1), got %d", dtype);
    return DISPATCH(dtype == MHX_F64, ctx_create, device, out);
}
extern "C" int mhx_ctx_dtype(const mhx_ctx* ctx)
{
    REFUSE_NULL(ctx_dtype, "ctx", ctx);
    return is64(ctx) ? MHX_F64 : MHX_F32;
}
extern "C" int mhx_ctx_device(const mhx_ctx* ctx, int* device)
{
    if (!ctx || !device) return mhx_fail(MHX_EINVAL, "mhx_ctx_device: NULL argument");
    *device = FWD(ctx_device, ctx);
    return MHX_OK;
}
extern "C" int mhx_ctx_set_option(mhx_ctx* ctx, const char* name, const char* value) { NEED(ctx_set_option, ctx, name, value); }
extern "C" int mhx_ctx_get_option(const mhx_ctx* ctx, const char* name, char* buf, size_t len) { NEED(ctx_get_option, ctx, name, buf, len); }
extern "C" int mhx_ctx_pci_bus_id(const mhx_ctx* ctx, char* buf, size_t len) { NEED(ctx_pci_bus_id, ctx, buf, len); }
extern "C" int mhx_ctx_jit_counts(const mhx_ctx* ctx, int64_t* compiles, int64_t* cache_hits) { NEED_CTX(ctx_jit_counts, ctx, compiles, cache_hits); }
extern "C" int mhx_ctx_jit_compiler(const mhx_ctx* ctx, char* compiler, size_t len, int64_t* ext_compiles)
{
    NEED_CTX(ctx_jit_compiler, ctx, compiler, len, ext_compiles);
}
extern "C" int mhx_ctx_host_pin_counts(const mhx_ctx* ctx, int64_t* registered, int64_t* released)
{
    NEED_CTX(ctx_host_pin_counts, ctx, registered, released);
}
extern "C" int mhx_host_alloc(size_t bytes, void** out)
{
    if (!out) return mhx_fail(MHX_EINVAL, "mhx_host_alloc: out is NULL");
    *out = nullptr;
    if (!bytes) return MHX_OK;
    // on the memory node of the calling thread's current device: what fills a result tensor -- the GPU's DMA engine, or the host
    // threads that expand accept-compacted blocks, which keep to that node -- then works on local memory
    int dev = 0, node = -1;
    char bus[32] = {0};
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetPCIBusId(bus, (int)sizeof bus, dev) == hipSuccess) node = mhx_numa_node_of_pci(bus);
    else (void)hipGetLastError();
    if (node >= 0) mhx_numa_prefer(node);
    hipError_t e = hipHostMalloc(out, bytes, node >= 0 ? hipHostMallocNumaUser : hipHostMallocDefault);
    if (node >= 0) mhx_numa_default();
    if (e != hipSuccess) {
        *out = nullptr;
        return mhx_fail(MHX_ENOMEM, "mhx_host_alloc: %zu page-locked bytes: %s", bytes, hipGetErrorString(e));
    }
    return MHX_OK;
}
extern "C" int mhx_host_free(void* p)
{
    if (!p) return MHX_OK;
    hipError_t e = hipHostFree(p);
    return e == hipSuccess ? MHX_OK : mhx_fail(MHX_EHIP, "mhx_host_free: %s", hipGetErrorString(e));
}
extern "C" int mhx_ctx_destroy(mhx_ctx* ctx) { NULL_OK(ctx_destroy, ctx); }

extern "C" int mhx_target_builtin(mhx_ctx* ctx, int kind, int dim, const void* params, size_t nparams, mhx_target** out)
{
    NEED(target_builtin, ctx, kind, dim, params, nparams, out);
}
extern "C" int mhx_target_from_hip_source(mhx_ctx* ctx, const char* src, int dim, const void* data, size_t ndata, mhx_target** out)
{
    NEED(target_from_hip_source, ctx, src, dim, data, ndata, out);
}
extern "C" int mhx_target_destroy(mhx_target* t) { NULL_OK(target_destroy, t); }
extern "C" int mhx_target_eval(mhx_ctx* ctx, const mhx_target* t, const void* x, int n, void* lp) { NEED_SAME(target_eval, ctx, t, x, n, lp); }

extern "C" int mhx_rwmh_create(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, mhx_run** out) { NEED_SAME(rwmh_create, ctx, t, cfg, out); }
extern "C" int mhx_emcee_create(mhx_ctx* ctx, const mhx_target* t, const mhx_emcee_cfg* cfg, mhx_run** out) { NEED_SAME(emcee_create, ctx, t, cfg, out); }
extern "C" int mhx_ram_create(mhx_ctx* ctx, const mhx_target* t, const mhx_ram_cfg* cfg, mhx_run** out) { NEED_SAME(ram_create, ctx, t, cfg, out); }
extern "C" int mhx_mala_create(mhx_ctx* ctx, const mhx_target* t, const mhx_mala_cfg* cfg, mhx_run** out) { NEED_SAME(mala_create, ctx, t, cfg, out); }
extern "C" int mhx_rwmh_create_components(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_proposal_component* comps,
                                          int32_t ncomps, mhx_run** out)
{
    NEED_SAME(rwmh_create_components, ctx, t, cfg, comps, ncomps, out);
}
extern "C" int mhx_rwmh_create_conditional(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_proposal_component* comps,
                                           int32_t ncomps, const char* params_src, const void* data, size_t ndata, mhx_run** out)
{
    NEED_SAME(rwmh_create_conditional, ctx, t, cfg, comps, ncomps, params_src, data, ndata, out);
}
extern "C" int mhx_rwmh_create_composite(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_proposal_component* comps,
                                         int32_t ncomps, const mhx_proposal_block* blocks, int32_t nblocks, const int32_t* mapped,
                                         const char* params_src, const void* data, size_t ndata, mhx_run** out)
{
    NEED_SAME(rwmh_create_composite, ctx, t, cfg, comps, ncomps, blocks, nblocks, mapped, params_src, data, ndata, out);
}

extern "C" int mhx_ram_set_factor(mhx_run* r, const void* S) { NEED_SAMPLER(ram_set_factor, r, S); }
extern "C" int mhx_ram_set_factor_all(mhx_run* r, const void* S) { NEED_SAMPLER(ram_set_factor_all, r, S); }
extern "C" int mhx_ram_get_factor(mhx_run* r, void* S, uint8_t* status) { NEED_SAMPLER(ram_get_factor, r, S, status); }
extern "C" int mhx_ram_get_diag_range(mhx_run* r, void* diag_min, void* diag_max) { NEED_SAMPLER(ram_get_diag_range, r, diag_min, diag_max); }
extern "C" int mhx_ram_watch_factors(mhx_run* r, const int32_t* chains, int32_t n) { NEED_SAMPLER(ram_watch_factors, r, chains, n); }
extern "C" int mhx_ram_get_watched_factors(mhx_run* r, void* S, int64_t capacity, int64_t* n_recorded, int32_t* n_watched)
{
    NEED_SAMPLER(ram_get_watched_factors, r, S, capacity, n_recorded, n_watched);
}
extern "C" int mhx_ram_get_step_stats(mhx_run* r, void* log_alpha, double* eta, int64_t capacity, int64_t* n_recorded)
{
    NEED_SAMPLER(ram_get_step_stats, r, log_alpha, eta, capacity, n_recorded);
}
extern "C" int mhx_ram_get_adapt_state(mhx_run* r, void* log_alpha, double* eta, uint8_t* isaccept, uint64_t* iteration)
{
    NEED_SAMPLER(ram_get_adapt_state, r, log_alpha, eta, isaccept, iteration);
}

extern "C" int mhx_run_init(mhx_run* r, const void* initial_params) { NEED_SAMPLER(run_init, r, initial_params); }
extern "C" int mhx_run_sample(mhx_run* r, const mhx_schedule* s, int save_samples) { NEED_SAMPLER(run_sample, r, s, save_samples); }
extern "C" int mhx_run_get_samples(mhx_run* r, void* samples, uint8_t* accepted) { NEED(run_get_samples, r, samples, accepted); }
extern "C" int mhx_run_host_stats(mhx_run* r, mhx_host_stats* out) { NEED(run_host_stats, r, out); }
extern "C" int mhx_run_sample_to_host(mhx_run* r, const mhx_schedule* s, void* samples, uint8_t* accepted, int32_t slab_samples)
{
    NEED_SAMPLER(run_sample_to_host, r, s, samples, accepted, slab_samples);
}
extern "C" int mhx_run_device_samples(mhx_run* r, void** samples, void** accepted, int64_t* n_samples)
{
    NEED(run_device_samples, r, samples, accepted, n_samples);
}
extern "C" int mhx_run_get_state(mhx_run* r, void* x, void* lp, uint32_t* accept_counts) { NEED_SAMPLER(run_get_state, r, x, lp, accept_counts); }
extern "C" int mhx_run_set_state(mhx_run* r, const void* x) { NEED_SAMPLER(run_set_state, r, x); }
extern "C" int mhx_run_state_size(mhx_run* r, size_t* bytes) { NEED_SAMPLER(run_state_size, r, bytes); }
extern "C" int mhx_run_save_state(mhx_run* r, void* blob, size_t bytes) { NEED_SAMPLER(run_save_state, r, blob, bytes); }
extern "C" int mhx_run_load_state(mhx_run* r, const void* blob, size_t bytes) { NEED_SAMPLER(run_load_state, r, blob, bytes); }
extern "C" int mhx_run_stats(mhx_run* r, mhx_stats* out) { NEED(run_stats, r, out); }
extern "C" const char* mhx_run_form_name(const mhx_run* r)
{
    if (!r) return "";
    return FWD(run_form_name, r);
}
extern "C" int mhx_run_shape(const mhx_run* r, int32_t* dim, int32_t* nchains) { NEED(run_shape, r, dim, nchains); }
extern "C" int mhx_run_destroy(mhx_run* r) { NULL_OK(run_destroy, r); }
extern "C" int mhx_run_diagnostics(mhx_run* r, const mhx_diag_cfg* cfg, double* sum_m, double* sum_m2, double* sum_v, double* ess)
{
    NEED(run_diagnostics, r, cfg, sum_m, sum_m2, sum_v, ess);
}
extern "C" int mhx_run_ess_bulk_tail(mhx_run* r, const mhx_diag_cfg* cfg, const int32_t* params, int32_t nparams, double* ess_bulk, double* ess_tail)
{
    NEED(run_ess_bulk_tail, r, cfg, params, nparams, ess_bulk, ess_tail);
}
extern "C" int mhx_run_rank_diagnostics(mhx_run* r, const mhx_diag_cfg* cfg, const int32_t* params, int32_t nparams, double* ess_bulk,
                                        double* ess_tail, double* rhat_bulk, double* rhat_tail)
{
    NEED(run_rank_diagnostics, r, cfg, params, nparams, ess_bulk, ess_tail, rhat_bulk, rhat_tail);
}
extern "C" int mhx_run_rank_scores(mhx_run* r, int32_t param, int32_t folded, void* out_host) { NEED(run_rank_scores, r, param, folded, out_host); }
extern "C" int mhx_ctx_order_statistics(mhx_ctx* ctx, const void* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,
                                        const int32_t* params, int32_t nparams, const int64_t* ranks, int32_t nranks, double* out)
{
    NEED(ctx_order_statistics, ctx, d_tensor, n_samples, dim1, nchains, params, nparams, ranks, nranks, out);
}
extern "C" int mhx_run_order_statistics(mhx_run* r, const int32_t* params, int32_t nparams, const int64_t* ranks, int32_t nranks, double* out)
{
    NEED(run_order_statistics, r, params, nparams, ranks, nranks, out);
}
extern "C" int mhx_run_select_histogram(mhx_run* r, const int32_t* params, int32_t nparams, const uint64_t* prefixes, const int32_t* ngroups,
                                        int32_t gstride, int32_t shift, int32_t digit_bits, uint64_t* hist)
{
    NEED(run_select_histogram, r, params, nparams, prefixes, ngroups, gstride, shift, digit_bits, hist);
}
extern "C" int mhx_ctx_hpd(mhx_ctx* ctx, const void* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const int32_t* params,
                           int32_t nparams, double alpha, double* lower, double* upper)
{
    NEED(ctx_hpd, ctx, d_tensor, n_samples, dim1, nchains, params, nparams, alpha, lower, upper);
}
extern "C" int mhx_run_hpd(mhx_run* r, const int32_t* params, int32_t nparams, double alpha, double* lower, double* upper)
{
    NEED(run_hpd, r, params, nparams, alpha, lower, upper);
}
extern "C" int mhx_ctx_histogram(mhx_ctx* ctx, const void* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const int32_t* params,
                                 int32_t nparams, const double* edges, int32_t nbins, uint64_t* counts, uint64_t* outside)
{
    NEED(ctx_histogram, ctx, d_tensor, n_samples, dim1, nchains, params, nparams, edges, nbins, counts, outside);
}
extern "C" int mhx_run_histogram(mhx_run* r, const int32_t* params, int32_t nparams, const double* edges, int32_t nbins, uint64_t* counts,
                                 uint64_t* outside)
{
    NEED(run_histogram, r, params, nparams, edges, nbins, counts, outside);
}
extern "C" int mhx_ctx_histogram2d(mhx_ctx* ctx, const void* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const int32_t* params,
                                   int32_t nparams, const double* edges, int32_t nbins, const int32_t* pairs, int32_t npairs, uint64_t* counts,
                                   uint64_t* outside)
{
    NEED(ctx_histogram2d, ctx, d_tensor, n_samples, dim1, nchains, params, nparams, edges, nbins, pairs, npairs, counts, outside);
}
extern "C" int mhx_run_histogram2d(mhx_run* r, const int32_t* params, int32_t nparams, const double* edges, int32_t nbins, const int32_t* pairs,
                                   int32_t npairs, uint64_t* counts, uint64_t* outside)
{
    NEED(run_histogram2d, r, params, nparams, edges, nbins, pairs, npairs, counts, outside);
}
extern "C" int mhx_ctx_autocovariance(mhx_ctx* ctx, const void* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const int32_t* params,
                                      int32_t nparams, const int32_t* lags, int32_t nlags, int64_t chain_begin, int64_t chain_count,
                                      int32_t normalise, double* acov, int64_t* nvalid)
{
    NEED(ctx_autocovariance, ctx, d_tensor, n_samples, dim1, nchains, params, nparams, lags, nlags, chain_begin, chain_count, normalise, acov, nvalid);
}
extern "C" int mhx_run_autocovariance(mhx_run* r, const int32_t* params, int32_t nparams, const int32_t* lags, int32_t nlags, int64_t chain_begin,
                                      int64_t chain_count, int32_t normalise, double* acov, int64_t* nvalid)
{
    NEED(run_autocovariance, r, params, nparams, lags, nlags, chain_begin, chain_count, normalise, acov, nvalid);
}
extern "C" int mhx_run_derive(const mhx_run* src, const char* source, int32_t nout, const void* data, size_t ndata, mhx_run** out)
{
    NEED(run_derive, src, source, nout, data, ndata, out);
}
extern "C" int mhx_ctx_derive(mhx_ctx* ctx, const void* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const char* source,
                              int32_t nout, const void* data, size_t ndata, mhx_run** out)
{
    NEED(ctx_derive, ctx, d_tensor, n_samples, dim1, nchains, source, nout, data, ndata, out);
}
extern "C" int mhx_run_predict(const mhx_run* src, const char* source, int32_t nout, const void* data, size_t ndata, uint64_t seed, mhx_run** out)
{
    NEED(run_predict, src, source, nout, data, ndata, seed, out);
}
extern "C" int mhx_ctx_predict(mhx_ctx* ctx, const void* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, int64_t first_chain,
                               const char* source, int32_t nout, const void* data, size_t ndata, uint64_t seed, mhx_run** out)
{
    NEED(ctx_predict, ctx, d_tensor, n_samples, dim1, nchains, first_chain, source, nout, data, ndata, seed, out);
}
extern "C" int mhx_ctx_cross_moments(mhx_ctx* ctx, const void* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,
                                     const int32_t* params, int32_t nparams, const double* shift, double* sum, double* cross)
{
    NEED(ctx_cross_moments, ctx, d_tensor, n_samples, dim1, nchains, params, nparams, shift, sum, cross);
}
extern "C" int mhx_run_cross_moments(mhx_run* r, const int32_t* params, int32_t nparams, const double* shift, double* sum, double* cross,
                                     int64_t* n_draws)
{
    NEED(run_cross_moments, r, params, nparams, shift, sum, cross, n_draws);
}
extern "C" int mhx_emcee_half_step(mhx_run* r, int half, int begin, int count) { NEED_SAMPLER(emcee_half_step, r, half, begin, count); }
extern "C" int mhx_emcee_end_sweep(mhx_run* r) { NEED_SAMPLER(emcee_end_sweep, r); }
extern "C" int mhx_emcee_device_state(mhx_run* r, void** xw, int32_t* pitch, void** lp, uint32_t** acc_count, uint8_t** last_acc)
{
    NEED_SAMPLER(emcee_device_state, r, xw, pitch, lp, acc_count, last_acc);
}
extern "C" int mhx_emcee_exchange_plan(mhx_run* r, int half, int world, size_t* stride, void** stream)
{
    NEED_SAMPLER(emcee_exchange_plan, r, half, world, stride, stream);
}
extern "C" int mhx_emcee_exchange_pack(mhx_run* r, int half, int rank, int world, void* part) { NEED_SAMPLER(emcee_exchange_pack, r, half, rank, world, part); }
extern "C" int mhx_emcee_exchange_unpack(mhx_run* r, int half, int rank, int world, const void* stage, size_t stride)
{
    NEED_SAMPLER(emcee_exchange_unpack, r, half, rank, world, stage, stride);
}

#include "mhx_abi_pointwise.inc"
#include "mhx_abi_tempered.inc"
#include "mhx_abi_adaptive.inc"
