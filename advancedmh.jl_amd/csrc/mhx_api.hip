// mhx_api.hip -- host side of libmhx.so: the C ABI of include/mhx.h, device memory ownership,
// kernel selection (pre-built register kernel / hiprtc-specialised kernel / generic kernel) and
// the mcmcsample-equivalent launch schedule.  No torch types, no C++ types across the boundary.
#include "../../include/mhx.h"

#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include <errno.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <rocprim/rocprim.hpp>   // device radix sort for the rank-normalised ESS (after <cstring>: it calls memset)

#include "mhx_rwmh_kernels.h"
#include "mhx_rwmh_family_kernels.h"
#include "mhx_rwmh_cond_kernels.h"
#include "mhx_rwmh_composite_kernels.h"
#include "mhx_rwmh_tempered_kernels.h"
#include "mhx_rwmh_adaptive_kernels.h"
#include "mhx_evidence_kernels.h"
#include "mhx_emcee_kernels.h"
#include "mhx_ram_kernels.h"
#include "mhx_mala_kernels.h"
#include "mhx_rwmh_dense_kernels.h"
#include "mhx_rwmh_mfma_kernels.h"
#include "mhx_mala_mfma_kernels.h"
#include "mhx_diag_kernels.h"
#include "mhx_cross_kernels.h"
#include "mhx_hpd_kernels.h"
#include "mhx_hist_kernels.h"
#include "mhx_acf_kernels.h"
#include "mhx_derive_kernels.h"     // (its constants: the frame itself is compiled at run time only)
#include "mhx_pointwise_kernels.h"  // (likewise)
#include "mhx_psis_kernels.h"       // (likewise)
#ifdef MHX_TOOLS_BUILD
#include "mhx_jit_embed_tools.inc"   // generated: the device headers as string literals for hiprtc, probes included
#else
#include "mhx_jit_embed.inc"         // generated (embed_headers.py --release): the same text without its MHX_TOOLS_BUILD blocks
#endif
#include "mhx_jit_ext.h"        // run-time kernels through the installation's clang++ (pure host code)
#include "mhx_select.h"         // bucket scan and pass loop of the exact order statistics (pure host code, shared likewise)
#include "mhx_host_expand.h"    // the host threads of the accept-compacted return path (pure host code, shared by both instantiations)
#include "mhx_impl.h"           // the prototypes of this instantiation (api_*), shared with the dispatcher mhx_abi.cpp

#define HIP_TRY(expr)                                                                              \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return mhx_fail(MHX_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,  \
                        __LINE__);                                                                  \
    } while (0)

// Every copy that touches run / target state goes through the context's stream (created non-blocking: the null stream
// does not order against it) and is waited for, so that all accesses to device state are ordered on ONE stream.
#define COPY_SYNC(stream, dst, src, bytes, kind)                                                    \
    do {                                                                                            \
        HIP_TRY(hipMemcpyAsync((dst), (src), (bytes), (kind), (stream)));                           \
        HIP_TRY(hipStreamSynchronize(stream));                                                      \
    } while (0)

namespace MHX_NS {

// ---------------------------------------------------------------------------------------------
// pre-built kernels (hipcc, gfx950)
template <int D, int TK, int PK>
__global__ void __launch_bounds__(64)
k_rwmh_reg(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ pvec)
{
    mhx_rwmh_reg_body<D, TK, PK>(a, tparams, pvec);
}
template <int PK, int K>
__global__ void __launch_bounds__(64)
k_rwmh_wave(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ pvec)
{
    mhx_rwmh_wave_body<PK, K>(a, tparams, pvec);
}
__global__ void __launch_bounds__(256)
k_rwmh_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ pvec)
{
    mhx_rwmh_generic_body<MHX_TARGET_DYNAMIC>(a, tparams, pvec);
}
__global__ void __launch_bounds__(256)
k_rwmh_init(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ pvec, const int draw)
{
    mhx_rwmh_init_body<MHX_TARGET_DYNAMIC>(a, tparams, pvec, draw);
}
__global__ void __launch_bounds__(256)
k_target_eval(const mhx_real* __restrict__ x, mhx_real* __restrict__ lp, const int n, const int d, const int kind,
              const mhx_real* __restrict__ tparams, const int ntparams, const mhx_real tconst, const int lanes)
{
    mhx_target_eval_body<MHX_TARGET_DYNAMIC>(x, lp, n, d, kind, tparams, ntparams, tconst, lanes);
}
__global__ void __launch_bounds__(256)
k_record_state(const mhx_real* __restrict__ x, const mhx_real* __restrict__ lp, const unsigned char* __restrict__ last_acc,
               mhx_real* samples, unsigned char* accepted, const int n, const long ld, const int d, const long slot)
{
    mhx_record_state_body(x, lp, last_acc, samples, accepted, n, ld, d, slot);
}

// proposals of univariate family components (mhx_rwmh_family_kernels.h): the state-in-HBM form, the initial draw, q(x) of a static run
__global__ void __launch_bounds__(256)
k_fam_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_fam_comp* __restrict__ fam, const int symmetric)
{
    mhx_fam_generic_body<MHX_TARGET_DYNAMIC>(a, tparams, fam, symmetric);
}
__global__ void __launch_bounds__(256)
k_fam_init_draw(const mhx_rwmh_args a, const mhx_fam_comp* __restrict__ fam)
{
    mhx_fam_init_draw_body(a, fam);
}
__global__ void __launch_bounds__(256)
k_fam_q(const mhx_rwmh_args a, const mhx_fam_comp* __restrict__ fam)
{
    mhx_fam_q_body(a, fam);
}

// (MHX_COOP_WAVES, the occupancy target of the cooperative kernel, comes from mhx_rwmh_kernels.h)
template <int L, int NBL, int TK, int PK, bool MOM, int GEN = MHX_GEN_BOX_MULLER>
__global__ void __launch_bounds__(256, MHX_COOP_WAVES(NBL))
k_rwmh_coop(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ pvec)
{
    mhx_rwmh_coop_body<L, NBL, TK, PK, MOM, MHX_WALK_PLAIN, GEN>(a, tparams, pvec);
}
#if MHX_REAL64
// the same shape as generator / consumer wave pairs (mhx_rwmh_coop_pairs_body): 512 threads, two waves per SIMD
template <int L, int NBL, int TK, int PK>
__global__ void __launch_bounds__(512)
k_rwmh_coop_pairs(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ pvec)
{
    mhx_rwmh_coop_pairs_body<L, NBL, TK, PK>(a, tparams, pvec);
}
#endif
__global__ void __launch_bounds__(256)
k_moments_first(const mhx_real* __restrict__ x, const mhx_real* __restrict__ lp, mhx_real* mean, mhx_real* m2, const int n,
                const long ld, const int d)
{
    mhx_moments_first_body(x, lp, mean, m2, n, ld, d);
}

// `fn` records samples, `fn_mom` keeps running moments instead (null: specialised by hiprtc on demand)
struct prebuilt_coop {
    int L, NBL, TK, PK;
    void (*fn)(const mhx_rwmh_args, const mhx_real*, const mhx_real*);
    void (*fn_mom)(const mhx_rwmh_args, const mhx_real*, const mhx_real*);
    int gen;                             // MHX_GEN_*: the normal generator the kernel was built with
    void (*fn_pairs)(const mhx_rwmh_args, const mhx_real*, const mhx_real*);   // `fn` as generator / consumer wave pairs, or null
};
// the BASELINE shapes: C2 (65 536 chains x d = 100) and C5 (32 768 chains per GPU x d = 1000); a double takes two VGPRs,
// so the fp64 engine spreads a chain over more lanes
#if MHX_REAL64
#define MHX_C2_L 2
#define MHX_C2_NBL 13
#define MHX_C5_L 64
#define MHX_C5_NBL 4
#else
#define MHX_C2_L 2
#define MHX_C2_NBL 13
#define MHX_C5_L 32
#define MHX_C5_NBL 8
#endif
static const prebuilt_coop k_prebuilt_coop[] = {
    {MHX_C2_L, MHX_C2_NBL, MHX_TARGET_ISO_GAUSS, MHX_PROP_ISO, k_rwmh_coop<MHX_C2_L, MHX_C2_NBL, MHX_TARGET_ISO_GAUSS, MHX_PROP_ISO, false>, nullptr},
    {MHX_C5_L, MHX_C5_NBL, MHX_TARGET_FUNNEL, MHX_PROP_ISO, k_rwmh_coop<MHX_C5_L, MHX_C5_NBL, MHX_TARGET_FUNNEL, MHX_PROP_ISO, false>,
     k_rwmh_coop<MHX_C5_L, MHX_C5_NBL, MHX_TARGET_FUNNEL, MHX_PROP_ISO, true>},
    {MHX_C5_L, MHX_C5_NBL, MHX_TARGET_BANANA, MHX_PROP_ISO, k_rwmh_coop<MHX_C5_L, MHX_C5_NBL, MHX_TARGET_BANANA, MHX_PROP_ISO, false>,
     k_rwmh_coop<MHX_C5_L, MHX_C5_NBL, MHX_TARGET_BANANA, MHX_PROP_ISO, true>},
    // the same shapes with the ziggurat generator (MHX_FLAG_ZIGGURAT; both widths since round 6)
    {MHX_C2_L, MHX_C2_NBL, MHX_TARGET_ISO_GAUSS, MHX_PROP_ISO,
     k_rwmh_coop<MHX_C2_L, MHX_C2_NBL, MHX_TARGET_ISO_GAUSS, MHX_PROP_ISO, false, MHX_GEN_ZIGGURAT>, nullptr, MHX_GEN_ZIGGURAT,
#if MHX_REAL64
     k_rwmh_coop_pairs<MHX_C2_L, MHX_C2_NBL, MHX_TARGET_ISO_GAUSS, MHX_PROP_ISO>
#else
     nullptr
#endif
    },
    {MHX_C5_L, MHX_C5_NBL, MHX_TARGET_FUNNEL, MHX_PROP_ISO,
     k_rwmh_coop<MHX_C5_L, MHX_C5_NBL, MHX_TARGET_FUNNEL, MHX_PROP_ISO, false, MHX_GEN_ZIGGURAT>,
     k_rwmh_coop<MHX_C5_L, MHX_C5_NBL, MHX_TARGET_FUNNEL, MHX_PROP_ISO, true, MHX_GEN_ZIGGURAT>, MHX_GEN_ZIGGURAT},
};

// sum of a u32 array into a u64 (one atomic per block)
__global__ void __launch_bounds__(256)
k_sum_u32(const unsigned* __restrict__ v, const long n, unsigned long long* out)
{
    __shared__ unsigned long long red[4];
    unsigned long long s = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) s += v[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

struct prebuilt_reg { int D, TK, PK; void (*fn)(const mhx_rwmh_args, const mhx_real*, const mhx_real*); };
static const prebuilt_reg k_prebuilt_reg[] = {
#if !MHX_REAL64
    {100, MHX_TARGET_ISO_GAUSS, MHX_PROP_ISO, k_rwmh_reg<100, MHX_TARGET_ISO_GAUSS, MHX_PROP_ISO>},
#endif
    {2, MHX_TARGET_IID_NORMAL, MHX_PROP_ISO, k_rwmh_reg<2, MHX_TARGET_IID_NORMAL, MHX_PROP_ISO>},     // C1, README.md:29-31
};

// ---------------------------------------------------------------------------------------------
// context + JIT cache
struct jit_module {
    hipModule_t mod = nullptr;
    std::map<std::string, hipFunction_t> fns;
};

// one of three buffer sets a compacted slab travels through (mhx_api_host.inc): device block -> page-locked staging -> host threads
struct compact_pair {
    unsigned char* dev_fixed = nullptr;  // header + masks + ranks + accept flags
    size_t dev_fixed_cap = 0;
    unsigned char* dev_pay = nullptr;    // the changed columns
    size_t dev_pay_cap = 0;
    unsigned char* host = nullptr;       // the block as the host threads read it (page-locked)
    size_t host_cap = 0;
    hipEvent_t c0 = nullptr, c1 = nullptr, scattered = nullptr;   // copy begin / end (timed), payload written
    uint64_t seq = 0;                    // the expander job that reads `host`
    bool used = false;
    int device = 0;
    double link_ms = 0.0;                // copy time of this pair's blocks in the current call (written by one expander thread)
};

struct mhx_ctx : mhx_handle_hdr {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::map<std::string, std::unique_ptr<jit_module>> jit;
    long jit_compiles = 0, jit_cache_hits = 0;      // compilations / code objects taken from the on-disk cache
    long jit_ext_compiles = 0;                      // ... of the compilations, by the installation's clang++ (mhx_jit_ext.h)
    // the return path of mhx_run_sample_to_host: a second stream for the D2H copies + the slab hand-over events
    hipStream_t copy_stream = nullptr;
    hipEvent_t slab_done[2] = {nullptr, nullptr}, slab_free[2] = {nullptr, nullptr};
    long pins_registered = 0, pins_released = 0;    // caller buffers page-locked for the duration of a call / released again
    std::map<std::string, std::string> options;     // mhx_ctx_set_option: explicit engine options (never the environment)
    bool tainted = false;                           // a probe / fault-injection option of the tools build was set: results may be invalid
    // the accept-compacted return path: three buffer sets, the pinned landing place of a block's header, the host threads
    compact_pair cpair[3];
    mhx_compact_hdr* hdr_pinned = nullptr;
    mhx_expander* expander = nullptr;
    int expander_threads = 0, expander_chunk = 0, expander_numa = -1;   // the options / memory node the expander was created with
    // three scratch blocks of the post-run statistics, each grown on demand by scratch_carve and kept until the context closes
    // (DESIGN.md section 6.5).  A block belongs to one call at a time: whoever carves it owns all of it until that call returns.
    void* select_scratch = nullptr;                 // the sweeps that return counters or sums: a select pass (also the one inside HPD), the
    size_t select_bytes = 0;                        // histograms, the autocovariance
    uint64_t* select_landing = nullptr;             // the select's page-locked landing place on the host (grown on demand)
    size_t select_landing_words = 0;
    void* cross_scratch = nullptr;                  // the cross moments alone: partial tiles, tables and results
    size_t cross_bytes = 0;
    void* hpd_scratch = nullptr;                    // the tails of HPD or of PSIS-LOO, held across the call's select passes: tail keys,
    size_t hpd_bytes = 0;                           // their sort, what follows it (bounded by HPD_SCRATCH_MB / PSIS_SCRATCH_MB)
    ~mhx_ctx()
    {
        if (hpd_scratch) (void)hipFree(hpd_scratch);
        if (cross_scratch) (void)hipFree(cross_scratch);
        if (select_scratch) (void)hipFree(select_scratch);
        if (select_landing) (void)hipHostFree(select_landing);
        if (expander) mhx_expander_destroy(expander);
        for (compact_pair& P : cpair) {
            if (P.dev_fixed) (void)hipFree(P.dev_fixed);
            if (P.dev_pay) (void)hipFree(P.dev_pay);
            if (P.host) (void)hipHostFree(P.host);
            if (P.c0) (void)hipEventDestroy(P.c0);
            if (P.c1) (void)hipEventDestroy(P.c1);
            if (P.scattered) (void)hipEventDestroy(P.scattered);
        }
        if (hdr_pinned) (void)hipHostFree(hdr_pinned);
        for (int i = 0; i < 2; ++i) {
            if (slab_done[i]) (void)hipEventDestroy(slab_done[i]);
            if (slab_free[i]) (void)hipEventDestroy(slab_free[i]);
        }
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        for (auto& kv : jit)
            if (kv.second && kv.second->mod) (void)hipModuleUnload(kv.second->mod);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

int api_ctx_create(int device, mhx_ctx** out)
{
    if (!out) return mhx_fail(MHX_EINVAL, "mhx_ctx_create: out is NULL");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return mhx_fail(MHX_EINVAL, "mhx_ctx_create: device %d of %d", device, n);
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<mhx_ctx> c(new mhx_ctx);
    c->device = device;
    c->dtype = MHX_REAL64 ? MHX_F64 : MHX_F32;
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&c->ev0));
    HIP_TRY(hipEventCreate(&c->ev1));
    *out = c.release();
    return MHX_OK;
}

int api_ctx_device(const mhx_ctx* ctx) { return ctx->device; }

// ---- engine options (include/mhx.h: mhx_ctx_set_option) -------------------------------------------------------------------
// probe = 1: timing probes and fault injection -- they exist in the tools build only (libmhx_tools.so, -DMHX_TOOLS_BUILD) and
// taint the context; the release library does not even carry their names.
struct opt_name { const char* name; int probe; };
static const opt_name k_opt_names[] = {
    {"NO_PREBUILT", 0}, {"NO_MFMA", 0}, {"MFMA_WAVES", 0}, {"REG_MAX_DIM", 0}, {"REG_XR", 0}, {"REG_UNROLL", 0}, {"REG_WAVES", 0}, {"REG_ZSLAB", 0}, {"COOP_WAVES", 0}, {"COOP_PAIRS", 0},
    {"MALA_XR", 0}, {"RAM_G", 0}, {"RAM_LDS_PAD", 0}, {"WAVE_K", 0},
    {"EMCEE_MFMA", 0}, {"EMCEE_MFMA_WAVES", 0}, {"EMCEE_SCALAR", 0}, {"EMCEE_SCAL_MODE", 0}, {"EMCEE_SCAL_WPB", 0}, {"EMCEE_SCAL_REC", 0},
    {"EMCEE_FUSED", 0}, {"EMCEE_PERSIST", 0}, {"EMCEE_PRELOAD", 0}, {"EMCEE_DEFER", 0}, {"EMCEE_SWEEP_DEFER", 0}, {"EMCEE_WAVES", 0},
    {"EMCEE_REC_STORE", 0}, {"EMCEE_ROW_STORE", 0}, {"EMCEE_COOP_REC", 0},
    {"HOST_COMPACT", 0}, {"HOST_THREADS", 0}, {"HOST_CHUNK", 0}, {"HOST_NUMA", 0}, {"TOTAL_CHAINS", 0}, {"JIT_COMPILER", 0}, {"SELECT_BITS", 0}, {"HPD_SCRATCH_MB", 0}, {"ACF_R", 0}, {"DERIVE_DRAWS", 0}, {"POINTWISE_ROWS", 0}, {"PSIS_SCRATCH_MB", 0}, {"PSIS_ROWS", 0},
#ifdef MHX_TOOLS_BUILD
    {"ZIG_PROBE", 1}, {"ZIG_FORCE_FAIL", 1}, {"JIT_DEFS", 1}, {"JIT_FLAGS", 1}, {"EMCEE_PROBE", 1}, {"EMCEE_STAMPS", 1}, {"EMCEE_STAMPS_FILE", 1},
    {"FAULT_SLAB", 1}, {"RAM_PROF", 1}, {"HPD_STOP_AFTER", 1}, {"PSIS_STOP_AFTER", 1},
#endif
};
static const opt_name* opt_find(const char* name)
{
    if (name)
        for (const opt_name& o : k_opt_names)
            if (!strcmp(o.name, name)) return &o;
    return nullptr;
}
// probe options are compiled out of the release library, names included
#ifdef MHX_TOOLS_BUILD
#define MHX_PROBE_OPT(ctx, name) opt(ctx, name)
#else
#define MHX_PROBE_OPT(ctx, name) ((const char*)nullptr)
#endif
// the value of an option, or nullptr when unset (the shape of the getenv() calls this replaced)
static const char* opt(const mhx_ctx* ctx, const char* name)
{
    if (!ctx || ctx->options.empty()) return nullptr;
    auto it = ctx->options.find(name);
    return it == ctx->options.end() ? nullptr : it->second.c_str();
}
// ... as a number (`unset_value` when the option is not set), and as a switch (set and not 0)
static int opt_int(const mhx_ctx* ctx, const char* name, int unset_value)
{
    const char* v = opt(ctx, name);
    return v ? atoi(v) : unset_value;
}
static bool opt_on(const mhx_ctx* ctx, const char* name) { return opt_int(ctx, name, 0) != 0; }
// The chains of the WHOLE run a shard belongs to (option TOTAL_CHAINS; mhx_group_shard sets it on the member's context, a process
// of a multi-process run sets it itself): the kernel form -- and with it the summation order of the log-density -- is chosen for
// that count, so that a shard takes the form the unsharded run takes and stays bit for bit its part of it (the
// wave-per-chain kernel was picked from the LOCAL count: 8 x 1024 chains ran shape 64 where 8192 run shape 1).
static long chains_of_whole_run(const mhx_ctx* ctx, long local)
{
    const char* v = opt(ctx, "TOTAL_CHAINS");
    const long all = v ? atol(v) : 0;
    return all > local ? all : local;
}

int api_ctx_set_option(mhx_ctx* ctx, const char* name, const char* value)
{
    const opt_name* o = opt_find(name);
    if (!o) return mhx_fail(MHX_EINVAL, "mhx_ctx_set_option: unknown option '%s'%s", name ? name : "(null)",
#ifdef MHX_TOOLS_BUILD
                            "");
#else
                            " (timing probes and fault injection exist in the tools build only: libmhx_tools.so)");
#endif
    if (!value) { ctx->options.erase(name); return MHX_OK; }
    ctx->options[name] = value;
    if (o->probe) ctx->tainted = true;              // sticky: a context that ever carried a probe stays marked
    return MHX_OK;
}
int api_ctx_get_option(const mhx_ctx* ctx, const char* name, char* buf, size_t len)
{
    if (!opt_find(name)) return mhx_fail(MHX_EINVAL, "mhx_ctx_get_option: unknown option '%s'", name ? name : "(null)");
    if (!buf || !len) return mhx_fail(MHX_EINVAL, "mhx_ctx_get_option: no buffer");
    const char* v = opt(ctx, name);
    snprintf(buf, len, "%s", v ? v : "");
    return MHX_OK;
}
int api_ctx_pci_bus_id(const mhx_ctx* ctx, char* buf, size_t len)
{
    if (!buf || len < 16) return mhx_fail(MHX_EINVAL, "mhx_ctx_pci_bus_id: buffer of >= 16 bytes needed");
    HIP_TRY(hipDeviceGetPCIBusId(buf, (int)len, ctx->device));
    return MHX_OK;
}
int api_ctx_host_pin_counts(const mhx_ctx* ctx, int64_t* registered, int64_t* released)
{
    if (registered) *registered = ctx->pins_registered;
    if (released) *released = ctx->pins_released;
    return MHX_OK;
}

int api_ctx_jit_counts(const mhx_ctx* ctx, int64_t* compiles, int64_t* cache_hits)
{
    if (compiles) *compiles = ctx->jit_compiles;
    if (cache_hits) *cache_hits = ctx->jit_cache_hits;
    return MHX_OK;
}

int api_ctx_jit_compiler(const mhx_ctx* ctx, char* compiler, size_t len, int64_t* ext_compiles)
{
    if (compiler && len) {
        const char* jc = nullptr;
        auto it = ctx->options.find("JIT_COMPILER");
        if (it != ctx->options.end()) jc = it->second.c_str();
        if (!jc) { jc = getenv("MHX_JIT_COMPILER"); if (jc && !*jc) jc = nullptr; }
        const std::string id = (jc && !strcmp(jc, "hiprtc")) ? std::string() : mhx_jit_ext_identity();
        snprintf(compiler, len, "%s", id.c_str());
    }
    if (ext_compiles) *ext_compiles = ctx->jit_ext_compiles;
    return MHX_OK;
}

int api_ctx_destroy(mhx_ctx* ctx)
{
    if (!ctx) return MHX_OK;
    (void)hipSetDevice(ctx->device);
    delete ctx;
    return MHX_OK;
}

// ---- persistent code-object cache -------------------------------------------------------------------------------------
// hiprtc takes 0.3 s for a small specialisation and up to a minute for the unrolled matrix-core kernels (d = 1000); the code
// object depends only on (source, embedded headers, options, compiler), so it is kept on disk: $MHX_CACHE_DIR, else
// $XDG_CACHE_HOME/mhx, else $HOME/.cache/mhx; MHX_CACHE_DIR="" (or MHX_NO_JIT_CACHE=1) switches it off.  Files are written to
// a temporary name and renamed, so concurrent processes (one per GPU) never see a partial object.
static unsigned long long fnv64(const void* data, size_t n, unsigned long long h)
{
    const unsigned char* p = (const unsigned char*)data;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}
static std::string jit_cache_dir()
{
    if (const char* off = getenv("MHX_NO_JIT_CACHE")) if (*off && *off != '0') return "";
    std::string dir;
    if (const char* e = getenv("MHX_CACHE_DIR")) { if (!*e) return ""; dir = e; }
    else if (const char* x = getenv("XDG_CACHE_HOME")) { if (*x) dir = std::string(x) + "/mhx"; }
    if (dir.empty()) { const char* h = getenv("HOME"); if (!h || !*h) return ""; dir = std::string(h) + "/.cache/mhx"; }
    // mkdir -p (two levels are enough for the defaults; an explicit MHX_CACHE_DIR must have an existing parent)
    const size_t cut = dir.find_last_of('/');
    if (cut != std::string::npos && cut > 0) (void)mkdir(dir.substr(0, cut).c_str(), 0755);
    if (mkdir(dir.c_str(), 0755) != 0 && errno != EEXIST) return "";
    return dir;
}
static std::string jit_cache_name(const std::string& source, const std::vector<std::string>& opts, const char* const* hdr_src, int nhdr,
                                  const std::string& compiler_id)
{
    unsigned long long h1 = 1469598103934665603ull, h2 = 0x9e3779b97f4a7c15ull;
    auto mix = [&](const void* d, size_t n) { h1 = fnv64(d, n, h1); h2 = fnv64(d, n, h2 ^ (unsigned long long)n); };
    mix(source.data(), source.size());
    mix(compiler_id.data(), compiler_id.size());
    for (auto& o : opts) { mix(o.data(), o.size()); mix("\0", 1); }
    for (int i = 0; i < nhdr; ++i) mix(hdr_src[i], strlen(hdr_src[i]));
    int vmaj = 0, vmin = 0, rt = 0;
    (void)hiprtcVersion(&vmaj, &vmin);
    (void)hipRuntimeGetVersion(&rt);
    const int ver[4] = {vmaj, vmin, rt, MHX_VERSION};
    mix(ver, sizeof ver);
    char b[64];
    snprintf(b, sizeof b, "%016llx%016llx.hsaco", h1, h2);
    return b;
}
static bool jit_cache_read(const std::string& path, std::vector<char>* code)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    bool ok = false;
    if (fseek(f, 0, SEEK_END) == 0) {
        const long n = ftell(f);
        if (n > 16 && fseek(f, 0, SEEK_SET) == 0) {
            code->resize((size_t)n);
            ok = fread(code->data(), 1, (size_t)n, f) == (size_t)n && memcmp(code->data(), "\x7f" "ELF", 4) == 0;
        }
    }
    fclose(f);
    return ok;
}
static void jit_cache_write(const std::string& dir, const std::string& name, const std::vector<char>& code)
{
    char tmp[64];
    snprintf(tmp, sizeof tmp, "/.tmp.%ld.%llx", (long)getpid(), (unsigned long long)(size_t)code.data());
    const std::string t = dir + tmp;
    FILE* f = fopen(t.c_str(), "wb");
    if (!f) return;
    const bool ok = fwrite(code.data(), 1, code.size(), f) == code.size();
    if (fclose(f) != 0 || !ok || rename(t.c_str(), (dir + "/" + name).c_str()) != 0) (void)remove(t.c_str());
}

// compile `source` (which #includes the embedded device headers) with hiprtc for gfx950
static int jit_compile(mhx_ctx* ctx, const std::string& source, const std::vector<std::string>& defines, jit_module** out,
                       const std::vector<std::string>& extra_opts = {})
{
    // tools build, option JIT_DEFS = "NAME=VALUE NAME=VALUE": extra defines for every hiprtc compile of the context -- how the A/B
    // scripts reach the kernels' compile-time knobs; part of both cache keys.  It taints the context (a define can change a
    // kernel's LDS layout behind the host's back), and the release library has no such door.
    const char* xdefs = MHX_PROBE_OPT(ctx, "JIT_DEFS");
    struct jit_guard { jit_guard() { mhx_jit_lock(); } ~jit_guard() { mhx_jit_unlock(); } } one_at_a_time;
    const char* xflags = MHX_PROBE_OPT(ctx, "JIT_FLAGS");      // (tools build: raw compiler options, blank-separated, for A/B of code generation)
    const char* hdr_src[] = {k_src_mhx_zig_table_h, k_src_mhx_device_math_h, k_src_mhx_targets_h, k_src_mhx_rwmh_kernels_h,
                             k_src_mhx_emcee_kernels_h, k_src_mhx_ram_kernels_h, k_src_mhx_mala_kernels_h,
                             k_src_mhx_rwmh_dense_kernels_h, k_src_mhx_rwmh_mfma_kernels_h,
                             k_src_mhx_mala_mfma_kernels_h, k_src_mhx_emcee_mfma_kernels_h, k_src_mhx_rwmh_family_kernels_h,
                             k_src_mhx_rwmh_cond_kernels_h, k_src_mhx_rwmh_composite_kernels_h, k_src_mhx_derive_kernels_h,
                             k_src_mhx_pointwise_kernels_h, k_src_mhx_psis_kernels_h, k_src_mhx_rwmh_tempered_kernels_h,
                             k_src_mhx_rwmh_adaptive_kernels_h};
    const char* hdr_name[] = {"mhx_zig_table.h", "mhx_device_math.h", "mhx_targets.h", "mhx_rwmh_kernels.h",
                              "mhx_emcee_kernels.h", "mhx_ram_kernels.h", "mhx_mala_kernels.h",
                              "mhx_rwmh_dense_kernels.h", "mhx_rwmh_mfma_kernels.h", "mhx_mala_mfma_kernels.h", "mhx_emcee_mfma_kernels.h",
                              "mhx_rwmh_family_kernels.h", "mhx_rwmh_cond_kernels.h", "mhx_rwmh_composite_kernels.h", "mhx_derive_kernels.h",
                              "mhx_pointwise_kernels.h", "mhx_psis_kernels.h", "mhx_rwmh_tempered_kernels.h", "mhx_rwmh_adaptive_kernels.h"};
    const int nhdr = (int)(sizeof hdr_src / sizeof hdr_src[0]);
    std::vector<std::string> opts = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                                     MHX_REAL64 ? "-DMHX_REAL64=1" : "-DMHX_REAL64=0", "-DMHX_XW_LINE=" + std::to_string(MHX_XW_LINE)};
#ifdef MHX_TOOLS_BUILD
    opts.push_back("-DMHX_TOOLS_BUILD=1");              // the embedded headers of this build carry the probes
#endif
    // the blank-separated words of `list`, each behind `prefix`
    auto push_words = [&opts](const char* list, const char* prefix) {
        for (const char* p = list; p && *p;) {
            while (*p == ' ') ++p;
            const char* e = p;
            while (*e && *e != ' ') ++e;
            if (e > p) opts.push_back(prefix + std::string(p, e));
            p = e;
        }
    };
    for (auto& d : defines) opts.push_back("-D" + d);
    push_words(xdefs, "-D");
    for (auto& o : extra_opts) opts.push_back(o);
    push_words(xflags, "");
    // the context's modules are keyed by what is compiled: the source and every option ('\0' occurs in neither).  Not by the
    // compiler: a module the context holds is reused whichever one the option names now
    std::string key = source;
    for (auto& o : opts) { key += '\0'; key += o; }
    auto it = ctx->jit.find(key);
    if (it != ctx->jit.end()) { *out = it->second.get(); return MHX_OK; }
    // Which compiler: the installation's clang++ where there is one (mhx_jit_ext.h: hiprtc is whichever copy the process loaded first,
    // a PyTorch wheel's older one inside Python), hiprtc otherwise or when option JIT_COMPILER says "hiprtc"; "clang" = no fall-back
    const char* jc = opt(ctx, "JIT_COMPILER");
    if (!jc) { jc = getenv("MHX_JIT_COMPILER"); if (jc && !*jc) jc = nullptr; }     // (the process-wide default of the option)
    const bool want_ext = !(jc && !strcmp(jc, "hiprtc")) && !mhx_jit_ext_identity().empty();
    if (jc && !strcmp(jc, "clang") && !want_ext) return mhx_fail(MHX_EJIT, "JIT_COMPILER=clang: no clang++ found (MHX_JIT_CLANG, ROCM_PATH, /opt/rocm)");
    const std::string cdir = jit_cache_dir();
    const std::string cname = cdir.empty() ? std::string() : jit_cache_name(source, opts, hdr_src, nhdr, want_ext ? mhx_jit_ext_identity() : std::string());
    // (where the offline compiler is preferred but failed on this source before, hiprtc's object is there under its own name)
    const std::string cname_rtc = (cdir.empty() || !want_ext) ? cname : jit_cache_name(source, opts, hdr_src, nhdr, std::string());
    std::vector<char> code;
    bool from_cache = !cdir.empty() && (jit_cache_read(cdir + "/" + cname, &code) || (want_ext && jit_cache_read(cdir + "/" + cname_rtc, &code)));
    if (from_cache) {
        std::unique_ptr<jit_module> m(new jit_module);
        if (hipModuleLoadData(&m->mod, code.data()) == hipSuccess) {
            ctx->jit_cache_hits++;
            *out = m.get();
            ctx->jit[key] = std::move(m);
            return MHX_OK;
        }
        (void)hipGetLastError();            // a stale / foreign object: fall through and compile
        from_cache = false;
    }
    if (want_ext) {
        std::string xlog;
        if (mhx_jit_ext_compile(source, hdr_src, hdr_name, nhdr, opts, &code, &xlog)) {
            std::unique_ptr<jit_module> m(new jit_module);
            const hipError_t e = hipModuleLoadData(&m->mod, code.data());
            if (e == hipSuccess) {
                ctx->jit_compiles++;
                ctx->jit_ext_compiles++;
                if (!cdir.empty()) jit_cache_write(cdir, cname, code);
                *out = m.get();
                ctx->jit[key] = std::move(m);
                return MHX_OK;
            }
            (void)hipGetLastError();
            xlog = std::string("hipModuleLoadData: ") + hipGetErrorString(e);
        }
        if (jc && !strcmp(jc, "clang")) {
            if (xlog.size() > 1800) xlog.resize(1800);
            return mhx_fail(MHX_EJIT, "JIT_COMPILER=clang: %s", xlog.c_str());
        }
        // (a source that does not compile fails here too: hiprtc's log is the one the caller gets; MHX_JIT_VERBOSE=1 shows this one)
        if (const char* v = getenv("MHX_JIT_VERBOSE")) if (*v && *v != '0') {
            std::string what;
            for (auto& d : defines) what += " " + d;
            fprintf(stderr, "mhx: the offline compiler failed on%s, hiprtc takes over: %.1500s\n", what.c_str(), xlog.c_str());
        }
    }
    hiprtcProgram prog = nullptr;
    hiprtcResult r = hiprtcCreateProgram(&prog, source.c_str(), "mhx_jit.hip", nhdr, hdr_src, hdr_name);
    if (r != HIPRTC_SUCCESS) return mhx_fail(MHX_EJIT, "hiprtcCreateProgram: %s", hiprtcGetErrorString(r));
    std::vector<const char*> copts;
    for (auto& o : opts) copts.push_back(o.c_str());
    r = hiprtcCompileProgram(prog, (int)copts.size(), copts.data());
    if (r != HIPRTC_SUCCESS) {
        size_t ls = 0;
        hiprtcGetProgramLogSize(prog, &ls);
        std::string log(ls, '\0');
        if (ls) hiprtcGetProgramLog(prog, &log[0]);
        hiprtcDestroyProgram(&prog);
        if (log.size() > 1800) log.resize(1800);
        return mhx_fail(MHX_EJIT, "hiprtc compile failed (%s): %s", hiprtcGetErrorString(r), log.c_str());
    }
    size_t cs = 0;
    hiprtcGetCodeSize(prog, &cs);
    code.resize(cs);
    hiprtcGetCode(prog, code.data());
    hiprtcDestroyProgram(&prog);
    ctx->jit_compiles++;
    std::unique_ptr<jit_module> m(new jit_module);
    hipError_t e = hipModuleLoadData(&m->mod, code.data());
    if (e != hipSuccess) return mhx_fail(MHX_EJIT, "hipModuleLoadData: %s", hipGetErrorString(e));
    if (!cdir.empty()) jit_cache_write(cdir, cname_rtc, code);
    *out = m.get();
    ctx->jit[key] = std::move(m);
    return MHX_OK;
}

static int jit_function(jit_module* m, const char* name, hipFunction_t* fn)
{
    auto it = m->fns.find(name);
    if (it != m->fns.end()) { *fn = it->second; return MHX_OK; }
    hipError_t e = hipModuleGetFunction(fn, m->mod, name);
    if (e != hipSuccess) return mhx_fail(MHX_EJIT, "hipModuleGetFunction(%s): %s", name, hipGetErrorString(e));
    m->fns[name] = *fn;
    return MHX_OK;
}
// let a kernel (pre-built, or a hipFunction_t of a run-time module) use `lds_bytes` of dynamic LDS; what a refusal means is the caller's
static int kernel_lds_limit(const void* fn, size_t lds_bytes, const char* what)
{
    if (lds_bytes && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
        return mhx_fail(MHX_EHIP, "%s: %zu bytes of LDS refused", what, lds_bytes);
    return MHX_OK;
}

// ---------------------------------------------------------------------------------------------
// targets
struct mhx_target : mhx_handle_hdr {
    mhx_ctx* ctx = nullptr;
    int kind = 0, dim = 0, nparams = 0;
    mhx_real cst = MHX_R(0.0);
    mhx_real* dparams = nullptr;
    std::string user_src;        // MHX_TARGET_USER
    int bandwidth = -1;          // CORR_GAUSS: largest r - c with A_rc != 0 (exact zeros only), -1 otherwise: a banded precision
                                 // factor (Markov / autoregressive model) lets the row products skip the zeros
    ~mhx_target() { if (dparams) (void)hipFree(dparams); }
};

static mhx_real target_const(int kind, int dim, const mhx_real* p)
{
    const double LOG_2PI = 1.8378770664093454835606594728112;
    double c = -0.5 * (double)dim * LOG_2PI;
    switch (kind) {
    case MHX_TARGET_CORR_GAUSS: {
        size_t off = 0;
        for (int i = 0; i < dim; ++i) { c += std::log((double)p[off + i]); off += (size_t)i + 1; }
        break;
    }
    case MHX_TARGET_BANANA: c -= 0.5 * std::log(100.0); break;
    case MHX_TARGET_FUNNEL: c -= std::log(3.0); break;
    case MHX_TARGET_IID_NORMAL:
    case MHX_TARGET_USER: c = 0.0; break;
    default: break;
    }
    return (mhx_real)c;
}

static int target_upload(mhx_target* t, const mhx_real* params, size_t nparams)
{
    t->nparams = (int)nparams;
    // one dummy element keeps the pointer valid for kinds without parameters
    const size_t n = nparams ? nparams : 1;
    HIP_TRY(hipMalloc(&t->dparams, n * sizeof(mhx_real)));
    if (nparams) COPY_SYNC(t->ctx->stream, t->dparams, params, nparams * sizeof(mhx_real), hipMemcpyHostToDevice);
    else HIP_TRY(hipMemsetAsync(t->dparams, 0, sizeof(mhx_real), t->ctx->stream));
    return MHX_OK;
}

int api_target_builtin(mhx_ctx* ctx, int kind, int dim, const mhx_real* params, size_t nparams,
                                  mhx_target** out)
{
    if (!ctx || !out) return mhx_fail(MHX_EINVAL, "mhx_target_builtin: NULL argument");
    if (dim <= 0) return mhx_fail(MHX_EINVAL, "mhx_target_builtin: dim must be positive, got %d", dim);
    if (nparams && !params) return mhx_fail(MHX_EINVAL, "mhx_target_builtin: params is NULL");
    const size_t tri = (size_t)dim * ((size_t)dim + 1) / 2;
    switch (kind) {
    case MHX_TARGET_ISO_GAUSS:
        if (nparams) return mhx_fail(MHX_EINVAL, "ISO_GAUSS takes no parameters");
        break;
    case MHX_TARGET_CORR_GAUSS:
        if (nparams != tri) return mhx_fail(MHX_EINVAL, "CORR_GAUSS needs %zu packed-lower parameters, got %zu", tri, nparams);
        for (int i = 0; i < dim; ++i)
            if (!(params[(size_t)i * (i + 1) / 2 + i] > MHX_R(0.0)))
                return mhx_fail(MHX_ENOTPD, "CORR_GAUSS: diagonal %d of inv(chol(Sigma)) is not positive", i);
        break;
    case MHX_TARGET_IID_NORMAL:
        if (dim != 2) return mhx_fail(MHX_EINVAL, "IID_NORMAL is a 2-parameter (mu, sigma) model, dim=%d", dim);
        if (nparams < 1) return mhx_fail(MHX_EINVAL, "IID_NORMAL needs at least one data point");
        break;
    case MHX_TARGET_BANANA:
        if (dim < 2 || nparams != 1) return mhx_fail(MHX_EINVAL, "BANANA needs dim >= 2 and params = {b}");
        break;
    case MHX_TARGET_FUNNEL:
        if (dim < 2 || nparams != 0) return mhx_fail(MHX_EINVAL, "FUNNEL needs dim >= 2 and no parameters");
        break;
    default:
        return mhx_fail(MHX_EINVAL, "mhx_target_builtin: unknown kind %d", kind);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<mhx_target> t(new mhx_target);
    t->dtype = ctx->dtype;
    t->ctx = ctx;
    t->kind = kind;
    t->dim = dim;
    t->cst = target_const(kind, dim, params);
    if (kind == MHX_TARGET_CORR_GAUSS) {
        int bw = 0;
        size_t off = 0;
        for (int r = 0; r < dim; ++r) {
            for (int c = 0; c < r - bw; ++c) if (params[off + c] != MHX_R(0.0)) { bw = r - c; break; }
            off += (size_t)r + 1;
        }
        t->bandwidth = bw;
    }
    int rc = target_upload(t.get(), params, nparams);
    if (rc) return rc;
    *out = t.release();
    return MHX_OK;
}

static std::string jit_source(const mhx_target* t, const char* family_header)
{
    std::string s = "#include \"mhx_device_math.h\"\n";
    if (t->kind == MHX_TARGET_USER) {
        s += "#line 1 \"user_logdensity.hip\"\n";
        s += t->user_src;
        s += "\n#define MHX_HAVE_USER_TARGET 1\n";
    }
    s += "#include \"";
    s += family_header;
    s += "\"\n";
    return s;
}

static int jit_generic_rwmh(const mhx_target* t, jit_module** m)
{
    return jit_compile(t->ctx, jit_source(t, "mhx_rwmh_kernels.h"),
                       {"MHX_JIT_RWMH_GENERIC=1", "MHX_JIT_TK=" + std::to_string(t->kind)}, m);
}

int api_target_from_hip_source(mhx_ctx* ctx, const char* src, int dim, const mhx_real* data,
                                          size_t ndata, mhx_target** out)
{
    if (!ctx || !src || !out) return mhx_fail(MHX_EINVAL, "mhx_target_from_hip_source: NULL argument");
    if (dim <= 0) return mhx_fail(MHX_EINVAL, "mhx_target_from_hip_source: dim must be positive");
    if (ndata && !data) return mhx_fail(MHX_EINVAL, "mhx_target_from_hip_source: data is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<mhx_target> t(new mhx_target);
    t->dtype = ctx->dtype;
    t->ctx = ctx;
    t->kind = MHX_TARGET_USER;
    t->dim = dim;
    t->cst = MHX_R(0.0);
    t->user_src = src;
    int rc = target_upload(t.get(), data, ndata);
    if (rc) return rc;
    // compile now so that a bad source is reported at model construction, like a MethodError would be
    jit_module* m = nullptr;
    rc = jit_generic_rwmh(t.get(), &m);
    if (rc) return rc;
    *out = t.release();
    return MHX_OK;
}

int api_target_destroy(mhx_target* t)
{
    if (!t) return MHX_OK;
    (void)hipSetDevice(t->ctx->device);
    delete t;
    return MHX_OK;
}

// Launch a kernel of a run-time module.  The arguments are taken BY VALUE, in the kernel's order and each of the kernel's parameter type
// up to const (a long where it says long, an int where it says int): the array of addresses hipModuleLaunchKernel wants is formed here.
template <class... A>
static int launch_module(hipFunction_t fn, dim3 grid, unsigned block, hipStream_t s, A... args)
{
    static_assert(((!std::is_same<A, void**>::value) && ...), "launch_module takes the kernel's arguments, not an array of their addresses");
    void* params[] = {(void*)&args...};
    HIP_TRY(hipModuleLaunchKernel(fn, grid.x, grid.y, grid.z, block, 1, 1, 0, s, params, nullptr));
    return MHX_OK;
}

int api_target_eval(mhx_ctx* ctx, const mhx_target* t, const mhx_real* x, int n, mhx_real* lp)
{
    if (!ctx || !t || !x || !lp || n <= 0) return mhx_fail(MHX_EINVAL, "mhx_target_eval: bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    mhx_real *dx = nullptr, *dlp = nullptr;
    const size_t nx = (size_t)t->dim * (size_t)n;
    HIP_TRY(hipMalloc(&dx, nx * sizeof(mhx_real)));
    HIP_TRY(hipMalloc(&dlp, (size_t)n * sizeof(mhx_real)));
    int rc = MHX_OK;
    do {
        if (hipMemcpyAsync(dx, x, nx * sizeof(mhx_real), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { rc = mhx_fail(MHX_EHIP, "H2D copy failed"); break; }
        const unsigned grid = (unsigned)((n + 255) / 256);
        int d = t->dim, kind = t->kind, np = t->nparams, lanes = 1;
        mhx_real cst = t->cst;
        const mhx_real* tp = t->dparams;
        if (t->kind == MHX_TARGET_USER) {
            jit_module* m = nullptr;
            hipFunction_t fn;
            if ((rc = jit_generic_rwmh(t, &m))) break;
            if ((rc = jit_function(m, "mhx_jit_target_eval", &fn))) break;
            if ((rc = launch_module(fn, grid, 256, ctx->stream, dx, dlp, n, d, kind, tp, np, cst, lanes))) break;
        } else {
            hipLaunchKernelGGL(k_target_eval, dim3(grid), dim3(256), 0, ctx->stream, dx, dlp, n, d, kind, tp, np, cst, lanes);
        }
        if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess) { rc = mhx_fail(MHX_EHIP, "target_eval kernel failed"); break; }
        if (hipMemcpyAsync(lp, dlp, (size_t)n * sizeof(mhx_real), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = mhx_fail(MHX_EHIP, "D2H copy failed"); break; }
    } while (0);
    (void)hipFree(dx);
    (void)hipFree(dlp);
    return rc;
}

// ---------------------------------------------------------------------------------------------
// runs
// RUN_DERIVED (mhx_api_derive.inc): a sample tensor and nothing else -- no target, no sampler state; dim, n, n_saved, d_samples, ctx
// and the seed and first_id inherited from its source (what a predictive map of it keys its streams by) are its only fields in use.  The entry points that step or read sampler state refuse it in mhx_abi.cpp (api_run_is_derived).
enum run_kind { RUN_RWMH = 0, RUN_EMCEE = 1, RUN_RAM = 2, RUN_MALA = 3, RUN_DERIVED = 4 };
// The kernel form of a run.  The numbers are frozen: they travel as mhx_stats.kernel_variant (described at include/mhx.h:403), in
// ckpt_header.variant, and the host mirrors and bench.py read them.
enum kernel_form {
    KF_GENERIC = 0,         // run-time dimension, state in HBM
    KF_REG = 1,             // pre-built register kernel
    KF_REG_JIT = 2,         // run-time specialised register kernel
    KF_COOP = 3,            // pre-built cooperative kernel
    KF_COOP_JIT = 4,        // run-time specialised cooperative kernel
    KF_DENSE_COOP = 5,      // cooperative RWMH kernel with dense factor images in LDS
    KF_EMCEE_PERSIST = 6,   // a small ensemble as one persistent block
    KF_EMCEE_SEQ = 7,       // the reference's sequential ensemble sweep
    KF_MFMA = 8,            // matrix-core RWMH / MALA
    KF_EMCEE_SCAL = 9,      // scalar-factor form of the stretch move
    KF_EMCEE_MFMA = 10,     // matrix-core form of the stretch move
    KF_WAVE = 11,           // a wave per chain
    KF_RAM_DEFER = 12,      // RAM with a deferred factor
    KF_FAMILY = 13,         // a proposal of univariate family components: specialised register form or state in HBM
    KF_COND = 14,           // ... whose parameters are a function of the state (a conditional proposal): the same two forms
    KF_COMPOSITE = 15,      // ... and whose kind, symmetric flag and parameter map vary per block of components (a composite proposal)
    KF_TEMPERED = 16,       // parallel tempering of the plain random walk: specialised register form or state in HBM (mhx_api_tempered.inc)
    KF_TEMPERED_ADAPT = 17, // ... whose ladders tune their temperatures from their swaps while the run warms up: the same two forms
    KF_TEMPERED_ANCHOR = 18, // ... whose rungs temper towards a normalised reference density, down to beta = 0: the same two forms
    KF_ADAPTIVE = 19,       // the plain random walk whose chains tune their own proposal while the run warms up, then freeze it: two
                            // phases, each the specialised register form or state in HBM (mhx_api_adaptive.inc)
};

// One kernel of a run, ready to launch: everything the host needs for it, filled ONCE, in the branch of a create function that
// chooses the run's form, and launched by `launch` below.  No sampling call works a grid, a block size or an
// LDS size out again, and a new kernel form adds one record where it is chosen.
#define MHX_LAUNCH_MAX_TAIL 10
struct launch_rec {
    const void* fn = nullptr;            // the kernel: a pre-built __global__ function, or
    hipFunction_t mod_fn = nullptr;      // ... a kernel of a run-time module
    unsigned block = 64;                 // threads per block
    size_t lds = 0;                      // dynamic LDS bytes: the size rec_bind had the kernel allowed IS the size launched
    int per_block = 64;                  // chains (walkers) per block
    unsigned grid_round = 1;             // the grid is rounded up to a multiple of this (8: the kernels with an XCD-aware block -> chain map)
    void* tail[MHX_LAUNCH_MAX_TAIL] = {};   // the arguments after the per-launch block: ADDRESSES of members of the run, whose values are
    int ntail = 0;                          // fixed for its life (tp, d_pvec, d_fam, ...)
    const char* what = "";               // for messages
    explicit operator bool() const { return fn || mod_fn; }
};
static launch_rec rec_shape(const char* what, unsigned block, int per_block, size_t lds, std::initializer_list<const void*> tail, unsigned grid_round = 1)
{
    launch_rec k;
    k.what = what; k.block = block; k.per_block = per_block; k.lds = lds; k.grid_round = grid_round;
    for (const void* p : tail) k.tail[k.ntail++] = const_cast<void*>(p);
    return k;
}
// the record's kernel: a pre-built function / the kernel `name` of a run-time module, allowed the record's own LDS size
static int rec_bind(launch_rec* k, const void* fn)
{
    k->fn = fn; k->mod_fn = nullptr;
    return kernel_lds_limit(fn, k->lds, k->what);
}
static int rec_bind(launch_rec* k, jit_module* m, const char* name)
{
    k->fn = nullptr;
    const int rc = jit_function(m, name, &k->mod_fn);
    return rc ? rc : kernel_lds_limit((const void*)k->mod_fn, k->lds, k->what);
}
// launch it for `n_items` chains (walkers), `grid_y` ensembles; `args_block`: the kernel's first argument, the per-launch block
static int launch(const launch_rec& k, hipStream_t s, long n_items, unsigned grid_y, void* args_block)
{
    if (!k) return mhx_fail(MHX_ESTATE, "%s: the run holds no such kernel", k.what);
    void* params[1 + MHX_LAUNCH_MAX_TAIL] = {args_block};
    for (int i = 0; i < k.ntail; ++i) params[1 + i] = k.tail[i];
    unsigned grid = (unsigned)((n_items + k.per_block - 1) / k.per_block);
    grid = (grid + k.grid_round - 1) / k.grid_round * k.grid_round;
    if (k.mod_fn) HIP_TRY(hipModuleLaunchKernel(k.mod_fn, grid, grid_y, 1, k.block, 1, 1, (unsigned)k.lds, s, params, nullptr));
    else HIP_TRY(hipLaunchKernel(k.fn, dim3(grid, grid_y), dim3(k.block), params, k.lds, s));
    return MHX_OK;
}

struct mhx_run : mhx_handle_hdr {
    mhx_ctx* ctx = nullptr;
    const mhx_target* target = nullptr;
    int kind = RUN_RWMH;
    int dim = 0, n = 0;                  // n = chains / walkers (an Ensemble run: all walkers of all its ensembles)
    int ens_w = 0, n_ens = 1;            // Ensemble runs: walkers per ensemble, ensembles (ids first_id .. first_id + n_ens - 1)
    uint64_t seed = 0, first_id = 0;
    int flags = 0;
    bool initialised = false;
    uint64_t tau = 0;                    // transitions done so far (RNG step counter)
    // rwmh
    int prop_kind = 0;
    mhx_real prop_scale = MHX_R(1.0);
    mhx_real* d_pvec = nullptr;
    // emcee
    mhx_real stretch = MHX_R(2.0);
    mhx_real* d_xw = nullptr;               // walker-major copy [W][round4(dim)]: the state while the cooperative kernel runs
    mhx_real* d_pmean = nullptr;            // drifting walk: mu[dim] then 2 L^-1 mu [dim]
    mhx_real* d_mfma_img = nullptr;         // streamed matrix-core kernels: the operand images [target][proposal] in global memory
    mhx_real* d_mfma_img2 = nullptr;        // ... the second of them (inside d_mfma_img: not freed)
    mhx_real* d_qx = nullptr;               // static proposal: logpdf of the proposal at each chain's state (up to its constant)
    mhx_fam_comp* d_fam = nullptr;          // KF_FAMILY: the component table [dim]
    bool fam_reg = false;                   // ... stepped by the specialised register form, else by the state-in-HBM form (sizes d_cond_p; stats)
    int fam_symmetric = 0;                  // ... a random walk declared symmetric: no ratio
    // KF_COND (mhx_api_cond.inc): d_fam, fam_reg and fam_symmetric as above, and
    std::string cond_src;                   // the parameter map's source (MHX_PROPOSAL_PARAMS)
    mhx_real* d_cond_data = nullptr;        // its data block
    int cond_ndata = 0;
    int cond_static = 0;                    // MHX_FLAG_STATIC_PROPOSAL, as the state-in-HBM form's argument
    mhx_real* d_cond_p = nullptr;           // [2 dim][n] p(x) of the check kernel; the state-in-HBM form: [4 dim][n], p(x) then p(y)
    int* d_cond_bad = nullptr;              // chains whose p(x) the last check found invalid
    hipFunction_t jit_cond_check = nullptr;
    // KF_COMPOSITE (mhx_api_composite.inc): everything of KF_COND, and
    int* d_cmp_tab = nullptr;               // {kind bit, mapped mask} per component, then {first, count, flags} per block
    int cmp_nblocks = 0;
    bool cmp_mapped = false;                // some parameter is mapped: the first state must be given
    // KF_TEMPERED (mhx_api_tempered.inc): fam_reg as above, and
    int tmp_R = 0;                          // rungs per ladder (0: not a tempered run)
    int tmp_swap_every = 0;                 // a swap round after every so many transitions (0: none)
    mhx_real* d_ttab = nullptr;             // beta[R] | dbeta[R] | sig[R] or sig[R][dim]
    uint32_t* d_swapc = nullptr;            // [2][n] swap attempts, swaps of pair (r, r + 1), kept by the lower slot
    // KF_TEMPERED_ADAPT: everything of KF_TEMPERED but d_ttab, and
    bool tmp_adapt = false;
    mhx_real* d_tadapt = nullptr;           // rho[n] | beta[n] | rho0[n] | gamma[adapt_steps / swap_every]
    mhx_tmp_adapt tmp_ad{};                 // the step kernel's adaptation block: pointers into d_tadapt and d_pvec, the constants
    // KF_TEMPERED_ANCHOR: everything of KF_TEMPERED, and
    bool tmp_anchor = false;
    bool tmp_beta_end_zero = false;         // the ladder reaches the reference itself (mhx_run_evidence)
    mhx_real* d_tanchor = nullptr;          // omb[R] | m[dim] | w[dim]
    mhx_tmp_anchor tmp_an{};                // the step kernel's reference block: pointers into d_tanchor, lc
    // KF_ADAPTIVE (mhx_api_adaptive.inc): `step` is the adapting phase's kernel, `step_frozen` the frozen phase's
    bool adp = false;
    uint64_t adp_steps = 0;                 // transitions 1 .. adp_steps adapt
    int adp_shape = 0;                      // the per-coordinate standard deviations adapt too
    int adp_perk = 0;                       // eff has a row per coordinate (DIAG or shape), else one row
    bool adp_reg = false, adp_frozen_reg = false;   // the phase is stepped by its register form
    mhx_real* d_adp = nullptr;              // lam[n] | eff[n or dim n] | (shape) m, v, sig [dim n] each | gamma[adp_steps] | s, vlo, vhi [dim] each
    uint32_t* d_acc_freeze = nullptr;       // [n] the accept counters as they stood after transition adp_steps
    mhx_adp adp_a{};                        // the adapting kernels' block: pointers into d_adp, the constants
    // mala
    mhx_real mala_sigma = MHX_R(1.0);
    mhx_real *d_gx = nullptr, *d_gy = nullptr, *d_z = nullptr;
    // ram
    mhx_ram_cfg ramcfg{};
    mhx_real* d_S = nullptr;                        // packed factors [n][2][tri_pad]: both buffers of a chain side by side
    unsigned char* d_Ssel = nullptr;             // which buffer holds chain c's current factor
    unsigned char* d_status = nullptr;
    mhx_real *d_dmin = nullptr, *d_dmax = nullptr;  // [dim][n]
    mhx_real* d_eta = nullptr;                      // adaptation step sizes of the current launch
    mhx_real* d_loga = nullptr;                     // [n] log acceptance ratio of each chain's latest transition
    mhx_real* d_defer = nullptr;                    // RAM, deferred-factor form: [n][MHX_RAM_DEFER_REALS] pending updates
    int defer_R = 0;                                // rows per lane of that form's kernel (0: the sweep form)
    double last_eta = 0.0;                          // step size of the latest adapting transition (state.η; 0 before any)
    mhx_real* d_rec_loga = nullptr;                 // [n_saved][n] logα of every recorded transition of the last sampling call
    mhx_real* rec_loga_view = nullptr;              // where slot 0 of the current launches lands in it (slab-wise calls)
    size_t rec_loga_cap = 0;
    // RAM: the factors of a few watched chains after every recorded step (mhx_ram_watch_factors)
    int32_t* d_watch_chains = nullptr;
    mhx_real* d_watch = nullptr;                    // [n recorded][watch_n][dim (dim + 1) / 2], packed row-major
    size_t watch_cap = 0;
    int watch_n = 0;
    long watch_count = 0;
    std::vector<double> rec_eta;                    // [n_saved] state.η after every recorded transition
    int64_t rec_n = 0;                              // recorded transitions held by the two above
    size_t eta_cap = 0;
    // state
    mhx_real *d_x = nullptr, *d_lp = nullptr, *d_ybuf = nullptr;
    uint32_t* d_acc = nullptr;
    unsigned char* d_last = nullptr;
    unsigned long long* d_acc_total = nullptr;
    // mhx_run_sample reads d_acc_total ONCE per call: `acc_total_host` is the total the previous call read (valid until the counter
    // is reset or a call fails half way), the new one lands in the page-locked `acc_total_pin` by a copy ahead of the call's one sync
    unsigned long long acc_total_host = 0;
    bool acc_total_known = false;
    unsigned long long* acc_total_pin = nullptr;
    // sample buffer of the last mhx_run_sample
    mhx_real* d_samples = nullptr;
    unsigned char* d_accepted = nullptr;
    size_t samples_cap = 0, accepted_cap = 0;
    int64_t n_saved = 0;
    // running moments of the last mhx_run_sample(save = 2)
    mhx_real *d_mom_mean = nullptr, *d_mom_m2 = nullptr;
    size_t mom_cap = 0, mom_cap2 = 0;
    uint64_t mom_n = 0;                  // states folded in so far
    bool moments_mode = false;
    std::vector<std::string> coop_defs;  // defines of the cooperative kernel (its moments twin differs in MHX_JIT_MOM)
    // kernel choice: the form (variant) and the launch records of its kernels.  The records' trailing arguments point INTO this
    // struct (k_tp and the members named at launch_rec::tail): a run is never copied or moved
    const mhx_real* k_tp = nullptr;      // target->dparams, as a kernel argument (run_alloc_state)
    launch_rec step;                     // the step kernel (an ensemble: the half-step, or the sequential sweep)
    launch_rec step_k8;                  // KF_WAVE: the K = 8 build of the wave-per-chain kernel
    launch_rec step_frozen;              // KF_ADAPTIVE: the frozen phase's kernel (transitions after adp_steps)
    launch_rec step_mom;                 // KF_COOP / KF_COOP_JIT: the running-moments twin (pre-built, or built by the first MHX_SAVE_MOMENTS call)
    launch_rec sweep;                    // an ensemble: the stretch move as ONE launch per sweep (mhx_emcee_coop_sweep_body); state double-buffered
    launch_rec persist;                  // ... a small one as one persistent block (mhx_emcee_persist_body): a whole call per launch
    bool sweep_mixed = false;            // ... the sweep kernel's blocks take walkers of both halves (scalar-factor form), not one half each
    int normal_gen = MHX_GEN_BOX_MULLER; // how stream bits become standard normals (MHX_FLAG_ZIGGURAT: the table ziggurat, fp64)
    bool coop_pairs = false;             // the cooperative kernel as generator / consumer wave pairs (the form's name; not the moments twin)
    int coop_tr = 0;                     // the cooperative kernel's LDS holds the row-transposition buffer of the one / two-chains-per-wave shapes
    int coop_L = 1;                      // lanes per chain (reduction shape of the separable targets)
    int emcee_band = -1;                 // bandwidth of the precision factor the cooperative stretch move exploits (-1: dense form)
    int coop_waves = MHX_EMCEE_COOP_WAVES;  // waves per block of the cooperative stretch move (tuning knob MHX_EMCEE_WAVES)
    size_t emcee_stamp_words = 0;        // MHX_EMCEE_STAMPS (tools): 64-bit words of the stamp buffer in d_ybuf
    int emcee_wpb = 64;                  // walkers per block of the scalar-factor form
    mhx_real *d_xw2 = nullptr, *d_lp2 = nullptr;   // the buffers the next launch of `sweep` writes (swapped with d_xw / d_lp after every launch)
    bool emcee_preload = false;          // the half-step kernel takes its hot arguments as preloaded scalars (MHX_JIT_PRELOAD)
    int variant = KF_GENERIC;            // kernel_form
    int wave_k = 4;                      // KF_WAVE: candidates per round of the next call (8 after a call that accepted < 1 step in 8)
    hipFunction_t jit_init = nullptr;    // a user target's initial kernel (256 threads, no LDS)
    mhx_stats stats{};
    mhx_host_stats host_stats{};         // what the last mhx_run_sample_to_host moved

    ~mhx_run()
    {
        void* ptrs[] = {d_pvec, d_S, d_Ssel, d_status, d_dmin, d_dmax, d_eta, d_x, d_lp, d_ybuf,
                        d_acc, d_last, d_acc_total, d_samples, d_accepted, d_mom_mean, d_mom_m2, d_gx, d_gy, d_z, d_pmean, d_qx, d_xw, d_loga, d_mfma_img, d_rec_loga,
                        d_watch_chains, d_watch, d_xw2, d_lp2, d_defer, d_fam, d_cond_data, d_cond_p, d_cond_bad, d_cmp_tab, d_ttab, d_swapc, d_tadapt, d_tanchor, d_adp, d_acc_freeze};
        for (void* p : ptrs) if (p) (void)hipFree(p);
        if (acc_total_pin) (void)hipHostFree(acc_total_pin);
    }
};

static int run_alloc_state(mhx_run* r)
{
    const size_t n = (size_t)r->n, d = (size_t)r->dim;
    r->k_tp = r->target->dparams;
    HIP_TRY(hipMalloc(&r->d_x, d * n * sizeof(mhx_real)));
    HIP_TRY(hipMalloc(&r->d_lp, n * sizeof(mhx_real)));
    HIP_TRY(hipMalloc(&r->d_acc, n * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&r->d_last, n));
    HIP_TRY(hipMalloc(&r->d_acc_total, sizeof(unsigned long long)));
    HIP_TRY(hipHostMalloc((void**)&r->acc_total_pin, sizeof(unsigned long long), hipHostMallocDefault));
    HIP_TRY(hipMemsetAsync(r->d_acc, 0, n * sizeof(uint32_t), r->ctx->stream));
    HIP_TRY(hipMemsetAsync(r->d_last, 0, n, r->ctx->stream));
    HIP_TRY(hipMemsetAsync(r->d_acc_total, 0, sizeof(unsigned long long), r->ctx->stream));
    return MHX_OK;
}

static mhx_rwmh_args rwmh_args(const mhx_run* r)
{
    mhx_rwmh_args a;
    memset(&a, 0, sizeof a);
    a.x = r->d_x; a.lp = r->d_lp; a.acc_count = r->d_acc; a.acc_total = r->d_acc_total;
    a.samples = r->d_samples; a.accepted = r->d_accepted; a.last_acc = r->d_last; a.ybuf = r->d_ybuf;
    a.seed = r->seed; a.first_chain = r->first_id;
    a.nchains = r->n; a.ld = r->n; a.dim = r->dim;
    a.target_kind = r->target->kind; a.ntparams = r->target->nparams; a.tconst = r->target->cst;
    a.prop_kind = r->prop_kind; a.pscale = r->prop_scale;
    a.save_next = MHX_NO_SAVE; a.thinning = 1;
    a.reduce_lanes = r->coop_L;
    if (r->moments_mode) { a.mom_mean = r->d_mom_mean; a.mom_m2 = r->d_mom_m2; a.mom_n0 = (mhx_u32)r->mom_n; }
    a.pmean = r->d_pmean;
    a.qx = r->d_qx;
    a.normal_gen = r->normal_gen;
    a.tr_lds = r->coop_tr;
    return a;
}

__global__ void __launch_bounds__(256)
k_rwmh_whiten(const mhx_rwmh_args a, const mhx_real* __restrict__ pvec)
{
    mhx_rwmh_whiten_body(a, pvec);
}
// logpdf of a static proposal at the current states (after init / set_state)
static int cond_check(mhx_run* r);
static int rwmh_whiten(mhx_run* r)
{
    if (r->variant == KF_COND || r->variant == KF_COMPOSITE) return cond_check(r);         // no cached q(x); p(x) must be a distribution's
    if (!r->d_qx) return MHX_OK;
    mhx_rwmh_args a = rwmh_args(r);
    if (r->variant == KF_FAMILY)
        hipLaunchKernelGGL(k_fam_q, dim3((unsigned)((r->n + 255) / 256)), dim3(256), 0, r->ctx->stream, a, (const mhx_fam_comp*)r->d_fam);
    else
    hipLaunchKernelGGL(k_rwmh_whiten, dim3((unsigned)((r->n + 255) / 256)), dim3(256), 0, r->ctx->stream, a, r->d_pvec);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    return MHX_OK;
}

// register budgets: a double takes two VGPRs
#define MHX_REG_MAX_DIM (MHX_REAL64 ? 80 : 160)
#define MHX_REG_MAX_DIM_DENSE (MHX_REAL64 ? 48 : 96)
#define MHX_REG_XR_ALL (MHX_REAL64 ? 64 : 128)          // up to here the whole state stays in registers beside the candidate
#define MHX_REG_XR_CAP (MHX_REAL64 ? 60 : 120)          // above: this many coordinates of it, the rest in LDS
#define MHX_DENSE_COOP_MAX_DIM 256
#define MHX_EMCEE_MAX_BAND 8                 // widest band the band form of the cooperative stretch move is specialised for
#define MHX_LDS_PER_BLOCK 163840             // gfx950: 160 KB of LDS, all of it available to one block
// lanes per chain of the dense cooperative kernel: at most 12.5 rows of a factor per lane
static int dense_coop_lanes(int d) { int L = 2; while ((MHX_REAL64 ? 4 : 2) * d > 25 * L && L < 64) L *= 2; return L; }
// dynamic LDS of the dense cooperative kernel: the candidate rows of a 4-wave block + `nimages` factor images
static size_t dense_coop_lds_bytes(int d, int L, int nimages, int waves = MHX_EMCEE_COOP_WAVES)
{
    long total4 = 0;
    for (int m = 0; m * L < d; ++m) total4 += (long)((std::min(L * (m + 1), d) + 3) / 4) * L;
    const long rows4 = (long)waves * (64 / L) * ((((d + 3) & ~3) + 4) / 4);
    return (size_t)(rows4 + nimages * total4) * 4 * sizeof(mhx_real);
}
static bool dense_coop_fits(int d, int L, int nimages)
{
    if (L < 2 || L > 64 || (L & (L - 1)) || L > d) return true;      // let the caller report the bad shape
    return dense_coop_lds_bytes(d, L, nimages) <= MHX_LDS_PER_BLOCK;
}

// the matrix-core kernel (mhx_rwmh_mfma_kernels.h): 4 lanes per chain, NS = ceil(d/4) reals of state and of candidate per
// lane, `nimages` operand images in LDS
#define MHX_MFMA_MAX_NS (MHX_REAL64 ? 44 : 64)
static size_t mfma_image_reals(int d)
{
    const int NS = (d + 3) / 4, NT = (d + 15) / 16;
    const int last = std::min(4 * NT, NS);
    return (size_t)(2 * (NT - 1) * NT + 4 * ((last + 3) / 4)) * 64;
}
static size_t mfma_image_reals_T(int d) { const int NT = (d + 15) / 16; return (size_t)(NT * (NT + 1) / 2) * 256; }   // the image of A^T
static bool mfma_fits(const mhx_ctx* ctx, int d, int reduce_lanes, int nimages)
{
    // (NO_MFMA, tuning knob: the vector kernel instead)
    return (reduce_lanes == 0 || reduce_lanes == 4) && d >= 16 && (d + 3) / 4 <= MHX_MFMA_MAX_NS && !opt_on(ctx, "NO_MFMA") &&
           nimages * mfma_image_reals(d) * sizeof(mhx_real) <= MHX_LDS_PER_BLOCK;
}
// streamed images (larger than a block's LDS): two ring buffers of whole 256-thread rounds of 16-byte pieces of the largest chunk
// -- a tile pair, or (the largest dimensions) a single tile with the chain state re-read from its slab instead of held in registers
#define MHX_MFMA_STREAM_MAX_NS (MHX_REAL64 ? 64 : 100)
#define MHX_MFMA_XMEM_MAX_NS (MHX_REAL64 ? 128 : 250)   // fp64 d <= 512, fp32 d <= 1000: the candidate alone fills the registers of a wave (1 per SIMD)
static size_t mfma_ring_bytes(int d, bool pair = true)
{
    const int NS = (d + 3) / 4, NT = (d + 15) / 16;
    auto groups = [&](int t) { return (std::min(4 * (t + 1), NS) + 3) / 4; };
    int maxg = 0;
    if (pair) for (int p = 0; 2 * p < NT; ++p) maxg = std::max(maxg, groups(2 * p) + (2 * p + 1 < NT ? groups(2 * p + 1) : 0));
    else for (int t = 0; t < NT; ++t) maxg = std::max(maxg, groups(t));
    const int p16 = (int)(4 * sizeof(mhx_real)) / 16;
    const int pf = (maxg * 64 * p16 + 64 * MHX_MFMA_WAVES - 1) / (64 * MHX_MFMA_WAVES);
    return (size_t)2 * pf * 64 * MHX_MFMA_WAVES * 16;
}
// 0 = no, 1 = tile pairs + state in registers, 2 = single tiles + state in HBM
static int mfma_stream_mode(const mhx_ctx* ctx, int d, int reduce_lanes)
{
    if (!((reduce_lanes == 0 || reduce_lanes == 4) && d >= 16) || opt_on(ctx, "NO_MFMA")) return 0;
    const int NS = (d + 3) / 4;
    if (NS <= MHX_MFMA_STREAM_MAX_NS && mfma_ring_bytes(d, true) <= MHX_LDS_PER_BLOCK) return 1;
    if (NS <= MHX_MFMA_XMEM_MAX_NS && mfma_ring_bytes(d, false) <= MHX_LDS_PER_BLOCK) return 2;
    return 0;
}
static bool mfma_stream_fits(const mhx_ctx* ctx, int d, int reduce_lanes) { return mfma_stream_mode(ctx, d, reduce_lanes) != 0; }
static int mfma_waves(const mhx_ctx* ctx, int d)
{
    const int NS = (d + 3) / 4;
    if (const char* w = opt(ctx, "MFMA_WAVES")) return std::max(1, atoi(w));        // tuning knob
    return MHX_REAL64 ? (NS <= 25 ? 2 : 1) : (NS <= 25 ? 3 : (NS <= 40 ? 2 : 1));
}

int api_rwmh_create(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, mhx_run** out)
{
    if (!ctx || !t || !cfg || !out) return mhx_fail(MHX_EINVAL, "mhx_rwmh_create: NULL argument");
    if (cfg->dim != t->dim)
        return mhx_fail(MHX_EINVAL, "mhx_rwmh_create: proposal dim %d != model dim %d", cfg->dim, t->dim);
    if (cfg->nchains <= 0) return mhx_fail(MHX_EINVAL, "mhx_rwmh_create: nchains must be positive");
    const int d = cfg->dim;
    const mhx_real* cfg_vec = (const mhx_real*)cfg->proposal_vec;       // reals of this instantiation (include/mhx.h)
    const mhx_real* cfg_mean = (const mhx_real*)cfg->proposal_mean;
    size_t nvec = 0;
    switch (cfg->proposal_kind) {
    case MHX_PROP_ISO:
        if (!(cfg->proposal_scale > 0.0)) return mhx_fail(MHX_EINVAL, "ISO proposal needs a positive scale");
        break;
    case MHX_PROP_DIAG: nvec = (size_t)d; break;
    case MHX_PROP_DENSE: nvec = (size_t)d * ((size_t)d + 1) / 2; break;
    default: return mhx_fail(MHX_EINVAL, "mhx_rwmh_create: unknown proposal kind %d", cfg->proposal_kind);
    }
    if (nvec && !cfg_vec) return mhx_fail(MHX_EINVAL, "mhx_rwmh_create: proposal_vec is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<mhx_run> r(new mhx_run);
    r->dtype = ctx->dtype;
    r->ctx = ctx; r->target = t; r->kind = RUN_RWMH;
    r->dim = d; r->n = cfg->nchains; r->seed = cfg->seed; r->first_id = cfg->first_chain;
    r->flags = cfg->flags;
    r->prop_kind = cfg->proposal_kind; r->prop_scale = (mhx_real)cfg->proposal_scale;
    HIP_TRY(hipMalloc(&r->d_pvec, (nvec ? nvec : 1) * sizeof(mhx_real)));
    if (nvec) COPY_SYNC(ctx->stream, r->d_pvec, cfg_vec, nvec * sizeof(mhx_real), hipMemcpyHostToDevice);
    int rc = run_alloc_state(r.get());
    if (rc) return rc;
    // drifting random walk: keep mu and 2 L^-1 mu (double arithmetic on the host, rounded once) and use the
    // generic kernel, the only one that evaluates the Hastings ratio
    bool drift = false;
    if (cfg_mean)
        for (int k = 0; k < d; ++k) drift = drift || cfg_mean[k] != MHX_R(0.0);
    if (drift) {
        std::vector<mhx_real> pm(2 * (size_t)d);
        std::vector<double> m((size_t)d);
        size_t off = 0;
        for (int i = 0; i < d; ++i) {
            double acc = (double)cfg_mean[i];
            if (cfg->proposal_kind == MHX_PROP_ISO) m[i] = acc / (double)cfg->proposal_scale;
            else if (cfg->proposal_kind == MHX_PROP_DIAG) m[i] = acc / (double)cfg_vec[i];
            else {
                for (int j = 0; j < i; ++j) acc -= (double)cfg_vec[off + j] * m[j];
                m[i] = acc / (double)cfg_vec[off + i];
                off += (size_t)i + 1;
            }
            pm[i] = cfg_mean[i];
            pm[(size_t)d + i] = (mhx_real)(2.0 * m[i]);
        }
        HIP_TRY(hipMalloc(&r->d_pmean, pm.size() * sizeof(mhx_real)));
        COPY_SYNC(ctx->stream, r->d_pmean, pm.data(), pm.size() * sizeof(mhx_real), hipMemcpyHostToDevice);
    }
    // static (independence) proposal, src/proposal.jl:9-11,66-83: one more mhx_real of state per chain
    if (cfg->flags & MHX_FLAG_STATIC_PROPOSAL) HIP_TRY(hipMalloc(&r->d_qx, (size_t)r->n * sizeof(mhx_real)));
    // walks with a Hastings ratio run on the cooperative kernel (separable target, ISO / DIAG proposal) or on the
    // state-in-HBM kernel; the register kernels know the plain random walk only
    const int walk = (cfg->flags & MHX_FLAG_STATIC_PROPOSAL) ? MHX_WALK_STATIC : (drift ? MHX_WALK_DRIFT : MHX_WALK_PLAIN);

    // the register / cooperative kernels address a [dim+1][nchains] slab with 32-bit byte offsets
    if (((uint64_t)d + 1) * (uint64_t)r->n * (uint64_t)sizeof(mhx_real) >= (1ull << 32)) r->flags |= MHX_FLAG_GENERIC;
    // ---- kernel choice
    r->variant = KF_GENERIC;
    const int tk = t->kind, pk = r->prop_kind;
    // a launch record of this sampler: kernel(args, tparams, pvec)
    auto rec = [&](const char* what, unsigned block, int per_block, size_t lds, unsigned grid_round = 1) {
        return rec_shape(what, block, per_block, lds, {&r->k_tp, &r->d_pvec}, grid_round);
    };
    // (fp32, round 6: 256 layers, one Philox word per normal -- on the cooperative kernel, the register kernel and MALA's register kernel
    // like fp64; the check at the end of this function refuses a run whose kernel has no ziggurat form)
    if ((cfg->flags & MHX_FLAG_ZIGGURAT) && d >= (1 << 20))      // the retry blocks are numbered (normal index << 8 | attempt) in 28 bits
        return mhx_fail(MHX_EINVAL, "MHX_FLAG_ZIGGURAT: dim must be below 2^20");
    int regmax = opt_int(ctx, "REG_MAX_DIM", pk == MHX_PROP_DENSE ? MHX_REG_MAX_DIM_DENSE : MHX_REG_MAX_DIM);      // tuning knob
    const int nblk = (d + 3) / 4;
    const bool separable = tk == MHX_TARGET_ISO_GAUSS || tk == MHX_TARGET_BANANA || tk == MHX_TARGET_FUNNEL;
    // lanes per chain: cfg->reduce_lanes, or (auto) the smallest power of two that (a) keeps a lane's
    // blocks in registers (<= 13 blocks = 104 VGPRs of state) and (b) gives the chip >= 2 waves per SIMD
    // A wave per chain (KF_WAVE): the data-sum target of the README example with FEW chains -- the lanes split the likelihood's
    // terms (reduction shape 64).  Asked for (reduce_lanes = 64), or by default while every chain can have a wave to itself (<= 2 per
    // SIMD) and there are terms to split; the plain random walk, ISO / DIAG proposal, Box-Muller normals.
    if (tk == MHX_TARGET_IID_NORMAL && d == 2 && pk != MHX_PROP_DENSE && walk == MHX_WALK_PLAIN &&
        !(r->flags & (MHX_FLAG_GENERIC | MHX_FLAG_ZIGGURAT)) &&
        (cfg->reduce_lanes == 64 || (cfg->reduce_lanes == 0 && t->nparams >= 8 && chains_of_whole_run(ctx, r->n) <= 2048))) {
        r->step = r->step_k8 = rec("wave-per-chain kernel", 64, 1, 0);
        if ((rc = rec_bind(&r->step, (const void*)(pk == MHX_PROP_ISO ? k_rwmh_wave<MHX_PROP_ISO, 4> : k_rwmh_wave<MHX_PROP_DIAG, 4>)))) return rc;
        if ((rc = rec_bind(&r->step_k8, (const void*)(pk == MHX_PROP_ISO ? k_rwmh_wave<MHX_PROP_ISO, 8> : k_rwmh_wave<MHX_PROP_DIAG, 8>)))) return rc;
        r->variant = KF_WAVE;
        r->coop_L = 64;
    } else if (tk == MHX_TARGET_IID_NORMAL && cfg->reduce_lanes > 1) {
        return mhx_fail(MHX_EINVAL, "mhx_rwmh_create: the data-sum target knows reduce_lanes 0, 1 and 64 (a wave per chain: plain walk, "
                        "ISO / DIAG proposal, Box-Muller), got %d", cfg->reduce_lanes);
    }
    int L = 1;
    bool coop_one_lane = false;                       // a walk with a Hastings ratio on ONE lane per chain: still the cooperative body
    if (separable && pk != MHX_PROP_DENSE && !(r->flags & MHX_FLAG_GENERIC) && !(walk && (r->flags & MHX_FLAG_NO_JIT))) {
        if (cfg->reduce_lanes > 1 || (cfg->reduce_lanes == 1 && walk)) {
            L = cfg->reduce_lanes;
            if (L > 64 || (L & (L - 1))) return mhx_fail(MHX_EINVAL, "reduce_lanes must be a power of two <= 64, got %d", L);
        } else if (cfg->reduce_lanes == 0) {
            while (L < 64 && (nblk + L - 1) / L > MHX_COOP_NBL_AUTO) L *= 2;
            // the kernels are bound by VALU throughput, and every block slot of a lane costs a full Philox + Box-Muller
            // round whether it holds dimensions or padding: halve the lanes while that removes > 5 % of the slots and the
            // blocks still fit a lane (C2 in fp64: 4 lanes x 7 = 28 slots for 25 blocks -> 2 lanes x 13 = 26: +4 %)
            while (L > 1 && (nblk + L / 2 - 1) / (L / 2) <= MHX_COOP_NBL_MAX &&
                   (long)(L / 2) * ((nblk + L / 2 - 1) / (L / 2)) * 105 < (long)L * ((nblk + L - 1) / L) * 100) L /= 2;
            while (L < 64 && 2 * L <= nblk && chains_of_whole_run(ctx, r->n) * L / 64 < 2048) L *= 2;
            if ((nblk + L - 1) / L > MHX_COOP_NBL_MAX) L = 1;      // not even a whole wave holds the chain: state in HBM
        }
        // (the ziggurat generator lives in the cooperative body: a chain on ONE lane still runs it there)
        coop_one_lane = (walk || (cfg->flags & MHX_FLAG_ZIGGURAT)) && L == 1 && nblk <= MHX_COOP_NBL_MAX;
    } else if (((tk == MHX_TARGET_CORR_GAUSS) || (tk == MHX_TARGET_ISO_GAUSS && pk == MHX_PROP_DENSE)) &&
               !walk && !(r->flags & (MHX_FLAG_GENERIC | MHX_FLAG_NO_JIT)) && d >= 2 && d <= 4 * std::max(MHX_MFMA_STREAM_MAX_NS, MHX_MFMA_XMEM_MAX_NS) &&
               (cfg->reduce_lanes > 1 || (cfg->reduce_lanes == 0 && d >= 16)) &&
               (mfma_fits(ctx, d, cfg->reduce_lanes, (tk == MHX_TARGET_CORR_GAUSS ? 1 : 0) + (pk == MHX_PROP_DENSE ? 1 : 0)) ||
                mfma_stream_fits(ctx, d, cfg->reduce_lanes) ||
                dense_coop_fits(d, cfg->reduce_lanes > 1 ? cfg->reduce_lanes : dense_coop_lanes(d),
                                (tk == MHX_TARGET_CORR_GAUSS ? 1 : 0) + (pk == MHX_PROP_DENSE ? 1 : 0)))) {
        // a dense factor in play (dense Gaussian target, dense proposal, or both): the cooperative kernel of
        // mhx_rwmh_dense_kernels.h (L lanes per chain, factor images in LDS).  Lanes per chain by default: at most
        // 12.5 rows per lane (measured at 65 536 chains, dense target: d = 32 / 50 / 64 / 100 / 128 run 1.8e10 /
        // 8.5e9 / 6.8e9 / 2.9e9 / 2.0e9 steps/s; the lane-per-chain register kernel 1.4e10 / 7.2e9 / 4.9e9 / - / -;
        // more rows per lane than ~16 spill)
        // ONE factor for all chains makes the row products a GEMM over the chains of a wave: the matrix-core kernel
        // (reduction shape L = 4, bit-identical to the vector kernel in that shape) wherever its images and state fit
        const int nimg = (tk == MHX_TARGET_CORR_GAUSS ? 1 : 0) + (pk == MHX_PROP_DENSE ? 1 : 0);
        if (mfma_fits(ctx, d, cfg->reduce_lanes, nimg)) {
            jit_module* m = nullptr;
            const int waves = mfma_waves(ctx, d);
            rc = jit_compile(ctx, jit_source(t, "mhx_rwmh_mfma_kernels.h"),
                             {"MHX_JIT_RWMH_MFMA=1", "MHX_JIT_DIM=" + std::to_string(d), "MHX_JIT_PK=" + std::to_string(pk),
                              "MHX_JIT_TK=" + std::to_string(tk), "MHX_JIT_WAVES=" + std::to_string(waves)}, &m);
            // 16 chains per wave, the images resident in LDS
            launch_rec k = rec("matrix-core kernel", 64 * MHX_MFMA_WAVES, 16 * MHX_MFMA_WAVES, nimg * mfma_image_reals(d) * sizeof(mhx_real));
            if (rc == MHX_OK) rc = rec_bind(&k, m, "mhx_jit_rwmh_mfma");
            if (rc == MHX_OK) { r->step = k; r->variant = KF_MFMA; r->coop_L = 4; }
        }
        if (r->variant == KF_GENERIC && mfma_stream_fits(ctx, d, cfg->reduce_lanes)) {
            // the images do not fit a block's LDS: they stay in global memory (built once, here) and every block walks them
            // through an LDS ring, one tile pair at a time
            jit_module* m = nullptr;
            const int smode = mfma_stream_mode(ctx, d, cfg->reduce_lanes);
            // the kernel is fully unrolled over its tiles: lift hipcc's size limit for `#pragma unroll` (past it the candidate
            // would be indexed dynamically, i.e. live in scratch)
            rc = jit_compile(ctx, jit_source(t, "mhx_rwmh_mfma_kernels.h"),
                             {"MHX_JIT_RWMH_MFMA_STREAM=1", "MHX_JIT_DIM=" + std::to_string(d), "MHX_JIT_PK=" + std::to_string(pk),
                              "MHX_JIT_TK=" + std::to_string(tk), "MHX_JIT_WAVES=1", std::string("MHX_JIT_PAIR=") + (smode == 1 ? "1" : "0"),
                              std::string("MHX_JIT_XMEM=") + (smode == 2 ? "1" : "0")}, &m,
                             {"-mllvm", "-pragma-unroll-threshold=4000000"});
            hipFunction_t fimg = nullptr;
            // the same geometry, the LDS is the ring; the kernel takes the two images after the usual arguments
            launch_rec k = rec_shape("streamed matrix-core kernel", 64 * MHX_MFMA_WAVES, 16 * MHX_MFMA_WAVES, mfma_ring_bytes(d, smode == 1),
                                     {&r->k_tp, &r->d_pvec, &r->d_mfma_img, &r->d_mfma_img2});
            if (rc == MHX_OK) rc = jit_function(m, "mhx_jit_mfma_image", &fimg);
            if (rc == MHX_OK) rc = rec_bind(&k, m, "mhx_jit_rwmh_mfma_stream");
            if (rc == MHX_OK) {
                const size_t reals = mfma_image_reals(d);
                HIP_TRY(hipMalloc(&r->d_mfma_img, 2 * reals * sizeof(mhx_real)));
                r->d_mfma_img2 = r->d_mfma_img + reals;
                HIP_TRY(hipMemsetAsync(r->d_mfma_img, 0, 2 * reals * sizeof(mhx_real), ctx->stream));
                const mhx_real* srcs[2] = {tk == MHX_TARGET_CORR_GAUSS ? t->dparams : nullptr, pk == MHX_PROP_DENSE ? r->d_pvec : nullptr};
                for (int im = 0; im < 2 && rc == MHX_OK; ++im) {
                    if (!srcs[im]) continue;
                    mhx_real* dst = r->d_mfma_img + im * reals;
                    rc = launch_module(fimg, 1, 256, ctx->stream, srcs[im], dst);
                }
                if (rc == MHX_OK) HIP_TRY(hipStreamSynchronize(ctx->stream));
            }
            if (rc == MHX_OK) { r->step = k; r->variant = KF_MFMA; r->coop_L = 4; }
        }
        // reduce_lanes = 4 asked for explicitly and a matrix-core kernel was tried but did not come up: the error is the
        // caller's, like every other explicit reduce_lanes (no silent change of the summation shape)
        if (r->variant == KF_GENERIC && rc != MHX_OK && cfg->reduce_lanes == 4) return rc;
        L = cfg->reduce_lanes > 1 ? cfg->reduce_lanes : dense_coop_lanes(d);
        if (r->variant == KF_MFMA || !dense_coop_fits(d, L, nimg)) {
            L = 1;
        } else {
        if (L > 64 || (L & (L - 1)) || L > d) return mhx_fail(MHX_EINVAL, "reduce_lanes must be a power of two <= min(64, dim), got %d", L);
        jit_module* m = nullptr;
        rc = jit_compile(ctx, jit_source(t, "mhx_rwmh_dense_kernels.h"),
                         {"MHX_JIT_RWMH_DENSE=1", "MHX_JIT_DIM=" + std::to_string(d), "MHX_JIT_L=" + std::to_string(L),
                          "MHX_JIT_PK=" + std::to_string(pk), "MHX_JIT_TK=" + std::to_string(tk)}, &m);
        launch_rec k = rec("dense cooperative kernel", 64 * MHX_EMCEE_COOP_WAVES, (64 / L) * MHX_EMCEE_COOP_WAVES, dense_coop_lds_bytes(d, L, nimg));
        if (rc == MHX_OK) rc = rec_bind(&k, m, "mhx_jit_rwmh_dense");
        if (rc == MHX_OK) { r->step = k; r->variant = KF_DENSE_COOP; r->coop_L = L; }
        else if (cfg->reduce_lanes > 1) return rc;
        L = 1;                                                        // not the separable cooperative path below
        }
    } else if (cfg->reduce_lanes > 1 && r->variant != KF_WAVE) {
        return mhx_fail(MHX_EINVAL, "reduce_lanes > 1 needs a separable catalogue target or the dense Gaussian target "
                                "(dim <= 128, JIT), and an ISO/DIAG proposal");
    }
    if (L > 1 || coop_one_lane) {
        const int NBL = (nblk + L - 1) / L;
        if (NBL > MHX_COOP_NBL_MAX) return mhx_fail(MHX_EINVAL, "reduce_lanes=%d leaves %d blocks per lane (max %d)", L, NBL, MHX_COOP_NBL_MAX);
        // tuning knobs: MHX_NO_PREBUILT=1 specialises with hiprtc even where a pre-built kernel exists; MHX_COOP_WAVES=w
        // overrides the waves-per-SIMD launch bound of the hiprtc kernel (register budget 512 / w)
        const int waves_override = opt_int(ctx, "COOP_WAVES", 0);
        const bool zig = (cfg->flags & MHX_FLAG_ZIGGURAT) != 0;
        if (zig && MHX_ZIG_LDS_BYTES(NBL) > MHX_LDS_PER_BLOCK)
            return mhx_fail(MHX_EINVAL, "MHX_FLAG_ZIGGURAT: %d blocks per lane need %d bytes of LDS per block (limit %d); use more lanes per chain",
                            NBL, (int)MHX_ZIG_LDS_BYTES(NBL), (int)MHX_LDS_PER_BLOCK);
        // The kernel's LDS: the ziggurat's slab (layer table + the step's normals).  One or two chains per wave: rows of the
        // [dim][chains] arrays move through LDS, CB = 4 * (64 / L) chains at a time (mhx_rwmh_coop_body); the ziggurat's slab holds that
        // buffer, the Box-Muller kernels get one of their own
        size_t coop_lds = zig ? MHX_ZIG_LDS_BYTES(NBL) : 0;
        int coop_tr = 0;
        if (L >= 32) {
            const size_t need = (size_t)d * (size_t)(4 * (64 / L)) * sizeof(mhx_real);
            if (zig) coop_tr = 1;
            else if (need <= 65536) { coop_lds = (need + 15) & ~(size_t)15; coop_tr = 1; }
        }
        // 256-thread blocks of whole waves of 64 / L chains; L >= 32: the kernel's XCD-aware block -> chain map wants whole rounds of 8.
        // The moments twin has this shape too; wave pairs the same grid (a block's 4 pairs serve the chains of the one-wave body's 4
        // waves) in 512-thread blocks
        const launch_rec coop = rec("cooperative kernel", 256, 4 * (64 / L), coop_lds, L >= 32 ? 8 : 1);
        // Generator / consumer wave pairs (mhx_rwmh_coop_pairs_body): where the fp64 ziggurat form runs ONE wave per SIMD, a plain walk
        // with one scale, one step per fix-up group (10 to 13 blocks per lane).  Option COOP_PAIRS: 0 = the one-wave body, 1 = pairs,
        // unset = the library's choice (MHX_COOP_PAIRS_DEFAULT); a shape outside the rule keeps the one-wave body whatever the option
        // says.  Same chains bit for bit either way.
        const bool pairs_fit = MHX_REAL64 && zig && !walk && pk == MHX_PROP_ISO && MHX_COOP_WAVES(NBL) == 1 && MHX_ZIG_KS(NBL) == 1 && L < 32 &&
                               !waves_override;      // (8 or 9 blocks per lane: two steps per fix-up group, the one-wave body's own gain)
        const bool pairs = pairs_fit && opt_int(ctx, "COOP_PAIRS", MHX_COOP_PAIRS_DEFAULT) != 0;
        if (!opt_on(ctx, "NO_PREBUILT") && !waves_override && !walk)
            for (const auto& pb : k_prebuilt_coop)
                if (pb.L == L && pb.NBL == NBL && pb.TK == tk && pb.PK == pk && pb.gen == (zig ? MHX_GEN_ZIGGURAT : MHX_GEN_BOX_MULLER)) {
                    r->variant = KF_COOP; r->normal_gen = pb.gen;
                    r->coop_pairs = pairs && pb.fn_pairs;
                    r->step = coop;
                    if (r->coop_pairs) r->step.block = 512;
                    if ((rc = rec_bind(&r->step, (const void*)(r->coop_pairs ? pb.fn_pairs : pb.fn)))) return rc;
                    if (pb.fn_mom) {
                        r->step_mom = coop;
                        if ((rc = rec_bind(&r->step_mom, (const void*)pb.fn_mom))) return rc;
                    }
                }
        // the kernel's defines; its running-moments twin (mhx_run_sample, MHX_SAVE_MOMENTS) is built from this list with MHX_JIT_MOM=1
        r->coop_defs = {"MHX_JIT_RWMH_COOP=1", "MHX_JIT_L=" + std::to_string(L), "MHX_JIT_NBL=" + std::to_string(NBL),
                        "MHX_JIT_TK=" + std::to_string(tk), "MHX_JIT_PK=" + std::to_string(pk), "MHX_JIT_MOM=0",
                        "MHX_JIT_WALK=" + std::to_string(walk), std::string("MHX_JIT_GEN=") + (zig ? "1" : "0")};
        if (r->variant == KF_GENERIC && !(r->flags & MHX_FLAG_NO_JIT)) {
            jit_module* m = nullptr;
            std::vector<std::string> defs = r->coop_defs;
            if (waves_override > 0) defs.push_back("MHX_JIT_WAVES=" + std::to_string(waves_override));
            if (pairs) defs.push_back("MHX_JIT_PAIRS=1");
#ifdef MHX_TOOLS_BUILD
            if (const int zf = opt_int(ctx, "ZIG_FORCE_FAIL", 0); zf > 0)          // test hook: see mhx_rwmh_kernels.h (the chains stay valid)
                defs.push_back("MHX_ZIG_FORCE_FAIL=" + std::to_string(zf));
            if (const char* zp = opt(ctx, "ZIG_PROBE")) {                          // timing probe: the chains of such a run are NOT valid
                defs.push_back(std::string("MHX_ZIG_PROBE=") + zp);
                fprintf(stderr, "mhx (tools build): ZIG_PROBE=%s -- timing probe, this run's chains are NOT valid (stats.tainted = 1)\n", zp);
            }
#endif
            rc = jit_compile(ctx, jit_source(t, "mhx_rwmh_kernels.h"), defs, &m);
            launch_rec k = coop;
            if (pairs) k.block = 512;
            if (rc == MHX_OK) rc = rec_bind(&k, m, pairs ? "mhx_jit_rwmh_coop_pairs" : "mhx_jit_rwmh_coop");
            if (rc == MHX_OK) {
                r->step = k; r->coop_pairs = pairs;
                r->variant = KF_COOP_JIT; r->normal_gen = zig ? MHX_GEN_ZIGGURAT : MHX_GEN_BOX_MULLER;
            }
            else if (cfg->reduce_lanes > 1 || zig) return rc;      // the caller asked for this shape explicitly
        }
        if (r->variant != KF_GENERIC) {
            r->coop_L = L;
            r->coop_tr = coop_tr;
        } else if (cfg->reduce_lanes > 1) {
            return mhx_fail(MHX_EINVAL, "reduce_lanes=%d: no pre-built kernel and JIT disabled", L);
        }
    }
    if (r->variant == KF_GENERIC && walk) {
        // no cooperative kernel for this target / proposal family: the state-in-HBM kernel evaluates the ratio
        if (cfg->reduce_lanes > 1) return mhx_fail(MHX_EINVAL, "reduce_lanes > 1 with a drifting / static proposal needs a separable catalogue target and an ISO / DIAG proposal");
        r->flags |= MHX_FLAG_GENERIC;
    }
    if (r->variant == KF_GENERIC && !(r->flags & MHX_FLAG_GENERIC)) {
        if (tk != MHX_TARGET_USER && !(cfg->flags & MHX_FLAG_ZIGGURAT))
            for (const auto& pb : k_prebuilt_reg)
                if (pb.D == d && pb.TK == tk && pb.PK == pk) {          // a lane per chain, one wave per block
                    r->step = rec("register kernel", 64, 64, 0);
                    if ((rc = rec_bind(&r->step, (const void*)pb.fn))) return rc;
                    r->variant = KF_REG;
                }
        // The candidate must be whole in a lane's registers (an arbitrary log-density reads all of it); the state need not be: above
        // MHX_REG_XR_ALL dimensions only its first MHX_REG_XR_CAP coordinates stay in registers, the tail lives in LDS
        // (mhx_rwmh_reg_body<..., XR>).  That carries the kernel to twice its old dimension limit -- an fp64 user log-density at
        // d = 100 ran the state-in-HBM kernel at 4.9e8 steps/s, now 2.4e9 -- and is faster below it too (fp64 d = 80: 2.8 -> 3.3e9,
        // fp32 d = 160: 1.6 -> 2.8e9): tools/reg_xr_sweep.sh, profiles/r04v_reg_xr_sweep.log.  ISO / DIAG proposals.
        // -amdgpu-unroll-threshold-private: hipcc unrolls a loop over a private array only up to a cost of 2 700; a user's
        // `for (k < d)` loop above that (d = 100 with one division per term) stays a loop, its array lands in scratch memory and
        // the kernel runs 3 x slower (the cliff between d = 96 and d = 100 of the first measurement).
        const bool split = d > MHX_REG_XR_ALL && d <= 2 * MHX_REG_MAX_DIM && pk != MHX_PROP_DENSE;
        if (!opt(ctx, "REG_MAX_DIM") && split) regmax = 2 * MHX_REG_MAX_DIM;
        if (r->variant == KF_GENERIC && !(r->flags & MHX_FLAG_NO_JIT) && d <= regmax &&
            !(tk == MHX_TARGET_CORR_GAUSS && d > (MHX_REAL64 ? 32 : 64)) && !(tk == MHX_TARGET_IID_NORMAL && t->nparams > 4096)) {
            jit_module* m = nullptr;
            int xr = split ? MHX_REG_XR_CAP : d;
            if (const char* xe = opt(ctx, "REG_XR")) xr = std::max(0, std::min(d, atoi(xe)));      // tuning knobs
            const char* ut = opt(ctx, "REG_UNROLL");
            std::vector<std::string> xo;
            if (!ut || atoi(ut) > 0) xo = {"-mllvm", std::string("-amdgpu-unroll-threshold-private=") + (ut ? ut : "100000")};
            // MHX_FLAG_ZIGGURAT (ISO / DIAG proposal; both widths since round 6): the register kernel's ziggurat form (mhx_rwmh_reg_zig_body) -- any target,
            // a user's HIP source included
            const bool zig_reg = (cfg->flags & MHX_FLAG_ZIGGURAT) && pk != MHX_PROP_DENSE;
            // waves per SIMD the kernel's register budget is cut for (REG_WAVES; measured on the fp32 ziggurat form: no gain from 2)
            int rwaves = 1;
            if (const char* we = opt(ctx, "REG_WAVES")) rwaves = std::max(1, std::min(4, atoi(we)));
            // fp32: the step's normals through an LDS slab instead of the hand-back walk, where four one-wave blocks of it fit a CU
            // (option REG_ZSLAB = 0 / 1 overrides)
            bool zslab = !MHX_REAL64 && zig_reg && 4 * (MHX_REG_ZIG_LDS_BYTES(d, xr) + MHX_REG_ZIG_SLAB_BYTES(d)) <= 163840;
            if (const char* ze = opt(ctx, "REG_ZSLAB")) zslab = !MHX_REAL64 && zig_reg && atoi(ze) != 0;
            std::vector<std::string> rdefs = {"MHX_JIT_RWMH_REG=1", "MHX_JIT_DIM=" + std::to_string(d),
                                              "MHX_JIT_TK=" + std::to_string(tk), "MHX_JIT_PK=" + std::to_string(pk), "MHX_JIT_XR=" + std::to_string(xr)};
            if (zig_reg) rdefs.push_back("MHX_JIT_GEN=1");
            if (zslab) rdefs.push_back("MHX_JIT_ZSLAB=1");
            if (rwaves > 1) rdefs.push_back("MHX_JIT_REG_WAVES=" + std::to_string(rwaves));
            rc = jit_compile(ctx, jit_source(t, "mhx_rwmh_kernels.h"), rdefs, &m, xo);
            // its LDS: the tail of a state that does not fit beside the candidate, or the ziggurat's table (and slab)
            launch_rec k = rec("register kernel", 64, 64, zig_reg ? MHX_REG_ZIG_LDS_BYTES(d, xr) + (zslab ? MHX_REG_ZIG_SLAB_BYTES(d) : 0)
                                                                  : (size_t)(d - xr) * 64 * sizeof(mhx_real));
            if (rc == MHX_OK) rc = rec_bind(&k, m, "mhx_jit_rwmh_reg");
            if (rc == MHX_OK) { r->step = k; r->variant = KF_REG_JIT; if (zig_reg) r->normal_gen = MHX_GEN_ZIGGURAT; }
            else if (tk == MHX_TARGET_USER) return rc;      // no pre-built kernel can run a user source
            // built-in target: the generic kernel below computes the same chain; keep the message
        }
    }
    jit_module* umod = nullptr;
    if (tk == MHX_TARGET_USER) {
        jit_module* m = nullptr;
        if ((rc = jit_generic_rwmh(t, &m))) return rc;
        if ((rc = jit_function(m, "mhx_jit_rwmh_init", &r->jit_init))) return rc;
        umod = m;
    }
    if (r->variant == KF_GENERIC) {      // the state-in-HBM kernel: pre-built, or of the user target's module
        r->step = rec("state-in-HBM kernel", 256, 256, 0);
        if ((rc = umod ? rec_bind(&r->step, umod, "mhx_jit_rwmh_generic") : rec_bind(&r->step, (const void*)k_rwmh_generic))) return rc;
    }
    if ((cfg->flags & MHX_FLAG_ZIGGURAT) && r->normal_gen != MHX_GEN_ZIGGURAT)
        return mhx_fail(MHX_EINVAL, "MHX_FLAG_ZIGGURAT: this run's kernel (variant %d) has no ziggurat form -- it exists on the cooperative "
                                    "kernel (separable catalogue target) and on the register kernel (any target within its "
                                    "dimension limit), ISO / DIAG proposal, JIT allowed", r->variant);
    // candidate scratch of the state-in-HBM kernel; a static proposal whitens the state into it whatever kernel steps the chain
    if (r->variant == KF_GENERIC || r->d_qx) HIP_TRY(hipMalloc(&r->d_ybuf, (size_t)d * (size_t)r->n * sizeof(mhx_real)));
    *out = r.release();
    return MHX_OK;
}

// the component table of a family proposal: parameters and what the kernels derive from them once, in double, each rounded once
// to the engine's width; `pattern` is the comma-separated list of families (MHX_JIT_FAM_LIST)
static int fam_build_table(const char* me, const mhx_proposal_component* comps, const int d, std::vector<mhx_fam_comp>& tab, std::string& pattern)
{
    tab.assign((size_t)d, mhx_fam_comp{});
    pattern.clear();
    for (int k = 0; k < d; ++k) {
        const mhx_proposal_component& c = comps[k];
        const double p0 = c.p0, p1 = c.p1;
        mhx_fam_comp& o = tab[(size_t)k];
        memset(&o, 0, sizeof o);
        o.family = c.family;
        const bool fin0 = std::isfinite(p0), fin1 = std::isfinite(p1);
        const char* bad = nullptr;
        switch (c.family) {
        case MHX_FAMILY_NORMAL: if (!fin0 || !fin1 || !(p1 > 0.0)) bad = "Normal(mu, sigma) needs finite mu and sigma > 0"; break;
        case MHX_FAMILY_UNIFORM: if (!fin0 || !fin1 || !(p0 < p1)) bad = "Uniform(a, b) needs finite a < b"; break;
        case MHX_FAMILY_LAPLACE: if (!fin0 || !fin1 || !(p1 > 0.0)) bad = "Laplace(mu, theta) needs finite mu and theta > 0"; break;
        case MHX_FAMILY_CAUCHY: if (!fin0 || !fin1 || !(p1 > 0.0)) bad = "Cauchy(mu, sigma) needs finite mu and sigma > 0"; break;
        case MHX_FAMILY_EXPONENTIAL: if (!fin0 || !(p0 > 0.0)) bad = "Exponential(theta) needs finite theta > 0"; break;
        case MHX_FAMILY_GAMMA: if (!fin0 || !fin1 || !(p0 > 0.0) || !(p1 > 0.0)) bad = "Gamma(alpha, theta) needs finite alpha > 0 and theta > 0"; break;
        case MHX_FAMILY_INVERSE_GAMMA: if (!fin0 || !fin1 || !(p0 > 0.0) || !(p1 > 0.0)) bad = "InverseGamma(alpha, theta) needs finite alpha > 0 and theta > 0"; break;
        default: return mhx_fail(MHX_EINVAL, "%s: component %d has unknown family %d", me, k, c.family);
        }
        if (bad) return mhx_fail(MHX_EINVAL, "%s: component %d: %s, got (%g, %g)", me, k, bad, p0, p1);
        o.p[0] = (mhx_real)p0;
        o.p[1] = (mhx_real)p1;
        if (c.family == MHX_FAMILY_UNIFORM) {
            o.p[2] = o.p[1] - o.p[0];                       // the rounded bounds' difference, in the engine's width
            if (!(o.p[0] < o.p[1])) bad = "Uniform(a, b): a and b round to the same number in this width";
        } else if (c.family == MHX_FAMILY_GAMMA || c.family == MHX_FAMILY_INVERSE_GAMMA) {
            // everything from alpha AS ROUNDED to the run's width -- the number the kernel compares with 1 to apply the boost
            const double al = (double)o.p[0];
            const double ae = al < 1.0 ? al + 1.0 : al, dd = ae - 1.0 / 3.0;
            o.p[2] = (mhx_real)dd;
            o.p[3] = (mhx_real)(1.0 / std::sqrt(9.0 * dd));
            o.p[4] = (mhx_real)(1.0 / al);
            o.p[5] = (mhx_real)(c.family == MHX_FAMILY_GAMMA ? al - 1.0 : -(al + 1.0));
            if (!(o.p[0] > MHX_R(0.0)) || !(o.p[1] > MHX_R(0.0)) || !std::isfinite((double)o.p[4])) bad = "the parameters leave this width's range";
        } else if (c.family != MHX_FAMILY_UNIFORM && c.family != MHX_FAMILY_EXPONENTIAL && !(o.p[1] > MHX_R(0.0))) {
            bad = "the scale rounds to zero in this width";
        }
        if (c.family == MHX_FAMILY_EXPONENTIAL && !(o.p[0] > MHX_R(0.0))) bad = "the scale rounds to zero in this width";
        if (bad) return mhx_fail(MHX_EINVAL, "%s: component %d: %s, got (%g, %g)", me, k, bad, p0, p1);
        if (k) pattern += ',';
        pattern += std::to_string(c.family);
    }
    return MHX_OK;
}

// ---------------------------------------------------------------------------------------------
// A proposal of independent univariate components (include/mhx.h: mhx_rwmh_create_components)
int api_rwmh_create_components(mhx_ctx* ctx, const mhx_target* t, const mhx_rwmh_cfg* cfg, const mhx_proposal_component* comps,
                               int32_t ncomps, mhx_run** out)
{
    const char* me = "mhx_rwmh_create_components";
    if (!ctx || !t || !cfg || !comps || !out) return mhx_fail(MHX_EINVAL, "%s: NULL argument", me);
    if (cfg->dim != t->dim) return mhx_fail(MHX_EINVAL, "%s: proposal dim %d != model dim %d", me, cfg->dim, t->dim);
    if (ncomps != cfg->dim) return mhx_fail(MHX_EINVAL, "%s: %d components for dim %d (one component per parameter)", me, ncomps, cfg->dim);
    if (cfg->nchains <= 0) return mhx_fail(MHX_EINVAL, "%s: nchains must be positive", me);
    if (cfg->flags & MHX_FLAG_ZIGGURAT)
        return mhx_fail(MHX_EINVAL, "%s: MHX_FLAG_ZIGGURAT -- a family run draws its Normal components by Box-Muller only", me);
    if (cfg->reduce_lanes > 1)
        return mhx_fail(MHX_EINVAL, "%s: reduce_lanes = %d -- a family run is one lane per chain (reduce_lanes 0 or 1)", me, cfg->reduce_lanes);
    const int d = cfg->dim;
    if (d >= (1 << 20)) return mhx_fail(MHX_EINVAL, "%s: dim must be below 2^20 (the Gamma blocks are numbered component << 8 | attempt)", me);
    const bool stat = (cfg->flags & MHX_FLAG_STATIC_PROPOSAL) != 0;
    std::vector<mhx_fam_comp> tab;
    std::string pattern;
    { const int rct = fam_build_table(me, comps, d, tab, pattern); if (rct) return rct; }
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<mhx_run> r(new mhx_run);
    r->dtype = ctx->dtype;
    r->ctx = ctx; r->target = t; r->kind = RUN_RWMH;
    r->dim = d; r->n = cfg->nchains; r->seed = cfg->seed; r->first_id = cfg->first_chain;
    r->flags = cfg->flags;
    r->prop_kind = 3;                                        // none of mhx_proposal_kind: a checkpoint of an (Mv)Normal run does not load here
    r->variant = KF_FAMILY;
    r->fam_symmetric = (!stat && (cfg->flags & MHX_FLAG_SYMMETRIC_PROPOSAL)) ? 1 : 0;
    HIP_TRY(hipMalloc(&r->d_fam, tab.size() * sizeof(mhx_fam_comp)));
    COPY_SYNC(ctx->stream, r->d_fam, tab.data(), tab.size() * sizeof(mhx_fam_comp), hipMemcpyHostToDevice);
    int rc = run_alloc_state(r.get());
    if (rc) return rc;
    if (stat) HIP_TRY(hipMalloc(&r->d_qx, (size_t)r->n * sizeof(mhx_real)));
    const int tk = t->kind;
    // the register form addresses a [dim+1][nchains] slab with 32-bit byte offsets and holds x and y in VGPRs
    const bool small = ((uint64_t)d + 1) * (uint64_t)r->n * (uint64_t)sizeof(mhx_real) < (1ull << 32);
    if (!(r->flags & (MHX_FLAG_GENERIC | MHX_FLAG_NO_JIT)) && small && d <= MHX_FAM_REG_MAX_DIM &&
        !(tk == MHX_TARGET_CORR_GAUSS && d > (MHX_REAL64 ? 32 : 64)) && !(tk == MHX_TARGET_IID_NORMAL && t->nparams > 4096)) {
        jit_module* m = nullptr;
        // the component loop must unroll whole (y[k] indexed by a constant): its body -- Philox, a draw, two log-kernels -- passes
        // hipcc's size limit for `#pragma unroll` from about 48 components on, and y would then live in scratch
        const char* ut = opt(ctx, "REG_UNROLL");
        std::vector<std::string> xo = {"-mllvm", "-pragma-unroll-threshold=4000000"};
        if (!ut || atoi(ut) > 0) { xo.push_back("-mllvm"); xo.push_back(std::string("-amdgpu-unroll-threshold-private=") + (ut ? ut : "100000")); }
        rc = jit_compile(ctx, jit_source(t, "mhx_rwmh_family_kernels.h"),
                         {"MHX_JIT_FAM_REG=1", "MHX_JIT_DIM=" + std::to_string(d), "MHX_JIT_TK=" + std::to_string(tk),
                          "MHX_JIT_FAM_LIST=" + pattern, std::string("MHX_JIT_FAM_STATIC=") + (stat ? "1" : "0"),
                          std::string("MHX_JIT_FAM_SYM=") + (r->fam_symmetric ? "1" : "0")}, &m, xo);
        // kernel(args, tparams, fam): a lane per chain, one wave per block
        r->step = rec_shape("family register kernel", 64, 64, 0, {&r->k_tp, &r->d_fam});
        if (rc == MHX_OK) rc = rec_bind(&r->step, m, "mhx_jit_fam_reg");
        if (rc) return rc;
        r->fam_reg = true;
    }
    // ... else kernel(args, tparams, fam, symmetric): the state in HBM
    if (!r->fam_reg) r->step = rec_shape("family state-in-HBM kernel", 256, 256, 0, {&r->k_tp, &r->d_fam, &r->fam_symmetric});
    if (tk == MHX_TARGET_USER) {
        jit_module* m = nullptr;
        if ((rc = jit_generic_rwmh(t, &m))) return rc;
        if ((rc = jit_function(m, "mhx_jit_rwmh_init", &r->jit_init))) return rc;
        if (!r->fam_reg) {
            if ((rc = jit_compile(ctx, jit_source(t, "mhx_rwmh_family_kernels.h"), {"MHX_JIT_FAM_GENERIC=1", "MHX_JIT_TK=" + std::to_string(tk)}, &m))) return rc;
            if ((rc = rec_bind(&r->step, m, "mhx_jit_fam_generic"))) return rc;
        }
    } else if (!r->fam_reg && (rc = rec_bind(&r->step, (const void*)k_fam_generic))) return rc;
    if (!r->fam_reg) HIP_TRY(hipMalloc(&r->d_ybuf, (size_t)d * (size_t)r->n * sizeof(mhx_real)));
    *out = r.release();
    return MHX_OK;
}

#include "mhx_api_cond.inc"
#include "mhx_api_composite.inc"

// ---- emcee / ram creation, init and stepping live in their own sections below
static int emcee_init(mhx_run* r, const mhx_real* init);
static int emcee_sync_state(mhx_run* r, int to_abi);
static int emcee_advance(mhx_run* r, uint64_t nsteps, uint32_t save_next, int save_slot, int thinning);
static int ram_init(mhx_run* r, const mhx_real* init);
static int ram_advance(mhx_run* r, uint64_t nsteps, uint64_t n_adapt, uint32_t save_next, int save_slot, int thinning);
static int ram_prepare_step_stats(mhx_run* r, const mhx_schedule* s, uint64_t n_adapt);
static int mala_init(mhx_run* r, const mhx_real* init);
static int mala_eval_state(mhx_run* r, int reset_counts);
static int mala_advance(mhx_run* r, uint64_t nsteps, uint32_t save_next, int save_slot, int thinning);

// A caller-supplied state enters an RWMH chain with -0.0 coordinates as +0.0 (x + 0.0: every other value, NaN and the
// infinities included, is unchanged; -0.0 == +0.0, so `chain[1].params == initial_params` of test/runtests.jl:203-213 holds).
// The chain itself never produces a -0.0 (a rounded sum is -0 only if both terms are), and the fp64 plain-walk kernel relies on
// that: it re-forms a REJECTED state as fma(0, n, x), which is x exactly for every x but -0.0.  The oracle does the same
// (orc_rwmh, `init`).
__global__ void k_plus_zero(mhx_real* x, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = x[i] + MHX_R(0.0);
}

static int rwmh_canonical_zero(mhx_run* r)
{
    const size_t nx = (size_t)r->dim * (size_t)r->n;
    hipLaunchKernelGGL(k_plus_zero, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, r->ctx->stream, r->d_x, nx);
    HIP_TRY(hipGetLastError());
    return MHX_OK;
}

static int tempered_reset_ladder(mhx_run* r);                       // (mhx_api_tempered.inc)
static int adaptive_reset(mhx_run* r);                              // (mhx_api_adaptive.inc)
static int adaptive_seam(mhx_run* r);

static int rwmh_init(mhx_run* r, const mhx_real* init)
{
    mhx_ctx* ctx = r->ctx;
    const size_t nx = (size_t)r->dim * (size_t)r->n;
    if ((r->variant == KF_COND || (r->variant == KF_COMPOSITE && r->cmp_mapped)) && !init)
        return mhx_fail(MHX_EINVAL, "mhx_run_init: a conditional proposal has no distribution to draw the first state from -- "
                                "give initial_params (as for MALA)");
    if (init) {
        HIP_TRY(hipMemcpyAsync(r->d_x, init, nx * sizeof(mhx_real), hipMemcpyHostToDevice, ctx->stream));
        int rcz = rwmh_canonical_zero(r);
        if (rcz) return rcz;
    }
    if (r->d_swapc) HIP_TRY(hipMemsetAsync(r->d_swapc, 0, 2 * (size_t)r->n * sizeof(uint32_t), ctx->stream));      // a tempered run: its swap counts begin here
    if (int rct = tempered_reset_ladder(r)) return rct;                                                             // ... and an adaptive ladder at rho0
    mhx_rwmh_args a = rwmh_args(r);
    const mhx_real* tp = r->target->dparams;
    const mhx_real* pv = r->d_pvec;
    int draw = init ? 0 : 1;
    const unsigned grid = (unsigned)((r->n + 255) / 256);
    if ((r->variant == KF_FAMILY || r->variant == KF_COMPOSITE) && draw) {         // the bare draw from the component proposal; the kernel below then evaluates lp
        hipLaunchKernelGGL(k_fam_init_draw, dim3(grid), dim3(256), 0, ctx->stream, a, (const mhx_fam_comp*)r->d_fam);
        HIP_TRY(hipGetLastError());
        draw = 0;
    }
    if (r->target->kind == MHX_TARGET_USER) {
        int rc = launch_module(r->jit_init, grid, 256, ctx->stream, a, tp, pv, draw);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(k_rwmh_init, dim3(grid), dim3(256), 0, ctx->stream, a, tp, pv, draw);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (r->adp) return adaptive_reset(r);                            // an adaptive run: lam = 0, eff = s, m = the first state
    return rwmh_whiten(r);
}

#define MHX_MAX_STEPS_PER_LAUNCH 65536ull

// Move the save cursor past a launch of `chunk` transitions that begins after r->tau: the next transition to record, the slot it
// lands in, and (a running-moments call, RWMH only) the states folded in so far
static void save_cursor_skip(mhx_run* r, uint64_t chunk, int thinning, uint32_t* save_next, int* save_slot)
{
    const uint64_t last = r->tau + chunk;
    if (*save_next == MHX_NO_SAVE || (uint64_t)*save_next > last) return;
    const uint64_t k = (last - *save_next) / (uint64_t)thinning + 1;
    *save_next += (uint32_t)(k * (uint64_t)thinning);
    *save_slot += (int)k;
    if (r->moments_mode) r->mom_n += k;
}

static int rwmh_advance(mhx_run* r, uint64_t nsteps, uint32_t save_next, int save_slot, int thinning)
{
    mhx_ctx* ctx = r->ctx;
    uint64_t done = 0;
    while (done < nsteps) {
        uint64_t chunk = std::min<uint64_t>(nsteps - done, MHX_MAX_STEPS_PER_LAUNCH);
        // an adaptive run: a launch is of one phase, the schedule is split at the seam
        const bool adapting = r->adp && r->tau < r->adp_steps;
        if (adapting) chunk = std::min<uint64_t>(chunk, r->adp_steps - r->tau);
        mhx_rwmh_args a = rwmh_args(r);
        a.step0 = (uint32_t)(r->tau + 1);
        a.nsteps = (int)chunk;
        a.save_next = save_next;
        a.save_slot = save_slot;
        a.thinning = thinning;
        // the record: the running-moments twin, the K = 8 build of the wave-per-chain kernel (candidates per round: by the last call's
        // acceptance, or option WAVE_K), else the run's step kernel
        const launch_rec& k = r->moments_mode && r->step_mom ? r->step_mom
                            : (r->step_k8 && opt_int(ctx, "WAVE_K", r->wave_k) == 8 ? r->step_k8
                            : (r->adp && !adapting ? r->step_frozen : r->step));
        int rc = launch(k, ctx->stream, r->n, 1, &a);
        if (rc) return rc;
        HIP_TRY(hipGetLastError());
        r->stats.launches++;
        save_cursor_skip(r, chunk, thinning, &save_next, &save_slot);
        r->tau += chunk;
        done += chunk;
        if (adapting && r->tau == r->adp_steps && (rc = adaptive_seam(r))) return rc;
    }
    return MHX_OK;
}

int api_run_init(mhx_run* r, const mhx_real* initial_params)
{
    if (!r) return mhx_fail(MHX_EINVAL, "mhx_run_init: run is NULL");
    HIP_TRY(hipSetDevice(r->ctx->device));
    int rc;
    switch (r->kind) {
    case RUN_RWMH: rc = rwmh_init(r, initial_params); break;
    case RUN_EMCEE: rc = emcee_init(r, initial_params); break;
    case RUN_MALA: rc = mala_init(r, initial_params); break;
    default: rc = ram_init(r, initial_params); break;
    }
    if (rc) return rc;
    r->initialised = true;
    r->tau = 0;
    r->acc_total_known = false;
    HIP_TRY(hipMemsetAsync(r->d_acc_total, 0, sizeof(unsigned long long), r->ctx->stream));
    return MHX_OK;
}

// [upstream AbstractMCMC.mcmcsample, restated from memory]: see DESIGN.md section 5
static void schedule_counts(const mhx_schedule* s, uint64_t* n_transitions, uint64_t* n_adapt)
{
    const int64_t N = s->n_samples, di = s->discard_initial, th = s->thinning, nw = s->num_warmup;
    const int64_t dfw = nw < di ? nw : di;
    const int64_t kfw = nw - dfw;
    const int64_t k = kfw < N ? kfw : N;
    *n_transitions = (uint64_t)(di + (N - 1) * th);
    *n_adapt = (uint64_t)(dfw + (k >= 2 ? (k - 1) * th : 0));
}

// a device buffer that only grows: kept (never shrunk) until its owner closes, replaced -- its contents lost -- by a call that needs
// more.  who: the entry point, what: what the bytes are, for the message
static int ensure_buffer(void** p, size_t* cap, size_t need, const char* who, const char* what)
{
    if (*cap >= need && *p) return MHX_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
    hipError_t e = hipMalloc(p, need);
    if (e != hipSuccess) { *p = nullptr; return mhx_fail(MHX_ENOMEM, "%s: %zu bytes of %s: %s", who, need, what, hipGetErrorString(e)); }
    *cap = need;
    return MHX_OK;
}

// accepted proposals of all chains so far
static int run_total_accepts(mhx_run* r, unsigned long long* out)
{
    mhx_ctx* ctx = r->ctx;
    if (r->kind == RUN_EMCEE) {            // per-walker counts summed on demand (no atomics in the half-step kernels)
        HIP_TRY(hipMemsetAsync(r->d_acc_total, 0, sizeof(unsigned long long), ctx->stream));
        hipLaunchKernelGGL(k_sum_u32, dim3(64), dim3(256), 0, ctx->stream, (const unsigned*)r->d_acc, (long)r->n, r->d_acc_total);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    COPY_SYNC(r->ctx->stream, out, r->d_acc_total, sizeof *out, hipMemcpyDeviceToHost);
    return MHX_OK;
}

int api_run_sample(mhx_run* r, const mhx_schedule* s, int save_samples)
{
    if (!r || !s) return mhx_fail(MHX_EINVAL, "mhx_run_sample: NULL argument");
    if (!r->initialised) return mhx_fail(MHX_ESTATE, "mhx_run_sample: call mhx_run_init first");
    if (s->n_samples < 1 || s->thinning < 1 || s->discard_initial < 0 || s->num_warmup < 0)
        return mhx_fail(MHX_EINVAL, "mhx_run_sample: bad schedule (N=%d discard=%d thinning=%d warmup=%d)",
                    s->n_samples, s->discard_initial, s->thinning, s->num_warmup);
    mhx_ctx* ctx = r->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    uint64_t nT = 0, nA = 0;
    schedule_counts(s, &nT, &nA);
    if (r->tau + nT >= 0xffffffffull) return mhx_fail(MHX_EINVAL, "step counter would exceed 2^32-1; start a new seed");
    const auto t0 = std::chrono::steady_clock::now();
    r->stats = mhx_stats{};
    r->stats.kernel_variant = r->variant;
    r->stats.reduce_lanes = r->coop_L;
    r->stats.dtype = r->dtype;
    r->stats.normal_gen = r->normal_gen;
    r->stats.factor_band = r->kind == RUN_EMCEE ? r->emcee_band : -1;
    auto total_accepts = [&](unsigned long long* out) -> int { return run_total_accepts(r, out); };
    // One synchronisation per call: the total before this call is what the previous call read (the counter moves in mhx_run_sample /
    // mhx_run_sample_to_host only, and both leave their reading here); the total after it is copied to a page-locked word on the
    // stream, ahead of the single hipStreamSynchronize.  An ensemble sums its per-walker counts on demand (run_total_accepts).
    const bool one_sync = r->kind != RUN_EMCEE;
    unsigned long long acc_before = r->acc_total_host;
    if (!one_sync || !r->acc_total_known) { int rc0 = total_accepts(&acc_before); if (rc0) return rc0; }
    r->acc_total_known = false;          // (until this call has read the new total: an error return leaves the counter unknown)

    uint32_t save_next = MHX_NO_SAVE;
    int save_slot = 0;
    r->n_saved = 0;
    r->moments_mode = false;
    r->rec_n = 0;
    r->watch_count = 0;              // (with rec_n: a call that keeps nothing must not leave the previous call's watched factors behind)
    r->rec_loga_view = nullptr;
    if (save_samples == MHX_SAVE_MOMENTS) {
        // running moments instead of a sample tensor
        if (r->tmp_R)
            return mhx_fail(MHX_ESTATE, "mhx_run_sample: running moments (MHX_SAVE_MOMENTS) are not kept by a tempered run: record samples");
        if (r->adp)
            return mhx_fail(MHX_ESTATE, "mhx_run_sample: running moments (MHX_SAVE_MOMENTS) are not kept by an adaptive run: record samples");
        if (r->kind == RUN_RWMH && r->variant == KF_COMPOSITE)
            return mhx_fail(MHX_EINVAL, "running moments (MHX_SAVE_MOMENTS) are not kept by a run with a composite proposal "
                                    "(kernel variant 15): record samples");
        if (r->kind == RUN_RWMH && r->variant == KF_COND)
            return mhx_fail(MHX_EINVAL, "running moments (MHX_SAVE_MOMENTS) are not kept by a run with a conditional proposal "
                                    "(kernel variant 14): record samples");
        if (r->kind == RUN_RWMH && r->variant == KF_FAMILY)
            return mhx_fail(MHX_EINVAL, "running moments (MHX_SAVE_MOMENTS) are not kept by a run whose proposal is a vector of family "
                                    "components (kernel variant 13): record samples");
        if (r->kind != RUN_RWMH || (r->variant != KF_GENERIC && r->variant != KF_COOP && r->variant != KF_COOP_JIT))
            return mhx_fail(MHX_EINVAL, "running moments need an RWMH run on the cooperative or the generic kernel "
                                    "(separable target, or MHX_FLAG_GENERIC); this run uses kernel variant %d", r->variant);
        if ((r->variant == KF_COOP || r->variant == KF_COOP_JIT) && !r->step_mom) {
            jit_module* m = nullptr;
            std::vector<std::string> defs = r->coop_defs;
            for (auto& df : defs) if (df == "MHX_JIT_MOM=0") df = "MHX_JIT_MOM=1";
            int rcj = jit_compile(ctx, jit_source(r->target, "mhx_rwmh_kernels.h"), defs, &m);
            launch_rec k = r->step;          // the step kernel's grid and LDS, never as wave pairs: 256-thread blocks
            k.what = "cooperative kernel (moments)"; k.block = 256;
            if (rcj == MHX_OK) rcj = rec_bind(&k, m, "mhx_jit_rwmh_coop");
            if (rcj) return rcj;
            r->step_mom = k;
        }
        const size_t bytes = ((size_t)r->dim + 1) * (size_t)r->n * sizeof(mhx_real);
        int rc = ensure_buffer((void**)&r->d_mom_mean, &r->mom_cap, bytes, "mhx_run_sample", "running-moment buffer");
        if (rc) return rc;
        rc = ensure_buffer((void**)&r->d_mom_m2, &r->mom_cap2, bytes, "mhx_run_sample", "running-moment buffer");
        if (rc) return rc;
        r->moments_mode = true;
        r->mom_n = 0;
        r->n_saved = s->n_samples;
        if (s->discard_initial == 0) {
            const unsigned grid = (unsigned)((r->n + 255) / 256);
            hipLaunchKernelGGL(k_moments_first, dim3(grid), dim3(256), 0, ctx->stream, r->d_x, r->d_lp, r->d_mom_mean,
                               r->d_mom_m2, r->n, (long)r->n, r->dim);
            HIP_TRY(hipGetLastError());
            r->mom_n = 1;
            save_next = s->n_samples > 1 ? (uint32_t)(r->tau + (uint64_t)s->thinning) : MHX_NO_SAVE;
        } else {
            save_next = (uint32_t)(r->tau + (uint64_t)s->discard_initial);
        }
    } else if (save_samples) {
        const size_t N = (size_t)s->n_samples, n = (size_t)r->n, d1 = (size_t)r->dim + 1;
        int rc = ensure_buffer((void**)&r->d_samples, &r->samples_cap, N * d1 * n * sizeof(mhx_real), "mhx_run_sample", "sample buffer");
        if (rc) return rc;
        rc = ensure_buffer((void**)&r->d_accepted, &r->accepted_cap, N * n, "mhx_run_sample", "accept-flag buffer");
        if (rc) return rc;
        r->n_saved = s->n_samples;
        if (r->kind == RUN_RAM) { rc = ram_prepare_step_stats(r, s, nA); if (rc) return rc; }
        if (s->discard_initial == 0) {
            // sample 1 is the current state itself (test/runtests.jl:203-213: chain[1].params == initial_params)
            // an ensemble on the register / cooperative kernels lives in its walker-major copy: bring d_x up to date
            if (r->kind == RUN_EMCEE) { int rcs = emcee_sync_state(r, 1); if (rcs) return rcs; }
            const unsigned grid = (unsigned)((r->n + 255) / 256);
            hipLaunchKernelGGL(k_record_state, dim3(grid), dim3(256), 0, ctx->stream, r->d_x, r->d_lp, r->d_last,
                               r->d_samples, r->d_accepted, r->n, (long)r->n, r->dim, 0L);
            HIP_TRY(hipGetLastError());
            save_slot = 1;
            save_next = s->n_samples > 1 ? (uint32_t)(r->tau + (uint64_t)s->thinning) : MHX_NO_SAVE;
        } else {
            save_slot = 0;
            save_next = (uint32_t)(r->tau + (uint64_t)s->discard_initial);
        }
    }
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    int rc = MHX_OK;
    if (nT) {
        switch (r->kind) {
        case RUN_RWMH: rc = rwmh_advance(r, nT, save_next, save_slot, s->thinning); break;
        case RUN_EMCEE: rc = emcee_advance(r, nT, save_next, save_slot, s->thinning); break;
        case RUN_MALA: rc = mala_advance(r, nT, save_next, save_slot, s->thinning); break;
        default: rc = ram_advance(r, nT, nA, save_next, save_slot, s->thinning); break;
        }
    }
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    if (one_sync) HIP_TRY(hipMemcpyAsync(r->acc_total_pin, r->d_acc_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    unsigned long long acc_after = 0;
    if (one_sync) acc_after = *r->acc_total_pin;
    else { int rc1 = total_accepts(&acc_after); if (rc1) return rc1; }
    r->acc_total_host = acc_after;
    r->acc_total_known = one_sync;
    r->stats.kernel_ms = ms;
    r->stats.transitions = nT * (uint64_t)r->n;
    r->stats.accepted = acc_after - acc_before;
    r->stats.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r->variant == KF_WAVE && r->stats.transitions >= 64)        // (the same chain for either K: only the speed depends on it)
        r->wave_k = 8.0 * (double)r->stats.accepted < (double)r->stats.transitions ? 8 : 4;
    return MHX_OK;
}

int api_run_get_samples(mhx_run* r, mhx_real* samples, uint8_t* accepted)
{
    if (!r) return mhx_fail(MHX_EINVAL, "mhx_run_get_samples: run is NULL");
    if (r->n_saved <= 0 || r->moments_mode)
        return mhx_fail(MHX_ESTATE, "mhx_run_get_samples: the last mhx_run_sample kept no sample tensor");
    if (accepted && !r->d_accepted)
        return mhx_fail(MHX_EINVAL, "mhx_run_get_samples: a derived run holds no accept flags (they are its source's): pass accepted = NULL");
    HIP_TRY(hipSetDevice(r->ctx->device));
    const size_t N = (size_t)r->n_saved, n = (size_t)r->n, d1 = (size_t)r->dim + 1;
    if (samples) COPY_SYNC(r->ctx->stream, samples, r->d_samples, N * d1 * n * sizeof(mhx_real), hipMemcpyDeviceToHost);
    if (accepted) COPY_SYNC(r->ctx->stream, accepted, r->d_accepted, N * n, hipMemcpyDeviceToHost);
    return MHX_OK;
}

#include "mhx_api_host.inc"

int api_run_device_samples(mhx_run* r, void** samples, void** accepted, int64_t* n_samples)
{
    if (!r) return mhx_fail(MHX_EINVAL, "mhx_run_device_samples: run is NULL");
    if (samples) *samples = r->d_samples;
    if (accepted) *accepted = r->d_accepted;
    if (n_samples) *n_samples = r->n_saved;
    return MHX_OK;
}

int api_run_get_state(mhx_run* r, mhx_real* x, mhx_real* lp, uint32_t* accept_counts)
{
    if (!r) return mhx_fail(MHX_EINVAL, "mhx_run_get_state: run is NULL");
    if (!r->initialised) return mhx_fail(MHX_ESTATE, "mhx_run_get_state: run is not initialised");
    HIP_TRY(hipSetDevice(r->ctx->device));
    const size_t n = (size_t)r->n, d = (size_t)r->dim;
    if (x && r->kind == RUN_EMCEE) { int rc = emcee_sync_state(r, 1); if (rc) return rc; }
    if (x) COPY_SYNC(r->ctx->stream, x, r->d_x, d * n * sizeof(mhx_real), hipMemcpyDeviceToHost);
    if (lp) COPY_SYNC(r->ctx->stream, lp, r->d_lp, n * sizeof(mhx_real), hipMemcpyDeviceToHost);
    if (accept_counts) COPY_SYNC(r->ctx->stream, accept_counts, r->d_acc, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    return MHX_OK;
}

int api_run_set_state(mhx_run* r, const mhx_real* x)
{
    if (!r || !x) return mhx_fail(MHX_EINVAL, "mhx_run_set_state: NULL argument");
    if (!r->initialised) return mhx_fail(MHX_ESTATE, "mhx_run_set_state: run is not initialised");
    mhx_ctx* ctx = r->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n = (size_t)r->n, d = (size_t)r->dim;
    COPY_SYNC(r->ctx->stream, r->d_x, x, d * n * sizeof(mhx_real), hipMemcpyHostToDevice);
    if (r->kind == RUN_RWMH) { int rc = rwmh_canonical_zero(r); if (rc) return rc; }
    if (r->kind == RUN_EMCEE) { int rc = emcee_sync_state(r, 0); if (rc) return rc; }
    if (r->kind == RUN_MALA) return mala_eval_state(r, 0);   // src/MALA.jl:27-35: lp and gradient are recomputed
    // lp is a cache of logdensity(model, x) (src/AdvancedMH.jl:75): recompute it
    const unsigned grid = (unsigned)((r->n + 255) / 256);
    int nn = r->n, dd = r->dim, kind = r->target->kind, np = r->target->nparams, lanes = r->coop_L;
    mhx_real cst = r->target->cst;
    const mhx_real* tp = r->target->dparams;
    const mhx_real* dx = r->d_x;
    mhx_real* dlp = r->d_lp;
    if (kind == MHX_TARGET_USER) {
        jit_module* m = nullptr;
        hipFunction_t fn;
        int rc = jit_generic_rwmh(r->target, &m);
        if (rc) return rc;
        if ((rc = jit_function(m, "mhx_jit_target_eval", &fn))) return rc;
        if ((rc = launch_module(fn, grid, 256, ctx->stream, dx, dlp, nn, dd, kind, tp, np, cst, lanes))) return rc;
    } else {
        hipLaunchKernelGGL(k_target_eval, dim3(grid), dim3(256), 0, ctx->stream, dx, dlp, nn, dd, kind, tp, np, cst, lanes);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return r->kind == RUN_RWMH ? rwmh_whiten(r) : MHX_OK;
}

// ---- checkpoint / resume: the complete state of a run as one host blob ------------------------------------------
struct ckpt_header {
    uint32_t magic, version;
    int32_t kind, dim, n, flags;
    uint64_t tau, seed, first_id;
    // what fixes the arithmetic of the continuation: the log-density, the proposal family, the kernel variant and
    // the lanes per chain (summation order of lp); and the exact payload size
    int32_t target_kind, prop_kind, variant, coop_L;
    uint64_t payload_bytes;
    double last_eta;           // RAM: step size of the latest adapting transition
};
static const uint32_t k_ckpt_magic = 0x5848484du;          // "MHXX"
// the static-proposal bit and, for Ensemble runs, how many ensembles the walkers form (2 x 8 walkers are not 1 x 16)
static int32_t ckpt_flags(const mhx_run* r) { return (r->flags & MHX_FLAG_STATIC_PROPOSAL) | (r->n_ens > 1 ? r->n_ens << 8 : 0); }
struct ckpt_part { void* dev; size_t bytes; };
// the device arrays that make up the state, in blob order
static std::vector<ckpt_part> ckpt_parts(mhx_run* r)
{
    const size_t n = (size_t)r->n, d = (size_t)r->dim;
    std::vector<ckpt_part> p = {{r->d_x, d * n * sizeof(mhx_real)}, {r->d_lp, n * sizeof(mhx_real)},
                                {r->d_acc, n * sizeof(uint32_t)}, {r->d_last, n}};
    if (r->kind == RUN_RAM) {
        const size_t trip = (size_t)mhx_ram_tri_pad(r->dim);
        p.push_back({r->d_S, 2 * trip * n * sizeof(mhx_real)});
        p.push_back({r->d_Ssel, n});
        p.push_back({r->d_status, n});
        p.push_back({r->d_dmin, d * n * sizeof(mhx_real)});
        p.push_back({r->d_dmax, d * n * sizeof(mhx_real)});
        p.push_back({r->d_loga, n * sizeof(mhx_real)});
    }
    if (r->kind == RUN_MALA) p.push_back({r->d_gx, d * n * sizeof(mhx_real)});
    if (r->d_qx) p.push_back({r->d_qx, n * sizeof(mhx_real)});
    return p;
}
int api_run_state_size(mhx_run* r, size_t* bytes)
{
    if (!r || !bytes) return mhx_fail(MHX_EINVAL, "mhx_run_state_size: NULL argument");
    if (r->tmp_R) return mhx_fail(MHX_ESTATE, "mhx_run_state_size: a tempered run has no checkpoint / resume");
    if (r->adp) return mhx_fail(MHX_ESTATE, "mhx_run_state_size: an adaptive run has no checkpoint / resume");
    size_t total = sizeof(ckpt_header);
    for (const auto& p : ckpt_parts(r)) total += p.bytes;
    *bytes = total;
    return MHX_OK;
}
int api_run_save_state(mhx_run* r, void* blob, size_t bytes)
{
    if (!r || !blob) return mhx_fail(MHX_EINVAL, "mhx_run_save_state: NULL argument");
    if (r->tmp_R) return mhx_fail(MHX_ESTATE, "mhx_run_save_state: a tempered run has no checkpoint / resume");
    if (r->adp) return mhx_fail(MHX_ESTATE, "mhx_run_save_state: an adaptive run has no checkpoint / resume");
    if (!r->initialised) return mhx_fail(MHX_ESTATE, "mhx_run_save_state: run is not initialised");
    size_t need = 0;
    api_run_state_size(r, &need);
    if (bytes < need) return mhx_fail(MHX_EINVAL, "mhx_run_save_state: the blob holds %zu bytes, the state needs %zu", bytes, need);
    HIP_TRY(hipSetDevice(r->ctx->device));
    if (r->kind == RUN_EMCEE) { int rc = emcee_sync_state(r, 1); if (rc) return rc; }      // walker-major -> ABI layout
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    ckpt_header h = {k_ckpt_magic, 2u, (int32_t)r->kind, r->dim, r->n, ckpt_flags(r), r->tau, r->seed, r->first_id,
                     r->target->kind, r->prop_kind, r->variant, r->coop_L, (uint64_t)(need - sizeof(ckpt_header)), r->last_eta};
    char* out = (char*)blob;
    memcpy(out, &h, sizeof h);
    out += sizeof h;
    for (const auto& p : ckpt_parts(r)) {
        COPY_SYNC(r->ctx->stream, out, p.dev, p.bytes, hipMemcpyDeviceToHost);
        out += p.bytes;
    }
    return MHX_OK;
}
int api_run_load_state(mhx_run* r, const void* blob, size_t bytes)
{
    if (!r || !blob) return mhx_fail(MHX_EINVAL, "mhx_run_load_state: NULL argument");
    if (r->tmp_R) return mhx_fail(MHX_ESTATE, "mhx_run_load_state: a tempered run has no checkpoint / resume");
    if (r->adp) return mhx_fail(MHX_ESTATE, "mhx_run_load_state: an adaptive run has no checkpoint / resume");
    size_t need = 0;
    api_run_state_size(r, &need);
    ckpt_header h;
    if (bytes < sizeof h) return mhx_fail(MHX_EINVAL, "mhx_run_load_state: the blob is too short");
    memcpy(&h, blob, sizeof h);
    if (h.magic != k_ckpt_magic || h.version != 2u) return mhx_fail(MHX_EINVAL, "mhx_run_load_state: not a state blob of this library version");
    if (h.kind != (int32_t)r->kind || h.dim != r->dim || h.n != r->n || bytes != need || h.payload_bytes != need - sizeof h)
        return mhx_fail(MHX_EINVAL, "mhx_run_load_state: the blob is a state of sampler kind %d, dim %d, %d chains (%zu bytes); "
                                "this run is kind %d, dim %d, %d chains (%zu bytes)", h.kind, h.dim, h.n, bytes, (int)r->kind, r->dim, r->n, need);
    if (h.flags != ckpt_flags(r) || h.target_kind != r->target->kind || h.prop_kind != r->prop_kind ||
        h.variant != r->variant || h.coop_L != r->coop_L)
        return mhx_fail(MHX_EINVAL, "mhx_run_load_state: the blob was saved by a different configuration (target kind %d, proposal kind %d, "
                                "static %d, kernel variant %d, %d lane(s) per chain; this run: %d, %d, %d, %d, %d) -- the continuation "
                                "would not be the saved chain", h.target_kind, h.prop_kind, h.flags, h.variant, h.coop_L,
                    r->target->kind, r->prop_kind, ckpt_flags(r), r->variant, r->coop_L);
    HIP_TRY(hipSetDevice(r->ctx->device));
    const char* in = (const char*)blob + sizeof h;
    for (const auto& p : ckpt_parts(r)) {
        COPY_SYNC(r->ctx->stream, p.dev, in, p.bytes, hipMemcpyHostToDevice);
        in += p.bytes;
    }
    // the counter-based streams continue where the saved run stopped: same seed, same global ids, same step counter
    r->seed = h.seed; r->first_id = h.first_id; r->tau = h.tau; r->last_eta = h.last_eta;
    r->initialised = true;
    r->n_saved = 0;
    r->acc_total_known = false;
    HIP_TRY(hipMemsetAsync(r->d_acc_total, 0, sizeof(unsigned long long), r->ctx->stream));
    if (r->kind == RUN_EMCEE) { int rc = emcee_sync_state(r, 0); if (rc) return rc; }      // ABI layout -> walker-major
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    return MHX_OK;
}

int api_run_stats(mhx_run* r, mhx_stats* out)
{
    if (!r || !out) return mhx_fail(MHX_EINVAL, "mhx_run_stats: NULL argument");
    *out = r->stats;
    out->tainted = r->ctx->tainted ? 1 : 0;
    out->register_form = (r->adp ? (r->tau < r->adp_steps ? r->adp_reg : r->adp_frozen_reg) : r->fam_reg) ? 1 : 0;
    return MHX_OK;
}

// the name of the run's kernel form (enum kernel_form), with the body it was compiled as where a form has two
const char* api_run_form_name(const mhx_run* r)
{
    if (!r) return "";
    if (r->kind == RUN_DERIVED) return "derived";
    switch (r->variant) {
    case KF_GENERIC: return "generic";
    case KF_REG: return "reg";
    case KF_REG_JIT: return "reg_jit";
    case KF_COOP: return r->coop_pairs ? "coop_pairs" : "coop";
    case KF_COOP_JIT: return r->coop_pairs ? "coop_jit_pairs" : "coop_jit";
    case KF_DENSE_COOP: return "dense_coop";
    case KF_EMCEE_PERSIST: return "emcee_persist";
    case KF_EMCEE_SEQ: return "emcee_seq";
    case KF_MFMA: return "mfma";
    case KF_EMCEE_SCAL: return "emcee_scal";
    case KF_EMCEE_MFMA: return "emcee_mfma";
    case KF_WAVE: return "wave";
    case KF_RAM_DEFER: return "ram_defer";
    case KF_TEMPERED: return r->fam_reg ? "tempered_reg" : "tempered_generic";
    case KF_TEMPERED_ADAPT: return r->fam_reg ? "tempered_adapt_reg" : "tempered_adapt_generic";
    case KF_TEMPERED_ANCHOR: return r->fam_reg ? "tempered_anchored_reg" : "tempered_anchored_generic";
    case KF_ADAPTIVE:           // the form of the phase the next transition belongs to
        if (r->tau < r->adp_steps) return r->adp_reg ? "adaptive_reg" : "adaptive_generic";
        return r->adp_frozen_reg ? "adaptive_frozen_reg" : "adaptive_frozen_generic";
    case KF_FAMILY: return "family";
    case KF_COND: return "cond";
    case KF_COMPOSITE: return "composite";
    }
    return "";
}

int api_run_host_stats(mhx_run* r, mhx_host_stats* out)
{
    if (!r || !out) return mhx_fail(MHX_EINVAL, "mhx_run_host_stats: NULL argument");
    *out = r->host_stats;
    return MHX_OK;
}

bool api_run_is_derived(const mhx_run* r) { return r && r->kind == RUN_DERIVED; }

int api_run_shape(const mhx_run* r, int32_t* dim, int32_t* nchains)
{
    if (dim) *dim = r->dim;
    if (nchains) *nchains = r->n;
    return MHX_OK;
}

int api_run_destroy(mhx_run* r)
{
    if (!r) return MHX_OK;
    (void)hipSetDevice(r->ctx->device);
    delete r;
    return MHX_OK;
}

#include "mhx_api_emcee.inc"
#include "mhx_api_ram.inc"
#include "mhx_api_mala.inc"

// ---- what the post-run statistics share (the .inc files below) ----
// The draws a statistic reads: a tensor [N][d1][C] on ctx's device, and the entry point's name for its messages.
struct draws_view {
    mhx_ctx* ctx;
    const mhx_real* tensor;
    long N, C;
    int d1;
    const char* who;
    uint64_t seed, first_id;                        // of the run the draws came from (0 for a caller's tensor): what a derived run inherits
    unsigned long long S() const { return (unsigned long long)N * (unsigned long long)C; }      // draws of a row
};

// ... a caller's tensor (the mhx_ctx_* forms)
static int draws_of_ctx(const char* who, mhx_ctx* ctx, const mhx_real* d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, draws_view* v)
{
    if (!ctx || !d_tensor) return mhx_fail(MHX_EINVAL, "%s: bad argument", who);
    if (n_samples < 1 || dim1 < 1 || nchains < 1) return mhx_fail(MHX_EINVAL, "%s: tensor of %lld x %d x %lld", who, (long long)n_samples, (int)dim1, (long long)nchains);
    *v = draws_view{ctx, d_tensor, (long)n_samples, (long)nchains, dim1, who, 0, 0};
    return MHX_OK;
}

// ... the sample buffer of a run (the mhx_run_* forms)
static int draws_of_run(const char* who, const mhx_run* r, draws_view* v)
{
    if (!r) return mhx_fail(MHX_EINVAL, "%s: run is NULL", who);
    if (r->moments_mode || r->n_saved < 1 || !r->d_samples)
        return mhx_fail(MHX_ESTATE, "%s: the run holds no device sample tensor (moments mode, save_samples = 0 or a host-streamed run)", who);
    *v = draws_view{r->ctx, r->d_samples, (long)r->n_saved, (long)r->n, r->dim + 1, who, r->seed, r->first_id};
    return MHX_OK;
}

// The pieces of a scratch block, listed ONCE by the call that uses it: scratch_carve runs the list twice, first to add up the bytes,
// then -- the block grown to hold them -- to hand out the pointers.  Every piece starts on a 256-byte line.
struct scratch_pieces {
    char* base;                                     // NULL: the sizing run
    size_t bytes = 0;
    template <class T> T* take(size_t count)
    {
        T* p = base ? (T*)(base + bytes) : nullptr;
        bytes += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};
template <class List>
static int scratch_carve(void** block, size_t* cap, const char* who, const char* what, List&& list)
{
    scratch_pieces sizing{nullptr};
    list(sizing);
    int rc = ensure_buffer(block, cap, sizing.bytes, who, what);
    if (rc) return rc;
    scratch_pieces placing{(char*)*block};
    list(placing);
    return MHX_OK;
}

// The grid of a sweep over the S draws of each of `rows` rows (k_select_hist, k_hpd_gather, k_hist1d / 2d): enough blocks for the whole
// chip, chunks of at least one unrolled block sweep and below 2^31 draws
static unsigned long long sweep_blocks(unsigned long long S, int rows, unsigned long long* chunk)
{
    const unsigned long long sweep = (unsigned long long)MHX_SELECT_THREADS * MHX_SELECT_UNROLL;
    unsigned long long nblk = std::min<unsigned long long>((2048 + rows - 1) / rows, (S + sweep - 1) / sweep);
    nblk = std::max<unsigned long long>(std::max<unsigned long long>(nblk, 1), (S + (1ull << 31) - 1) >> 31);
    *chunk = (S + nblk - 1) / nblk;
    return nblk;
}

// device memory of one call, freed however the call returns
template <class T>
struct dev_array {
    T* p = nullptr;
    dev_array() = default;
    dev_array(const dev_array&) = delete;
    dev_array& operator=(const dev_array&) = delete;
    ~dev_array() { if (p) (void)hipFree(p); }
    bool alloc(size_t count) { return hipMalloc(&p, count * sizeof(T)) == hipSuccess; }
};

// ---- what the statistics that compile a caller's text share (derive, predict, pointwise, psis) ----
// One frame header of a user module and the define that switches its kernels on
struct user_frame {
    const char* have;
    const char* header;
};
// The run-time module of a caller's text and its kernels.  The module's source -- with the defines the kernel key (jit_compile) -- is
// the device math, the text under the name `file` (what the compiler's diagnostics call it), then every frame behind its define.  A
// diagnostic on the caller's text makes the source the argument at fault: MHX_EINVAL, "the <noun> does not compile", the compiler's
// log kept in the message.  Any other failure of the compile (no compiler, a module that does not load) stays MHX_EJIT.
static int user_module(const draws_view& v, const char* file, const char* noun, const char* source, std::initializer_list<user_frame> frames,
                       const std::vector<std::string>& defines, std::initializer_list<std::pair<const char*, hipFunction_t*>> kernels)
{
    std::string s = "#include \"mhx_device_math.h\"\n#line 1 \"";
    s += file;
    s += "\"\n";
    s += source;
    s += "\n";
    for (const user_frame& f : frames) {
        s += "#define ";
        s += f.have;
        s += " 1\n#include \"";
        s += f.header;
        s += "\"\n";
    }
    jit_module* m = nullptr;
    int rc = jit_compile(v.ctx, s, defines, &m);
    if (rc == MHX_EJIT) {
        const std::string log = mhx_last_error();
        if (log.find(file) != std::string::npos) return mhx_fail(MHX_EINVAL, "%s: the %s does not compile: %.1900s", v.who, noun, log.c_str());
        return rc;
    }
    for (const auto& k : kernels)
        if (rc == MHX_OK) rc = jit_function(m, k.first, k.second);
    return rc;
}

// the data block of a user function: closed-over constants, at most 2^31 - 1 reals
static int data_block_checked(const char* who, const mhx_real* data, size_t ndata)
{
    if (ndata && !data) return mhx_fail(MHX_EINVAL, "%s: data is NULL", who);
    if (ndata > 0x7fffffffull) return mhx_fail(MHX_EINVAL, "%s: the data block is too large", who);
    return MHX_OK;
}
// ... and the data rows of a pointwise function (`rows` itself is checked with the caller's other pointers), the data block, and the
// tensor's extents, which the sweeps count in 31 bits
static int row_blocks_checked(const draws_view& v, int64_t nrows, int32_t rowlen, const mhx_real* data, size_t ndata)
{
    const char* who = v.who;
    if (nrows < 1 || rowlen < 1)
        return mhx_fail(MHX_EINVAL, "%s: %lld data rows of %d reals: at least one row of at least one real", who, (long long)nrows, (int)rowlen);
    if (nrows > 0x7fffffffll || (unsigned long long)nrows * (unsigned long long)rowlen > 0x7fffffffull)
        return mhx_fail(MHX_EINVAL, "%s: %lld data rows of %d reals: rows are indexed in 31 bits", who, (long long)nrows, (int)rowlen);
    if (int rc = data_block_checked(who, data, ndata)) return rc;
    if (v.C > 0x7fffffffl || v.N > 0x7fffffffl)
        return mhx_fail(MHX_EINVAL, "%s: %ld saved draws of %ld chains: each is counted in 31 bits", who, v.N, v.C);
    return MHX_OK;
}
// The data block on the device: `count` reals of a scratch block or an allocation are `ndata ? ndata : 1` (one dummy element keeps the
// pointer valid), and only a block that has reals is copied
static size_t data_block_reals(size_t ndata) { return ndata ? ndata : 1; }
static int data_block_upload(mhx_ctx* ctx, mhx_real* d_data, const mhx_real* data, size_t ndata)
{
    if (ndata) HIP_TRY(hipMemcpyAsync(d_data, data, ndata * sizeof(mhx_real), hipMemcpyHostToDevice, ctx->stream));
    return MHX_OK;
}

// The grid of a sweep of the pointwise frame (mhx_pointwise_sweep): chain blocks x strip slots x row tiles.  Slots only while the grid
// is small -- MHX_POINTWISE_TARGET_BLOCKS, a few blocks per compute unit, is what it aims at before it stops splitting a chain block's
// draws over strip slots -- and never more than MHX_POINTWISE_MAX_SLOTS: the partials are ncb * slots * nrows * K doubles whatever N
// is.  `ntiles`: the row-tile term.  The pointwise sweep passes its tiles; PSIS passes 1, which makes the slots a function of the
// tensor's shape alone -- not of the rows of a batch or of a tile -- so that the order of the sums over the draws, and with it every
// bit of the result, is the same whatever PSIS_SCRATCH_MB and PSIS_ROWS are.
#define MHX_POINTWISE_TARGET_BLOCKS 2048
struct sweep_plan {
    long ncb, nstrips, slots;
};
static sweep_plan pointwise_sweep_plan(const draws_view& v, long ntiles)
{
    sweep_plan g;
    g.ncb = (v.C + MHX_POINTWISE_THREADS - 1) / MHX_POINTWISE_THREADS;
    g.nstrips = (v.N + MHX_POINTWISE_STRIP - 1) / MHX_POINTWISE_STRIP;
    const long want = (MHX_POINTWISE_TARGET_BLOCKS + g.ncb * ntiles - 1) / (g.ncb * ntiles);
    g.slots = std::max(1l, std::min(std::min(want, g.nstrips), (long)MHX_POINTWISE_MAX_SLOTS));
    return g;
}

#include "mhx_api_diag.inc"
#include "mhx_api_moments.inc"
#include "mhx_api_hpd.inc"
#include "mhx_api_hist.inc"
#include "mhx_api_acf.inc"
#include "mhx_api_derive.inc"
#include "mhx_api_tempered.inc"
#include "mhx_api_adaptive.inc"
#include "mhx_api_evidence.inc"
#include "mhx_api_pointwise.inc"
#include "mhx_api_psis.inc"

}  // namespace MHX_NS
