/*
 * mhx.h -- C ABI of libmhx.so, the MI355X (gfx950) many-chain Metropolis-Hastings engine.
 *
 * The reference (TuringLang/AdvancedMH.jl v0.8.8) is pure Julia and has no FFI today; its operator
 * API for this path is the AbstractMCMC interface.  Each entry point below names the reference
 * interface it replaces (file:line under the reference tree).  A Julia maintainer binds these with
 * `ccall` (advancedmh.jl_amd/julia/AdvancedMHHIP.jl); the executable host mirror in
 * this repo is the Python package advancedmh.jl_amd/mhx (ctypes).
 *
 * Conventions
 *   - every function returns MHX_OK (0) or a negative mhx_status; mhx_last_error() gives the
 *     message for the calling thread.  Nothing throws across the boundary.
 *   - the caller owns every host buffer; the library owns device memory behind opaque handles.
 *   - calls are blocking: the device work they enqueue has completed when they return.
 *   - host tensor layouts are C order with the CHAIN index fastest:
 *       x        [dim][nchains]
 *       samples  [n_samples][dim + 1][nchains]   (row `dim` is lp; cf. ext/AdvancedMHMCMCChainsExt.jl:96-105)
 *       accepted [n_samples][nchains]            (Transition.accepted, src/AdvancedMH.jl:61-65)
 *       S        [nchains][dim*(dim+1)/2]        packed lower triangle, row-major (RAM factor)
 *   - `real` below is the context's arithmetic type: double for MHX_F64 -- what the reference computes in (Distributions'
 *     Float64 rand / logpdf; src/RobustAdaptiveMetropolis.jl:187-196: T = eltype(sampler.gamma) = Float64) -- or float
 *     for MHX_F32 (the same engine at half the bytes and ~3x the rate).  Every `void *` / `const void *` real buffer of
 *     a call is an array of the dtype of the context the handle belongs to; scalar parameters travel as double and are
 *     rounded once to the context's type.
 *   - a handle is not thread-safe; distinct contexts (one per GPU) may be driven concurrently.
 *   - chains carry GLOBAL ids first_chain .. first_chain+nchains-1 in their RNG counters, so a run
 *     sharded over several GPUs/processes is bit-identical to the unsharded run.
 */
#ifndef MHX_H
#define MHX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHX_VERSION 600 /* 0.6.0: the accept-compacted return path (mhx_compact_hdr, mhx_compact_expand, mhx_run_host_stats, options HOST_COMPACT / HOST_THREADS / HOST_CHUNK); 0.5.0: mhx_group_* (many GPUs from one process), mhx_ctx_set_option (explicit engine options: the library no longer reads tuning variables from the environment), mhx_stats.tainted, mhx_comm_init_timed / deadlines on the collectives, mhx_ctx_pci_bus_id, mhx_run_shape; 0.4.0: mhx_ram_get_step_stats takes a capacity, watched factors, host pin accounting, kernel variant 9 (0.3.0: overlapped host return path, page-locked host buffers, persistent JIT cache) */

typedef enum {
    MHX_OK = 0,
    MHX_EINVAL = -1,   /* bad argument: dim mismatch, non-zero-mean RW proposal, missing initial_params ... */
    MHX_ENOMEM = -2,
    MHX_EHIP = -3,     /* HIP runtime error */
    MHX_EJIT = -4,     /* hiprtc failed to compile a user log-density / specialised kernel */
    MHX_ENOTPD = -5,   /* replaces LinearAlgebra.PosDefException of lowrankdowndate (reported, never thrown) */
    MHX_ESTATE = -6    /* call out of order (e.g. sampling before init) */
} mhx_status;

typedef struct mhx_ctx mhx_ctx;       /* one per GPU: device, stream, JIT cache */
typedef struct mhx_target mhx_target; /* a log-density on the device  == DensityModel (src/AdvancedMH.jl:52-54) */
typedef struct mhx_run mhx_run;       /* device-resident chains of one sampler + their sample buffer */

int mhx_version(void);
const char *mhx_last_error(void);

typedef enum { MHX_F32 = 0, MHX_F64 = 1 } mhx_dtype;

int mhx_ctx_create(int device, int dtype /* mhx_dtype */, mhx_ctx **out);
int mhx_ctx_dtype(const mhx_ctx *ctx);
int mhx_ctx_device(const mhx_ctx *ctx, int *device);
int mhx_ctx_destroy(mhx_ctx *ctx);
/* "dddd:bb:dd.f" of the context's device (hipDeviceGetPCIBusId): ordinals depend on HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES, the
 * bus id does not -- N ranks (or the members of a group) run on N GPUs iff their bus ids are distinct.  len >= 16. */
int mhx_ctx_pci_bus_id(const mhx_ctx *ctx, char *buf, size_t len);

/* Engine options: explicit, per context, set BEFORE the runs they steer are created.  The library reads nothing but
 * MHX_CACHE_DIR / MHX_NO_JIT_CACHE / XDG_CACHE_HOME / HOME (where compiled kernels are kept), MHX_JIT_COMPILER / MHX_JIT_CLANG / ROCM_PATH / MHX_JIT_VERBOSE (who compiles them) and MHX_RCCL_LIB from the environment;
 * which kernel form runs is chosen from (dim, chains, dtype) unless an option says otherwise, and mhx_stats reports the form.
 * Every option below yields the SAME chain law and, for a given reduction shape, the same bits (each form is held to the oracle
 * in tests/): they exist so that every form can be reached at every size, and for A/B measurements.
 *   kernel form     NO_PREBUILT NO_MFMA EMCEE_MFMA EMCEE_SCALAR EMCEE_FUSED EMCEE_PERSIST EMCEE_DEFER EMCEE_SWEEP_DEFER
 *                   EMCEE_PRELOAD RAM_G COOP_PAIRS (fp64 ziggurat cooperative kernel at one wave per SIMD: 1 = generator / consumer
 *                   wave pairs, 0 = the one-wave body, unset = the library's choice; mhx_run_form_name tells which)
 *   tuning          COOP_WAVES MFMA_WAVES REG_MAX_DIM REG_XR REG_UNROLL REG_WAVES REG_ZSLAB MALA_XR EMCEE_WAVES EMCEE_MFMA_WAVES
 *                   EMCEE_SCAL_WPB EMCEE_SCAL_MODE EMCEE_SCAL_REC EMCEE_REC_STORE EMCEE_ROW_STORE EMCEE_COOP_REC RAM_LDS_PAD
 *                   WAVE_K (4 | 8 speculative candidates per round of the wave-per-chain kernel; default: by the last call's acceptance)
 *   return path     HOST_COMPACT (1 / 0: the accept-compacted form of mhx_run_sample_to_host on / off; default: on for thinning == 1
 *                   and >= 1024 chains) HOST_THREADS (host threads that expand; default: what the process may use) HOST_CHUNK (chains
 *                   per unit of their work, a multiple of 64; default: so that a unit's state fits a core's L2) HOST_NUMA (0: do not
 *                   place the staging memory and the expanding threads on the GPU's memory node)
 *   run-time kernels JIT_COMPILER ("hiprtc" | "clang" | unset = clang++ of the installation when found, else hiprtc; mhx_ctx_jit_compiler)
 *   sharding        TOTAL_CHAINS (the chains of the WHOLE run this context's runs are shards of: where the engine picks a kernel
 *                   form -- hence a summation order -- from the chain count (reduce_lanes = 0), it picks for that count, so a shard
 *                   runs what the unsharded run runs; mhx_group_shard sets it on the member's context, a process of a
 *                   multi-process run sets it itself)
 *   summary         SELECT_BITS (digit width of a pass of mhx_*_order_statistics, 1..11; default 11; read at every call)
 *                   HPD_SCRATCH_MB (bound, in MiB, on the device scratch of a call of mhx_*_hpd: the rows go in batches that fit;
 *                   default 1024; a positive number, fractions allowed; read at every call)
 *                   ACF_R (8 | 16 | 32 lags per tile of mhx_*_autocovariance; default: the fastest measured per width; read at every call)
 *                   DERIVE_DRAWS (1..16 draws a lane of mhx_*_derive / mhx_*_predict maps together; default 4 / 1; never more than the outputs leave registers for; read at every call)
 *                   POINTWISE_ROWS (2 | 4 | 8 | 16 data rows per tile of mhx_*_pointwise, five fp64 accumulators each in registers; default: the fastest measured per width, 8 in fp64 and 4 in fp32; read at every call)
 *                   PSIS_SCRATCH_MB (as HPD_SCRATCH_MB, for mhx_*_psis; default 1024; read at every call)
 *                   PSIS_ROWS (1 | 2 | 4 | 8 data rows per tile of the sweeps of mhx_*_psis, 2^11 LDS counters each; default 4; read at every call)
 * value == NULL unsets.  An unknown name is MHX_EINVAL.  The tools build (libmhx_tools.so, `make tools`) additionally knows
 * timing probes and fault injection (ZIG_PROBE, EMCEE_PROBE, EMCEE_STAMPS, ZIG_FORCE_FAIL, FAULT_SLAB, JIT_DEFS, JIT_FLAGS, RAM_PROF, HPD_STOP_AFTER, PSIS_STOP_AFTER): setting one
 * marks the context TAINTED -- mhx_stats.tainted = 1 for every run of it, and the host mirrors refuse to build a Chains from
 * such a run.  In libmhx.so those names do not exist. */
int mhx_ctx_set_option(mhx_ctx *ctx, const char *name, const char *value);
/* the value in effect ("" when unset) copied to buf; MHX_EINVAL for an unknown name */
int mhx_ctx_get_option(const mhx_ctx *ctx, const char *name, char *buf, size_t len);
/* run-time specialisations of this context so far: compiled / loaded from the on-disk code-object cache
 * ($MHX_CACHE_DIR, default ~/.cache/mhx; key = hash(source, device headers, options, compiler + runtime version);
 * MHX_CACHE_DIR="" or MHX_NO_JIT_CACHE=1 switches the cache off).  Either pointer may be NULL. */
int mhx_ctx_jit_counts(const mhx_ctx *ctx, int64_t *compiles, int64_t *cache_hits);
/* WHICH compiler builds them (0.6.0).  The installation's own clang++ where one is found -- $MHX_JIT_CLANG (a path; "0" = none),
 * $ROCM_PATH/lib/llvm/bin/clang++, /opt/rocm/lib/llvm/bin/clang++ -- run as a child process on the same source, headers and options;
 * the hiprtc library otherwise, when that fails, or when option JIT_COMPILER = "hiprtc" ("clang" = no fall-back; $MHX_JIT_COMPILER is
 * the process-wide default of the option: a child process costs ~0.5 s more per kernel than hiprtc in-process, which a test suite that
 * compiles hundreds of small kernels may not want to pay).  Why: hiprtc is
 * whichever libhiprtc.so.7 / libamd_comgr.so.3 the PROCESS loaded first -- inside Python after `import torch` the wheel's bundled,
 * older compiler, whose cooperative RWMH kernel runs 7 % behind the one hipcc builds from the same text.  `compiler` receives
 * "clang++:<path>:<size>:<mtime>" or "" (none found: hiprtc only), ext_compiles how many of mhx_ctx_jit_counts' compilations it did. */
int mhx_ctx_jit_compiler(const mhx_ctx *ctx, char *compiler, size_t len, int64_t *ext_compiles);

/* Page-locked host memory for result tensors (the `Chains` array of ext/AdvancedMHMCMCChainsExt.jl:12-39 lives on the
 * host): device-to-host copies into it run at the link rate and asynchronously.  Any other host buffer works too --
 * mhx_run_sample_to_host registers it for the duration of the call. */
int mhx_host_alloc(size_t bytes, void **out);
/* Caller buffers this context page-locked for the duration of a mhx_run_sample_to_host call (hipHostRegister) and released
 * again: equal between calls, whatever path a call left by (every exit first drains both streams).  Either may be NULL. */
int mhx_ctx_host_pin_counts(const mhx_ctx *ctx, int64_t *registered, int64_t *released);
int mhx_host_free(void *p);

/* ---------------------------------------------------------------------------------------------
 * Targets.  Replaces DensityModel(f) / logdensity(model, x) (src/AdvancedMH.jl:52-54, :74-77). */
typedef enum {
    MHX_TARGET_ISO_GAUSS = 0,  /* logpdf(MvNormal(zeros(d), I), x);            params: none               */
    MHX_TARGET_CORR_GAUSS = 1, /* logpdf(MvNormal(zeros(d), Sigma), x);        params: inv(chol(Sigma)) packed lower */
    MHX_TARGET_IID_NORMAL = 2, /* README.md:29-31: theta=(mu,sigma), sum logpdf(Normal(mu,sigma), data); params: data */
    MHX_TARGET_BANANA = 3,     /* twisted Gaussian N(0, diag(100,1,...)) with x2 += b(x1^2-100); params: {b}   */
    MHX_TARGET_FUNNEL = 4,     /* Neal's funnel: x1~N(0,9), xk~N(0,exp(x1));  params: none               */
    MHX_TARGET_USER = 100      /* hiprtc-compiled user source                                              */
} mhx_target_kind;

int mhx_target_builtin(mhx_ctx *ctx, int kind, int dim, const void *params, size_t nparams,
                       mhx_target **out);
/* `src` must define   MHX_LOGDENSITY(x, d, data, ndata) { ... return lp; }   using x[k] and the
 * mhx_fma / mhx_log / mhx_exp / mhx_sqrt device functions, written against `mhx_real` and `MHX_R(literal)` so that one
 * text serves both dtypes (a source that says `float` is fp32-only); it is compiled by hiprtc and inlined
 * into the sampler kernels (the "JIT-lowered user log-density" of the design). */
int mhx_target_from_hip_source(mhx_ctx *ctx, const char *src, int dim, const void *data, size_t ndata,
                               mhx_target **out);
int mhx_target_destroy(mhx_target *t);
/* logdensity(model, x) for a batch: x [dim][n] (host) -> lp [n] (host).  src/AdvancedMH.jl:74 */
int mhx_target_eval(mhx_ctx *ctx, const mhx_target *t, const void *x, int n, void *lp);

/* ---------------------------------------------------------------------------------------------
 * Schedule.  Replaces the kwargs of AbstractMCMC.sample/mcmcsample [upstream]: N, discard_initial,
 * thinning, num_warmup.  Sample 1 is the state after `discard_initial` transitions from the
 * initial state; sample i is `thinning` transitions after sample i-1. */
typedef struct {
    int32_t n_samples;
    int32_t discard_initial;
    int32_t thinning;   /* >= 1 */
    int32_t num_warmup; /* RAM: transitions that adapt (step_warmup) */
} mhx_schedule;

/* ---------------------------------------------------------------------------------------------
 * Random-walk Metropolis-Hastings.  Replaces MetropolisHastings{RandomWalkProposal{_, <:MvNormal}}
 * (src/mh-core.jl:44-51, src/proposal.jl:13-25) and its step methods (src/mh-core.jl:76-117). */
typedef enum { MHX_PROP_ISO = 0, MHX_PROP_DIAG = 1, MHX_PROP_DENSE = 2 } mhx_proposal_kind;

typedef struct {
    int32_t dim;
    int32_t nchains;
    uint64_t seed;
    uint64_t first_chain;   /* global id of chain 0 of this shard */
    int32_t proposal_kind;  /* one of mhx_proposal_kind; src/proposal.jl:49-64 */
    double proposal_scale;   /* ISO: sigma of N(0, sigma^2 I) */
    const void *proposal_vec; /* DIAG: sigma_k [dim]; DENSE: chol(Sigma) packed lower [dim(dim+1)/2] */
    int32_t flags;          /* MHX_FLAG_* */
    const void *proposal_mean; /* NULL = zero mean.  mu[dim]: a drifting random walk x + mu + L z; its Hastings ratio
                               q(x | y) - q(y | x) (src/proposal.jl:58-64,190-192) is then non-zero and is computed.
                               Runs on the generic kernel. */
    int32_t reduce_lanes;   /* lanes that share one chain (power of two <= 64) for the separable catalogue
                               targets (MHX_TARGET_IID_NORMAL: 64 = a wave per chain, the few-chain kernel, which is also the
                               engine's choice up to 2048 chains); 0 = let the engine choose from nchains and dim, 1 = one lane per chain.
                               The value in effect is reported in mhx_stats.reduce_lanes: it fixes the
                               summation order of the log-density and therefore the exact chain. */
} mhx_rwmh_cfg;

#define MHX_FLAG_NO_JIT 1 /* never specialise with hiprtc; use the pre-built kernels only */
#define MHX_FLAG_GENERIC 2 /* force the generic (state-in-HBM) kernel even when a register kernel exists */
#define MHX_FLAG_EMCEE_SEQUENTIAL 8 /* Ensemble runs only: the reference's sweep (src/emcee.jl:39-58) -- walkers move one after
                                      another and pair with already-updated walkers (Gauss-Seidel), one wavefront, for
                                      fidelity checks at the reference's test sizes; the default is the parallel half-split */
#define MHX_FLAG_ZIGGURAT 16 /* RWMH and (round 5) MALA runs: standard normals by the table ZIGGURAT of the arithmetic spec (DESIGN.md
                                section 3.11: fp64 contexts 1024 equal-area layers and 64 bits per normal; fp32 contexts -- since 0.6.0 --
                                256 layers and 32 bits per normal; exact rejection sampling) instead of
                                Box-Muller -- a third fewer instructions per transition on the cooperative kernel (separable
                                catalogue targets) and on the register kernel (any target within its dimension limit, a user's
                                HIP source included), ISO / DIAG proposals.  It selects the STREAM of normals, so the chain differs
                                from the Box-Muller chain of the same seed (both target the same law); the value in effect is
                                reported in mhx_stats.normal_gen and fixes the chain bit for bit.  MHX_EINVAL where the run's
                                kernel has no ziggurat form (dense factors, the matrix-core and state-in-HBM kernels).  MALA: the
                                noise z of the Langevin proposal, on the lane-per-chain register kernel (any target with a gradient
                                within that kernel's dimension limit; reduce_lanes <= 1). */
#define MHX_FLAG_DENSE_FACTOR 32 /* Ensemble runs: treat the precision factor of a dense-Gaussian target as dense even when it is
                                   banded (exact zeros below a band of width <= 8 are otherwise detected and skipped -- same bits) */
#define MHX_FLAG_RAM_DEFERRED 64 /* RAM runs, dim <= 256: the DEFERRED-FACTOR form.  ram_adapt's rank-one step is S <- S chol(I +- c^2 U U')
                                   (src/RobustAdaptiveMetropolis.jl:153-173 with w = c S U), a triangular factor known from U and two
                                   scalars: up to 8 accepted updates stay pending as O(dim) triples -- proposals read the stored factor
                                   once and apply the pending factors to the noise first -- and are folded into S in ONE read + write pass
                                   (kernel variant 12): 9/8 reads + 1/8 writes of S per adapting step instead of 1 + 1.  The same Markov
                                   chain in exact arithmetic, ANOTHER ROUNDING than the reference's sequential lowrankupdate! sweeps
                                   (arithmetic spec 3.12; its own oracle twin, orc_ram_deferred): S S' agrees with the default form's to
                                   ~1e-15 relative per step, accept decisions may differ where |log u - log alpha| is at rounding level.
                                   Folds happen when 8 updates are pending, at the end of the warm-up and at the end of every launch (a
                                   sampling call is cut into launches of 4096 transitions), so the factor is whole whenever the host can
                                   see it; mhx_ram_watch_factors is refused (MHX_EINVAL). */
#define MHX_FLAG_STATIC_PROPOSAL 4 /* RWMH runs only: the proposal is a StaticProposal (src/proposal.jl:9-11,66-83) --
                                      the candidate is a draw mean + L z that ignores the current state (independence
                                      sampler) and the ratio is logpdf(p, x) - logpdf(p, y) */

int mhx_rwmh_create(mhx_ctx *ctx, const mhx_target *t, const mhx_rwmh_cfg *cfg, mhx_run **out);

/* A proposal made of independent univariate components (src/proposal.jl:23-35 with a vector of Distributions univariates): component
 * k of a RandomWalkProposal / StaticProposal is one of the families below, its two parameters as in Distributions.jl (Exponential
 * has one; sigma, theta, alpha > 0, a < b, all finite).  The draws, the streams they take their bits from and the unnormalised
 * log-kernels the acceptance ratio sums are the arithmetic spec's section 3.13. */
typedef enum {
    MHX_FAMILY_NORMAL = 0,        /* Normal(mu, sigma) */
    MHX_FAMILY_UNIFORM = 1,       /* Uniform(a, b) */
    MHX_FAMILY_LAPLACE = 2,       /* Laplace(mu, theta) */
    MHX_FAMILY_CAUCHY = 3,        /* Cauchy(mu, sigma); TDist(1) is Cauchy(0, 1) */
    MHX_FAMILY_EXPONENTIAL = 4,   /* Exponential(theta): p0 = theta, p1 unused */
    MHX_FAMILY_GAMMA = 5,         /* Gamma(alpha, theta) */
    MHX_FAMILY_INVERSE_GAMMA = 6  /* InverseGamma(alpha, theta) */
} mhx_family;

typedef struct {
    int32_t family;   /* one of mhx_family */
    int32_t reserved; /* 0 */
    double p0;
    double p1;
} mhx_proposal_component;

#define MHX_FLAG_SYMMETRIC_PROPOSAL 128 /* mhx_rwmh_create_components, random walk only: the proposal was declared symmetric
                                           (RandomWalkProposal{true}, src/proposal.jl:195) -- the ratio q(x - y) - q(y - x) is not formed.
                                           mhx_rwmh_create_conditional: walk or static */

/* An RWMH run whose proposal is comps[0 .. ncomps-1], ncomps == cfg->dim; cfg->proposal_kind / _scale / _vec / _mean are ignored,
 * MHX_FLAG_STATIC_PROPOSAL selects y = xi with the ratio q(x) - q(y) (else y = x + xi with q(x - y) - q(y - x)).  One lane per chain,
 * Box-Muller normals: MHX_FLAG_ZIGGURAT, reduce_lanes > 1, a bad parameter and (at mhx_run_sample) MHX_SAVE_MOMENTS are MHX_EINVAL.
 * Kernel variant 13 in both of its forms: run-time specialised to the pattern of families with the state in registers (dim <= 32 in
 * fp64, 48 in fp32: what compiles without scratch memory), or -- MHX_FLAG_GENERIC / MHX_FLAG_NO_JIT / larger dim -- the pre-built state-in-HBM form; the same chain bit for
 * bit.  A one-sided family in a random walk never accepts (q(x - y) = -Inf), exactly as the reference behaves. */
int mhx_rwmh_create_components(mhx_ctx *ctx, const mhx_target *t, const mhx_rwmh_cfg *cfg, const mhx_proposal_component *comps,
                               int32_t ncomps, mhx_run **out);

/* A CONDITIONAL proposal: the function proposals of src/proposal.jl:92-126 -- StaticProposal(x -> Normal(x, 1)),
 * RandomWalkProposal(x -> Laplace(x, 1)).  Component k keeps the fixed family comps[k].family; its parameters are a function of the
 * whole state, given as HIP source (the arithmetic: DESIGN.md section 3.14):
 *
 *     MHX_PROPOSAL_PARAMS(x, p, d, data, ndata) { p.set(0, 1, MHX_R(0.5) + x[0] * x[0]); }
 *
 * x[j] reads coordinate j of the state, p.set(k, j, value) sets parameter j (0 or 1, as in mhx_proposal_component) of component k, data
 * points to the ndata reals (of the context's width) passed here.  An entry the source does not set keeps comps[k].p0 / p1, which
 * must be valid parameters on their own.  The shape alpha of a Gamma / InverseGamma component cannot depend on the state (its lgamma
 * would not cancel, and the sampler's constants are derived from it on the host): p.set(k, 0, .) on such a component has no effect.
 * Every transition evaluates p at the candidate y and checks it (sigma, theta > 0, a < b, everything finite); a candidate whose
 * parameters are not a distribution's is REJECTED -- the one departure from the reference, which would throw from the
 * distribution's constructor at the next step.  The ratio is (K(p(y); x - y) - K(p(x); y - x)) + (Z(p(y)) - Z(p(x))) for a walk,
 * (K(p(y); x) - K(p(x); y)) + (Z(p(y)) - Z(p(x))) with MHX_FLAG_STATIC_PROPOSAL; MHX_FLAG_SYMMETRIC_PROPOSAL (here allowed with a
 * static proposal too: StaticProposal{true}, src/proposal.jl:195-196) leaves it out.  A map that sets nothing, or constants, runs the
 * chain of mhx_rwmh_create_components bit for bit.
 * Kernel variant 14, compiled at run time only, in two forms with the same chain: state, candidate and both parameter sets in
 * registers (dim <= 20 in fp64, 32 in fp32: what compiles without scratch memory), or -- MHX_FLAG_GENERIC / larger dim -- in HBM.  MHX_EINVAL: MHX_FLAG_NO_JIT (nothing is
 * pre-built), MHX_FLAG_ZIGGURAT, reduce_lanes > 1, MHX_SAVE_MOMENTS at mhx_run_sample, mhx_run_init without initial_params (there is no
 * distribution to draw a first state from) and initial or mhx_run_set_state states at which p is not valid.  A compile error in
 * params_src is MHX_EJIT with the compiler's log in mhx_last_error, as for mhx_target_from_hip_source; a user log-density and a
 * parameter map compile together in one module. */
int mhx_rwmh_create_conditional(mhx_ctx *ctx, const mhx_target *t, const mhx_rwmh_cfg *cfg, const mhx_proposal_component *comps,
                                int32_t ncomps, const char *params_src, const void *data, size_t ndata, mhx_run **out);

/* A COMPOSITE proposal: the reference's Array{Proposal} and NamedTuple{Proposal} (src/proposal.jl:128-175,198-240) -- an ordered
 * list of blocks of components, each block with its own kind, its own symmetric flag and, optionally, parameters that depend on the
 * block's own slice of the state (the arithmetic: DESIGN.md section 3.15).  blocks[b] covers components first .. first + count - 1;
 * the blocks are contiguous, in order, and cover 0 .. dim-1 exactly.  flags: MHX_BLOCK_STATIC (y_k = xi_k, else y_k = x_k + xi_k),
 * MHX_BLOCK_SYMMETRIC (the block adds nothing to the ratio: the user is trusted); reserved must be 0. */
typedef struct {
    int32_t first, count, flags, reserved;
} mhx_proposal_block;
#define MHX_BLOCK_STATIC 1
#define MHX_BLOCK_SYMMETRIC 2

/* An RWMH run under the composite proposal (comps, blocks).  mapped[k] (or mapped == NULL: nothing is) says which parameters of
 * component k the source sets: bit j set = p.set(k, j, .) of params_src, an MHX_PROPOSAL_PARAMS source as for
 * mhx_rwmh_create_conditional, with GLOBAL indices k and x[j]; a p.set on an entry not declared mapped is ignored.  params_src is NULL
 * or "" when nothing is mapped.  Component k draws exactly as in mhx_rwmh_create_components / _conditional, keyed by its global index,
 * so the draws do not depend on the grouping; every block not declared symmetric adds r_b = (K_b(p(y); .) - K_b(p(x); .)) +
 * (Z_b(p(y)) - Z_b(p(x))) to the ratio, in block order; p(y) of every mapped component is checked at every step and an invalid
 * candidate is rejected.  One block reproduces mhx_rwmh_create_conditional bit for bit, and mhx_rwmh_create_components when nothing is
 * mapped.  With nothing mapped mhx_run_init(run, NULL) draws the first state x = 0 + xi from the components, for both kinds.
 * Kernel variant 15, compiled at run time only, in two forms with the same chain: state, candidate and the MAPPED parameters in
 * registers (nothing mapped: dim <= 32 in fp64, 48 in fp32; else 2 dim + mapped components + half the non-symmetric blocks with a
 * mapped component <= 60 / 96: what compiles without scratch
 * memory), or -- MHX_FLAG_GENERIC / larger shapes -- in HBM.  MHX_EINVAL: blocks that do not tile 0 .. dim-1 in order, unknown block
 * flags or a non-zero reserved, MHX_FLAG_STATIC_PROPOSAL / MHX_FLAG_SYMMETRIC_PROPOSAL in cfg->flags (the blocks carry them), a mapped
 * shape alpha of a Gamma family, a mask without source or source without a mask, and everything mhx_rwmh_create_conditional refuses
 * (MHX_FLAG_NO_JIT, MHX_FLAG_ZIGGURAT, reduce_lanes > 1, MHX_SAVE_MOMENTS, init without initial_params when anything is mapped, states at
 * which p is not valid).  A compile error in params_src is MHX_EJIT with the compiler's log in mhx_last_error. */
int mhx_rwmh_create_composite(mhx_ctx *ctx, const mhx_target *t, const mhx_rwmh_cfg *cfg, const mhx_proposal_component *comps,
                              int32_t ncomps, const mhx_proposal_block *blocks, int32_t nblocks, const int32_t *mapped,
                              const char *params_src, const void *data, size_t ndata, mhx_run **out);

/* ---------------------------------------------------------------------------------------------
 * Affine-invariant ensemble.  Replaces Ensemble{StretchProposal} (src/emcee.jl:1-4, :63-68), its
 * step (:14-24), sweep (:39-58) and stretch move (:70-102).  The device sweep is the parallel
 * half-split of the walker set, not the reference's sequential loop. */
typedef struct {
    int32_t dim;
    int32_t nwalkers;
    uint64_t seed;
    uint64_t ensemble_id;    /* < 2^32: one word of the RNG counter (walker index is the other) */
    double stretch;          /* a = 2.0 */
    int32_t flags;          /* MHX_FLAG_*; MHX_FLAG_EMCEE_SEQUENTIAL selects the reference's own sweep */
    int32_t reduce_lanes;   /* lanes per walker (dense-Gaussian target): 0 = engine's choice, 1 = one lane per walker */
    /* the distribution StretchProposal wraps (src/emcee.jl:63-68), used ONLY for the initial walkers (:29-34: W draws
     * from it): a (Mv)Normal  mu + L z  drawn on the device by mhx_run_init(run, NULL).  init_kind < 0: none given --
     * mhx_run_init then requires the walkers (any other prior is drawn by the host). */
    int32_t init_kind;      /* mhx_proposal_kind, or -1 */
    double init_scale;      /* ISO: sigma */
    const void *init_vec;   /* DIAG: sigma_k [dim]; DENSE: chol(Sigma) packed lower [dim(dim+1)/2] */
    const void *init_mean;  /* mu [dim] or NULL */
    int32_t n_ensembles;    /* 0.6.0: E independent ensembles in ONE run -- `sample(model, Ensemble(W, ..), MCMCThreads(), N, nchains)`
                               (README.md:135-148) runs nchains ENSEMBLES, and emcee is run at sizes (test/emcee.jl:24: 1000 walkers) that
                               leave the chip idle one at a time.  0 / 1 = one.  Ensemble e carries id ensemble_id + e in its RNG counters
                               and is bit for bit the run of that id alone; its walkers are columns e W .. e W + W - 1 of every
                               [..][E W] array (x, samples, accepted; mhx_run_shape reports E W chains).  Every launch takes E as a second
                               grid dimension; an ensemble of <= 1024 walkers (kernel variant 6) is one persistent block, so E of them
                               occupy E CUs.  The sharded-ensemble building blocks below (mhx_emcee_half_step ...) need E = 1. */
} mhx_emcee_cfg;

int mhx_emcee_create(mhx_ctx *ctx, const mhx_target *t, const mhx_emcee_cfg *cfg, mhx_run **out);

/* ---------------------------------------------------------------------------------------------
 * Robust adaptive Metropolis.  Replaces RobustAdaptiveMetropolis (src/RobustAdaptiveMetropolis.jl:75-87),
 * its state (:99-114) and step / step_warmup (:175-278). */
typedef struct {
    int32_t dim;
    int32_t nchains;
    uint64_t seed;
    uint64_t first_chain;
    double alpha;            /* 0.234 */
    double gamma;            /* 0.6 */
    double eig_lo, eig_hi;   /* eigenvalue (diagonal) bounds, 0 and +inf */
    int32_t flags;           /* MHX_FLAG_RAM_DEFERRED */
} mhx_ram_cfg;

int mhx_ram_create(mhx_ctx *ctx, const mhx_target *t, const mhx_ram_cfg *cfg, mhx_run **out);
/* in/out Cholesky factors, [nchains][dim(dim+1)/2]; S == NULL on set means identity */
int mhx_ram_set_factor(mhx_run *run, const void *S);
/* the same factor for every chain (RobustAdaptiveMetropolis(S = ...), :198-206): S [dim(dim+1)/2] */
int mhx_ram_set_factor_all(mhx_run *run, const void *S);
int mhx_ram_get_factor(mhx_run *run, void *S, uint8_t *status /* [nchains] or NULL */);
/* running min / max of diag(S) over every adapted state so far, [dim][nchains] each */
int mhx_ram_get_diag_range(mhx_run *run, void *diag_min, void *diag_max);
/* the rest of RobustAdaptiveMetropolisState (src/RobustAdaptiveMetropolis.jl:99-114): log_alpha [nchains] reals = the log
 * acceptance ratio min(lp' - lp, 0) of each chain's latest transition (kept bounded at 0 so that users can average
 * exp(log_alpha), :141-147); *eta = the adaptation step size iteration^-gamma of the latest warm-up transition (0 before
 * any, :211); isaccept [nchains]; *iteration = 1 + transitions so far.  Any pointer may be NULL. */
int mhx_ram_get_adapt_state(mhx_run *run, void *log_alpha, double *eta, uint8_t *isaccept, uint64_t *iteration);
/* The same statistics for EVERY recorded step of the last mhx_run_sample / mhx_run_sample_to_host that kept samples -- what a
 * `callback(rng, model, sampler, sample, state, i)` reads off `state` after each saved step in the reference
 * (test/RobustAdaptiveMetropolis.jl:11-28,55): log_alpha [n_samples][nchains] reals = state.logα after the recorded transition
 * (min(lp' - lp, 0): average exp(log_alpha) for the acceptance rate, RAM.jl:141-147; sample 1 of an un-discarded call carries
 * the state's own value, 0 right after init, :211), eta [n_samples] doubles = state.η (iteration^-gamma of the latest adapting
 * transition at or before that step; the same for every chain).  state.isaccept is the `accepted` tensor.  Either may be NULL.
 * `capacity` = the number of samples the two buffers hold: fewer than the last call recorded is MHX_EINVAL (nothing is written);
 * n_recorded (may be NULL) receives that count -- with both buffers NULL the call is just this query. */
int mhx_ram_get_step_stats(mhx_run *run, void *log_alpha, double *eta, int64_t capacity, int64_t *n_recorded);

/* state.S of a few WATCHED chains after EVERY recorded step -- what a reference callback that stores `state.S` keeps
 * (test/RobustAdaptiveMetropolis.jl:11-28; :57-69 checks the eigenvalue bounds on that record).  mhx_ram_watch_factors(run, chains, n)
 * names the chains (indices into this run, n = 0 switches it off); every later mhx_run_sample / mhx_run_sample_to_host that keeps
 * samples also keeps S [n_samples][n][dim (dim + 1) / 2] (packed lower, row-major, like mhx_ram_get_factor); a watched run ends a
 * launch at every recorded transition, others are unaffected.  mhx_ram_get_watched_factors copies the record out: `capacity` = the
 * number of samples S holds (fewer than recorded: MHX_EINVAL); n_recorded / n_watched may be NULL; S == NULL just queries them. */
int mhx_ram_watch_factors(mhx_run *run, const int32_t *chains, int32_t n);
int mhx_ram_get_watched_factors(mhx_run *run, void *S, int64_t capacity, int64_t *n_recorded, int32_t *n_watched);

/* ---------------------------------------------------------------------------------------------
 * Metropolis-adjusted Langevin.  Replaces MALA (src/MALA.jl:1-11), GradientTransition (:14-19) and its step
 * (:54-93) for the standard proposal  g -> MvNormal((sigma2/2) g, sigma2 I)  of the reference's tests
 * (test/runtests.jl:291,352).  Gradients are analytic for the catalogue targets; a user source must also
 * define  MHX_LOGDENSITY_AND_GRADIENT(x, g, d, data, ndata) { ... g.set(k, dlp_dxk); ... return lp; }
 * (the reference throws in check_capabilities, src/MALA.jl:42-52, when no gradient is available).
 * mhx_run_init requires initial_params (src/MALA.jl:37). */
typedef struct {
    int32_t dim;
    int32_t nchains;
    uint64_t seed;
    uint64_t first_chain;
    double sigma2;
    int32_t flags;
    int32_t reduce_lanes;   /* lanes per chain (separable catalogue targets; 4 = the matrix-core kernel of the dense Gaussian target): 0 = engine's choice, 1 = one lane per chain; the
                               value in effect (mhx_stats.reduce_lanes) fixes the summation order of the three sums of a step */
} mhx_mala_cfg;

int mhx_mala_create(mhx_ctx *ctx, const mhx_target *t, const mhx_mala_cfg *cfg, mhx_run **out);

/* ---------------------------------------------------------------------------------------------
 * Running chains.  mhx_run_init == the initial AbstractMCMC.step (src/mh-core.jl:76-86,
 * src/emcee.jl:29-34, src/RobustAdaptiveMetropolis.jl:175-214): x0 = initial_params if given, else
 * a draw (RWMH: from the proposal; RAM: randn(d); Ensemble: W draws from the (Mv)Normal of cfg.init_*, else required).
 * mhx_run_sample == the mcmcsample loop + bundle_samples into the device sample buffer.  It may be
 * called repeatedly; each call continues the chains (counter-based RNG => resumable).  RWMH: a -0.0 coordinate of a caller's state
 * (here and in mhx_run_set_state) enters the chain as +0.0 -- equal under ==, so `chain[1].params == initial_params` holds. */
int mhx_run_init(mhx_run *run, const void *initial_params /* host [dim][nchains] or NULL */);
/* save_samples: 0 = keep nothing, 1 = sample tensor, 2 = running moments only (per chain and parameter the
 * mean / M2 of the states the schedule selects; for runs whose sample tensor would not fit, e.g.
 * 262 144 chains x 1000 dims -- mhx_run_diagnostics then works from the moments; RWMH on the cooperative or
 * generic kernel) */
#define MHX_SAVE_NONE 0
#define MHX_SAVE_SAMPLES 1
#define MHX_SAVE_MOMENTS 2
int mhx_run_sample(mhx_run *run, const mhx_schedule *sched, int save_samples);

/* copy the sample buffer of the last mhx_run_sample to the host (either pointer may be NULL) */
int mhx_run_get_samples(mhx_run *run, void *samples, uint8_t *accepted);
/* mhx_run_sample + mhx_run_get_samples in ONE call with the copy overlapped: what `sample(model, sampler, N)` returns is
 * a host container (bundle_samples, src/AdvancedMH.jl:80-104, ext/AdvancedMHMCMCChainsExt.jl:12-39).  The schedule is cut
 * into slabs of |slab_samples| saved samples (0 = about 256 MiB); the kernels fill one device slab while the previous one
 * drains to `samples` [n_samples][dim+1][nchains] / `accepted` [n_samples][nchains] (NULL = not wanted) on a second
 * stream.  A tensor that fits into HBM stays there as well (mhx_run_device_samples and the diagnostics work as after
 * mhx_run_sample); one that does not -- or slab_samples < 0 -- goes through TWO alternating slabs and the device keeps
 * nothing (mhx_run_device_samples then reports 0 samples): n_samples is bounded by host memory, not by HBM.  Blocking; the
 * buffers are complete on return.  Bit-identical to mhx_run_sample + mhx_run_get_samples.
 * mhx_stats.kernel_ms then spans the kernels including their waits for a free slab, wall_ms the whole call. */
int mhx_run_sample_to_host(mhx_run *run, const mhx_schedule *sched, void *samples, uint8_t *accepted, int32_t slab_samples);

/* The ACCEPT-COMPACTED form of that return path (0.6.0).  A rejected transition re-emits the previous Transition
 * (src/mh-core.jl:109-114; src/emcee.jl:93-101; src/RobustAdaptiveMetropolis.jl:148-150), so at the acceptance rates these samplers
 * are tuned to three quarters of a save-all tensor repeat the row above, byte for byte.  With thinning == 1 and >= 1024 chains
 * (or context option HOST_COMPACT = 1; 0 switches it off) mhx_run_sample_to_host therefore moves, per slab, one BLOCK over the link:
 * a bit per (sample, chain) -- "this chain's column [dim+1] differs from the sample before", found by comparing the bits of the two
 * columns on the device, whatever the sampler -- and the columns of the chains whose bit is set; sample 0 of a call travels whole.
 * Host threads inside the library (context option HOST_THREADS; default = what the process may use: affinity mask and cgroup CPU
 * quota, at most 64) rebuild the caller's tensor from the blocks with non-temporal stores while the next slab is in flight.  The
 * caller's buffers need not be page-locked on this path (the CPU writes them) and none is registered.  Bit-identical to the plain
 * path by construction.  C2 in fp64: 13.4 GB of tensor per 250 transitions of 65 536 chains cross the link as 3.2 GB.
 *
 * A block:  mhx_compact_hdr | mask u64[count][words] | rank u32[count][words] (pad to 8) | accepted u8[count][nchains] (pad to 8)
 *           | payload: for sample i  elem[dim1][m_i]   (m_i = set bits of mask[i][.]; row k holds parameter k of the changed
 *           chains in chain order; parameter dim1-1 is lp)
 * rank[i][w] = set bits of the block's masks before word (i, w) in (sample, word) order, so sample i's payload starts at element
 * dim1 * rank[i][0] and chain c of it sits at  rank[i][c/64] - rank[i][0] + popcount(mask[i][c/64] & ((1 << c%64) - 1)). */
#define MHX_COMPACT_MAGIC 0x4358484du /* "MHXC" */
typedef struct {
    uint32_t magic;
    uint32_t elem_bytes;      /* 4 | 8: the run's dtype */
    uint32_t dim1;            /* dim + 1 */
    uint32_t nchains;
    uint64_t first_sample;    /* row of the call's tensor the block starts at */
    uint32_t count;           /* samples in the block */
    uint32_t words;           /* (nchains + 63) / 64 */
    uint64_t total_changed;   /* sum of m_i */
    uint64_t payload_offset;  /* bytes from the start of the block */
    uint64_t block_bytes;     /* payload_offset + total_changed * dim1 * elem_bytes */
    uint64_t reserved_;
} mhx_compact_hdr;            /* 64 bytes */
/* Expand ONE block into the caller's whole tensor samples [n_samples][dim1][nchains] (and accepted [n_samples][nchains], or NULL);
 * blocks of a call are expanded in order (a block reads the row above its first sample).  The block is validated (sizes, ranks
 * against masks) before anything is written: MHX_EINVAL otherwise.  For hosts that move samples with their own transport -- the
 * workers of Distributed.jl or MPI ranks ship blocks, not tensors.  threads <= 0: as above.  Needs no GPU. */
int mhx_compact_expand(const void *block, size_t block_bytes, void *samples, uint8_t *accepted, int64_t n_samples, int32_t threads);

/* What the last mhx_run_sample_to_host of the run moved, and how */
typedef struct {
    uint64_t tensor_bytes;    /* samples + accepted delivered to the caller */
    uint64_t wire_bytes;      /* bytes of device-to-host copies behind them */
    double link_ms;           /* time the copies occupied the link (stream events, summed over the slabs) */
    double expand_ms;         /* compacted path: time the host threads spent on blocks (first worker in to last worker out, summed) */
    int32_t compact;          /* 1: the accept-compacted path ran */
    int32_t threads;          /* host threads that expanded */
    int32_t slabs;
    int32_t ring;             /* 1: two alternating device slabs (the device kept nothing) */
} mhx_host_stats;
int mhx_run_host_stats(mhx_run *run, mhx_host_stats *out);
/* getparams / setparams!! (src/AdvancedMH.jl:146-157, src/RobustAdaptiveMetropolis.jl:116-121) */
int mhx_run_get_state(mhx_run *run, void *x, void *lp, uint32_t *accept_counts);
int mhx_run_set_state(mhx_run *run, const void *x /* lp is recomputed */);

/* Checkpoint / resume -- the `state` half of AbstractMCMC's (sample, state) = step(...) and of upstream's
 * `initial_state` keyword (src/mh-core.jl:92-117, src/emcee.jl:14-24, src/RobustAdaptiveMetropolis.jl:99-114): the
 * complete state of a run -- positions, cached log-densities, accept bookkeeping, the RNG step counter with its
 * seed and global ids, and per sampler the RAM factors / selectors / diagonal ranges, the MALA gradients, the
 * static proposal's log-densities -- as one host blob.  A run created with the same sampler, model, dim and chain
 * count continues the saved one bit for bit after mhx_run_load_state (its own seed / first_chain are replaced). */
int mhx_run_state_size(mhx_run *run, size_t *bytes);
int mhx_run_save_state(mhx_run *run, void *blob, size_t bytes);
int mhx_run_load_state(mhx_run *run, const void *blob, size_t bytes);

typedef struct {
    uint64_t transitions;      /* chain-steps executed by the last mhx_run_sample (all chains)         */
    uint64_t accepted;         /* accepted proposals among them (wavefront ballot + popcount reduction) */
    double kernel_ms;          /* device time of the sampler kernels (hipEvent)                         */
    double wall_ms;            /* host wall time of the call                                            */
    int32_t kernel_variant;    /* 0 generic (HBM state), 1 pre-built register kernel, 2 hiprtc-specialised register
                                  kernel, 3 pre-built cooperative kernel, 4 hiprtc-specialised cooperative kernel,
                                  5 hiprtc-specialised cooperative kernel for the dense Gaussian target (RWMH),
                                  6 a small ensemble (<= 1024 walkers, lane per walker) as ONE persistent block: a whole sampling
                                  call per launch, block barriers between the half-steps,
                                  7 the reference's sequential ensemble sweep (MHX_FLAG_EMCEE_SEQUENTIAL),
                                  8 matrix-core kernel: RWMH / MALA with one dense factor for all chains (dense Gaussian
                                  target and / or dense proposal) on v_mfma_*_16x16x4, reduction shape 4,
                                  9 scalar-factor form of the cooperative stretch move (dense precision factor: a lane owns a
                                  walker during A y, the wave-uniform factor entry is a DPP-broadcast / SGPR operand; reduction
                                  shape = reduce_lanes = waves per block),
                                  10 matrix-core form of the stretch move (dense precision factor, dim <= 64 in fp64 / 128 in fp32:
                                  4 lanes per walker, A y of the 16 walkers of a wave on v_mfma_*_16x16x4, the factor's operands
                                  fetched into registers from an image built once per run; reduction shape 4),
                                  11 a WAVE per chain (RWMH on the data-sum target MHX_TARGET_IID_NORMAL with few chains -- the
                                  reference's own README example, one chain: the 64 lanes split the likelihood's terms, the draws of
                                  64 steps are made side by side off the chain's critical path; reduction shape 64),
                                  12 RAM with a deferred factor (MHX_FLAG_RAM_DEFERRED),
                                  13 a proposal of univariate family components (mhx_rwmh_create_components), lane per chain: the
                                  run-time specialised register form or the pre-built state-in-HBM form, the same chain,
                                  14 a conditional proposal (mhx_rwmh_create_conditional), lane per chain, compiled at run time:
                                  the register form or the state-in-HBM form, the same chain,
                                  15 a composite proposal (mhx_rwmh_create_composite): blocks of components with their own kind,
                                  symmetric flag and parameter map; lane per chain, compiled at run time, the same two forms,
                                  16 a tempered run (mhx_rwmh_create_tempered): ladders of temperatures in consecutive lanes, swaps
                                  across lanes inside the step kernel; the run-time specialised register form or the state-in-HBM
                                  form (pre-built for the catalogue targets), the same chain,
                                  17 a tempered run whose ladders adapt (mhx_rwmh_create_tempered_adaptive): the same two forms,
                                  18 a tempered run anchored at a reference density (mhx_rwmh_create_tempered_anchored): the same
                                  two forms,
                                  19 an adaptive random walk (mhx_rwmh_create_adaptive): an adapting and a frozen phase, each with
                                  the same two forms */
    int32_t launches;
    int32_t reduce_lanes;      /* lanes per chain in effect (1 unless a cooperative kernel runs) */
    int32_t dtype;             /* mhx_dtype of the run's context */
    int32_t normal_gen;        /* 0 Box-Muller, 1 ziggurat (MHX_FLAG_ZIGGURAT): how the run turns stream bits into normals */
    int32_t factor_band;       /* Ensemble runs on a dense-Gaussian target: the bandwidth of the precision factor the kernel exploits
                                  (0 = diagonal, 1 = bidiagonal: an AR(1) / Markov model, ...), -1 = none (dense form, other samplers) */
    int32_t tainted;           /* 1: a probe / fault-injection option of the tools build was set on the run's context -- the chains of
                                  such a run may be INVALID (timing probes skip work).  Always 0 from libmhx.so. */
    int32_t register_form;     /* kernel variants 13 .. 19: 1 = the run is stepped by the run-time specialised register form, 0 = by
                                  the state-in-HBM form (MHX_FLAG_GENERIC or a shape outside the register rule); 0 for every other variant.
                                  Variant 19: of the phase the run's next transition belongs to */
} mhx_stats;
int mhx_run_stats(mhx_run *run, mhx_stats *out);
/* The name of the run's kernel form -- kernel_variant spelled out ("generic", "reg", "coop", "coop_jit", "wave", ...) -- with the body
   it was compiled as where a form has two: "coop_pairs" / "coop_jit_pairs" is the cooperative kernel as generator / consumer wave
   pairs (option COOP_PAIRS; same chains, kernel_variant stays 3 / 4).  A static string; "" for a NULL run. */
const char *mhx_run_form_name(const mhx_run *run);
/* dimension and number of chains (walkers) of a run; either pointer may be NULL */
int mhx_run_shape(const mhx_run *run, int32_t *dim, int32_t *nchains);

/* device pointers of the sample buffer of the last mhx_run_sample (for zero-copy consumers on the
 * same HIP runtime, e.g. diagnostics or a torch tensor view); valid until the next sample/destroy */
int mhx_run_device_samples(mhx_run *run, void **samples, void **accepted, int64_t *n_samples);

int mhx_run_destroy(mhx_run *run);

/* ---------------------------------------------------------------------------------------------
 * Diagnostics on the device sample buffer of the last mhx_run_sample (what MCMCChains prints for the
 * reference, README.md:59-63).  Per parameter p (dim parameters, then lp), each array [dim+1]:
 *   sum_m  = sum_c m_c        sum_m2 = sum_c m_c^2        sum_v = sum_c s2_c
 * with m_c / s2_c the mean / unbiased variance of chain c over the N draws.  They are returned
 * un-normalised so that shards on several GPUs combine with ONE all-reduce of 3(dim+1)+1 doubles
 * (DESIGN.md section 8); R-hat and the between-chain ESS follow on the host:
 *   W = sum_v/C, Vm = (sum_m2 - sum_m^2/C)/(C-1), var+ = (N-1)/N W + Vm,
 *   R-hat = sqrt(var+/W), ESS_between = C var+/Vm.
 * ess[p] (optional) = C N / tau_p with tau_p from Geyer's initial monotone sequence on the multi-chain
 * autocorrelations rho_t = 1 - (W' - A_t)/var+ (Vehtari et al. 2021, eq. 10: A_t the lag-t autocovariance
 * averaged over the first `ess_chains` chains, W' = A_0, var+ from all chains; one chain: A_t/A_0), lags
 * 0..max_lag; it is returned NEGATED when the sequence was still positive at max_lag (|ess| is then an upper
 * bound).  With cfg.split every chain is two half-chains: C -> 2C, N -> floor(N/2) in all of the above (the last draw of an odd N
 * is not read).  Lags: nlag = min(max_lag + 1, N) rounded down to even, summed in pairs P_m = rho_2m + rho_2m+1 up to the first
 * P_m <= 0, each pair no larger than the one before; tau = -1 + 2 sum P_m, never below 1e-3.  Any max_lag is served: the lags are
 * launched in slices of the device's grid limit (hipDeviceProp_t::maxGridSize[2]).
 * Rows without an answer say so -- they never report the C N draws of a perfect sampler:
 *   - a row without variance in the chains read (a parameter that never moved: A_0 == 0; or var+ == 0): ess = NaN.  The mean of
 *     a chain is taken about its first draw, so a chain that repeats ANY value has m_c equal to it and s2_c == 0 exactly.  Its
 *     R-hat (from the sums, W == 0) is NaN when all chains share the constant and Vm comes out 0 (exact when the constant and its
 *     square times C are representable), +inf when they differ (Vm > 0);
 *   - a row that holds a non-finite draw (NaN of either sign, +inf, -inf -- the lp row of a chain outside the support) among the
 *     draws read: sum_m, sum_m2, sum_v and ess are all NaN (never +-inf), and so are R-hat and the between-chain ESS;
 *   - no such row changes the numbers of any other row. */
typedef struct {
    int32_t max_lag;    /* 0: skip the autocovariance ESS (ess[] = NaN) */
    int32_t ess_chains; /* chains used for the autocovariances, 0 = all */
    int32_t split;      /* 1: every chain counts as two half-chains of floor(N/2) draws (split R-hat, Vehtari et al.
                           2021): the sums then run over 2 nchains chains, and so do the autocovariances */
} mhx_diag_cfg;
int mhx_run_diagnostics(mhx_run *run, const mhx_diag_cfg *cfg, double *sum_m, double *sum_m2,
                        double *sum_v, double *ess /* each [dim+1], any may be NULL */);

/* ---- building blocks of ONE ensemble sharded over several GPUs (src/emcee.jl:14-24, parallel half-split form).
 * (mhx_emcee_half_step is stream-ordered, not blocking: the exchange and the next half-step queue behind it.)
 * Every rank holds the whole ensemble; for each half h of a sweep every rank moves its own slice
 * [begin, begin + count) of the moving half with mhx_emcee_half_step and the ranks then exchange the slices (an
 * all-gather of the walker-major rows and the lp / accept arrays that mhx_emcee_device_state exposes -- device
 * pointers, valid for the life of the run; pitch = floats per walker row); mhx_emcee_end_sweep advances the RNG
 * sweep counter after both halves.  Walkers carry their global index in the RNG counter, so any partition moves
 * exactly the walkers a single GPU would (advancedmh.jl_amd/mhx/dist.py: ShardedEnsemble). */
int mhx_emcee_half_step(mhx_run *run, int half, int begin, int count);
int mhx_emcee_end_sweep(mhx_run *run);
int mhx_emcee_device_state(mhx_run *run, void **xw, int32_t *pitch /* reals per walker row */, void **lp, uint32_t **acc_count,
                           uint8_t **last_acc);

/* The exchange step of the sharded ensemble as stream-ordered pieces (what mhx_comm_allgather_walkers does with RCCL; a
 * host that brings its own transport -- MPI, Distributed.jl -- uses them directly): every rank's slice of half `half` is
 * walkers [cnt q / world, cnt (q+1) / world) of that half; *stride = bytes of one rank's part of the staging buffer
 * ([world][stride], device memory), *stream = the hipStream_t the run's kernels are queued on.  pack writes this rank's
 * slice (rows, lp, accept counts, last accept flags) to `part`, unpack scatters the parts of all OTHER ranks into the run. */
int mhx_emcee_exchange_plan(mhx_run *run, int half, int world, size_t *stride, void **stream);
int mhx_emcee_exchange_pack(mhx_run *run, int half, int rank, int world, void *part);
int mhx_emcee_exchange_unpack(mhx_run *run, int half, int rank, int world, const void *stage, size_t stride);

/* ---- building block of the order statistics of ONE set of draws sharded over several GPUs (mhx_group_order_statistics; a host
 * that brings its own transport adds the histograms of its ranks the same way).  One pass of the radix select described at
 * mhx_run_order_statistics below over this run's sample tensor: for parameter slot i (row params[i]) and group g < ngroups[i],
 *   hist[((i * gstride + g) << digit_bits) + b] = number of draws whose key has the prefix prefixes[i * gstride + g] above bit
 *   shift + digit_bits (right-aligned) and the digit (key >> shift) & (2^digit_bits - 1) == b
 * (shift + digit_bits == key width, 32 or 64: the first pass, one group holding every draw, its prefix ignored).  1 <= digit_bits
 * <= 11.  hist is HOST memory of (nparams * gstride) << digit_bits counters; those of the groups in use are overwritten.  Counts
 * are integers: the histograms of shards add, in any order, to the histogram of the whole.  Blocking. */
int mhx_run_select_histogram(mhx_run *run, const int32_t *params, int32_t nparams, const uint64_t *prefixes, const int32_t *ngroups,
                             int32_t gstride, int32_t shift, int32_t digit_bits, uint64_t *hist);

/* ---------------------------------------------------------------------------------------------
 * Collectives (RCCL over xGMI; one process per GPU).  Chains shard by global id with no data-path collective; these
 * carry the acceptance totals and the R-hat / ESS sums of a sharded run (ONE all-reduce of 3(dim+1)+3 doubles per
 * reporting interval) and the half-step exchange of ONE ensemble sharded over the GPUs (ONE all-gather).  librccl is
 * resolved at run time.  mhx_comm_unique_id is called on one rank; the 128 bytes travel to the others by whatever the
 * host has (Distributed.jl, MPI, a file) and every rank calls mhx_comm_init with them. */
typedef struct mhx_comm mhx_comm;
#define MHX_COMM_ID_BYTES 128
int mhx_comm_unique_id(void *id128);
int mhx_comm_init(mhx_ctx *ctx, int rank, int world, const void *id128, mhx_comm **out);
/* ncclCommInitRank returns only when EVERY rank has called it: a missing rank, a stale id or a fabric that cannot connect the
 * ranks is a hang, not an error.  mhx_comm_init waits MHX_COMM_INIT_TIMEOUT_S for it, mhx_comm_init_timed `timeout_s` (<= 0: the
 * default); on expiry MHX_EHIP with a message that names the rank -- the caller can report it or fall back to another transport
 * (bench.py: RCCL behind this ABI, then torch.distributed's own nccl backend, then gloo).  mhx_comm_set_timeout bounds every
 * later blocking collective of the communicator the same way (default: the same 300 s). */
#define MHX_COMM_INIT_TIMEOUT_S 300.0
int mhx_comm_init_timed(mhx_ctx *ctx, int rank, int world, const void *id128, double timeout_s, mhx_comm **out);
int mhx_comm_set_timeout(mhx_comm *comm, double seconds);
int mhx_comm_destroy(mhx_comm *comm);
int mhx_comm_rank(const mhx_comm *comm, int *rank, int *world);
/* in-place sum over the ranks of n doubles in HOST memory (blocking) */
int mhx_comm_allreduce_sum(mhx_comm *comm, double *inout, size_t n);
/* this rank's slice [*begin, *begin + *count) of a half with cnt walkers */
int mhx_comm_slice(const mhx_comm *comm, int cnt, int *begin, int *count);
/* after mhx_emcee_half_step(run, half, begin, count) with the slice above: exchange the moved slices (stream-ordered) */
int mhx_comm_allgather_walkers(mhx_comm *comm, mhx_run *run, int half);

/* Rank-normalised bulk ESS and tail ESS (Vehtari et al. 2021, sections 4.1-4.3; what MCMCChains / ArviZ print as
 * ess_bulk, ess_tail) of the parameters params[0..nparams) (indices into the dim+1 rows, lp = dim) of the sample
 * buffer: the draws of one parameter are sorted on the device, replaced by the normal scores of their ranks (bulk)
 * and by the indicators of the 5 % / 95 % quantiles (tail: the smaller of the two), and the multi-chain ESS above
 * (cfg.max_lag, cfg.ess_chains, cfg.split) is taken of those series.  Negated values: as for ess[] above.
 * Equal draws share the average of their ranks.  All n_saved x nchains draws are ranked; with cfg.split and an odd n_saved the
 * series of the last draw is then not read.  Rows without an answer, as above:
 *   - a row that holds a NaN of either sign (found at the ends of the sorted draws: the sort's bit order puts a NaN with the sign
 *     set first and one with it clear last; no rank is computed): ess_bulk = ess_tail = NaN;
 *   - +inf / -inf draws have ranks like any other: both values are finite (where mhx_run_diagnostics gives NaN for the row);
 *   - a constant row, or one whose 5 % or 95 % indicator is constant within every (half-)chain read: NaN for the value built on the
 *     series without variance (ess_tail is NaN when either indicator's is). */
int mhx_run_ess_bulk_tail(mhx_run *run, const mhx_diag_cfg *cfg, const int32_t *params, int32_t nparams,
                          double *ess_bulk, double *ess_tail /* each [nparams], either may be NULL */);

/* Rank-normalised split R-hat (Vehtari et al. 2021, section 4.1; MCMCDiagnosticTools' rhat kinds :bulk, :tail and, as the larger of
 * the two, :rank) next to the bulk / tail ESS above, from the SAME one sort per parameter.  With y the ascending order of a row's
 * S = n_saved x nchains draws (all of them are ranked, as above):
 *   median        m = y[S/2] for an odd S, else y[S/2-1]/2 + y[S/2]/2 added in the run's width (Julia's `middle`)
 *   bulk scores   z  = Phi^-1((rank(x) - 3/8) / (S + 1/4)), equal draws sharing the average of their ranks: the series of ess_bulk.
 *                 Evaluated to a few ulp of double at every rank, then rounded to the run's width: sqrt2 erfinv(2 (p - 1/2)) with
 *                 p - 1/2 = (rank - (S+1)/2) / (S + 1/4) in the middle half, -+sqrt2 erfcinv(2 t) of the tail probability t outside
 *                 it (numerators exact).  mhx_run_ess_bulk_tail keeps its own evaluation (p rounded in double, then inverted: off by
 *                 up to 1e-13 absolute at the extremes, which its bounds cover), so the ESS of the two entries agree within those
 *                 bounds, not bit for bit
 *   folded scores zf = the same of the ranks of g = |x - m|, the subtraction rounded once to the run's width.  No second sort: g falls
 *                 over the draws below m and rises over the rest (rounding is monotone), so the number of draws with g < f and with
 *                 g <= f is found by binary searches in y with g evaluated on the fly, and rank = (less + leq - 1) / 2 + 1.  Draws that
 *                 the rounding collapses onto one g tie, as they do in the definition.
 *   rhat_bulk     R-hat = sqrt(var+ / W) of z, rhat_tail of zf, from the three sums of mhx_run_diagnostics over the M = nchains
 *                 (cfg.split: 2 nchains half-chains of floor(n_saved/2) draws; the scores of the last draw of an odd n_saved are not
 *                 read) chains: W = sum_v/M, Vm = max(0, (sum_m2 - sum_m^2/M)/(M-1)), var+ = (n-1)/n W + Vm
 *   ess_bulk, ess_tail   as mhx_run_ess_bulk_tail gives them (cfg.max_lag, cfg.ess_chains), run only when one of the two is asked for
 * Any of the four outputs may be NULL.  Rows without an answer:
 *   - a row that holds a NaN of either sign (found at the ends of the sort; no search is run on it): NaN in all four;
 *   - a median that is not finite (half of the draws or more infinite, or -inf and +inf as the middle pair): rhat_tail = NaN, the
 *     other three untouched by it;
 *   - +inf / -inf draws with a finite median are ranked like any other (g = +inf for them);
 *   - scores without variance within every (half-)chain (W == 0: a constant row has z == zf == 0): NaN when Vm == 0, +inf when Vm > 0;
 *   - one (half-)chain (M == 1): both R-hat values are NaN.
 * Not here: the mhx_group_* twin (ranks pooled over the members need the histograms of the select, not a sort per member) and the
 * Julia glue.  MHX_ESTATE: fewer than 4 saved draws or no sample tensor; MHX_EINVAL: a parameter outside [0, dim], 2^32 draws or
 * more per parameter.  Blocking. */
int mhx_run_rank_diagnostics(mhx_run *run, const mhx_diag_cfg *cfg, const int32_t *params, int32_t nparams,
                             double *ess_bulk, double *ess_tail, double *rhat_bulk, double *rhat_tail /* each [nparams] or NULL */);
/* The scores themselves, for the rank plots of the same paper: out_host [n_saved][nchains] in the run's width (HOST memory), z of row
 * `param` (folded = 0) or zf (folded = 1).  A row that holds a NaN fills out_host with NaN; so does a median that is not finite when
 * folded = 1. */
int mhx_run_rank_scores(mhx_run *run, int32_t param, int32_t folded, void *out_host);

/* Exact order statistics (and with them quantiles, medians, credible intervals: what MCMCChains prints as its "Quantiles" table,
 * README.md:65-71) of the parameters params[0..nparams) (indices into the dim+1 rows, lp = dim) of the sample buffer, without a
 * sort and without a copy of the draws: a histogram radix SELECT that reads the [n_saved][dim+1][nchains] tensor in place.
 *   ranks[0..nranks)   0-based positions in the ascending order of a parameter's S = n_saved * nchains draws; any order, repeats
 *                      allowed; NaNs order last (as numpy.sort); there is no 2^32 limit on S
 *   out[nparams][nranks]  the draws at those positions as double (an fp32 draw is widened exactly); -0.0 and +0.0 are equal
 *                      draws: either may be returned
 * A draw is mapped to an unsigned key of its own width whose order is the numeric order; a pass histograms one digit (11 bits;
 * option SELECT_BITS: 1..11) of the keys that match the prefix selected so far -- all parameters and all ranks in ONE sweep
 * over the tensor, per-block histograms in LDS added to uint64 counters with integer atomics, so results are reproducible bit
 * for bit -- and the host picks the bin that holds each rank.  6 passes for fp64, 3 for fp32; ranks are served in batches of 32,
 * so scratch is nparams x 32 x 2048 counters at most, whatever S.
 * MHX_EINVAL: a rank outside [0, S), a parameter outside [0, dim]; MHX_ESTATE: the run holds no device sample tensor (moments
 * mode, save_samples = 0, a host-streamed run that kept nothing).  Nothing is written to `out` unless the call succeeds. */
int mhx_run_order_statistics(mhx_run *run, const int32_t *params, int32_t nparams, const int64_t *ranks, int32_t nranks, double *out);
/* the same select on a caller's device tensor [n_samples][dim1][nchains] (chain fastest: the engine's layout, what
 * mhx_run_device_samples hands out) of the context's dtype; work queued on other streams must have completed */
int mhx_ctx_order_statistics(mhx_ctx *ctx, const void *d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,
                             const int32_t *params, int32_t nparams, const int64_t *ranks, int32_t nranks, double *out);

/* First and second cross moments of the parameters params[0..nparams) (indices into the dim+1 rows, lp = dim; a row may repeat)
 * over all K = n_saved * nchains draws of the sample buffer, on the fp64 matrix cores, reading the [n_saved][dim+1][nchains] tensor
 * in place.  With y[i][k] = x[params[i]][k] - shift[i] rounded once to double (shift NULL: 0; an fp32 draw
 * is widened exactly):
 *   sum[i]       = sum over k of y[i][k]
 *   cross[i][j]  = sum over k of y[i][k] * y[j][k]      [nparams][nparams], exactly symmetric, both halves written
 * in double whatever the context's dtype.  Covariance of the pooled draws: (cross - sum sum^T / K) / (K - 1) -- a shift near the
 * mean takes the cancellation out of that formula.  No floating-point atomics: partial tiles are added in a fixed order, so two
 * calls on the same tensor return the same bits.  A NaN or an infinity among the draws of row params[i] reaches sum[i], row i and
 * column i of cross and nothing else.  *n_draws = K.
 * MHX_EINVAL: a parameter outside [0, dim], a shift that is not finite; MHX_ESTATE: the run holds no device sample tensor.  Nothing
 * is written to sum / cross unless the call succeeds. */
int mhx_run_cross_moments(mhx_run *run, const int32_t *params, int32_t nparams, const double *shift, double *sum, double *cross,
                          int64_t *n_draws);
/* the same on a caller's device tensor [n_samples][dim1][nchains] of the context's dtype (as mhx_ctx_order_statistics) */
int mhx_ctx_cross_moments(mhx_ctx *ctx, const void *d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,
                          const int32_t *params, int32_t nparams, const double *shift, double *sum, double *cross);

/* Highest-posterior-density intervals (what MCMCChains offers as `hpd(chain; alpha = 0.05)`: the Chen-Shao interval, the shortest of
 * the intervals that span S - m + 1 consecutive order statistics) of the parameters params[0..nparams) (indices into the dim+1 rows,
 * lp = dim; any order, a row may repeat) over the S = n_saved * nchains draws of ALL chains pooled, as the quantiles are.  With y the
 * ascending order of a row's draws (NaNs last) and m = max(1, (int64)ceil(alpha * (double)S)), computed in double:
 *   a = y[0:m], b = y[S-m:S], i = the first argmin of b - a, lower = a[i], upper = b[i]      (double; an fp32 draw is widened exactly)
 * No full sort and no copy of the draws: the radix select above finds y[m-1], y[S-m] and the NaN check y[S-1]; one more sweep of the
 * tensor in place gathers the keys strictly outside the two thresholds (2 alpha of the draws; draws EQUAL to a threshold -- the
 * repeats of rejected transitions -- are counted, never stored); only those tails are sorted; a reduction finds the first minimum.
 *   width         b[i] - a[i] in fp64 of the widened values in BOTH engine widths (the reference, on a Float32 array, rounds the
 *                 width to Float32: a deviation -- two fp32 widths that differ below a Float32 ulp of their size tie there, not here)
 *   comparison    as numpy.argmin and Julia's findmin: a NaN width (inf - inf) is smaller than every number; among equal widths the
 *                 lowest i wins
 *   reproducible  integer atomics only reserve slots in buffers that are sorted before they are read, and the minimum is taken under
 *                 a total order on (width, i): the result depends on neither the launch geometry nor the order of arrival, two calls
 *                 return the same bits
 *   NaN rows      a row whose top order statistic is NaN (it holds a NaN) has lower = upper = NaN; other rows are untouched (the rule
 *                 of the quantiles)
 *   signed zeros  -0.0 and +0.0 are equal draws: either may be returned
 *   2m > S        (alpha > 0.5) the two tails overlap: legal, and the same definition
 * Scratch: 4 x (m - 1) keys per row in flight plus the sort's own space, bounded by option HPD_SCRATCH_MB; rows are served in batches
 * that fit and the context keeps the buffer from call to call.
 * MHX_EINVAL: alpha not in (0, 1) (NaN included), a parameter outside [0, dim], a single row whose tails do not fit HPD_SCRATCH_MB
 * (the message names the option); MHX_ESTATE: the run holds no device sample tensor; MHX_EHIP: more draws beyond a threshold than its
 * rank allows (the tensor changed during the call) -- never a write out of bounds.  Nothing is written to lower / upper unless the call
 * succeeds.  Blocking. */
int mhx_run_hpd(mhx_run *run, const int32_t *params, int32_t nparams, double alpha, double *lower, double *upper);
/* the same on a caller's device tensor [n_samples][dim1][nchains] of the context's dtype (as mhx_ctx_order_statistics) */
int mhx_ctx_hpd(mhx_ctx *ctx, const void *d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,
                const int32_t *params, int32_t nparams, double alpha, double *lower, double *upper);

/* Histograms of the pooled draws over caller-given bin edges (what MCMCChains offers as `histogram`, and the counts behind `density`
 * and `corner`) of the parameters params[0..nparams) (indices into the dim+1 rows, lp = dim; any order, a row may repeat), counted on
 * the device in ONE sweep of the [n_saved][dim+1][nchains] tensor in place.
 *   edges[nparams][nbins+1]  the edges of every row slot: finite, non-decreasing (repeats allowed); nbins in [1, 2048]
 *   counts[nparams][nbins]   bin j of a slot holds the draws with e[j] <= x < e[j+1]; the last bin is closed: x == e[nbins] counts in
 *                            bin nbins - 1.  j = (number of edges <= x) - 1, so of a run of equal edges the last one takes the draw
 *   outside[nparams][3]      (NULL: not wanted) draws below e[0] (-inf included), above e[nbins] (+inf included), NaN (either sign)
 * A draw is widened exactly to double and every comparison is a double comparison: the counts are those of numpy.histogram on the
 * draws cast to float64 with bins=edges.  -0.0 and +0.0 are the same draw.  Per-block counts in LDS, added to uint64 counters with
 * integer atomics: exact, two calls return the same bits, and for every slot sum(counts) + below + above + nan == n_saved * nchains
 * (no 2^32 limit).  No floating-point atomics.
 * MHX_EINVAL: a parameter outside [0, dim], nbins outside [1, 2048], an edge that is not finite, edges that decrease, more than 65535
 * slots; MHX_ESTATE: the run holds no device sample tensor.  Nothing is written unless the call succeeds.  Blocking. */
int mhx_run_histogram(mhx_run *run, const int32_t *params, int32_t nparams, const double *edges, int32_t nbins, uint64_t *counts,
                      uint64_t *outside);
/* the same on a caller's device tensor [n_samples][dim1][nchains] of the context's dtype (as mhx_ctx_order_statistics) */
int mhx_ctx_histogram(mhx_ctx *ctx, const void *d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,
                      const int32_t *params, int32_t nparams, const double *edges, int32_t nbins, uint64_t *counts, uint64_t *outside);
/* Pair histograms (the cells of a corner plot): pair q counts the draws of the rows params[pairs[2q]] and params[pairs[2q+1]] --
 * slots into params, which also pick each axis' edges -- that share a saved sample and a chain.
 *   edges[nparams][nbins+1]  as above; one nbins for both axes, in [1, 128]
 *   counts[npairs][nbins][nbins]  the first slot slowest: cell [bin of the first row][bin of the second], each by the rule above (what
 *                            numpy.histogram2d gives for the widened draws)
 *   outside[npairs]          (NULL: not wanted) draws without a bin on either axis: NaN, below or above
 * One sweep reads both rows of every pair, so m (m - 1) / 2 pairs read m (m - 1) rows.  sum(counts) + outside == n_saved * nchains for
 * every pair.  MHX_EINVAL as above with nbins outside [1, 128], and a pair slot outside [0, nparams) or more than 65535 pairs. */
int mhx_run_histogram2d(mhx_run *run, const int32_t *params, int32_t nparams, const double *edges, int32_t nbins, const int32_t *pairs,
                        int32_t npairs, uint64_t *counts, uint64_t *outside);
int mhx_ctx_histogram2d(mhx_ctx *ctx, const void *d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,
                        const int32_t *params, int32_t nparams, const double *edges, int32_t nbins, const int32_t *pairs, int32_t npairs,
                        uint64_t *counts, uint64_t *outside);

/* Autocovariance sums of the rows params[0..nparams) (indices into the dim+1 rows, lp = dim) at the lags lags[0..nlags) (strictly
 * increasing, 0 <= lag < n_saved), over the chains [chain_begin, chain_begin + chain_count) (chain_count 0: to the last chain), from the
 * [n_saved][dim+1][nchains] tensor in place.  With m_c = x_0 + sum_t (x_t - x_0) / N the chain's own mean
 * (fp64) and A_c(k) = sum_{t < N-k} (x_t - m_c)(x_{t+k} - m_c):
 *   normalise = 0   acov[i][j] = sum_c A_c(k_j): un-normalised, so the sums of shards (members of a group, ranks of a job) simply add;
 *                   nvalid[i] (NULL: not wanted) = the chains with A_c(0) > 0
 *   normalise = 1   acov[i][j] = sum_c A_c(k_j) / A_c(0) over the chains with A_c(0) > 0, nvalid[i] of them: the sum over chains of each
 *                   chain's own autocorrelation function (StatsBase.autocor per chain; emcee's walker-averaged f times nvalid).  A
 *                   chain that never moved is left out and counted out, never divided by zero; A_c(0) here is the fp64 sum of the
 *                   squares about m_c, which is exactly 0 for such a chain.
 * How the sums are accumulated (the tests' bounds are built from this): m_c is rounded once to the run's width; x - m_c, and the
 * products, are taken and accumulated in that width by fused multiply-adds, at most 512 in a row per accumulator, which is then
 * added to an fp64 partner; the draws go in time chunks of 1024, a chain's fp64 partial of a chunk is (normalise = 1: multiplied by
 * 1 / A_c(0) and) added over the 64 chains of a wave in 6 shuffle steps, and ONE fp64 atomic per (lag, 64 chains, chunk) adds it to
 * the result -- the order of those atomics is not fixed, so two calls may differ in the last bits.  The lags go in tiles of R
 * consecutive lags (a register window of the series; R per width, option ACF_R = 8 | 16 | 32 overrides it); a sparse list launches
 * only the tiles that hold a listed lag.
 * A row with a non-finite draw among the chains read is NaN at every lag, its nvalid 0; no other row changes.
 * MHX_EINVAL: acov NULL, a parameter outside [0, dim], no lags, a lag outside [0, n_saved) or not above its predecessor (the message
 * names the entry), a chain range outside [0, nchains); MHX_ESTATE: no device sample tensor, or fewer than 2 saved draws.  Nothing is
 * written unless the call succeeds.  Blocking. */
int mhx_run_autocovariance(mhx_run *run, const int32_t *params, int32_t nparams, const int32_t *lags, int32_t nlags,
                           int64_t chain_begin, int64_t chain_count, int32_t normalise, double *acov, int64_t *nvalid);
/* the same on a caller's device tensor [n_samples][dim1][nchains] of the context's dtype (as mhx_ctx_order_statistics) */
int mhx_ctx_autocovariance(mhx_ctx *ctx, const void *d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,
                           const int32_t *params, int32_t nparams, const int32_t *lags, int32_t nlags,
                           int64_t chain_begin, int64_t chain_count, int32_t normalise, double *acov, int64_t *nvalid);

/* Derived quantities: every saved draw of `src` mapped through a user function on the device -- MCMCChains'
 * one-liners on a Chains object (sigma^2, exp(beta[3]), mu[1] - mu[0], an indicator), Turing's generated_quantities.  `source` is HIP
 * source of the form
 *     MHX_DERIVED(x, y, d, data, ndata) { y.set(0, x[1] * x[1]); y.set(1, x[d]); }
 * x[0 .. d-1] is one draw of the d = dim parameters of `src`, x[d] its lp (a row is loaded only where it is named; an index outside
 * [0, d] reads x[d]); y.set(j, value), j < nout, writes output j (another j is ignored; an output that is not set is NaN); data /
 * ndata: `ndata` reals of the context's dtype, copied by the call, NULL / 0 for none.  mhx_real, MHX_R(literal), mhx_log, mhx_exp,
 * mhx_sqrt, mhx_abs, mhx_fma, MHX_INF and MHX_NAN are there as for mhx_target_from_hip_source, so one text serves both widths; the
 * arithmetic is the engine's (no contraction: a host restatement reproduces it bit for bit).  No random numbers.
 * *out is a DERIVED RUN: an mhx_run of dim = nout and the chains of `src` that holds a device sample tensor
 * [n_saved][nout + 1][nchains] -- rows 0 .. nout-1 the outputs, row nout the lp row of `src`, copied -- and nothing else: no target, no
 * sampler state, no accept flags.  It is a snapshot: sampling `src` again, or destroying it, does not change it.  It is destroyed by
 * mhx_run_destroy, lives on the context of `src` (destroy it first), and may itself be a `src`.  On a derived run
 *   work      mhx_run_device_samples (accepted = NULL), mhx_run_get_samples (accepted must be NULL: MHX_EINVAL otherwise),
 *             mhx_run_stats (no transitions; kernel_ms = the map's launch, kernel_variant = -1), mhx_run_form_name ("derived"),
 *             mhx_run_shape, mhx_run_host_stats (zeros), mhx_run_destroy, mhx_run_derive, mhx_run_predict, mhx_run_pointwise, mhx_run_psis, mhx_group_attach, and every post-run statistic:
 *             mhx_run_diagnostics, _ess_bulk_tail, _rank_diagnostics, _rank_scores, _order_statistics, _select_histogram, _cross_moments,
 *             _hpd, _histogram, _histogram2d, _autocovariance
 *   refuse    with MHX_ESTATE and a message that says the run is derived, before anything else is looked at: mhx_run_init, _sample,
 *             _sample_to_host, _get_state, _set_state, _state_size, _save_state, _load_state; mhx_ram_set_factor, _set_factor_all,
 *             _get_factor, _get_diag_range, _get_adapt_state, _get_step_stats, _watch_factors, _get_watched_factors; mhx_emcee_half_step,
 *             _end_sweep, _device_state, _exchange_plan, _exchange_pack, _exchange_unpack (and with them mhx_comm_allgather_walkers and
 *             the mhx_group_init / _sample / _sample_to_host of a group it is attached to)
 * The map is compiled at run time, once per (source, nout, dtype, draws per lane), through the context's module table and the on-disk
 * code-object cache as every run-time kernel: a second call with the same source and nout compiles nothing (mhx_ctx_jit_counts).
 * MHX_ESTATE: `src` holds no device sample tensor (moments mode, save_samples = 0, a host-streamed run); MHX_EINVAL: source or out
 * NULL, nout < 1 or > 128 (the outputs of a draw are held in registers: split the map), data NULL with ndata > 0, and a source that
 * does not compile -- the compiler's log is in mhx_last_error, as for mhx_target_from_hip_source, but the code is MHX_EINVAL: the
 * source is this call's argument (a compile that fails for another reason, no compiler or a module that does not load, is MHX_EJIT);
 * MHX_ENOMEM: the tensor cannot be allocated.  *out is written only when the call succeeds and no
 * partial object is left behind otherwise.  Blocking. */
int mhx_run_derive(const mhx_run *src, const char *source, int32_t nout, const void *data, size_t ndata, mhx_run **out);
/* the same on a caller's device tensor [n_samples][dim1][nchains] of the context's dtype (as mhx_ctx_order_statistics): d = dim1 - 1,
 * the last row is copied as lp; the derived run lives on ctx */
int mhx_ctx_derive(mhx_ctx *ctx, const void *d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,
                   const char *source, int32_t nout, const void *data, size_t ndata, mhx_run **out);

/* Posterior predictive draws: mhx_run_derive for a map that draws random numbers (DESIGN.md sections 3.16 and 6.5.6) -- Turing's
 * predict / generated_quantities with a rand in it: y_rep ~ Normal(mu, sigma) for every saved draw.  `source` is HIP source of the form
 *     MHX_PREDICTIVE(x, rng, y, d, data, ndata) { y.set(0, rng.draw(0, MHX_FAMILY_NORMAL, x[0], x[1])); }
 * x, y, d, data and ndata as for MHX_DERIVED; rng is the stream of this (chain, saved draw).  Draw k -- k = 0, 1, 2, ... a compile-time
 * constant below 2^20, each used once -- is rng.draw(k, family, p0, p1) for Normal, Uniform, Laplace, Cauchy and Exponential (p1 = 0)
 * with the parameters of Distributions.jl, or rng.gamma(k, family, alpha, theta, d, c, 1 / alpha) for Gamma and InverseGamma with a
 * constant shape and the Marsaglia-Tsang constants of csrc/mhx_device_math.h (documented there at the macro; mhx.trace.trace_predictive
 * emits them).  A parameter is any mhx_real expression: of x, of data, of an earlier draw.
 * The arithmetic: key = the Philox schedule of seed ^ MHX_PREDICT_SALT (0x5052454449435421); counter = (global chain id low word, high
 * word, index t of the saved draw, stream << 28 | block), the id first_id + chain as the samplers form it.  Draw k takes block k of
 * stream 8 (MHX_STREAM_FAMILY): a Normal draw is mu + sigma * (normal 0 of that block's Box-Muller pair) -- NOT the shared normal stream
 * of the proposals --, the other families spend the block as the proposal components do; the Gamma families take blocks k << 8 | attempt
 * of streams 9 and 10.  Parameters that are not a distribution's (a scale <= 0, a >= b, NaN, Inf) give NaN where the reference would
 * throw; a NaN propagates through what reads it.  A draw is a pure function of (seed, global chain id, t, k, parameters): the same call
 * twice gives the same bits, whatever the grid, the chain blocks or DERIVE_DRAWS (default 1 for these maps).
 * `seed` is taken as given (the host layers pass the run's own unless told otherwise; with the salt the map does not replay the words
 * the run's proposals consumed).  *out is a derived run exactly as mhx_run_derive makes it -- row nout the lp row of `src`, a snapshot,
 * the same entries work on it and the same refuse it, it may be the `src` of either call.  A derived run inherits seed and first_id
 * from its source, so a predictive map of a derived run uses the original chains' ids.  Errors as mhx_run_derive (a compiler
 * diagnostic names the text predictive.hip); also MHX_EINVAL for n_saved > 2^32 (t is one counter word).  Blocking. */
int mhx_run_predict(const mhx_run *src, const char *source, int32_t nout, const void *data, size_t ndata,
                    uint64_t seed, mhx_run **out);
/* the same on a caller's device tensor; first_chain: the global id of the tensor's chain 0 (what the derived run inherits as first_id,
 * with seed) */
int mhx_ctx_predict(mhx_ctx *ctx, const void *d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,
                    int64_t first_chain, const char *source, int32_t nout, const void *data, size_t ndata,
                    uint64_t seed, mhx_run **out);

/* Pointwise log-likelihood: l[i, s] = log p(y_i | theta_s) of every data row i under every saved draw s of `src`, reduced over the draws
 * on the device -- what Turing's pointwise_loglikelihoods gives WAIC / lppd and MCMCChains' dic; the matrix
 * itself (T x nrows) is never stored.  `source` is HIP source of the form
 *     MHX_POINTWISE(x, r, m, d, data, ndata) { const mhx_real z = (r[0] - x[0]) / x[1]; return MHX_R(-0.5) * z * z; }
 * x is the draw exactly as MHX_DERIVED sees it (x[k] a lazy load of row k clamped to [0, d], x[d] the lp); r[j] is entry j < m = rowlen
 * of the current data row (j clamped to [0, m)); data / ndata as for mhx_run_derive, and so are mhx_log, mhx_exp and the other
 * operations of the engine; the function returns an mhx_real.
 * Definitions.
 *   T = n_saved x nchains     the pooled saved draws of the source (a run, a derived run, or a caller's tensor); written to *T
 *   rows                      nrows >= 1 data rows of rowlen >= 1 reals of the context's dtype, on the host, copied by the call
 *   l[i, s]                   the function of draw s and row i, evaluated in the run's width with the engine's operations, then
 *                             widened to fp64.  Every accumulator below is fp64 in both widths; exp is the engine's fp64 exp.
 * out5 receives five fp64 arrays of nrows, one after the other:
 *   max[i]      max_s l[i, s]: one of the l values, bit for bit (no rounding); -inf if every l is -inf
 *   sumexp[i]   sum_s exp(l[i, s] - max[i]), so that log sum_s exp l = max + log(sumexp)
 *   s1[i]       sum_s (l[i, s] - shift[i])       over the draws whose l is finite
 *   s2[i]       sum_s (l[i, s] - shift[i])^2     over the same draws
 *   bad[i]      as a double: the number of draws whose l is NaN, +inf or -inf
 * A -inf l adds 0 to sumexp, is counted in bad and left out of s1 and s2 (it never meets a -inf running maximum in a subtraction).  A
 * NaN or +inf l is counted in bad, left out of s1 and s2, and makes max[i] and sumexp[i] NaN.  No other row is affected.
 * shift is in/out, double[nrows]: with shift_given != 0 the caller supplies it; otherwise the engine sets shift[i] = l[i, draw 0 of
 * chain 0] (0 where that is not finite) and returns it.  The sums are raw on purpose, so that members of a group add: s1, s2 and bad
 * add under a common shift; (max, sumexp) merge as max = max(a, b), sumexp = sumexp_big + sumexp_small exp(max_small - max_big), and
 * on equal maxima the sums add.
 * The order of every operation is a function of the shape (n_saved, nchains, nrows) and option POINTWISE_ROWS alone -- no atomics;
 * per-block partials go to scratch and are merged in index order -- so two calls on the same tensor give the same bits.
 * Compiled at run time through the context's module table, keyed by source and defines: a second call with the same source compiles
 * nothing.  MHX_ESTATE: `src` holds no device sample tensor; MHX_EINVAL: a NULL argument, nrows < 1, rowlen < 1, nrows x rowlen,
 * n_saved or nchains >= 2^31, more than 65535 tiles of rows, and a source that does not compile (the compiler's diagnostic, which
 * names the text pointwise.hip, is in mhx_last_error).  Rows and data are not checked for finiteness, as for mhx_run_derive.  A
 * refusal writes nothing to shift, out5 or T.  Works on a derived run.  Blocking. */
int mhx_run_pointwise(const mhx_run *src, const char *source, const void *rows, int64_t nrows, int32_t rowlen,
                      const void *data, size_t ndata, int32_t shift_given, double *shift, double *out5, int64_t *T);
/* the same on a caller's device tensor [n_samples][dim1][nchains] of the context's dtype (as mhx_ctx_derive): d = dim1 - 1 */
int mhx_ctx_pointwise(mhx_ctx *ctx, const void *d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains,
                      const char *source, const void *rows, int64_t nrows, int32_t rowlen, const void *data,
                      size_t ndata, int32_t shift_given, double *shift, double *out5, int64_t *T);

/* PSIS-LOO: Pareto-smoothed importance-sampling leave-one-out of every data row from the saved draws (Vehtari, Gelman, Gabry 2017;
 * R loo's psis / gpdfit), on the device, with l[i, s] never stored.  `source`, rows, data and l[i, s] exactly as
 * for mhx_run_pointwise: l is evaluated in the run's width and widened; everything after the widening is fp64 in both widths, with the
 * engine's fp64 exp and log (log1p and expm1 are Kahan's forms on them).
 * Definitions, per data row i, with T = n_saved x nchains (as a double where it enters arithmetic) and l_(0) <= ... <= l_(T-1) the draws
 * ascending (ordered as the exact order statistics order them: -0 before +0):
 *   M         the tail length min(floor(0.2 T), ceil(3 sqrt(T / reff))), computed in double on the host; M < 5 counts as M = 0
 *   tau       the cutoff l_(M); it belongs to the body.  n_below = #{l < tau} <= M, n_eq = #{l == tau}
 *   tail      a_0 <= ... <= a_(M-1): the n_below draws below tau, then M - n_below copies of tau.  lmin = a_0 (tau where M = 0)
 *   c         exp(lmin - tau);  x_j = exp(lmin - a_(M-1-j)) - c, j < M: the tail's importance ratios relative to the largest, ascending
 *   fit       (M >= 5, and a_(M-1) - a_0 >= 2^-52 / 100)  m = 30 + floor(sqrt(M)) grid points
 *               theta_j = 1 / x_(M-1) + (1 - sqrt(m / (j - 1/2))) / (3 x*),  j = 1 .. m,  x* = x at index floor(M / 4 + 1/2) - 1
 *               k_j = mean_i log1p(-theta_j x_i);  L_j = M (log(-theta_j / k_j) - k_j - 1);  w_j = 1 / sum_j' exp(L_j' - L_j)
 *               theta^ = sum_j w_j theta_j;  k = mean_i log1p(-theta^ x_i);  sigma = -k / theta^;  khat = (k M + 5) / (M + 10)
 *             where there is no fit, or theta^ or khat is not finite, or sigma is not a positive finite number (ties: x* = 0):
 *             khat = +inf, sigma = NaN and the tail keeps its raw weights
 *   lw~_j     fitted: min(0, log(sigma expm1(-khat log1p(-p_j)) / khat + c)), p_j = (j + 1/2) / M (the khat -> 0 limit
 *             -sigma log1p(-p_j) + c where khat == 0);  raw: lmin - a_(M-1-j)
 *   B         sum_{l_s > tau} exp(tau - l_s) + (n_eq - (M - n_below)): the body's ratios relative to the cutoff's, every term <= 1
 *   elpd_loo  lmin + log((T - M) + sum_j exp(lw~_j + (a_(M-1-j) - lmin))) - log(c B + sum_j exp(lw~_j))
 * out8 receives eight fp64 arrays of nrows, one after the other: elpd_loo, khat, sigma, tau, lmin, B, n_below, bad.  tail_out (may be
 * NULL) receives [nrows][M] doubles, the tails a ascending.  *T and *M (each may be NULL) receive T and M.  tau, lmin, n_below, bad and
 * the tails are exact (draws, bit for bit, and counts).
 * A row with any NaN, +inf or -inf l among its draws has bad[i] = their number and NaN in its seven other entries and in its tail; no
 * other row is affected.
 * The order of every operation is a function of (n_saved, nchains) and reff alone: histograms are integer sums, the floating
 * sums run lane-strided with a butterfly, over the waves in wave order and over the blocks' partials in index order; the tails are
 * sorted before anything reads them.  Two calls give the same bits, whatever SELECT_BITS, PSIS_SCRATCH_MB and PSIS_ROWS are.
 * Cost: (key passes of the select + 1) sweeps that each evaluate l for every (draw, row), a sort of nrows x M keys, nrows x m x M log1p.
 * Rows go in batches whose scratch fits option PSIS_SCRATCH_MB (default 1024).  MHX_ESTATE and MHX_EINVAL as mhx_run_pointwise (out8
 * in place of shift and out5); also MHX_EINVAL for reff not a positive finite number, M > 2^20, and one row whose scratch does not fit
 * PSIS_SCRATCH_MB (refused before any sweep).  A refusal writes nothing to out8, tail_out, T or M.  Works on a derived run.  Blocking. */
int mhx_run_psis(const mhx_run *src, const char *source, const void *rows, int64_t nrows, int32_t rowlen, const void *data,
                 size_t ndata, double reff, double *out8, double *tail_out, int64_t *T, int64_t *M);
/* the same on a caller's device tensor [n_samples][dim1][nchains] of the context's dtype (as mhx_ctx_pointwise) */
int mhx_ctx_psis(mhx_ctx *ctx, const void *d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, const char *source,
                 const void *rows, int64_t nrows, int32_t rowlen, const void *data, size_t ndata, double reff, double *out8,
                 double *tail_out, int64_t *T, int64_t *M);

/* ---------------------------------------------------------------------------------------------
 * Parallel tempering (replica exchange) of random-walk Metropolis-Hastings.  A run of `nchains` device chains is
 * nchains / R ladders of R rungs: chain c is rung r = c mod R of ladder c div R and samples target^beta[r] with the proposal scaled by
 * scale[r]; after every swap_every-th transition neighbouring rungs of a ladder may exchange their states (deterministic even-odd
 * pairs, one uniform per pair).  The chain to read is rung 0 (beta = 1): mhx_run_rung.  A slot keeps its temperature; the accept
 * counters of a slot are those of its temperature.  The run records EVERY rung (R times the cold rung's memory and store traffic).
 *     R           a power of two in 2..64; cfg.nchains and cfg.first_chain are multiples of it
 *     swap_every  >= 0; 0 = no swap rounds
 *     beta        [R] doubles, beta[0] == 1, strictly decreasing, all > 0 (swap_every == 0: non-increasing is enough, so that a
 *                 ladder of equal temperatures can be timed against the plain run); rounded once to the run's width
 *     scale       [R] doubles or NULL = beta^(-1/2) (computed in double); scale[0] == 1, all > 0; the proposal of rung r is
 *                 ISO scale[r] * sigma, DIAG scale[r] * sigma_k: one product in double, rounded once
 * cfg: proposal kinds ISO and DIAG with zero mean; any target.  MHX_EINVAL with a message that names the rule for: a bad R, nchains
 * or first_chain not a multiple of R, a bad ladder or scale, swap_every < 0, MHX_FLAG_ZIGGURAT, MHX_FLAG_STATIC_PROPOSAL, a proposal
 * mean, MHX_PROP_DENSE, reduce_lanes > 1, MHX_FLAG_NO_JIT with a user target.  Initial states as mhx_rwmh_create's.
 * A tempered run refuses, with MHX_ESTATE: MHX_SAVE_MOMENTS, mhx_run_sample_to_host (the accept-compacted return path assumes that a
 * rejected transition repeats the row above; a swap breaks that), mhx_run_state_size / _save_state / _load_state, mhx_group_attach. */
typedef struct {
    int32_t R;
    int32_t swap_every;
    const void *beta;  /* [R] doubles (whatever the run's width) */
    const void *scale; /* [R] doubles or NULL */
} mhx_tempered_cfg;
int mhx_rwmh_create_tempered(mhx_ctx *ctx, const mhx_target *t, const mhx_rwmh_cfg *cfg, const mhx_tempered_cfg *tcfg, mhx_run **out);
/* attempts[R - 1], swaps[R - 1]: swap rounds pair (r, r + 1) took part in since mhx_run_init and how many of them swapped, summed
 * over the ladders (the per-slot counters are kept without atomics: the counts are deterministic).  MHX_ESTATE: not a tempered run. */
int mhx_run_swap_stats(mhx_run *run, uint64_t *attempts, uint64_t *swaps);
/* Rung r of every ladder as a snapshot run in the sense of mhx_run_derive: a device tensor [n_samples][dim + 1][nchains / R] gathered
 * from columns r, r + R, r + 2R, ... of the sample tensor; it inherits seed and first_chain as a derived run does and every post-run
 * statistic reads it like any run.  MHX_EINVAL: r out of range; MHX_ESTATE: not a tempered run, or no sample tensor.  Blocking. */
int mhx_run_rung(mhx_run *run, int32_t r, mhx_run **out);
/* An adaptive ladder: every ladder tunes its own temperatures from its own swap rounds while the run warms
 * up, inside the step kernel -- no second kernel, no trip to the host; there is no shared ladder and no reduction over ladders, so a
 * shard is still the matching columns of the larger run and two calls are one.  The ladder is parametrised by rho[r], the log of the
 * gap of pair (r, r + 1) in log beta: beta[r] = exp(-sum_{q < r} exp(rho[q])), the proposal scale of rung r is beta[r]^(-1/2), and
 * after swap round s with s * swap_every <= adapt_steps every attempted pair moves
 *     rho[r] += c * s^(-kappa) * (min(1, swap ratio) - target_rate),   clamped to [rho_min, rho_max]
 * (the "Geometric" schedule of Miasojedow, Moulines and Vihola as MCMCTempering.jl implements it).  After adapt_steps transitions the
 * ladder is frozen.  tcfg.beta is the ladder the run starts from (rho0 = log log (beta[r] / beta[r + 1]), clamped).  Draws taken while
 * the ladder moves are not draws of the target: discard at least adapt_steps transitions.
 *     adapt_steps  >= 0 transitions; 0: the ladder of rho0 for the whole run
 *     a double field that is NaN takes its default: target_rate 0.234, c 1, kappa 0.6, rho_min -10, rho_max log(16 / (R - 1)).  (0 is
 *     a value like any other -- c = 0 is the ladder that never moves -- so NaN is the one encoding of "default" for all five.)
 * MHX_EINVAL with a message that names the rule for everything mhx_rwmh_create_tempered refuses, and for: swap_every == 0, tcfg.scale
 * given (the scales follow the ladder), adapt_steps < 0, kappa outside (0.5, 1], c < 0, target_rate outside (0, 1), rho_min > rho_max,
 * (R - 1) exp(rho_max) > 80 (the coldest beta would leave fp32's normal range).  The run is kernel variant 17; mhx_run_swap_stats and
 * mhx_run_rung work on it; it refuses what a fixed ladder refuses (MHX_SAVE_MOMENTS, mhx_run_sample_to_host, checkpoints, mhx_group_attach). */
typedef struct {
    int32_t adapt_steps;
    double target_rate, c, kappa, rho_min, rho_max;
} mhx_ladder_adapt_cfg;
int mhx_rwmh_create_tempered_adaptive(mhx_ctx *ctx, const mhx_target *t, const mhx_rwmh_cfg *cfg, const mhx_tempered_cfg *tcfg,
                                      const mhx_ladder_adapt_cfg *acfg, mhx_run **out);
/* beta[nchains]: slot c's current inverse temperature, widened exactly from the run's width (slot c is rung c mod R of ladder c div R).
 * An adaptive run: as of the end of the last mhx_run_sample (after create or mhx_run_init: the ladder of rho0); a fixed ladder: its
 * table.  MHX_ESTATE: not a tempered run.  Blocking. */
int mhx_run_ladder_betas(mhx_run *run, double *beta);
/* An anchored ladder: rung r samples target^beta[r] * q^(1 - beta[r]) where q is a normalised reference
 * density, a diagonal Gaussian N(mean[k], sd[k]^2) given as doubles (every sd > 0).  This is the power posterior when q is the prior
 * and the generalised stepping stone otherwise.  beta[0] == 1 and the ladder is strictly decreasing as before, but the LAST beta may
 * be exactly 0 (only the last): that rung samples q, and the path from beta = 1 to beta = 0 integrates to the log evidence,
 *     log Z = integral_0^1 E_beta[log target - log q] d beta            (mhx_run_evidence below).
 * With a beta of 0 tcfg.scale must be given: the default beta^(-1/2) has no value there.  Fixed ladders only.
 *     transition   log a = beta (lp(y) - lp(x)) + (1 - beta) (lq(y) - lq(x)); with beta = 1 this has the bits of the plain chain's
 *     swap round   log s = dbeta ((lp - lq)[r + 1] - (lp - lq)[r]); a swap exchanges x, lp and lq
 *     recorded     row dim of the sample tensor stays the UNTEMPERED log target(x)
 * SUPPORT: at beta = 0 a candidate outside the target's support has lp = -inf, 0 * (-inf) = NaN, and is rejected: the hot rung samples
 * q RESTRICTED to the support of the target, and the evidence is then relative to q's mass on that support -- choose q inside it, or
 * account for the missing mass.  (A chain that STARTS outside the support stays where it is on a beta = 0 rung until a swap moves it.)
 * MHX_EINVAL with a message that names the rule for everything mhx_rwmh_create_tempered refuses, and for: a NULL or non-finite mean or
 * sd, an sd <= 0, a zero beta that is not the last, a zero beta without tcfg.scale.  The run is kernel variant 18 (its register form is
 * built for dim <= 44 in fp64, 76 in fp32); mhx_run_swap_stats, mhx_run_rung and mhx_run_ladder_betas work on it; it refuses what a
 * fixed ladder refuses. */
typedef struct {
    const void *mean;          /* [dim] doubles */
    const void *sd;            /* [dim] doubles, each > 0 */
} mhx_tempered_reference;
int mhx_rwmh_create_tempered_anchored(mhx_ctx *ctx, const mhx_target *t, const mhx_rwmh_cfg *cfg, const mhx_tempered_cfg *tcfg,
                                      const mhx_tempered_reference *ref, mhx_run **out);
/* What the log evidence of an anchored run is made of: out[nchains][8], per chain c (rung c mod R of ladder c div R, whose temperature
 * never changes) over that chain's saved draws, u = lp - lq(x) formed in the run's width as the step kernel forms it, then fp64:
 *     [0] bad        draws whose u is NaN or +-inf: counted and left out of every sum
 *     [1] shift      the chain's first saved u, 0 where that is not finite
 *     [2] s1         sum (u - shift)               [3] s2  sum (u - shift)^2
 *     [4] max_f, [5] sumexp_f   max and sum exp(. - max) of dbeta[r - 1] u, rungs r >= 1: the stepping-stone weight towards the colder rung
 *     [6] max_b, [7] sumexp_b   ... of -dbeta[r] u, rungs r <= R - 2: the backward weight          (an unused pair: -inf, 0)
 * *n_saved (may be NULL): the draws per chain.  From these: thermodynamic integration is the trapezoid of the rung means of u over
 * beta; the stepping-stone estimate is sum_r log mean exp(dbeta[r] u) over rung r + 1.  One sweep of the tensor, no atomics: two calls
 * give the same bits.  MHX_ESTATE: not an anchored run, no sample tensor, or the ladder's last beta is not 0.  Blocking. */
int mhx_run_evidence(mhx_run *run, double *out, int64_t *n_saved);

/* ---------------------------------------------------------------------------------------------
 * Adaptive random-walk Metropolis (Andrieu & Thoms 2008, Algorithm 4 with a diagonal covariance): during the
 * first adapt_steps transitions every chain tunes its OWN proposal inside the step kernel -- a log-scale lam driven towards the
 * acceptance rate target_rate,
 *     lam += min(1, c t^(-kappa)) * (min(1, accept ratio) - target_rate),   clamped to [lam_min, lam_max]
 * and, with shape != 0, a running mean and variance per coordinate whose square root replaces the configured standard deviation; the
 * proposal's standard deviations are sd[k] = sig[k] * exp(lam).  Afterwards nothing adapts: sd is a constant of the chain and the run
 * is a plain random walk with a diagonal proposal, at the plain lane-per-chain kernels' rate.  Everything is per chain -- no reduction
 * over chains -- and indexed by the global step, so a shard is still the matching columns of the larger run and two calls are one.
 * Draws taken while the proposal moves are not draws of the target: discard at least adapt_steps transitions.
 *     cfg          an ISO or a DIAG proposal with zero mean: where every chain starts from (lam = 0)
 *     adapt_steps  >= 0 transitions; 0: the plain run
 *     shape        0: the scale alone, else the per-coordinate standard deviations too
 *     a double field that is NaN takes its default: target_rate 0.234, c 1, kappa 0.6, lam_min -20, lam_max 20 (0 is a value)
 * MHX_EINVAL with a message that names the rule: a DENSE proposal, a proposal mean, MHX_FLAG_STATIC_PROPOSAL, MHX_FLAG_ZIGGURAT,
 * reduce_lanes > 1, MHX_FLAG_NO_JIT with a user target, adapt_steps < 0, kappa outside (0.5, 1], c < 0, target_rate outside (0, 1),
 * lam_min > lam_max, and (shape) a configured s[k] whose s[k]^2 2^-40 is not normal or whose s[k]^2 2^40 is not finite in the run's
 * width (the clamps of the adapted variance).  The run is kernel variant 19; mhx_run_init / mhx_run_sample drive it; it refuses with
 * MHX_ESTATE what the tempered runs refuse (MHX_SAVE_MOMENTS, mhx_run_sample_to_host, checkpoints, mhx_group_attach). */
typedef struct {
    int32_t adapt_steps;
    int32_t shape;
    double target_rate, c, kappa, lam_min, lam_max;
} mhx_proposal_adapt_cfg;
int mhx_rwmh_create_adaptive(mhx_ctx *ctx, const mhx_target *t, const mhx_rwmh_cfg *cfg,
                             const mhx_proposal_adapt_cfg *acfg, mhx_run **out);
/* The proposal of every chain as of the end of the last mhx_run_sample (after mhx_run_init: the configured one), widened exactly from
 * the run's width: lam[nchains], sd[dim][nchains] (the standard deviations the proposal uses), mean[dim][nchains] (may be NULL; NaN
 * without shape), acc_at_freeze[nchains] (may be NULL): the accept counters as they stood after transition adapt_steps, 0 while the
 * run still adapts.  MHX_ESTATE: not an adaptive run.  Blocking. */
int mhx_run_proposal_state(mhx_run *run, double *lam, double *sd, double *mean, uint32_t *acc_at_freeze);

/* ---------------------------------------------------------------------------------------------
 * Many chains over many GPUs as ONE call from ONE process. Replaces `sample(model, sampler, MCMCThreads(), N, nchains)`
 * (README.md:135-148: one task per chain) -- here one host thread per GPU behind the ABI.  A group is N member contexts (one
 * per entry of `devices`; entries may repeat -- several members on one device are legal, which is how the form is verified on a
 * one-GPU box), N persistent worker threads and the host-side sum of the statistics that ranks of a multi-process run all-reduce
 * over RCCL (mhx_comm_allreduce_sum).  Chains shard by global id with no data-path collective, so member i's run is created by
 * the caller on mhx_group_ctx(g, i) like any run, with cfg.first_chain / cfg.nchains from mhx_group_shard (ensembles: one per
 * member, distinct ensemble_id), and attached; the group then drives all members CONCURRENTLY:
 *     mhx_group_init / _sample / _sample_to_host   == mhx_run_init / _sample / _sample_to_host of every member, side by side
 *     mhx_group_stats        transitions / accepted summed, kernel_ms = the slowest member, wall_ms = the whole call
 *     mhx_group_diagnostics  the sums of mhx_run_diagnostics added in member order (+ the chain count): R-hat over ALL chains
 * The union of the members' chains is bit for bit the unsharded run (tests/test_gpu_group.py).  A failing member's message is
 * returned with its index and device.  Ownership: the group owns contexts and threads; the caller destroys runs and targets
 * BEFORE mhx_group_destroy.  One group call at a time (a group is a handle: not thread-safe). */
typedef struct mhx_group mhx_group;
int mhx_group_create(const int32_t *devices, int32_t n, int dtype /* mhx_dtype */, mhx_group **out);
int mhx_group_destroy(mhx_group *g);
int mhx_group_size(const mhx_group *g, int32_t *n);
int mhx_group_ctx(mhx_group *g, int32_t i, mhx_ctx **ctx);      /* borrowed: valid until mhx_group_destroy */
/* member i's contiguous block of `nchains_total` global chain ids (sizes differ by at most one); also tells member i's context that
 * its runs are shards of a run of nchains_total chains (option TOTAL_CHAINS: the kernel form is picked for the whole run) */
int mhx_group_shard(const mhx_group *g, int64_t nchains_total, int32_t i, uint64_t *first_chain, int32_t *nchains);
int mhx_group_attach(mhx_group *g, mhx_run *const *runs /* [n]: runs[i] was created on mhx_group_ctx(g, i); equal dim */);
int mhx_group_run(mhx_group *g, int32_t i, mhx_run **run);
int mhx_group_init(mhx_group *g, const void *const *initial_params /* NULL, or [n] host pointers, each NULL or [dim][nchains_i] */);
int mhx_group_sample(mhx_group *g, const mhx_schedule *sched, int save_samples);
int mhx_group_sample_to_host(mhx_group *g, const mhx_schedule *sched, void *const *samples /* [n] host tensors [n_samples][dim+1][nchains_i] */,
                             uint8_t *const *accepted /* NULL, or [n] (entries may be NULL) */, int32_t slab_samples);
int mhx_group_stats(mhx_group *g, mhx_stats *out);
/* ess (optional): the members' ESS added (each from the autocovariances of its own shard); negated when any member's was.
 * *n_chains = the chains behind the sums (2x with cfg.split). */
int mhx_group_diagnostics(mhx_group *g, const mhx_diag_cfg *cfg, double *sum_m, double *sum_m2, double *sum_v, double *ess /* each [dim+1] or NULL */,
                          int64_t *n_chains);
/* bulk / tail ESS of every member (ranks pooled within a member's shard) added over the members */
int mhx_group_ess_bulk_tail(mhx_group *g, const mhx_diag_cfg *cfg, const int32_t *params, int32_t nparams, double *ess_bulk, double *ess_tail);
/* mhx_run_order_statistics over the UNION of all members' draws: ranks index S = n_saved x (the sum of the members' chains).  Per
 * pass every member histograms its own shard concurrently (mhx_run_select_histogram), the group adds the integer histograms on the
 * host and scans once: exact, and equal to the unsharded run's answer */
int mhx_group_order_statistics(mhx_group *g, const int32_t *params, int32_t nparams, const int64_t *ranks, int32_t nranks, double *out);
/* mhx_run_cross_moments over the UNION of all members' draws: every member takes the moments of its shard about the same shift
 * (concurrently), and sums about a common shift add -- here on the host, in member order.  *n_draws = the draws of all members. */
int mhx_group_cross_moments(mhx_group *g, const int32_t *params, int32_t nparams, const double *shift, double *sum, double *cross,
                            int64_t *n_draws);
/* mhx_run_histogram / mhx_run_histogram2d over the UNION of all members' draws and the same edges: the members count their shards
 * concurrently and the group adds the integers on the host -- exact, and equal to the unsharded run's arrays */
int mhx_group_histogram(mhx_group *g, const int32_t *params, int32_t nparams, const double *edges, int32_t nbins, uint64_t *counts,
                        uint64_t *outside);
int mhx_group_histogram2d(mhx_group *g, const int32_t *params, int32_t nparams, const double *edges, int32_t nbins, const int32_t *pairs,
                          int32_t npairs, uint64_t *counts, uint64_t *outside);
/* mhx_run_autocovariance over all chains of all members: the sums are sums over chains, so the members take their shards
 * concurrently and the group adds acov and nvalid on the host, in member order (a row NaN in one member: NaN, nvalid 0) */
int mhx_group_autocovariance(mhx_group *g, const int32_t *params, int32_t nparams, const int32_t *lags, int32_t nlags,
                             int32_t normalise, double *acov, int64_t *nvalid);

#ifdef __cplusplus
}
#endif
#endif /* MHX_H */
