// mhx_rwmh_family_kernels.h -- Metropolis-Hastings with a proposal made of independent univariate components, one lane per chain.
//
// Replaces the reference's step (src/mh-core.jl:92-117) for the proposal forms of src/proposal.jl:23-35,41-83 whose distribution is a
// vector of univariate Distributions: component k is Normal, Uniform, Laplace, Cauchy, Exponential, Gamma or InverseGamma (the draws
// and log-kernels: mhx_device_math.h).
//   RandomWalkProposal   y = x + xi, log ratio q(x - y) - q(y - x) from the two states (src/proposal.jl:58-64), left out when the
//                        proposal was declared symmetric (:195);
//   StaticProposal       y = xi, log ratio q(x) - q(y), q(x) one more real of chain state (:66-83);
// q = the sum over the components, in index order, of the log-kernels.
//
// Two kernels share the arithmetic, as mhx_rwmh_reg_body / mhx_rwmh_generic_body do:
//   mhx_fam_reg_body<D, ...>   run-time specialised; x[D] and y[D] in VGPRs for a whole launch, records through SRD stores.  The family
//                              of EVERY component is a compile-time constant (MHX_JIT_FAM_LIST): the per-component dispatch folds away
//                              and only the Philox blocks some component reads are generated.  The parameters stay a run-time table,
//                              so one compilation serves every parameter set of a pattern of families.
//   mhx_fam_generic_body       pre-built; run-time dimension, state in HBM as [dim][nchains], family and parameters read from the
//                              table (a wave-uniform branch per component).
// Both produce the same chain bit for bit: same counters, same operations in the same order.
#pragma once
#include "mhx_rwmh_kernels.h"

MHX_NS_BEGIN

// Largest dimension the register form is built for: x[D], y[D] and the temporaries of the unrolled component loop must fit 512
// VGPRs without scratch memory.  Measured by cross-compiling for gfx950 with the options of the run-time build, every family alone
// and mixed, walk and static (worst: Cauchy, whose division and two polynomials are live per component): fp64 clean at 32, scratch
// at 40; fp32 clean at 48 and 56, scratch at 64.  tests/test_families_cpu.py compiles the kernel at the limit and checks it.  Above
// it the state-in-HBM form runs.
#define MHX_FAM_REG_MAX_DIM (MHX_REAL64 ? 32 : 48)

// the candidate of one transition (sbase = MHX_STREAM_FAMILY) or the initial draw (MHX_STREAM_FAMILY_INIT): xi[k] for k < d through
// `put(k, xi)`.  `famof(k)` is the family of component k -- a table read here, a constant in the specialised kernel.
// UNROLL: the dimension is a compile-time constant and the component loop is unrolled whatever its size (candidate in registers).
// `fam[k].p` is the parameter row of component k: the table itself here, a lane's own rows in mhx_rwmh_cond_kernels.h.
template <bool UNROLL, class FamOf, class Tab, class Put>
MHX_DEV void mhx_fam_draw_all(const int d, const FamOf& famof, const Tab& fam, const mhx_philox_key& ks,
                              const mhx_u32 id_lo, const mhx_u32 id_hi, const mhx_u32 step, const mhx_u32 nstream, const mhx_u32 sbase,
                              const Put& put)
{
    const auto block = [&](const int b) {
        bool any_normal = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) any_normal = any_normal || (4 * b + j < d && famof(4 * b + j) == MHX_FAMILY_NORMAL);
        mhx_real n[4] = {MHX_R(0.0), MHX_R(0.0), MHX_R(0.0), MHX_R(0.0)};
        if (any_normal) mhx_normal4(ks, id_lo, id_hi, step, nstream, (mhx_u32)b, n);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 4 * b + j;
            if (k < d) put(k, mhx_fam_draw(famof(k), fam[k].p, n[j], ks, id_lo, id_hi, step, sbase, (mhx_u32)k));
        }
    };
    if constexpr (UNROLL) {
#pragma unroll
        for (int b = 0; b < (d + 3) / 4; ++b) block(b);
    } else {
        for (int b = 0; b < (d + 3) / 4; ++b) block(b);
    }
}

// ---------------------------------------------------------------------------------------------
// state in HBM, run-time dimension
template <int TK>
MHX_DEV void mhx_fam_generic_body(const mhx_rwmh_args& a, const mhx_real* __restrict__ tparams, const mhx_fam_comp* __restrict__ fam,
                                  const int symmetric)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchains) return;
    const mhx_u64 id = a.first_chain + (mhx_u64)c;
    const mhx_u32 id_lo = (mhx_u32)id, id_hi = (mhx_u32)(id >> 32);
    const mhx_philox_key ks = mhx_philox_schedule(a.seed);
    const long ld = a.ld;
    const int d = a.dim;
    mhx_real* xs = a.x + c;
    mhx_real* ys = a.ybuf + c;

    mhx_real lp = a.lp[c];
    mhx_u32 nacc = a.acc_count[c];
    mhx_u32 wave_acc = 0;
    bool last = a.last_acc[c] != 0;
    mhx_accept_cache ac;
    ac.group = 0xffffffffu;
    ac.w.x = ac.w.y = ac.w.z = ac.w.w = 0u;
    mhx_u32 save_next = a.save_next;
    long slot = a.save_slot;
    const bool stat = a.qx != nullptr;
    mhx_real qxc = stat ? a.qx[c] : MHX_R(0.0);
    const auto famof = [&](const int k) -> int { return fam[k].family; };

    for (int i = 0; i < a.nsteps; ++i) {
        const mhx_u32 step = a.step0 + (mhx_u32)i;
        mhx_fam_draw_all<false>(d, famof, fam, ks, id_lo, id_hi, step, MHX_STREAM_PROPOSAL, MHX_STREAM_FAMILY,
                         [&](const int k, const mhx_real xi) { ys[(long)k * ld] = stat ? xi : xs[(long)k * ld] + xi; });
        mhx_real ratio = MHX_R(0.0), qy = MHX_R(0.0);
        if (stat) {
            for (int k = 0; k < d; ++k) qy = qy + mhx_fam_logk(famof(k), fam[k].p, ys[(long)k * ld]);
            ratio = qxc - qy;
        } else if (!symmetric) {
            mhx_real qb = MHX_R(0.0), qf = MHX_R(0.0);
            for (int k = 0; k < d; ++k) {
                const mhx_real xk = xs[(long)k * ld], yk = ys[(long)k * ld];
                qb = qb + mhx_fam_logk(famof(k), fam[k].p, xk - yk);
                qf = qf + mhx_fam_logk(famof(k), fam[k].p, yk - xk);
            }
            ratio = qb - qf;
        }
        mhx_strided_x yv;
        yv.base = ys;
        yv.ld = ld;
        const mhx_real lpy = mhx_target_eval<TK>(a.target_kind, yv, d, tparams, a.ntparams, a.tconst);
        const mhx_real logu = mhx_accept_logu(ks, id_lo, id_hi, step, ac);
        const mhx_real loga = (stat || !symmetric) ? (lpy - lp) + ratio : (lpy - lp);
        const bool acc = logu < loga;                    // strict; NaN compares false => reject
        lp = acc ? lpy : lp;
        qxc = (stat && acc) ? qy : qxc;
        nacc += acc ? 1u : 0u;
        last = acc;
        wave_acc += (mhx_u32)__popcll(__ballot(acc));
        if (step == save_next) {
            mhx_real* row = a.samples + slot * (long)(d + 1) * ld + c;
            for (int k = 0; k < d; ++k) {
                const mhx_real v = acc ? ys[(long)k * ld] : xs[(long)k * ld];
                if (acc) xs[(long)k * ld] = v;
                row[(long)k * ld] = v;
            }
            row[(long)d * ld] = lp;
            a.accepted[slot * ld + c] = acc ? 1 : 0;
            save_next += (mhx_u32)a.thinning;
            ++slot;
        } else if (acc) {
            for (int k = 0; k < d; ++k) xs[(long)k * ld] = ys[(long)k * ld];
        }
    }
    a.lp[c] = lp;
    if (stat) a.qx[c] = qxc;
    a.acc_count[c] = nacc;
    a.last_acc[c] = last ? 1 : 0;
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
        atomicAdd(a.acc_total, (mhx_u64)wave_acc);
}

// initial_params === nothing: the first state is a bare draw from the proposal (src/mh-core.jl:83, src/proposal.jl:41-47), x = 0 + xi
MHX_DEV void mhx_fam_init_draw_body(const mhx_rwmh_args& a, const mhx_fam_comp* __restrict__ fam)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchains) return;
    const mhx_u64 id = a.first_chain + (mhx_u64)c;
    const mhx_philox_key ks = mhx_philox_schedule(a.seed);
    const long ld = a.ld;
    mhx_real* xs = a.x + c;
    mhx_fam_draw_all<false>(a.dim, [&](const int k) -> int { return fam[k].family; }, fam, ks, (mhx_u32)id, (mhx_u32)(id >> 32), 0u,
                     MHX_STREAM_INIT, MHX_STREAM_FAMILY_INIT, [&](const int k, const mhx_real xi) { xs[(long)k * ld] = MHX_R(0.0) + xi; });
}

// q(x) of every chain's current state, for a static proposal (after init / set_state)
MHX_DEV void mhx_fam_q_body(const mhx_rwmh_args& a, const mhx_fam_comp* __restrict__ fam)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchains) return;
    const long ld = a.ld;
    mhx_real q = MHX_R(0.0);
    for (int k = 0; k < a.dim; ++k) q = q + mhx_fam_logk(fam[k].family, fam[k].p, a.x[(long)k * ld + c]);
    a.qx[c] = q;
}

// ---------------------------------------------------------------------------------------------
// state in registers, everything but the parameters a compile-time constant
#ifdef MHX_JIT_FAM_REG
MHX_DEV constexpr int mhx_jit_fam_of(const int k)
{
    constexpr int list[] = {MHX_JIT_FAM_LIST};
    static_assert(sizeof(list) / sizeof(list[0]) == MHX_JIT_DIM, "one family per component");
    return list[k];
}

template <int D, int TK, bool STATIC, bool SYM>
MHX_DEV void mhx_fam_reg_body(const mhx_rwmh_args& a, const mhx_real* __restrict__ tparams, const mhx_fam_comp* __restrict__ fam)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchains) return;
    const mhx_u64 id = a.first_chain + (mhx_u64)c;
    const mhx_u32 id_lo = (mhx_u32)id, id_hi = (mhx_u32)(id >> 32);
    const mhx_philox_key ks = mhx_philox_schedule(a.seed);
    const long ld = a.ld;

    mhx_real x[D], y[D];
    const mhx_u32 cu = (mhx_u32)c * MHX_RB;  // row pointers are wave-uniform (scalar), the lane adds its byte offset
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = mhx_ld_off(a.x + (long)k * ld, cu);
    mhx_real lp = a.lp[c];
    mhx_u32 nacc = a.acc_count[c];
    mhx_u32 wave_acc = 0;
    bool last = a.last_acc[c] != 0;
    mhx_accept_cache ac;
    ac.group = 0xffffffffu;
    ac.w.x = ac.w.y = ac.w.z = ac.w.w = 0u;
    mhx_u32 save_next = a.save_next;
    long slot = a.save_slot;
    mhx_real qxc = STATIC ? a.qx[c] : MHX_R(0.0);
    const auto famof = [](const int k) -> int { return mhx_jit_fam_of(k); };

    for (int i = 0; i < a.nsteps; ++i) {
        const mhx_u32 step = a.step0 + (mhx_u32)i;
        mhx_fam_draw_all<true>(D, famof, fam, ks, id_lo, id_hi, step, MHX_STREAM_PROPOSAL, MHX_STREAM_FAMILY,
                         [&](const int k, const mhx_real xi) { y[k] = STATIC ? xi : x[k] + xi; });
        mhx_real ratio = MHX_R(0.0), qy = MHX_R(0.0);
        if (STATIC) {
#pragma unroll
            for (int k = 0; k < D; ++k) qy = qy + mhx_fam_logk(famof(k), fam[k].p, y[k]);
            ratio = qxc - qy;
        } else if (!SYM) {
            mhx_real qb = MHX_R(0.0), qf = MHX_R(0.0);
#pragma unroll
            for (int k = 0; k < D; ++k) {
                qb = qb + mhx_fam_logk(famof(k), fam[k].p, x[k] - y[k]);
                qf = qf + mhx_fam_logk(famof(k), fam[k].p, y[k] - x[k]);
            }
            ratio = qb - qf;
        }
        const mhx_real lpy = mhx_target_eval<TK>(TK, y, D, tparams, a.ntparams, a.tconst);
        const mhx_real logu = mhx_accept_logu(ks, id_lo, id_hi, step, ac);
        const mhx_real loga = (STATIC || !SYM) ? (lpy - lp) + ratio : (lpy - lp);
        const bool acc = logu < loga;                    // strict; NaN compares false => reject
        // (fp64: a move under the execute mask, fp32: a select -- see mhx_rwmh_reg_body)
        if (MHX_REAL64) {
            if (acc) {
#pragma unroll
                for (int k = 0; k < D; ++k) x[k] = y[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) x[k] = acc ? y[k] : x[k];
        }
        lp = acc ? lpy : lp;
        if (STATIC) qxc = acc ? qy : qxc;
        nacc += acc ? 1u : 0u;
        last = acc;
        wave_acc += (mhx_u32)__popcll(__ballot(acc));
        if (step == save_next) {
            mhx_real* slotp = a.samples + slot * (long)(D + 1) * ld;
            const mhx_srd srd = mhx_make_srd(slotp, (mhx_u32)(D + 1) * (mhx_u32)ld * MHX_RB);
            const mhx_u32 ldb = (mhx_u32)ld * MHX_RB;
            mhx_u32 roff = 0u;
            asm volatile("" : "+s"(roff));
#pragma unroll
            for (int k = 0; k < D; ++k) { mhx_srd_store<MHX_REC_STORE_AUX>(srd, cu, roff, x[k]); roff += ldb; }
            mhx_srd_store<MHX_REC_STORE_AUX>(srd, cu, roff, lp);
            a.accepted[slot * ld + c] = acc ? 1 : 0;
            save_next += (mhx_u32)a.thinning;
            ++slot;
        }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) mhx_st_off(a.x + (long)k * ld, cu, x[k]);
    a.lp[c] = lp;
    if (STATIC) a.qx[c] = qxc;
    a.acc_count[c] = nacc;
    a.last_acc[c] = last ? 1 : 0;
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
        atomicAdd(a.acc_total, (mhx_u64)wave_acc);
}

extern "C" __global__ void __launch_bounds__(64)
mhx_jit_fam_reg(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_fam_comp* __restrict__ fam)
{
    mhx_fam_reg_body<MHX_JIT_DIM, MHX_JIT_TK, (MHX_JIT_FAM_STATIC != 0), (MHX_JIT_FAM_SYM != 0)>(a, tparams, fam);
}
#endif
#ifdef MHX_JIT_FAM_GENERIC
extern "C" __global__ void __launch_bounds__(256)
mhx_jit_fam_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_fam_comp* __restrict__ fam, const int symmetric)
{
    mhx_fam_generic_body<MHX_JIT_TK>(a, tparams, fam, symmetric);
}
#endif
MHX_NS_END
