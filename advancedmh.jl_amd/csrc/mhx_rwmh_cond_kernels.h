// mhx_rwmh_cond_kernels.h -- Metropolis-Hastings with a conditional proposal: independent univariate components whose parameters
// are a function of the state, one lane per chain.
//
// Replaces the reference's step (src/mh-core.jl:92-117) for the function proposals of src/proposal.jl:92-126:
// StaticProposal(x -> Normal(x, 1)), RandomWalkProposal(x -> Laplace(x, 1)), ...  Component k has a fixed family of
// mhx_device_math.h and the parameters (p0_k, p1_k) = P_k(x), P the user's parameter map
// (MHX_PROPOSAL_PARAMS, inlined).  With K(p; v) the sum of the log-kernels and Z(p) the sum of the log-normalisers, both in index
// order:
//   RandomWalkProposal   y = x + xi,  xi ~ p(x);   ratio = (K(p(y); x - y) - K(p(x); y - x)) + (Z(p(y)) - Z(p(x)))
//   StaticProposal       y = xi,      xi ~ p(x);   ratio = (K(p(y); x) - K(p(x); y)) + (Z(p(y)) - Z(p(x)))     (proposal.jl:120-126)
//   declared symmetric   the ratio is not formed (proposal.jl:195-196): the user is trusted.
// p(y) is evaluated and checked at every step, symmetric or not: a candidate whose parameters are not those of a distribution
// (sigma, theta <= 0, a >= b, anything not finite) is REJECTED by a branch of its own.  This is the one place the engine departs
// from the reference, which would throw from the distribution's constructor at the next step.  p(x) and Z(p(x)) are carried from
// step to step and recomputed from x at the start of every launch (the map is deterministic: the same bits), so a checkpoint, a
// resumed run and a shard need no state beyond x.  A map that returns constants gives Z - Z = +0 and the chain of
// mhx_rwmh_family_kernels.h with those constants, bit for bit.
//
// Both kernels are compiled at run time only (the map is user source) and share the arithmetic:
//   mhx_cond_reg_body<D, ...>   x[D], y[D], p(x), p(y) and Z in VGPRs for a whole launch, families compile-time constants
//                               (MHX_JIT_FAM_LIST), records through SRD stores;
//   mhx_cond_generic_body       run-time dimension, state in HBM as [dim][nchains], p(x) and p(y) as [2 dim][nchains] rows each of
//                               a buffer the run owns.
// The same chain bit for bit: same counters, same operations in the same order.
#pragma once
#include "mhx_rwmh_family_kernels.h"

// Largest dimension the register form is built for: x[D], y[D], p(x)[2 D], p(y)[2 D] and the temporaries of the unrolled loops
// must fit 512 VGPRs without scratch memory.  Measured by cross-compiling for gfx950 with the options of the run-time build, a map
// that sets every parameter of every component from two coordinates of the state, all-Cauchy (the worst family) and all seven
// mixed, walk and static, in steps of 4 (fp64) and 8 (fp32):
//   fp64   d = 12: 339 VGPRs   16: 426   20: 512, no scratch   24: 364 bytes of scratch (Cauchy), 12 (mixed walk)
//   fp32   d = 16: 240 VGPRs   24: 345   32: 447, no scratch   40: 164 bytes of scratch (Cauchy)
// tests/test_conditional_cpu.py compiles the kernel at the limit and at the next size tried.  Above the limit the state-in-HBM
// form runs.
#define MHX_COND_REG_MAX_DIM (MHX_REAL64 ? 20 : 32)
#define MHX_COND_REG_NEXT_DIM_TRIED (MHX_REAL64 ? 24 : 40)

#ifdef MHX_HAVE_PROPOSAL_PARAMS
MHX_NS_BEGIN

template <bool UNROLL, class F>
MHX_DEV void mhx_cond_for(const int d, const F& f)
{
    if constexpr (UNROLL) {
#pragma unroll
        for (int k = 0; k < d; ++k) f(k);
    } else {
        for (int k = 0; k < d; ++k) f(k);
    }
}

// The parameter row of component k as mhx_fam_draw / mhx_fam_logk read it, made from a lane's own (p0, p1) = get(k, 0 / 1) and the
// constant table: Uniform's p[2] = b - a is formed here, in the width; the shape of a Gamma family and what the host derived
// from it (p[2 .. 5]) are the table's.
struct mhx_cond_row { mhx_real p[6]; };
template <class FamOf, class Get>
struct mhx_cond_tab {
    const FamOf& famof;
    const mhx_fam_comp* fam;
    const Get& get;
    MHX_DEV mhx_cond_row operator[](const int k) const
    {
        const int f = famof(k);
        const bool gam = f == MHX_FAMILY_GAMMA || f == MHX_FAMILY_INVERSE_GAMMA;
        mhx_cond_row r;
        r.p[0] = gam ? fam[k].p[0] : get(k, 0);
        r.p[1] = get(k, 1);
        r.p[2] = f == MHX_FAMILY_UNIFORM ? r.p[1] - r.p[0] : fam[k].p[2];
        r.p[3] = fam[k].p[3];
        r.p[4] = fam[k].p[4];
        r.p[5] = fam[k].p[5];
        return r;
    }
};
template <class FamOf, class Get>
MHX_DEV mhx_cond_tab<FamOf, Get> mhx_cond_make_tab(const FamOf& famof, const mhx_fam_comp* fam, const Get& get)
{
    return mhx_cond_tab<FamOf, Get>{famof, fam, get};
}

// what the user's source calls: p.set(k, j, value); a k or j outside the table is ignored (hand-written source must not write
// out of bounds)
template <class FamOf, class Set>
struct mhx_cond_sink {
    const FamOf& famof;
    const Set& put;
    const int d;
    MHX_DEV void set(const int k, const int j, const mhx_real v) const
    {
        if ((unsigned)k >= (unsigned)d || (unsigned)j > 1u) return;
        const int f = famof(k);
        if (j == 0 && (f == MHX_FAMILY_GAMMA || f == MHX_FAMILY_INVERSE_GAMMA)) return;       // the shape is a constant
        put(k, j, v);
    }
};

// p(s): the table's constants, then the map; whether every row is a distribution's; Z(p(s)) when the caller forms a ratio
template <bool UNROLL, bool WANT_Z, class FamOf, class X, class Get, class Set>
MHX_DEV bool mhx_cond_eval(const int d, const FamOf& famof, const mhx_fam_comp* __restrict__ fam, const X& s, const Get& get, const Set& put,
                           const mhx_real* __restrict__ cdata, const int ncdata, mhx_real& Z)
{
    mhx_cond_for<UNROLL>(d, [&](const int k) { put(k, 0, fam[k].p[0]); put(k, 1, fam[k].p[1]); });
    mhx_user_proposal_params(s, mhx_cond_sink<FamOf, Set>{famof, put, d}, d, cdata, ncdata);
    const auto tab = mhx_cond_make_tab(famof, fam, get);
    bool ok = true;
    mhx_real z = MHX_R(0.0);
    mhx_cond_for<UNROLL>(d, [&](const int k) {
        const mhx_cond_row r = tab[k];
        ok = ok && mhx_fam_valid(famof(k), r.p);
        if (WANT_Z) z = z + mhx_fam_lognorm(famof(k), r.p);
    });
    Z = z;
    return ok;
}

// (K(p(y); .) - K(p(x); .)) + (Z(p(y)) - Z(p(x))) of one transition x -> y
template <bool UNROLL, class FamOf, class GetX, class GetY, class XA, class YA>
MHX_DEV mhx_real mhx_cond_ratio(const int d, const bool stat, const FamOf& famof, const mhx_fam_comp* __restrict__ fam, const GetX& getx,
                                const GetY& gety, const XA& xa, const YA& ya, const mhx_real Zx, const mhx_real Zy)
{
    const auto tx = mhx_cond_make_tab(famof, fam, getx);
    const auto ty = mhx_cond_make_tab(famof, fam, gety);
    mhx_real kb = MHX_R(0.0), kf = MHX_R(0.0);
    mhx_cond_for<UNROLL>(d, [&](const int k) {
        const mhx_real xk = xa(k), yk = ya(k);
        kb = kb + mhx_fam_logk(famof(k), ty[k].p, stat ? xk : xk - yk);
        kf = kf + mhx_fam_logk(famof(k), tx[k].p, stat ? yk : yk - xk);
    });
    return (kb - kf) + (Zy - Zx);
}

// ---------------------------------------------------------------------------------------------
// state in HBM, run-time dimension.  pbuf: [4 dim][ld], rows 2 k + j of p(x) then rows 2 dim + 2 k + j of p(y)
template <int TK>
MHX_DEV void mhx_cond_generic_body(const mhx_rwmh_args& a, const mhx_real* __restrict__ tparams, const mhx_fam_comp* __restrict__ fam,
                                   const mhx_real* __restrict__ cdata, const int ncdata, mhx_real* __restrict__ pbuf, const int stat,
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
    mhx_real* pxs = pbuf + c;
    mhx_real* pys = pbuf + 2l * d * ld + c;

    mhx_real lp = a.lp[c];
    mhx_u32 nacc = a.acc_count[c];
    mhx_u32 wave_acc = 0;
    bool last = a.last_acc[c] != 0;
    mhx_accept_cache ac;
    ac.group = 0xffffffffu;
    ac.w.x = ac.w.y = ac.w.z = ac.w.w = 0u;
    mhx_u32 save_next = a.save_next;
    long slot = a.save_slot;
    const auto famof = [&](const int k) -> int { return fam[k].family; };
    const auto getx = [&](const int k, const int j) -> mhx_real { return pxs[(long)(2 * k + j) * ld]; };
    const auto gety = [&](const int k, const int j) -> mhx_real { return pys[(long)(2 * k + j) * ld]; };
    const auto putx = [&](const int k, const int j, const mhx_real v) { pxs[(long)(2 * k + j) * ld] = v; };
    const auto puty = [&](const int k, const int j, const mhx_real v) { pys[(long)(2 * k + j) * ld] = v; };
    mhx_strided_x xv, yv;
    xv.base = xs; xv.ld = ld;
    yv.base = ys; yv.ld = ld;
    mhx_real Zx = MHX_R(0.0);
    if (symmetric) (void)mhx_cond_eval<false, false>(d, famof, fam, xv, getx, putx, cdata, ncdata, Zx);
    else (void)mhx_cond_eval<false, true>(d, famof, fam, xv, getx, putx, cdata, ncdata, Zx);
    const auto tabx = mhx_cond_make_tab(famof, fam, getx);

    for (int i = 0; i < a.nsteps; ++i) {
        const mhx_u32 step = a.step0 + (mhx_u32)i;
        mhx_fam_draw_all<false>(d, famof, tabx, ks, id_lo, id_hi, step, MHX_STREAM_PROPOSAL, MHX_STREAM_FAMILY,
                                [&](const int k, const mhx_real xi) { ys[(long)k * ld] = stat ? xi : xs[(long)k * ld] + xi; });
        mhx_real Zy = MHX_R(0.0), ratio = MHX_R(0.0);
        bool ok;
        if (symmetric) {
            ok = mhx_cond_eval<false, false>(d, famof, fam, yv, gety, puty, cdata, ncdata, Zy);
        } else {
            ok = mhx_cond_eval<false, true>(d, famof, fam, yv, gety, puty, cdata, ncdata, Zy);
            ratio = mhx_cond_ratio<false>(d, stat != 0, famof, fam, getx, gety, [&](const int k) { return xs[(long)k * ld]; },
                                          [&](const int k) { return ys[(long)k * ld]; }, Zx, Zy);
        }
        const mhx_real lpy = mhx_target_eval<TK>(a.target_kind, yv, d, tparams, a.ntparams, a.tconst);
        const mhx_real logu = mhx_accept_logu(ks, id_lo, id_hi, step, ac);
        const mhx_real loga = symmetric ? (lpy - lp) : (lpy - lp) + ratio;
        const bool acc = ok && logu < loga;              // invalid p(y): rejected here; strict; NaN compares false => reject
        lp = acc ? lpy : lp;
        Zx = acc ? Zy : Zx;
        nacc += acc ? 1u : 0u;
        last = acc;
        wave_acc += (mhx_u32)__popcll(__ballot(acc));
        if (acc) {
            for (int k = 0; k < d; ++k) xs[(long)k * ld] = ys[(long)k * ld];
            for (int k = 0; k < 2 * d; ++k) pxs[(long)k * ld] = pys[(long)k * ld];
        }
        if (step == save_next) {
            mhx_real* row = a.samples + slot * (long)(d + 1) * ld + c;
            for (int k = 0; k < d; ++k) row[(long)k * ld] = xs[(long)k * ld];
            row[(long)d * ld] = lp;
            a.accepted[slot * ld + c] = acc ? 1 : 0;
            save_next += (mhx_u32)a.thinning;
            ++slot;
        }
    }
    a.lp[c] = lp;
    a.acc_count[c] = nacc;
    a.last_acc[c] = last ? 1 : 0;
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
        atomicAdd(a.acc_total, (mhx_u64)wave_acc);
}

// p(x) of every chain's current state (after init / set_state): the rows of p(x) are written to pbuf ([2 dim][ld] is enough), every
// chain whose parameters are not a distribution's counts one in *nbad
MHX_DEV void mhx_cond_check_body(const mhx_rwmh_args& a, const mhx_fam_comp* __restrict__ fam, const mhx_real* __restrict__ cdata,
                                 const int ncdata, mhx_real* __restrict__ pbuf, int* __restrict__ nbad)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchains) return;
    const long ld = a.ld;
    mhx_real* pxs = pbuf + c;
    mhx_strided_x xv;
    xv.base = a.x + c;
    xv.ld = ld;
    mhx_real Z;
    const bool ok = mhx_cond_eval<false, false>(a.dim, [&](const int k) -> int { return fam[k].family; }, fam, xv,
                                                [&](const int k, const int j) -> mhx_real { return pxs[(long)(2 * k + j) * ld]; },
                                                [&](const int k, const int j, const mhx_real v) { pxs[(long)(2 * k + j) * ld] = v; },
                                                cdata, ncdata, Z);
    if (!ok) atomicAdd(nbad, 1);
}

extern "C" __global__ void __launch_bounds__(256)
mhx_jit_cond_check(const mhx_rwmh_args a, const mhx_fam_comp* __restrict__ fam, const mhx_real* __restrict__ cdata, const int ncdata,
                   mhx_real* __restrict__ pbuf, int* __restrict__ nbad)
{
    mhx_cond_check_body(a, fam, cdata, ncdata, pbuf, nbad);
}

// ---------------------------------------------------------------------------------------------
// state in registers, everything but the table's constants a compile-time constant
#ifdef MHX_JIT_COND_REG
MHX_DEV constexpr int mhx_jit_cond_fam_of(const int k)
{
    constexpr int list[] = {MHX_JIT_FAM_LIST};
    static_assert(sizeof(list) / sizeof(list[0]) == MHX_JIT_DIM, "one family per component");
    return list[k];
}

template <int D, int TK, bool STATIC, bool SYM>
MHX_DEV void mhx_cond_reg_body(const mhx_rwmh_args& a, const mhx_real* __restrict__ tparams, const mhx_fam_comp* __restrict__ fam,
                               const mhx_real* __restrict__ cdata, const int ncdata)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchains) return;
    const mhx_u64 id = a.first_chain + (mhx_u64)c;
    const mhx_u32 id_lo = (mhx_u32)id, id_hi = (mhx_u32)(id >> 32);
    const mhx_philox_key ks = mhx_philox_schedule(a.seed);
    const long ld = a.ld;

    mhx_real x[D], y[D], px[2 * D], py[2 * D];
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
    const auto famof = [](const int k) -> int { return mhx_jit_cond_fam_of(k); };
    const auto getx = [&](const int k, const int j) -> mhx_real { return px[2 * k + j]; };
    const auto gety = [&](const int k, const int j) -> mhx_real { return py[2 * k + j]; };
    const auto putx = [&](const int k, const int j, const mhx_real v) { px[2 * k + j] = v; };
    const auto puty = [&](const int k, const int j, const mhx_real v) { py[2 * k + j] = v; };
    mhx_real Zx = MHX_R(0.0);
    (void)mhx_cond_eval<true, !SYM>(D, famof, fam, x, getx, putx, cdata, ncdata, Zx);
    const auto tabx = mhx_cond_make_tab(famof, fam, getx);

    for (int i = 0; i < a.nsteps; ++i) {
        const mhx_u32 step = a.step0 + (mhx_u32)i;
        mhx_fam_draw_all<true>(D, famof, tabx, ks, id_lo, id_hi, step, MHX_STREAM_PROPOSAL, MHX_STREAM_FAMILY,
                               [&](const int k, const mhx_real xi) { y[k] = STATIC ? xi : x[k] + xi; });
        mhx_real Zy = MHX_R(0.0), ratio = MHX_R(0.0);
        const bool ok = mhx_cond_eval<true, !SYM>(D, famof, fam, y, gety, puty, cdata, ncdata, Zy);
        if (!SYM)
            ratio = mhx_cond_ratio<true>(D, STATIC, famof, fam, getx, gety, [&](const int k) { return x[k]; },
                                         [&](const int k) { return y[k]; }, Zx, Zy);
        const mhx_real lpy = mhx_target_eval<TK>(TK, y, D, tparams, a.ntparams, a.tconst);
        const mhx_real logu = mhx_accept_logu(ks, id_lo, id_hi, step, ac);
        const mhx_real loga = SYM ? (lpy - lp) : (lpy - lp) + ratio;
        const bool acc = ok && logu < loga;              // invalid p(y): rejected here; strict; NaN compares false => reject
        // (fp64: a move under the execute mask, fp32: a select -- see mhx_rwmh_reg_body)
        if (MHX_REAL64) {
            if (acc) {
#pragma unroll
                for (int k = 0; k < D; ++k) x[k] = y[k];
#pragma unroll
                for (int k = 0; k < 2 * D; ++k) px[k] = py[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) x[k] = acc ? y[k] : x[k];
#pragma unroll
            for (int k = 0; k < 2 * D; ++k) px[k] = acc ? py[k] : px[k];
        }
        lp = acc ? lpy : lp;
        Zx = acc ? Zy : Zx;
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
    a.acc_count[c] = nacc;
    a.last_acc[c] = last ? 1 : 0;
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
        atomicAdd(a.acc_total, (mhx_u64)wave_acc);
}

extern "C" __global__ void __launch_bounds__(64)
mhx_jit_cond_reg(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_fam_comp* __restrict__ fam,
                 const mhx_real* __restrict__ cdata, const int ncdata)
{
    mhx_cond_reg_body<MHX_JIT_DIM, MHX_JIT_TK, (MHX_JIT_FAM_STATIC != 0), (MHX_JIT_FAM_SYM != 0)>(a, tparams, fam, cdata, ncdata);
}
#endif
#ifdef MHX_JIT_COND_GENERIC
extern "C" __global__ void __launch_bounds__(256)
mhx_jit_cond_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_fam_comp* __restrict__ fam,
                     const mhx_real* __restrict__ cdata, const int ncdata, mhx_real* __restrict__ pbuf, const int stat, const int symmetric)
{
    mhx_cond_generic_body<MHX_JIT_TK>(a, tparams, fam, cdata, ncdata, pbuf, stat, symmetric);
}
#endif
MHX_NS_END
#endif
