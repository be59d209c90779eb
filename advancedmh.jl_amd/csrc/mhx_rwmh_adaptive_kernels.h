// mhx_rwmh_adaptive_kernels.h -- adaptive random-walk Metropolis-Hastings, one lane per chain: during a warm-up every chain tunes its
// own proposal inside the step kernel, afterwards it runs on as the plain random walk with a diagonal proposal of its own.
//
// The arithmetic is DESIGN.md section 3.18 (Andrieu & Thoms 2008, Algorithm 4 with a diagonal covariance): a log-scale `lam` per chain
// driven towards an acceptance rate, and -- SHAPE -- a running mean m[k] and variance v[k] per coordinate; the proposal's standard
// deviations are eff[k] = sig[k] * exp(lam), sig[k] = sqrt(v[k]) (without SHAPE: the configured s[k]).  Everything is per chain: no
// reduction over chains, so a shard is the matching columns of the larger run, and the recursion is indexed by the GLOBAL step, so
// two calls are one.  Normals, streams, counters and the accept test are the plain lane-per-chain kernels' (mhx_rwmh_kernels.h).
//
// Two phases, and a launch is of one phase only (the host splits the schedule at adapt_steps):
//   adapting    mhx_adp_reg_body<D, TK, PERK, SHAPE>     run-time specialised, one wave per block; x[D], y[D] and (SHAPE) m[D], v[D],
//                                                        sig[D] in VGPRs for the launch.  eff is not held: eff[k] = sig[k] * el is one
//                                                        product, formed where the candidate is, and stored when the launch ends.
//               mhx_adp_generic_body<TK, SHAPE>          run-time dimension, everything in HBM as [dim][ld] / [ld], chain fastest.
//   frozen      mhx_adp_frozen_reg_body<D, TK, PERK>     the plain bodies with ONE change: the proposal's standard deviation is the
//               mhx_adp_frozen_generic_body<TK>          lane's own, read from eff[k][c] (the register form: once per launch).  No m, v,
//                                                        sig or lam: this is the phase that runs long.
// PERK: eff has a row per coordinate (a DIAG proposal, or SHAPE); else one row (an ISO proposal without SHAPE).
#pragma once
#include "mhx_rwmh_kernels.h"

MHX_NS_BEGIN

// Largest dimension the register forms are built for, per phase: the arrays and the temporaries of the unrolled candidate loop must
// fit 512 VGPRs without scratch memory.  Measured by cross-compiling for gfx950 with the options of the run-time build, isotropic
// Gaussian target (tests/test_adaptive_rwmh_cpu.py compiles each at its limit and at the next size tried; the VGPR counts are in
// DESIGN.md section 6.1).  Above the limit the state-in-HBM form of that phase runs.
//   adapting, SHAPE off (x, y; DIAG)            fp64 clean at 60 (501 registers), 76 bytes of scratch at 64;  fp32 clean at 104 (511), 148 bytes at 112
//   adapting, SHAPE on (x, y, m, v, sig)       fp64 clean at 20 (483), 236 bytes at 24;                     fp32 clean at 32 (500), 420 bytes at 40
//   frozen (x, y, eff; a row per coordinate)   fp64 clean at 52 (512), 156 bytes at 56;                     fp32 clean at 80 (471), 20 bytes at 88
// sig is kept, not recomputed: before a coordinate's first finite update it is the configured s, which sqrt(s * s) need not be; and
// the five arrays of SHAPE are VGPRs or AGPRs as the allocator likes -- m, v and sig are touched once per step, so a copy through
// v_accvgpr costs little beside the Philox rounds, and the phase is short.  The frozen form carries only what the plain one does, plus eff.
#define MHX_ADAPT_REG_MAX_DIM (MHX_REAL64 ? 60 : 104)
#define MHX_ADAPT_SHAPE_REG_MAX_DIM (MHX_REAL64 ? 20 : 32)
#define MHX_ADAPT_FROZEN_REG_MAX_DIM (MHX_REAL64 ? 52 : 80)

// the adaptation block of a run: pointers into the run's own arrays and the constants, built once on the host
struct mhx_adp {
    mhx_real* lam;               // [ld]        the log-scale
    mhx_real* eff;               // [ld] or [dim][ld]  the standard deviations the proposal uses
    mhx_real* m;                 // [dim][ld]   SHAPE: running mean
    mhx_real* v;                 // [dim][ld]   ... variance
    mhx_real* sig;               // [dim][ld]   ... sqrt(v) of the last finite update (the configured s before any)
    const mhx_real* gamma;       // [adapt_steps] step sizes min(1, c t^-kappa), t = 1 ..
    const mhx_real* s;           // [dim]       the configured standard deviations (ISO: the scale, repeated)
    const mhx_real* vlo;         // [dim]       s^2 2^-40
    const mhx_real* vhi;         // [dim]       s^2 2^40
    mhx_real target;
    mhx_real lam_min, lam_max;
};

MHX_DEV mhx_real mhx_adp_clamp(const mhx_real v, const mhx_real lo, const mhx_real hi) { return v < lo ? lo : (v > hi ? hi : v); }

// lam after the transition whose log acceptance ratio is loga: p = min(1, exp(loga)), 0 where loga is NaN
MHX_DEV mhx_real mhx_adp_lam(const mhx_adp& ad, const mhx_real g, const mhx_real loga, const mhx_real lam)
{
    const mhx_real p = loga >= MHX_R(0.0) ? MHX_R(1.0) : (loga == loga ? mhx_exp(loga) : MHX_R(0.0));
    return mhx_adp_clamp(mhx_fma(g, p - ad.target, lam), ad.lam_min, ad.lam_max);
}

// one coordinate's mean / variance / sd after the transition; a coordinate whose update is not finite keeps all three
MHX_DEV void mhx_adp_shape(const mhx_real g, const mhx_real xk, const mhx_real vlo, const mhx_real vhi, mhx_real& m, mhx_real& v, mhx_real& sig)
{
    const mhx_real dl = xk - m;
    const mhx_real mn = mhx_fma(g, dl, m);
    const mhx_real vn = mhx_adp_clamp(mhx_fma(g, mhx_fma(dl, dl, -v), v), vlo, vhi);
    if (mhx_fam_finite(mn) && mhx_fam_finite(vn)) {
        m = mn;
        v = vn;
        sig = mhx_sqrt(vn);
    }
}

// lam = 0, sig = eff = s, m = x, v = s * s of every chain (create, mhx_run_init)
MHX_DEV void mhx_adp_reset_body(const mhx_adp& ad, const mhx_real* __restrict__ x, const int nchains, const long ld, const int d,
                                const int perk, const int shape)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchains) return;
    ad.lam[c] = MHX_R(0.0);
    if (!perk) ad.eff[c] = ad.s[0];
    for (int k = 0; k < d; ++k) {
        const mhx_real s = ad.s[k];
        if (perk) ad.eff[(long)k * ld + c] = s;
        if (shape) {
            ad.m[(long)k * ld + c] = x[(long)k * ld + c];
            ad.v[(long)k * ld + c] = s * s;
            ad.sig[(long)k * ld + c] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// adapting phase, state in HBM: every transition `step` of the launch has step <= adapt_steps
template <int TK, bool SHAPE>
MHX_DEV void mhx_adp_generic_body(const mhx_rwmh_args& a, const mhx_real* __restrict__ tparams, const mhx_adp& ad, const int perk)
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
    mhx_real* es = ad.eff + c;

    mhx_real lp = a.lp[c];
    mhx_real lam = ad.lam[c];
    mhx_u32 nacc = a.acc_count[c];
    mhx_u32 wave_acc = 0;
    bool last = a.last_acc[c] != 0;
    mhx_accept_cache ac;
    ac.group = 0xffffffffu;
    ac.w.x = ac.w.y = ac.w.z = ac.w.w = 0u;
    mhx_u32 save_next = a.save_next;
    long slot = a.save_slot;
    const int nblk = (d + 3) >> 2;

    for (int i = 0; i < a.nsteps; ++i) {
        const mhx_u32 step = a.step0 + (mhx_u32)i;
        for (int b = 0; b < nblk; ++b) {
            mhx_real n[4];
            mhx_normal4(ks, id_lo, id_hi, step, MHX_STREAM_PROPOSAL, (mhx_u32)b, n);
            for (int j = 0; j < 4; ++j) {
                const int k = 4 * b + j;
                if (k < d) ys[(long)k * ld] = mhx_fma(es[perk ? (long)k * ld : 0l], n[j], xs[(long)k * ld]);
            }
        }
        mhx_strided_x yv;
        yv.base = ys;
        yv.ld = ld;
        const mhx_real lpy = mhx_target_eval<TK>(a.target_kind, yv, d, tparams, a.ntparams, a.tconst);
        const mhx_real logu = mhx_accept_logu(ks, id_lo, id_hi, step, ac);
        const mhx_real loga = lpy - lp;
        const bool acc = logu < loga;
        lp = acc ? lpy : lp;
        nacc += acc ? 1u : 0u;
        last = acc;
        wave_acc += (mhx_u32)__popcll(__ballot(acc));
        if (acc)
            for (int k = 0; k < d; ++k) xs[(long)k * ld] = ys[(long)k * ld];
        if (step == save_next) {
            mhx_real* row = a.samples + slot * (long)(d + 1) * ld + c;
            for (int k = 0; k < d; ++k) row[(long)k * ld] = xs[(long)k * ld];
            row[(long)d * ld] = lp;
            a.accepted[slot * ld + c] = acc ? 1 : 0;
            save_next += (mhx_u32)a.thinning;
            ++slot;
        }
        // ---- adapt: lam, then the shape for k ascending, then eff
        const mhx_real g = ad.gamma[step - 1u];
        lam = mhx_adp_lam(ad, g, loga, lam);
        const mhx_real el = mhx_exp(lam);
        if (SHAPE) {
            for (int k = 0; k < d; ++k) {
                const long o = (long)k * ld + c;
                mhx_real m = ad.m[o], v = ad.v[o], sg = ad.sig[o];
                mhx_adp_shape(g, xs[(long)k * ld], ad.vlo[k], ad.vhi[k], m, v, sg);
                ad.m[o] = m;
                ad.v[o] = v;
                ad.sig[o] = sg;
                es[(long)k * ld] = sg * el;
            }
        } else if (perk) {
            for (int k = 0; k < d; ++k) es[(long)k * ld] = ad.s[k] * el;
        } else {
            es[0] = ad.s[0] * el;
        }
    }
    a.lp[c] = lp;
    ad.lam[c] = lam;
    a.acc_count[c] = nacc;
    a.last_acc[c] = last ? 1 : 0;
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
        atomicAdd(a.acc_total, (mhx_u64)wave_acc);
}

// frozen phase, state in HBM: mhx_rwmh_generic_body's zero-mean random walk with the lane's own standard deviations
template <int TK>
MHX_DEV void mhx_adp_frozen_generic_body(const mhx_rwmh_args& a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ eff,
                                         const int perk)
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
    const mhx_real* es = eff + c;

    mhx_real lp = a.lp[c];
    mhx_u32 nacc = a.acc_count[c];
    mhx_u32 wave_acc = 0;
    bool last = a.last_acc[c] != 0;
    mhx_accept_cache ac;
    ac.group = 0xffffffffu;
    ac.w.x = ac.w.y = ac.w.z = ac.w.w = 0u;
    mhx_u32 save_next = a.save_next;
    long slot = a.save_slot;
    const int nblk = (d + 3) >> 2;

    for (int i = 0; i < a.nsteps; ++i) {
        const mhx_u32 step = a.step0 + (mhx_u32)i;
        for (int b = 0; b < nblk; ++b) {
            mhx_real n[4];
            mhx_normal4(ks, id_lo, id_hi, step, MHX_STREAM_PROPOSAL, (mhx_u32)b, n);
            for (int j = 0; j < 4; ++j) {
                const int k = 4 * b + j;
                if (k < d) ys[(long)k * ld] = mhx_fma(es[perk ? (long)k * ld : 0l], n[j], xs[(long)k * ld]);
            }
        }
        mhx_strided_x yv;
        yv.base = ys;
        yv.ld = ld;
        const mhx_real lpy = mhx_target_eval<TK>(a.target_kind, yv, d, tparams, a.ntparams, a.tconst);
        const mhx_real logu = mhx_accept_logu(ks, id_lo, id_hi, step, ac);
        const bool acc = logu < (lpy - lp);
        lp = acc ? lpy : lp;
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
    a.acc_count[c] = nacc;
    a.last_acc[c] = last ? 1 : 0;
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
        atomicAdd(a.acc_total, (mhx_u64)wave_acc);
}

// ---------------------------------------------------------------------------------------------
// the register forms: run-time specialised, one wave per block (mhx_rwmh_reg_body's frame: scalar row pointers, SRD record stores)
#if defined(MHX_JIT_ADAPTIVE_REG) || defined(MHX_JIT_ADAPTIVE_FROZEN_REG)
// the record of one state (ext/AdvancedMHMCMCChainsExt.jl:96-105 layout, chain fastest), as mhx_rwmh_reg_body writes it
template <int D>
MHX_DEV void mhx_adp_record(const mhx_rwmh_args& a, const long slot, const long ld, const int c, const mhx_u32 cu, const mhx_real (&x)[D],
                            const mhx_real lp, const bool acc)
{
    mhx_real* slotp = a.samples + slot * (long)(D + 1) * ld;
    const mhx_srd srd = mhx_make_srd(slotp, (mhx_u32)(D + 1) * (mhx_u32)ld * MHX_RB);
    const mhx_u32 ldb = (mhx_u32)ld * MHX_RB;
    mhx_u32 roff = 0u;
    asm volatile("" : "+s"(roff));
#pragma unroll
    for (int k = 0; k < D; ++k) { mhx_srd_store<MHX_REC_STORE_AUX>(srd, cu, roff, x[k]); roff += ldb; }
    mhx_srd_store<MHX_REC_STORE_AUX>(srd, cu, roff, lp);
    a.accepted[slot * ld + c] = acc ? 1 : 0;
}
#endif

#ifdef MHX_JIT_ADAPTIVE_REG
template <int D, int TK, bool PERK, bool SHAPE>
MHX_DEV void mhx_adp_reg_body(const mhx_rwmh_args& a, const mhx_real* __restrict__ tparams, const mhx_adp& ad)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchains) return;
    const mhx_u64 id = a.first_chain + (mhx_u64)c;
    const mhx_u32 id_lo = (mhx_u32)id, id_hi = (mhx_u32)(id >> 32);
    const mhx_philox_key ks = mhx_philox_schedule(a.seed);
    const long ld = a.ld;

    mhx_real x[D], y[D];
    mhx_real m[SHAPE ? D : 1], v[SHAPE ? D : 1], sg[SHAPE ? D : 1];
    const mhx_u32 cu = (mhx_u32)c * MHX_RB;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        x[k] = mhx_ld_off(a.x + (long)k * ld, cu);
        if (SHAPE) {
            m[SHAPE ? k : 0] = mhx_ld_off(ad.m + (long)k * ld, cu);
            v[SHAPE ? k : 0] = mhx_ld_off(ad.v + (long)k * ld, cu);
            sg[SHAPE ? k : 0] = mhx_ld_off(ad.sig + (long)k * ld, cu);
        }
    }
    mhx_real lp = a.lp[c];
    mhx_real lam = ad.lam[c];
    // el = exp(lam) as the last adapting transition left it; before the first one eff is the configured s itself (no exp applied)
    mhx_real el = a.step0 == 1u ? MHX_R(1.0) : mhx_exp(lam);
    mhx_u32 nacc = a.acc_count[c];
    mhx_u32 wave_acc = 0;
    bool last = a.last_acc[c] != 0;
    mhx_accept_cache ac;
    ac.group = 0xffffffffu;
    ac.w.x = ac.w.y = ac.w.z = ac.w.w = 0u;
    mhx_u32 save_next = a.save_next;
    long slot = a.save_slot;

    for (int i = 0; i < a.nsteps; ++i) {
        const mhx_u32 step = a.step0 + (mhx_u32)i;
#pragma unroll
        for (int b = 0; b < (D + 3) / 4; ++b) {
            mhx_real n[4];
            mhx_normal4(ks, id_lo, id_hi, step, MHX_STREAM_PROPOSAL, (mhx_u32)b, n);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 4 * b + j;
                if (k < D) y[k] = mhx_fma((SHAPE ? sg[SHAPE ? k : 0] : ad.s[PERK ? k : 0]) * el, n[j], x[k]);
            }
        }
        const mhx_real lpy = mhx_target_eval<TK>(TK, y, D, tparams, a.ntparams, a.tconst);
        const mhx_real logu = mhx_accept_logu(ks, id_lo, id_hi, step, ac);
        const mhx_real loga = lpy - lp;
        const bool acc = logu < loga;
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
        nacc += acc ? 1u : 0u;
        last = acc;
        wave_acc += (mhx_u32)__popcll(__ballot(acc));
        if (step == save_next) {
            mhx_adp_record<D>(a, slot, ld, c, cu, x, lp, acc);
            save_next += (mhx_u32)a.thinning;
            ++slot;
        }
        // ---- adapt
        const mhx_real g = ad.gamma[step - 1u];
        lam = mhx_adp_lam(ad, g, loga, lam);
        if (SHAPE) {
#pragma unroll
            for (int k = 0; k < D; ++k) mhx_adp_shape(g, x[k], ad.vlo[k], ad.vhi[k], m[SHAPE ? k : 0], v[SHAPE ? k : 0], sg[SHAPE ? k : 0]);
        }
        el = mhx_exp(lam);
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        mhx_st_off(a.x + (long)k * ld, cu, x[k]);
        if (SHAPE) {
            mhx_st_off(ad.m + (long)k * ld, cu, m[SHAPE ? k : 0]);
            mhx_st_off(ad.v + (long)k * ld, cu, v[SHAPE ? k : 0]);
            mhx_st_off(ad.sig + (long)k * ld, cu, sg[SHAPE ? k : 0]);
        }
        if (PERK || k == 0) mhx_st_off(ad.eff + (long)k * ld, cu, (SHAPE ? sg[SHAPE ? k : 0] : ad.s[k]) * el);
    }
    a.lp[c] = lp;
    ad.lam[c] = lam;
    a.acc_count[c] = nacc;
    a.last_acc[c] = last ? 1 : 0;
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
        atomicAdd(a.acc_total, (mhx_u64)wave_acc);
}

extern "C" __global__ void __launch_bounds__(64)
mhx_jit_adaptive_reg(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_adp ad)
{
    mhx_adp_reg_body<MHX_JIT_DIM, MHX_JIT_TK, (MHX_JIT_PERK != 0), (MHX_JIT_SHAPE != 0)>(a, tparams, ad);
}
#endif

#ifdef MHX_JIT_ADAPTIVE_FROZEN_REG
template <int D, int TK, bool PERK>
MHX_DEV void mhx_adp_frozen_reg_body(const mhx_rwmh_args& a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ eff)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchains) return;
    const mhx_u64 id = a.first_chain + (mhx_u64)c;
    const mhx_u32 id_lo = (mhx_u32)id, id_hi = (mhx_u32)(id >> 32);
    const mhx_philox_key ks = mhx_philox_schedule(a.seed);
    const long ld = a.ld;

    mhx_real x[D], y[D], e[PERK ? D : 1];
    const mhx_u32 cu = (mhx_u32)c * MHX_RB;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        x[k] = mhx_ld_off(a.x + (long)k * ld, cu);
        if (PERK || k == 0) e[PERK ? k : 0] = mhx_ld_off(eff + (long)k * ld, cu);      // the lane's column, once per launch
    }
    mhx_real lp = a.lp[c];
    mhx_u32 nacc = a.acc_count[c];
    mhx_u32 wave_acc = 0;
    bool last = a.last_acc[c] != 0;
    mhx_accept_cache ac;
    ac.group = 0xffffffffu;
    ac.w.x = ac.w.y = ac.w.z = ac.w.w = 0u;
    mhx_u32 save_next = a.save_next;
    long slot = a.save_slot;

    for (int i = 0; i < a.nsteps; ++i) {
        const mhx_u32 step = a.step0 + (mhx_u32)i;
#pragma unroll
        for (int b = 0; b < (D + 3) / 4; ++b) {
            mhx_real n[4];
            mhx_normal4(ks, id_lo, id_hi, step, MHX_STREAM_PROPOSAL, (mhx_u32)b, n);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 4 * b + j;
                if (k < D) y[k] = mhx_fma(e[PERK ? k : 0], n[j], x[k]);
            }
        }
        const mhx_real lpy = mhx_target_eval<TK>(TK, y, D, tparams, a.ntparams, a.tconst);
        const mhx_real logu = mhx_accept_logu(ks, id_lo, id_hi, step, ac);
        const bool acc = logu < (lpy - lp);          // strict; NaN compares false => reject
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
        nacc += acc ? 1u : 0u;
        last = acc;
        wave_acc += (mhx_u32)__popcll(__ballot(acc));
        if (step == save_next) {
            mhx_adp_record<D>(a, slot, ld, c, cu, x, lp, acc);
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
mhx_jit_adaptive_frozen_reg(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ eff)
{
    mhx_adp_frozen_reg_body<MHX_JIT_DIM, MHX_JIT_TK, (MHX_JIT_PERK != 0)>(a, tparams, eff);
}
#endif

#ifdef MHX_JIT_ADAPTIVE_GENERIC
extern "C" __global__ void __launch_bounds__(256)
mhx_jit_adaptive_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_adp ad, const int perk)
{
    mhx_adp_generic_body<MHX_JIT_TK, (MHX_JIT_SHAPE != 0)>(a, tparams, ad, perk);
}
extern "C" __global__ void __launch_bounds__(256)
mhx_jit_adaptive_frozen_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ eff, const int perk)
{
    mhx_adp_frozen_generic_body<MHX_JIT_TK>(a, tparams, eff, perk);
}
#endif
MHX_NS_END
