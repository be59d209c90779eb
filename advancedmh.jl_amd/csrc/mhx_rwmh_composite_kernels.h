// mhx_rwmh_composite_kernels.h -- Metropolis-Hastings with a COMPOSITE proposal: an ordered list of blocks of univariate components,
// each block with its own kind (walk or static), its own symmetric flag and, optionally, parameters that depend on the block's own
// slice of the state; one lane per chain.
//
// Replaces the reference's step (src/mh-core.jl:92-117) for Array{Proposal} and NamedTuple{Proposal} (src/proposal.jl:128-175,
// 198-240): the shape is ragged across parameters but the same for every chain.  DESIGN.md section 3.15:
//   draws    component k, by its GLOBAL index, draws xi_k as mhx_rwmh_family_kernels.h / mhx_rwmh_cond_kernels.h do, from its row
//            p_k(x): the draws do not depend on the grouping.  y_k = xi_k in a static block, x_k + xi_k in a walk block.
//   ratio    every block b NOT declared symmetric gives r_b = (K_b(p(y); .) - K_b(p(x); .)) + (Z_b(p(y)) - Z_b(p(x))), K_b and Z_b the
//            sums over the block's components from 0 in index order, the arguments x_k / y_k (static) or x_k - y_k / y_k - x_k
//            (walk); ratio = the first r_b, then + r_b in block order (logratio_proposal_density summed per entry).  A block
//            without a mapped component leaves Z_b - Z_b = +0 out.  No such block: log alpha = lp_y - lp_x.
//   validity p(y) of every mapped component is checked at every step, in symmetric blocks too; an invalid candidate is rejected by
//            a branch of its own.
// p(x) and Z_b(p(x)) are recomputed from x at the start of a launch (register form) or of a step (state-in-HBM form): the map is
// deterministic, so a checkpoint, a resumed run and a shard need no state beyond x.  One block reproduces the chain of
// mhx_rwmh_cond_kernels.h bit for bit, and that of mhx_rwmh_family_kernels.h when nothing is mapped.
//
// The user's map writes p.set(k, j, value) with the GLOBAL component index k; a p.set on an entry not declared mapped is ignored.
//
// Both kernels are compiled at run time only and share the arithmetic:
//   mhx_composite_reg_body<D, ...>   x[D], y[D], the MAPPED entries of p(x) and p(y) and the Z_b of the blocks that need one in VGPRs;
//                                    unmapped parameters are read from the wave-uniform table.  Families, kinds, block ids, mapped
//                                    masks and symmetric bits are compile-time lists (MHX_JIT_FAM_LIST, MHX_JIT_CMP_STATIC_LIST,
//                                    MHX_JIT_CMP_BLOCK_LIST, MHX_JIT_CMP_MAPPED_LIST, MHX_JIT_CMP_SYM_LIST).
//   mhx_composite_generic_body       run-time dimension, state in HBM, kinds / masks / blocks from a small device table, the
//                                    parameter buffer of mhx_cond_generic_body.
// The same chain bit for bit: same counters, same operations in the same order.
#pragma once
#include "mhx_rwmh_cond_kernels.h"

// What the register form is built for.  Its VGPRs hold x[D], y[D], two reals per mapped ENTRY (p(x), p(y)) and two per block that
// carries a Z (a block that is not symmetric and has a mapped component).  The rule (mhx_api_composite.inc):
//     nothing mapped:   dim <= MHX_FAM_REG_MAX_DIM                                                             (32 fp64, 48 fp32)
//     otherwise:        2 dim + (components with a mapped parameter) + (blocks that carry a Z) / 2 <= 3 MHX_COND_REG_MAX_DIM
//                       (60 fp64, 96 fp32; the division rounds down)
// With everything mapped in one block it is the limit of mhx_cond_reg_body (20 / 32), with nothing mapped that of mhx_fam_reg_body.
// Measured by cross-compiling for gfx950 with the options of the run-time build, mapped components getting both parameters from two
// coordinates of their block.  "Cauchy" = Cauchy throughout (the worst family) in one static block; "own" = Cauchy throughout, every
// component a block of its own (static / walk); "mixed" = the seven families in turn, the kind alternating per component, every
// component a block of its own.  VGPRs (vector + accumulation, of 512) / bytes of scratch:
//   fp64  one block   d = 32, none mapped: Cauchy 457 / 0   d = 24, 12 mapped: 484 / 0   d = 20, all: 488 / 0
//                     d = 26, 8 mapped: 504 / 0     d = 28, 4: 502 / 0     d = 29, 2: 502 / 0     d = 29, 1: 492 / 0
//         own blocks  d = 17, all mapped: own 454 / 0 (static and walk), mixed (d = 15) 396 / 0     d = 22, 11 mapped: own 466 / 0
//                     d = 32, none mapped: mixed 404 / 0
//         rejected    one block: d = 25, 12 mapped: 512 / 44     d = 26, 13: 512 / 28     d = 30, 15: 512 / 316     d = 28, 8: 512 / 84
//                     d = 32, 2 mapped: 512 / 124 -- one mapped component ends the nothing-mapped regime
//                     own blocks: d = 20, all mapped: own 512 / 60 (static), 512 / 76 (walk) -- the Z pairs: the same shape in one
//                     block is clean;  still clean beyond the rule: d = 18, all mapped: own 478 / 0, d = 19: 506 / 0
//   fp32  one block   d = 48, none mapped: Cauchy 418 / 0   d = 38, 19 mapped: 449 / 0   d = 32, all: 449 / 0
//                     d = 44, 8 mapped: 465 / 0     d = 46, 4: 469 / 0     d = 47, 2: 470 / 0
//         own blocks  d = 27, all mapped: own 409 / 0 (static), 406 / 0 (walk)     d = 35, 17 mapped: own 415 / 0, 417 / 0
//                     d = 48, none mapped: mixed 350 / 0
//         rejected    one block: d = 44, 22 mapped: 512 / 36   (d = 40, 20 mapped is still clean, 473 / 0: the rule is the fp64 expression)
// A wider rule, dim + 2 mapped <= 3 MHX_COND_REG_MAX_DIM, admits the one-block shapes with scratch above.
// tests/test_composite_cpu.py compiles the limit with none, half and all of the components mapped, in one block and in blocks of
// their own, and the first shapes found to need scratch.
#define MHX_COMPOSITE_REG_COST_MAX (3 * MHX_COND_REG_MAX_DIM)

// bits of the device table of the state-in-HBM form: per component {kind bit, mapped mask}, per block {first, count, flags}
#define MHX_CMP_STATIC 1
#define MHX_CMP_SYMMETRIC 2

#ifdef MHX_HAVE_PROPOSAL_PARAMS
MHX_NS_BEGIN

// p(s) of the mapped entries: the table's constants, then the map; whether every mapped row is a distribution's (an unmapped row
// is a constant the host checked)
template <bool UNROLL, class FamOf, class MaskOf, class X, class Get, class Set>
MHX_DEV bool mhx_composite_eval(const int d, const FamOf& famof, const MaskOf& maskof, const mhx_fam_comp* __restrict__ fam, const X& s,
                                const Get& get, const Set& put, const mhx_real* __restrict__ cdata, const int ncdata)
{
    mhx_cond_for<UNROLL>(d, [&](const int k) { put(k, 0, fam[k].p[0]); put(k, 1, fam[k].p[1]); });
    mhx_user_proposal_params(s, mhx_cond_sink<FamOf, Set>{famof, put, d}, d, cdata, ncdata);
    const auto tab = mhx_cond_make_tab(famof, fam, get);
    bool ok = true;
    mhx_cond_for<UNROLL>(d, [&](const int k) {
        if (maskof(k) != 0) {
            const mhx_cond_row r = tab[k];
            ok = ok && mhx_fam_valid(famof(k), r.p);
        }
    });
    return ok;
}

// ---------------------------------------------------------------------------------------------
// state in HBM, run-time dimension.  pbuf: [4 dim][ld] as in mhx_cond_generic_body (only the mapped entries are used);
// ctab: int [2 dim + 3 nblocks]: {kind bit, mapped mask} per component, then {first, count, flags} per block
template <int TK>
MHX_DEV void mhx_composite_generic_body(const mhx_rwmh_args& a, const mhx_real* __restrict__ tparams, const mhx_fam_comp* __restrict__ fam,
                                        const mhx_real* __restrict__ cdata, const int ncdata, mhx_real* __restrict__ pbuf,
                                        const int* __restrict__ ctab, const int nblocks)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchains) return;
    const mhx_u64 id = a.first_chain + (mhx_u64)c;
    const mhx_u32 id_lo = (mhx_u32)id, id_hi = (mhx_u32)(id >> 32);
    const mhx_philox_key ks = mhx_philox_schedule(a.seed);
    const long ld = a.ld;
    const int d = a.dim;
    const int* btab = ctab + 2 * d;
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
    const auto maskof = [&](const int k) -> int { return ctab[2 * k + 1]; };
    const auto mapped = [&](const int k, const int j) -> bool { return ((ctab[2 * k + 1] >> j) & 1) != 0; };
    const auto getx = [&](const int k, const int j) -> mhx_real { return mapped(k, j) ? pxs[(long)(2 * k + j) * ld] : fam[k].p[j]; };
    const auto gety = [&](const int k, const int j) -> mhx_real { return mapped(k, j) ? pys[(long)(2 * k + j) * ld] : fam[k].p[j]; };
    const auto putx = [&](const int k, const int j, const mhx_real v) { if (mapped(k, j)) pxs[(long)(2 * k + j) * ld] = v; };
    const auto puty = [&](const int k, const int j, const mhx_real v) { if (mapped(k, j)) pys[(long)(2 * k + j) * ld] = v; };
    mhx_strided_x xv, yv;
    xv.base = xs; xv.ld = ld;
    yv.base = ys; yv.ld = ld;
    (void)mhx_composite_eval<false>(d, famof, maskof, fam, xv, getx, putx, cdata, ncdata);
    const auto tabx = mhx_cond_make_tab(famof, fam, getx);
    const auto taby = mhx_cond_make_tab(famof, fam, gety);

    for (int i = 0; i < a.nsteps; ++i) {
        const mhx_u32 step = a.step0 + (mhx_u32)i;
        mhx_fam_draw_all<false>(d, famof, tabx, ks, id_lo, id_hi, step, MHX_STREAM_PROPOSAL, MHX_STREAM_FAMILY,
                                [&](const int k, const mhx_real xi) { ys[(long)k * ld] = (ctab[2 * k] & MHX_CMP_STATIC) ? xi : xs[(long)k * ld] + xi; });
        const bool ok = mhx_composite_eval<false>(d, famof, maskof, fam, yv, gety, puty, cdata, ncdata);
        mhx_real ratio = MHX_R(0.0);
        bool any = false;
        for (int b = 0; b < nblocks; ++b) {
            const int first = btab[3 * b], count = btab[3 * b + 1], bf = btab[3 * b + 2];
            if (bf & MHX_CMP_SYMMETRIC) continue;
            const bool stat = (bf & MHX_CMP_STATIC) != 0;
            mhx_real kb = MHX_R(0.0), kf = MHX_R(0.0), zx = MHX_R(0.0), zy = MHX_R(0.0);
            bool withz = false;
            for (int k = first; k < first + count; ++k) {
                const mhx_real xk = xs[(long)k * ld], yk = ys[(long)k * ld];
                const mhx_cond_row rx = tabx[k], ry = taby[k];
                kb = kb + mhx_fam_logk(famof(k), ry.p, stat ? xk : xk - yk);
                kf = kf + mhx_fam_logk(famof(k), rx.p, stat ? yk : yk - xk);
                zx = zx + mhx_fam_lognorm(famof(k), rx.p);
                zy = zy + mhx_fam_lognorm(famof(k), ry.p);
                withz = withz || maskof(k) != 0;
            }
            const mhx_real rb = withz ? (kb - kf) + (zy - zx) : (kb - kf);
            ratio = any ? ratio + rb : rb;
            any = true;
        }
        const mhx_real lpy = mhx_target_eval<TK>(a.target_kind, yv, d, tparams, a.ntparams, a.tconst);
        const mhx_real logu = mhx_accept_logu(ks, id_lo, id_hi, step, ac);
        const mhx_real loga = any ? (lpy - lp) + ratio : (lpy - lp);
        const bool acc = ok && logu < loga;              // invalid p(y): rejected here; strict; NaN compares false => reject
        lp = acc ? lpy : lp;
        nacc += acc ? 1u : 0u;
        last = acc;
        wave_acc += (mhx_u32)__popcll(__ballot(acc));
        if (acc) {
            for (int k = 0; k < d; ++k) xs[(long)k * ld] = ys[(long)k * ld];
            for (int k = 0; k < d; ++k) {
                if (mapped(k, 0)) pxs[(long)(2 * k) * ld] = pys[(long)(2 * k) * ld];
                if (mapped(k, 1)) pxs[(long)(2 * k + 1) * ld] = pys[(long)(2 * k + 1) * ld];
            }
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

// p(x) of every chain's current state (after init / set_state), as mhx_cond_check_body: every chain whose mapped parameters are not
// a distribution's counts one in *nbad.  pbuf: [2 dim][ld] is enough
MHX_DEV void mhx_composite_check_body(const mhx_rwmh_args& a, const mhx_fam_comp* __restrict__ fam, const mhx_real* __restrict__ cdata,
                                      const int ncdata, mhx_real* __restrict__ pbuf, int* __restrict__ nbad, const int* __restrict__ ctab)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchains) return;
    const long ld = a.ld;
    mhx_real* pxs = pbuf + c;
    mhx_strided_x xv;
    xv.base = a.x + c;
    xv.ld = ld;
    const auto mapped = [&](const int k, const int j) -> bool { return ((ctab[2 * k + 1] >> j) & 1) != 0; };
    const bool ok = mhx_composite_eval<false>(
        a.dim, [&](const int k) -> int { return fam[k].family; }, [&](const int k) -> int { return ctab[2 * k + 1]; }, fam, xv,
        [&](const int k, const int j) -> mhx_real { return mapped(k, j) ? pxs[(long)(2 * k + j) * ld] : fam[k].p[j]; },
        [&](const int k, const int j, const mhx_real v) { if (mapped(k, j)) pxs[(long)(2 * k + j) * ld] = v; }, cdata, ncdata);
    if (!ok) atomicAdd(nbad, 1);
}

extern "C" __global__ void __launch_bounds__(256)
mhx_jit_composite_check(const mhx_rwmh_args a, const mhx_fam_comp* __restrict__ fam, const mhx_real* __restrict__ cdata, const int ncdata,
                        mhx_real* __restrict__ pbuf, int* __restrict__ nbad, const int* __restrict__ ctab)
{
    mhx_composite_check_body(a, fam, cdata, ncdata, pbuf, nbad, ctab);
}

// ---------------------------------------------------------------------------------------------
// state in registers, everything but the table's constants a compile-time constant
#ifdef MHX_JIT_COMPOSITE_REG
// f(mhx_ic<K>{}) for K = FROM .. TO - 1: the index is a constant expression inside f, so what depends on it is decided when the
// kernel is compiled and not left to the optimiser's loop folding
template <int K> struct mhx_ic { static constexpr int value = K; };
template <int FROM, int TO, class F>
MHX_DEV void mhx_static_for(const F& f)
{
    if constexpr (FROM < TO) {
        f(mhx_ic<FROM>{});
        mhx_static_for<FROM + 1, TO>(f);
    }
}

// the compile-time lists, one function each (a constexpr array local to a constexpr function folds in device code)
struct mhx_jit_cmp {
    static constexpr int D = MHX_JIT_DIM;
    MHX_DEV static constexpr int fam(const int k) { constexpr int l[] = {MHX_JIT_FAM_LIST}; static_assert(sizeof(l) / sizeof(l[0]) == D, "one family per component"); return l[k]; }
    // per component: 1 = its block is static
    MHX_DEV static constexpr int stat(const int k) { constexpr int l[] = {MHX_JIT_CMP_STATIC_LIST}; static_assert(sizeof(l) / sizeof(l[0]) == D, "one kind per component"); return l[k]; }
    // per component: its block, 0 .. NB - 1, non-decreasing
    MHX_DEV static constexpr int blk(const int k) { constexpr int l[] = {MHX_JIT_CMP_BLOCK_LIST}; static_assert(sizeof(l) / sizeof(l[0]) == D, "one block per component"); return l[k]; }
    // per component: bit j set = the map sets parameter j
    MHX_DEV static constexpr int mask(const int k) { constexpr int l[] = {MHX_JIT_CMP_MAPPED_LIST}; static_assert(sizeof(l) / sizeof(l[0]) == D, "one mask per component"); return l[k]; }
    // per block: 1 = declared symmetric
    MHX_DEV static constexpr int sym(const int b) { constexpr int l[] = {MHX_JIT_CMP_SYM_LIST}; return l[b]; }
    MHX_DEV static constexpr int nblocks() { constexpr int l[] = {MHX_JIT_CMP_SYM_LIST}; return (int)(sizeof(l) / sizeof(l[0])); }
    MHX_DEV static constexpr bool mapped(const int k, const int j) { return ((mask(k) >> j) & 1) != 0; }
    // whether block b carries a Z: not symmetric and some component mapped
    MHX_DEV static constexpr bool withz(const int b)
    {
        if (sym(b)) return false;
        for (int i = 0; i < D; ++i) if (blk(i) == b && mask(i) != 0) return true;
        return false;
    }
    MHX_DEV static constexpr bool any_nonsym()
    {
        for (int b = 0; b < nblocks(); ++b) if (!sym(b)) return true;
        return false;
    }
    MHX_DEV static constexpr bool first_nonsym(const int b)
    {
        for (int i = 0; i < b; ++i) if (!sym(i)) return false;
        return true;
    }
};

// Z_b of the blocks that carry one, from 0 in index order
template <class Tab, int NB>
MHX_DEV void mhx_composite_zsum(const Tab& tab, mhx_real (&Z)[NB])
{
    using J = mhx_jit_cmp;
    mhx_static_for<0, NB>([&](auto B) {
        constexpr int b = decltype(B)::value;
        if constexpr (J::withz(b)) Z[b] = MHX_R(0.0);
    });
    mhx_static_for<0, J::D>([&](auto K) {
        constexpr int k = decltype(K)::value, b = J::blk(k);
        if constexpr (J::withz(b)) Z[b] = Z[b] + mhx_fam_lognorm(J::fam(k), tab[k].p);
    });
}

template <int TK>
MHX_DEV void mhx_composite_reg_body(const mhx_rwmh_args& a, const mhx_real* __restrict__ tparams, const mhx_fam_comp* __restrict__ fam,
                                    const mhx_real* __restrict__ cdata, const int ncdata)
{
    using J = mhx_jit_cmp;
    constexpr int D = J::D, NB = J::nblocks();
    constexpr bool ANY_NONSYM = J::any_nonsym();
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchains) return;
    const mhx_u64 id = a.first_chain + (mhx_u64)c;
    const mhx_u32 id_lo = (mhx_u32)id, id_hi = (mhx_u32)(id >> 32);
    const mhx_philox_key ks = mhx_philox_schedule(a.seed);
    const long ld = a.ld;

    // (of px / py / Zx / Zy only the entries of mapped parameters and of blocks that carry a Z are ever touched: the others are no registers)
    mhx_real x[D], y[D], px[2 * D], py[2 * D], Zx[NB], Zy[NB];
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
    const auto famof = [](const int k) -> int { return J::fam(k); };
    const auto maskof = [](const int k) -> int { return J::mask(k); };
    const auto getx = [&](const int k, const int j) -> mhx_real { return J::mapped(k, j) ? px[2 * k + j] : fam[k].p[j]; };
    const auto gety = [&](const int k, const int j) -> mhx_real { return J::mapped(k, j) ? py[2 * k + j] : fam[k].p[j]; };
    const auto putx = [&](const int k, const int j, const mhx_real v) { if (J::mapped(k, j)) px[2 * k + j] = v; };
    const auto puty = [&](const int k, const int j, const mhx_real v) { if (J::mapped(k, j)) py[2 * k + j] = v; };
    const auto tabx = mhx_cond_make_tab(famof, fam, getx);
    const auto taby = mhx_cond_make_tab(famof, fam, gety);
    (void)mhx_composite_eval<true>(D, famof, maskof, fam, x, getx, putx, cdata, ncdata);
    mhx_composite_zsum(tabx, Zx);

    for (int i = 0; i < a.nsteps; ++i) {
        const mhx_u32 step = a.step0 + (mhx_u32)i;
        mhx_fam_draw_all<true>(D, famof, tabx, ks, id_lo, id_hi, step, MHX_STREAM_PROPOSAL, MHX_STREAM_FAMILY,
                               [&](const int k, const mhx_real xi) { y[k] = J::stat(k) ? xi : x[k] + xi; });
        const bool ok = mhx_composite_eval<true>(D, famof, maskof, fam, y, gety, puty, cdata, ncdata);
        mhx_composite_zsum(taby, Zy);
        mhx_real ratio = MHX_R(0.0), kb = MHX_R(0.0), kf = MHX_R(0.0);
        mhx_static_for<0, D>([&](auto K) {
            constexpr int k = decltype(K)::value, b = J::blk(k);
            if constexpr (!J::sym(b)) {
                if constexpr (k == 0 || J::blk(k > 0 ? k - 1 : 0) != b) kb = kf = MHX_R(0.0);                   // a block begins
                kb = kb + mhx_fam_logk(J::fam(k), taby[k].p, J::stat(k) ? x[k] : x[k] - y[k]);
                kf = kf + mhx_fam_logk(J::fam(k), tabx[k].p, J::stat(k) ? y[k] : y[k] - x[k]);
                if constexpr (k == D - 1 || J::blk(k < D - 1 ? k + 1 : k) != b) {                             // ... and ends
                    mhx_real rb = kb - kf;
                    if constexpr (J::withz(b)) rb = rb + (Zy[b] - Zx[b]);
                    if constexpr (J::first_nonsym(b)) ratio = rb; else ratio = ratio + rb;
                }
            }
        });
        const mhx_real lpy = mhx_target_eval<TK>(TK, y, D, tparams, a.ntparams, a.tconst);
        const mhx_real logu = mhx_accept_logu(ks, id_lo, id_hi, step, ac);
        const mhx_real loga = ANY_NONSYM ? (lpy - lp) + ratio : (lpy - lp);
        const bool acc = ok && logu < loga;              // invalid p(y): rejected here; strict; NaN compares false => reject
        // (fp64: a move under the execute mask, fp32: a select -- see mhx_rwmh_reg_body); the mapped entries only
        if (MHX_REAL64) {
            if (acc) {
#pragma unroll
                for (int k = 0; k < D; ++k) x[k] = y[k];
#pragma unroll
                for (int e = 0; e < 2 * D; ++e) if (J::mapped(e / 2, e % 2)) px[e] = py[e];
                mhx_static_for<0, NB>([&](auto B) {
                    constexpr int b = decltype(B)::value;
                    if constexpr (J::withz(b)) Zx[b] = Zy[b];
                });
            }
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) x[k] = acc ? y[k] : x[k];
#pragma unroll
            for (int e = 0; e < 2 * D; ++e) if (J::mapped(e / 2, e % 2)) px[e] = acc ? py[e] : px[e];
            mhx_static_for<0, NB>([&](auto B) {
                constexpr int b = decltype(B)::value;
                if constexpr (J::withz(b)) Zx[b] = acc ? Zy[b] : Zx[b];
            });
        }
        lp = acc ? lpy : lp;
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
mhx_jit_composite_reg(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_fam_comp* __restrict__ fam,
                      const mhx_real* __restrict__ cdata, const int ncdata)
{
    mhx_composite_reg_body<MHX_JIT_TK>(a, tparams, fam, cdata, ncdata);
}
#endif
#ifdef MHX_JIT_COMPOSITE_GENERIC
extern "C" __global__ void __launch_bounds__(256)
mhx_jit_composite_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_fam_comp* __restrict__ fam,
                          const mhx_real* __restrict__ cdata, const int ncdata, mhx_real* __restrict__ pbuf, const int* __restrict__ ctab,
                          const int nblocks)
{
    mhx_composite_generic_body<MHX_JIT_TK>(a, tparams, fam, cdata, ncdata, pbuf, ctab, nblocks);
}
#endif
MHX_NS_END
#endif
