// mhx_rwmh_tempered_kernels.h -- parallel tempering (replica exchange) of random-walk Metropolis-Hastings, one lane per chain.
//
// A run is `nladders` ladders of R rungs: chain c is rung r = c mod R of ladder c div R and samples pi^beta[r]
// with its own proposal scale; beta[0] = 1 is the chain that is read.  R is a power of two <= 64 and the first chain's id a multiple
// of R, so a ladder is R consecutive lanes of ONE wave and neighbouring temperatures exchange their states across lanes, inside the
// step kernel: no second kernel, no trip through memory, nothing to wait for but the wave itself.
//
//   transition    y = fma(sig[r], n, x) as the plain lane-per-chain kernels form it, accept iff logu < beta[r] * (lpy - lp)
//   swap round    after the accept / reject of every transition `step` with step % swap_every == 0; round s = step / swap_every (the
//                 GLOBAL step: a run advanced in two calls is the run advanced in one); pairs (r, r + 1) with r = s (mod 2); one
//                 Philox block per pair, keyed by the LOWER slot's chain id, step word s, stream MHX_STREAM_SWAP; swap iff
//                 logu_s < dbeta[r] * (lp[r + 1] - lp[r]); a swap exchanges x[0..d) and lp, nothing else.
// A slot keeps its temperature, its RNG streams and its accept counters; states move.  Both lanes of a pair evaluate the SAME
// expression on the SAME operands (lower slot's lp, upper slot's lp, the pair's dbeta and uniform), so they cannot disagree.
//
// Two kernels share the arithmetic, as mhx_rwmh_reg_body / mhx_rwmh_generic_body do:
//   mhx_tmp_reg_body<D, TK, PK, R>   run-time specialised, one wave per block; x[D] and y[D] in VGPRs for a whole launch, records
//                                    through SRD stores.  The exchange is in registers: even rounds pair lane ^ 1 (a DPP quad
//                                    permutation, one v_mov_b32_dpp per 32-bit word, in place), odd rounds lane +- 1 across the 16- and
//                                    32-lane rows (ds_bpermute_b32, one per word, in place), both under the execute mask of the lanes
//                                    that swap and skipped whole when none does.
//   mhx_tmp_generic_body             run-time dimension, state in HBM as [dim][nchains] plus ybuf, 256-thread blocks (whole ladders):
//                                    a lane exchange of lp, then each lane of a swapping pair hands its column over through registers.
// The tempering table `tt` (reals, built on the host): beta[R], dbeta[R] (dbeta[R - 1] unused, 0), then the proposal scales,
// sig[R] (ISO) or sig[R][dim] (DIAG).  `swapc`: [2][nchains] u32, attempts then swaps of pair (r, r + 1), kept by the lower slot.
// Both bodies have an ADAPT variant (a template bool; MHX_JIT_ADAPT for the run-time kernels) in which every ladder tunes its
// temperatures from its own swap rounds: see mhx_tmp_adapt below.  With ADAPT false nothing of it is compiled in.
// ... and an ANCHOR variant (a template bool; MHX_JIT_ANCHOR) in which rung r samples target^beta[r] * q^(1 - beta[r]) for a normalised
// reference density q, so that beta = 0 is a legal last rung and the ladder carries the evidence: see mhx_tmp_anchor below.  With
// ANCHOR false nothing of it is compiled in either.
#pragma once
#include "mhx_rwmh_kernels.h"

MHX_NS_BEGIN

// stream tag of the swap uniforms: 0 .. 3 are the older streams, 4 .. 7 their retry twins, 8 .. 10 and 12 .. 14 the family streams
#define MHX_STREAM_SWAP 11u

// Largest dimension the register form is built for: x[D], y[D] and the temporaries of the unrolled candidate loop (DIAG: the lane's
// own scales too, which the compiler hoists out of the step loop) must fit 512 VGPRs without scratch memory.  Measured by
// cross-compiling for gfx950 with the options of the run-time build, isotropic Gaussian target, R = 64, ISO and DIAG: fp64 clean at
// 48 (DIAG: all 512 registers), scratch at 52 and 56 (DIAG; ISO is clean at 56 and spills at 64); fp32 clean at 72 and 80, scratch
// at 88 (DIAG; ISO is clean at 96 and spills at 128).  tests/test_tempered_cpu.py compiles the kernel at the limit and at the next
// size tried.  Above it the state-in-HBM form runs.  The adaptive variant (below) holds the limit too: it keeps no per-lane scales
// (DIAG: 460 registers in fp64, 433 in fp32) and a few more reals of its own (ISO: 452 / 426); tests/test_tempered_adaptive_cpu.py.
#define MHX_TEMPERED_REG_MAX_DIM (MHX_REAL64 ? 48 : 80)
// ... and of the anchored variant (below), which carries lq and forms lqy beside the target's own value.  Measured the same way:
// fp64 clean at 44 (DIAG: 496 registers; 460 at 40), scratch at 48 (DIAG, 84 bytes; ISO is clean there with 442); fp32 clean at 76
// (DIAG: 501; 479 at 72), scratch at 80 (DIAG, 44 bytes; ISO is clean with 445).  tests/test_tempered_anchored_cpu.py compiles both.
#define MHX_TEMPERED_ANCHORED_REG_MAX_DIM (MHX_REAL64 ? 44 : 76)

// ---------------------------------------------------------------------------------------------
// An anchored ladder: rung r samples target^beta[r] * q^(1 - beta[r]), q a diagonal Gaussian of known
// normaliser, so the last rung may sit at beta = 0 (it samples q, restricted to the target's support) and the path from beta = 1 to 0
// integrates to the log evidence (mhx_evidence_kernels.h).  Everything here is wave-uniform: a lane keeps of it only omb of its rung
// and lq of its state.  Built on the host: w[k] = 1 / sd[k] and m[k], rounded once; lc = -sum log sd[k] - (d / 2) log 2 pi in double,
// rounded once; omb[r] = 1 - beta[r] of the rounded betas.
struct mhx_tmp_anchor {
    const mhx_real* m;           // [dim] the reference's mean
    const mhx_real* w;           // [dim] 1 / sd
    const mhx_real* omb;         // [R] 1 - beta
    mhx_real lc;                 // the log of the reference's normaliser
};
// log q(x): z = (x[k] - m[k]) * w[k], acc = fma(z, z, acc) for k ascending from 0, lq = fma(-0.5, acc, lc).  A pure function of the
// state: the step kernels recompute it at the start of every launch, the evidence sweep per draw.  d: the loop's extent (a constant
// where x is a register array).
template <class X>
MHX_DEV mhx_real mhx_tmp_logq(const X& x, const int d, const mhx_tmp_anchor& an)
{
    mhx_real acc = MHX_R(0.0);
#pragma unroll
    for (int k = 0; k < d; ++k) {
        const mhx_real z = (x[k] - an.m[k]) * an.w[k];
        acc = mhx_fma(z, z, acc);
    }
    return mhx_fma(MHX_R(-0.5), acc, an.lc);
}
// what a lane of an anchored ladder carries through a launch; nothing where the ladder is not anchored
template <bool ANCHOR>
struct mhx_tmp_lq {};
template <>
struct mhx_tmp_lq<true> {
    mhx_real lq;                 // log q of the state
    mhx_real lqy;                // ... of the candidate
    mhx_real omb;                // 1 - beta of the lane's rung
};
// the log acceptance ratio from its target part `b` = beta * (lpy - lp): two products and one sum.  beta = 1: + 0, the plain chain's
// bits; beta = 0 and a candidate outside the target's support: 0 * (-inf) = NaN, a reject.
MHX_DEV mhx_real mhx_tmp_loga(const mhx_real b, const mhx_tmp_lq<false>&) { return b; }
MHX_DEV mhx_real mhx_tmp_loga(const mhx_real b, const mhx_tmp_lq<true>& q) { return b + q.omb * (q.lqy - q.lq); }
// what the swap round compares: lp, or u = lp - lq
MHX_DEV mhx_real mhx_tmp_swap_u(const mhx_real lp, const mhx_tmp_lq<false>&) { return lp; }
MHX_DEV mhx_real mhx_tmp_swap_u(const mhx_real lp, const mhx_tmp_lq<true>& q) { return lp - q.lq; }

// the value of `v` in lane (lane ^ 1): a quad permutation [1, 0, 3, 2]
MHX_DEV mhx_u32 mhx_tmp_xor1_u32(const mhx_u32 v)
{
    return (mhx_u32)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false);
}
// the value of `v` in the lane whose byte address (4 * lane) is `paddr`
MHX_DEV mhx_u32 mhx_tmp_perm_u32(const int paddr, const mhx_u32 v) { return (mhx_u32)__builtin_amdgcn_ds_bpermute(paddr, (int)v); }

template <bool EVEN>
MHX_DEV mhx_real mhx_tmp_partner(const mhx_real v, const int paddr)
{
#if MHX_REAL64
    const mhx_u64 b = (mhx_u64)__double_as_longlong(v);
    mhx_u32 lo = (mhx_u32)b, hi = (mhx_u32)(b >> 32);
    if constexpr (EVEN) { lo = mhx_tmp_xor1_u32(lo); hi = mhx_tmp_xor1_u32(hi); }
    else { lo = mhx_tmp_perm_u32(paddr, lo); hi = mhx_tmp_perm_u32(paddr, hi); }
    return __longlong_as_double((long long)(((mhx_u64)hi << 32) | (mhx_u64)lo));
#else
    const mhx_u32 b = __float_as_uint(v);
    return __uint_as_float(EVEN ? mhx_tmp_xor1_u32(b) : mhx_tmp_perm_u32(paddr, b));
#endif
}

// What a lane knows of its place in the ladder, fixed for a launch (an adaptive ladder: the place is, beta and dbeta move)
struct mhx_tmp_lane {
    int r;              // rung
    int paddr_odd;      // byte address of the odd rounds' partner lane (the lane itself where it has none)
    bool low_odd;       // odd rounds: the lower slot of a pair
    bool pair_odd;      // odd rounds: in a pair at all (rungs 0 and R - 1 are not)
    mhx_real beta;
    mhx_real db_even;   // dbeta of the even rounds' pair, of the odd rounds' pair
    mhx_real db_odd;
};

template <bool ADAPT = false>
MHX_DEV mhx_tmp_lane mhx_tmp_lane_of(const int c, const int R, const mhx_real* __restrict__ tt)
{
    mhx_tmp_lane t;
    const int lane = (int)(threadIdx.x & 63u);
    t.r = c & (R - 1);
    t.low_odd = (t.r & 1) != 0 && t.r + 1 < R;
    const bool up_odd = (t.r & 1) == 0 && t.r >= 2;
    t.pair_odd = t.low_odd || up_odd;
    t.paddr_odd = 4 * (t.low_odd ? lane + 1 : (up_odd ? lane - 1 : lane));
    if constexpr (!ADAPT) {                                         // (an adaptive ladder has no table: mhx_tmp_derive fills these)
        t.beta = tt[t.r];
        t.db_even = tt[R + (t.r & ~1)];
        t.db_odd = tt[R + (t.low_odd ? t.r : (up_odd ? t.r - 1 : 0))];
    } else t.beta = t.db_even = t.db_odd = MHX_R(0.0);
    return t;
}

// The decision of swap round `s` for this lane's pair: true in BOTH lanes of a pair that swaps, false elsewhere.  `plp` receives the
// partner's lp, `logs` the log of the pair's swap ratio (the same value in both lanes).  attempts / swaps: the lower slot's counters.
// An anchored ladder passes u = lp - lq for lp: the ratio is of u, and `plp` receives the partner's u (the same one subtraction of the
// partner's own lp and lq, whichever lane makes it); the lanes that swap fetch lp and lq themselves afterwards.
template <bool EVEN>
MHX_DEV bool mhx_tmp_decide(const mhx_tmp_lane& t, const mhx_philox_key& ks, const mhx_u64 id, const mhx_u32 s, const mhx_real lp,
                            mhx_real& plp, mhx_u32& attempts, mhx_u32& swaps, mhx_real& logs)
{
    const bool low = EVEN ? (t.r & 1) == 0 : t.low_odd;
    const bool paired = EVEN ? true : t.pair_odd;
    plp = mhx_tmp_partner<EVEN>(lp, t.paddr_odd);
    const mhx_u64 idl = low ? id : id - 1ull;                       // the pair's uniform is keyed by its lower slot
    const mhx_u32x4 w = mhx_philox(ks, (mhx_u32)idl, (mhx_u32)(idl >> 32), s, MHX_STREAM_SWAP << 28);
    const mhx_real logu = mhx_log_pos(mhx_fam_u_open(w));           // words (x, y) in fp64, word x in fp32: as mhx_accept_logu's even steps
    const mhx_real lp_lo = low ? lp : plp, lp_hi = low ? plp : lp;
    logs = (EVEN ? t.db_even : t.db_odd) * (lp_hi - lp_lo);
    const bool sw = paired && (logu < logs);                        // strict; NaN compares false => no swap
    attempts += (paired && low) ? 1u : 0u;
    swaps += (sw && low) ? 1u : 0u;
    return sw;
}

// ---------------------------------------------------------------------------------------------
// An adaptive ladder: every ladder tunes its own temperatures from its own swaps while the run warms up.
// The ladder is parametrised by rho[r], the log of the gap of pair (r, r + 1) in log beta, kept by the pair's lower slot;
//   h[r] = sum_{q < r} exp(rho[q]),   beta[r] = exp(-h[r]),   proposal scale s[r] = exp(h[r] / 2) = beta[r]^(-1/2),   beta[0] = s[0] = 1
// and after swap round s <= nrounds every attempted pair moves rho by gamma[s] * (min(1, swap ratio) - target_rate), clamped.
// The sum is an inclusive Hillis-Steele scan over the R lanes of the ladder, in the order the spec fixes: for off = 1, 2, 4, .. < R
// every lane with r >= off adds the value of lane r - off.  A lane that adds has r >= off, so the lane it reads is a rung of ITS OWN
// ladder: nothing leaks between two ladders of a wave, and a lane of a ladder is never read by a lane of another.
struct mhx_tmp_adapt {
    mhx_real* rho;               // [ld] rho of pair (r, r + 1) at its lower slot (slot R - 1: unused, 0)
    mhx_real* beta;              // [ld] the slot's temperature, written at the end of every launch (mhx_run_ladder_betas)
    const mhx_real* gamma;       // [nrounds] step size of swap round s at gamma[s - 1]
    const mhx_real* sigk;        // DIAG: sigma_k [dim] (wave-uniform); ISO: unused
    mhx_real sigma;              // ISO: the proposal's scale
    mhx_real target_rate, rho_min, rho_max;
    mhx_u32 nrounds;             // swap rounds 1 .. nrounds adapt (adapt_steps / swap_every)
};

// the value of `v` in lane (lane - OFF).  ROW (a ladder inside a 16-lane row, OFF < 16): a DPP row shift, one v_mov_b32_dpp per
// 32-bit word; lanes it has no source for keep their own value, which no caller uses.  Otherwise ds_bpermute_b32: the source may
// lie in the row, or the 32-lane half, below.
template <int OFF, bool ROW>
MHX_DEV mhx_u32 mhx_tmp_below_u32(const mhx_u32 v, const int lane)
{
    if constexpr (ROW) return (mhx_u32)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x110 + OFF, 0xF, 0xF, false);      // row_shr:OFF
    else return mhx_tmp_perm_u32(4 * ((lane - OFF) & 63), v);
}
template <int OFF, bool ROW>
MHX_DEV mhx_real mhx_tmp_below(const mhx_real v, const int lane)
{
#if MHX_REAL64
    const mhx_u64 b = (mhx_u64)__double_as_longlong(v);
    const mhx_u32 lo = mhx_tmp_below_u32<OFF, ROW>((mhx_u32)b, lane), hi = mhx_tmp_below_u32<OFF, ROW>((mhx_u32)(b >> 32), lane);
    return __longlong_as_double((long long)(((mhx_u64)hi << 32) | (mhx_u64)lo));
#else
    return __uint_as_float(mhx_tmp_below_u32<OFF, ROW>(__float_as_uint(v), lane));
#endif
}
// one step of the scan.  R is the ladder's size where it is a compile-time constant (the register form), else 0 (rr: its value)
template <int OFF, int R>
MHX_DEV mhx_real mhx_tmp_scan_step(const mhx_real h, const int r, const int rr, const int lane)
{
    if (R ? OFF >= R : OFF >= rr) return h;
    const mhx_real below = mhx_tmp_below<OFF, (R != 0 && R <= 16)>(h, lane);
    return r >= OFF ? h + below : h;
}

// The lane's temperature, its pairs' dbeta and its proposal scale `sc` from the ladder's rho.  Every live lane of the wave calls it
// together (whole ladders; the callers' branches are wave-uniform).
template <int R>
MHX_DEV void mhx_tmp_derive(mhx_tmp_lane& t, const mhx_real rho, const int rr, mhx_real& sc)
{
    const int lane = (int)(threadIdx.x & 63u);
    const mhx_real g = mhx_exp(rho);
    const mhx_real gb = mhx_tmp_below<1, (R != 0 && R <= 16)>(g, lane);
    mhx_real h = t.r >= 1 ? gb : MHX_R(0.0);
    h = mhx_tmp_scan_step<1, R>(h, t.r, rr, lane);
    h = mhx_tmp_scan_step<2, R>(h, t.r, rr, lane);
    h = mhx_tmp_scan_step<4, R>(h, t.r, rr, lane);
    h = mhx_tmp_scan_step<8, R>(h, t.r, rr, lane);
    h = mhx_tmp_scan_step<16, R>(h, t.r, rr, lane);
    h = mhx_tmp_scan_step<32, R>(h, t.r, rr, lane);
    const mhx_real b = mhx_exp(-h), s = mhx_exp(MHX_R(0.5) * h);
    t.beta = t.r ? b : MHX_R(1.0);                                  // rung 0 by definition, not computed
    sc = t.r ? s : MHX_R(1.0);
    // dbeta = beta_lo - beta_hi: the same one subtraction in both lanes of a pair (a lane without an odd pair reads itself: 0, unused)
    const mhx_real pe = mhx_tmp_partner<true>(t.beta, t.paddr_odd), po = mhx_tmp_partner<false>(t.beta, t.paddr_odd);
    t.db_even = (t.r & 1) == 0 ? t.beta - pe : pe - t.beta;
    t.db_odd = t.low_odd ? t.beta - po : po - t.beta;
}

// After swap round `s`: the lower slot of an attempted pair (`low`) moves its rho; then the ladder is derived again.
template <int R>
MHX_DEV void mhx_tmp_adapt_round(mhx_tmp_lane& t, const mhx_tmp_adapt& ad, const mhx_u32 s, const bool low, const mhx_real logs,
                                 const int rr, mhx_real& rho, mhx_real& sc)
{
    const mhx_real gam = ad.gamma[s - 1u];                          // wave-uniform
    const mhx_real acc = logs >= MHX_R(0.0) ? MHX_R(1.0) : mhx_exp(logs);
    mhx_real nr = rho + gam * (acc - ad.target_rate);
    nr = nr < ad.rho_min ? ad.rho_min : (nr > ad.rho_max ? ad.rho_max : nr);
    rho = (low && logs == logs) ? nr : rho;                         // (a NaN ratio leaves the pair's rho alone)
    mhx_tmp_derive<R>(t, rho, rr, sc);
}

// ---------------------------------------------------------------------------------------------
// state in HBM, run-time dimension
// ADAPT: an adaptive ladder -- `ad` in place of the table `tt` (each is NULL where the other is read)
// ANCHOR: an anchored ladder -- the table and `an` (fixed ladders only)
template <int TK, bool ADAPT = false, bool ANCHOR = false>
MHX_DEV void mhx_tmp_generic_body(const mhx_rwmh_args& a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ tt,
                                  mhx_u32* __restrict__ swapc, const int swap_every, const int R, const mhx_tmp_adapt* ad = nullptr,
                                  const mhx_tmp_anchor* an = nullptr)
{
    static_assert(!(ADAPT && ANCHOR), "an anchored ladder is a fixed ladder");
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchains) return;                                     // (whole ladders leave together: nchains is a multiple of R)
    const mhx_u64 id = a.first_chain + (mhx_u64)c;
    const mhx_u32 id_lo = (mhx_u32)id, id_hi = (mhx_u32)(id >> 32);
    const mhx_philox_key ks = mhx_philox_schedule(a.seed);
    const long ld = a.ld;
    const int d = a.dim;
    mhx_real* xs = a.x + c;
    mhx_real* ys = a.ybuf + c;
    mhx_tmp_lane t = mhx_tmp_lane_of<ADAPT>(c, R, tt);            // (ADAPT: beta and dbeta move with the ladder)
    const bool iso = a.prop_kind == MHX_PROP_ISO;
    const mhx_real* sig = ADAPT ? nullptr : tt + 2 * R + (iso ? (long)t.r : (long)t.r * d);
    mhx_real rho = MHX_R(0.0), sc = MHX_R(1.0);                      // ADAPT: the pair's rho, the rung's proposal scale s[r]
    if constexpr (ADAPT) {
        rho = ad->rho[c];
        mhx_tmp_derive<0>(t, rho, R, sc);
    }

    mhx_real lp = a.lp[c];
    mhx_tmp_lq<ANCHOR> q;                                            // ANCHOR: log q of the state, recomputed (no state of its own is kept)
    if constexpr (ANCHOR) {
        mhx_strided_x xv;
        xv.base = xs;
        xv.ld = ld;
        q.lq = mhx_tmp_logq(xv, d, *an);
        q.omb = an->omb[t.r];
    }
    mhx_u32 nacc = a.acc_count[c];
    mhx_u32 wave_acc = 0;
    bool last = a.last_acc[c] != 0;
    mhx_u32 attempts = swapc[c], swaps = swapc[ld + c];
    mhx_accept_cache ac;
    ac.group = 0xffffffffu;
    ac.w.x = ac.w.y = ac.w.z = ac.w.w = 0u;
    mhx_u32 save_next = a.save_next;
    long slot = a.save_slot;
    const int nblk = (d + 3) >> 2;
    mhx_u32 swap_next = 0xffffffffu;                                 // the next step with a swap round
    mhx_u32 sround = 0u;                                             // ... and its round number, step / swap_every of the GLOBAL step
    if (swap_every > 0) {
        sround = (a.step0 + (mhx_u32)swap_every - 1u) / (mhx_u32)swap_every;
        swap_next = sround * (mhx_u32)swap_every;
    }

    for (int i = 0; i < a.nsteps; ++i) {
        const mhx_u32 step = a.step0 + (mhx_u32)i;
        for (int b = 0; b < nblk; ++b) {
            mhx_real n[4];
            mhx_normal4(ks, id_lo, id_hi, step, MHX_STREAM_PROPOSAL, (mhx_u32)b, n);
            for (int j = 0; j < 4; ++j) {
                const int k = 4 * b + j;
                if (k < d) {
                    mhx_real sg;
                    if constexpr (ADAPT) sg = sc * (iso ? ad->sigma : ad->sigk[k]);
                    else sg = iso ? sig[0] : sig[k];
                    ys[(long)k * ld] = mhx_fma(sg, n[j], xs[(long)k * ld]);
                }
            }
        }
        mhx_strided_x yv;
        yv.base = ys;
        yv.ld = ld;
        const mhx_real lpy = mhx_target_eval<TK>(a.target_kind, yv, d, tparams, a.ntparams, a.tconst);
        const mhx_real logu = mhx_accept_logu(ks, id_lo, id_hi, step, ac);
        if constexpr (ANCHOR) q.lqy = mhx_tmp_logq(yv, d, *an);
        const mhx_real loga = mhx_tmp_loga(t.beta * (lpy - lp), q);
        const bool acc = logu < loga;                    // strict; NaN compares false => reject
        lp = acc ? lpy : lp;
        if constexpr (ANCHOR) q.lq = acc ? q.lqy : q.lq;
        nacc += acc ? 1u : 0u;
        last = acc;
        wave_acc += (mhx_u32)__popcll(__ballot(acc));
        if (acc) {
            for (int k = 0; k < d; ++k) xs[(long)k * ld] = ys[(long)k * ld];
        }
        if (step == swap_next) {                         // wave-uniform
            const mhx_u32 s = sround++;
            mhx_real plp, logs;
            if ((s & 1u) == 0u) {
                const bool sw = mhx_tmp_decide<true>(t, ks, id, s, mhx_tmp_swap_u(lp, q), plp, attempts, swaps, logs);
                if (__ballot(sw) != 0ull) {
                    for (int k = 0; k < d; ++k) {
                        const mhx_real mine = xs[(long)k * ld];
                        const mhx_real theirs = mhx_tmp_partner<true>(mine, t.paddr_odd);
                        if (sw) xs[(long)k * ld] = theirs;
                    }
                    if constexpr (ANCHOR) {             // (plp is the partner's u)
                        plp = mhx_tmp_partner<true>(lp, t.paddr_odd);
                        const mhx_real plq = mhx_tmp_partner<true>(q.lq, t.paddr_odd);
                        q.lq = sw ? plq : q.lq;
                    }
                    lp = sw ? plp : lp;
                }
            } else {
                const bool sw = mhx_tmp_decide<false>(t, ks, id, s, mhx_tmp_swap_u(lp, q), plp, attempts, swaps, logs);
                if (__ballot(sw) != 0ull) {
                    for (int k = 0; k < d; ++k) {
                        const mhx_real mine = xs[(long)k * ld];
                        const mhx_real theirs = mhx_tmp_partner<false>(mine, t.paddr_odd);
                        if (sw) xs[(long)k * ld] = theirs;
                    }
                    if constexpr (ANCHOR) {             // (plp is the partner's u)
                        plp = mhx_tmp_partner<false>(lp, t.paddr_odd);
                        const mhx_real plq = mhx_tmp_partner<false>(q.lq, t.paddr_odd);
                        q.lq = sw ? plq : q.lq;
                    }
                    lp = sw ? plp : lp;
                }
            }
            if constexpr (ADAPT) {
                if (s >= 1u && s <= ad->nrounds)         // wave-uniform; the new ladder applies from the next transition
                    mhx_tmp_adapt_round<0>(t, *ad, s, (s & 1u) == 0u ? (t.r & 1) == 0 : t.low_odd, logs, R, rho, sc);
            }
            swap_next += (mhx_u32)swap_every;
        }
        if (step == save_next) {                         // the state after the step's swap round
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
    swapc[c] = attempts;
    swapc[ld + c] = swaps;
    if constexpr (ADAPT) {
        ad->rho[c] = rho;
        ad->beta[c] = t.beta;
    }
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
        atomicAdd(a.acc_total, (mhx_u64)wave_acc);
}

// the ladder of every slot from its rho, outside a step launch (after create and init: mhx_run_ladder_betas reads ad.beta)
MHX_DEV void mhx_tmp_derive_body(const mhx_tmp_adapt& ad, const int nchains, const int R)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchains) return;                                       // (whole ladders leave together)
    mhx_tmp_lane t = mhx_tmp_lane_of<true>(c, R, nullptr);
    mhx_real sc;
    mhx_tmp_derive<0>(t, ad.rho[c], R, sc);
    ad.beta[c] = t.beta;
}

// column r, r + R, r + 2R, ... of a [N][d1][C] sample tensor as a [N][d1][C / R] tensor (mhx_run_rung)
MHX_DEV void mhx_tmp_rung_body(const mhx_real* __restrict__ src, mhx_real* __restrict__ dst, const long rows, const long C, const int R, const int r)
{
    const long L = C / R;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * L) return;
    const long row = i / L, l = i - row * L;
    dst[i] = src[row * C + l * R + r];
}

// ---------------------------------------------------------------------------------------------
// state in registers; dimension, target, proposal kind and ladder size compile-time constants
#ifdef MHX_JIT_TEMPERED_REG
template <int D, int TK, int PK, int R, bool ADAPT = false, bool ANCHOR = false>
MHX_DEV void mhx_tmp_reg_body(const mhx_rwmh_args& a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ tt,
                              mhx_u32* __restrict__ swapc, const int swap_every, const mhx_tmp_adapt* ad = nullptr,
                              const mhx_tmp_anchor* an = nullptr)
{
    static_assert(!(ADAPT && ANCHOR), "an anchored ladder is a fixed ladder");
    static_assert(R >= 2 && R <= 64 && (R & (R - 1)) == 0, "a ladder is a power of two of lanes of one wave");
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchains) return;                                     // (whole ladders leave together: nchains is a multiple of R)
    const mhx_u64 id = a.first_chain + (mhx_u64)c;
    const mhx_u32 id_lo = (mhx_u32)id, id_hi = (mhx_u32)(id >> 32);
    const mhx_philox_key ks = mhx_philox_schedule(a.seed);
    const long ld = a.ld;
    mhx_tmp_lane t = mhx_tmp_lane_of<ADAPT>(c, R, tt);            // (ADAPT: beta and dbeta move with the ladder)
    const mhx_real* sig = ADAPT ? nullptr : tt + 2 * R + (PK == MHX_PROP_ISO ? t.r : t.r * D);
    mhx_real rho = MHX_R(0.0), sc = MHX_R(1.0);                      // ADAPT: the pair's rho, the rung's proposal scale s[r]
    if constexpr (ADAPT) {
        rho = ad->rho[c];
        mhx_tmp_derive<R>(t, rho, R, sc);
    }
    // (ADAPT, DIAG: sigma_k is wave-uniform and multiplied in at every use -- the lane holds no scales of its own in VGPRs)
    const mhx_real sig0 = ADAPT ? MHX_R(0.0) : sig[0];

    mhx_real x[D], y[D];
    const mhx_u32 cu = (mhx_u32)c * MHX_RB;  // row pointers are wave-uniform (scalar), the lane adds its byte offset
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = mhx_ld_off(a.x + (long)k * ld, cu);
    mhx_real lp = a.lp[c];
    mhx_tmp_lq<ANCHOR> q;                                            // ANCHOR: log q of the state, recomputed (no state of its own is kept)
    if constexpr (ANCHOR) {
        q.lq = mhx_tmp_logq(x, D, *an);
        q.omb = an->omb[t.r];
    }
    mhx_u32 nacc = a.acc_count[c];
    mhx_u32 wave_acc = 0;
    bool last = a.last_acc[c] != 0;
    mhx_u32 attempts = swapc[c], swaps = swapc[ld + c];
    mhx_accept_cache ac;
    ac.group = 0xffffffffu;
    ac.w.x = ac.w.y = ac.w.z = ac.w.w = 0u;
    mhx_u32 save_next = a.save_next;
    long slot = a.save_slot;
    mhx_u32 swap_next = 0xffffffffu;                                 // the next step with a swap round
    mhx_u32 sround = 0u;                                             // ... and its round number, step / swap_every of the GLOBAL step
    if (swap_every > 0) {
        sround = (a.step0 + (mhx_u32)swap_every - 1u) / (mhx_u32)swap_every;
        swap_next = sround * (mhx_u32)swap_every;
    }

    for (int i = 0; i < a.nsteps; ++i) {
        const mhx_u32 step = a.step0 + (mhx_u32)i;
#pragma unroll
        for (int b = 0; b < (D + 3) / 4; ++b) {
            mhx_real n[4];
            mhx_normal4(ks, id_lo, id_hi, step, MHX_STREAM_PROPOSAL, (mhx_u32)b, n);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 4 * b + j;
                if (k < D) {
                    mhx_real sg;
                    if constexpr (ADAPT) sg = sc * (PK == MHX_PROP_ISO ? ad->sigma : ad->sigk[k]);
                    else sg = PK == MHX_PROP_ISO ? sig0 : sig[k];
                    y[k] = mhx_fma(sg, n[j], x[k]);
                }
            }
        }
        const mhx_real lpy = mhx_target_eval<TK>(TK, y, D, tparams, a.ntparams, a.tconst);
        const mhx_real logu = mhx_accept_logu(ks, id_lo, id_hi, step, ac);
        if constexpr (ANCHOR) q.lqy = mhx_tmp_logq(y, D, *an);
        const mhx_real loga = mhx_tmp_loga(t.beta * (lpy - lp), q);
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
        if constexpr (ANCHOR) q.lq = acc ? q.lqy : q.lq;
        nacc += acc ? 1u : 0u;
        last = acc;
        wave_acc += (mhx_u32)__popcll(__ballot(acc));
        if (step == swap_next) {                         // wave-uniform
            const mhx_u32 s = sround++;
            mhx_real plp, logs = MHX_R(0.0);
            // the exchange runs under the execute mask of the lanes that swap -- both lanes of a pair, by construction -- and in place:
            // y is dead here, but not even it is needed
            if ((s & 1u) == 0u) {
                const bool sw = mhx_tmp_decide<true>(t, ks, id, s, mhx_tmp_swap_u(lp, q), plp, attempts, swaps, logs);
                if (__ballot(sw) != 0ull) {
                    if (sw) {
#pragma unroll
                        for (int k = 0; k < D; ++k) x[k] = mhx_tmp_partner<true>(x[k], t.paddr_odd);
                        if constexpr (ANCHOR) {         // (plp is the partner's u)
                            plp = mhx_tmp_partner<true>(lp, t.paddr_odd);
                            q.lq = mhx_tmp_partner<true>(q.lq, t.paddr_odd);
                        }
                        lp = plp;
                    }
                }
            } else if (R > 2) {                          // (R = 2: the odd rounds have no pair)
                const bool sw = mhx_tmp_decide<false>(t, ks, id, s, mhx_tmp_swap_u(lp, q), plp, attempts, swaps, logs);
                if (__ballot(sw) != 0ull) {
                    if (sw) {
#pragma unroll
                        for (int k = 0; k < D; ++k) x[k] = mhx_tmp_partner<false>(x[k], t.paddr_odd);
                        if constexpr (ANCHOR) {         // (plp is the partner's u)
                            plp = mhx_tmp_partner<false>(lp, t.paddr_odd);
                            q.lq = mhx_tmp_partner<false>(q.lq, t.paddr_odd);
                        }
                        lp = plp;
                    }
                }
            }
            if constexpr (ADAPT) {
                if (s >= 1u && s <= ad->nrounds)         // wave-uniform; the new ladder applies from the next transition
                    mhx_tmp_adapt_round<R>(t, *ad, s, (s & 1u) == 0u ? (t.r & 1) == 0 : (R > 2 && t.low_odd), logs, R, rho, sc);
            }
            swap_next += (mhx_u32)swap_every;
        }
        if (step == save_next) {                         // the state after the step's swap round
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
    swapc[c] = attempts;
    swapc[ld + c] = swaps;
    if constexpr (ADAPT) {
        ad->rho[c] = rho;
        ad->beta[c] = t.beta;
    }
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
        atomicAdd(a.acc_total, (mhx_u64)wave_acc);
}

#if defined(MHX_JIT_ANCHOR)
extern "C" __global__ void __launch_bounds__(64)
mhx_jit_tempered_anchored_reg(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ tt,
                              mhx_u32* __restrict__ swapc, const int swap_every, const mhx_tmp_anchor an)
{
    mhx_tmp_reg_body<MHX_JIT_DIM, MHX_JIT_TK, MHX_JIT_PK, MHX_JIT_R, false, true>(a, tparams, tt, swapc, swap_every, nullptr, &an);
}
#elif defined(MHX_JIT_ADAPT)
extern "C" __global__ void __launch_bounds__(64)
mhx_jit_tempered_adapt_reg(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_tmp_adapt ad,
                           mhx_u32* __restrict__ swapc, const int swap_every)
{
    mhx_tmp_reg_body<MHX_JIT_DIM, MHX_JIT_TK, MHX_JIT_PK, MHX_JIT_R, true>(a, tparams, nullptr, swapc, swap_every, &ad);
}
#else
extern "C" __global__ void __launch_bounds__(64)
mhx_jit_tempered_reg(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ tt,
                     mhx_u32* __restrict__ swapc, const int swap_every)
{
    mhx_tmp_reg_body<MHX_JIT_DIM, MHX_JIT_TK, MHX_JIT_PK, MHX_JIT_R>(a, tparams, tt, swapc, swap_every);
}
#endif
#endif
#if defined(MHX_JIT_TEMPERED_GENERIC) && defined(MHX_JIT_ANCHOR)
extern "C" __global__ void __launch_bounds__(256)
mhx_jit_tempered_anchored_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ tt,
                                  mhx_u32* __restrict__ swapc, const int swap_every, const int R, const mhx_tmp_anchor an)
{
    mhx_tmp_generic_body<MHX_JIT_TK, false, true>(a, tparams, tt, swapc, swap_every, R, nullptr, &an);
}
#elif defined(MHX_JIT_TEMPERED_GENERIC) && defined(MHX_JIT_ADAPT)
extern "C" __global__ void __launch_bounds__(256)
mhx_jit_tempered_adapt_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_tmp_adapt ad,
                               mhx_u32* __restrict__ swapc, const int swap_every, const int R)
{
    mhx_tmp_generic_body<MHX_JIT_TK, true>(a, tparams, nullptr, swapc, swap_every, R, &ad);
}
#elif defined(MHX_JIT_TEMPERED_GENERIC)
extern "C" __global__ void __launch_bounds__(256)
mhx_jit_tempered_generic(const mhx_rwmh_args a, const mhx_real* __restrict__ tparams, const mhx_real* __restrict__ tt,
                         mhx_u32* __restrict__ swapc, const int swap_every, const int R)
{
    mhx_tmp_generic_body<MHX_JIT_TK>(a, tparams, tt, swapc, swap_every, R);
}
#endif
MHX_NS_END
