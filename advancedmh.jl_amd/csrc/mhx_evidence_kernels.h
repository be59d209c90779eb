// mhx_evidence_kernels.h -- what the log evidence of an anchored tempered run is made of (include/mhx.h: mhx_run_evidence; DESIGN.md
// sections 3.17.2 and 6.5.9): per CHAIN -- a (ladder, rung) slot, whose temperature never changes -- running fp64 reductions of
// u = lp - lq(x) over that chain's saved draws.  One sweep of the sample tensor, all d + 1 rows; eight doubles per chain leave it.
//
//   source  [N][d + 1][C]        the sample tensor of the run (row d: the untempered lp)
//   part    [slots][8][C]        one partial per strip slot and chain, fp64, written with plain stores
//   out     [C][8]               the partials of a chain merged in slot order (mhx_evidence_merge_body): bad, shift, s1, s2, max_f,
//                                sumexp_f, max_b, sumexp_b
// Pre-built in both widths: there is no user function, nothing is compiled at run time.
//
// Work layout: the pointwise frame's (mhx_pointwise_kernels.h) without its row tiles and without its block reduction.  A lane is a
// chain, a block 256 consecutive chains, every load of a draw's row one coalesced segment per wave through a scalar base and the
// lane's 32-bit byte offset; blockIdx.y is a strip slot -- strips of MHX_POINTWISE_STRIP consecutive draws dealt round robin -- so that
// a run of a few thousand chains still fills the device.
//
// Per draw: lq = mhx_tmp_logq(x) and u = lp - lq in the RUN's width, by the functions the step kernels call (the bits are theirs),
// then u widened to fp64 and, all fp64 in both widths,
//   u finite        y = u - shift; s1 += y; s2 = fma(y, y, s2);
//                   rung r >= 1:      l = dbeta[r - 1] * u  into (max_f, sumexp_f), the stepping-stone weight towards the colder rung
//                   rung r <= R - 2:  l = -(dbeta[r] * u)   into (max_b, sumexp_b), the backward weight
//                   where (max, sumexp) takes l as section 6.5.7's does: e = exp(-|l - max|); l > max ? (sumexp = sumexp e + 1, max = l)
//                   : (sumexp += e)
//   u NaN or +-inf  bad += 1, nothing else: the draw is left out of every sum
// shift = the chain's first saved u where that is finite, else 0 (every slot's block forms it again from draw 0: the same bits).
// The pair a rung has no use for keeps the neutral (-inf, 0).  No atomics: the order of every operation is a function of the shape
// alone, and two calls give the same bits.
#pragma once
#include "mhx_rwmh_tempered_kernels.h"
#include "mhx_pointwise_kernels.h"

MHX_NS_BEGIN

#define MHX_EVIDENCE_FIELDS 8

// (max, sumexp) takes one finite l
MHX_DEV void mhx_ev_lse_update(double& mx, double& se, const double l)
{
    const double e = mhx_exp_f64(-__builtin_fabs(l - mx));
    const bool up = l > mx;
    se = up ? __builtin_fma(se, e, 1.0) : se + e;
    mx = up ? l : mx;
}
// (max, sumexp) of two partials: the max-shifted merge of section 6.5.7.  Equal maxima (two -inf among them) add the sums.
MHX_DEV void mhx_ev_lse_merge(double& mx, double& se, const double bmx, const double bse)
{
    if (mx == bmx) {
        se = se + bse;
        return;
    }
    const bool a_big = mx > bmx;
    const double big = a_big ? se : bse, small = a_big ? bse : se;
    const double e = mhx_exp_f64(a_big ? bmx - mx : mx - bmx);
    se = __builtin_fma(small, e, big);
    mx = a_big ? mx : bmx;
}

// u of draw t of this lane's chain, widened
MHX_DEV double mhx_ev_u(const mhx_real* __restrict__ src, const long t, const long c0, const long ld, const int d, const mhx_u32 lane,
                        const mhx_tmp_anchor& an)
{
    const mhx_derive_in x = {src + t * (long)(d + 1) * ld + c0, ld, d, lane};
    const mhx_real lq = mhx_tmp_logq(x, d, an);
    const mhx_real u = x[d] - lq;
    return (double)u;
}

// grid (chain blocks, strip slots), MHX_POINTWISE_THREADS threads.  dbeta: the run's table, [R] reals (dbeta[R - 1] unused).
MHX_DEV void mhx_evidence_sweep_body(const mhx_real* __restrict__ src, const long N, const long C, const int d, const int R,
                                     const mhx_tmp_anchor& an, const mhx_real* __restrict__ dbeta, double* __restrict__ part)
{
    const long c0 = (long)blockIdx.x * MHX_POINTWISE_THREADS;
    const long c = c0 + (long)threadIdx.x;
    if (c >= C) return;                                             // (no block-wide step follows)
    long ld = C;
    mhx_u32 l = (mhx_u32)threadIdx.x * MHX_RB;
    asm volatile("" : "+s"(ld), "+v"(l));
    const int r = (int)(c & (long)(R - 1));                         // (a run's chain 0 is rung 0: first_chain is a multiple of R)
    const bool fwd = r >= 1, bwd = r + 1 < R;
    const double dbf = fwd ? (double)dbeta[r - 1] : 0.0, dbb = bwd ? (double)dbeta[r] : 0.0;
    const double inf = __builtin_inf();
    const double u0 = mhx_ev_u(src, 0, c0, ld, d, l, an);
    const double shift = __builtin_fabs(u0) < inf ? u0 : 0.0;
    double bad = 0.0, s1 = 0.0, s2 = 0.0, mxf = -inf, sef = 0.0, mxb = -inf, seb = 0.0;
    const long nstrips = (N + MHX_POINTWISE_STRIP - 1) / MHX_POINTWISE_STRIP;
    for (long s = blockIdx.y; s < nstrips; s += gridDim.y) {
        const long t0 = s * MHX_POINTWISE_STRIP;
        const long end = t0 + MHX_POINTWISE_STRIP < N ? t0 + MHX_POINTWISE_STRIP : N;
        for (long t = t0; t < end; ++t) {
            const double u = mhx_ev_u(src, t, c0, ld, d, l, an);
            if (__builtin_fabs(u) < inf) {
                const double y = u - shift;
                s1 = s1 + y;
                s2 = __builtin_fma(y, y, s2);
                if (fwd) mhx_ev_lse_update(mxf, sef, dbf * u);
                if (bwd) mhx_ev_lse_update(mxb, seb, -(dbb * u));
            } else bad += 1.0;                                      // (a lane counts at most N < 2^53 draws)
        }
    }
    double* o = part + (long)blockIdx.y * MHX_EVIDENCE_FIELDS * C + c;
    o[0] = bad; o[C] = shift; o[2 * C] = s1; o[3 * C] = s2;
    o[4 * C] = mxf; o[5 * C] = sef; o[6 * C] = mxb; o[7 * C] = seb;
}

// the partials of a chain merged in slot order; one thread per chain
MHX_DEV void mhx_evidence_merge_body(const double* __restrict__ part, const long slots, const long C, double* __restrict__ out)
{
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double* a = part + c;
    double bad = a[0], s1 = a[2 * C], s2 = a[3 * C], mxf = a[4 * C], sef = a[5 * C], mxb = a[6 * C], seb = a[7 * C];
    const double shift = a[C];
    for (long p = 1; p < slots; ++p) {
        const double* b = part + p * MHX_EVIDENCE_FIELDS * C + c;
        bad = bad + b[0];
        s1 = s1 + b[2 * C];
        s2 = s2 + b[3 * C];
        mhx_ev_lse_merge(mxf, sef, b[4 * C], b[5 * C]);
        mhx_ev_lse_merge(mxb, seb, b[6 * C], b[7 * C]);
    }
    double* o = out + c * MHX_EVIDENCE_FIELDS;
    o[0] = bad; o[1] = shift; o[2] = s1; o[3] = s2; o[4] = mxf; o[5] = sef; o[6] = mxb; o[7] = seb;
}

MHX_NS_END
