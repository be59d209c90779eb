// mhx_pointwise_kernels.h -- the pointwise log-likelihood l[i, s] = log p(row i | saved draw s) of every (draw, data row) pair,
// reduced over the draws where it is computed: only five fp64 numbers per data row leave the kernel (include/mhx.h:
// mhx_run_pointwise / mhx_ctx_pointwise).  What lppd, WAIC and DIC are made of.
//
//   source  [N][d + 1][C]        the sample tensor, as the derive frame reads it (mhx_derive_kernels.h: x[k], lazy and clamped)
//   rows    [nrows][rowlen]      the data rows, in the run's width
//   part    [P][nrows][5]        one partial (max, sumexp, s1, s2, bad) per (chain block, strip slot) and row, fp64
//   out     [5][nrows]           the partials of a row merged in index order p = 0 .. P-1 (mhx_jit_pointwise_merge)
// Compiled at run time only (the function is user source, MHX_POINTWISE), once per (source, width, rows per tile).
//
// Work layout.  A lane is a chain, a block 256 consecutive chains (every load of a draw's row is one coalesced segment per wave);
// blockIdx.y is a strip slot -- strips of MHX_POINTWISE_STRIP consecutive draws, dealt round robin to gridDim.y slots, which the
// host caps so that the partials do not grow with N --, blockIdx.z a tile of R = MHX_JIT_POINTWISE_ROWS data rows.  Per draw the
// user function is called R times with the same x, unrolled: the loads its source names are the same expression in every copy
// (the tensor is __restrict__ and nothing is stored in the loop), so each named row is loaded once per draw; the row entries
// r[j] have a wave-uniform address and come through the scalar cache.
//
// Per (draw, row): l widened to fp64, then -- all fp64, in both widths --
//   l finite            e = exp(-|l - max|); l > max ? (sumexp = sumexp e + 1, max = l) : (sumexp += e);  y = l - shift;
//                       s1 += y;  s2 = fma(y, y, s2)
//   l = -inf            bad += 1, nothing else (it adds 0 to sumexp and never meets a -inf max in a subtraction)
//   l NaN or +inf       bad += 1, sumexp = NaN (which no later step removes); max[i] is made NaN when the row is written
// A running max of -inf meets only finite l: exp(-inf) = 0 and sumexp (0 until then) becomes 0 * 0 + 1.
//
// The end of a lane's strips: mhx_block_partials (butterfly over the wave, the block's four waves through LDS in wave order).  Lanes
// beyond C hold the neutral partial (-inf, 0, 0, 0, 0) and take part.  No atomics anywhere: the order of every operation is a
// function of the shape alone, and two calls give the same bits.
//
// This header also holds what the PSIS sweeps (mhx_psis_kernels.h) share with this one: the sweep frame mhx_pointwise_sweep and the
// block reduction mhx_block_partials.
#pragma once
#include "mhx_device_math.h"

#define MHX_POINTWISE_THREADS 256
#ifndef MHX_JIT_POINTWISE_ROWS
#define MHX_JIT_POINTWISE_ROWS 8        // data rows per tile: 5 accumulators each, in registers (the host always says: mhx_api_pointwise.inc)
#endif
#ifndef MHX_POINTWISE_STRIP
#define MHX_POINTWISE_STRIP 16          // consecutive draws of one strip
#endif
#define MHX_POINTWISE_MAX_SLOTS 64      // strip slots per chain block at most (the host asks for fewer where the grid is large)
#ifndef MHX_DERIVE_MIN_WAVES
#define MHX_DERIVE_MIN_WAVES 1
#endif

#ifdef MHX_HAVE_POINTWISE
MHX_NS_BEGIN

typedef mhx_derive_in mhx_pointwise_in;     // one draw as the function reads it (mhx_device_math.h)

// one data row
struct mhx_pointwise_row {
    const mhx_real* p;
    int m;
    MHX_DEV mhx_real operator[](const int j) const { return p[j < 0 ? 0 : (j >= m ? m - 1 : j)]; }
};

// the running reductions of one data row
struct mhx_pw_acc {
    double mx, se, s1, s2;
    mhx_u32 bad;
};

MHX_DEV void mhx_pw_update(mhx_pw_acc& a, const double l, const double shift)
{
    const double inf = __builtin_inf();
    if (__builtin_fabs(l) < inf) {
        const double e = mhx_exp_f64(-__builtin_fabs(l - a.mx));
        const bool up = l > a.mx;
        a.se = up ? __builtin_fma(a.se, e, 1.0) : a.se + e;
        a.mx = up ? l : a.mx;
        const double y = l - shift;
        a.s1 = a.s1 + y;
        a.s2 = __builtin_fma(y, y, a.s2);
    } else {
        a.bad += 1u;
        if (!(l == -inf)) a.se = __builtin_nan("");
    }
}

// (max, sumexp) of two partials; symmetric in (a, b) bit for bit.  Equal maxima (two -inf among them) add the sums.
MHX_DEV void mhx_pw_merge_lse(double& mx, double& se, const double bmx, const double bse)
{
    if (mx == bmx) {
        se = se + bse;
        return;
    }
    const bool a_big = mx > bmx;
    const double big = a_big ? se : bse, small = a_big ? bse : se;
    const double e = mhx_exp_f64(a_big ? bmx - mx : mx - bmx);       // (the smaller max may be -inf: exp gives 0, its sum is 0)
    se = __builtin_fma(small, e, big);
    mx = a_big ? mx : bmx;
}

// ---- what the sweeps of this module and of mhx_psis_kernels.h share ---------------------------------------------------------------
// The merge of two partials of K doubles, a <- a (+) b: every field a plain sum, or (max, sumexp) first and plain sums after.
struct mhx_merge_sums {
    template <int K>
    MHX_DEV void operator()(double (&a)[K], const double (&b)[K]) const
    {
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = a[k] + b[k];
    }
};
struct mhx_merge_pw {
    MHX_DEV void operator()(double (&a)[5], const double (&b)[5]) const
    {
        mhx_pw_merge_lse(a[0], a[1], b[0], b[1]);
        a[2] = a[2] + b[2];
        a[3] = a[3] + b[3];
        a[4] = a[4] + b[4];
    }
};

// The sweep frame: every draw of this lane's strips x every row of the block's tile -> f(j, l), l = the user function of (draw, row
// i0 + j).  grid (chain blocks, strip slots, row tiles); a lane beyond C calls nothing.  SKIP: the rows of a ragged last tile beyond
// nrows are skipped (what a sweep that counts needs); otherwise they are evaluated on a repeat of the last row, for the caller not to
// write.  C and the lane offset are made opaque as in mhx_derive_draws: a scalar base plus the lane's 32-bit offset per load.
template <int R, bool SKIP, class F>
MHX_DEV void mhx_pointwise_sweep(const mhx_real* __restrict__ src, const long N, const long C, const int d,
                                 const mhx_real* __restrict__ rows, const int nrows, const int rowlen,
                                 const mhx_real* __restrict__ data, const int ndata, const F& f)
{
    const long c0 = (long)blockIdx.x * MHX_POINTWISE_THREADS;
    const int i0 = (int)blockIdx.z * R;
    if (c0 + (long)threadIdx.x < C) {
        long ld = C;
        mhx_u32 l = (mhx_u32)threadIdx.x * MHX_RB;
        asm volatile("" : "+s"(ld), "+v"(l));
        const long nstrips = (N + MHX_POINTWISE_STRIP - 1) / MHX_POINTWISE_STRIP;
        for (long s = blockIdx.y; s < nstrips; s += gridDim.y) {
            const long t0 = s * MHX_POINTWISE_STRIP;
            const long end = t0 + MHX_POINTWISE_STRIP < N ? t0 + MHX_POINTWISE_STRIP : N;
            for (long t = t0; t < end; ++t) {
                const mhx_pointwise_in x = {src + t * (long)(d + 1) * ld + c0, ld, d, l};
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const bool live = i0 + j < nrows;               // uniform over the block
                    if (SKIP && !live) continue;
                    const mhx_pointwise_row r = {rows + (long)(live ? i0 + j : nrows - 1) * rowlen, rowlen};
                    f(j, mhx_user_pointwise(x, r, rowlen, d, data, ndata));
                }
            }
        }
    }
}

// The block's partial of R rows x K doubles: v[j] of every lane merged over the wave by a butterfly of shuffles (xor 1, 2, .. 32: a
// merge that is symmetric in its arguments bit for bit leaves every lane with the same value), then over the block's waves through
// LDS in wave order by thread j, which writes row i0 + j of part [P][nrows][K] at p = blockIdx.x * gridDim.y + blockIdx.y.  Every
// lane of the block calls it, the lanes beyond C with the neutral partial.
template <int R, int K, class M>
MHX_DEV void mhx_block_partials(double (&v)[R][K], const M& merge, const int nrows, double* __restrict__ part)
{
    __shared__ double lds[MHX_POINTWISE_THREADS / 64][R][K];
    const int i0 = (int)blockIdx.z * R;
#pragma unroll
    for (int j = 0; j < R; ++j) {
#pragma unroll
        for (int mask = 1; mask < 64; mask <<= 1) {
            double b[K];
#pragma unroll
            for (int k = 0; k < K; ++k) b[k] = __shfl_xor(v[j][k], mask, 64);
            merge(v[j], b);
        }
    }
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int j = 0; j < R; ++j)
#pragma unroll
            for (int k = 0; k < K; ++k) lds[wave][j][k] = v[j][k];
    }
    __syncthreads();
    const int j = (int)threadIdx.x;
    if (j < R && i0 + j < nrows) {
        double a[K];
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = lds[0][j][k];
        for (int w = 1; w < MHX_POINTWISE_THREADS / 64; ++w) merge(a, lds[w][j]);
        const long p = (long)blockIdx.x * gridDim.y + blockIdx.y;
        double* o = part + (p * (long)nrows + (i0 + j)) * K;
#pragma unroll
        for (int k = 0; k < K; ++k) o[k] = a[k];
    }
}

// The pointwise sweep.  Its loop is mhx_pointwise_sweep<R, false> written out: on the frame the fp64 kernel at R = 8 goes from 159 to
// 169 - 191 VGPRs and from three waves per SIMD to two (DESIGN.md section 6.7 has the forms tried).
template <int R>
MHX_DEV void mhx_pointwise_body(const mhx_real* __restrict__ src, const long N, const long C, const int d,
                                const mhx_real* __restrict__ rows, const int nrows, const int rowlen,
                                const mhx_real* __restrict__ data, const int ndata, const double* __restrict__ shift,
                                double* __restrict__ part)
{
    const long c0 = (long)blockIdx.x * MHX_POINTWISE_THREADS;
    const bool active = c0 + (long)threadIdx.x < C;
    const int i0 = (int)blockIdx.z * R;
    mhx_pw_acc acc[R];
    double sh[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        acc[j] = mhx_pw_acc{-__builtin_inf(), 0.0, 0.0, 0.0, 0u};
        const int i = i0 + j < nrows ? i0 + j : nrows - 1;          // (a tile's rows beyond nrows repeat the last row; not written)
        sh[j] = shift[i];
    }
    if (active) {
        long ld = C;
        mhx_u32 l = (mhx_u32)threadIdx.x * MHX_RB;
        asm volatile("" : "+s"(ld), "+v"(l));
        const long nstrips = (N + MHX_POINTWISE_STRIP - 1) / MHX_POINTWISE_STRIP;
        for (long s = blockIdx.y; s < nstrips; s += gridDim.y) {
            const long t0 = s * MHX_POINTWISE_STRIP;
            const long end = t0 + MHX_POINTWISE_STRIP < N ? t0 + MHX_POINTWISE_STRIP : N;
            for (long t = t0; t < end; ++t) {
                const mhx_pointwise_in x = {src + t * (long)(d + 1) * ld + c0, ld, d, l};
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const int i = i0 + j < nrows ? i0 + j : nrows - 1;
                    const mhx_pointwise_row r = {rows + (long)i * rowlen, rowlen};
                    const mhx_real v = mhx_user_pointwise(x, r, rowlen, d, data, ndata);
                    mhx_pw_update(acc[j], (double)v, sh[j]);
                }
            }
        }
    }
    double v[R][5];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        v[j][0] = acc[j].mx; v[j][1] = acc[j].se; v[j][2] = acc[j].s1; v[j][3] = acc[j].s2;
        v[j][4] = (double)acc[j].bad;                               // (a lane counts at most N < 2^32 draws; their sums are doubles)
    }
    mhx_block_partials(v, mhx_merge_pw{}, nrows, part);
}

extern "C" __global__ void __launch_bounds__(MHX_POINTWISE_THREADS, MHX_DERIVE_MIN_WAVES)
mhx_jit_pointwise(const mhx_real* __restrict__ src, const long N, const long C, const int d, const mhx_real* __restrict__ rows,
                  const int nrows, const int rowlen, const mhx_real* __restrict__ data, const int ndata,
                  const double* __restrict__ shift, double* __restrict__ part)
{
    mhx_pointwise_body<MHX_JIT_POINTWISE_ROWS>(src, N, C, d, rows, nrows, rowlen, data, ndata, shift, part);
}

// shift[i] = l[i, draw 0 of chain 0] where that is finite, else 0: one thread per data row
extern "C" __global__ void __launch_bounds__(64)
mhx_jit_pointwise_shift(const mhx_real* __restrict__ src, const long C, const int d, const mhx_real* __restrict__ rows, const int nrows,
                        const int rowlen, const mhx_real* __restrict__ data, const int ndata, double* __restrict__ shift)
{
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= nrows) return;
    const mhx_pointwise_in x = {src, C, d, 0u};
    const mhx_pointwise_row r = {rows + i * rowlen, rowlen};
    const double v = (double)mhx_user_pointwise(x, r, rowlen, d, data, ndata);
    shift[i] = __builtin_fabs(v) < __builtin_inf() ? v : 0.0;
}

// the partials of a row merged in index order; one thread per data row.  out [5][nrows]: max, sumexp, s1, s2, bad
extern "C" __global__ void __launch_bounds__(64)
mhx_jit_pointwise_merge(const double* __restrict__ part, const long P, const int nrows, double* __restrict__ out)
{
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= nrows) return;
    const double* a = part + i * 5;
    double mx = a[0], se = a[1], s1 = a[2], s2 = a[3], bad = a[4];
    for (long p = 1; p < P; ++p) {
        const double* b = part + (p * (long)nrows + i) * 5;
        mhx_pw_merge_lse(mx, se, b[0], b[1]);
        s1 = s1 + b[2];
        s2 = s2 + b[3];
        bad = bad + b[4];
    }
    const bool poisoned = se != se;                                 // a NaN or +inf l somewhere among the draws
    out[i] = poisoned ? __builtin_nan("") : mx;
    out[(long)nrows + i] = se;
    out[2l * nrows + i] = s1;
    out[3l * nrows + i] = s2;
    out[4l * nrows + i] = bad;
}

MHX_NS_END
#endif
