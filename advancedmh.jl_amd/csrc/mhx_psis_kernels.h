// mhx_psis_kernels.h -- Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO) of every data row from the saved draws, with the
// draws x rows matrix l[i, s] never stored (include/mhx.h: mhx_run_psis / mhx_ctx_psis).  The definitions are
// R loo's psis / gpdfit, stated at the prototypes.  Per data row the M smallest l (the M largest importance ratios exp(-l)) are needed;
// they are found by an exact radix select and one gather that RE-EVALUATE l where the HPD sweeps load a draw:
//
//   mhx_jit_psis_hist     one pass of the select (mhx_select_drive's callback, one rank per row): per row the histogram of one digit of
//                         the keys whose upper bits equal the row's prefix
//   mhx_jit_psis_gather   keys strictly below the cutoff's key go to the row's tail buffer (at most M of them: an atomic cursor, the
//                         order arbitrary, a sort follows); per row the number of keys equal to the cutoff, the number of non-finite l
//                         and B' = sum over l > tau of exp(tau - l)
//   (the host sorts every row's tail: one rocPRIM segmented radix sort of a batch)
//   mhx_jit_psis_fit      one block per row: the partials merged in index order, the generalised-Pareto fit of Zhang and Stephens, the
//                         smoothed tail and the two sums of elpd_loo
// Compiled at run time behind the user's MHX_POINTWISE text, after mhx_pointwise_kernels.h, whose draw and row views and whose frame
// (lane = chain, strips of draws dealt to strip slots, tiles of R data rows: mhx_pointwise_sweep) and block reduction
// (mhx_block_partials) the two sweeps share.  l is evaluated in the run's width and keyed in that width (mhx_order_key); everything
// after the widening is fp64 in both widths, with mhx_exp_f64 / mhx_log_f64.
//
// Order of operations.  The histograms are integer sums (LDS and global atomics: independent of arrival).  B', n_eq and bad are reduced
// as the pointwise partials are: butterfly over the wave, LDS in wave order, per-block partials merged in index order.  Every sum of the
// fit runs lane-strided with a butterfly, then over the waves in wave order.  Two calls give the same bits.
#pragma once
#include "mhx_device_math.h"

#ifndef MHX_JIT_PSIS_ROWS
#define MHX_JIT_PSIS_ROWS 4             // data rows per tile of the two sweeps: R x 2^11 LDS counters of 4 bytes (32 KiB at 4)
#endif
#define MHX_PSIS_MAX_DIGIT_BITS 11      // MHX_SELECT_MAX_DIGIT_BITS
#define MHX_PSIS_FIT_THREADS 256
#define MHX_PSIS_MAX_GRID 1054          // grid points of the fit at most: 30 + floor(sqrt(M)), M <= 2^20 (the host refuses more)

#if defined(MHX_HAVE_POINTWISE) && defined(MHX_HAVE_PSIS)
MHX_NS_BEGIN

// log(1 + y) and exp(y) - 1 in fp64 from the engine's log and exp (Kahan's forms: the rounding of 1 + y, or of exp(y), is divided out)
MHX_DEV double mhx_log1p_f64(const double y)
{
    const double u = 1.0 + y;
    if (u == 1.0) return y;
    if (!(__builtin_fabs(u) < __builtin_inf())) return mhx_log_f64(u);
    return mhx_log_f64(u) * (y / (u - 1.0));
}
MHX_DEV double mhx_expm1_f64(const double y)
{
    const double u = mhx_exp_f64(y);
    if (u == 1.0) return y;
    const double um1 = u - 1.0;
    if (um1 == -1.0 || !(u < __builtin_inf())) return um1;
    return um1 * (y / mhx_log_f64(u));
}

MHX_DEV double mhx_psis_wave_sum(double v)
{
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) v = v + __shfl_xor(v, mask, 64);
    return v;
}

// ---- 1. one pass of the select ---------------------------------------------------------------------------------------------------
// grid (chain blocks, strip slots, row tiles), block MHX_POINTWISE_THREADS.  hist [nrows][1 << digit_bits] of 64-bit counters, zeroed by
// the host.  `top`: the first pass, where every key belongs to the one group.  A block counts at most 256 lanes x its draws per row
// in a 32-bit LDS counter: the host deals the strips to enough slots that this stays below 2^32.
extern "C" __global__ void __launch_bounds__(MHX_POINTWISE_THREADS)
mhx_jit_psis_hist(const mhx_real* __restrict__ src, const long N, const long C, const int d, const mhx_real* __restrict__ rows,
                  const int nrows, const int rowlen, const mhx_real* __restrict__ data, const int ndata,
                  const unsigned long long* __restrict__ prefixes, const int shift, const int digit_bits, const int top,
                  unsigned long long* __restrict__ hist)
{
    constexpr int R = MHX_JIT_PSIS_ROWS;
    __shared__ unsigned lds[R << MHX_PSIS_MAX_DIGIT_BITS];
    const int nb = 1 << digit_bits;
    for (int k = threadIdx.x; k < R * nb; k += MHX_POINTWISE_THREADS) lds[k] = 0u;
    const int i0 = (int)blockIdx.z * R;
    mhx_key pf[R];
#pragma unroll
    for (int j = 0; j < R; ++j) pf[j] = (mhx_key)prefixes[i0 + j < nrows ? i0 + j : nrows - 1];
    const mhx_key dmask = (mhx_key)(nb - 1);
    const int hshift = top ? 0 : shift + digit_bits;            // top: shift + digit_bits is the key width, not a legal shift count
    __syncthreads();
    mhx_pointwise_sweep<R, true>(src, N, C, d, rows, nrows, rowlen, data, ndata, [&](const int j, const mhx_real v) {
        const mhx_key key = mhx_order_key(v);
        const unsigned digit = (unsigned)((key >> shift) & dmask);
        if (top || (mhx_key)(key >> hshift) == pf[j]) atomicAdd(&lds[j * nb + (int)digit], 1u);
    });
    __syncthreads();
    for (int k = threadIdx.x; k < R * nb; k += MHX_POINTWISE_THREADS) {
        const unsigned v = lds[k];
        const int j = k >> digit_bits;
        if (v && i0 + j < nrows) atomicAdd(&hist[((long)(i0 + j) << digit_bits) + (k & (nb - 1))], (unsigned long long)v);
    }
}

// ---- 2. the gather ----------------------------------------------------------------------------------------------------------------
// tau_key [nrows], tau [nrows] (the cutoff widened), cursor [nrows] zeroed by the host, tails [nrows][cap] keys,
// part [P][nrows][3] doubles (B', n_eq, bad), P = gridDim.x * gridDim.y.  A non-finite l is counted in bad and goes nowhere else.
// A slot at or above cap is never written (at most M keys lie strictly below the key of rank M).
extern "C" __global__ void __launch_bounds__(MHX_POINTWISE_THREADS)
mhx_jit_psis_gather(const mhx_real* __restrict__ src, const long N, const long C, const int d, const mhx_real* __restrict__ rows,
                    const int nrows, const int rowlen, const mhx_real* __restrict__ data, const int ndata,
                    const unsigned long long* __restrict__ tau_key, const double* __restrict__ tau, const unsigned long long cap,
                    unsigned long long* __restrict__ cursor, mhx_key* __restrict__ tails, double* __restrict__ part)
{
    constexpr int R = MHX_JIT_PSIS_ROWS;
    const int i0 = (int)blockIdx.z * R;
    mhx_key tk[R];
    double tv[R], body[R];
    mhx_u32 neq[R], bad[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int i = i0 + j < nrows ? i0 + j : nrows - 1;
        tk[j] = (mhx_key)tau_key[i];
        tv[j] = tau[i];
        body[j] = 0.0;
        neq[j] = bad[j] = 0u;
    }
    mhx_pointwise_sweep<R, true>(src, N, C, d, rows, nrows, rowlen, data, ndata, [&](const int j, const mhx_real v) {
        const double lv = (double)v;
        if (!(__builtin_fabs(lv) < __builtin_inf())) {
            bad[j] += 1u;
        } else {
            const mhx_key key = mhx_order_key(v);
            if (key < tk[j]) {
                const unsigned long long pos = atomicAdd(&cursor[i0 + j], 1ull);
                if (pos < cap) tails[(unsigned long long)(i0 + j) * cap + pos] = key;
            } else if (key == tk[j]) {
                neq[j] += 1u;
            } else {
                body[j] = body[j] + mhx_exp_f64(tv[j] - lv);
            }
        }
    });
    double v[R][3];
#pragma unroll
    for (int j = 0; j < R; ++j) { v[j][0] = body[j]; v[j][1] = (double)neq[j]; v[j][2] = (double)bad[j]; }
    mhx_block_partials(v, mhx_merge_sums{}, nrows, part);
}

// ---- 4. fit and sums --------------------------------------------------------------------------------------------------------------
// sum over i < n of f(i): lane-strided over the calling WAVE, butterfly; every lane returns the sum
template <class F>
MHX_DEV double mhx_psis_wave_strided(const unsigned long long n, const F& f)
{
    double acc = 0.0;
    for (unsigned long long i = threadIdx.x & 63u; i < n; i += 64) acc = acc + f(i);
    return mhx_psis_wave_sum(acc);
}

// one block per row.  sorted [nrows][cap] the row's keys strictly below the cutoff, ascending, count[i] of them; part as the gather
// wrote it; xbuf [nrows][cap] doubles of scratch; out [8][nrows]: elpd_loo, khat, sigma, tau, lmin, body, n_below, bad;
// tail_out [nrows][M] the tail ascending, copies of tau included.  M = cap.
extern "C" __global__ void __launch_bounds__(MHX_PSIS_FIT_THREADS)
mhx_jit_psis_fit(const mhx_key* __restrict__ sorted, const unsigned long long* __restrict__ count, const double* __restrict__ tau,
                 const double* __restrict__ part, const long P, const int nrows, const unsigned long long M, const double T,
                 double* xbuf, double* __restrict__ out, double* tail_out)
{
    __shared__ double s_theta[MHX_PSIS_MAX_GRID], s_l[MHX_PSIS_MAX_GRID], s_w[MHX_PSIS_MAX_GRID];
    __shared__ double s_red[MHX_PSIS_FIT_THREADS / 64][2];
    __shared__ double s_head[3], s_fit[3];
    const int i = (int)blockIdx.x;
    const int tid = (int)threadIdx.x, wave = tid >> 6, nwaves = MHX_PSIS_FIT_THREADS / 64;
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    if (tid == 0) {                                             // the partials of the row in index order
        double b = 0.0, e = 0.0, n = 0.0;
        for (long p = 0; p < P; ++p) {
            const double* q = part + (p * (long)nrows + i) * 3;
            b = b + q[0]; e = e + q[1]; n = n + q[2];
        }
        s_head[0] = b; s_head[1] = e; s_head[2] = n;
    }
    __syncthreads();
    const double bsum = s_head[0], neq = s_head[1], bad = s_head[2];
    double* tl = tail_out + (unsigned long long)i * M;
    if (bad > 0.0) {                                            // uniform over the block
        for (unsigned long long j = tid; j < M; j += MHX_PSIS_FIT_THREADS) tl[j] = nan;
        if (tid < 7) out[(long)tid * nrows + i] = nan;
        if (tid == 7) out[7l * nrows + i] = bad;
        return;
    }
    const double tv = tau[i];
    unsigned long long nbelow = count[i];
    if (nbelow > M) nbelow = M;
    const mhx_key* keys = sorted + (unsigned long long)i * M;
    const double lmin = nbelow ? mhx_key_value(keys[0]) : tv;
    const double ecut = mhx_exp_f64(lmin - tv);
    const double B = bsum + (neq - (double)(M - nbelow));
    double* x = xbuf + (unsigned long long)i * M;
    // the tail ascending (a[j], j < M) and the abscissae ascending: x[j] belongs to a[M - 1 - j]
    for (unsigned long long j = tid; j < M; j += MHX_PSIS_FIT_THREADS) {
        const double a = j < nbelow ? mhx_key_value(keys[j]) : tv;
        tl[j] = a;
        x[M - 1 - j] = mhx_exp_f64(lmin - a) - ecut;
    }
    __syncthreads();                                            // (x and tl are global: the block's own writes, visible after the barrier)
    double khat = inf, sigma = nan;
    bool fitted = false;
    if (M >= 5) {
        const double spread = tl[M - 1] - tl[0];
        if (!(spread < 0x1p-52 / 100.0)) {
            const int m = 30 + (int)__builtin_sqrt((double)M);  // exact floor: sqrt is correctly rounded and M < 2^52
            const double xstar = x[(unsigned long long)((double)M / 4.0 + 0.5) - 1], xmax = x[M - 1];
            for (int j = tid; j < m; j += MHX_PSIS_FIT_THREADS)
                s_theta[j] = 1.0 / xmax + (1.0 - __builtin_sqrt((double)m / ((double)(j + 1) - 0.5))) / (3.0 * xstar);
            __syncthreads();
            for (int j = wave; j < m; j += nwaves) {            // a wave per grid point
                const double th = s_theta[j];
                const double k = mhx_psis_wave_strided(M, [&](const unsigned long long q) { return mhx_log1p_f64(-th * x[q]); }) / (double)M;
                if ((tid & 63) == 0) s_l[j] = (double)M * (mhx_log_f64(-th / k) - k - 1.0);
            }
            __syncthreads();
            for (int j = tid; j < m; j += MHX_PSIS_FIT_THREADS) {
                double s = 0.0;
                for (int q = 0; q < m; ++q) s = s + mhx_exp_f64(s_l[q] - s_l[j]);
                s_w[j] = 1.0 / s;
            }
            __syncthreads();
            if (tid == 0) {
                double th = 0.0;
                for (int j = 0; j < m; ++j) th = __builtin_fma(s_w[j], s_theta[j], th);
                s_fit[0] = th;
            }
            __syncthreads();
            const double th = s_fit[0];
            const double k = mhx_psis_wave_strided(M, [&](const unsigned long long q) { return mhx_log1p_f64(-th * x[q]); }) / (double)M;
            const double sg = -k / th, kh = (k * (double)M + 5.0) / ((double)M + 10.0);
            if (__builtin_fabs(th) < inf && __builtin_fabs(kh) < inf && sg > 0.0 && sg < inf) { khat = kh; sigma = sg; fitted = true; }
        }
    }
    // the smoothed (or raw) log-weights of the tail, and the two sums: block-strided, butterfly, waves in wave order
    double snum = 0.0, sden = 0.0;
    for (unsigned long long j = tid; j < M; j += MHX_PSIS_FIT_THREADS) {
        const double a = tl[M - 1 - j];                         // the draw that x[j] belongs to
        double lw = lmin - a;
        if (fitted) {
            const double lp = mhx_log1p_f64(-(((double)j + 0.5) / (double)M));
            const double q = (khat == 0.0 ? -sigma * lp : sigma * mhx_expm1_f64(-khat * lp) / khat) + ecut;
            lw = mhx_log_f64(q);
            lw = lw < 0.0 ? lw : 0.0;                           // (a NaN gives 0: the raw weight's ceiling)
        }
        snum = snum + mhx_exp_f64(lw + (a - lmin));
        sden = sden + mhx_exp_f64(lw);
    }
    snum = mhx_psis_wave_sum(snum);
    sden = mhx_psis_wave_sum(sden);
    if ((tid & 63) == 0) { s_red[wave][0] = snum; s_red[wave][1] = sden; }
    __syncthreads();
    if (tid == 0) {
        double num = s_red[0][0], den = s_red[0][1];
        for (int w = 1; w < nwaves; ++w) { num = num + s_red[w][0]; den = den + s_red[w][1]; }
        const double elpd = lmin + mhx_log_f64((T - (double)M) + num) - mhx_log_f64(__builtin_fma(ecut, B, den));
        out[i] = elpd;
        out[(long)nrows + i] = khat;
        out[2l * nrows + i] = sigma;
        out[3l * nrows + i] = tv;
        out[4l * nrows + i] = lmin;
        out[5l * nrows + i] = B;
        out[6l * nrows + i] = (double)nbelow;
        out[7l * nrows + i] = 0.0;
    }
}

MHX_NS_END
#endif
