// mhx_diag_kernels.h -- chain diagnostics on the device sample tensor [N][dim+1][C] (chain fastest).
//
// What MCMCChains prints for the reference (README.md:59-63: mean, ESS, R-hat) needs, per parameter:
//   m_c, s2_c          per-chain mean and (unbiased) variance over the N draws
//   sum_c m_c, sum_c m_c^2, sum_c s2_c   -> between/within variances, R-hat, between-chain ESS
//   chain-averaged autocovariances up to max_lag over a subset of chains -> Geyer ESS
// All reads are coalesced over the chain index; accumulation is fp64.
#pragma once
#include "mhx_device_math.h"

MHX_NS_BEGIN

// grid (ceil(C/256), dim+1): one thread per (chain, parameter)
MHX_DEV void mhx_diag_moments_body(const mhx_real* __restrict__ samples, const long N, const int d1, const long C,
                                   double* __restrict__ mean, double* __restrict__ sums /* [3][d1] */, double* red)
{
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int p = blockIdx.y;
    double m = 0.0, v = 0.0;
    if (c < C) {
        const mhx_real* s = samples + (long)p * C + c;
        const long stride = (long)d1 * C;
        // the mean about the first draw: a chain that never moved has m == x_0 and v == 0 exactly, whatever x_0 is
        const double x0 = (double)s[0];
        double sum = 0.0;
        for (long t = 0; t < N; ++t) sum += (double)s[t * stride] - x0;
        m = x0 + sum / (double)N;
        double ss = 0.0;
        for (long t = 0; t < N; ++t) { const double e = (double)s[t * stride] - m; ss += e * e; }
        v = N > 1 ? ss / (double)(N - 1) : 0.0;
        // a non-finite draw: the chain's mean, and with it every sum and autocovariance of the row, is NaN (never +-inf)
        if (!(fabs(m) <= 1.7976931348623157e308) || v != v) m = v = __longlong_as_double(0x7ff8000000000000ll);
        mean[(long)p * C + c] = m;
    }
    // block reduction of (m, m^2, v) then one fp64 atomic each
    double vals[3] = {c < C ? m : 0.0, c < C ? m * m : 0.0, c < C ? v : 0.0};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        double x = vals[q];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if ((threadIdx.x & 63) == 0) red[q * 4 + (threadIdx.x >> 6)] = x;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const double x = red[threadIdx.x * 4] + red[threadIdx.x * 4 + 1] + red[threadIdx.x * 4 + 2] + red[threadIdx.x * 4 + 3];
        atomicAdd(&sums[(long)threadIdx.x * d1 + p], x);
    }
}

// grid (ceil(nc/64), dim+1, lags of this launch), block 64: acov[k][p] += sum_{c<nc} sum_t (x_t-m_c)(x_{t+k}-m_c), k = k0 + blockIdx.z
// (the host slices the lags so that grid.z stays within the device's limit)
MHX_DEV void mhx_diag_autocov_body(const mhx_real* __restrict__ samples, const long N, const int d1, const long C,
                                   const long nc, const long k0, const double* __restrict__ mean, double* __restrict__ acov)
{
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int p = blockIdx.y;
    const long k = k0 + blockIdx.z;
    double acc = 0.0;
    if (c < nc && k < N) {
        const mhx_real* s = samples + (long)p * C + c;
        const long stride = (long)d1 * C;
        const mhx_real m = (mhx_real)mean[(long)p * C + c];
        mhx_real a0 = MHX_R(0.0), a1 = MHX_R(0.0);
        long t = 0;
        for (; t + 1 < N - k; t += 2) {
            a0 = mhx_fma(s[t * stride] - m, s[(t + k) * stride] - m, a0);
            a1 = mhx_fma(s[(t + 1) * stride] - m, s[(t + 1 + k) * stride] - m, a1);
            if ((t & 1023) == 1022) { acc += (double)a0 + (double)a1; a0 = a1 = MHX_R(0.0); }
        }
        for (; t < N - k; ++t) a0 = mhx_fma(s[t * stride] - m, s[(t + k) * stride] - m, a0);
        acc += (double)a0 + (double)a1;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (threadIdx.x == 0) atomicAdd(&acov[k * d1 + p], acc);
}

// grid (ceil(C/256), dim+1) per half: between[p] += sum_c (m_c - sum_m[p] / M)^2 -- the between-chain variance of the ESS about the
// mean of the chain means.  (sum_m2 - sum_m^2 / M, which the un-normalised sums leave to the caller, cancels |mean|^2 / Vm of the
// digits: 1e-3 of var+ is lost to it in fp64 for a parameter at 1e4 +- 0.01.)
MHX_DEV void mhx_diag_between_body(const double* __restrict__ mean, const double* __restrict__ sums, const int d1, const long C,
                                   const double M, double* __restrict__ between, double* red)
{
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int p = blockIdx.y;
    double x = 0.0;
    if (c < C) { const double e = mean[(long)p * C + c] - sums[p] / M; x = e * e; }
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&between[p], red[0] + red[1] + red[2] + red[3]);
}

// the same three sums from running moments (runs that kept no sample tensor): m_c = mean, s2_c = M2/(n-1)
MHX_DEV void mhx_diag_from_moments_body(const mhx_real* __restrict__ mom_mean, const mhx_real* __restrict__ mom_m2,
                                        const long nsamp, const int d1, const long C, double* __restrict__ sums,
                                        double* red)
{
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int p = blockIdx.y;
    double m = 0.0, v = 0.0;
    if (c < C) {
        m = (double)mom_mean[(long)p * C + c];
        v = nsamp > 1 ? (double)mom_m2[(long)p * C + c] / (double)(nsamp - 1) : 0.0;
    }
    double vals[3] = {c < C ? m : 0.0, c < C ? m * m : 0.0, c < C ? v : 0.0};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        double x = vals[q];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if ((threadIdx.x & 63) == 0) red[q * 4 + (threadIdx.x >> 6)] = x;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const double x = red[threadIdx.x * 4] + red[threadIdx.x * 4 + 1] + red[threadIdx.x * 4 + 2] + red[threadIdx.x * 4 + 3];
        atomicAdd(&sums[(long)threadIdx.x * d1 + p], x);
    }
}

// ---- the rank of a draw among the FOLDED draws g = fl(|x - m|), from the one ascending array of the draws ----
// x -> fl(x - m) is non-decreasing (rounding is monotone), so g is non-increasing over the draws below m and non-decreasing over
// the rest.  With `left(i)` = sorted[i] < m, each of the four predicates
//   !(left && g > f)    !(left && g >= f)    (!left && g >= f)    (!left && g > f)
// is false on a prefix of the whole array and true behind it; the first true index of each, iL_leq <= iL_less <= iR_less <= iR_leq,
// gives the number of draws with g < f (iR_less - iL_less) and with g <= f (iR_leq - iL_leq) without knowing where the sides meet.
// The tie-averaged 1-based rank of the draw at sorted index r follows.  Exact where the subtraction collapses distinct draws onto
// one g as well: only the order of g is used, never that of x within a side.
// The searches run in pairs: the two loads of a step are independent, so the dependent chain is 2 log2 S loads, not 4.  A pair
// keeps its loads unconditional (the probe of a finished search is clamped into the array and its result dropped).
MHX_DEV double mhx_diag_fold_rank(const mhx_real* __restrict__ sorted, const long S, const mhx_real m, const long r)
{
    const mhx_real f = mhx_abs(sorted[r] - m);
    // iL_less in [0, S], iR_less in [0, S]
    long a0 = 0, a1 = S, b0 = 0, b1 = S;
    while (a0 < a1 || b0 < b1) {
        const long ma = (a0 + a1) >> 1, mb = (b0 + b1) >> 1;
        const mhx_real ya = sorted[ma < S ? ma : S - 1], yb = sorted[mb < S ? mb : S - 1];
        const bool pa = !(ya < m && mhx_abs(ya - m) >= f), pb = !(yb < m) && mhx_abs(yb - m) >= f;
        if (a0 < a1) { if (pa) a1 = ma; else a0 = ma + 1; }
        if (b0 < b1) { if (pb) b1 = mb; else b0 = mb + 1; }
    }
    const long il_less = a0, ir_less = b0;
    // iL_leq in [0, iL_less], iR_leq in [iR_less, S]
    a0 = 0; a1 = il_less; b0 = ir_less; b1 = S;
    while (a0 < a1 || b0 < b1) {
        const long ma = (a0 + a1) >> 1, mb = (b0 + b1) >> 1;
        const mhx_real ya = sorted[ma < S ? ma : S - 1], yb = sorted[mb < S ? mb : S - 1];
        const bool pa = !(ya < m && mhx_abs(ya - m) > f), pb = !(yb < m) && mhx_abs(yb - m) > f;
        if (a0 < a1) { if (pa) a1 = ma; else a0 = ma + 1; }
        if (b0 < b1) { if (pb) b1 = mb; else b0 = mb + 1; }
    }
    const long less = ir_less - il_less, leq = b0 - a0;
    return 0.5 * ((double)less + (double)leq - 1.0) + 1.0;
}

// ---- exact order statistics: one pass of a histogram radix SELECT over the strided tensor ----
// The draws are compared as their order keys (mhx_order_key, mhx_device_math.h): NaNs come last, -0.0 < +0.0.

#define MHX_SELECT_THREADS 512
// loads in flight per thread: 32 bytes per thread either way (16 KiB per block, up to 64 KiB per CU)
#if MHX_REAL64
#define MHX_SELECT_UNROLL 4
#else
#define MHX_SELECT_UNROLL 8
#endif

// one draw into the block's histograms.  The prefixes of a parameter's groups are distinct, so at most one matches: the slot is
// picked by compares and selects and ONE LDS atomic follows (unused slots repeat prefix 0 and are visited first, so they never win)
template <int BITS, int G>
MHX_DEV void mhx_select_count(const mhx_key key, const mhx_key (&pf)[G], const int top, const int shift, const int hshift,
                              const mhx_key dmask, unsigned* lds)
{
    const unsigned digit = (unsigned)((key >> shift) & dmask);
    if (top) { atomicAdd(&lds[digit], 1u); return; }       // the first pass: one group of all draws
    const mhx_key hi = (mhx_key)(key >> hshift);
    int slot = -1;
#pragma unroll
    for (int g = G - 1; g >= 0; --g) slot = hi == pf[g] ? g : slot;
    if (slot >= 0) atomicAdd(&lds[(slot << BITS) + digit], 1u);
}

// grid (blocks per parameter, parameters), block MHX_SELECT_THREADS.  Block (b, i) owns elements [b chunk, (b+1) chunk) of the
// flattened (t, c) index space of row params[i]: element e is draw t = e / C of chain c = e - t C, so consecutive lanes read
// consecutive chains (one division per thread, then a running offset).  A draw whose key has, above the current digit, the
// prefix of group g (groups first .. first + ng - 1 of this parameter; `top`: the first pass, where every draw belongs to the
// one group) counts in bin `digit` of that group's histogram in LDS (uint32: chunk < 2^32); the non-zero bins are then added to
// the global uint64 histogram hist[i][gstride][1 << digit_bits] with integer atomics (sums independent of the order of
// arrival).  LDS: G << BITS words whatever the number of ranks asked for.
template <int BITS, int G>
MHX_DEV void mhx_select_hist_body(const mhx_real* __restrict__ samples, const long N, const int d1, const long C,
                                  const int* __restrict__ params, const unsigned long long* __restrict__ prefixes,
                                  const int* __restrict__ ngroups, const int gstride, const int first, const int shift,
                                  const int digit_bits, const int top, const unsigned long long chunk,
                                  unsigned long long* __restrict__ hist, unsigned* lds)
{
    const int i = blockIdx.y;
    int ng = ngroups[i] - first;
    if (ng <= 0) return;                                   // uniform over the block
    if (ng > G) ng = G;
    const long p = params[i];
    const unsigned long long S = (unsigned long long)N * (unsigned long long)C;
    const unsigned long long e0 = (unsigned long long)blockIdx.x * chunk;
    if (e0 >= S) return;
    const unsigned long long e1 = e0 + chunk < S ? e0 + chunk : S;
    for (int k = threadIdx.x; k < (ng << BITS); k += MHX_SELECT_THREADS) lds[k] = 0u;
    mhx_key pf[G];
    const unsigned long long* mine = prefixes + (long)i * gstride + first;
#pragma unroll
    for (int g = 0; g < G; ++g) pf[g] = (mhx_key)mine[g < ng ? g : 0];
    __syncthreads();
    const mhx_key dmask = (mhx_key)((1u << digit_bits) - 1u);
    const int hshift = top ? 0 : shift + digit_bits;       // top: shift + digit_bits is the key width, not a legal shift count
    // this thread's element e0 + tid + k THREADS: offset t ld + c into the row, advanced by the block width
    const unsigned long long ef = e0 + threadIdx.x;
    const long t0 = (long)(ef / (unsigned long long)C);
    long c = (long)(ef - (unsigned long long)t0 * (unsigned long long)C);
    const long ld = (long)d1 * C;
    const long qt = MHX_SELECT_THREADS / C, qc = MHX_SELECT_THREADS - qt * C, step = qt * ld + qc, wrap = ld - C;
    const mhx_real* src = samples + p * C + t0 * ld + c;
    // whole sweeps of UNROLL elements per thread: every load is in bounds, none is predicated, all are issued before the first is used
    const unsigned long long sweeps = (e1 - e0) / ((unsigned long long)MHX_SELECT_THREADS * MHX_SELECT_UNROLL);
    for (unsigned long long it = 0; it < sweeps; ++it) {
        mhx_real x[MHX_SELECT_UNROLL];
#pragma unroll
        for (int u = 0; u < MHX_SELECT_UNROLL; ++u) {
            x[u] = *src;
            src += step; c += qc;
            if (c >= C) { c -= C; src += wrap; }
        }
#pragma unroll
        for (int u = 0; u < MHX_SELECT_UNROLL; ++u) mhx_select_count<BITS, G>(mhx_order_key(x[u]), pf, top, shift, hshift, dmask, lds);
    }
    // the rest of the chunk, one element at a time
    for (unsigned long long e = ef + sweeps * MHX_SELECT_THREADS * MHX_SELECT_UNROLL; e < e1; e += MHX_SELECT_THREADS) {
        const mhx_real x = *src;
        src += step; c += qc;
        if (c >= C) { c -= C; src += wrap; }
        mhx_select_count<BITS, G>(mhx_order_key(x), pf, top, shift, hshift, dmask, lds);
    }
    __syncthreads();
    // bins at or above 1 << digit_bits stay zero (the digit is masked), so only legal bins of the global histogram are touched
    unsigned long long* out = hist + (((long)i * gstride + first) << digit_bits);
    for (int k = threadIdx.x; k < (ng << BITS); k += MHX_SELECT_THREADS) {
        const unsigned v = lds[k];
        if (v) atomicAdd(&out[((long)(k >> BITS) << digit_bits) + (k & ((1 << BITS) - 1))], (unsigned long long)v);
    }
}
MHX_NS_END
