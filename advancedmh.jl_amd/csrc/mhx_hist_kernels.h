// mhx_hist_kernels.h -- histograms and pair histograms of the pooled draws of parameter rows over caller-given bin edges
// (what MCMCChains offers as `histogram`, `density` and `corner`).
//
// A draw is widened exactly to double, edges are doubles, every comparison is a double comparison.  For the non-decreasing finite
// edges e[0..B] of a row the slot of a draw x is
//   x != x            NaN                     (slot B + 2)
//   x <  e[0]         below, -inf included    (slot B)
//   x >  e[B]         above, +inf included    (slot B + 1)
//   otherwise         bin j = (number of edges <= x) - 1, i.e. e[j] <= x < e[j+1]; x == e[B] closes the last bin: j = B - 1
// which is numpy.histogram(x64, bins=e).  -0.0 and +0.0 compare equal, so they are the same draw.
//   mhx_hist1d_body   ONE sweep of the [N][d1][C] tensor in place for all rows asked for: the sweep of mhx_select_hist_body with this
//                     bin function; per-block counts in LDS (uint32), the non-zero ones added to uint64 counters with integer atomics
//   mhx_hist2d_body   the same sweep over the two rows of a pair at once: cell [bin of the first row][bin of the second]; a draw
//                     without a bin on either axis counts in the pair's `outside`
// No floating-point atomics: integer sums do not depend on the order of arrival, two calls return the same bits.
#pragma once
#include "mhx_diag_kernels.h"

MHX_NS_BEGIN

#define MHX_HIST_MAX_BINS 2048                              // 1-D: 2048 + 3 counters and 2049 edges in LDS, 24.6 KB
#define MHX_HIST2D_MAX_BINS 128                             // 2-D: 128 x 128 counters (64 KiB) and 2 x 129 edges beside them

// The slot of x among the edges e[0..B] (LDS).  The uniform-bin guess (int)((x - e[0]) B / (e[B] - e[0])) is off by at most one bin
// for uniform edges; with non-decreasing edges e[j] <= x < e[j+1] holds for exactly one j, so a guess that passes that test IS the
// bin whatever the edges, and every other draw is placed by bisection: (number of edges <= x) - 1.
MHX_DEV int mhx_hist_slot(const double x, const double* e, const int B, const double e0, const double eB, const double scale)
{
    if (x != x) return B + 2;
    if (x < e0) return B;
    if (x > eB) return B + 1;
    const double g = (x - e0) * scale;                      // >= 0, or NaN (inf x 0: edges further apart than the largest double)
    int j = g < (double)B ? (g >= 0.0 ? (int)g : 0) : B - 1;
    if (e[j] <= x && x < e[j + 1]) return j;
    int lo = 1, hi = B + 1;                                 // the first edge above x lies in [lo, hi] (e[0] <= x; B + 1: none)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid + 1; else hi = mid;
    }
    j = lo - 1;
    return j < B ? j : B - 1;
}

// B / (e[B] - e[0]), 0 where all edges are equal (then every draw in range is placed by the bisection)
MHX_DEV double mhx_hist_scale(const double e0, const double eB, const int B)
{
    return eB > e0 ? (double)B / (eB - e0) : 0.0;
}

// grid (blocks per row, rows), block MHX_SELECT_THREADS: the geometry and the element-to-(t, c) map of mhx_select_hist_body (block
// (b, i) owns elements [b chunk, (b + 1) chunk) of row params[i], chunk < 2^32 so the LDS counters cannot wrap).  Row i of the call
// has the edges edges[i (B + 1) ..], the counters counts[i B ..] and outside[3 i ..] = below, above, NaN.
// LDS: lds_e[B + 1] edges, lds_n[B + 3] counters (bins, then below, above, NaN).
MHX_DEV void mhx_hist1d_body(const mhx_real* __restrict__ samples, const long N, const int d1, const long C,
                             const int* __restrict__ params, const double* __restrict__ edges, const int B,
                             const unsigned long long chunk, unsigned long long* __restrict__ counts,
                             unsigned long long* __restrict__ outside, double* lds_e, unsigned* lds_n)
{
    const int i = blockIdx.y;
    const long p = params[i];
    const unsigned long long S = (unsigned long long)N * (unsigned long long)C;
    const unsigned long long e0 = (unsigned long long)blockIdx.x * chunk;
    if (e0 >= S) return;                                    // uniform over the block
    const unsigned long long e1 = e0 + chunk < S ? e0 + chunk : S;
    for (int k = threadIdx.x; k < B + 3; k += MHX_SELECT_THREADS) lds_n[k] = 0u;
    for (int k = threadIdx.x; k <= B; k += MHX_SELECT_THREADS) lds_e[k] = edges[(long)i * (B + 1) + k];
    __syncthreads();
    const double lo = lds_e[0], hi = lds_e[B], scale = mhx_hist_scale(lo, hi, B);
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
        for (int u = 0; u < MHX_SELECT_UNROLL; ++u) atomicAdd(&lds_n[mhx_hist_slot((double)x[u], lds_e, B, lo, hi, scale)], 1u);
    }
    // the rest of the chunk, one element at a time
    for (unsigned long long e = ef + sweeps * MHX_SELECT_THREADS * MHX_SELECT_UNROLL; e < e1; e += MHX_SELECT_THREADS) {
        const mhx_real x = *src;
        src += step; c += qc;
        if (c >= C) { c -= C; src += wrap; }
        atomicAdd(&lds_n[mhx_hist_slot((double)x, lds_e, B, lo, hi, scale)], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < B + 3; k += MHX_SELECT_THREADS) {
        const unsigned v = lds_n[k];
        if (v) atomicAdd(k < B ? &counts[(long)i * B + k] : &outside[(long)i * 3 + (k - B)], (unsigned long long)v);
    }
}

// grid (blocks per pair, pairs), block MHX_SELECT_THREADS.  Pair q reads the rows params[pairs[2 q]] and params[pairs[2 q + 1]] (slots
// into params, which also pick the edges: edges[slot (B + 1) ..]); every thread reads the same (t, c) element of both.
// counts[q][B][B], the first slot slowest; outside[q].  A thread keeps its outside draws in a register and adds them once.
// LDS: lds_e[2 (B + 1)] edges (first slot, then second), lds_n[B B + 1] counters (cells, then outside).
MHX_DEV void mhx_hist2d_body(const mhx_real* __restrict__ samples, const long N, const int d1, const long C,
                             const int* __restrict__ params, const double* __restrict__ edges, const int B,
                             const int* __restrict__ pairs, const unsigned long long chunk,
                             unsigned long long* __restrict__ counts, unsigned long long* __restrict__ outside, double* lds_e,
                             unsigned* lds_n)
{
    const int q = blockIdx.y;
    const int sa = pairs[2 * q], sb = pairs[2 * q + 1];
    const long pa = params[sa], pb = params[sb];
    const unsigned long long S = (unsigned long long)N * (unsigned long long)C;
    const unsigned long long e0 = (unsigned long long)blockIdx.x * chunk;
    if (e0 >= S) return;                                    // uniform over the block
    const unsigned long long e1 = e0 + chunk < S ? e0 + chunk : S;
    const int cells = B * B;
    for (int k = threadIdx.x; k <= cells; k += MHX_SELECT_THREADS) lds_n[k] = 0u;
    double* ea = lds_e;
    double* eb = lds_e + (B + 1);
    for (int k = threadIdx.x; k <= B; k += MHX_SELECT_THREADS) {
        ea[k] = edges[(long)sa * (B + 1) + k];
        eb[k] = edges[(long)sb * (B + 1) + k];
    }
    __syncthreads();
    const double alo = ea[0], ahi = ea[B], ascale = mhx_hist_scale(alo, ahi, B);
    const double blo = eb[0], bhi = eb[B], bscale = mhx_hist_scale(blo, bhi, B);
    const unsigned long long ef = e0 + threadIdx.x;
    const long t0 = (long)(ef / (unsigned long long)C);
    long c = (long)(ef - (unsigned long long)t0 * (unsigned long long)C);
    const long ld = (long)d1 * C;
    const long qt = MHX_SELECT_THREADS / C, qc = MHX_SELECT_THREADS - qt * C, step = qt * ld + qc, wrap = ld - C;
    const mhx_real* src = samples + pa * C + t0 * ld + c;
    const long other = (pb - pa) * C;                       // the second row's element, relative to the first's
    unsigned out = 0u;
    const unsigned long long sweeps = (e1 - e0) / ((unsigned long long)MHX_SELECT_THREADS * MHX_SELECT_UNROLL);
    for (unsigned long long it = 0; it < sweeps; ++it) {
        mhx_real x[MHX_SELECT_UNROLL], y[MHX_SELECT_UNROLL];
#pragma unroll
        for (int u = 0; u < MHX_SELECT_UNROLL; ++u) {
            x[u] = src[0];
            y[u] = src[other];
            src += step; c += qc;
            if (c >= C) { c -= C; src += wrap; }
        }
#pragma unroll
        for (int u = 0; u < MHX_SELECT_UNROLL; ++u) {
            const int ja = mhx_hist_slot((double)x[u], ea, B, alo, ahi, ascale), jb = mhx_hist_slot((double)y[u], eb, B, blo, bhi, bscale);
            if (ja < B && jb < B) atomicAdd(&lds_n[ja * B + jb], 1u); else ++out;
        }
    }
    for (unsigned long long e = ef + sweeps * MHX_SELECT_THREADS * MHX_SELECT_UNROLL; e < e1; e += MHX_SELECT_THREADS) {
        const mhx_real x = src[0], y = src[other];
        src += step; c += qc;
        if (c >= C) { c -= C; src += wrap; }
        const int ja = mhx_hist_slot((double)x, ea, B, alo, ahi, ascale), jb = mhx_hist_slot((double)y, eb, B, blo, bhi, bscale);
        if (ja < B && jb < B) atomicAdd(&lds_n[ja * B + jb], 1u); else ++out;
    }
    if (out) atomicAdd(&lds_n[cells], out);
    __syncthreads();
    for (int k = threadIdx.x; k <= cells; k += MHX_SELECT_THREADS) {
        const unsigned v = lds_n[k];
        if (v) atomicAdd(k < cells ? &counts[(long)q * cells + k] : &outside[q], (unsigned long long)v);
    }
}
MHX_NS_END
