// mhx_hpd_kernels.h -- highest-posterior-density intervals of the pooled draws of a parameter row.
//
// With y the ascending order of a row's S draws and m = max(1, ceil(alpha S)), the Chen-Shao interval reads the m smallest draws
// a = y[0:m] and the m largest b = y[S-m:S] only: i = the first argmin of b - a, interval [a[i], b[i]].  The radix select of
// mhx_diag_kernels.h gives the thresholds tL = y[m-1] and tU = y[S-m]; here
//   mhx_hpd_gather_body   ONE sweep of the [N][d1][C] tensor in place: the keys strictly below key(tL) go to the row's lower buffer,
//                         the keys strictly above key(tU) to its upper buffer (draws equal to a threshold are never stored: cL, cU <=
//                         m - 1 of them arrive, the counters say how many)
//   (the host sorts the two buffers of every row: rocPRIM radix sort of the unsigned keys)
//   mhx_hpd_argmin_body / mhx_hpd_final_body   the first minimum of b[i] - a[i] over i < m, a and b rebuilt from the sorted buffers,
//                         the thresholds and the counts
// Everything works on the select's own keys (mhx_order_key and its inverse mhx_key_value, mhx_device_math.h), so the order is the
// select's bit for bit.
#pragma once
#include "mhx_diag_kernels.h"

MHX_NS_BEGIN

// lanes of this wave below the calling lane whose bit is set in `mask`
MHX_DEV unsigned mhx_hpd_rank_in(const unsigned long long mask)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// counters live MHX_HPD_COUNT_STRIDE words apart: one 256-byte line each.  A returning atomic on one word runs at a fixed rate per
// line, and the 2 x rows counters of a batch packed into a handful of lines made that rate the whole sweep's
#define MHX_HPD_COUNT_STRIDE 32

// Both tails of one sweep of a wave: lane l holds lo[u] / hi[u] for its U keys.  Per tail the wave reserves sum_u popc(ballot(hit[u]))
// slots with ONE integer atomic (the lowest lane issues both tails' atomics back to back, one wait for the two; the bases travel by
// readfirstlane) and lane l stores key u at base + (hits of the elements before u) + (hits of element u in the lanes below l).
// Which slots a wave gets depends on the order of arrival; the buffer is sorted before anything reads it, and equal keys are
// indistinguishable, so nothing downstream does.  A slot at or above `cap` is never written.
MHX_DEV unsigned long long mhx_hpd_first_lane(const unsigned long long v)
{
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}
template <int U>
MHX_DEV void mhx_hpd_push(const mhx_key (&key)[U], const bool (&lo)[U], const bool (&hi)[U], unsigned long long* cntL,
                          unsigned long long* cntU, mhx_key* __restrict__ bufL, mhx_key* __restrict__ bufU, const unsigned long long cap)
{
    unsigned long long mL[U], mU[U];
    unsigned totL = 0, totU = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        mL[u] = __ballot(lo[u]); totL += (unsigned)__popcll(mL[u]);
        mU[u] = __ballot(hi[u]); totU += (unsigned)__popcll(mU[u]);
    }
    if (!(totL | totU)) return;                             // wave-uniform
    unsigned long long baseL = 0, baseU = 0;
    if (mhx_hpd_rank_in(~0ull) == 0u) {
        if (totL) baseL = atomicAdd(cntL, (unsigned long long)totL);
        if (totU) baseU = atomicAdd(cntU, (unsigned long long)totU);
    }
    baseL = mhx_hpd_first_lane(baseL);
    baseU = mhx_hpd_first_lane(baseU);
    unsigned beforeL = 0, beforeU = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned long long sL = baseL + beforeL + mhx_hpd_rank_in(mL[u]), sU = baseU + beforeU + mhx_hpd_rank_in(mU[u]);
        if (lo[u] && sL < cap) bufL[sL] = key[u];
        if (hi[u] && sU < cap) bufU[sU] = key[u];
        beforeL += (unsigned)__popcll(mL[u]);
        beforeU += (unsigned)__popcll(mU[u]);
    }
}

// grid (blocks per row, rows), block MHX_SELECT_THREADS: the geometry and the element-to-(t, c) map of mhx_select_hist_body.  Row i of
// the batch is row params[i] of the tensor; its thresholds are keyL[i], keyU[i]; its buffers are tails[(2 i) cap ..) (lower) and
// tails[(2 i + 1) cap ..) (upper), its counters count[(2 i) MHX_HPD_COUNT_STRIDE] and count[(2 i + 1) MHX_HPD_COUNT_STRIDE].  A row that
// needs no gather carries keyL = 0 and keyU = all ones: nothing is below the one or above the other.
MHX_DEV void mhx_hpd_gather_body(const mhx_real* __restrict__ samples, const long N, const int d1, const long C,
                                 const int* __restrict__ params, const unsigned long long* __restrict__ keyL,
                                 const unsigned long long* __restrict__ keyU, const unsigned long long chunk,
                                 const unsigned long long cap, unsigned long long* __restrict__ count, mhx_key* __restrict__ tails)
{
    const int i = blockIdx.y;
    const mhx_key kL = (mhx_key)keyL[i], kU = (mhx_key)keyU[i];
    if (kL == (mhx_key)0 && kU == (mhx_key)~(mhx_key)0) return;      // uniform over the block
    const long p = params[i];
    const unsigned long long S = (unsigned long long)N * (unsigned long long)C;
    const unsigned long long e0 = (unsigned long long)blockIdx.x * chunk;
    if (e0 >= S) return;
    const unsigned long long e1 = e0 + chunk < S ? e0 + chunk : S;
    unsigned long long* cntL = count + 2 * (long)i * MHX_HPD_COUNT_STRIDE;
    unsigned long long* cntU = cntL + MHX_HPD_COUNT_STRIDE;
    mhx_key* bufL = tails + (unsigned long long)(2 * (long)i) * cap;
    mhx_key* bufU = bufL + cap;
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
        mhx_key key[MHX_SELECT_UNROLL];
        bool lo[MHX_SELECT_UNROLL], hi[MHX_SELECT_UNROLL];
#pragma unroll
        for (int u = 0; u < MHX_SELECT_UNROLL; ++u) { key[u] = mhx_order_key(x[u]); lo[u] = key[u] < kL; hi[u] = key[u] > kU; }
        mhx_hpd_push<MHX_SELECT_UNROLL>(key, lo, hi, cntL, cntU, bufL, bufU, cap);
    }
    // the rest of the chunk, one element per thread and round: every lane of a wave takes part in the ballots, in range or not
    const unsigned long long rest0 = e0 + sweeps * MHX_SELECT_THREADS * MHX_SELECT_UNROLL;
    for (unsigned long long eb = rest0; eb < e1; eb += MHX_SELECT_THREADS) {
        const bool in = eb + threadIdx.x < e1;
        mhx_key key[1] = {(mhx_key)0};
        if (in) {
            key[0] = mhx_order_key(*src);
            src += step; c += qc;
            if (c >= C) { c -= C; src += wrap; }
        }
        const bool lo[1] = {in && key[0] < kL}, hi[1] = {in && key[0] > kU};
        mhx_hpd_push<1>(key, lo, hi, cntL, cntU, bufL, bufU, cap);
    }
}

// ---- the first minimum of b[i] - a[i] ----
// Of the m candidates only T = cL + (1 if cL < m - cU) + (m - max(cL, m - cU)) are looked at: on the plateau cL <= i < m - cU both
// ends are the thresholds, the width is one constant and only its first index can win.  Compact index j < T, ascending in i:
//   j < cL: i = j;   the plateau's first index i = cL where there is a plateau;   then i = max(cL, m - cU) ...  m - 1
// (2m > S, overlapping tails: cL + cU may exceed m, then there is no plateau and every i is a candidate).
struct mhx_hpd_row {
    unsigned long long m, cL, cU;                           // candidates; keys in the lower / upper buffer
    unsigned long long keyL, keyU;                          // the thresholds' keys
};

MHX_DEV unsigned long long mhx_hpd_candidates(const mhx_hpd_row& r)
{
    const unsigned long long edge = r.m - r.cU, start2 = edge > r.cL ? edge : r.cL;
    return r.cL + (r.cL < edge ? 1ull : 0ull) + (r.m - start2);
}
MHX_DEV unsigned long long mhx_hpd_candidate_index(const mhx_hpd_row& r, const unsigned long long j)
{
    if (j < r.cL) return j;
    const unsigned long long edge = r.m - r.cU, flat = r.cL < edge ? 1ull : 0ull;
    if (flat && j == r.cL) return r.cL;
    return (edge > r.cL ? edge : r.cL) + (j - r.cL - flat);
}
MHX_DEV void mhx_hpd_ends(const mhx_hpd_row& r, const mhx_key* __restrict__ low, const mhx_key* __restrict__ up,
                          const unsigned long long i, double* a, double* b)
{
    const unsigned long long edge = r.m - r.cU;
    *a = mhx_key_value(i < r.cL ? low[i] : (mhx_key)r.keyL);
    *b = mhx_key_value(i < edge ? (mhx_key)r.keyU : up[i - edge]);
}
// the order of numpy.argmin / Julia's findmin on (width, index): a NaN width before every number, then the smaller width, then the
// lower index.  A total order on distinct indices, so the minimum does not depend on how the reduction is bracketed.
MHX_DEV bool mhx_hpd_before(const double w1, const unsigned long long i1, const double w2, const unsigned long long i2)
{
    const bool n1 = w1 != w1, n2 = w2 != w2;
    if (n1 != n2) return n1;
    if (!n1 && w1 != w2) return w1 < w2;
    return i1 < i2;
}

#define MHX_HPD_ARGMIN_THREADS 256
#define MHX_HPD_ARGMIN_PER_BLOCK 1024                       // candidates a block takes at least (4 per thread)
#define MHX_HPD_NONE (~0ull)                                // the index of "no candidate": loses to every candidate

// grid (blocks per row, rows), block MHX_HPD_ARGMIN_THREADS: block (bx, i) reduces candidates [bx per, (bx + 1) per) of row i to
// part_w / part_i [i gridDim.x + bx] (index MHX_HPD_NONE where it has none).  red_w / red_i: one slot per wave of the block in LDS.
MHX_DEV void mhx_hpd_argmin_body(const mhx_hpd_row* __restrict__ rows, const mhx_key* __restrict__ tails, const unsigned long long cap,
                                 const unsigned long long per, double* __restrict__ part_w, unsigned long long* __restrict__ part_i,
                                 double* red_w, unsigned long long* red_i)
{
    const int i = blockIdx.y;
    const mhx_hpd_row r = rows[i];
    const mhx_key* low = tails + (unsigned long long)(2 * (long)i) * cap;
    const mhx_key* up = low + cap;
    const unsigned long long T = mhx_hpd_candidates(r);
    const unsigned long long j0 = (unsigned long long)blockIdx.x * per, j1 = j0 + per < T ? j0 + per : T;
    double bw = 0.0;
    unsigned long long bi = MHX_HPD_NONE;
    for (unsigned long long j = j0 + threadIdx.x; j < j1; j += MHX_HPD_ARGMIN_THREADS) {
        const unsigned long long idx = mhx_hpd_candidate_index(r, j);
        double a, b;
        mhx_hpd_ends(r, low, up, idx, &a, &b);
        const double w = b - a;
        if (bi == MHX_HPD_NONE || mhx_hpd_before(w, idx, bw, bi)) { bw = w; bi = idx; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ow = __shfl_down(bw, off, 64);
        const unsigned long long oi = __shfl_down(bi, off, 64);
        if (oi != MHX_HPD_NONE && (bi == MHX_HPD_NONE || mhx_hpd_before(ow, oi, bw, bi))) { bw = ow; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { red_w[threadIdx.x >> 6] = bw; red_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MHX_HPD_ARGMIN_THREADS / 64; ++w)
            if (red_i[w] != MHX_HPD_NONE && (bi == MHX_HPD_NONE || mhx_hpd_before(red_w[w], red_i[w], bw, bi))) { bw = red_w[w]; bi = red_i[w]; }
        part_w[(long)i * gridDim.x + blockIdx.x] = bw;
        part_i[(long)i * gridDim.x + blockIdx.x] = bi;
    }
}

// grid (rows), block 64: the blocks' partial minima of row i in block order, then out[2 i] = a[i*], out[2 i + 1] = b[i*]
MHX_DEV void mhx_hpd_final_body(const mhx_hpd_row* __restrict__ rows, const mhx_key* __restrict__ tails, const unsigned long long cap,
                                const int nblk, const double* __restrict__ part_w, const unsigned long long* __restrict__ part_i,
                                double* __restrict__ out)
{
    const int i = blockIdx.x;
    double bw = 0.0;
    unsigned long long bi = MHX_HPD_NONE;
    for (int k = threadIdx.x; k < nblk; k += 64) {
        const double ow = part_w[(long)i * nblk + k];
        const unsigned long long oi = part_i[(long)i * nblk + k];
        if (oi != MHX_HPD_NONE && (bi == MHX_HPD_NONE || mhx_hpd_before(ow, oi, bw, bi))) { bw = ow; bi = oi; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ow = __shfl_down(bw, off, 64);
        const unsigned long long oi = __shfl_down(bi, off, 64);
        if (oi != MHX_HPD_NONE && (bi == MHX_HPD_NONE || mhx_hpd_before(ow, oi, bw, bi))) { bw = ow; bi = oi; }
    }
    if (threadIdx.x == 0) {
        const mhx_hpd_row r = rows[i];
        const mhx_key* low = tails + (unsigned long long)(2 * (long)i) * cap;
        double a = 0.0, b = 0.0;
        if (bi != MHX_HPD_NONE) mhx_hpd_ends(r, low, low + cap, bi, &a, &b);   // (m >= 1: there always is a candidate)
        out[2 * (long)i] = a;
        out[2 * (long)i + 1] = b;
    }
}
MHX_NS_END
