// mhx_cross_kernels.h -- first and second cross moments of chosen rows of the device sample tensor [N][dim+1][C] (chain fastest)
// on the fp64 matrix cores.
//
// For rows p_0 .. p_{m-1} and a shift s_i per row, with y_{i,k} = fl64(x_{p_i,k} - s_i) over all K = N C draws k = (sample, chain):
//   sum[i] = sum_k y_{i,k}          cross[i][j] = sum_k y_{i,k} y_{j,k}
// X^T X over the draws is a SYRK with a very long K whose K index (the chain) is the contiguous one of the tensor, so the operands
// are read where they lie.  fp64 throughout in both engine widths: a Float32 draw is widened on load (exact).
//
// Lane map.  v_mfma_f64_16x16x4_f64 takes A[row = lane & 15][k = lane >> 4] and B[k = lane >> 4][col = lane & 15] -- the same map --
// so ONE register per lane holding y[row 16 I + (lane & 15)][k-slot lane >> 4] is at once the A operand of every tile (I, .) and
// the B operand of every tile (., I): a wave that keeps the G row tiles of a group in registers forms all tile pairs of the group
// without LDS.  The sum over k is order-free, so the draws are dealt to the k-slots such that a lane reads 16-byte pieces: a UNIT
// is CH = 4 E J consecutive chains of one sample; piece j of lane (row r, slot g) is the MHX_CROSS_E consecutive chains
// c0 + 4 E j + E g + e of its row (E = 2 doubles / 4 floats), and MFMA step (j, e) takes element e of piece j from every lane --
// i.e. k-slot g of that step is chain c0 + 4 E j + E g + e, for A and B alike.  The four lanes of a row read 64 contiguous bytes per
// piece, the J pieces of a unit 64 J contiguous bytes.
// C/D map (f64): col = lane & 15, row = (lane >> 4) + 4 reg.
//
// Padding is zero in y, not in x.  A padded row (tile rows past m) has no shift: its lanes read a block of zeros (one address at every
// unit: the lane's offset is masked to 0) and subtract 0, y = 0 - 0.  A padded k-slot (chains past C in the last unit of a sample)
// gets y = 0 by a select AFTER the subtraction, never 0 - s; the selects sit behind a wave-uniform branch that only that unit takes
// (kept a branch: the compiler would otherwise turn it into selects that every step of every unit pays for).  An entry (i, j)
// depends on rows i and j only; entries of padded rows are never written out.
//
// Schedule.  Units are dealt round-robin to the `nsplit` waves of a tile group (blockIdx.x); a wave keeps its accumulators for its
// whole share of K and stores them once as a partial (plain vector stores, no atomics); mhx_cross_fold then adds the partials
// in a fixed order -- bit-identical results from call to call.  The next unit's pieces are loaded before the current unit's MFMAs
// issue.  Only tiles I <= J are computed; the reduction mirrors them.  m <= 112: one group of G = ceil(m / 16) tiles, all
// G (G + 1) / 2 pairs in one wave (224 accumulator registers at G = 7).  Larger m: groups of 4 tiles; the DIAG form does the 10
// pairs inside a group, the OFF form the 16 pairs between two groups.
#pragma once
#include "mhx_device_math.h"

MHX_NS_BEGIN

typedef double mhx_cross_acc4 __attribute__((ext_vector_type(4)));
#define MHX_CROSS_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

#if MHX_REAL64
#define MHX_CROSS_E 2
typedef double mhx_cross_piece __attribute__((ext_vector_type(2)));
#else
#define MHX_CROSS_E 4
typedef float mhx_cross_piece __attribute__((ext_vector_type(4)));
#endif
// pieces per lane and unit: two, one where the accumulators of G tiles leave no room for four pieces in flight per tile
#define MHX_CROSS_J(G) 2
#define MHX_CROSS_CH(G) (4 * MHX_CROSS_E * MHX_CROSS_J(G))  // chains per unit: 8 or 16 (fp64), 16 or 32 (fp32)
#define MHX_CROSS_MAX_G 7                                   // row tiles one wave holds (DIAG form)
#define MHX_CROSS_SPLIT_G 4                                 // tiles per group when m needs more than MHX_CROSS_MAX_G

// the per-lane constants of one held tile: where its row starts, its shift, whether the row exists
template <int NT>
struct mhx_cross_rows {
    const mhx_real* base[NT];                               // the row's first draw; of a padded row: a block of zeros
    long mask[NT];                                          // all ones; of a padded row 0: its lanes read the zeros at every unit
    double s[NT];                                           // (of a padded row: 0, so that y = 0 - 0)
    bool rv[NT];
};

// the raw pieces of one unit (sample t, chains c0 .. c0 + CH - 1) for all held tiles; kmask bit (j E + e): that chain exists
template <int NT, int J>
MHX_DEV void mhx_cross_load(const long ld, const long C, const long t, const long c0, const int g,
                            const mhx_cross_rows<NT>& R, mhx_cross_piece (&raw)[NT][J], unsigned& kmask, bool& tail)
{
    constexpr int E = MHX_CROSS_E;
    tail = c0 + 4 * E * J > C;                           // wave-uniform
    const long at = t * ld + c0 + E * g;
    if (!tail) {
        kmask = ~0u;
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < J; ++j) {
                mhx_cross_piece v;
                __builtin_memcpy(&v, R.base[i] + (at & R.mask[i]) + 4 * E * j, sizeof v);
                raw[i][j] = v;
            }
    } else {
        kmask = 0u;
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (c0 + 4 * E * j + E * g + e < C) kmask |= 1u << (j * E + e);
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < J; ++j) {
                mhx_cross_piece v = {};
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (R.rv[i] && ((kmask >> (j * E + e)) & 1u)) v[e] = R.base[i][at + 4 * E * j + e];
                raw[i][j] = v;
            }
    }
}

// the E J MFMA steps of one unit.  DIAG: tiles 0 .. G-1 against themselves (pairs i <= j, row-major); else tiles 0 .. G-1 (A)
// against tiles G .. 2G-1 (B), all G G pairs.
template <int G, bool DIAG, int NT, int NP, int J>
MHX_DEV void mhx_cross_unit(const mhx_cross_rows<NT>& R, const mhx_cross_piece (&raw)[NT][J], const unsigned kmask, const bool tail,
                            mhx_cross_acc4 (&acc)[NP], double (&sum)[G])
{
    constexpr int E = MHX_CROSS_E;
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int e = 0; e < E; ++e) {
            double y[NT];
            const bool kv = ((kmask >> (j * E + e)) & 1u) != 0u;
#pragma unroll
            for (int i = 0; i < NT; ++i) y[i] = (double)raw[i][j][e] - R.s[i];
            if (tail) {                                     // wave-uniform, and kept a branch: full units skip the selects
                asm volatile("");
#pragma unroll
                for (int i = 0; i < NT; ++i) y[i] = (kv && R.rv[i]) ? y[i] : 0.0;
            }
            if (DIAG) {
#pragma unroll
                for (int i = 0; i < G; ++i) sum[i] += y[i];
            }
            int p = 0;
#pragma unroll
            for (int a = 0; a < G; ++a)
#pragma unroll
                for (int b = DIAG ? a : 0; b < G; ++b, ++p) acc[p] = MHX_CROSS_MFMA(y[a], y[DIAG ? b : G + b], acc[p]);
        }
}

// grid (nsplit, groups [DIAG] or group pairs a < b [OFF]), block 64.
//   rows / shift [ngroups G 16]: tensor row of every (padded) matrix row, -1 = padding; its shift (padding: 0)
//   zeros: 256 bytes of zeros, what the lanes of padded rows load
//   part [slot][nsplit][256]: slot = group * G(G+1)/2 + pair (DIAG), ngroups G(G+1)/2 + pair-of-groups * G G + a G + b (OFF);
//                             element reg * 64 + lane of the C/D fragment
//   psum [tile][nsplit][64]:  the lane's share of sum[row lane & 15 of the tile] (DIAG only)
template <int G, bool DIAG>
MHX_DEV void mhx_cross_body(const mhx_real* __restrict__ samples, const long N, const int d1, const long C, const int* __restrict__ rows,
                            const double* __restrict__ shift, const mhx_real* __restrict__ zeros, const int ngroups, double* __restrict__ part,
                            double* __restrict__ psum)
{
    constexpr int NT = DIAG ? G : 2 * G, NP = DIAG ? G * (G + 1) / 2 : G * G, J = MHX_CROSS_J(G), CH = MHX_CROSS_CH(G);
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const long nsplit = gridDim.x, split = blockIdx.x;
    int ta, tb;
    long slot0;
    if (DIAG) {
        ta = tb = (int)blockIdx.y * G;
        slot0 = (long)blockIdx.y * NP;
    } else {
        int a = 0, rem = (int)blockIdx.y;
        while (rem >= ngroups - 1 - a) { rem -= ngroups - 1 - a; ++a; }
        ta = a * G;
        tb = (a + 1 + rem) * G;
        slot0 = (long)ngroups * (G * (G + 1) / 2) + (long)blockIdx.y * NP;
    }
    mhx_cross_rows<NT> R;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int tile = i < G ? ta + i : tb + i - G;
        const int p = rows[tile * 16 + r];
        R.rv[i] = p >= 0;
        R.base[i] = p >= 0 ? samples + (long)p * C : zeros;
        R.mask[i] = p >= 0 ? -1L : 0L;
        R.s[i] = shift[tile * 16 + r];
    }
    constexpr mhx_cross_acc4 zero = {0.0, 0.0, 0.0, 0.0};
    mhx_cross_acc4 acc[NP];
    double sum[G];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = zero;
#pragma unroll
    for (int i = 0; i < G; ++i) sum[i] = 0.0;

    // unit u = sample t, chunk cc of U = ceil(C / CH); this wave's units are split, split + nsplit, ...
    const long ld = (long)d1 * C, U = (C + CH - 1) / CH, total = N * U;
    const long qt = nsplit / U, qc = nsplit - qt * U;
    long u = split, t = u / U, cc = u - t * U;
    // the pieces of the unit after the one in the MFMAs are in flight: loaded before those MFMAs issue
    mhx_cross_piece raw[NT][J], next[NT][J];
    unsigned km = 0u, km_next = 0u;
    bool tail = false, tail_next = false;
    if (u < total) mhx_cross_load<NT, J>(ld, C, t, cc * CH, g, R, next, km_next, tail_next);
    while (u < total) {
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < J; ++j) raw[i][j] = next[i][j];
        km = km_next; tail = tail_next;
        u += nsplit; t += qt; cc += qc;
        if (cc >= U) { cc -= U; ++t; }
        if (u < total) mhx_cross_load<NT, J>(ld, C, t, cc * CH, g, R, next, km_next, tail_next);
        mhx_cross_unit<G, DIAG, NT, NP, J>(R, raw, km, tail, acc, sum);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        double* dst = part + ((slot0 + p) * nsplit + split) * 256 + lane;
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[q * 64] = acc[p][q];
    }
    if (DIAG) {
#pragma unroll
        for (int i = 0; i < G; ++i) psum[((long)(ta + i) * nsplit + split) * 64 + lane] = sum[i];
    }
}

// grid (slots, W / 64), block (64, 16): src [slot][nsplit][W] -> dst [slot][W], the partials of every element added in a FIXED
// order -- thread (e, q) adds the splits q, q + 16, ... in four interleaved chains (so that four loads are in flight), the block
// then adds its 16 sums in the order of q -- whatever the grid of the kernel that wrote them: bit-identical from call to call.
MHX_DEV void mhx_cross_fold_body(const double* __restrict__ src, const int nsplit, const int W, double* __restrict__ dst, double* lds)
{
    const int e = threadIdx.x, q = threadIdx.y, el = blockIdx.y * 64 + e;
    const long slot = blockIdx.x;
    const double* p = src + slot * nsplit * W + el;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int s = q;
    for (; s + 48 < nsplit; s += 64) {
        a0 += p[(long)s * W];
        a1 += p[(long)(s + 16) * W];
        a2 += p[(long)(s + 32) * W];
        a3 += p[(long)(s + 48) * W];
    }
    for (; s < nsplit; s += 16) a0 += p[(long)s * W];
    lds[q * 64 + e] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (q == 0) {
        double v = 0.0;
        for (int k = 0; k < 16; ++k) v += lds[k * 64 + e];
        dst[slot * W + el] = v;
    }
}

// grid (slots), block 256: the (folded: nsplit = 1) partials of one tile pair, written to both halves of cross [m][m].
// tiles[slot] = (ti << 16) | tj with ti <= tj; of a diagonal tile only row <= col is written (and mirrored), so that cross is
// symmetric by construction.
MHX_DEV void mhx_cross_reduce_tiles_body(const double* __restrict__ part, const int* __restrict__ tiles, const int nsplit, const int m,
                                         double* __restrict__ cross)
{
    const long slot = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, reg = tid >> 6;
    const int ti = tiles[slot] >> 16, tj = tiles[slot] & 0xffff;
    const int row = (lane >> 4) + 4 * reg, col = lane & 15;
    const long i = (long)ti * 16 + row, j = (long)tj * 16 + col;
    if (i >= m || j >= m || (ti == tj && row > col)) return;
    const double* src = part + slot * nsplit * 256 + tid;
    double v = 0.0;
    for (int s = 0; s < nsplit; ++s) v += src[(long)s * 256];
    cross[i * m + j] = v;
    cross[j * m + i] = v;
}

// one thread per matrix row: the (folded: nsplit = 1) shares of the four k-slot lanes in order
MHX_DEV void mhx_cross_reduce_sums_body(const double* __restrict__ psum, const int nsplit, const int m, double* __restrict__ sum)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double* src = psum + (long)(i >> 4) * nsplit * 64 + (i & 15);
    double v = 0.0;
    for (int s = 0; s < nsplit; ++s)
        for (int g = 0; g < 4; ++g) v += src[(long)s * 64 + g * 16];
    sum[i] = v;
}
MHX_NS_END
