// mhx_acf_kernels.h -- autocovariance sums of the device sample tensor [N][dim+1][C] (chain fastest) at many lags in one sweep
// (include/mhx.h: mhx_run_autocovariance).
//
//   centre pass   per (chain, row): m_c = x_0 + sum(x_t - x_0) / N and ss_c = sum (x_t - m_c)^2, both fp64, stored [P][nc]
//   tile pass     a lane is a chain; a wave owns R consecutive lags k0 .. k0+R-1 of one row over one time chunk and keeps the R
//                 centred draws x[t+k0 .. t+k0+R-1] - m_c in registers: a step loads x[t] and the one draw that enters the window and
//                 performs R fused multiply-adds, so a multiply-add costs 2/R loads where the per-lag kernel of mhx_diag_kernels.h
//                 pays two.  The step loop is unrolled by R, so the window rotates by renaming.
// Arithmetic as mhx_diag_autocov_body fixes it: m_c rounded once to the run's width, products accumulated in that width, at most
// MHX_ACF_FLUSH fused steps in a row per accumulator before it is added to its fp64 partner.
#pragma once
#include "mhx_device_math.h"

MHX_NS_BEGIN

#define MHX_ACF_WAVES 4                 // waves of a block: adjacent lag tiles of the same 64 chains and the same time chunk
#define MHX_ACF_CHUNK 1024              // draws t of a time chunk: a multiple of MHX_ACF_FLUSH
#define MHX_ACF_FLUSH 512               // fused steps in a row per run-width accumulator; every tile width divides it

// grid (ceil(nc / 256), P), block 256: one thread per (chain of the range, row slot).  counters[slot] += chains with ss_c > 0,
// counters[P + slot] += chains with a non-finite draw (their m_c and ss_c are NaN, never +-inf)
MHX_DEV void mhx_acf_centre_body(const mhx_real* __restrict__ samples, const long N, const int d1, const long C,
                                 const int* __restrict__ params, const int P, const long c0, const long nc, double* __restrict__ mean,
                                 double* __restrict__ ss_out, unsigned long long* __restrict__ counters)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int slot = blockIdx.y;
    bool valid = false, bad = false;
    if (i < nc) {
        const mhx_real* s = samples + (long)params[slot] * C + c0 + i;
        const long stride = (long)d1 * C;
        // the mean about the first draw: a chain that never moved has m == x_0 and ss == 0 exactly, whatever x_0 is
        const double x0 = (double)s[0];
        double sum = 0.0;
        for (long t = 0; t < N; ++t) sum += (double)s[t * stride] - x0;
        double m = x0 + sum / (double)N;
        double ss = 0.0;
        for (long t = 0; t < N; ++t) { const double e = (double)s[t * stride] - m; ss += e * e; }
        bad = !(fabs(m) <= 1.7976931348623157e308) || !(ss <= 1.7976931348623157e308);
        if (bad) m = ss = __longlong_as_double(0x7ff8000000000000ll);
        valid = ss > 0.0;
        mean[(long)slot * nc + i] = m;
        ss_out[(long)slot * nc + i] = ss;
    }
    const unsigned long long nv = __popcll(__ballot(valid)), nb = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0) {
        if (nv) atomicAdd(&counters[slot], nv);
        if (nb) atomicAdd(&counters[P + slot], nb);
    }
}

// R steps t .. t+R-1 of a tile.  On entry w[j] = e[t + k0 + j] (e = x - m, 0 behind the series' end); on exit the same for t + R:
// step u reads lag j from w[(u + j) % R] and then puts e[t + u + k0 + R] where e[t + u + k0] was.  ZERO: the tile starts at lag 0,
// whose window entry IS e[t]: no load for it.  GUARD: the block overlaps the end of the chunk (t1) or of the series (N): draws
// behind either count as 0, per lag, which leaves an accumulator exactly as it was.
template <int R, bool ZERO, bool GUARD>
MHX_DEV void mhx_acf_steps(const mhx_real* __restrict__ pa, const mhx_real* __restrict__ pn, const long ld, const mhx_real m,
                           const long t, const long t1, const long s, const long N, mhx_real (&w)[R], mhx_real (&acc)[R])
{
#pragma unroll
    for (int u = 0; u < R; ++u) {
        mhx_real a;
        if (ZERO) a = (!GUARD || t + u < t1) ? w[u] : MHX_R(0.0);
        else a = (!GUARD || t + u < t1) ? pa[u * ld] - m : MHX_R(0.0);
#pragma unroll
        for (int j = 0; j < R; ++j) acc[j] = mhx_fma(a, w[(u + j) % R], acc[j]);
        w[u] = (!GUARD || s + u < N) ? pn[u * ld] - m : MHX_R(0.0);
    }
}

template <int R, bool ZERO>
MHX_DEV void mhx_acf_chunk(const mhx_real* __restrict__ base, const long ld, const mhx_real m, const long N, const long k0,
                           const long t0, const long t1, double (&dacc)[R])
{
    mhx_real w[R], acc[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        acc[j] = MHX_R(0.0);
        w[j] = t0 + k0 + j < N ? base[(t0 + k0 + j) * ld] - m : MHX_R(0.0);
    }
    int fused = 0;
    for (long t = t0; t < t1; t += R) {
        const long s = t + k0 + R;                          // the first draw that enters the window in this block
        const mhx_real* pa = base + t * ld;
        // behind the series' end nothing is addressed: the guarded form does not load there
        const mhx_real* pn = base + s * ld;
        if (t + R <= t1 && s + R <= N) mhx_acf_steps<R, ZERO, false>(pa, pn, ld, m, t, t1, s, N, w, acc);
        else mhx_acf_steps<R, ZERO, true>(pa, pn, ld, m, t, t1, s, N, w, acc);
        fused += R;
        if (fused == MHX_ACF_FLUSH) {
#pragma unroll
            for (int j = 0; j < R; ++j) { dacc[j] += (double)acc[j]; acc[j] = MHX_R(0.0); }
            fused = 0;
        }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) dacc[j] += (double)acc[j];
}

// grid (chain blocks x tile groups x P, time chunks), block 64 x MHX_ACF_WAVES.  blockIdx.x = (slot * ngroups + group) * ncb + cb.
// Wave v of a block owns tile `group * MHX_ACF_WAVES + v` of the list `tiles` (tile starts, multiples of R, increasing), chains
// c0 + 64 cb + lane and draws t in [chunk * MHX_ACF_CHUNK, +MHX_ACF_CHUNK) below N - k0.
// out[(slot * ntiles + tile) * R + j] += sum_c f_c sum_t (x_t - m_c)(x_{t+k0+j} - m_c), f_c = 1, or 1 / ss_c (0 where ss_c == 0) in the
// normalised mode: the fp64 partials of the 64 lanes are added by shuffles, then ONE fp64 atomic per (lag, wave).
template <int R>
MHX_DEV void mhx_acf_tile_body(const mhx_real* __restrict__ samples, const long N, const int d1, const long C,
                               const int* __restrict__ params, const long c0, const long nc, const int* __restrict__ tiles,
                               const int ntiles, const int ngroups, const long ncb, const int normalise,
                               const double* __restrict__ mean, const double* __restrict__ ss, double* __restrict__ out)
{
    static_assert(MHX_ACF_FLUSH % R == 0 && MHX_ACF_CHUNK % MHX_ACF_FLUSH == 0, "tile width");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long bx = blockIdx.x;
    const long cb = bx % ncb, rest = bx / ncb;
    const int group = (int)(rest % ngroups), slot = (int)(rest / ngroups);
    const int tile = group * MHX_ACF_WAVES + wave;
    if (tile >= ntiles) return;                             // uniform over the wave; the block shares nothing
    const long k0 = tiles[tile];
    const long t0 = (long)blockIdx.y * MHX_ACF_CHUNK;
    const long t1 = t0 + MHX_ACF_CHUNK < N - k0 ? t0 + MHX_ACF_CHUNK : N - k0;
    if (t0 >= t1) return;
    const long i = cb * 64 + lane;
    const bool live = i < nc;
    const long ic = live ? i : nc - 1;                      // an idle lane reads the range's last chain and adds nothing
    const mhx_real* base = samples + (long)params[slot] * C + c0 + ic;
    const long ld = (long)d1 * C;
    const mhx_real m = (mhx_real)mean[(long)slot * nc + ic];
    double dacc[R];
#pragma unroll
    for (int j = 0; j < R; ++j) dacc[j] = 0.0;
    if (k0 == 0) mhx_acf_chunk<R, true>(base, ld, m, N, k0, t0, t1, dacc);
    else mhx_acf_chunk<R, false>(base, ld, m, N, k0, t0, t1, dacc);
    double f = live ? 1.0 : 0.0;
    if (normalise && live) { const double q = ss[(long)slot * nc + ic]; f = q == 0.0 ? 0.0 : 1.0 / q; }
    double* o = out + ((long)slot * ntiles + tile) * R;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        double x = f == 0.0 ? 0.0 : dacc[j] * f;            // a lane that adds nothing adds +0, whatever its chain holds
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if (lane == 0 && k0 + j < N) atomicAdd(&o[j], x);
    }
}
MHX_NS_END
