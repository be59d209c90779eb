// mhx_derive_kernels.h -- derived quantities: every saved draw of a sample tensor mapped through a user function, one lane per
// chain (include/mhx.h: mhx_run_derive / mhx_ctx_derive).
//
// What a user reports is rarely a raw parameter: sigma^2, exp(beta[3]), mu[1] - mu[0], an indicator theta > 0, a fitted mean at a
// new x -- MCMCChains' one-liners on a Chains object, Turing's generated_quantities.  This frame applies such a map (MHX_DERIVED,
// inlined) to the tensor where it lies and writes a tensor of the same kind, which every post-run statistic then reads:
//   source  [N][d + 1][C]     rows 0 .. d-1 the parameters, row d the draw's lp
//   result  [N][K + 1][C]     rows 0 .. K-1 the map's outputs, row K the source's lp row, copied in the same pass
// Compiled at run time only (the map is user source), once per (source, K, width, draws per lane).
//
// Work layout.  A block is 256 lanes = 256 consecutive chains, and covers a strip of MHX_DERIVE_STRIP consecutive draws; rows of
// both tensors are contiguous over chains, so every load and every store of a wave is one whole coalesced row segment of 64 reals.
// A lane maps MHX_JIT_DERIVE_DRAWS draws of its strip at a time: the map is called for each of them before anything is stored, so
// the loads of all of them are independent and may be in flight together.  4 draws by measurement (on the
// [250][101][65536] tensor every map tried runs at 0.98 to 1.08 of a device copy's rate with 4, while a map of 100 rows falls to
// 0.46 - 0.61 of it with 1 or 2 in fp64); the host lowers the count for many outputs (mhx_api_derive.inc).
//   x[k]        a load of row k of the draw, issued where the source names it: a map that names 3 of 100 rows reads 3 rows.  The
//               traced form (mhx.trace_map) names every row once, by a compile-time index; a row named twice is one load (the
//               tensor is __restrict__ and nothing is stored before the map returns).  k is clamped to [0, d]: x[d] is lp, and a
//               hand-written index beyond it reads lp instead of memory that is not the tensor's.
//   y.set(j, v) a register array indexed at compile time in the traced form; j outside [0, K) is ignored; an output that is not set
//               stays NaN.  The K + 1 rows are stored after the call.
// Addressing.  Draw, row and chain-block offsets are 64-bit element offsets into plain pointers and wave-uniform (scalar
// registers).  The only 32-bit offset is the lane's byte offset inside its block's 256 chains (< 2048), so no shape has to be
// refused, or take another form, because (d + 1) C sizeof(real) does not fit 32 bits.
// Bounds.  A lane whose chain is not below C leaves at once (no barrier follows); draws are bounded by N in both loops.
//
// Predictive maps (MHX_HAVE_PREDICTIVE: mhx_run_predict / mhx_ctx_predict; DESIGN.md sections 3.16 and 6.5.6).  The same frame with a
// second entry, mhx_jit_predict, whose map (MHX_PREDICTIVE) also gets `rng`, the stream of its (chain, saved draw): the key schedule of
// seed ^ MHX_PREDICT_SALT, computed once per kernel (wave-uniform: scalar registers), the lane's global chain id first_id + chain and
// the draw's index t.  rng.draw / rng.gamma build the parameter row of mhx_fam_comp and call mhx_fam_valid / mhx_fam_normal /
// mhx_fam_draw: the family arithmetic is that of the samplers, not a copy.  The Gamma attempt loop runs `while (__ballot(!done))`:
// the lanes beyond C have left before the first map and t is wave-uniform in the group path and in the ragged-end path alike, so
// every lane that is in the frame reaches every draw of the map together.
#pragma once
#include "mhx_device_math.h"

#define MHX_DERIVE_THREADS 256
#ifndef MHX_JIT_DERIVE_DRAWS
#define MHX_JIT_DERIVE_DRAWS 4          // draws a lane maps together
#endif
#ifndef MHX_DERIVE_ROUNDS
#define MHX_DERIVE_ROUNDS 2             // such groups per strip
#endif
#define MHX_DERIVE_STRIP (MHX_JIT_DERIVE_DRAWS * MHX_DERIVE_ROUNDS)
#ifndef MHX_DERIVE_MIN_WAVES
#define MHX_DERIVE_MIN_WAVES 1          // waves per SIMD the register allocation must leave room for
#endif

#if defined(MHX_HAVE_DERIVED) || defined(MHX_HAVE_PREDICTIVE)
MHX_NS_BEGIN

// (one draw as the map reads it: mhx_derive_in, mhx_device_math.h)

// the outputs of one draw
template <int K>
struct mhx_derive_out {
    mhx_real* y;
    MHX_DEV void set(const int j, const mhx_real v) const
    {
        if ((unsigned)j < (unsigned)K) y[j] = v;
    }
};

// what the derive entry passes where the predictive entry passes its streams
struct mhx_no_rng { static constexpr bool none = true; };

// draws t .. t + U - 1 of the block's chains: every map first, then every store
template <int K, int U, class RNG>
MHX_DEV void mhx_derive_draws(const mhx_real* __restrict__ src, mhx_real* __restrict__ dst, const long t, const long C, const int d,
                              const long c0, const mhx_u32 lane, const mhx_real* __restrict__ data, const int ndata, const RNG& rng)
{
    mhx_real y[U][K + 1];
    // C and the lane offset are made opaque here, once per group: the row addresses are then formed per load as a scalar base plus
    // the lane's 32-bit offset (the scalar-base addressing mode), not hoisted out of the strip loop as one 64-bit vector pointer per
    // named row and draw (a map of 100 rows: hundreds of registers held across the loop)
    long ld = C;                                            // (C is a kernel argument: ld must stay wave-uniform, it lives in SGPRs)
    mhx_u32 l = lane;
    asm volatile("" : "+s"(ld), "+v"(l));
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int j = 0; j < K; ++j) y[u][j] = MHX_NAN;
        const mhx_derive_in x = {src + (t + u) * (long)(d + 1) * ld + c0, ld, d, l};
        if constexpr (RNG::none) mhx_user_derived(x, mhx_derive_out<K>{y[u]}, d, data, ndata);
        else mhx_user_predictive(x, rng.at(t + u), mhx_derive_out<K>{y[u]}, d, data, ndata);
        y[u][K] = x[d];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        mhx_real* row = dst + (t + u) * (long)(K + 1) * ld + c0;
#pragma unroll
        for (int j = 0; j <= K; ++j) mhx_st_off(row + (long)j * ld, l, y[u][j]);
    }
}

template <int K, int U, class RNG>
MHX_DEV void mhx_derive_body(const mhx_real* __restrict__ src, mhx_real* __restrict__ dst, const long N, const long C, const int d,
                             const mhx_real* __restrict__ data, const int ndata, const RNG& rng)
{
    const long c0 = (long)blockIdx.x * MHX_DERIVE_THREADS;
    if (c0 + (long)threadIdx.x >= C) return;
    const mhx_u32 lane = (mhx_u32)threadIdx.x * MHX_RB;
    const long nstrips = (N + MHX_DERIVE_STRIP - 1) / MHX_DERIVE_STRIP;
    for (long s = blockIdx.y; s < nstrips; s += gridDim.y) {         // (a grid's y extent ends at 65535 strips)
        long t = s * MHX_DERIVE_STRIP;
        const long end = t + MHX_DERIVE_STRIP < N ? t + MHX_DERIVE_STRIP : N;
        for (; t + U <= end; t += U) mhx_derive_draws<K, U>(src, dst, t, C, d, c0, lane, data, ndata, rng);
        if constexpr (U > 1)                                                                             // the ragged end of the tensor
            for (; t < end; ++t) mhx_derive_draws<K, 1>(src, dst, t, C, d, c0, lane, data, ndata, rng);
    }
}

#ifdef MHX_HAVE_DERIVED
extern "C" __global__ void __launch_bounds__(MHX_DERIVE_THREADS, MHX_DERIVE_MIN_WAVES)
mhx_jit_derive(const mhx_real* __restrict__ src, mhx_real* __restrict__ dst, const long N, const long C, const int d,
               const mhx_real* __restrict__ data, const int ndata)
{
    mhx_derive_body<MHX_JIT_DERIVE_NOUT, MHX_JIT_DERIVE_DRAWS>(src, dst, N, C, d, data, ndata, mhx_no_rng{});
}
#endif

#ifdef MHX_HAVE_PREDICTIVE
// the stream of one (chain, saved draw): what MHX_PREDICTIVE's `rng` is (the calls are documented at the macro, mhx_device_math.h)
struct mhx_predict_rng {
    const mhx_philox_key& ks;   // of seed ^ MHX_PREDICT_SALT (wave-uniform)
    mhx_u32 id_lo, id_hi;       // the lane's global chain id
    mhx_u32 t;                  // index of the saved draw (wave-uniform)
    MHX_DEV mhx_real row(const int k, const int family, const mhx_real* p) const
    {
        mhx_real nk = MHX_R(0.0);
        if (family == MHX_FAMILY_NORMAL) nk = mhx_fam_normal(mhx_philox(ks, id_lo, id_hi, t, (MHX_STREAM_FAMILY << 28) | (mhx_u32)k));
        const mhx_real v = mhx_fam_draw(family, p, nk, ks, id_lo, id_hi, t, MHX_STREAM_FAMILY, (mhx_u32)k);
        return mhx_fam_valid(family, p) ? v : MHX_NAN;
    }
    MHX_DEV mhx_real draw(const int k, const int family, const mhx_real p0, const mhx_real p1) const
    {
        const mhx_real p[6] = {p0, p1, p1 - p0, MHX_R(0.0), MHX_R(0.0), MHX_R(0.0)};       // (p[2]: Uniform's b - a, in the width)
        return row(k, family, p);
    }
    MHX_DEV mhx_real gamma(const int k, const int family, const mhx_real alpha, const mhx_real theta, const mhx_real d, const mhx_real c,
                           const mhx_real inva) const
    {
        const mhx_real p[6] = {alpha, theta, d, c, inva, MHX_R(0.0)};
        return row(k, family, p);
    }
};

// the streams of one lane: what the frame carries, `at(t)` the stream of saved draw t
struct mhx_predict_streams {
    static constexpr bool none = false;
    const mhx_philox_key& ks;
    mhx_u32 id_lo, id_hi;
    MHX_DEV mhx_predict_rng at(const long t) const { return mhx_predict_rng{ks, id_lo, id_hi, (mhx_u32)t}; }
};

extern "C" __global__ void __launch_bounds__(MHX_DERIVE_THREADS, MHX_DERIVE_MIN_WAVES)
mhx_jit_predict(const mhx_real* __restrict__ src, mhx_real* __restrict__ dst, const long N, const long C, const int d,
                const mhx_real* __restrict__ data, const int ndata, const mhx_u64 seed, const mhx_u64 first_id)
{
    const mhx_philox_key ks = mhx_philox_schedule(seed ^ MHX_PREDICT_SALT);
    const mhx_u64 id = first_id + (mhx_u64)blockIdx.x * MHX_DERIVE_THREADS + threadIdx.x;
    mhx_derive_body<MHX_JIT_DERIVE_NOUT, MHX_JIT_DERIVE_DRAWS>(src, dst, N, C, d, data, ndata,
                                                               mhx_predict_streams{ks, (mhx_u32)id, (mhx_u32)(id >> 32)});
}
#endif

MHX_NS_END
#endif
