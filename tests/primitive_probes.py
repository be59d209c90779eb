"""The probe that evaluates any function of mhx_device_math.h at any input, and the inputs it is given (no GPU needed here).

A user log-density is compiled behind `#include "mhx_device_math.h"` and `mhx.logdensity(model, x)` evaluates it at the columns
of x, so `PROBE` -- one MHX_LOGDENSITY source for both widths whose body switches on data[0] -- returns any device function of the
arithmetic spec at any argument (tests/test_gpu_primitives.py).  Integer arguments (Philox words, hi:lo angles) travel as 16-bit
limbs, one per coordinate and each a small exactly representable real: `words_to_x` splits them, the probe recombines them with
(mhx_u32)x[k].  A function with two outputs takes a selector in the last coordinate.

The input generators below return numpy arrays from fixed seeds.  `dt` is "f32" or "f64" throughout.

Near-midpoint square roots (`sqrt_midpoint_cases`).  Let p be the precision (24 / 53) and M an odd (p+1)-bit integer: M / 2 is the
midpoint of two neighbouring p-bit significands.  If M^2 = r (mod 2^(p+1)) for M^2 < 2^(2p+1), or (mod 2^(p+2)) above -- the power
of two that leaves X = (M^2 - r) / 4 a p-bit significand times a power of two -- then x = X 2^(2 - 2p) in [1, 4) is representable and
sqrt(x) = (M / 2) sqrt(1 - r / M^2) 2^(1-p) lies |r| / (4 M) ulp from the midpoint, below it iff r > 0.  M odd forces r = 1 (mod 8);
each such r has four square roots modulo a power of two, found by Hensel lifting from 1, 3, 5, 7 (mod 8): a root m (mod 2^k) lifts
to m or m + 2^(k-1) (mod 2^(k+1)).  |r| < 1600 gives a few hundred cases per width and exponent parity, each within 2.4e-5 ulp.

Near-midpoint quotients (`div_midpoint_cases`).  B a random odd p-bit integer, r small and odd, M = r B^-1 (mod 2^(p+1)): when M has
p+1 bits and A = (M B - r) / 2^(p+1) has p, A / B = (M / 2 - r / (2 B)) 2^-p lies |r| / (2 B) <= |r| 2^-p ulp from the midpoint M / 2
of two p-bit significands, below it iff r > 0.

Both constructions come with the correctly rounded answer from the sign of r alone -- exact integer arithmetic, no floating point.
"""
import contextlib
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_MATH_H = os.path.join(ROOT, "advancedmh.jl_amd", "csrc", "mhx_device_math.h")
TARGETS_H = os.path.join(ROOT, "advancedmh.jl_amd", "csrc", "mhx_targets.h")

# ---- the probe -------------------------------------------------------------------------------------------------------------------
(F_LOG, F_LOG_SEL, F_LOG_POS, F_EXP, F_SQRT_NORMAL, F_DIV_NORMAL, F_LOG_CORE_DIV, F_SINCOS, F_U01_OPEN, F_U01_HALF, F_NORMAL_PAIR,
 F_FAM_U_OPEN2, F_CAUCHY_QUOTIENT) = range(13)

PROBE = r"""
MHX_LOGDENSITY(x, d, data, ndata)
{
    // words 0 .. 3 from the limbs x[0] .. x[d - 2] (high limb first), the selector of a two-output function from x[d - 1]
    mhx_u32 w[4] = {0u, 0u, 0u, 0u};
    const int nw = (d - 1) / 2;
    for (int j = 0; j < 4; ++j)
        if (j < nw) w[j] = ((mhx_u32)x[2 * j] << 16) | (mhx_u32)x[2 * j + 1];
    const bool second = nw > 0 && x[d - 1] != MHX_R(0.0);
    mhx_u32x4 blk; blk.x = w[0]; blk.y = w[1]; blk.z = w[2]; blk.w = w[3];
    mhx_real s, c;
    switch ((int)data[0]) {
    case 0: return mhx_log(x[0]);
    case 1: return mhx_log_sel(x[0]);
    case 2: return mhx_log_pos(x[0]);
    case 3: return mhx_exp(x[0]);
    case 4: return mhx_sqrt_normal(x[0]);
#if MHX_REAL64
    case 5: return mhx_div_normal(x[0], x[1]);
    case 6: { const double f = x[0] - 1.0; return mhx_div_normal(f, 2.0 + f); }        // the division of mhx_log_core, from its m
    case 7: mhx_sincos2pi_u64(w[0], w[1], s, c); return second ? c : s;
    case 8: return mhx_u01_open(w[0], w[1]);
    case 9: return mhx_u01_half(w[0], w[1]);
    case 10: mhx_normal_pair(blk, s, c); return second ? c : s;                          // (n0, n1)
#else
    case 7: mhx_sincos2pi_u32(w[0], s, c); return second ? c : s;
    case 8: return mhx_u01_open(w[0]);
    case 9: return mhx_u01_half(w[0]);
    case 10: mhx_normal_pair(w[0], w[1], s, c); return second ? c : s;
#endif
    case 11: return mhx_fam_u_open2(blk);
    case 12: mhx_fam_phase(blk, s, c); return s / c;                                     // the quotient of the Cauchy draw
    default: return MHX_NAN;
    }
}
"""


def words_to_x(words, selector=None):
    """integer words [nwords][n] (each < 2^32) -> the probe's coordinates [2 nwords + 1][n] in float64: 16-bit limbs, high limb
    first, then the selector (0: first output, 1: second)"""
    words = np.atleast_2d(np.asarray(words, dtype=np.uint64))
    nw, n = words.shape
    assert (words < 2 ** 32).all()
    x = np.empty((2 * nw + 1, n), dtype=np.float64)
    x[0:2 * nw:2] = (words >> np.uint64(16)).astype(np.float64)
    x[1:2 * nw:2] = (words & np.uint64(0xffff)).astype(np.float64)
    x[2 * nw] = 0.0 if selector is None else selector
    return x


# ---- widths ----------------------------------------------------------------------------------------------------------------------
class Width:
    def __init__(self, dt):
        self.dt = dt
        self.real = np.float64 if dt == "f64" else np.float32
        self.uint = np.uint64 if dt == "f64" else np.uint32
        self.p = 53 if dt == "f64" else 24                     # precision
        self.mant = self.p - 1                                 # explicit mantissa bits
        self.one = 0x3ff0000000000000 if dt == "f64" else 0x3f800000
        self.tiny = 1 << self.mant                             # bits of the smallest normal
        self.inf = 0x7ff0000000000000 if dt == "f64" else 0x7f800000
        self.sign = 1 << (63 if dt == "f64" else 31)
        self.qnan = self.inf | (1 << (self.mant - 1))
        self.log_split = 0x3fe6a09e667f3bcd if dt == "f64" else 0x3f2aaaab     # where mhx_log splits mantissa from exponent
        self.emin = -1022 if dt == "f64" else -126
        # the cut-offs of mhx_exp, as written in mhx_device_math.h and oracle/mhx_oracle.c
        self.exp_hi_text, self.exp_lo_text = (("0x1.62e42fefa39efp+9", "-0x1.74910d52d3052p+9") if dt == "f64"
                                              else ("0x1.62e42ep+6", "-0x1.9fe368p+6"))
        self.exp_hi, self.exp_lo = float.fromhex(self.exp_hi_text), float.fromhex(self.exp_lo_text)
        self.log2e = float.fromhex("0x1.71547652b82fep+0" if dt == "f64" else "0x1.715476p+0")

    def from_bits(self, b):
        return np.asarray(b, dtype=self.uint).view(self.real)

    def to_bits(self, v):
        return np.ascontiguousarray(v, dtype=self.real).view(self.uint)

    def neighbours(self, v, k):
        """v and its k neighbours on each side (v finite, not within k ulp of zero)"""
        b = int(self.to_bits([v])[0])
        return self.from_bits([b + j for j in range(-k, k + 1)])


@contextlib.contextmanager
def oracle_width(dt):
    from oracle import oracle as O
    old = O.get_dtype()
    O.set_dtype(dt)
    try:
        yield O
    finally:
        O.set_dtype(old)


def orc_map(name, a, dt):
    """the oracle's scalar export `name` (orc_log, orc_exp) over an array, in width dt"""
    with oracle_width(dt) as O:
        f = getattr(O.lib(), name)
        return np.array([f(v) for v in np.asarray(a, dtype=np.float64).tolist()], dtype=O.real())


def orc_sincos(words, dt):
    """oracle.sincos2pi_u64 / _u32 over an array of angle words -> (sin[], cos[])"""
    with oracle_width(dt) as O:
        L = O.lib()
        cr = C.c_double if dt == "f64" else C.c_float
        s, c = cr(), cr()
        ps, pc = C.byref(s), C.byref(c)
        out = np.empty((2, len(words)), dtype=O.real())
        if dt == "f64":
            f = L.orc_sincos2pi_u64
            f.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
            for i, a in enumerate(np.asarray(words, dtype=np.uint64).tolist()):
                f(a >> 32, a & 0xffffffff, ps, pc)
                out[0, i], out[1, i] = s.value, c.value
        else:
            f = L.orc_sincos2pi_u32
            f.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
            for i, a in enumerate(np.asarray(words, dtype=np.uint64).tolist()):
                f(a, ps, pc)
                out[0, i], out[1, i] = s.value, c.value
        return out[0], out[1]


def orc_u01(which, words, dt):
    """oracle.u01_open / u01_half over uniform words: [2][n] (hi, lo) in f64, [1][n] in f32"""
    with oracle_width(dt) as O:
        f = getattr(O.lib(), "orc_u01_" + which)
        cols = np.atleast_2d(np.asarray(words, dtype=np.uint64)).T.tolist()
        return np.array([f(*w) for w in cols], dtype=O.real())


# ---- log -------------------------------------------------------------------------------------------------------------------------
def log_edges(dt):
    """positive finite arguments at the edges of mhx_log: subnormals, the smallest normal, 1, the mantissa split point, max"""
    W = Width(dt)
    bits = [1, 2, 3, 5, 1000, W.tiny - 1]                                           # k * smallest; the last has a full mantissa
    bits += [W.tiny, W.tiny + 1]                                                     # (tiny's lower neighbour is that last one)
    bits += [W.one + j for j in range(-8, 9)]
    for e in (-40, 0, 1):                                                            # the split point in three binades
        bits += [W.log_split + (e << W.mant) + j for j in (-2, -1, 0, 1, 2)]
    bits += [W.inf - 1]
    return W.from_bits(bits)


def log_specials(dt):
    """+inf, -inf, +-0, -tiny, -1, a quiet NaN of each sign"""
    W = Width(dt)
    return W.from_bits([W.inf, W.sign | W.inf, 0, W.sign, W.sign | W.tiny, W.sign | W.one, W.qnan, W.sign | W.qnan])


def log_random(dt, n=2 ** 20):
    """uniformly random finite positive bit patterns"""
    W = Width(dt)
    return W.from_bits(np.random.default_rng(20261).integers(1, W.inf, n, dtype=np.uint64))


def log_inputs(dt, n_random=2 ** 20):
    return np.concatenate([log_edges(dt), log_specials(dt), log_random(dt, n_random)])


def positive_normal(dt, a):
    W = Width(dt)
    b = W.to_bits(a)
    return a[(b >= W.tiny) & (b < W.inf)]


# ---- exp -------------------------------------------------------------------------------------------------------------------------
def exp_edges(dt):
    """6 neighbours on each side of each cut-off, 2^12 arguments with subnormal results, the arguments where rint(x LOG2E)
    changes parity near 0, +-0, +-eps, +-smallest"""
    W = Width(dt)
    R = W.real
    parts = [W.neighbours(W.exp_hi, 6), W.neighbours(W.exp_lo, 6)]
    log_tiny = np.log(np.ldexp(1.0, W.emin))
    parts.append(np.linspace(W.exp_lo, log_tiny, 2 ** 12).astype(R))
    for j in range(-3, 3):                                                           # x LOG2E = j + 1/2
        parts.append(W.neighbours(R((j + 0.5) / W.log2e), 3))
    eps = np.finfo(R).eps
    parts.append(np.array([0.0, -0.0, eps, -eps], dtype=R))
    parts.append(W.from_bits([1, W.sign | 1]))
    return np.concatenate(parts)


def exp_specials(dt):
    W = Width(dt)
    return W.from_bits([W.inf, W.sign | W.inf, W.qnan, W.sign | W.qnan])


def exp_random(dt, n=2 ** 20):
    W = Width(dt)
    return np.random.default_rng(20262).uniform(W.exp_lo, W.exp_hi, n).astype(W.real)


def exp_inputs(dt, n_random=2 ** 20):
    return np.concatenate([exp_edges(dt), exp_specials(dt), exp_random(dt, n_random)])


# ---- near-midpoint square roots and quotients ------------------------------------------------------------------------------------
def sqrt_roots_mod_pow2(r, k):
    """the four square roots of r = 1 (mod 8) modulo 2^k (k >= 3), by Hensel lifting from the roots modulo 8"""
    assert r % 8 == 1 and k >= 3
    roots = set()
    for m in (1, 3, 5, 7):
        # a root m modulo 2^j lifts to m or m + 2^(j-1) modulo 2^(j+1)
        for j in range(3, k):
            if (m * m - r) % (1 << (j + 1)):
                m += 1 << (j - 1)
            assert (m * m - r) % (1 << (j + 1)) == 0
        roots.add(m % (1 << k))
        roots.add((-m) % (1 << k))
        roots.add((m + (1 << (k - 1))) % (1 << k))
        roots.add((-m + (1 << (k - 1))) % (1 << k))
    roots = sorted(m for m in roots if (m * m - r) % (1 << k) == 0)
    assert len(roots) == 4
    return roots


def sqrt_midpoint_cases(p, parity, rmax=1600):
    """[(M, r)]: odd (p+1)-bit M with M^2 = r (mod 2^(p+1+parity)), |r| < rmax, r = 1 (mod 8); parity 0: M^2 < 2^(2p+1) (x in
    [1, 2)), parity 1: above (x in [2, 4)).  x = (M^2 - r) / 4 * 2^(2 - 2p), sqrt(x) within |r| / (4 M) ulp of M / 2 * 2^(1 - p)."""
    k = p + 1 + parity
    out = []
    for r in range(-rmax + 1, rmax):
        if r % 8 != 1:
            continue
        for M in sqrt_roots_mod_pow2(r, k):
            if not (1 << p) <= M < (1 << (p + 1)):
                continue
            if (M * M >= (1 << (2 * p + 1))) != bool(parity):
                continue
            out.append((M, r))
    return out


def sqrt_midpoint_arrays(dt, scales):
    """the cases of both parities as (x, correctly rounded sqrt(x)) in width dt, repeated at x 4^k for k in `scales`"""
    W = Width(dt)
    p = W.p
    xs, ys = [], []
    for parity in (0, 1):
        for M, r in sqrt_midpoint_cases(p, parity):
            X = (M * M - r) // 4
            sh = X.bit_length() - p
            assert X % (1 << sh) == 0
            Y = (M - 1) // 2 if r > 0 else (M + 1) // 2                  # below the midpoint iff r > 0
            for k in scales:
                xs.append(np.ldexp(float(X >> sh), sh + 2 - 2 * p + 2 * k))
                ys.append(np.ldexp(float(Y), 1 - p + k))
    return np.array(xs, dtype=W.real), np.array(ys, dtype=W.real)


def div_midpoint_cases(p, n, seed=20263, rmax=100):
    """[(A, B, M, r)]: p-bit A, odd p-bit B with A / B within |r| 2^-p ulp of the midpoint M / 2 (M odd, p+1 bits) of two p-bit
    significands; the quotient A / B lies in [1/2, 1) and rounds down to (M - 1) / 2 iff r > 0"""
    rng = np.random.default_rng(seed)
    out = []
    mod = 1 << (p + 1)
    while len(out) < n:
        B = int(rng.integers(1 << (p - 1), 1 << p, dtype=np.uint64)) | 1
        r = 2 * int(rng.integers(-(rmax // 2), rmax // 2)) + 1
        M = (r * pow(B, -1, mod)) % mod
        if M < (1 << p):
            continue
        A, rem = divmod(M * B - r, mod)
        assert rem == 0
        if not (1 << (p - 1)) <= A < (1 << p):
            continue
        out.append((A, B, M, r))
    return out


def div_midpoint_arrays(dt, n, eb, eq, seed=20263):
    """n cases as (a, b, correctly rounded a / b) in width dt with b in [2^eb, 2^(eb+1)) and the quotient in [2^eq, 2^(eq+1))"""
    W = Width(dt)
    p = W.p
    a, b, q = [], [], []
    for A, B, M, r in div_midpoint_cases(p, n, seed):
        Q = (M - 1) // 2 if r > 0 else (M + 1) // 2
        b.append(np.ldexp(float(B), eb - (p - 1)))
        a.append(np.ldexp(float(A), eb + eq + 1 - (p - 1)))           # A / B in [1/2, 1)
        q.append(np.ldexp(float(Q), eq - (p - 1)))
    return np.array(a, dtype=W.real), np.array(b, dtype=W.real), np.array(q, dtype=W.real)


# the exponents at which mhx_div_normal is probed: (exponent of b, exponent of the quotient).  MEMBERS is the domain its comment
# claims -- |b| < 2^1022 (1 / b is normal), a normal quotient and |a| >= 2^-968 (the residual a - b q, a multiple of
# ulp(b) ulp(q), is exact); NON_MEMBERS are finite normal operands with a normal quotient outside it, kept to show the edge.
DIV_MEMBERS = [(0, 0), (1, -2), (1, -53), (0, 52), (-1022, 1000), (-1022, 54), (1021, -1022), (1021, 1), (500, -1022), (-54, -914),
               (-484, -484), (511, 511), (-1000, 1023), (1021, 0), (-1022, 1023)]
DIV_NON_MEMBERS = [(1022, -3), (1023, -1022), (1022, -1022), (-54, -916), (-500, -500), (-1022, 0), (0, -1000)]


def div_member(eb, eq):
    """is (exponent of b, exponent of the quotient) inside the domain claimed for mhx_div_normal?  (a has exponent eb + eq or
    eb + eq + 1; the generators put a = A 2^(eb + eq + 1 - 52) with A in [2^52, 2^53), exponent eb + eq + 1)"""
    return -1022 <= eb <= 1021 and -1022 <= eq <= 1023 and -968 <= eb + eq + 1 <= 1023


def log_core_div_inputs(n_random=2 ** 22):
    """mantissas m of mhx_log_core: the bit patterns [bits(sqrt(1/2)), bits(sqrt(1/2)) + 2^52); the probe divides f = m - 1 by 2 + f"""
    W = Width("f64")
    lo, hi = W.log_split, W.log_split + (1 << 52) - 1
    bits = [W.one, W.one + 1, W.one - 1, W.one - 2]                       # 1, 1 + 2^-52, 1 - 2^-53, 1 - 2^-52
    bits += [lo - 1, lo, lo + 1, lo + 2, hi - 2, hi - 1, hi, hi + 1]
    rnd = np.random.default_rng(20264).integers(lo, hi + 1, n_random, dtype=np.uint64)
    return np.concatenate([W.from_bits(bits), W.from_bits(rnd)])


# ---- sqrt ------------------------------------------------------------------------------------------------------------------------
def box_muller_domain_ends(dt):
    """-2 log(u) for the largest and smallest u01_open, and (fp32: the largest rounds to 1) for the largest u below 1"""
    W = Width(dt)
    top = 0xffffffff
    words = [[0, 0], [top, top]] if dt == "f64" else [[0], [top], [top - 128]]
    u = orc_u01("open", np.array(words, dtype=np.uint64).T, dt)
    return (W.real(-2.0) * orc_map("orc_log", u, dt)).astype(W.real)


def sqrt_f32_binade(which):
    """all 2^23 floats of [1, 2) (which = 0) or [2, 4) (which = 1): exhaustive in the mantissa for one exponent parity"""
    lo = 0x3f800000 + (which << 23)
    return np.arange(lo, lo + (1 << 23), dtype=np.uint32).view(np.float32)


def sqrt_extras(dt):
    """+-0 (fp32: inside the claimed domain), the ends of the Box-Muller domain, 1 - 2^-53 and 1 + 2^-52 (fp64; the neighbours of 1
    in fp32) and their images in the neighbouring binades"""
    W = Width(dt)
    parts = [box_muller_domain_ends(dt)]
    near1 = W.from_bits([W.one - 1, W.one + 1])
    parts.append(np.concatenate([near1, near1 * W.real(2), near1 * W.real(0.5), near1 * W.real(4)]))
    if dt == "f32":
        parts.append(W.from_bits([0, W.sign]))
    return np.concatenate(parts)


def sqrt_f32_non_members():
    """normal floats below the domain claimed for the fp32 mhx_sqrt_normal, where its residuals underflow: the smallest normal
    (whose root comes out one ulp low) and its neighbourhood"""
    W = Width("f32")
    return W.from_bits([W.tiny, W.tiny + 1, W.tiny << 1, 0x0c800000])             # FLT_MIN, its successor, 2^-125, 2^-102


def sqrt_f64_random(n=2 ** 22):
    """[2.2e-16, 74]: half log-uniform, half uniform"""
    rng = np.random.default_rng(20265)
    lo, hi = 2.0 ** -52, 74.0
    a = np.exp(rng.uniform(np.log(lo), np.log(hi), n // 2))
    b = rng.uniform(lo, hi, n - n // 2)
    return np.clip(np.concatenate([a, b]), lo, hi)


# x 4^k: fp64 inside the Box-Muller domain [2^-52, 74]; fp32 across the domain its header claims, [2^-80, 2^122), with the
# Box-Muller domain [1.19e-7, 46] at k = -11, 0, 1
SQRT_MIDPOINT_SCALES = {"f64": (-26, -10, 0, 2), "f32": (-40, -11, 0, 1, 60)}


# ---- angle and uniform words -----------------------------------------------------------------------------------------------------
def angle_edge_words(dt):
    """0, max, every multiple of an eighth of a turn and its neighbours: +-1, and in fp64 +-2^10 and +-(2^10 - 1), where the
    residual's shift truncates"""
    nbits = 64 if dt == "f64" else 32
    offs = (0, 1, -1, 1 << 10, -(1 << 10), (1 << 10) - 1, -((1 << 10) - 1)) if dt == "f64" else (0, 1, -1)
    ws = [0, (1 << nbits) - 1]
    for j in range(8):
        ws += [((j << (nbits - 3)) + o) % (1 << nbits) for o in offs]
    return np.array(ws, dtype=np.uint64)


def quarter_turn_words(dt):
    nbits = 64 if dt == "f64" else 32
    return np.array([j << (nbits - 2) for j in range(4)], dtype=np.uint64)


def angle_random_words(dt, n=2 ** 20):
    return np.random.default_rng(20266).integers(0, 2 ** 64 if dt == "f64" else 2 ** 32, n, dtype=np.uint64)


def split_angle(dt, a):
    """angle words -> [nwords][n] Philox words: (hi, lo) in fp64, (k) in fp32"""
    a = np.asarray(a, dtype=np.uint64)
    if dt == "f64":
        return np.stack([a >> np.uint64(32), a & np.uint64(0xffffffff)])
    return a[None, :]


def uniform_edge_words(dt):
    """single 32-bit words at the edges of the uniform conversions"""
    top = 0xffffffff
    ws = [0, 1, (1 << 12) - 1, 1 << 12, top, top - (1 << 12)]
    if dt == "f32":
        ws += [top - 127, top - 128]                                     # 2^32 - 128 and 2^32 - 129: where (float)k rounds to 2^32
    return np.array(ws, dtype=np.uint64)


def uniform_words(dt, n_random=2 ** 16):
    """[2][n] (hi, lo) in fp64 / [1][n] in fp32: every combination of the edge words, then random ones"""
    e = uniform_edge_words(dt)
    rng = np.random.default_rng(20267)
    if dt == "f64":
        hi, lo = np.meshgrid(e, e, indexing="ij")
        edge = np.stack([hi.ravel(), lo.ravel()])
        return np.concatenate([edge, rng.integers(0, 2 ** 32, (2, n_random), dtype=np.uint64)], axis=1)
    return np.concatenate([e[None, :], rng.integers(0, 2 ** 32, (1, n_random), dtype=np.uint64)], axis=1)


def block_words(dt, n_random=2 ** 16):
    """Philox blocks [4][n]: the uniform's edge words combined with the angle's edge words, then random blocks.  fp64 spends words
    (x, y) on the uniform and (z, w) on the angle; fp32 word x on the uniform and word y (mhx_normal_pair) or z (the family
    helpers) on the angle -- the fp32 blocks carry the angle in both y and z."""
    u = uniform_words(dt, 0)
    ang = split_angle(dt, angle_edge_words(dt))
    nu, na = u.shape[1], ang.shape[1]
    iu, ia = np.meshgrid(np.arange(nu), np.arange(na), indexing="ij")
    iu, ia = iu.ravel(), ia.ravel()
    if dt == "f64":
        edge = np.stack([u[0, iu], u[1, iu], ang[0, ia], ang[1, ia]])
    else:
        edge = np.stack([u[0, iu], ang[0, ia], ang[0, ia], u[0, iu]])
    rnd = np.random.default_rng(20268).integers(0, 2 ** 32, (4, n_random), dtype=np.uint64)
    return np.concatenate([edge, rnd], axis=1)


# ---- composed references ---------------------------------------------------------------------------------------------------------
def normal_pair_reference(dt, blocks):
    """mhx_normal_pair of Philox blocks [4][n] as family_restatement composes it: u01_open of the words, the oracle's log,
    np.sqrt(-2 l), the oracle's sincos, two products -- every step rounded in the width"""
    W = Width(dt)
    if dt == "f64":
        u = orc_u01("open", blocks[0:2], dt)
        ang = (blocks[2] << np.uint64(32)) | blocks[3]
    else:
        u = orc_u01("open", blocks[0:1], dt)
        ang = blocks[1]
    l = orc_map("orc_log", u, dt)
    rad = np.sqrt(W.real(-2.0) * l)
    s, c = orc_sincos(ang, dt)
    return rad * c, rad * s


def cauchy_quotient_reference(dt, blocks):
    """s / c of mhx_fam_phase: the oracle's sincos of words (z, w) / word z, one division in the width"""
    ang = ((blocks[2] << np.uint64(32)) | blocks[3]) if dt == "f64" else blocks[2]
    s, c = orc_sincos(ang, dt)
    with np.errstate(all="ignore"):
        return s / c
