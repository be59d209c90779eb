"""Test-side restatement of the proposal-family arithmetic: the draws, the log-kernels and the
Metropolis-Hastings step of a run whose proposal is a vector of univariate components, in plain Python with numpy scalars of the
run's width.

It is composed ONLY from the oracle's exported primitives -- oracle.philox, u01_open / u01_half, log / exp, sincos2pi_u32 / _u64,
normals, accept_logu, Target.__call__ and orc_normal_pair bound through oracle.lib() -- and fma / fmaf of the system libm (this
Python has no math.fma).  It imports nothing from the engine: what it computes is what the spec says, not what the kernels do.

Every constant is wrapped in the width's scalar type before it meets another operand, so every operation rounds once, in the run's
width, like the device code built with -ffp-contract=off."""
import ctypes as C
import ctypes.util
import math

import numpy as np

from oracle import oracle as O

NORMAL, UNIFORM, LAPLACE, CAUCHY, EXPONENTIAL, GAMMA, INVERSE_GAMMA = range(7)
STREAM_FAMILY, STREAM_FAMILY_INIT = 8, 12
GAMMA_ATTEMPTS = 128

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = C.c_double
_libm.fma.argtypes = [C.c_double] * 3
_libm.fmaf.restype = C.c_float
_libm.fmaf.argtypes = [C.c_float] * 3


def r(v):
    """v in the run's width"""
    return O.real()(v)


def fma(a, b, c):
    if O.get_dtype() == "f64":
        return np.float64(_libm.fma(float(a), float(b), float(c)))
    return np.float32(_libm.fmaf(float(np.float32(a)), float(np.float32(b)), float(np.float32(c))))


def log(x):
    return r(O.log(r(x))[0])


def exp(x):
    return r(O.exp(r(x))[0])


def block(seed, cid, step, stream, blk):
    """Philox block `blk` of stream `stream` of (seed, chain id, step): counter word 3 = stream << 28 | blk"""
    return O.philox([cid & 0xffffffff, cid >> 32, step, ((stream << 28) | blk) & 0xffffffff], [seed & 0xffffffff, seed >> 32])


# how a block of a family stream is spent: fp64 -- words (x, y) the uniform, (z, w) the second uniform / the phase; fp32 -- word x
# and word z; bit 31 of z is the sign in both; a Marsaglia-Tsang normal is normal 0 of the block's Box-Muller pair
def u_open(w):
    return r(O.u01_open(w[0], w[1]) if O.get_dtype() == "f64" else O.u01_open(w[0]))


def u_half(w):
    return r(O.u01_half(w[0], w[1]) if O.get_dtype() == "f64" else O.u01_half(w[0]))


def u_open2(w):
    return r(O.u01_open(w[2], w[3]) if O.get_dtype() == "f64" else O.u01_open(w[2]))


def phase(w):
    s, c = O.sincos2pi_u64((w[2] << 32) | w[3]) if O.get_dtype() == "f64" else O.sincos2pi_u32(w[2])
    return r(s), r(c)


def bm_normal(w):
    L = O.lib()
    if O.get_dtype() == "f64":
        a, b = C.c_double(), C.c_double()
        L.orc_normal_pair((C.c_uint32 * 4)(*w), C.byref(a), C.byref(b))
    else:
        a, b = C.c_float(), C.c_float()
        L.orc_normal_pair(C.c_uint32(w[0]), C.c_uint32(w[1]), C.byref(a), C.byref(b))
    return r(a.value)


def table(comps):
    """[(family, p0, p1)] in doubles -> the rows the kernels read: parameters and what is derived from them once, in double, each
    rounded once to the run's width.  Uniform: b - a of the ROUNDED bounds, in the width.  Gamma families, from alpha AS ROUNDED to the width: d = alpha' - 1/3,
    c = 1 / sqrt(9 d) with alpha' = alpha or (alpha < 1) alpha + 1, 1 / alpha, and the power of the argument in the log-kernel."""
    rows = []
    for fam, p0, p1 in comps:
        p = [r(p0), r(p1), r(0), r(0), r(0), r(0)]
        if fam == UNIFORM:
            p[2] = p[1] - p[0]
        elif fam in (GAMMA, INVERSE_GAMMA):
            al = float(p[0])                        # alpha as rounded to the width: the number the draw compares with 1
            ae = al + 1.0 if al < 1.0 else al
            dd = ae - 1.0 / 3.0
            p[2], p[3], p[4] = r(dd), r(1.0 / math.sqrt(9.0 * dd)), r(1.0 / al)
            p[5] = r(al - 1.0 if fam == GAMMA else -(al + 1.0))
        rows.append((fam, p))
    return rows


def gamma1(p, seed, cid, step, sbase, k):
    """Gamma(alpha, 1), Marsaglia & Tsang: attempt t takes normal block and uniform block (k << 8 | t) of streams sbase + 1, sbase + 2"""
    alpha, d, c, inva = p[0], p[2], p[3], p[4]
    with np.errstate(all="ignore"):
        for t in range(GAMMA_ATTEMPTS):
            blk = (k << 8) | t
            n = bm_normal(block(seed, cid, step, sbase + 1, blk))
            wu = block(seed, cid, step, sbase + 2, blk)
            v1 = fma(c, n, r(1))
            if not v1 > r(0):
                continue
            v = (v1 * v1) * v1
            lu = log(u_open(wu))
            h = (r(0.5) * n) * n
            rhs = fma(d, log(v), h + (d - d * v))
            if lu < rhs:
                g = d * v
                if alpha < r(1):
                    g = g * exp(log(u_open2(wu)) * inva)
                return g
    return r(np.nan)


def draw(row, nk, seed, cid, step, sbase, k):
    """xi_k; nk = standard normal k of the step's Box-Muller stream (the Normal family)"""
    fam, p = row
    with np.errstate(all="ignore"):
        if fam == NORMAL:
            return fma(p[1], nk, p[0])
        if fam == GAMMA:
            return gamma1(p, seed, cid, step, sbase, k) * p[1]
        if fam == INVERSE_GAMMA:
            return p[1] / gamma1(p, seed, cid, step, sbase, k)
        w = block(seed, cid, step, sbase, k)
        if fam == UNIFORM:
            v = fma(p[2], u_half(w), p[0])
            return p[1] if v > p[1] else v
        if fam == CAUCHY:
            s, c = phase(w)
            return fma(p[1], s / c, p[0])
        e = -log(u_open(w))
        if fam == EXPONENTIAL:
            return e * p[0]
        m = e * p[1]
        return p[0] + (-m if (w[2] >> 31) else m)


def logk(row, v):
    """logpdf minus its constant, -Inf outside the support"""
    fam, p = row
    v = r(v)
    ninf = r(-np.inf)
    with np.errstate(all="ignore"):
        if fam == NORMAL:
            t = (v - p[0]) / p[1]
            return r(-0.5) * (t * t)
        if fam == UNIFORM:
            return r(0) if (v >= p[0] and v <= p[1]) else ninf
        if fam == LAPLACE:
            return -(abs(v - p[0]) / p[1])
        if fam == CAUCHY:
            t = (v - p[0]) / p[1]
            return -log(fma(t, t, r(1)))
        if fam == EXPONENTIAL:
            return -(v / p[0]) if v >= r(0) else ninf
        if fam == GAMMA:
            return fma(p[5], log(v), -(v / p[1])) if v > r(0) else ninf
        return fma(p[5], log(v), -(p[1] / v)) if v > r(0) else ninf


def draw_all(rows, seed, cid, step, nstream, sbase):
    d = len(rows)
    nrm = O.normals(seed, cid, step, nstream, d) if any(f == NORMAL for f, _ in rows) else [r(0)] * d
    return [draw(rows[k], r(nrm[k]), seed, cid, step, sbase, k) for k in range(d)]


def qsum(rows, vs):
    q = r(0)
    with np.errstate(all="ignore"):
        for row, v in zip(rows, vs):
            q = q + logk(row, v)
    return q


def run(target, comps, n_samples, seed, first_chain, nchains, static=False, symmetric=False, init=None):
    """The chains of `n_samples` recorded states (sample 1 = the initial state, one transition between samples) of a run whose
    proposal is `comps` [(family, p0, p1)]: random walk y = x + xi with q(x - y) - q(y - x) unless `symmetric`, or static y = xi
    with q(x) - q(y).  init [d][nchains] or None = a bare draw from the proposal (streams INIT / FAMILY_INIT, step 0)."""
    rows = table(comps)
    d, N, Cn = len(rows), n_samples, nchains
    samples = np.empty((N, d + 1, Cn), dtype=O.real())
    accepted = np.zeros((N, Cn), dtype=np.uint8)
    fx = np.empty((d, Cn), dtype=O.real())
    flp = np.empty(Cn, dtype=O.real())
    fq = np.zeros(Cn, dtype=O.real())
    cnt = np.zeros(Cn, dtype=np.uint32)
    with np.errstate(all="ignore"):
        for c in range(Cn):
            cid = first_chain + c
            if init is not None:
                x = [r(init[k][c]) + r(0) for k in range(d)]
            else:
                x = [r(0) + xi for xi in draw_all(rows, seed, cid, 0, O.STREAM_INIT, STREAM_FAMILY_INIT)]
            lp = r(target(np.array(x, dtype=O.real())))
            qx = qsum(rows, x) if static else r(0)
            samples[0, :d, c], samples[0, d, c] = x, lp
            for step in range(1, N):
                xi = draw_all(rows, seed, cid, step, O.STREAM_PROPOSAL, STREAM_FAMILY)
                y = list(xi) if static else [x[k] + xi[k] for k in range(d)]
                qy = r(0)
                if static:
                    qy = qsum(rows, y)
                    ratio = qx - qy
                elif not symmetric:
                    ratio = qsum(rows, [x[k] - y[k] for k in range(d)]) - qsum(rows, [y[k] - x[k] for k in range(d)])
                lpy = r(target(np.array(y, dtype=O.real())))
                loga = (lpy - lp) + ratio if (static or not symmetric) else (lpy - lp)
                acc = bool(r(O.accept_logu(seed, cid, step)) < loga)
                if acc:
                    x, lp, qx = y, lpy, qy
                    cnt[c] += 1
                samples[step, :d, c], samples[step, d, c] = x, lp
                accepted[step, c] = 1 if acc else 0
            fx[:, c], flp[c], fq[c] = x, lp, qx
    return dict(samples=samples, accepted=accepted, final_x=fx, final_lp=flp, final_q=fq, accept_counts=cnt)
