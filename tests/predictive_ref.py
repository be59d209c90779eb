"""Test-side reference for posterior predictive draws: the predictive tensor of a map, in plain Python with
numpy scalars of the run's width.

It is composed ONLY from tests/family_restatement.py (block, bm_normal, draw, table, r -- and through draw: gamma1, fma, log, exp)
and, through it, the oracle's exported primitives.  It imports nothing from the engine: what it computes is what the spec says.

A test writes its map ONCE, as `make(draw)` -> `fn(theta)`, with the distributions below (anything with `.family` and `.params()` is a
distribution to the engine's tracer too):
    engine      mhx.trace.trace_predictive(make(mhx.trace.draw), d)        theta is the tracer's vector
    reference   tensor(make, x, seed, first_chain)                         theta is a list of numpy scalars of the width, and draw
                a Stream: a counter of draw indices that calls the restatement with the salted seed, the global chain id and t
The parameter expressions of such a map must be single-rounding operations (+ - * /, abs) on the parameters, earlier draws and
constants that both widths hold exactly: the numpy-scalar evaluation is then the engine's arithmetic bit for bit.  No log / exp /
** in them: Python's are not the oracle's."""
import numpy as np

import family_restatement as FR

PREDICT_SALT = 0x5052454449435421              # MHX_PREDICT_SALT (csrc/mhx_device_math.h), "PREDICT!"


class Dist:
    def __init__(self, family, p0, p1=0.0):
        self.family, self.p0, self.p1 = family, p0, p1

    def params(self):
        return self.p0, self.p1


def Normal(mu, sigma): return Dist(FR.NORMAL, mu, sigma)                     # noqa: E704
def Uniform(a, b): return Dist(FR.UNIFORM, a, b)                             # noqa: E704
def Laplace(mu, theta): return Dist(FR.LAPLACE, mu, theta)                   # noqa: E704
def Cauchy(mu, sigma): return Dist(FR.CAUCHY, mu, sigma)                     # noqa: E704
def Exponential(theta): return Dist(FR.EXPONENTIAL, theta)                   # noqa: E704
def Gamma(alpha, theta): return Dist(FR.GAMMA, alpha, theta)                 # noqa: E704
def InverseGamma(alpha, theta): return Dist(FR.INVERSE_GAMMA, alpha, theta)  # noqa: E704


def valid(row):
    """whether the row's parameters are a distribution's (mhx_fam_valid): finite, scale > 0, a < b; a Gamma shape is a constant"""
    fam, p = row
    fin = lambda v: bool(abs(v) < np.inf)                   # noqa: E731  (false for NaN)
    if fam == FR.UNIFORM:
        return fin(p[0]) and fin(p[1]) and bool(p[0] < p[1])
    if fam == FR.EXPONENTIAL:
        return fin(p[0]) and bool(p[0] > 0)
    if fam in (FR.GAMMA, FR.INVERSE_GAMMA):
        return fin(p[1]) and bool(p[1] > 0)
    return fin(p[0]) and fin(p[1]) and bool(p[1] > 0)


def one_draw(dist, seed, cid, t, k, salt=PREDICT_SALT):
    """draw k of (seed, global chain id, saved draw t) from `dist`, in the run's width"""
    key = seed ^ salt
    with np.errstate(all="ignore"):
        row = FR.table([(dist.family, dist.p0, dist.p1)])[0]
        if not valid(row):
            return FR.r(np.nan)
        nk = FR.bm_normal(FR.block(key, cid, t, FR.STREAM_FAMILY, k)) if dist.family == FR.NORMAL else FR.r(0)
        return FR.r(FR.draw(row, nk, key, cid, t, FR.STREAM_FAMILY, k))


class Stream:
    """`draw` of the reference: the k-th call is draw index k of this (seed, chain, saved draw)"""

    def __init__(self, seed, cid, t):
        self.seed, self.cid, self.t, self.k = seed, cid, t, 0

    def __call__(self, dist):
        k, self.k = self.k, self.k + 1
        return one_draw(dist, self.seed, self.cid, self.t, k)


def outputs(make, theta, seed, cid, t):
    """the map's outputs for one saved draw; an output that is a distribution is a draw from it, taken after the function returned"""
    s = Stream(seed, cid, t)
    with np.errstate(all="ignore"):
        out = make(s)(theta)
        out = list(out) if isinstance(out, (list, tuple)) else [out]
        return [s(v) if isinstance(v, Dist) else FR.r(v) for v in out]


def tensor(make, x, seed, first_chain=0):
    """[N][nout + 1][C]: the predictive tensor of the source tensor x [N][d + 1][C] (of the width the oracle is set to); the last row is
    x's lp row"""
    N, d1, C = x.shape
    rows = None
    for t in range(N):
        for c in range(C):
            o = outputs(make, [x[t, k, c] for k in range(d1 - 1)], seed, first_chain + c, t)
            if rows is None:
                rows = np.empty((N, len(o) + 1, C), dtype=x.dtype)
            rows[t, :-1, c] = o
    rows[:, -1, :] = x[:, -1, :]
    return rows
