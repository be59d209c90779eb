"""Test-side restatement of the conditional-proposal arithmetic: the Metropolis-Hastings step of a run
whose proposal components have parameters that depend on the state, in plain Python with numpy scalars of the run's width.

It is composed from tests/family_restatement.py (`table`, `draw_all`, `logk`, `r`, `log`, `exp`, `fma`) and the oracle's primitives
only, and imports nothing from the engine.

A parameter map is written ONCE, against a small namespace `m` (`m.log`, `m.exp`, `m.abs`, `m.fma`, `m.c(constant)`,
`m.sum_over(array, fn)`), as `pmap(m, x) -> [(family, p0, p1)] * d` where p0 / p1 are plain numbers (constants of the table) or
values computed from the state x (a list of d numbers).  The same callable is then used twice: the GPU test passes a namespace of
tracing functions and wraps the result in the engine's distribution classes (that makes the kernel source), and `run` below
passes WIDTH, whose functions work on scalars of the run's width (that makes the expected chain).  The tracer records one engine
operation per Python operation, without re-association or contraction, so both give the same bits."""
import numpy as np

import family_restatement as F
from oracle import oracle as O


class _Width:
    """the namespace of a parameter map evaluated on scalars of the run's width: every operation rounds once, in the width"""
    log = staticmethod(F.log)
    exp = staticmethod(F.exp)
    fma = staticmethod(F.fma)

    @staticmethod
    def abs(v):
        return abs(F.r(v))

    @staticmethod
    def c(v):
        return F.r(v)

    @staticmethod
    def sum_over(data, fn):
        """acc = acc + fn(row) over the rows in order, from 0; the rows as they are uploaded: rounded once to the width"""
        acc = F.r(0)
        for row in np.asarray(data, dtype=np.float64):
            acc = acc + fn(F.r(row))
        return acc


WIDTH = _Width()


def rows_of(params):
    """[(family, p0, p1)] at one state -> the rows the draws and log-kernels read (Uniform's b - a in the width, a Gamma family's
    derived constants from its constant shape)"""
    return F.table([(f, float(p0), float(p1)) for f, p0, p1 in params])


def _finite(v):
    return bool(abs(v) < F.r(np.inf))


def valid(rows):
    """sigma, theta > 0, a < b, everything finite (the shape of a Gamma family is a constant)"""
    for fam, p in rows:
        if fam == F.UNIFORM:
            ok = _finite(p[0]) and _finite(p[1]) and bool(p[0] < p[1])
        elif fam == F.EXPONENTIAL:
            ok = _finite(p[0]) and bool(p[0] > F.r(0))
        elif fam in (F.GAMMA, F.INVERSE_GAMMA):
            ok = _finite(p[1]) and bool(p[1] > F.r(0))
        else:
            ok = _finite(p[0]) and _finite(p[1]) and bool(p[1] > F.r(0))
        if not ok:
            return False
    return True


def lognorm(row):
    """z: the part of logpdf that depends on the parameters, minus the constants that cancel between the two directions"""
    fam, p = row
    if fam == F.UNIFORM:
        return -F.log(p[2])
    if fam == F.EXPONENTIAL:
        return -F.log(p[0])
    if fam == F.GAMMA:
        return -(p[0] * F.log(p[1]))
    if fam == F.INVERSE_GAMMA:
        return p[0] * F.log(p[1])
    return -F.log(p[1])


def Z(rows):
    z = F.r(0)
    for row in rows:
        z = z + lognorm(row)
    return z


def K(rows, vs):
    return F.qsum(rows, vs)


def run(target, pmap, d, n_samples, seed, first_chain, nchains, init, static=False, symmetric=False, with_z=True):
    """The chains of `n_samples` recorded states (sample 1 = the given initial state, one transition between samples) under the
    conditional proposal `pmap`.  `with_z=False` leaves Z out of the ratio: it exists ONLY so that a test can show that Z matters."""
    N, Cn = n_samples, nchains
    samples = np.empty((N, d + 1, Cn), dtype=O.real())
    accepted = np.zeros((N, Cn), dtype=np.uint8)
    fx = np.empty((d, Cn), dtype=O.real())
    flp = np.empty(Cn, dtype=O.real())
    cnt = np.zeros(Cn, dtype=np.uint32)
    with np.errstate(all="ignore"):
        for c in range(Cn):
            cid = first_chain + c
            x = [F.r(init[k][c]) + F.r(0) for k in range(d)]
            lp = F.r(target(np.array(x, dtype=O.real())))
            rx = rows_of(pmap(WIDTH, x))
            assert valid(rx), "the initial state of chain %d has invalid parameters" % c
            Zx = Z(rx)
            samples[0, :d, c], samples[0, d, c] = x, lp
            for step in range(1, N):
                xi = F.draw_all(rx, seed, cid, step, O.STREAM_PROPOSAL, F.STREAM_FAMILY)
                y = list(xi) if static else [x[k] + xi[k] for k in range(d)]
                ry = rows_of(pmap(WIDTH, y))
                ok = valid(ry)
                lpy = F.r(target(np.array(y, dtype=O.real())))
                acc, Zy = False, F.r(0)
                if ok:                                      # an invalid p(y) is rejected by a branch of its own
                    if symmetric:
                        loga = lpy - lp
                    else:
                        Zy = Z(ry)
                        if static:
                            kk = K(ry, x) - K(rx, y)
                        else:
                            kk = K(ry, [x[k] - y[k] for k in range(d)]) - K(rx, [y[k] - x[k] for k in range(d)])
                        ratio = kk + (Zy - Zx) if with_z else kk
                        loga = (lpy - lp) + ratio
                    acc = bool(F.r(O.accept_logu(seed, cid, step)) < loga)
                if acc:
                    x, lp, rx, Zx = y, lpy, ry, Zy
                    cnt[c] += 1
                samples[step, :d, c], samples[step, d, c] = x, lp
                accepted[step, c] = 1 if acc else 0
            fx[:, c], flp[c] = x, lp
    return dict(samples=samples, accepted=accepted, final_x=fx, final_lp=flp, accept_counts=cnt)


# ---------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_conditional.py: name -> (d, pmap, initial states (d, C) -> array).  Every target is the isotropic
# standard Gaussian of the case's dimension (oracle.iso_gauss(d) / mhx.IsoGaussian(d)).
_W = np.array([0.05, 0.1, 0.15])


def _scale(m, xk, a=0.4, b=0.2):
    return m.c(a) + m.c(b) * m.abs(xk)


def _a(m, x):                    # d = 1: Normal(0, 0.5 + |x|)
    return [(F.NORMAL, 0.0, m.c(0.5) + m.abs(x[0]))]


def _b(m, x):                    # d = 2: each component reads the OTHER coordinate
    return [(F.NORMAL, m.c(0.25) * x[1], m.exp(m.c(0.3) * x[1])), (F.LAPLACE, m.c(0.25) * x[0], m.exp(m.c(0.3) * x[0]))]


def _c(m, x):                    # d = 7: one component of each family, a state-dependent scale on each; Gamma shape 0.7: the alpha < 1 branch
    s = [_scale(m, x[k]) for k in range(7)]
    return [(F.NORMAL, 0.0, s[0]), (F.UNIFORM, -s[1], s[1]), (F.LAPLACE, 0.0, s[2]), (F.CAUCHY, 0.0, m.c(0.5) * s[3]),
            (F.EXPONENTIAL, s[4], 0.0), (F.GAMMA, 0.7, s[5]), (F.INVERSE_GAMMA, 2.0, s[6])]


def _d(m, x):                    # d = 5: a partial Philox block of four; a closed-over array travels in the data block
    s = [m.c(0.3) + m.sum_over(_W, lambda w, k=k: w * m.abs(x[k])) for k in (0, 2)]
    return [(F.NORMAL, 0.0, s[0]), (F.LAPLACE, 0.0, _scale(m, x[1])), (F.CAUCHY, 0.0, m.c(0.5) * s[1]),
            (F.UNIFORM, -_scale(m, x[3]), _scale(m, x[3])), (F.NORMAL, m.c(0.1) * x[0], m.fma(m.c(0.2), m.abs(x[4]), m.c(0.4)))]


def _e(m, x):                    # d = 1: Normal(0, x): a distribution only where x > 0
    return [(F.NORMAL, 0.0, x[0])]


def _init(d, C, positive):
    z = np.random.default_rng(1234 + d).normal(size=(d, C))
    return (np.abs(z) + 0.25 if positive else z).astype(np.float32)


CASES = {
    "a_scalar_scale_abs": (1, _a, lambda C: _init(1, C, False)),
    "b_cross_coordinates": (2, _b, lambda C: _init(2, C, False)),
    "c_every_family": (7, _c, lambda C: _init(7, C, True)),          # (x > 0: the one-sided families' support, static form)
    "d_data_block": (5, _d, lambda C: _init(5, C, False)),
    "e_scale_is_the_state": (1, _e, lambda C: _init(1, C, True)),
}
