"""Test-side restatement of the adaptive random-walk Metropolis arithmetic: chains that tune their own
log-scale and, with `shape`, their own per-coordinate standard deviations during a warm-up and run on as plain random walks, in plain
Python with numpy scalars of the run's width.

Like tempered_restatement.py, whose helpers it imports, it is composed ONLY from the oracle's exported primitives -- normals,
accept_logu, exp, the targets -- fma / fmaf of the system libm and numpy's correctly rounded sqrt, and imports nothing from the
engine.  The host-side part of the spec (the step sizes, the clamps of the variance) is Python's math, which is the C library's double
arithmetic."""
import math

import numpy as np

from oracle import oracle as O
from tempered_restatement import fma, r

DEFAULTS = dict(target_rate=0.234, c=1.0, kappa=0.6, lam_min=-20.0, lam_max=20.0)


def exp(v):
    return r(O.exp(r(v))[0])


def sqrt(v):
    return r(np.sqrt(r(v)))


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def gammas(c, kappa, steps):
    """gamma[t] = min(1, c * t^(-kappa)), t = 1 .. steps (returned at index t - 1): pow and one product in double, rounded once"""
    return [r(min(1.0, float(c) * math.pow(float(t), -float(kappa)))) for t in range(1, steps + 1)]


def base_sds(prop_kind, sigma, d):
    """the configured standard deviations in the width: ISO the double scale rounded once, DIAG sigma_k as given in the width"""
    return [r(sigma)] * d if prop_kind == O.PROP_ISO else [r(v) for v in sigma]


def run(target, prop_kind, sigma, n_samples, seed, first_chain, nchains, adapt_steps, shape=False, discard_initial=0, thinning=1,
        init=None, target_rate=None, c=None, kappa=None, lam_min=None, lam_max=None):
    """The chains of an adaptive run; schedule as mcmcsample's (discard_initial = 0 records the initial state as sample 1), init
    [d][nchains] or None = the plain run's initial draw; a None parameter = the default of the spec.  Returns samples [N][d + 1][nchains],
    accepted [N][nchains], final_x, final_lp, accept_counts, lam [nchains], sd [d][nchains] (eff), mean [d][nchains] (NaN without shape),
    var [d][nchains] (v; NaN without shape) and acc_at_freeze [nchains]."""
    d = target.dim if hasattr(target, "dim") else len(init)
    p = dict(DEFAULTS)
    for k, v in dict(target_rate=target_rate, c=c, kappa=kappa, lam_min=lam_min, lam_max=lam_max).items():
        if v is not None:
            p[k] = v
    N = n_samples
    nT = discard_initial + (N - 1) * thinning
    gam = gammas(p["c"], p["kappa"], adapt_steps)
    tr, lo, hi = r(p["target_rate"]), r(p["lam_min"]), r(p["lam_max"])
    s = base_sds(prop_kind, sigma, d)
    vlo = [r(float(v) * float(v) * 2.0 ** -40) for v in s]
    vhi = [r(float(v) * float(v) * 2.0 ** 40) for v in s]
    samples = np.empty((N, d + 1, nchains), dtype=O.real())
    accepted = np.zeros((N, nchains), dtype=np.uint8)
    fx = np.empty((d, nchains), dtype=O.real())
    flp = np.empty(nchains, dtype=O.real())
    cnt = np.zeros(nchains, dtype=np.uint32)
    frz = np.zeros(nchains, dtype=np.uint32)
    flam = np.empty(nchains, dtype=O.real())
    fsd = np.empty((d, nchains), dtype=O.real())
    fmean = np.full((d, nchains), np.nan, dtype=O.real())
    fvar = np.full((d, nchains), np.nan, dtype=O.real())
    with np.errstate(all="ignore"):
        for cc in range(nchains):
            cid = first_chain + cc
            if init is not None:
                x = [r(init[k][cc]) + r(0) for k in range(d)]
            else:
                n0 = O.normals(seed, cid, 0, O.STREAM_INIT, d)
                x = [fma(s[k], n0[k], r(0)) for k in range(d)]
            lp = r(target(np.array(x, dtype=O.real())))
            lam = r(0)
            eff, sig = list(s), list(s)
            m, v = list(x), [s[k] * s[k] for k in range(d)]
            last, slot = 0, 0
            save_next = discard_initial if discard_initial > 0 else 0
            if discard_initial == 0:
                samples[0, :d, cc], samples[0, d, cc], accepted[0, cc] = x, lp, 0
                slot, save_next = 1, thinning
            for step in range(1, nT + 1):
                n = O.normals(seed, cid, step, O.STREAM_PROPOSAL, d)
                y = [fma(eff[k], n[k], x[k]) for k in range(d)]
                lpy = r(target(np.array(y, dtype=O.real())))
                loga = lpy - lp
                acc = bool(r(O.accept_logu(seed, cid, step)) < loga)
                if acc:
                    x, lp = y, lpy
                    cnt[cc] += 1
                last = 1 if acc else 0
                if step <= adapt_steps:
                    pa = r(0) if bool(np.isnan(loga)) else (r(1) if bool(loga >= r(0)) else exp(loga))
                    g = gam[step - 1]
                    lam = clamp(fma(g, pa - tr, lam), lo, hi)
                    if shape:
                        for k in range(d):
                            dl = x[k] - m[k]
                            mn = fma(g, dl, m[k])
                            vn = clamp(fma(g, fma(dl, dl, -v[k]), v[k]), vlo[k], vhi[k])
                            if bool(np.isfinite(mn)) and bool(np.isfinite(vn)):
                                m[k], v[k], sig[k] = mn, vn, sqrt(vn)
                    el = exp(lam)
                    eff = [sig[k] * el for k in range(d)]
                if step == adapt_steps:
                    frz[cc] = cnt[cc]
                if step == save_next and slot < N:
                    samples[slot, :d, cc], samples[slot, d, cc], accepted[slot, cc] = x, lp, last
                    slot += 1
                    save_next += thinning
            fx[:, cc], flp[cc], flam[cc], fsd[:, cc] = x, lp, lam, eff
            if shape:
                fmean[:, cc], fvar[:, cc] = m, v
    return dict(samples=samples, accepted=accepted, final_x=fx, final_lp=flp, accept_counts=cnt, lam=flam, sd=fsd, mean=fmean, var=fvar,
                acc_at_freeze=frz)
