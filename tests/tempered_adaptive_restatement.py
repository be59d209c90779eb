"""Test-side restatement of the adaptive temperature ladder of a tempered run: the chains of
tests/tempered_restatement.py on ladders that tune themselves from their own swap rounds, in plain Python with numpy scalars of the
run's width.

Like tempered_restatement.py, whose helpers it imports, it is composed ONLY from the oracle's exported primitives -- philox, u01_open,
log, exp, normals, accept_logu, the targets -- and fma / fmaf of the system libm, and imports nothing from the engine.  The host-side
part of the spec (rho0, the step sizes) is Python's math, which is the C library's double arithmetic.

The ladder is parametrised by rho[q], q = 0 .. R - 2, the log of the gap of pair (q, q + 1) in log beta."""
import math

import numpy as np

from oracle import oracle as O
from tempered_restatement import fma, r, swap_logu

DEFAULTS = dict(target_rate=0.234, c=1.0, kappa=0.6, rho_min=-10.0)


def exp(v):
    return r(O.exp(r(v))[0])


def default_rho_max(R):
    return math.log(16.0 / (R - 1))


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def rho0(betas, rho_min, rho_max):
    """log(log(beta[q] / beta[q + 1])) in double, rounded once to the width, clamped in the width"""
    lo, hi = r(rho_min), r(rho_max)
    return [clamp(r(math.log(math.log(float(betas[q]) / float(betas[q + 1])))), lo, hi) for q in range(len(betas) - 1)]


def gammas(c, kappa, nrounds):
    """gamma[s] = c * s^(-kappa), s = 1 .. nrounds (returned at index s - 1): pow and one product in double, rounded once"""
    return [r(float(c) * math.pow(float(s), -float(kappa))) for s in range(1, nrounds + 1)]


def scan(h):
    """inclusive Hillis-Steele scan in the spec's order: for off = 1, 2, 4, .. < R, all lanes at once, h[i] += h[i - off] where i >= off"""
    R, off = len(h), 1
    while off < R:
        h = [h[i] + h[i - off] if i >= off else h[i] for i in range(R)]
        off *= 2
    return h


def ladder(rho):
    """(beta[R], s[R]) of rho[R - 1]: g = exp(rho), h[i] = g[i - 1] with h[0] = 0, scanned; beta = exp(-h), s = exp(0.5 h); rung 0 is 1, 1"""
    g = [exp(v) for v in rho]
    h = scan([r(0)] + g)
    beta = [r(1)] + [exp(-h[i]) for i in range(1, len(h))]
    s = [r(1)] + [exp(r(0.5) * h[i]) for i in range(1, len(h))]
    return beta, s


def run(target, prop_kind, sigma, betas, n_samples, seed, first_chain, nchains, adapt_steps, swap_every=1, discard_initial=0, thinning=1,
        init=None, target_rate=None, c=None, kappa=None, rho_min=None, rho_max=None):
    """The chains of an adaptive tempered run; arguments and schedule as tempered_restatement.run (no user scales: they follow the
    ladder), `betas` the ladder every ladder starts from, None = the default of the spec.  Returns what tempered_restatement.run
    returns, plus betas [nladders][R] at the end, betas_rounds [rounds][nladders][R] after every swap round, rho [nladders][R - 1], and
    frozen_attempts / frozen_counts [nladders][R - 1]: the swap statistics of the rounds after the ladder froze."""
    R = len(betas)
    d = target.dim if hasattr(target, "dim") else len(init)
    assert nchains % R == 0 and first_chain % R == 0 and swap_every > 0 and adapt_steps >= 0
    target_rate = DEFAULTS["target_rate"] if target_rate is None else target_rate
    c = DEFAULTS["c"] if c is None else c
    kappa = DEFAULTS["kappa"] if kappa is None else kappa
    rho_min = DEFAULTS["rho_min"] if rho_min is None else rho_min
    rho_max = default_rho_max(R) if rho_max is None else rho_max
    nl = nchains // R
    N = n_samples
    nT = discard_initial + (N - 1) * thinning
    nrounds = adapt_steps // swap_every
    gam = gammas(c, kappa, nrounds)
    tr, lo, hi = r(target_rate), r(rho_min), r(rho_max)
    base = [r(sigma)] * d if prop_kind == O.PROP_ISO else [r(v) for v in sigma]
    samples = np.empty((N, d + 1, nchains), dtype=O.real())
    accepted = np.zeros((N, nchains), dtype=np.uint8)
    fx = np.empty((d, nchains), dtype=O.real())
    flp = np.empty(nchains, dtype=O.real())
    cnt = np.zeros(nchains, dtype=np.uint32)
    att = np.zeros((nl, R - 1), dtype=np.uint64)
    swp = np.zeros((nl, R - 1), dtype=np.uint64)
    att_f = np.zeros((nl, R - 1), dtype=np.uint64)                  # ... of the rounds after the ladder froze
    swp_f = np.zeros((nl, R - 1), dtype=np.uint64)
    fbeta = np.empty((nl, R), dtype=O.real())
    rounds = np.empty((nT // swap_every, nl, R), dtype=O.real())
    frho = np.empty((nl, R - 1), dtype=O.real())
    with np.errstate(all="ignore"):
        for l in range(nl):
            rho = rho0(betas, rho_min, rho_max)
            beta, sc = ladder(rho)
            xs, lps = [], []
            for q in range(R):
                cid = first_chain + l * R + q
                if init is not None:
                    x = [r(init[k][l * R + q]) + r(0) for k in range(d)]
                else:
                    n0 = O.normals(seed, cid, 0, O.STREAM_INIT, d)
                    x = [fma(base[k], n0[k], r(0)) for k in range(d)]
                xs.append(x)
                lps.append(r(target(np.array(x, dtype=O.real()))))
            last = [0] * R
            slot, save_next = 0, (discard_initial if discard_initial > 0 else 0)

            def record():
                nonlocal slot
                for q in range(R):
                    cc = l * R + q
                    samples[slot, :d, cc], samples[slot, d, cc] = xs[q], lps[q]
                    accepted[slot, cc] = last[q]
                slot += 1
            if discard_initial == 0:
                record()
                save_next = thinning
            for step in range(1, nT + 1):
                for q in range(R):
                    cid = first_chain + l * R + q
                    n = O.normals(seed, cid, step, O.STREAM_PROPOSAL, d)
                    y = [fma(sc[q] * base[k], n[k], xs[q][k]) for k in range(d)]        # the scale: one product in the width
                    lpy = r(target(np.array(y, dtype=O.real())))
                    loga = beta[q] * (lpy - lps[q])
                    acc = bool(r(O.accept_logu(seed, cid, step)) < loga)
                    if acc:
                        xs[q], lps[q] = y, lpy
                        cnt[l * R + q] += 1
                    last[q] = 1 if acc else 0
                if step % swap_every == 0:
                    s = step // swap_every
                    adapting = s * swap_every <= adapt_steps
                    for q in range(s % 2, R - 1, 2):
                        logu = swap_logu(seed, first_chain + l * R + q, s)
                        logs = (beta[q] - beta[q + 1]) * (lps[q + 1] - lps[q])
                        att[l, q] += 1
                        att_f[l, q] += 0 if adapting else 1
                        if bool(logu < logs):
                            xs[q], xs[q + 1] = xs[q + 1], xs[q]
                            lps[q], lps[q + 1] = lps[q + 1], lps[q]
                            swp[l, q] += 1
                            swp_f[l, q] += 0 if adapting else 1
                        if adapting and not bool(np.isnan(logs)):
                            a = r(1) if bool(logs >= r(0)) else exp(logs)
                            rho[q] = clamp(rho[q] + gam[s - 1] * (a - tr), lo, hi)
                    if adapting:
                        beta, sc = ladder(rho)
                    rounds[s - 1, l] = beta
                if step == save_next and slot < N:
                    record()
                    save_next += thinning
            for q in range(R):
                fx[:, l * R + q], flp[l * R + q] = xs[q], lps[q]
            fbeta[l], frho[l] = beta, rho
    return dict(samples=samples, accepted=accepted, final_x=fx, final_lp=flp, accept_counts=cnt, swap_attempts=att, swap_counts=swp,
                betas=fbeta, betas_rounds=rounds, rho=frho, frozen_attempts=att_f, frozen_counts=swp_f)
