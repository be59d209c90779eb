"""Test-side restatement of the parallel-tempering arithmetic: ladders of random-walk Metropolis-Hastings
chains on pi^beta whose neighbouring rungs swap states, in plain Python with numpy scalars of the run's width.

It is composed ONLY from the oracle's exported primitives -- oracle.normals, accept_logu, philox, u01_open, log, Target.__call__ (or
any callable x -> float) -- and fma / fmaf of the system libm (this Python has no math.fma).  It imports nothing from the engine:
what it computes is what the spec says, not what the kernels do.

Every constant is wrapped in the width's scalar type before it meets another operand, so every operation rounds once, in the run's
width, like the device code built with -ffp-contract=off."""
import ctypes as C
import ctypes.util
import math

import numpy as np

from oracle import oracle as O

STREAM_SWAP = 11

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


def swap_logu(seed, lower_id, s):
    """log of the uniform of swap round s of the pair whose lower slot has global chain id `lower_id`: one Philox block, counter
    (id_lo, id_hi, s, STREAM_SWAP << 28); its first words as accept_logu spends them on its even steps"""
    w = O.philox([lower_id & 0xffffffff, lower_id >> 32, s & 0xffffffff, (STREAM_SWAP << 28) & 0xffffffff], [seed & 0xffffffff, seed >> 32])
    u = O.u01_open(w[0], w[1]) if O.get_dtype() == "f64" else O.u01_open(w[0])
    return r(O.log(r(u))[0])


def default_scales(betas):
    """s_r = beta_r^(-1/2) in float64: 1 / sqrt(beta_r), two correctly rounded operations; s_0 = 1"""
    return [1.0] + [1.0 / math.sqrt(float(b)) for b in list(betas)[1:]]


def tables(betas, prop_kind, sigma, d, scales=None):
    """beta[R] rounded once; dbeta[r] = beta[r] - beta[r + 1] of the rounded values; sig[r][k] = s_r * sigma_k, one product in
    float64 rounded once (ISO: sigma the double scale, DIAG: sigma_k as rounded to the width)"""
    beta = [r(b) for b in betas]
    dbeta = [beta[i] - beta[i + 1] for i in range(len(beta) - 1)]
    s = default_scales(betas) if scales is None else [float(v) for v in scales]
    if prop_kind == O.PROP_ISO:
        sig = [[r(s[i] * float(sigma))] * d for i in range(len(beta))]
    else:
        sig = [[r(s[i] * float(r(sigma[k]))) for k in range(d)] for i in range(len(beta))]
    return beta, dbeta, sig


def run(target, prop_kind, sigma, betas, n_samples, seed, first_chain, nchains, swap_every=1, scales=None, discard_initial=0,
        thinning=1, init=None, swap_sign=1):
    """The chains of a tempered run: `nchains` = nladders * R slots, slot c rung c mod R of ladder c div R, global id first_chain + c.
    Schedule as mcmcsample's: discard_initial = 0 records the initial state as sample 1.  init [d][nchains] or None = the plain run's
    initial draw (stream INIT, step 0, x = fma(sigma, n, 0) with the UNSCALED proposal).  swap_sign = -1 flips the sign of the swap
    ratio: a deliberately wrong sampler, for the test that shows the detailed-balance check can fail.
    Returns samples [N][d + 1][nchains], accepted [N][nchains], final_x, final_lp, accept_counts [nchains], and swap_attempts /
    swap_counts [nladders][R - 1]."""
    R = len(betas)
    d = target.dim if hasattr(target, "dim") else len(init)
    assert nchains % R == 0 and first_chain % R == 0
    nl = nchains // R
    beta, dbeta, sig = tables(betas, prop_kind, sigma, d, scales)
    N = n_samples
    nT = discard_initial + (N - 1) * thinning
    samples = np.empty((N, d + 1, nchains), dtype=O.real())
    accepted = np.zeros((N, nchains), dtype=np.uint8)
    fx = np.empty((d, nchains), dtype=O.real())
    flp = np.empty(nchains, dtype=O.real())
    cnt = np.zeros(nchains, dtype=np.uint32)
    att = np.zeros((nl, R - 1), dtype=np.uint64)
    swp = np.zeros((nl, R - 1), dtype=np.uint64)
    base = [r(sigma)] * d if prop_kind == O.PROP_ISO else [r(v) for v in sigma]
    with np.errstate(all="ignore"):
        for l in range(nl):
            xs, lps = [], []
            for q in range(R):
                c = l * R + q
                cid = first_chain + c
                if init is not None:
                    x = [r(init[k][c]) + r(0) for k in range(d)]
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
                    c = l * R + q
                    samples[slot, :d, c], samples[slot, d, c] = xs[q], lps[q]
                    accepted[slot, c] = last[q]
                slot += 1
            if discard_initial == 0:
                record()
                save_next = thinning
            for step in range(1, nT + 1):
                for q in range(R):
                    cid = first_chain + l * R + q
                    n = O.normals(seed, cid, step, O.STREAM_PROPOSAL, d)
                    y = [fma(sig[q][k], n[k], xs[q][k]) for k in range(d)]
                    lpy = r(target(np.array(y, dtype=O.real())))
                    loga = beta[q] * (lpy - lps[q])
                    acc = bool(r(O.accept_logu(seed, cid, step)) < loga)
                    if acc:
                        xs[q], lps[q] = y, lpy
                        cnt[l * R + q] += 1
                    last[q] = 1 if acc else 0
                if swap_every > 0 and step % swap_every == 0:
                    s = step // swap_every
                    for q in range(s % 2, R - 1, 2):
                        logu = swap_logu(seed, first_chain + l * R + q, s)
                        logs = dbeta[q] * (lps[q + 1] - lps[q])
                        if swap_sign < 0:
                            logs = -logs
                        att[l, q] += 1
                        if bool(logu < logs):
                            xs[q], xs[q + 1] = xs[q + 1], xs[q]
                            lps[q], lps[q + 1] = lps[q + 1], lps[q]
                            swp[l, q] += 1
                if step == save_next and slot < N:
                    record()
                    save_next += thinning
            for q in range(R):
                fx[:, l * R + q], flp[l * R + q] = xs[q], lps[q]
    return dict(samples=samples, accepted=accepted, final_x=fx, final_lp=flp, accept_counts=cnt, swap_attempts=att, swap_counts=swp)
