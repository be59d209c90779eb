"""Test-side restatement of the anchored-ladder arithmetic: ladders of random-walk Metropolis-Hastings chains
on target^beta * q^(1 - beta), q a diagonal Gaussian of known normaliser, whose neighbouring rungs swap states -- and of what the log
evidence is made of (section 6.5.9) -- in plain Python with numpy scalars of the run's width.

Composed ONLY from the oracle's exported primitives and the helpers of tests/tempered_restatement.py (themselves the oracle's); it
imports nothing from the engine.  Every operation rounds once, in the run's width; nothing is contracted but where fma is written."""
import math

import numpy as np

from oracle import oracle as O

import tempered_restatement as P

r, fma = P.r, P.fma


def reference_tables(betas, mean, sd):
    """omb[r] = 1 - beta[r] of the rounded betas; m[k] rounded once; w[k] = 1 / sd[k] in double, rounded once;
    lc = -sum_k log sd[k] - (d / 2) log 2 pi in double with libm, k ascending, rounded once"""
    beta = [r(b) for b in betas]
    omb = [r(1.0) - b for b in beta]
    m = [r(float(v)) for v in mean]
    w = [r(1.0 / float(s)) for s in sd]
    lc = 0.0
    for s in sd:
        lc -= math.log(float(s))
    lc -= 0.5 * float(len(sd)) * math.log(2.0 * 3.14159265358979323846)
    return omb, m, w, r(lc)


def logq(x, m, w, lc):
    """z_k = (x_k - m_k) * w_k; acc = fma(z_k, z_k, acc) from 0, k ascending; lq = fma(-0.5, acc, lc)"""
    acc = r(0.0)
    for k in range(len(m)):
        z = (r(x[k]) - m[k]) * w[k]
        acc = fma(z, z, acc)
    return fma(r(-0.5), acc, lc)


def run(target, prop_kind, sigma, betas, mean, sd, n_samples, seed, first_chain, nchains, swap_every=1, scales=None, discard_initial=0,
        thinning=1, init=None, swap_lq=True):
    """tempered_restatement.run with the anchored transition and swap.  swap_lq = False exchanges x and lp but leaves lq where it was:
    a deliberately wrong sampler, for the test that shows the detailed-balance check can fail.  Returns what that run returns."""
    R = len(betas)
    d = len(mean)
    assert nchains % R == 0 and first_chain % R == 0
    nl = nchains // R
    beta, dbeta, sig = P.tables(betas, prop_kind, sigma, d, scales)
    omb, m, w, lc = reference_tables(betas, mean, sd)
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
            xs, lps, lqs = [], [], []
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
                lqs.append(logq(x, m, w, lc))
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
                    lqy = logq(y, m, w, lc)
                    loga = beta[q] * (lpy - lps[q]) + omb[q] * (lqy - lqs[q])
                    acc = bool(r(O.accept_logu(seed, cid, step)) < loga)
                    if acc:
                        xs[q], lps[q], lqs[q] = y, lpy, lqy
                        cnt[l * R + q] += 1
                    last[q] = 1 if acc else 0
                if swap_every > 0 and step % swap_every == 0:
                    s = step // swap_every
                    for q in range(s % 2, R - 1, 2):
                        logu = P.swap_logu(seed, first_chain + l * R + q, s)
                        u_lo, u_hi = lps[q] - lqs[q], lps[q + 1] - lqs[q + 1]
                        logs = dbeta[q] * (u_hi - u_lo)
                        att[l, q] += 1
                        if bool(logu < logs):
                            xs[q], xs[q + 1] = xs[q + 1], xs[q]
                            lps[q], lps[q + 1] = lps[q + 1], lps[q]
                            if swap_lq:
                                lqs[q], lqs[q + 1] = lqs[q + 1], lqs[q]
                            swp[l, q] += 1
                if step == save_next and slot < N:
                    record()
                    save_next += thinning
            for q in range(R):
                fx[:, l * R + q], flp[l * R + q] = xs[q], lps[q]
    return dict(samples=samples, accepted=accepted, final_x=fx, final_lp=flp, accept_counts=cnt, swap_attempts=att, swap_counts=swp)


def u_of_samples(samples, betas, mean, sd):
    """u = lp - lq(x) of every saved draw, formed in the run's width, widened: [N][C] float64"""
    _, m, w, lc = reference_tables(betas, mean, sd)
    N, d1, C = samples.shape
    u = np.empty((N, C), dtype=np.float64)
    with np.errstate(all="ignore"):
        for t in range(N):
            for c in range(C):
                u[t, c] = float(r(samples[t, d1 - 1, c]) - logq(samples[t, :d1 - 1, c], m, w, lc))
    return u


def evidence_table(u, betas):
    """What mhx_run_evidence returns, from u [N][C] (float64): per chain bad, shift, s1, s2, max_f, sumexp_f, max_b, sumexp_b -- the
    sums in numpy longdouble over the draws in order, the terms as the spec forms them in fp64 (dbeta the table's value widened, its
    product with u rounded to fp64, exp the oracle's fp64 exp).  Also returns the sums of the absolute terms [C][8] (0 where a field is
    no sum), for the bound a comparison allows."""
    N, C = u.shape
    R = len(betas)
    beta = [r(b) for b in betas]
    dbeta = [float(beta[i] - beta[i + 1]) for i in range(R - 1)]
    dt = O.get_dtype()
    O.set_dtype("f64")
    out = np.zeros((C, 8), dtype=np.float64)
    mag = np.zeros((C, 8), dtype=np.float64)
    ld = np.longdouble
    with np.errstate(all="ignore"):
        for c in range(C):
            q = c % R
            col = u[:, c]
            ok = np.isfinite(col)
            out[c, 0] = float((~ok).sum())
            shift = col[0] if ok[0] else 0.0
            out[c, 1] = shift
            y = (col[ok] - np.float64(shift)).astype(np.float64)
            out[c, 2], mag[c, 2] = float(y.astype(ld).sum()), float(np.abs(y).astype(ld).sum())
            y2 = y.astype(ld) * y.astype(ld)
            out[c, 3], mag[c, 3] = float(y2.sum()), float(y2.sum())
            for k, have, db, sign in ((4, q >= 1, dbeta[q - 1] if q >= 1 else 0.0, 1.0), (6, q + 1 < R, dbeta[q] if q + 1 < R else 0.0, -1.0)):
                lv = sign * (np.float64(db) * col[ok])
                if not have or lv.size == 0:
                    out[c, k], out[c, k + 1] = -np.inf, 0.0
                    continue
                mx = lv.max()
                e = np.array([O.exp(v - mx)[0] for v in lv], dtype=np.float64)
                out[c, k], out[c, k + 1] = mx, float(e.astype(ld).sum())
                mag[c, k + 1] = out[c, k + 1]
    O.set_dtype(dt)
    return out, mag
