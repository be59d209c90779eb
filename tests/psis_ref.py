"""PSIS-LOO per data row (include/mhx.h: mhx_run_psis) from first principles: the definitions at the prototype,
which are R loo's psis / gpdfit, in numpy's 80-bit longdouble on the matrix l[i, s] that pointwise_ref.host_matrix gives bit for bit.

Exact columns -- tau, lmin, n_below, bad, the tails, T and M -- are draws and counts: the device must equal them bit for bit.  For every
other column the file carries a bound of the DEVICE's computation, derived here from the kernels' order of operations
(csrc/mhx_psis_kernels.h) and not tuned to it.  u = 2^-53; every operation after the widening of l is fp64 in both widths.

  elementary functions   DESIGN.md section 3: exp within 0.90 ulp, log within 0.79 ulp; an ulp is at most 2 u of the value, so relative
          E_EXP = 1.80 u and E_LOG = 1.58 u.  log1p(y) = log(w) y / (w - 1), w = fl(1 + y) (Kahan): the rounding of w cancels to first order,
          the subtraction is exact, one division, one product: E_L1P = E_LOG + 3 u, taken as 5 u.  expm1(y) = (w - 1) y / log(w), w = exp(y):
          likewise E_EXP enters through w on both sides and cancels to first order; E_LOG, a subtraction (exact near 1, u elsewhere), a
          division, a product: taken as 6 u.
  B       a term exp(tau - l): the subtraction rounds once (relative u |tau - l| in the value), exp adds E_EXP; all terms are positive and a
          term passes at most L = N + 6 + 3 + ceil(C / 256) x 64 additions (a lane's draws, the butterfly, the block's waves, the partials in
          index order): gamma_{L + 1}((2.80 + D) u) x B', D = max l - tau capped at 746, plus T x 2^-1021 for terms in the subnormal range;
          then B = B' + (n_eq - (M - n_below)) rounds once.
  c       exp(lmin - tau): (E_EXP + u |lmin - tau|) c.
  x_j     exp(lmin - a) - c: the two exp errors and one rounding; exactly 0 (on both sides) where a = tau.
  fit     theta_j, k_j, L_j, w_j, theta^, k, sigma, khat: no closed bound exists, so first-order propagation through the reference's own
          partial derivatives, absolute values added (fit_bounds below states each step); the sums over the tail run over at most
          ceil(M / 64) + 6 additions (a lane's stride, the butterfly) and the mean divides once.
  lw~_j   through G(khat) = expm1(-khat lp_j) / khat with its TOTAL derivative in khat (the partial ones cancel as khat -> 0), then
          q = sigma G + c and log q (1-Lipschitz in relative terms); min(0, .) is 1-Lipschitz.
  elpd    the two sums run over ceil(M / 256) + 6 + 3 additions of positive terms each carrying its argument's error and E_EXP; the
          two logarithms, then two additions.
Comparisons run at diag_ref.MARGIN x bound (pointwise_ref.within)."""
import math

import numpy as np

import diag_ref
import pointwise_ref as P

LD = np.longdouble
U = LD(2) ** -53
MARGIN = diag_ref.MARGIN
E_EXP, E_LOG, E_L1P, E_EM1 = LD(1.80) * U, LD(1.58) * U, LD(5) * U, LD(6) * U
THREADS, MAX_SLOTS, FIT_THREADS = 256, 64, 256      # MHX_POINTWISE_THREADS, MHX_POINTWISE_MAX_SLOTS, MHX_PSIS_FIT_THREADS
EXACT = ("tau", "lmin", "n_below", "bad")
BOUNDED = ("elpd_loo", "khat", "sigma", "body")


def tail_length(T, reff=1.0):
    """M = min(floor(0.2 T), ceil(3 sqrt(T / reff))) in float64; M < 5 counts as 0"""
    m = min(math.floor(0.2 * float(T)), math.ceil(3.0 * math.sqrt(float(T) / float(reff))))
    return 0 if m < 5 else int(m)


def gamma(k, u):
    return P.gamma(k, u)


def gpd_grid(x):
    """(theta_j, k_j), j = 1 .. m, of the ascending abscissae x: the grid of the fit and the mean log1p(-theta_j x) at each point"""
    x = np.asarray(x, dtype=LD)
    M = x.size
    m = 30 + int(math.floor(math.sqrt(M)))
    with np.errstate(all="ignore"):
        j = np.arange(1, m + 1, dtype=LD)
        theta = 1 / x[M - 1] + (1 - np.sqrt(LD(m) / (j - LD(0.5)))) / (3 * x[int(math.floor(M / 4.0 + 0.5)) - 1])
        return theta, np.log1p(-theta[:, None] * x[None, :]).mean(axis=1)


def gpdfit(x, e_x=None):
    """(khat, sigma, k, theta_hat, fitted) of the ascending abscissae x (longdouble), as the prototype states them -- and, with e_x
    (absolute bounds of the device's x), fit_bounds(...) as a sixth entry.  Not fitted (x* = 0, a non-finite fit, sigma <= 0): khat = inf,
    sigma = NaN."""
    x = np.asarray(x, dtype=LD)
    M = x.size
    m = 30 + int(math.floor(math.sqrt(M)))
    istar = int(math.floor(M / 4.0 + 0.5)) - 1
    with np.errstate(all="ignore"):
        xstar, xmax = x[istar], x[M - 1]
        j = np.arange(1, m + 1, dtype=LD)
        t1 = 1 / xmax
        t2 = (1 - np.sqrt(LD(m) / (j - LD(0.5)))) / (3 * xstar)
        theta = t1 + t2
        tx = theta[:, None] * x[None, :]
        l1 = np.log1p(-tx)
        kj = l1.mean(axis=1)
        Lj = M * (np.log(-theta / kj) - kj - 1)
        w = 1 / np.exp(Lj[None, :] - Lj[:, None]).sum(axis=1)
        th = (w * theta).sum()
        lh = np.log1p(-th * x)
        k = lh.mean()
        sigma = -k / th
        khat = (k * M + 5) / (LD(M) + 10)
    fitted = bool(np.isfinite(th) and np.isfinite(khat) and np.isfinite(sigma) and sigma > 0)
    if not fitted:
        return LD(np.inf), LD(np.nan), k, th, False, None
    bounds = None
    if e_x is not None:
        bounds = fit_bounds(x, np.asarray(e_x, dtype=LD), m, istar, theta, t1, t2, tx, l1, kj, Lj, w, th, lh, k, sigma)
    return khat, sigma, k, th, True, bounds


def fit_bounds(x, e_x, m, istar, theta, t1, t2, tx, l1, kj, Lj, w, th, lh, k, sigma):
    """dict(khat, sigma): absolute first-order bounds of the device's fit.  Each line is |partial derivative| x the bound of its argument,
    plus the roundings of the step itself."""
    M = x.size
    n_tail = (M + 63) // 64 + 6                                 # additions a term of a tail sum passes through
    xstar, xmax = x[istar], x[M - 1]
    # theta_j = 1 / xmax + (1 - sqrt(m / (j - 1/2))) / (3 x*): d/dxmax = -1 / xmax^2, d/dx* = -t2 / x*; a division; a division, a root, a
    # subtraction, a product, a division; an addition
    d_theta = np.abs(t1 / xmax) * e_x[M - 1] + np.abs(t2 / xstar) * e_x[istar] + 6 * U * (np.abs(t1) + np.abs(t2))
    # k_j = mean_i log1p(-theta_j x_i): d/dx_i = -theta_j / (M (1 - theta_j x_i)), d/dtheta_j = mean(-x_i / (1 - theta_j x_i)); the
    # product rounds once (u |t| / |1 - t| in the value), log1p E_L1P, the sum gamma_{n_tail}, the division by M
    den = np.abs(1 - tx)
    d_k = (np.abs(theta)[:, None] * e_x[None, :] / den).sum(axis=1) / M + (np.abs(x)[None, :] / den).mean(axis=1) * d_theta
    d_k = d_k + (E_L1P + gamma(n_tail, U) + U) * np.abs(l1).mean(axis=1) + U * (np.abs(tx) / den).mean(axis=1)
    # L_j = M (log(-theta_j / k_j) - k_j - 1): d/dtheta_j = M / theta_j, d/dk_j = -M (1 / k_j + 1); the quotient (u in the logarithm), the
    # logarithm, two subtractions, the product
    lg = np.abs(np.log(-theta / kj))
    d_L = np.abs(M / theta) * d_theta + M * np.abs(1 / kj + 1) * d_k + M * (U + E_LOG * lg + 2 * U * (lg + np.abs(kj) + 1)) + U * np.abs(Lj)
    # w_j = 1 / sum_j' exp(L_j' - L_j), theta^ = sum_j w_j theta_j: through the softmax d theta^ / dL_j = w_j (theta_j - theta^) and
    # d theta^ / dtheta_j = w_j; the roundings of a weight -- the subtraction (u |L_j' - L_j|, capped where exp has underflown), exp, m
    # additions, the reciprocal -- are relative, and m fused multiply-adds follow
    spread = min(float(Lj.max() - Lj.min()), 746.0)
    rho = E_EXP + U * LD(spread) + gamma(m, U) + U
    wt = np.abs(w * theta).sum()
    d_th = (w * np.abs(theta - th) * d_L).sum() + (w * d_theta).sum() + (rho + gamma(m, U)) * wt
    # k = mean_i log1p(-theta^ x_i), as k_j
    den = np.abs(1 - th * x)
    d_kk = (np.abs(th) * e_x / den).sum() / M + (np.abs(x) / den).mean() * d_th
    d_kk = d_kk + (E_L1P + gamma(n_tail, U) + U) * np.abs(lh).mean() + U * (np.abs(th * x) / den).mean()
    # sigma = -k / theta^; khat = (k M + 5) / (M + 10): a product, an addition, a division
    d_sigma = d_kk / np.abs(th) + np.abs(k) * d_th / (th * th) + U * np.abs(sigma)
    d_khat = M * d_kk / (M + 10) + 3 * U * (np.abs(k) * M + 5) / (M + 10)
    return dict(khat=d_khat, sigma=d_sigma)


def smooth(M, khat, sigma, c, e_khat=0, e_sigma=0, e_c=0):
    """(lw~_j, its absolute bound), j < M ascending, of a fitted tail"""
    p = (np.arange(M, dtype=LD) + LD(0.5)) / M
    lp = np.log1p(-p)
    # p_j: an addition (exact: integers plus a half) and a division; lp_j = log1p(-p_j)
    d_lp = E_L1P * np.abs(lp) + U * p / (1 - p)
    z = -khat * lp
    if khat == 0:
        G, dG = -lp, lp * lp / 2
    else:
        G = np.expm1(z) / khat
        dG = np.where(np.abs(z) < LD(1e-5), lp * lp / 2, (np.exp(z) * (-lp) * khat - np.expm1(z)) / (khat * khat))
    # G = expm1(z) / khat, z = -khat lp: total derivative in khat, dG; in lp, -exp(z); the product z rounds once (exp(z) u |lp| in G),
    # expm1 E_EM1, the division
    d_G = np.abs(dG) * e_khat + np.exp(z) * (d_lp + U * np.abs(lp)) + (E_EM1 + U) * np.abs(G)
    q = sigma * G + c
    d_q = np.abs(G) * e_sigma + sigma * d_G + e_c + 2 * U * (np.abs(sigma * G) + c)
    lw = np.log(q)
    d_lw = d_q / q + E_LOG * np.abs(lw)
    return np.minimum(lw, 0), d_lw


def reference(l, N, nch, reff=1.0):
    """dict of the eight columns, the tails, T and M, with e_<column> for the BOUNDED ones, from l [nrows][N * nch] float64"""
    l = np.asarray(l, dtype=np.float64)
    nrows, T = l.shape
    assert T == N * nch
    M = tail_length(T, reff)
    L_sum = int(N) + 6 + 3 + ((int(nch) + THREADS - 1) // THREADS) * MAX_SLOTS
    n_blk = (M + FIT_THREADS - 1) // FIT_THREADS + 6 + 3
    out = {k: np.full(nrows, np.nan) for k in EXACT}
    out.update({k: np.full(nrows, np.nan, dtype=LD) for k in BOUNDED})
    out.update({"e_" + k: np.full(nrows, np.nan, dtype=LD) for k in BOUNDED})
    out["tails"], out["T"], out["M"] = np.full((nrows, M), np.nan), T, M
    with np.errstate(all="ignore"):
        for i in range(nrows):
            li = l[i]
            nbad = int(T - np.isfinite(li).sum())
            out["bad"][i] = float(nbad)
            if nbad:
                continue
            s = np.sort(li)
            tau = s[M]
            nb, neq = int((li < tau).sum()), int((li == tau).sum())
            a = s[:M]
            lmin = a[0] if M else tau
            out["tau"][i], out["lmin"][i], out["n_below"][i], out["tails"][i] = tau, lmin, float(nb), a
            aL, tauL, lminL = a.astype(LD), LD(tau), LD(lmin)
            c = np.exp(lminL - tauL)
            e_c = (E_EXP + U * np.abs(lminL - tauL)) * c
            above = li[li > tau].astype(LD)
            Bp = np.exp(tauL - above).sum()
            D = min(float(li.max() - tau), 746.0)
            e_B = gamma(L_sum + 1, (LD(2.80) + LD(D)) * U) * Bp + LD(T) * LD(2) ** -1021
            B = Bp + (neq - (M - nb))
            e_B = e_B + U * np.abs(B)
            out["body"][i], out["e_body"][i] = B, e_B
            # the abscissae ascending: x_j belongs to a_(M-1-j)
            ar = aL[::-1]
            ex = np.exp(lminL - ar)
            x = ex - c
            e_x = np.where(ar == tauL, LD(0), (E_EXP + U * np.abs(lminL - ar)) * ex + e_c + U * np.abs(x))
            khat, sigma, fitted, d_lw = LD(np.inf), LD(np.nan), False, None
            out["e_khat"][i] = out["e_sigma"][i] = LD(0)
            if M >= 5 and not (a[M - 1] - a[0] < 2.0 ** -52 / 100.0):
                khat, sigma, _, _, fitted, fb = gpdfit(x, e_x)
                if fitted:
                    out["e_khat"][i], out["e_sigma"][i] = fb["khat"], fb["sigma"]
            if fitted:
                lw, d_lw = smooth(M, khat, sigma, c, fb["khat"], fb["sigma"], e_c)
            else:
                lw = lminL - ar                                 # the raw weights: one subtraction
                d_lw = U * np.abs(lw)
            out["khat"][i], out["sigma"][i] = khat, sigma
            arg = lw + (ar - lminL)
            tn, td = np.exp(arg), np.exp(lw)
            num, den = tn.sum(), td.sum()
            e_num = (tn * (d_lw + U * np.abs(ar - lminL) + U * np.abs(arg) + E_EXP)).sum() + gamma(n_blk, U) * num
            e_den = (td * (d_lw + E_EXP)).sum() + gamma(n_blk, U) * den
            Nn = LD(T - M) + num
            Dn = c * B + den
            e_N = e_num + U * Nn
            e_D = c * e_B + B * e_c + e_den + U * Dn
            lN, lD_ = np.log(Nn), np.log(Dn)
            out["elpd_loo"][i] = lminL + lN - lD_
            out["e_elpd_loo"][i] = e_N / Nn + e_D / Dn + E_LOG * (np.abs(lN) + np.abs(lD_)) + 2 * U * (np.abs(lminL) + np.abs(lN) + np.abs(lD_))
    return out
