"""Extended-precision reference of the device diagnostics (include/mhx.h: mhx_run_diagnostics, mhx_run_ess_bulk_tail), with a
running error bound for every quantity it returns.

Written from the formulas of the header, in numpy's 80-bit `longdouble` (u = 2^-64: five orders below the fp64 bounds it serves):

  per (half-)chain c of n draws   m_c = mean, s2_c = unbiased variance
  sum_m = sum_c m_c   sum_m2 = sum_c m_c^2   sum_v = sum_c s2_c             over all M (half-)chains
  W = sum_v / M   Vm = (sum_m2 - sum_m^2 / M) / (M - 1)   var+ = (n-1)/n W + Vm   R-hat = sqrt(var+ / W)
  A_t = sum_{c in subset} sum_s (x_s - m_c)(x_{s+t} - m_c) / (M' (n - 1))   the first `ess_chains` chains (both halves of each)
  rho_t = 1 - (A_0 - A_t) / var+    (M == 1: var+ := A_0)
  P_m = rho_2m + rho_2m+1, m < nlag / 2, nlag = min(max_lag + 1, n) rounded down to even
  tau = -1 + 2 sum_m min(P_0 .. P_m) up to the first P_m <= 0 (none: "truncated" at max_lag), floored at 1e-3
  ESS = M n / tau

split: halves of n = floor(N/2) draws, the last draw of an odd N dropped.  A row without variance (A_0 <= 0 or var+ <= 0) or with a
non-finite draw among those read has no ESS: NaN; its R-hat is NaN when W == Vm == 0 and +inf when W == 0 < Vm.

THE BOUNDS model how the sums are accumulated -- which width, how many terms in a row -- and nothing else; they are computed from
the data of the reference alone.  u64 = 2^-53, u32 = 2^-24, gamma_n(u) = n u / (1 - n u) (Higham 2002, section 3.1):
  m_c      an fp64 sum of the n differences to the chain's first draw: gamma_{n+2}(u64) sum|x - x_0| / n + u64 |m|
  s2_c     an fp64 sum of n squares about the computed mean: gamma_{n+4}(u64) sum e^2 + 2 dm |sum e| + n dm^2, over n - 1
  sum_*    the per-chain errors added, + gamma_r(u64) sum|terms| for the r additions of the reduction (a wave's 6 shuffle steps, 3
           adds over the block's waves, one atomic per block and half)
  A_t      in the width w of the build: two subtractions and at most 512 fused multiply-adds in a row per accumulator
           (gamma_{min(512, ceil((n-t)/2)) + 2}(u_w) sum|terms|), then fp64: two adds per flush of 1024 terms, 6 shuffle steps, one
           atomic per block of 64 chains and half; the per-chain mean as used is off by delta = dm (+ ulp_w(m)/2 in fp32, where it
           is rounded to the width), which enters as delta |sum(x_s - m) + sum(x_{s+t} - m)| + (n - t) delta^2
  var+     of R-hat: from the three sums as the caller combines them, Vm through the cancellation sum_m2 - sum_m^2 / M in fp64; of
           the ESS: Vm as sum_c (m_c - sum_m / M)^2 / (M - 1), each m_c off by dm and the centre by the bound of sum_m / M
  P_m      (2 eps_0 + eps_2m + eps_2m+1) / var+ plus the relative bound of var+ times (|A_0 - A_2m| + |A_0 - A_2m+1|) / var+, with two
           refinements that only tighten it: rho_t reads A_0 - A_t, in which the mean's delta is the SAME in both terms, so it
           enters as delta |E_t - E_0| + t delta^2 (E_t the sum of sums above); and A_0 - A_0 is exactly 0 in any arithmetic
  tau      2 sum_m dP_m while the truncation index holds (see `margin`), ESS: the relative bound of tau
An input that is itself uncertain (the normal scores: `dx`, absolute, per draw) adds its first- and second-order terms to each.

`margin` is the smallest |P_m| / bound(P_m) over the pairs that decide the truncation index (those summed, and the one that stops
the sum): a crafted input is only fit for a comparison at `k` times the bounds when margin > k, because ESS steps with the index.
Autocovariances are computed up to the truncating pair only (`A`, `P` hold that prefix): nothing behind it enters tau.
"""
import math

import numpy as np

LD = np.longdouble
U = {"f64": LD(2) ** -53, "f32": LD(2) ** -24}
NPW = {"f64": np.float64, "f32": np.float32}
MARGIN = 4                      # the comparisons run at MARGIN x bound
SCORE_ULPS = 4                  # what the device's normal score may differ from the reference's, in ulp of the device width


def gamma(n, u):
    return LD(n) * u / (LD(1) - LD(n) * u)


def nlag_rule(max_lag, n):
    k = 0 if max_lag < 1 else max_lag + 1
    return min(k, n) & ~1


def halves(x, split):
    """[n][M]: the (half-)chains side by side, first halves then second halves"""
    N = x.shape[0]
    if not split:
        return x
    h = N // 2
    return np.concatenate([x[:h], x[h:2 * h]], axis=1)


def series_stats(x, width, max_lag=0, ess_chains=0, split=False, dx=None):
    """x [N][C] (values of the device width, any float dtype) -> dict of the quantities above and their bounds (`b_<name>`)"""
    u64, uw = U["f64"], U[width]
    N, C = x.shape
    parts = 2 if split else 1
    H = halves(np.asarray(x), split)
    n, M = H.shape
    out = dict(n=n, M=M, parts=parts)
    nan = LD("nan")
    if not np.isfinite(np.asarray(H, dtype=np.float64)).all():
        for k in ("sum_m", "sum_m2", "sum_v", "rhat", "ess", "tau"):
            out[k], out["b_" + k] = nan, nan
        out.update(truncated=False, margin=math.inf, A=np.zeros(0, LD), P=np.zeros(0, LD), nlag=nlag_rule(max_lag, n))
        return out
    H = H.astype(LD)
    D = None if dx is None else halves(np.asarray(dx), split).astype(LD)
    m = H.sum(axis=0) / n
    e = H - m
    ss = (e * e).sum(axis=0)
    v = ss / (n - 1) if n > 1 else np.zeros(M, LD)
    dm = gamma(n + 2, u64) * np.abs(H - H[0]).sum(axis=0) / n + u64 * np.abs(m)
    b_ss = gamma(n + 4, u64) * ss + 2 * dm * np.abs(e.sum(axis=0)) + n * dm * dm
    if D is not None:
        dm = dm + D.sum(axis=0) / n
        b_ss = b_ss + 2 * (np.abs(e) * D).sum(axis=0) + (D * D).sum(axis=0) + 2 * dm * D.sum(axis=0)
    b_v = b_ss / (n - 1) + u64 * v if n > 1 else np.zeros(M, LD)
    g_red = gamma(6 + 3 + parts * ((C + 255) // 256), u64)
    sum_m, sum_m2, sum_v = m.sum(), (m * m).sum(), v.sum()
    b_sum_m = dm.sum() + g_red * np.abs(m).sum()
    b_sum_m2 = (2 * np.abs(m) * dm + dm * dm + u64 * m * m).sum() + g_red * sum_m2
    b_sum_v = b_v.sum() + g_red * sum_v
    out.update(sum_m=sum_m, sum_m2=sum_m2, sum_v=sum_v, b_sum_m=b_sum_m, b_sum_m2=b_sum_m2, b_sum_v=b_sum_v, mean=m, var=v)
    # W, Vm, var+, R-hat: fp64 on the host from the three sums (Vm through the cancellation sum_m2 - sum_m^2 / M)
    W = sum_v / M
    b_W = b_sum_v / M + u64 * W
    if M > 1:
        Vm = ((m - sum_m / M) ** 2).sum() / (M - 1)
        b_Vm = (b_sum_m2 + (2 * abs(sum_m) * b_sum_m + b_sum_m ** 2) / M + 3 * u64 * (sum_m2 + sum_m * sum_m / M)) / (M - 1) + u64 * Vm
        varp = LD(n - 1) / n * W + Vm
        b_varp = b_W + b_Vm + 2 * u64 * varp
        if W > 0:
            rhat = np.sqrt(varp / W)
            rel = 0.5 * (b_varp / varp + b_W / W) + 2 * u64
            b_rhat = rhat * rel / (1 - rel)
        else:
            rhat, b_rhat = (nan if Vm == 0 else LD("inf")), LD(0)
        # the var+ of the ESS takes Vm about the mean of the chain means (fp64, the same reduction): no cancellation
        dd = dm + b_sum_m / M + u64 * np.abs(m - sum_m / M)
        b_Vm_ess = ((2 * np.abs(m - sum_m / M) * dd + dd * dd).sum() + gamma(6 + 3 + 3 + parts * ((C + 255) // 256), u64) * Vm * (M - 1)) / (M - 1) + u64 * Vm
        b_varp_ess = b_W + b_Vm_ess + 2 * u64 * varp
        out.update(W=W, Vm=Vm, varp=varp, b_varp=b_varp, b_varp_ess=b_varp_ess, rhat=rhat, b_rhat=b_rhat)
    else:
        varp = b_varp = None
        out.update(W=W, rhat=nan, b_rhat=nan)
    nlag = nlag_rule(max_lag, n)
    out["nlag"] = nlag
    if nlag < 2:
        out.update(ess=nan, b_ess=nan, tau=nan, b_tau=nan, truncated=False, margin=math.inf, A=np.zeros(0, LD), P=np.zeros(0, LD))
        return out
    # the autocovariances over the subset: the first nc chains, both halves of each
    nc = C if ess_chains <= 0 else min(ess_chains, C)
    cols = np.concatenate([np.arange(nc) + part * C for part in range(parts)])
    es = e[:, cols]
    Ds = None if D is None else D[:, cols]
    ms = m[cols]
    delta = dm[cols]
    if width == "f32":
        delta = delta + np.spacing((np.abs(ms) + delta).astype(np.float32)).astype(LD) / 2
    Mnc = nc * parts
    g_tail = 6 + parts * ((nc + 63) // 64)
    csum = np.concatenate([np.zeros((1, Mnc), LD), np.cumsum(es, axis=0)])

    def acov(t):
        a, b = es[:n - t], es[t:]
        p = a * b
        absS = np.abs(p).sum()
        nw = min(512, (n - t + 1) // 2)
        bound = gamma(nw + 2, uw) * absS + gamma(2 * ((n - t) // 1024 + 1) + g_tail, u64) * absS
        E = csum[n - t] + (csum[n] - csum[t])
        shift = (delta * np.abs(E) + (n - t) * delta * delta).sum()
        # the same delta shifts A_0 and A_t: in A_0 - A_t, which is all that rho_t reads of them, (n - t) delta^2 of it cancels
        shift_diff = (delta * np.abs(E - 2 * csum[n]) + t * delta * delta).sum()
        if Ds is not None:
            da, db = Ds[:n - t], Ds[t:]
            bound = bound + (da * np.abs(b) + np.abs(a) * db + da * db).sum() + (delta * (da + db).sum(axis=0)).sum()
        A = p.sum() / (LD(Mnc) * (n - 1))
        rnd = bound / (LD(Mnc) * (n - 1)) + 2 * u64 * abs(A)
        eps_round.append(rnd)
        eps_diff.append(shift_diff / (LD(Mnc) * (n - 1)))
        return A, rnd + shift / (LD(Mnc) * (n - 1))

    eps_round, eps_diff = [], []
    A0, eps0 = acov(0)
    A, eps = [A0], [eps0]
    vp = varp if M > 1 else A0
    out["nc"] = nc
    if not (A0 > 0) or not (vp > 0):
        out.update(ess=nan, b_ess=nan, tau=nan, b_tau=nan, truncated=False, margin=math.inf, A=np.array(A), P=np.zeros(0, LD))
        return out
    relv = (b_varp_ess / varp) if M > 1 else eps0 / A0
    relv = relv / (1 - relv)
    tau, prev, b_tau, truncated, margin = LD(-1), LD("inf"), LD(0), True, math.inf
    P, bP = [], []
    for j in range(nlag // 2):
        for t in (2 * j, 2 * j + 1):
            if t:
                a_t, e_t = acov(t)
                A.append(a_t)
                eps.append(e_t)
        a0, a1 = A[2 * j], A[2 * j + 1]
        pm = (1 - (A0 - a0) / vp) + (1 - (A0 - a1) / vp)
        b = sum(0 if t == 0 else eps_round[0] + eps_round[t] + eps_diff[t] for t in (2 * j, 2 * j + 1)) / vp
        b = b + (abs(A0 - a0) + abs(A0 - a1)) / vp * relv + 8 * u64
        P.append(pm)
        bP.append(b)
        margin = min(margin, float(abs(pm) / b))
        if not pm > 0:
            truncated = False
            break
        pm = min(pm, prev)
        prev = pm
        tau += 2 * pm
        b_tau += 2 * b
    b_tau += 4 * u64 * (len(P) + 1) * max(abs(tau), LD(1))
    if tau < LD("1e-3"):
        tau = LD("1e-3")
    ess = LD(M) * n / tau
    rel = b_tau / tau
    b_ess = ess * (rel / (1 - rel) + 2 * u64) if rel < 1 else LD("inf")
    out.update(A=np.array(A), b_A=np.array(eps), P=np.array(P), b_P=np.array(bP), tau=tau, b_tau=b_tau, ess=ess, b_ess=b_ess,
               truncated=truncated, margin=margin)
    return out


# ---- rank normalisation -------------------------------------------------------------------------------------------------------
def average_ranks(flat):
    """1-based ranks, the run of equal draws sharing the mean of its positions (tiedrank)"""
    order = np.argsort(flat, kind="stable")
    srt = flat[order]
    new = np.concatenate([[True], srt[1:] != srt[:-1]])
    first = np.flatnonzero(new)
    last = np.concatenate([first[1:], [len(flat)]]) - 1
    grp = np.cumsum(new) - 1
    ranks = np.empty(len(flat), dtype=np.float64)
    ranks[order] = 0.5 * (first[grp] + last[grp]) + 1.0
    return ranks


_score_cache = {}


def normal_scores(ranks, S):
    """Phi^-1((rank - 3/8) / (S + 1/4)) as longdouble: scipy's ndtri (a few ulp of fp64) and one Newton step in 30 digits"""
    import mpmath
    from scipy.special import ndtri
    key2 = np.round(2 * ranks).astype(np.int64)
    uniq, inv = np.unique(key2, return_inverse=True)
    vals = np.empty(len(uniq), dtype=LD)
    with mpmath.workdps(30):
        for i, k in enumerate(uniq):
            z = _score_cache.get((int(k), S))
            if z is None:
                p = (mpmath.mpf(int(k)) / 2 - mpmath.mpf(3) / 8) / (mpmath.mpf(S) + mpmath.mpf(1) / 4)
                z0 = mpmath.mpf(float(ndtri(float(p))))
                z1 = z0 - (mpmath.ncdf(z0) - p) / mpmath.npdf(z0)
                hi = float(z1)
                z = LD(hi) + LD(float(z1 - mpmath.mpf(hi)))
                _score_cache[(int(k), S)] = z
            vals[i] = z
    return vals[inv]


def bulk_tail(x, width, max_lag, ess_chains=0, split=True, ordinal=False):
    """x [N][C] -> dict(bulk=series_stats of the normal scores, lo=, hi= of the two indicators, ess_bulk, ess_tail + bounds, flags,
    z, ind_lo, ind_hi).  The scores are rounded to the device width; the device's may differ from that by 4 ulp of the width."""
    N, C = x.shape
    S = N * C
    flat = np.asarray(x).reshape(-1)
    nan = LD("nan")
    if np.isnan(flat).any():
        return dict(ess_bulk=nan, ess_tail=nan, b_ess_bulk=nan, b_ess_tail=nan, bulk_truncated=False, tail_truncated=False,
                    margin=math.inf)
    ranks = average_ranks(flat) if not ordinal else (np.argsort(np.argsort(flat, kind="stable"), kind="stable") + 1.0)
    z = normal_scores(ranks, S).astype(NPW[width]).reshape(N, C)
    dz = SCORE_ULPS * np.spacing(np.abs(z)).astype(LD)
    srt = np.sort(flat)
    q05, q95 = srt[int(0.05 * (S - 1))], srt[int(0.95 * (S - 1))]
    lo, hi = (np.asarray(x) <= q05).astype(np.float64), (np.asarray(x) <= q95).astype(np.float64)
    b = series_stats(z, width, max_lag, ess_chains, split, dx=dz)
    l = series_stats(lo, width, max_lag, ess_chains, split)
    h = series_stats(hi, width, max_lag, ess_chains, split)
    out = dict(bulk=b, lo=l, hi=h, z=z, ind_lo=lo, ind_hi=hi, ranks=ranks.reshape(N, C), ess_bulk=b["ess"], b_ess_bulk=b["b_ess"],
               bulk_truncated=b["truncated"])
    margin = min(b["margin"], l["margin"], h["margin"])
    if np.isnan(l["ess"]) or np.isnan(h["ess"]):
        out.update(ess_tail=nan, b_ess_tail=nan, tail_truncated=False)
    else:
        t = l if l["ess"] < h["ess"] else h
        out.update(ess_tail=t["ess"], b_ess_tail=t["b_ess"], tail_truncated=t["truncated"])
    out["margin"] = margin
    return out


def tail_interval(bt, k=MARGIN):
    """min() is monotone in both arguments: with each indicator's ESS within k bounds of its reference, the smaller of the device's two
    lies in [min(l - k b_l, h - k b_h), min(l + k b_l, h + k b_h)] whichever of the two the device picks"""
    l, h = bt["lo"], bt["hi"]
    return (min(l["ess"] - k * l["b_ess"], h["ess"] - k * h["b_ess"]), min(l["ess"] + k * l["b_ess"], h["ess"] + k * h["b_ess"]))


# ---- the crafted tensor -------------------------------------------------------------------------------------------------------
def ar1(rng, N, C, phi):
    """stationary AR(1), unit innovation variance: [N][C] float64"""
    x = np.empty((N, C))
    x[0] = rng.normal(size=C) / math.sqrt(1 - phi * phi)
    eps = rng.normal(size=(N, C))
    for t in range(1, N):
        x[t] = phi * x[t - 1] + eps[t]
    return x


PHIS = (0.0, 0.5, 0.9)
AFFINE = ((0.0, 1.0), (1e4, 0.01), (-3e5, 10.0))
ROWS = (["ar%g@%g*%g" % (phi, off, sc) for off, sc in AFFINE for phi in PHIS] +
        ["mh", "const", "const_per_chain", "nan", "neg_nan", "pos_inf", "neg_inf"])
FINITE = list(range(10))
R_CONST, R_CONST_PC, R_NAN, R_NEG_NAN, R_PINF, R_NINF = range(10, 16)
DIM = len(ROWS) - 1             # the last row is the run's lp row: the chain sitting at -inf


def crafted(N, C, width, seed):
    """[N][16][C] in the device width, chain index fastest: the rows of ROWS"""
    rng = np.random.default_rng(seed)
    x = np.empty((N, len(ROWS), C))
    r = 0
    for off, sc in AFFINE:
        for phi in PHIS:
            x[:, r, :] = off + sc * ar1(rng, N, C, phi)
            r += 1
    # Metropolis-like: a proposal is taken with probability 0.3, else the state repeats (long runs of ties)
    prop = ar1(rng, N, C, 0.5)
    take = rng.random(size=(N, C)) < 0.3
    take[0] = True
    idx = np.maximum.accumulate(np.where(take, np.arange(N)[:, None], 0), axis=0)
    x[:, r, :] = np.take_along_axis(prop, idx, axis=0)
    x[:, R_CONST, :] = 1.5                                          # 1.5 M and 2.25 M are exact: Vm is exactly 0
    x[:, R_CONST_PC, :] = 0.7312 + 0.1 * np.arange(C)[None, :]       # not dyadic: the chain's mean has to come out exact all the same
    for row in (R_NAN, R_NEG_NAN, R_PINF, R_NINF):
        x[:, row, :] = ar1(rng, N, C, 0.5)
    t, c = N // 3, C // 2
    x[t, R_NAN, c] = np.nan
    x[t, R_PINF, c] = np.inf
    x[N // 4:N // 4 + max(1, N // 8), R_NINF, C - 1] = -np.inf     # a stretch of one chain
    x = x.astype(NPW[width])
    bits = {"f64": np.uint64, "f32": np.uint32}[width]
    neg = np.array(np.nan, dtype=NPW[width]).view(bits) | (bits(1) << bits(63 if width == "f64" else 31))
    x[t, R_NEG_NAN, c] = neg.view(NPW[width])
    assert np.signbit(x[t, R_NEG_NAN, c]) and not np.signbit(x[t, R_NAN, c])
    return np.ascontiguousarray(x)


# (N, C, max_lag, ess_chains, split, seed): a handful out of C in {1, 3, 63, 64, 65, 256, 257}, N in {4, 5, 97, 401, 1100}, ess_chains in
# {0, 1, 63, 64, 65, C-1}, max_lag in {1, 2, 3, N-1, N, 10 N}.  N = 1100 with max_lag = 80: N - k crosses 1024, 1025 and 1026, the
# flush of the fp32 accumulators and its remainder loop.  Seeds: fixed, chosen so that every finite row meets the truncation margin.
CASES = [
    (4, 1, 3, 0, False, 1),
    (5, 3, 1, 1, True, 1),
    (5, 63, 2, 0, False, 1),
    (97, 64, 3, 63, True, 1),
    (97, 65, 97, 64, False, 2),
    (97, 256, 970, 65, True, 1),
    (97, 257, 96, 256, False, 2),
    (401, 3, 200, 0, True, 7),
    (401, 65, 4010, 1, True, 1),
    (1100, 3, 80, 0, False, 4),
]
# the lag limit: more lags than one launch's grid.z holds (65535 on every HIP device so far)
LONG_CASE = (131073, 1, 65600, 0, False, 9)


def case_id(case):
    return "N%d-C%d-lag%d-nc%d-%s" % (case[0], case[1], case[2], case[3], "split" if case[4] else "whole")


_ref_cache = {}


def reference(case, width, rows=None, bulk=True):
    """(tensor, {row: series_stats}, {row: bulk_tail}) of a case, computed once per process"""
    key = (case, width, None if rows is None else tuple(rows), bulk)
    if key not in _ref_cache:
        N, C, max_lag, ess_chains, split, seed = case
        x = crafted(N, C, width, seed) if case != LONG_CASE else long_tensor(width)
        rr = range(x.shape[1]) if rows is None else rows
        st = {r: series_stats(x[:, r, :], width, max_lag, ess_chains, split) for r in rr}
        bt = {r: bulk_tail(x[:, r, :], width, max_lag, ess_chains, split) for r in rr} if bulk else {}
        _ref_cache[key] = (x, st, bt)
    return _ref_cache[key]


def long_tensor(width):
    N, C, _, _, _, seed = LONG_CASE
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([ar1(rng, N, C, 0.5), 3.0 + 0.5 * ar1(rng, N, C, 0.7)], axis=1).astype(NPW[width]))
