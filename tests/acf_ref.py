"""Extended-precision reference of the device autocovariance sums (include/mhx.h: mhx_run_autocovariance) and of what the host
makes of them (mhx.autocorrelation, mhx.integrated_time), with a running error bound for every quantity it returns.

Written from the definitions of the header, in numpy's 80-bit `longdouble` (diag_ref.py: LD, U, gamma):

  per chain c of the range, n draws   m_c = mean,  A_c(k) = sum_{t < n-k} (x_t - m_c)(x_{t+k} - m_c),  ss_c = A_c(0)
  acov[k]  = sum_c A_c(k)                                   (normalise = 0)
  nacov[k] = sum_{c: ss_c > 0} A_c(k) / ss_c,  nvalid = #{c: ss_c > 0}        (normalise = 1)
  rho[k]   = a[k] / a[0] of either (NaN where a[0] is not positive)
  taus[M]  = 2 sum_{k <= M} rho[k] - 1,  window = the first M with M >= c taus[M] (none: M = K, truncated),  tau = taus[window]

A row with a non-finite draw among the chains read is NaN everywhere, nvalid 0.

THE BOUNDS model how the header says the sums are accumulated, and nothing else; they are computed from the data of the reference
alone, the way diag_ref.series_stats builds the bound of its A_t:
  the run-width chain   x - m twice and at most 512 fused multiply-adds in a row: gamma_{min(512, n-k) + 2}(u_w) sum|terms|
  the fp64 adds         gamma_r(u64) sum|terms|: the flushes of a time chunk of 1024 draws (two, and the closing one), 6 shuffle
                        steps, one atomic per (64 chains, chunk) -- ceil(nc / 64) ceil(n / 1024) of them meet in one sum
  the mean as used      m_c is off by delta_c = dm (the fp64 mean's own bound, diag_ref) + half an ulp of the width in fp32, where it
                        is rounded; it enters as delta_c |E_k| + (n - k) delta_c^2, E_k = sum_{t<n-k} e_t + sum_{t>=k} e_t
  normalised            the quotient A_c(k) / ss_c: the numerator's bound over ss_c, plus |A_c(k)| / ss_c times the relative bound of
                        the fp64 ss_c (diag_ref's b_ss: gamma_{n+4}(u64) ss + 2 dm |sum e| + n dm^2), plus the roundings of 1 / ss_c
                        and of the product
  rho                   (b[k] + |rho[k]| b[0]) / (a[0] - b[0]) + an fp64 division; rho[0] is exactly 1
  taus                  2 cumsum(b_rho) + the fp64 cumsum;  b_tau = b_taus[window]
`margin`: every decision M' <= window of the window rule compares M' with c taus[M']; it holds for the device's sums too where
|M' - c taus[M']| > k c b_taus[M'].  margin = the smallest |M' - c taus[M']| / (c b_taus[M']): a row is compared on tau / window at
k = MARGIN times the bounds only where margin > MARGIN, because the window is a step function of the sums.
"""
import math

import numpy as np

from diag_ref import FINITE, LD, MARGIN, ROWS, U, ar1, crafted, gamma  # noqa: F401
from diag_ref import R_CONST, R_CONST_PC, R_NAN, R_NEG_NAN, R_NINF, R_PINF  # noqa: F401

CHUNK, FLUSH = 1024, 512            # MHX_ACF_CHUNK, MHX_ACF_FLUSH of the library, as the header states them


def ratio(a, b):
    """(rho, b_rho) of sums a and their bounds b whose first entry is lag 0 (a[0] > 0)"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    rho = a / a[0]
    den = a[0] - b[0]
    b_rho = (b + np.abs(rho) * b[0]) / den + U["f64"] * np.abs(rho) if den > 0 else np.full(len(a), LD("inf"))
    b_rho[0] = LD(0)                                        # x / x is exactly 1
    return rho, b_rho


def windowed(a, b, c=5.0):
    """a, b [K+1] (sums over lags 0..K and their bounds) -> dict(rho, b_rho, taus, b_taus, tau, b_tau, window, truncated, margin)"""
    u64 = U["f64"]
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    K = len(a) - 1
    nan = LD("nan")
    if not (a[0] > 0) or not np.isfinite(a.astype(np.float64)).all():
        full = np.full(K + 1, nan)
        return dict(rho=full, b_rho=full, taus=full, b_taus=full, tau=nan, b_tau=nan, window=K, truncated=True, margin=math.inf)
    rho, b_rho = ratio(a, b)
    taus = 2 * np.cumsum(rho) - 1
    b_taus = 2 * np.cumsum(b_rho) + 4 * u64 * (np.arange(K + 1) + 1) * np.maximum(np.abs(taus), LD(1))
    idx = np.arange(K + 1)
    hit = np.flatnonzero(idx >= LD(c) * taus)
    truncated = hit.size == 0
    window = K if truncated else int(hit[0])
    gap = np.abs(idx[:window + 1] - LD(c) * taus[:window + 1])
    den = LD(c) * b_taus[:window + 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        mg = np.where(den > 0, gap / np.where(den > 0, den, 1), np.inf)
    return dict(rho=rho, b_rho=b_rho, taus=taus, b_taus=b_taus, tau=taus[window], b_tau=b_taus[window], window=window,
                truncated=truncated, margin=float(mg.min()))


def acf_stats(x, width, lags, chains=None, c=5.0, bounds=True):
    """x [N][C] of one row (values of the device width, any float dtype), lags increasing in [0, N), chains (begin, count) with
    count 0 = to the last -> dict(acov, b_acov, nacov, b_nacov [nlags], nvalid); with lags == 0..K also un = windowed(acov),
    nm = windowed(nacov).  bounds=False: the sums alone (b_* are None), for tensors too large to bound quickly."""
    u64, uw = U["f64"], U[width]
    x = np.asarray(x)
    N, C = x.shape
    begin, count = (0, 0) if chains is None else chains
    count = C - begin if count == 0 else count
    x = x[:, begin:begin + count]
    lags = np.asarray(lags, dtype=np.int64)
    nl = len(lags)
    dense = nl > 0 and np.array_equal(lags, np.arange(nl))
    nan = LD("nan")
    if not np.isfinite(np.asarray(x, dtype=np.float64)).all():
        full = np.full(nl, nan)
        out = dict(acov=full, b_acov=full, nacov=full, b_nacov=full, nvalid=0, finite=False)
        if dense:
            out["un"] = out["nm"] = windowed(full, full, c)
        return out
    n, nc = N, count
    H = x.astype(LD)
    m = H.sum(axis=0) / n
    e = H - m
    ss = (e * e).sum(axis=0)
    valid = ss > 0
    ssv = np.where(valid, ss, LD(1))
    acov, nacov = np.zeros(nl, LD), np.zeros(nl, LD)
    b_acov, b_nacov = (np.zeros(nl, LD), np.zeros(nl, LD)) if bounds else (None, None)
    if bounds:
        dm = gamma(n + 2, u64) * np.abs(H - H[0]).sum(axis=0) / n + u64 * np.abs(m)
        b_ss = gamma(n + 4, u64) * ss + 2 * dm * np.abs(e.sum(axis=0)) + n * dm * dm
        rel_ss = np.where(valid, b_ss / ssv, LD(0))
        rel_ss = rel_ss / (1 - rel_ss)
        delta = dm
        if width == "f32":
            delta = delta + np.spacing((np.abs(m) + delta).astype(np.float32)).astype(LD) / 2
        csum = np.concatenate([np.zeros((1, nc), LD), np.cumsum(e, axis=0)])
        g_chunk = gamma(CHUNK // FLUSH + 1, u64)
        g_red = gamma(CHUNK // FLUSH + 1 + 6 + ((nc + 63) // 64) * ((n + CHUNK - 1) // CHUNK), u64)
    for j, k in enumerate(lags):
        p = e[:n - k] * e[k:]
        A = p.sum(axis=0)
        acov[j] = A.sum()
        nacov[j] = (np.where(valid, A, LD(0)) / ssv).sum()
        if not bounds:
            continue
        absS = np.abs(p).sum(axis=0)
        E = csum[n - k] + (csum[n] - csum[k])
        shift = delta * np.abs(E) + (n - k) * delta * delta
        chain = gamma(min(FLUSH, n - k) + 2, uw) * absS + shift
        b_acov[j] = chain.sum() + g_red * absS.sum() + 2 * u64 * abs(acov[j])
        q = (chain + g_chunk * absS + np.abs(A) * rel_ss) / ssv + 3 * u64 * np.abs(A) / ssv
        b_nacov[j] = np.where(valid, q, LD(0)).sum() + g_red * np.where(valid, absS / ssv, LD(0)).sum() + 2 * u64 * abs(nacov[j])
    out = dict(acov=acov, b_acov=b_acov, nacov=nacov, b_nacov=b_nacov, nvalid=int(valid.sum()), finite=True)
    if dense and bounds:
        out["un"] = windowed(acov, b_acov, c)
        out["nm"] = windowed(nacov, b_nacov, c)
    return out


_cache = {}


def reference(N, C, width, seed, lags, rows=None, chains=None):
    """(tensor, {row: acf_stats}) of diag_ref.crafted(N, C, width, seed), computed once per process"""
    lags = tuple(int(k) for k in lags)
    key = (N, C, width, seed, lags, None if rows is None else tuple(rows), chains)
    if key not in _cache:
        x = tensor(N, C, width, seed)
        rr = range(x.shape[1]) if rows is None else rows
        _cache[key] = (x, {r: acf_stats(x[:, r, :], width, lags, chains) for r in rr})
    return _cache[key]


_tensors = {}


def tensor(N, C, width, seed):
    key = (N, C, width, seed)
    if key not in _tensors:
        _tensors[key] = crafted(N, C, width, seed)
        _tensors[key].setflags(write=False)
    return _tensors[key]


def admitted(st, mode):
    """may this row be compared on tau / window at MARGIN x the bounds?"""
    return st["finite"] and st[mode]["margin"] > MARGIN
