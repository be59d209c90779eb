"""The yardstick of the HPD tests: MCMCChains' `_hpd` (the Chen-Shao interval) restated in numpy, on the float64 widening of the draws.
With y the ascending order of the S draws and m = max(1, ceil(alpha S)): a = y[:m], b = y[S-m:], i = the first argmin of b - a
(numpy.argmin: a NaN width wins over every number), interval [a[i], b[i]]."""
import math

import numpy as np


def ranks(S, alpha):
    return max(1, int(math.ceil(alpha * float(S))))


def hpd_numpy(x, alpha):
    """(lower, upper) of the draws x (any shape, any float dtype)"""
    y = np.sort(np.asarray(x).ravel().astype(np.float64))
    S = len(y)
    m = ranks(S, alpha)
    a, b = y[:m], y[S - m:]
    with np.errstate(invalid="ignore"):
        i = int(np.argmin(b - a))
    return a[i], b[i]


def hpd_rows(value, alpha):
    """(lower [d1], upper [d1]) of a tensor [N][d1][C], every row pooled over N and C; a row that holds a NaN gives (NaN, NaN), the
    rule of include/mhx.h (mhx_run_hpd)"""
    v = np.asarray(value)
    rows = np.moveaxis(v, 1, 0).reshape(v.shape[1], -1)
    out = np.array([(np.nan, np.nan) if np.isnan(r).any() else hpd_numpy(r, alpha) for r in rows], dtype=np.float64)
    return out[:, 0].copy(), out[:, 1].copy()


def tail_counts(x, alpha):
    """(m, cL, cU): the draws strictly below y[m-1] and strictly above y[S-m] -- what the device gathers and sorts"""
    y = np.sort(np.asarray(x).ravel().astype(np.float64))
    S = len(y)
    m = ranks(S, alpha)
    return m, int((y < y[m - 1]).sum()), int((y > y[S - m]).sum())
