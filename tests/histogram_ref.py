"""The arithmetic spec of the device histograms (include/mhx.h: mhx_run_histogram / mhx_run_histogram2d) restated in numpy, and the
direct-sum Gaussian kernel density estimate `Chains.density` is held to.  A draw is widened to float64, the edges are float64, and
for non-decreasing finite edges e[0..B]:
    NaN -> outside[2];  x < e[0] -> outside[0] (below);  x > e[B] -> outside[1] (above);
    otherwise bin (number of edges <= x) - 1 = searchsorted(e, x, 'right') - 1, and x == e[B] closes the last bin."""
import math

import numpy as np


def bins_of(x, edges):
    """(j int64 [n], ok bool [n]): the bin of every draw that has one"""
    x, e = np.asarray(x, dtype=np.float64).ravel(), np.asarray(edges, dtype=np.float64)
    B = len(e) - 1
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(x) & ~(x < e[0]) & ~(x > e[B])
    j = np.searchsorted(e, np.where(ok, x, e[0]), "right") - 1
    j[j == B] = B - 1
    return j, ok


def histogram_numpy(x, edges):
    """(counts int64 [B], outside int64 [3] = below, above, nan)"""
    x, e = np.asarray(x, dtype=np.float64).ravel(), np.asarray(edges, dtype=np.float64)
    j, ok = bins_of(x, e)
    with np.errstate(invalid="ignore"):
        outside = np.array([np.sum(x < e[0]), np.sum(x > e[-1]), np.sum(np.isnan(x))], dtype=np.int64)
    return np.bincount(j[ok], minlength=len(e) - 1).astype(np.int64), outside


def histogram2d_numpy(x, y, xedges, yedges):
    """(H int64 [B][B], outside): cell [bin of x][bin of y] of the draws that have a bin on both axes"""
    B = len(xedges) - 1
    assert len(yedges) - 1 == B
    jx, okx = bins_of(x, xedges)
    jy, oky = bins_of(y, yedges)
    ok = okx & oky
    H = np.bincount(jx[ok] * B + jy[ok], minlength=B * B).reshape(B, B).astype(np.int64)
    return H, int(np.sum(~ok))


def histogram_rows(value, params, edges):
    """the 1-D form on a tensor [N][d1][C]: (counts [m][B], outside [m][3])"""
    got = [histogram_numpy(value[:, p, :], e) for p, e in zip(params, edges)]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def histogram2d_rows(value, params, edges, pairs):
    """the 2-D form: (counts [npairs][B][B], outside [npairs]), pairs = slots into params"""
    got = [histogram2d_numpy(value[:, params[a], :], value[:, params[b], :], edges[a], edges[b]) for a, b in pairs]
    return np.stack([g[0] for g in got]), np.array([g[1] for g in got], dtype=np.int64)


def kde_direct(draws, grid, h):
    """sum over the draws of phi_h(grid[k] - x) / S, float64, the draws themselves (no binning)"""
    x, grid = np.asarray(draws, dtype=np.float64).ravel(), np.asarray(grid, dtype=np.float64)
    out = np.zeros(len(grid))
    for k0 in range(0, len(x), 4096):
        z = (grid[:, None] - x[None, k0:k0 + 4096]) / h
        out += np.exp(-0.5 * z * z).sum(axis=1)
    return out / (len(x) * h * math.sqrt(2.0 * math.pi))
