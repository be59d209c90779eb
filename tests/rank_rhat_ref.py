"""Reference of the rank-normalised split R-hat (include/mhx.h: mhx_run_rank_diagnostics, mhx_run_rank_scores) on top of
tests/diag_ref.py: the bulk scores are diag_ref's, the folded scores are those of the ranks of g = |x - m| with the median m and the
subtraction in the device width, and both R-hat values with their bounds are `series_stats` of the scores (dx = SCORE_ULPS ulp per
score), unchanged.

  m       y[S/2] for an odd S, else y[S/2-1]/2 + y[S/2]/2 in the width (y: the ascending draws of all chains)
  g       np.abs(x - m) in the width
  zf      normal_scores(average_ranks(g)), rounded to the width

`fold_ranks_by_search` restates the device's route to the same ranks (csrc/mhx_diag_kernels.h: mhx_diag_fold_rank) in numpy: no sort
of g, only searches in the two monotone halves of the one sorted array."""
import numpy as np

import diag_ref as R

# the handful of diag_ref.CASES planted here: C in {1, 3, 63, 64, 65, 257}; N = 4 (even) and 5, 97 (odd); S = N C even (4, 6208) and odd
# (15, 315, 6305, 24929); split and whole chains; one chain (R-hat has no answer)
CASES = [c for c in R.CASES if (c[0], c[1]) in ((4, 1), (5, 3), (5, 63), (97, 64), (97, 65), (97, 257))]
assert len(CASES) == 6
# rows of the crafted tensor that have ranks: the finite ones, the constant ones and the two with infinite draws
RANKED = R.FINITE + [R.R_CONST, R.R_CONST_PC, R.R_PINF, R.R_NINF]


def median(flat):
    """Julia's middle() of the middle pair, in the dtype of `flat`"""
    y = np.sort(flat)
    S = len(y)
    with np.errstate(invalid="ignore"):
        return y[S // 2] if S & 1 else y[S // 2 - 1] / 2 + y[S // 2] / 2


def fold(flat):
    """g = |x - m| in the dtype of `flat`, or None when the median is not finite"""
    m = median(flat)
    if not np.isfinite(m):
        return None
    g = np.abs(flat - m)
    assert g.dtype == flat.dtype
    return g


def fold_ranks_by_search(flat):
    """the tie-averaged ranks of fold(flat) as the device finds them: y < m is a prefix of the sorted draws on which g falls, g rises
    on the rest; `less` / `leq` = the draws with g < f / g <= f, counted on each side by a binary search"""
    order = np.argsort(flat, kind="stable")
    y = flat[order]
    m = median(flat)
    g = np.abs(y - m)
    sp = int(np.searchsorted(y, m, side="left"))
    assert (y[:sp] < m).all() and (y[sp:] >= m).all()
    down, up = g[:sp][::-1], g[sp:]                       # both ascending
    assert (down[1:] >= down[:-1]).all() and (up[1:] >= up[:-1]).all(), "rounding broke the monotone halves"
    less = np.searchsorted(down, g, side="left") + np.searchsorted(up, g, side="left")
    leq = np.searchsorted(down, g, side="right") + np.searchsorted(up, g, side="right")
    ranks = np.empty(len(flat), dtype=np.float64)
    ranks[order] = 0.5 * (less + leq - 1.0) + 1.0
    return ranks


def _scored(ranks, S, shape, width, split):
    z = R.normal_scores(ranks, S).astype(R.NPW[width]).reshape(shape)
    dz = R.SCORE_ULPS * np.spacing(np.abs(z)).astype(R.LD)
    return z, R.series_stats(z, width, 0, 0, split, dx=dz)


def rank_rhat(x, width, split):
    """x [N][C] of the device width -> dict(nan=True) for a row that holds a NaN, else dict(z, bulk, ranks, zf, tail, ranks_f) with
    bulk / tail the series_stats of the scores (`rhat`, `b_rhat`); zf = tail = None when the median is not finite"""
    assert x.dtype == R.NPW[width]
    N, C = x.shape
    S = N * C
    flat = np.ascontiguousarray(x).reshape(-1)
    if np.isnan(flat).any():
        return dict(nan=True)
    ranks = R.average_ranks(flat)
    z, bulk = _scored(ranks, S, (N, C), width, split)
    out = dict(nan=False, z=z, bulk=bulk, ranks=ranks, zf=None, tail=None, ranks_f=None)
    g = fold(flat)
    if g is not None:
        ranks_f = R.average_ranks(g)
        zf, tail = _scored(ranks_f, S, (N, C), width, split)
        out.update(zf=zf, tail=tail, ranks_f=ranks_f)
    return out


# ---- rows where the fold can go wrong -----------------------------------------------------------------------------------------
EXTRA_ROWS = ["ints", "two_valued", "exp8", "zeros_at_median", "scale3"]
EXTRA_SHAPES = [(97, 65), (64, 4)]                         # S odd (more than one block of 256 sorted indices) and S even


def extras(N, C, width, seed=11):
    """[N][5][C] in the device width:
      ints             integers uniform on -7..7: exact ties across the two sides of the median
      two_valued       two values only
      exp8             exp(8 normal): 30 orders of magnitude, the subtraction collapses distinct small draws onto one g in fp32
      zeros_at_median  a third of the draws are -0.0 or +0.0 and the median is one of them: a run of draws equal to the median
      scale3           every other chain three times as wide about the same location"""
    rng = np.random.default_rng(seed)
    x = np.empty((N, len(EXTRA_ROWS), C))
    x[:, 0, :] = rng.integers(-7, 8, size=(N, C))
    x[:, 1, :] = np.where(rng.random(size=(N, C)) < 0.4, -1.25, 3.5)
    x[:, 2, :] = np.exp(8.0 * rng.normal(size=(N, C)))
    v = rng.normal(size=(N, C))
    u = rng.random(size=(N, C))
    v[u < 1.0 / 3.0] = 0.0
    v[u < 1.0 / 6.0] = -0.0
    x[:, 3, :] = v
    x[:, 4, :] = rng.normal(size=(N, C)) * np.where(np.arange(C) % 2 == 0, 1.0, 3.0)[None, :]
    x = np.ascontiguousarray(x.astype(R.NPW[width]))
    assert median(x[:, 3, :].reshape(-1)) == 0 and np.signbit(x[:, 3, :]).any()
    return x


# ---- rows without an answer ---------------------------------------------------------------------------------------------------
NOANS_ROWS = ["nan", "half_inf", "inf_pair", "few_inf", "const", "const_per_chain"]
NO_NAN, NO_HALF_INF, NO_INF_PAIR, NO_FEW_INF, NO_CONST, NO_CONST_PC = range(6)


def no_answer(width, N=8, C=4, seed=12):
    """[8][6][4]: a NaN; half of the draws +inf (the median is +inf); -inf and +inf as the middle pair (the median is NaN); two infinite
    draws around a finite median; a constant; a constant per chain"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, len(NOANS_ROWS), C))
    x[3, NO_NAN, 1] = np.nan
    x[::2, NO_HALF_INF, :] = np.inf
    x[:, NO_INF_PAIR, :] = np.where(np.arange(N)[:, None] % 2 == 0, -np.inf, np.inf)
    x[2, NO_FEW_INF, 0], x[5, NO_FEW_INF, 3] = np.inf, -np.inf
    x[:, NO_CONST, :] = 1.5
    x[:, NO_CONST_PC, :] = 0.7312 + 0.1 * np.arange(C)[None, :]
    return np.ascontiguousarray(x.astype(R.NPW[width]))


_cache = {}


def reference(key, width):
    """key: one of CASES, ("extras", N, C) or "no_answer" -> (tensor, split, {row: rank_rhat}), computed once per process"""
    k = (key, width)
    if k not in _cache:
        if key == "no_answer":
            x, split, rows = no_answer(width), True, range(len(NOANS_ROWS))
        elif key[0] == "extras":
            x, split, rows = extras(key[1], key[2], width), True, range(len(EXTRA_ROWS))
        else:
            x, split, rows = R.crafted(key[0], key[1], width, key[5]), key[4], range(len(R.ROWS))
        _cache[k] = (x, split, {r: rank_rhat(x[:, r, :], width, split) for r in rows})
    return _cache[k]
