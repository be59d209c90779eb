"""Reference and error bound for the cross moments (mhx_*_cross_moments).

sum[i] = sum_k y_ik and cross[i][j] = sum_k y_ik y_jk are sums of K terms each.  Whatever order of fp64 fma / mul / add a kernel uses,
with each term entering once, the error is at most gamma_K * sum_k |y_ik y_jk| (gamma_K * sum_k |y_ik| for `sum`), gamma_K =
K u / (1 - K u), u = 2^-53: Higham's inner-product bound (Accuracy and Stability of Numerical Algorithms, section 3.1); fma only helps.
The bound is derived, not measured; one dropped or doubled draw costs about 1 / K of a sum, far above it.

y is formed here in numpy float64 exactly as the kernel forms it: the draw widened (exact) and ONE IEEE subtraction.  The true sums
are taken in exact rational arithmetic where K m^2 <= 2e5 -- every finite double is an integer multiple of 2^-1074, so the sums run
on Python integers over that common denominator and are compared as fractions.Fraction -- and otherwise in np.longdouble, with the
bound widened by 1 + 2^-10 for the reference's own rounding (64-bit significand: K 2^-64 against K 2^-53)."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
EXACT_LIMIT = 2e5
_SCALE = 1074


def gamma(K):
    return Fraction(K, 2 ** 53) / (1 - Fraction(K, 2 ** 53))


def shifted_rows(value, params, shift):
    """y [m][K] float64 of the rows `params` of a tensor [N][d1][C]: draws in (sample, chain) order, shift None = 0"""
    v = np.asarray(value)
    rows = np.moveaxis(v[:, np.asarray(params, dtype=np.int64), :], 1, 0).reshape(len(params), -1).astype(np.float64)
    s = np.zeros(len(params)) if shift is None else np.asarray(shift, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return rows - s[:, None]


class Moments:
    """exact (or extended-precision) sums of the FINITE rows of y, their absolute sums, and what IEEE gives for the other rows"""

    def __init__(self, y):
        y = np.asarray(y, dtype=np.float64)
        self.m, self.K = y.shape
        self.finite = np.isfinite(y).all(axis=1)
        yz = np.where(self.finite[:, None], y, 0.0)
        self.exact = self.K * self.m * self.m <= EXACT_LIMIT
        if self.exact:
            Y = [[int(Fraction(float(v)) * 2 ** _SCALE) for v in row] for row in yz]
            A = [[abs(v) for v in row] for row in Y]
            d1, d2 = 2 ** _SCALE, 2 ** (2 * _SCALE)
            self.sum = [Fraction(sum(r), d1) for r in Y]
            self.abs_sum = [Fraction(sum(r), d1) for r in A]
            self.cross = [[None] * self.m for _ in range(self.m)]
            self.abs_cross = [[None] * self.m for _ in range(self.m)]
            for i in range(self.m):
                for j in range(i, self.m):
                    c = Fraction(sum(a * b for a, b in zip(Y[i], Y[j])), d2)
                    a = Fraction(sum(a * b for a, b in zip(A[i], A[j])), d2)
                    self.cross[i][j] = self.cross[j][i] = c
                    self.abs_cross[i][j] = self.abs_cross[j][i] = a
            self.widen = Fraction(1)
        else:
            L = yz.astype(np.longdouble)
            A = np.abs(L)
            self.sum, self.abs_sum = L.sum(axis=1), A.sum(axis=1)
            self.cross, self.abs_cross = L @ L.T, A @ A.T
            self.widen = 1.0 + 2.0 ** -10
        # the non-finite rows: IEEE leaves no freedom (a NaN stays, one infinity among finite terms decides the sum)
        with np.errstate(invalid="ignore", over="ignore"):
            self.ieee_sum = y.sum(axis=1)
            self.ieee_cross = y @ y.T

    def subset(self, params):
        """the moments of rows params (any order, repeats allowed) of the same y: entries of these"""
        params = [int(p) for p in params]
        out = Moments.__new__(Moments)
        out.m, out.K, out.exact, out.widen = len(params), self.K, self.exact, self.widen
        out.finite = self.finite[params]
        if self.exact:
            pick = lambda a: [[a[i][j] for j in params] for i in params]      # noqa: E731
            out.sum, out.abs_sum = [self.sum[i] for i in params], [self.abs_sum[i] for i in params]
        else:
            pick = lambda a: a[np.ix_(params, params)]                        # noqa: E731
            out.sum, out.abs_sum = self.sum[params], self.abs_sum[params]
        out.cross, out.abs_cross = pick(self.cross), pick(self.abs_cross)
        out.ieee_sum, out.ieee_cross = self.ieee_sum[params], self.ieee_cross[np.ix_(params, params)]
        return out

    def check(self, got_sum, got_cross, label=""):
        """assert |got - exact| <= bound entrywise on finite rows, the IEEE class elsewhere; returns the largest error / bound"""
        got_sum, got_cross = np.asarray(got_sum), np.asarray(got_cross)
        assert got_sum.shape == (self.m,) and got_cross.shape == (self.m, self.m), label
        worst = 0.0
        fin = np.flatnonzero(self.finite)
        if self.exact:
            g = gamma(self.K)
            for i in fin:
                err, bound = abs(Fraction(float(got_sum[i])) - self.sum[i]), g * self.abs_sum[i]
                assert np.isfinite(got_sum[i]) and err <= bound, "%s sum[%d]: error %.3e, bound %.3e" % (label, i, err, bound)
                worst = max(worst, float(err / bound)) if bound else worst
                for j in fin:
                    v = float(got_cross[i, j])
                    assert np.isfinite(v), "%s cross[%d][%d] = %r" % (label, i, j, v)
                    err, bound = abs(Fraction(v) - self.cross[i][j]), g * self.abs_cross[i][j]
                    assert err <= bound, "%s cross[%d][%d]: error %.3e, bound %.3e" % (label, i, j, err, bound)
                    worst = max(worst, float(err / bound)) if bound else worst
        else:
            g = np.longdouble(float(gamma(self.K))) * np.longdouble(self.widen)
            es = np.abs(got_sum[fin].astype(np.longdouble) - self.sum[fin])
            bs = g * self.abs_sum[fin]
            assert np.isfinite(got_sum[fin]).all() and (es <= bs).all(), "%s sum: worst error / bound %.3e" % (label, float((es / bs).max()))
            sub = np.ix_(fin, fin)
            ec = np.abs(got_cross[sub].astype(np.longdouble) - self.cross[sub])
            bc = g * self.abs_cross[sub]
            assert np.isfinite(got_cross[sub]).all(), label
            bad = np.argwhere(ec > bc)
            assert len(bad) == 0, "%s cross: %d entries over the bound, first %s: error %.3e, bound %.3e" % (
                label, len(bad), bad[0], float(ec[tuple(bad[0])]), float(bc[tuple(bad[0])]))
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = float(np.nanmax(np.concatenate([(ec / bc).ravel(), (es / bs).ravel(), [0.0]])))
        for i in np.flatnonzero(~self.finite):
            assert _same_class(got_sum[i], self.ieee_sum[i]), "%s sum[%d] = %r, IEEE %r" % (label, i, got_sum[i], self.ieee_sum[i])
            for j in range(self.m):
                for a, b in ((i, j), (j, i)):
                    assert _same_class(got_cross[a, b], self.ieee_cross[a, b]), "%s cross[%d][%d] = %r, IEEE %r" % (
                        label, a, b, got_cross[a, b], self.ieee_cross[a, b])
        return worst

    def covariance(self):
        """(cov, tolerance) of the pooled draws from the exact sums, as fractions: (cross - s s^T / K) / (K - 1) and the bound of the
        sums carried through that formula, 4 gamma_K (sum|y_i y_j| + sum|y_i| sum|y_j| / K) / (K - 1)"""
        assert self.exact and self.finite.all() and self.K >= 2
        K, g = self.K, gamma(self.K)
        cov = [[(self.cross[i][j] - self.sum[i] * self.sum[j] / K) / (K - 1) for j in range(self.m)] for i in range(self.m)]
        tol = [[4 * g * (self.abs_cross[i][j] + self.abs_sum[i] * self.abs_sum[j] / K) / (K - 1) for j in range(self.m)] for i in range(self.m)]
        return cov, tol


def _same_class(got, want):
    if np.isnan(want):
        return bool(np.isnan(got))
    return bool(np.isinf(got)) and bool(np.isinf(want)) and (got > 0) == (want > 0)
