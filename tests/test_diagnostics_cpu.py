"""The extended-precision reference of the diagnostics (tests/diag_ref.py) against what is known without it: the integrated
autocorrelation time of AR(1), the numpy restatements tests/test_gpu_misc.py holds the device to, the lag / split / subset rules
of include/mhx.h, tied ranks -- and the truncation margin of every crafted input tests/test_gpu_diagnostics.py plants."""
import math

import numpy as np
import pytest

import diag_ref as R


# ---- known answer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_tau_of_ar1_is_the_known_integrated_autocorrelation_time(phi):
    """tau = (1 + phi) / (1 - phi).  The width of the assertion comes from the estimator, not from its output: a windowed sum of
    sample autocorrelations over K lags of n = C N draws has variance 2 (2K + 1) tau^2 / n (Sokal 1997, eq. 3.19; K: the lag the
    reference truncated at), and cutting the sum at K leaves out 2 phi^(K+1) / (1 - phi).  Four standard deviations + that bias."""
    C, N = 256, 4000
    x = R.ar1(np.random.default_rng(100 + int(10 * phi)), N, C, phi)
    s = R.series_stats(x, "f64", max_lag=400, ess_chains=0, split=False)
    tau = (1 + phi) / (1 - phi)
    K = 2 * len(s["P"])
    assert not s["truncated"] and K < 400
    sd = tau * math.sqrt(2.0 * (2 * K + 1) / (C * N))
    bias = 2 * phi ** (K + 1) / (1 - phi)
    print("phi %g: tau %.4f, reference %.4f, K %d, sd %.4f, bias %.4f" % (phi, tau, float(s["tau"]), K, sd, bias))
    assert abs(float(s["tau"]) - tau) < 4 * sd + bias
    assert abs(float(s["ess"]) - C * N / float(s["tau"])) < 1e-9 * C * N
    assert abs(float(s["rhat"]) - 1) < 0.01


# ---- the numpy restatements of tests/test_gpu_misc.py ----------------------------------------------------------------------------
def _ess_numpy(vv, nlag):
    """test_diagnostics_match_numpy.ess_numpy / test_bulk_and_tail_ess_match_numpy.ess, word for word"""
    Nn, Cc = vv.shape
    mm = vv.mean(axis=0)
    xc = vv - mm
    A = np.array([(xc[:Nn - k] * xc[k:]).sum() for k in range(nlag)]) / (Cc * (Nn - 1.0))
    W = vv.var(axis=0, ddof=1).mean()
    varp = (Nn - 1.0) / Nn * W + mm.var(ddof=1)
    rho = 1.0 - (A[0] - A) / varp
    tau, prev = -1.0, np.inf
    for j in range(nlag // 2):
        pm = rho[2 * j] + rho[2 * j + 1]
        if pm <= 0:
            break
        pm = min(pm, prev)
        prev = pm
        tau += 2 * pm
    return Cc * Nn / tau, np.sqrt(varp / W)


def _metropolis(rng, N, C, d, step, rho=0.0):
    """random-walk Metropolis on a (correlated) unit Gaussian, started in its stationary law: the kind of chain those tests sample"""
    cov = np.array([[1.0, rho], [rho, 1.0]]) if d == 2 else np.eye(d)
    prec, Lc = np.linalg.inv(cov), np.linalg.cholesky(cov)
    x = Lc @ rng.normal(size=(d, C))
    lp = -0.5 * np.einsum("ic,ij,jc->c", x, prec, x)
    out = np.empty((N, d + 1, C))
    for t in range(N):
        y = x + step * rng.normal(size=(d, C))
        lq = -0.5 * np.einsum("ic,ij,jc->c", y, prec, y)
        acc = np.log(rng.random(C)) < lq - lp
        x = np.where(acc, y, x)
        lp = np.where(acc, lq, lp)
        out[t, :d], out[t, d] = x, lp
    return out


def test_reference_agrees_with_the_numpy_restatement_of_the_plain_ess():
    """3 x 300 x 400, max_lag 100 (nlag = 100 there: the restatement sums 50 pairs, max_lag + 1 = 101 rounds down to the same)"""
    v = _metropolis(np.random.default_rng(3), 400, 300, 3, 1.0)
    for p in range(3):
        s = R.series_stats(v[:, p, :], "f64", max_lag=100, ess_chains=0, split=False)
        want, _ = _ess_numpy(v[:, p, :], 100)
        assert abs(float(s["ess"]) - want) / want < 1e-9
        s = R.series_stats(v[:, p, :], "f64", max_lag=100, ess_chains=0, split=True)
        halves = np.concatenate([v[:200, p, :], v[200:, p, :]], axis=1)
        want, rhat = _ess_numpy(halves, 100)
        assert abs(float(s["ess"]) - want) / want < 1e-9 and abs(float(s["rhat"]) - rhat) < 1e-12
        assert s["M"] == 600 and s["n"] == 200


def test_reference_agrees_with_the_numpy_restatement_of_bulk_and_tail_ess():
    from scipy.stats import norm, rankdata
    v = _metropolis(np.random.default_rng(12), 600, 64, 2, math.sqrt(0.6), rho=0.8)
    for p in range(3):
        x = v[:, p, :]
        S = x.size
        ranks = rankdata(x.ravel(), method="average")
        assert np.unique(x).size < S
        z = norm.ppf((ranks - 0.375) / (S + 0.25)).reshape(x.shape)
        srt = np.sort(x.ravel())
        q05, q95 = srt[int(0.05 * (S - 1))], srt[int(0.95 * (S - 1))]
        sp = lambda a: np.concatenate([a[:300], a[300:]], axis=1)
        want_bulk = _ess_numpy(sp(z), 120)[0]
        want_tail = min(_ess_numpy(sp((x <= q05).astype(float)), 120)[0], _ess_numpy(sp((x <= q95).astype(float)), 120)[0])
        got = R.bulk_tail(x, "f64", max_lag=120, ess_chains=0, split=True)
        assert abs(float(got["ess_bulk"]) - want_bulk) / want_bulk < 1e-9
        assert abs(float(got["ess_tail"]) - want_tail) / want_tail < 1e-9


# ---- the rules -------------------------------------------------------------------------------------------------------------------
def test_nlag_rule():
    """min(max_lag + 1, n) rounded down to even; fewer than 2 lags: no ESS"""
    assert [R.nlag_rule(k, 97) for k in (0, 1, 2, 3, 96, 97, 970)] == [0, 2, 2, 4, 96, 96, 96]
    assert [R.nlag_rule(k, 4) for k in (1, 3, 4)] == [2, 4, 4]
    assert R.nlag_rule(1, 2) == 2 and R.nlag_rule(5, 1) == 0
    x = R.ar1(np.random.default_rng(1), 30, 4, 0.5)
    assert np.isnan(float(R.series_stats(x, "f64", max_lag=0)["ess"]))
    a, b = R.series_stats(x, "f64", max_lag=29), R.series_stats(x, "f64", max_lag=300)
    assert a["nlag"] == b["nlag"] == 30 and a["ess"] == b["ess"]


def test_split_halves_drop_the_last_draw_of_an_odd_n():
    x = R.ar1(np.random.default_rng(2), 11, 5, 0.5)
    s = R.series_stats(x, "f64", max_lag=4, split=True)
    assert s["n"] == 5 and s["M"] == 10
    y = x.copy()
    y[10] = 1e6                                                         # the dropped draw is not read
    t = R.series_stats(y, "f64", max_lag=4, split=True)
    assert all(s[k] == t[k] for k in ("sum_m", "sum_m2", "sum_v", "ess", "rhat"))
    # the second halves start at draw 5, not 6
    want = np.concatenate([x[:5], x[5:10]], axis=1)
    u = R.series_stats(want, "f64", max_lag=4, split=False)
    assert all(s[k] == u[k] for k in ("sum_m", "sum_m2", "sum_v", "ess", "rhat"))
    wrong = R.series_stats(np.concatenate([x[:5], x[6:11]], axis=1), "f64", max_lag=4, split=False)
    assert wrong["sum_m"] != s["sum_m"]


def test_ess_chains_subset_takes_autocovariances_of_the_first_chains_and_var_plus_of_all():
    x = R.ar1(np.random.default_rng(3), 60, 7, 0.5)
    full = R.series_stats(x, "f64", max_lag=20)
    for nc in (1, 3, 6):
        s = R.series_stats(x, "f64", max_lag=20, ess_chains=nc)
        sub = R.series_stats(x[:, :nc], "f64", max_lag=20)
        k = min(len(s["A"]), len(sub["A"]))
        assert s["nc"] == nc and np.array_equal(s["A"][:k], sub["A"][:k])
        assert s["varp"] == full["varp"] and s["sum_v"] == full["sum_v"]
    assert R.series_stats(x, "f64", max_lag=20, ess_chains=7)["ess"] == full["ess"]
    assert R.series_stats(x, "f64", max_lag=20, ess_chains=99)["ess"] == full["ess"]
    # split: both halves of each of the first chains
    s = R.series_stats(x, "f64", max_lag=20, ess_chains=2, split=True)
    sub = R.series_stats(np.concatenate([x[:30, :2], x[30:, :2]], axis=1), "f64", max_lag=20)
    assert np.array_equal(s["A"][:2], sub["A"][:2])


def test_single_chain_form_uses_a0_for_var_plus():
    x = R.ar1(np.random.default_rng(4), 200, 1, 0.5)
    s = R.series_stats(x, "f64", max_lag=50)
    A = s["A"]
    rho = A / A[0]
    tau = -1.0
    prev = np.inf
    for j in range(len(A) // 2):
        pm = rho[2 * j] + rho[2 * j + 1]
        if pm <= 0:
            break
        prev = pm = min(pm, prev)
        tau += 2 * pm
    assert abs(float(s["tau"] - tau)) < 1e-15 * abs(float(tau)) and np.isnan(float(s["rhat"]))


def test_ties_get_average_ranks():
    from scipy.stats import rankdata
    rng = np.random.default_rng(5)
    x = rng.integers(0, 9, size=500).astype(np.float64)
    x[::7] = -np.inf
    x[3::11] = np.inf
    assert np.array_equal(R.average_ranks(x), rankdata(x, method="average"))
    assert np.array_equal(R.average_ranks(np.array([2.0, 1.0, 2.0, 2.0])), [3.0, 1.0, 3.0, 3.0])
    z = R.normal_scores(np.array([1.0, 2.5, 2.5, 4.0]), 4)
    assert z[1] == z[2] and abs(float(z[0] + z[3])) < 1e-18 and abs(float(z[1])) < 1e-18
    from scipy.special import ndtri
    assert abs(float(z[3]) - ndtri(3.625 / 4.25)) < 1e-15


def test_rows_without_an_answer():
    x = R.crafted(97, 5, "f64", 1)
    for row in (R.R_CONST, R.R_CONST_PC):
        s = R.series_stats(x[:, row, :], "f64", max_lag=10, split=True)
        assert np.isnan(float(s["ess"])) and s["sum_v"] == 0
        b = R.bulk_tail(x[:, row, :], "f64", max_lag=10)
        assert np.isnan(float(b["ess_tail"])) and (row == R.R_CONST_PC or np.isnan(float(b["ess_bulk"])))
    assert np.isnan(float(R.series_stats(x[:, R.R_CONST, :], "f64", max_lag=10)["rhat"]))
    assert np.isposinf(float(R.series_stats(x[:, R.R_CONST_PC, :], "f64", max_lag=10)["rhat"]))
    for row in (R.R_NAN, R.R_NEG_NAN, R.R_PINF, R.R_NINF):
        s = R.series_stats(x[:, row, :], "f64", max_lag=10)
        assert all(np.isnan(float(s[k])) for k in ("sum_m", "sum_m2", "sum_v", "ess", "rhat"))
        b = R.bulk_tail(x[:, row, :], "f64", max_lag=10)
        fin = row in (R.R_PINF, R.R_NINF)
        assert np.isfinite(float(b["ess_bulk"])) == fin and np.isfinite(float(b["ess_tail"])) == fin


# ---- every crafted input of the GPU tests meets the truncation margin --------------------------------------------------------------
@pytest.mark.parametrize("width", ["f32", "f64"])
@pytest.mark.parametrize("case", R.CASES + [R.LONG_CASE], ids=R.case_id)
def test_crafted_inputs_meet_the_truncation_margin(case, width):
    """every P_m before the truncating pair above MARGIN x its bound, the truncating one below -MARGIN x its bound: the device's
    truncation index is then the reference's, and ESS -- a step function of it -- can be compared at MARGIN x the bound"""
    if case == R.LONG_CASE:
        x, st, bt = R.reference(case, width, bulk=False)
        rows = range(x.shape[1])
    else:
        x, st, bt = R.reference(case, width)
        rows = R.FINITE + [R.R_PINF, R.R_NINF]
    worst = math.inf
    for r in rows:
        if r in st and np.isfinite(float(st[r]["sum_m"])):
            worst = min(worst, st[r]["margin"])
            P, bP = st[r]["P"], st[r].get("b_P", [])
            for j in range(len(P)):
                last = j == len(P) - 1 and not st[r]["truncated"]
                assert (P[j] < -R.MARGIN * bP[j]) if last else (P[j] > R.MARGIN * bP[j]), (r, j, P[j], bP[j])
        if r in bt:
            worst = min(worst, bt[r]["margin"])
            if case != R.LONG_CASE and r in (R.R_PINF, R.R_NINF) and case[0] >= 97:
                assert np.isfinite(float(bt[r]["ess_bulk"])) and np.isfinite(float(bt[r]["ess_tail"]))
    print("%s %s: smallest |P_m| / bound = %.3g" % (R.case_id(case), width, worst))
    assert worst > R.MARGIN
