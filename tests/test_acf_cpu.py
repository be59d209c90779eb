"""The extended-precision reference of the autocovariance sums (tests/acf_ref.py) and the host side of the feature
(mhx.autocorrelation, mhx.integrated_time), without a GPU: (a) the reference against plain numpy, (b) the AR(1) known answer,
(c) the window-margin condition that decides which rows the GPU test compares on tau / window."""
import math

import numpy as np
import pytest

import acf_ref as A
import diag_ref as R

WIDTHS = ("f64", "f32")
CENTRED = (0, 1, 2, 9)              # ar0@0*1, ar0.5@0*1, ar0.9@0*1, mh


def _np_acf(x, lags):
    """per-chain np.correlate in float64: (sum_c A_c(k), sum_c A_c(k) / A_c(0) over the chains with variance, their number)"""
    x = np.asarray(x, dtype=np.float64)
    N, C = x.shape
    un, nm, nv = np.zeros(len(lags)), np.zeros(len(lags)), 0
    for c in range(C):
        e = x[:, c] - x[:, c].mean()
        full = np.correlate(e, e, mode="full")[N - 1:]
        un += full[lags]
        if full[0] > 0 and not np.all(x[:, c] == x[0, c]):
            nm += full[lags] / full[0]
            nv += 1
    return un, nm, nv


# ---- (a) the reference against plain numpy -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 3, 1), (97, 65, 2), (401, 3, 7)])
def test_reference_against_numpy(shape):
    import mhx
    N, C, seed = shape
    lags = np.arange(N)
    x, st = A.reference(N, C, "f64", seed, lags, rows=(0, 1, 2, 9, R.R_CONST, R.R_CONST_PC, R.R_NAN))
    for r in (0, 1, 2, 9):
        un, nm, nv = _np_acf(x[:, r, :], lags)
        s = st[r]
        scale = float(s["acov"][0])
        assert np.allclose(s["acov"].astype(np.float64), un, rtol=1e-10, atol=1e-10 * scale), r
        assert np.allclose(s["nacov"].astype(np.float64), nm, rtol=1e-10, atol=1e-10 * nv), r
        assert s["nvalid"] == nv and (nv == C or r == 9)    # a short Metropolis chain may never have moved
        for mode, a in (("un", s["acov"]), ("nm", s["nacov"])):
            w = s[mode]
            rho = mhx.autocorrelation(a.astype(np.float64))
            assert rho[0] == 1.0 and np.allclose(rho, w["rho"].astype(np.float64), rtol=1e-10, atol=1e-12)
            tau, M, trunc = mhx.integrated_time(w["rho"].astype(np.float64))
            if w["margin"] > 1:
                assert (M, trunc) == (w["window"], w["truncated"]) and math.isclose(tau, float(w["tau"]), rel_tol=1e-10)
    # a sub-range and a sparse lag list
    sub = A.acf_stats(x[:, 1, :], "f64", [0, 3, N - 1], chains=(1, 2))
    un, nm, nv = _np_acf(x[:, 1, 1:3], [0, 3, N - 1])
    assert np.allclose(sub["acov"].astype(np.float64), un, rtol=1e-10, atol=1e-10 * un[0]) and sub["nvalid"] == 2 and "un" not in sub
    # rows without variance, and a row that holds a NaN
    for r in (R.R_CONST, R.R_CONST_PC):
        assert st[r]["nvalid"] == 0 and not st[r]["acov"].any() and not st[r]["nacov"].any()
        assert np.isnan(mhx.autocorrelation(st[r]["acov"].astype(np.float64))).all() and st[r]["un"]["truncated"]
    assert st[R.R_NAN]["nvalid"] == 0 and np.isnan(st[R.R_NAN]["acov"].astype(np.float64)).all()


def test_host_functions():
    import mhx
    rho = np.array([1.0, 0.5, 0.25, 0.125, 0.0625, 0.0, 0.0, 0.0])
    taus = 2 * np.cumsum(rho) - 1
    tau, M, trunc = mhx.integrated_time(rho, c=1.0)
    assert (M, trunc) == (int(np.flatnonzero(np.arange(8) >= taus)[0]), False) and tau == taus[M] and M == 3
    tau, M, trunc = mhx.integrated_time(rho, c=5.0)                       # 5 taus > 7 everywhere: no window within K = 7
    assert (M, trunc) == (7, True) and tau == taus[7]
    assert mhx.integrated_time([1.0])[1:] == (0, True)
    tau, M, trunc = mhx.integrated_time([1.0, np.nan, 0.0])
    assert np.isnan(tau) and (M, trunc) == (2, True)
    a = np.array([[4.0, 2.0, -1.0], [0.0, 0.0, 0.0], [np.nan, np.nan, np.nan], [-1.0, 1.0, 1.0]])
    rho = mhx.autocorrelation(a)
    assert np.array_equal(rho[0], [1.0, 0.5, -0.25]) and np.isnan(rho[1:]).all()
    with pytest.raises(mhx.ArgumentError, match="integrated_time"):
        mhx.integrated_time([])
    bare = mhx.Chains(np.zeros((5, 2, 3), dtype=np.float32), ["a", "lp"], 1, 1)
    for call, what in ((lambda: bare.autocor(), "autocor"), (lambda: bare.autocorr_time(), "autocorr_time")):
        with pytest.raises(mhx.ArgumentError, match="%s needs the live run" % what):
            call()
    text = str(mhx.AutocorTable(parameters=["mu"], lags=[1, 5], autocor=np.array([[0.5, 0.25]])))
    assert text.split("\n")[0] == "Autocorrelation" and "lag 5" in text and "0.2500" in text


# ---- (b) the AR(1) known answer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi,K", [(0.0, 16), (0.5, 40), (0.9, 160)])
def test_ar1_known_answer(phi, K):
    """rho(k) -> phi^k and tau -> (1 + phi) / (1 - phi) at C N = 1 024 000.  Tolerances: four standard deviations of the estimators
    -- Bartlett's var(rho_k) <= (1 + phi^2) / ((1 - phi^2) n) for an AR(1), Sokal's var(tau) = 2 (2M + 1) tau^2 / n for the window M
    -- plus what the estimator is off by construction: the tail 2 phi^(M+1) / (1 - phi) the window cuts, and the bias of centring
    every chain about its own mean, tau / N per lag, (2M + 1) tau / N in tau."""
    import mhx
    C, N = 8, 128000
    n = C * N
    x = R.ar1(np.random.default_rng(int(phi * 10) + 1), N, C, phi)
    st = A.acf_stats(x, "f64", np.arange(K + 1), bounds=False)
    truth = (1 + phi) / (1 - phi)
    for a in (st["acov"], st["nacov"]):
        rho = mhx.autocorrelation(a.astype(np.float64))
        tol = 4 * math.sqrt((1 + phi * phi) / ((1 - phi * phi) * n)) + 2 * truth / N
        assert np.abs(rho - phi ** np.arange(K + 1)).max() <= tol
        tau, M, trunc = mhx.integrated_time(rho)
        assert not trunc and M >= 5 * tau
        tol = 4 * math.sqrt(2 * (2 * M + 1) / n) * truth + 2 * phi ** (M + 1) / (1 - phi) + (2 * M + 1) * truth / N
        assert abs(tau - truth) <= tol, (tau, truth, tol, M)


# ---- (c) which rows are fit for a comparison of tau / window -----------------------------------------------------------------
@pytest.mark.parametrize("mode", ["un", "nm"])
def test_window_margins_admit_enough_rows(mode):
    """The window is a step function of the sums, so the GPU test compares tau / window only where every deciding margin exceeds
    MARGIN (acf_ref.admitted).  What that leaves out may not hide a failure: in fp64 at most 2 of the 100 (case, finite row) pairs;
    in fp32 the four centred rows are in, in at least 8 of the 10 cases (the rows at 1e4 +- 0.01 and -3e5 +- 10 cannot pin a window
    in fp32: half an ulp of their mean is 5 % of their standard deviation)."""
    out64, in32 = [], 0
    for case in R.CASES:
        N, C, seed = case[0], case[1], case[5]
        _, st64 = A.reference(N, C, "f64", seed, np.arange(N))
        _, st32 = A.reference(N, C, "f32", seed, np.arange(N))
        for r in R.FINITE:
            print("ACF_MARGIN %s N%d-C%d row %d (%s): f64 %.3g f32 %.3g" % (mode, N, C, r, R.ROWS[r], st64[r][mode]["margin"], st32[r][mode]["margin"]))
            if not A.admitted(st64[r], mode):
                out64.append((N, C, R.ROWS[r], st64[r][mode]["margin"]))
        in32 += all(A.admitted(st32[r], mode) for r in CENTRED)
    assert len(out64) <= 2, out64
    assert in32 >= 8, in32
