"""PSIS-LOO without a GPU (tests/psis_ref.py, mhx.psis_tail_length / loo_table / loo_from_table / compare, the run-time module's text, the
two entry points' guards).

The reference is what the device is held to, so it is checked here against what is known in closed form: the generalised-Pareto fit's
scale equivariance (exact for a power of two in the grid and the k_j, to rounding in khat), its shrink formula, the shape of genpareto draws at six asymptotic standard errors, and the
leave-one-out predictive density of the conjugate Normal-mean model at six Monte-Carlo standard errors -- both errors derived in the
tests from their own draws."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy import stats

import mhx.trace as T
import pointwise_ref as P
import psis_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "advancedmh.jl_amd", "csrc")
LD = np.longdouble
LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)


def normal_ll(t, y):
    return -0.5 * ((y - t.mu) / t.sigma) ** 2 - T.log(t.sigma) - LOG_SQRT_2PI


def test_gpdfit_is_scale_equivariant_and_shrinks_as_stated():
    """Scale equivariance under a power of two is exact where the definitions make it so -- the grid theta_j and the k_j, asserted bit
    for bit -- and holds to rounding for khat, k, sigma and theta^ (observed: 5.4e-19 in khat at 2^-7, asserted at 1e-15): the profile
    log-likelihoods are not scale free, see below."""
    rng = np.random.default_rng(3)
    x = np.sort(rng.pareto(3.0, size=200)).astype(LD)
    khat, sigma, k, th, fitted, _ = R.gpdfit(x)
    assert fitted and np.isfinite(khat) and sigma > 0
    assert khat == (k * 200 + 5) / (LD(200) + 10)                               # the prior shrink, on the unshrunk k
    assert sigma == -k / th
    # a power of two scales every product exactly: the grid scales and the k_j are the same bits.  The profile log-likelihoods
    # M (log(-theta_j / k_j) - k_j - 1) all move by M p log 2, which ROUNDS (an ulp of |L_j| <= 2^-63 x 200 x 50 each), so the weights, and
    # with them theta^, k and khat, are equivariant to that rounding carried through the softmax (|theta_j - theta^| / |theta^| <= 10 here)
    # and not to the bit: 1e-15 is three orders above it
    th_j, k_j = R.gpd_grid(x)
    for p in (-7, 3, 40):
        s = LD(2) ** p
        th_s, k_s = R.gpd_grid(x * s)
        assert np.array_equal(th_s, th_j / s) and np.array_equal(k_s, k_j)
        k2, s2, kk2, th2, f2, _ = R.gpdfit(x * s)
        assert f2 and abs(float(k2 - khat)) < 1e-15 and abs(float(kk2 - k)) < 1e-15
        assert abs(float(s2 / (sigma * s) - 1)) < 1e-15 and abs(float(th2 * s / th - 1)) < 1e-15
    k3, s3, _, _, _, _ = R.gpdfit(x * LD(3))                                    # any other scale: to rounding
    assert abs(float(k3 - khat)) < 1e-15 and abs(float(s3 / (3 * sigma) - 1)) < 1e-15
    # ties at the quarter point: x* = 0, no fit
    y = x.copy()
    y[:60] = 0
    assert R.gpdfit(y)[4] is False and np.isposinf(R.gpdfit(y)[0]) and np.isnan(R.gpdfit(y)[1])


def test_gpdfit_recovers_the_shape_of_generalised_pareto_draws():
    """the maximum-likelihood shape of n generalised-Pareto draws has asymptotic variance (1 + k)^2 / n (Smith 1987, k > -1/2), and Zhang
    and Stephens' estimator is asymptotically as efficient: the unshrunk k within six such standard errors of 0.3, the shrunk khat as the
    formula moves it"""
    n, k0 = 4000, 0.3
    x = np.sort(stats.genpareto.rvs(k0, scale=2.0, size=n, random_state=np.random.default_rng(11))).astype(LD)
    khat, sigma, k, _, fitted, _ = R.gpdfit(x)
    se = (1 + k0) / math.sqrt(n)
    assert fitted and abs(float(k) - k0) <= 6 * se and se < 0.03
    assert abs(float(khat) - (k0 * n + 5) / (n + 10)) <= 6 * se
    assert abs(float(sigma) / 2.0 - 1) <= 6 * math.sqrt(2 * (1 + k0) / n)      # var(sigma^) / sigma^2 -> 2 (1 + k) / n


def test_conjugate_normal_mean_model_in_closed_form():
    """y_i ~ N(mu, 1), flat prior: mu | y ~ N(ybar, 1 / n), and leaving row i out p(y_i | y_-i) = N(y_i; ybar_-i, 1 + 1 / (n - 1)).  The
    draws are exact posterior draws.  The standard error of a self-normalised importance-sampling estimate p^ = sum w p / sum w with
    normalised weights w~ is sqrt(sum w~^2 (p - p^)^2); of its logarithm, that over p^.  The raw ratios w = 1 / p have finite variance here
    (1 / n < 1 / 2), and smoothing only lowers it."""
    rng = np.random.default_rng(7)
    n, N, nch = 20, 200, 100
    y = rng.normal(0.3, 1.0, size=n)
    mu = rng.normal(y.mean(), 1 / math.sqrt(n), size=N * nch)
    l = -0.5 * (y[:, None] - mu[None, :]) ** 2 - LOG_SQRT_2PI
    ref = R.reference(l, N, nch)
    assert ref["M"] == R.tail_length(N * nch) == 425
    loo_mean = (y.sum() - y) / (n - 1)
    v = 1 + 1 / (n - 1)
    want = -0.5 * (y - loo_mean) ** 2 / v - 0.5 * math.log(2 * math.pi * v)
    w = np.exp(-(l - l.min(axis=1, keepdims=True)))
    wn = w / w.sum(axis=1, keepdims=True)
    p = np.exp(l)
    phat = (wn * p).sum(axis=1)
    se = np.sqrt((wn ** 2 * (p - phat[:, None]) ** 2).sum(axis=1)) / phat
    got = ref["elpd_loo"].astype(np.float64)
    assert np.all(np.abs(got - want) <= 6 * se), (got - want, se)
    assert np.all(se < 0.02) and np.all(ref["khat"] < 0.5)                      # (the check is not vacuous; a light tail)
    # and the bound the device is held to is far below the Monte-Carlo error
    assert np.all(ref["e_elpd_loo"] < 1e-9) and np.all(ref["e_khat"] < 1e-9)


def test_reference_on_ties_non_finite_draws_and_short_chains():
    rng = np.random.default_rng(5)
    l = np.rint(rng.normal(0.0, 6.0, size=(3, 63 * 17)))                        # about 40 levels, thin in the tail
    assert 30 <= np.unique(l).size <= 50
    for q in (1.0, 0.25):                                                       # integer and quarter-integer levels: finite fits
        ref = R.reference(l * q, 17, 63)
        assert ref["M"] == 99 and np.all(ref["n_below"] < 99) and np.all(np.isfinite(ref["khat"])) and np.all(np.isfinite(ref["elpd_loo"]))
        assert np.all(ref["tails"][:, -1] == ref["tau"]) and np.all(ref["tails"][:, 0] == ref["lmin"])
    l[1, 5] = -np.inf
    l[2, :] = np.nan
    ref = R.reference(l, 17, 63)
    assert ref["bad"].tolist() == [0.0, 1.0, 63.0 * 17] and np.isnan(ref["elpd_loo"][1:]).all() and np.isfinite(ref["elpd_loo"][0])
    short = R.reference(rng.normal(size=(2, 17)), 17, 1)                        # M < 5: raw weights, the plain harmonic-mean identity
    assert short["M"] == 0 and np.all(np.isposinf(short["khat"])) and np.all(short["n_below"] == 0)
    ll = short["elpd_loo"].astype(np.float64)
    assert ll.shape == (2,) and np.all(np.isfinite(ll))


def test_raw_weights_reduce_to_the_harmonic_mean():
    """with no smoothing elpd_loo_i = log(T / sum_s exp(-l_s)): the formula's sums, regrouped"""
    rng = np.random.default_rng(9)
    l = rng.normal(size=(4, 19)) * 3
    ref = R.reference(l, 19, 1)
    want = math.log(19) - np.log(np.exp(-l).sum(axis=1))
    assert ref["M"] == 0 and np.allclose(ref["elpd_loo"].astype(np.float64), want, rtol=0, atol=1e-13)


def test_tail_length(mhx):
    for T_, reff, want in ((10000, 1.0, 300), (10001, 1.0, 301), (9999, 1.0, 300), (189, 1.0, 37), (24, 1.0, 0), (25, 1.0, 5), (29, 1.0, 5),
                           (10000, 0.25, 600), (10000, 4.0, 150), (1, 1.0, 0), (51400, 1.0, 681), (100, 1.0, 20)):
        assert mhx.psis_tail_length(T_, reff) == R.tail_length(T_, reff) == want, (T_, reff)
    assert mhx.khat_threshold(51400) == min(1 - 1 / math.log10(51400), 0.7) == 0.7 and mhx.khat_threshold(100) == 0.5


def _fake(mhx, seed, n=12, T_=400):
    rng = np.random.default_rng(seed)
    l = rng.normal(-1.0, 0.5, size=(n, T_))
    mx = l.max(axis=1)
    sums = mhx.PointwiseSums(max=mx, sumexp=np.exp(l - mx[:, None]).sum(axis=1), s1=(l - l[:, :1]).sum(axis=1),
                             s2=((l - l[:, :1]) ** 2).sum(axis=1), bad=np.zeros(n), shift=l[:, 0].copy(), T=T_)
    ref = R.reference(l, T_, 1)
    psis = mhx.PsisResult({k: ref[k].astype(np.float64) for k in R.EXACT + R.BOUNDED}, T=T_, M=ref["M"], reff=1.0)
    return l, sums, psis


def test_loo_table_totals_and_compare_against_numpy(mhx):
    l, sums, psis = _fake(mhx, 1)
    tab = mhx.loo_table(psis, sums)
    lppd = np.log(np.exp(l).mean(axis=1))
    assert np.allclose(tab["lppd"], lppd, rtol=0, atol=1e-13) and np.array_equal(tab["elpd_loo"], psis["elpd_loo"])
    assert np.allclose(tab["p_loo"], lppd - psis["elpd_loo"], rtol=0, atol=1e-13) and np.all(tab["p_loo"] > 0)
    assert tab["T"] == 400 and tab["M"] == 60 and "PSIS-LOO" in str(tab)
    loo = mhx.loo_from_table(tab)
    e = tab["elpd_loo"]
    assert loo["elpd_loo"] == float(e.sum()) and loo["looic"] == -2.0 * loo["elpd_loo"] and loo["p_loo"] == float(tab["p_loo"].sum())
    assert loo["se"] == pytest.approx(2.0 * math.sqrt(12 * e.var(ddof=1)), rel=1e-15)     # as waic_from_table forms it
    tab2 = mhx.LooTable(tab, khat=np.array([-np.inf, 0.5, 0.50001, 0.7, 0.71, 1.0, 1.01, np.inf, np.nan, 0.0, 0.6, 2.0]))
    assert mhx.loo_from_table(tab2)["khat_counts"] == [3, 3, 2, 3]
    assert loo["khat_threshold"] == 1 - 1 / math.log10(400) and "(0.7, 1]" in str(loo)
    with pytest.raises(mhx.ArgumentError):
        mhx.loo_table(psis, dict(sums, T=401))
    # compare: best first, differences against the best, the paired standard error; a waic result is accepted
    _, sums_b, psis_b = _fake(mhx, 2)
    psis_b["elpd_loo"] = psis_b["elpd_loo"] - 0.3
    loo_b = mhx.loo_from_table(mhx.loo_table(psis_b, sums_b))
    waic = mhx.waic_from_table(mhx.pointwise_table(sums))
    table = mhx.compare({"b": loo_b, "a": loo, "w": waic})
    assert [r["name"] for r in table][0] in ("a", "w") and table[-1]["name"] == "b" and "elpd_diff" in str(table)
    best = table[0]
    eb = {"a": e, "w": waic["pointwise"]["elpd"]}[best["name"]]
    d = psis_b["elpd_loo"] - eb
    assert best["elpd_diff"] == 0.0 and best["se_diff"] == 0.0
    assert table[-1]["elpd_diff"] == pytest.approx(d.sum(), rel=1e-14) and table[-1]["se_diff"] == pytest.approx(math.sqrt(12 * d.var(ddof=1)), rel=1e-14)
    with pytest.raises(mhx.ArgumentError):
        mhx.compare({"a": loo, "short": mhx.LooTable(elpd_loo=np.zeros(3))})


def test_the_module_compiles_for_gfx950_behind_a_traced_function(tmp_path, real):
    """the text mhx_run_psis hands the run-time compiler, through hipcc here: the three kernels, no scratch memory, LDS within a block's"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the build needs it too"
    tp = T.trace_pointwise(normal_ll, 2, [0.5, 1.5, -2.0], names=["mu", "sigma"])
    inc = open(os.path.join(CSRC, "mhx_api_psis.inc")).read()
    api = open(os.path.join(CSRC, "mhx_api.hip")).read()
    tail = '#define MHX_HAVE_POINTWISE 1\n#include "mhx_pointwise_kernels.h"\n#define MHX_HAVE_PSIS 1\n#include "mhx_psis_kernels.h"\n'
    # what user_module appends for psis_checked: its frames in this order, each as "#define <have> 1\n#include \"<header>\"\n"
    assert '{{"MHX_HAVE_POINTWISE", "mhx_pointwise_kernels.h"}, {"MHX_HAVE_PSIS", "mhx_psis_kernels.h"}}' in inc
    frame = api[api.index("for (const user_frame& f : frames) {"):]
    frame = "".join(re.findall(r's \+= (.*);', frame[:frame.index("}")]))
    assert frame == '"#define "f.have" 1\\n#include \\""f.header"\\"\\n"', frame
    src = tmp_path / "psis.hip"
    src.write_text('#include "mhx_device_math.h"\n#line 1 "pointwise.hip"\n' + tp.source + "\n" + tail)
    out = tmp_path / "k.s"
    cmd = [hipcc, "-x", "hip", "--offload-device-only", "--no-gpu-bundle-output", "-S", "-DMHX_JIT_BUILD=1", "-I" + CSRC, "--offload-arch=gfx950",
           "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-DMHX_REAL64=%d" % (1 if real == "f64" else 0), "-DMHX_XW_LINE=64",
           "-DMHX_JIT_PSIS_ROWS=8", "-o", str(out), str(src)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-2000:]
    text = out.read_text()
    meta = re.findall(r"\.group_segment_fixed_size:\s*(\d+)|\.name:\s*(\w+)\s|\.private_segment_fixed_size:\s*(\d+)", text)
    names = [b for _, b, _ in meta if b]
    for k in ("mhx_jit_psis_hist", "mhx_jit_psis_gather", "mhx_jit_psis_fit", "mhx_jit_pointwise"):
        assert k in names, names
    assert max(int(c) for _, _, c in meta if c) == 0                            # no scratch
    assert max(int(a) for a, _, _ in meta if a) == 8 << 11 << 2                 # the histogram of 8 rows: 64 KiB, a block's limit


def test_entry_points_are_declared_exported_and_guarded(mhx):
    import importlib.util
    hdr = open(os.path.join(ROOT, "include", "mhx.h")).read()
    for name in ("mhx_run_psis", "mhx_ctx_psis"):
        assert name in mhx.EXPORTS and hasattr(mhx.lib(), name) and ("int %s(" % name) in hdr
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
        assert name not in open(os.path.join(ROOT, "advancedmh.jl_amd", "julia", "AdvancedMHHIP.jl")).read()
    assert not hasattr(mhx.Group, "psis")                                        # left out on purpose
    for name in ("psis", ):
        assert hasattr(mhx.Run, name)
    assert hasattr(mhx.Chains, "loo")
    lib = C.CDLL(mhx.LIB_PATH)
    lib.mhx_last_error.restype = C.c_char_p
    z = [None, None, None, C.c_int64(0), C.c_int32(0), None, C.c_size_t(0), C.c_double(1.0), None, None, None, None]
    assert lib.mhx_run_psis(*z) == mhx.MHX_EINVAL and lib.mhx_last_error().decode() == "mhx_run_psis: handle is NULL"
    z = [None, None, C.c_int64(0), C.c_int32(0), C.c_int64(0), None] + z[2:]
    assert lib.mhx_ctx_psis(*z) == mhx.MHX_EINVAL and lib.mhx_last_error().decode() == "mhx_ctx_psis: handle is NULL"
    spec = importlib.util.spec_from_file_location("embed_headers", os.path.join(CSRC, "embed_headers.py"))
    eh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(eh)
    assert "mhx_psis_kernels.h" in eh.HEADERS
    inc = open(os.path.join(CSRC, "mhx_api_psis.inc")).read()
    assert "row_blocks_checked(v, nrows, rowlen, data, ndata)" in inc            # the refusals of the rows and the data block: mhx_api.hip
    inc += open(os.path.join(CSRC, "mhx_api.hip")).read()
    for guard in ("NULL argument", "at least one row of at least one real", "rows are indexed in 31 bits", "reff = %g is not a positive finite number",
                  "PSIS_SCRATCH_MB"):
        assert guard in inc, guard
    math_h = open(os.path.join(CSRC, "mhx_device_math.h")).read()
    assert math_h.index("mhx_log_f64(double x)") < math_h.index("#if MHX_REAL64\n// ----")   # in front of the width sections
