"""Pointwise log-likelihood without a GPU (mhx.trace.trace_pointwise, MHX_POINTWISE, mhx.pointwise_table / waic_from_table /
dic_from_table / merge_pointwise): the emitted text, the recorded program against the plain callable, the host
restatement (tests/pointwise_ref.py) against the recorded program, what is refused, the host merge rule of (max, sumexp), the WAIC and
DIC arithmetic from raw sums against scipy and numpy, the closed form of a Normal mean model, and the two entry points' guards.

The raw sums are made here by `_raw_sums`, numpy float64 from a matrix l [nrows][T]: what the device returns, by the definitions of
include/mhx.h.  Tolerances: 1e-12 relative to max(1, |value|) for float64 sums of a few hundred terms of order one (their rounding
is ~1e-14); the closed form at six standard errors, which the test derives from its own draws."""
import ctypes as C
import math
import os

import numpy as np
import pytest
from scipy.special import logsumexp

import mhx.trace as T
import pointwise_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)


def normal_ll(t, y):
    """the README's line: log Normal(y | mu, sigma)"""
    return -0.5 * ((y - t.mu) / t.sigma) ** 2 - T.log(t.sigma) - LOG_SQRT_2PI


def regression_ll(t, r):
    """rows (x, y, w): a weighted straight-line fit with unit scale"""
    return -0.5 * r[2] * (r[1] - (t[0] + t[1] * r[0])) ** 2


def _raw_sums(mhx, l, shift=None):
    """the PointwiseSums of l [nrows][T] by the definitions, in numpy float64"""
    l = np.asarray(l, dtype=np.float64)
    nrows, T_ = l.shape
    fin = np.isfinite(l)
    sh = np.where(fin[:, 0], l[:, 0], 0.0) if shift is None else np.asarray(shift, dtype=np.float64)
    mx, se, s1, s2 = np.empty(nrows), np.empty(nrows), np.empty(nrows), np.empty(nrows)
    for i in range(nrows):
        lf = l[i][fin[i]]
        y = lf - sh[i]
        s1[i], s2[i] = y.sum(), (y * y).sum()
        if np.any(np.isnan(l[i]) | (l[i] == np.inf)):
            mx[i] = se[i] = np.nan
        elif lf.size == 0:
            mx[i], se[i] = -np.inf, 0.0
        else:
            mx[i] = lf.max()
            se[i] = np.exp(lf - mx[i]).sum()
    return mhx.PointwiseSums(max=mx, sumexp=se, s1=s1, s2=s2, bad=(~fin).sum(axis=1).astype(np.float64), shift=sh, T=T_)


def test_emitted_text_of_the_readme_line():
    tp = T.trace_pointwise(normal_ll, 2, [0.5, 1.5, -2.0], names=["mu", "sigma"])
    assert tp.dim == 2 and tp.rows.shape == (3, 1) and tp.data is None and not tp.lp
    want = """MHX_POINTWISE(x, r, m, d, data, ndata)
{
    const mhx_real t1 = x[0];
    const mhx_real t2 = x[1];
    const mhx_real t3 = r[0];
    const mhx_real t4 = t3 - t1;
    const mhx_real t5 = t4 / t2;
    const mhx_real t6 = t5 * t5;
    const mhx_real t8 = MHX_R(-0x1.0000000000000p-1) * t6;
    const mhx_real t9 = mhx_log(t2);
    const mhx_real t10 = t8 - t9;
    const mhx_real t12 = t10 - MHX_R(%s);
    return t12;
}
""" % LOG_SQRT_2PI.hex()
    head, _, body = tp.source.partition("\n")
    assert head.startswith("// traced by mhx.trace") and "7 operations" in head and "rows of 1 reals" in head
    assert body == want
    # a 2-D row is a vector of leaves r[j]; a row entry that is not named is not read; no loop is emitted
    tr = T.trace_pointwise(regression_ll, 2, np.ones((4, 3)))
    assert all(("r[%d]" % j) in tr.source for j in range(3)) and "for (" not in tr.source and "data[" not in tr.source
    t1 = T.trace_pointwise(lambda t, r: t[4] + r[1], 5, np.ones((2, 3)))
    assert "x[4]" in t1.source and "x[0]" not in t1.source and "r[1]" in t1.source and "r[0]" not in t1.source
    # the draw's lp and a constant function
    tl = T.trace_pointwise(lambda t, y, lp: lp - y, 2, [1.0], lp=True)
    assert tl.lp and "x[2]" in tl.source
    assert "return MHX_R(0x1.8000000000000p+0);" in T.trace_pointwise(lambda t, y: 1.5, 1, [1.0]).source


def test_evaluate_equals_the_callable_on_floats():
    rng = np.random.default_rng(5)
    ys = rng.normal(size=7)
    tp = T.trace_pointwise(normal_ll, 2, ys, names=["mu", "sigma"])
    tr = T.trace_pointwise(regression_ll, 2, rng.normal(size=(6, 3)))
    for _ in range(20):
        mu, sigma = rng.normal(), rng.uniform(0.5, 2.0)
        for y in ys:
            want = float(normal_ll(T.NamedVec([mu, sigma], ["mu", "sigma"]), y))
            assert tp.evaluate([mu, sigma], y) == pytest.approx(want, rel=1e-14, abs=1e-14)
        row = rng.normal(size=3)
        assert tr.evaluate([mu, sigma], row) == float(regression_ll(T.Vec([mu, sigma]), T.Vec(list(row))))
    with pytest.raises(T.TraceError, match="row of 2 entries"):
        tr.evaluate([0.0, 1.0], [1.0, 2.0])


def test_refusals_of_the_tracer(mhx):
    with pytest.raises(T.TraceError, match="not a predictive trace"):
        T.trace_pointwise(lambda t, y: T.draw(mhx.Normal(t[0], 1.0)) + y, 1, [1.0])
    for bad in (lambda t, y: [y, y], lambda t, y: None, lambda t, y: y > 0):
        with pytest.raises(T.TraceError, match="one number"):
            T.trace_pointwise(bad, 1, [1.0])
    with pytest.raises(T.TraceError, match="one number"):
        T.trace_pointwise(lambda t, r: r, 1, np.ones((2, 2)))                   # the row itself: a vector of two
    with pytest.raises(T.TraceError, match="sum_over inside sum_over"):
        T.trace_pointwise(lambda t, y: T.sum_over([1.0, 2.0], lambda v: v * y), 1, [1.0])
    with pytest.raises(T.TraceError, match="non-empty"):
        T.trace_pointwise(lambda t, y: y, 1, [])
    with pytest.raises(T.TraceError, match="non-empty"):
        T.trace_pointwise(lambda t, y: y, 1, np.ones((2, 2, 2)))
    with pytest.raises(T.TraceError, match="names"):
        T.trace_pointwise(lambda t, y: y, 2, [1.0], names=["a"])
    with pytest.raises(T.TraceError, match="dim"):
        T.trace_pointwise(lambda t, y: y, 0, [1.0])
    # a later sum_over is not left refused by a pointwise trace that failed half way
    assert T.sum_over([1.0, 2.0], lambda v: v) == 3.0
    with pytest.raises(mhx.ArgumentError, match="non-empty"):
        mhx.HipPointwise("MHX_POINTWISE(x, r, m, d, data, ndata) { return r[0]; }", [])


def test_host_restatement_equals_the_recorded_program(oracle, real):
    """tests/pointwise_ref.py compiles the emitted text for the host: without log / exp, on dyadic inputs, it equals evaluate exactly
    in both widths; with the README's log within the engine-against-libm bound of tests/test_derived_cpu.py"""
    rng = np.random.default_rng(9)
    x = (rng.integers(-8, 8, size=(3, 3, 5)) / 4.0).astype(np.float64)          # [N][d + 1][C], d = 2; every product below is exact in fp32
    rows = (rng.integers(-4, 4, size=(4, 3)) / 2.0).astype(np.float64)
    tr = T.trace_pointwise(regression_ll, 2, rows)
    l = P.host_matrix(oracle, tr.source)(x, rows)
    assert l.shape == (4, 15)
    for i in range(4):
        for t in range(3):
            for c in range(5):
                assert l[i, t * 5 + c] == tr.evaluate(x[t, :2, c], rows[i])
    x[:, 1, :] = np.abs(x[:, 1, :]) + 0.5
    tp = T.trace_pointwise(normal_ll, 2, rows[:, 0], names=["mu", "sigma"])
    l = P.host_matrix(oracle, tp.source)(x, rows[:, 0])
    tol = {"f64": 1e-12, "f32": 2e-5}[real]
    for i in range(4):
        want = np.array([tp.evaluate(x[t, :2, c], rows[i, 0]) for t in range(3) for c in range(5)])
        assert np.all(np.abs(l[i] - want) <= tol * np.maximum(1.0, np.abs(want)))


def test_merge_rule_of_max_and_sumexp(mhx):
    rng = np.random.default_rng(2)
    l = rng.normal(size=(6, 40)) * 5.0
    l[1, :20] = -np.inf                  # a member whose every l is -inf
    l[2, :] = -np.inf                    # both members all -inf
    l[3, 5], l[3, 30] = 7.25, 7.25       # equal maxima, one in each member
    l[3] = np.minimum(l[3], 7.25)
    l[4, 3] = -np.inf                    # a -inf among finite ones
    l[5, 25] = np.nan                    # a NaN in the second member
    sh = np.where(np.isfinite(l[:, 0]), l[:, 0], 0.0)
    a, b, whole = _raw_sums(mhx, l[:, :20], sh), _raw_sums(mhx, l[:, 20:], sh), _raw_sums(mhx, l, sh)
    for m in (mhx.merge_pointwise(a, b), mhx.merge_pointwise(b, a)):
        assert P.same_bits(m["max"], whole["max"]) and np.array_equal(m["bad"], whole["bad"]) and m["T"] == 40
        assert np.isnan(m["sumexp"][5]) and np.isnan(m["max"][5])
        assert m["max"][2] == -np.inf and m["sumexp"][2] == 0.0 and m["max"][1] == whole["max"][1]
        ok = ~np.isnan(whole["sumexp"])
        assert np.allclose(m["sumexp"][ok], whole["sumexp"][ok], rtol=1e-13, atol=0)
        assert np.allclose(m["s1"], whole["s1"], rtol=1e-12, atol=1e-12) and np.allclose(m["s2"], whole["s2"], rtol=1e-12)
        with np.errstate(divide="ignore"):
            lse = m["max"] + np.log(m["sumexp"])
        for i in (0, 1, 3, 4):
            assert lse[i] == pytest.approx(logsumexp(l[i]), rel=1e-13)
    m = mhx.merge_pointwise(a, b)
    assert m["sumexp"][3] == a["sumexp"][3] + b["sumexp"][3]                    # equal maxima: the sums add, no exp
    assert b["max"][1] == whole["max"][1] and m["sumexp"][1] == b["sumexp"][1]  # a -inf member leaves the other's bits
    c = _raw_sums(mhx, l[:, 20:], sh + 1.0)
    with pytest.raises(mhx.ArgumentError, match="different shifts"):
        mhx.merge_pointwise(a, c)


def test_waic_and_dic_arithmetic_from_planted_sums(mhx):
    rng = np.random.default_rng(4)
    T_, ys = 300, rng.normal(1.0, 2.0, size=9)
    mu, sigma = rng.normal(1.0, 0.3, size=T_), np.exp(rng.normal(0.7, 0.1, size=T_))
    l = -0.5 * ((ys[:, None] - mu[None, :]) / sigma[None, :]) ** 2 - np.log(sigma)[None, :] - LOG_SQRT_2PI
    l[4, 17] = -np.inf                                   # a draw of zero likelihood stays in lppd's divisor, and out of mean and var
    tab = mhx.pointwise_table(_raw_sums(mhx, l))
    lppd = logsumexp(l, axis=1) - math.log(T_)
    fin = np.isfinite(l)
    mean = np.array([l[i][fin[i]].mean() for i in range(9)])
    var = np.array([l[i][fin[i]].var(ddof=1) for i in range(9)])
    close = lambda a, b: np.all(np.abs(a - b) <= 1e-12 * np.maximum(1.0, np.abs(b)))        # noqa: E731
    assert close(tab["lppd"], lppd) and close(tab["mean"], mean) and close(tab["var"], var)
    assert np.array_equal(tab["p_waic"], tab["var"]) and close(tab["elpd"], lppd - var)
    assert np.array_equal(tab["bad"], (~fin).sum(axis=1)) and tab["bad"][4] == 1 and tab["T"] == T_
    assert "lppd" in str(tab) and len(str(tab).split("\n")) == 2 + 9
    w = mhx.waic_from_table(tab)
    elpd = lppd - var
    assert w["elpd_waic"] == pytest.approx(elpd.sum(), rel=1e-12) and w["p_waic"] == pytest.approx(var.sum(), rel=1e-12)
    assert w["waic"] == -2.0 * w["elpd_waic"] and w["se"] == pytest.approx(2.0 * math.sqrt(9 * elpd.var(ddof=1)), rel=1e-12)
    assert w["n_high_variance"] == int((var > 0.4).sum()) and w["pointwise"] is tab and "WAIC" in str(w)
    # DIC: the mean deviance from the same sums, the deviance at the posterior mean by the trace's evaluate
    tp = T.trace_pointwise(normal_ll, 2, ys, names=["mu", "sigma"])
    theta_bar = np.array([mu.mean(), sigma.mean()])
    d = mhx.dic_from_table(tab, tp, theta_bar, tp.rows)
    d_bar = -2.0 * mean.sum()
    d_hat = -2.0 * float(np.sum(-0.5 * ((ys - theta_bar[0]) / theta_bar[1]) ** 2 - math.log(theta_bar[1]) - LOG_SQRT_2PI))
    assert d["d_bar"] == pytest.approx(d_bar, rel=1e-12) and d["d_hat"] == pytest.approx(d_hat, rel=1e-12)
    assert d["p_d"] == pytest.approx(d_bar - d_hat, rel=1e-10) and d["dic"] == pytest.approx(2 * d_bar - d_hat, rel=1e-12) and "DIC" in str(d)
    # rows with too few finite draws have no variance; a NaN draw leaves the row without an lppd
    l2 = np.full((2, 5), -np.inf)
    l2[0, 2] = -1.0
    l2[1, 1] = np.nan
    t2 = mhx.pointwise_table(_raw_sums(mhx, l2))
    assert t2["lppd"][0] == pytest.approx(-1.0 - math.log(5)) and np.isnan(t2["var"][0]) and t2["mean"][0] == -1.0
    assert np.isnan(t2["lppd"][1]) and np.isnan(t2["mean"][1]) and t2["bad"][1] == 5


def test_closed_form_of_a_normal_mean_model(mhx):
    """l_i(mu) = -(y_i - mu)^2 / 2, mu ~ N(m, s^2): lppd_i -> -log(1 + s^2) / 2 - (y_i - m)^2 / (2 (1 + s^2)) and
    var l_i -> s^4 / 2 + s^2 (y_i - m)^2.  Over T = 10^6 draws each estimate lies within six standard errors: of log(mean p) the delta
    method's sd(p) / (mean(p) sqrt(T)); of the sample variance sqrt((m4 - var^2) / T), m4 the fourth central moment -- both from the
    draws themselves."""
    rng = np.random.default_rng(7)
    T_, m, s = 10 ** 6, 0.3, 0.8
    ys = np.array([-1.5, 0.0, 0.3, 2.0])
    mu = rng.normal(m, s, size=T_)
    l = -0.5 * (ys[:, None] - mu[None, :]) ** 2
    tab = mhx.pointwise_table(_raw_sums(mhx, l))
    lppd = -0.5 * math.log(1 + s * s) - (ys - m) ** 2 / (2 * (1 + s * s))
    var = 0.5 * s ** 4 + s * s * (ys - m) ** 2
    p = np.exp(l)
    se_lppd = p.std(axis=1) / (p.mean(axis=1) * math.sqrt(T_))
    c = l - l.mean(axis=1, keepdims=True)
    se_var = np.sqrt(((c ** 4).mean(axis=1) - (c ** 2).mean(axis=1) ** 2) / T_)
    assert np.all(np.abs(tab["lppd"] - lppd) <= 6 * se_lppd), (tab["lppd"] - lppd, se_lppd)
    assert np.all(np.abs(tab["var"] - var) <= 6 * se_var), (tab["var"] - var, se_var)
    assert np.all(se_lppd < 2e-3) and np.all(se_var < 1e-2)                      # (the check is not vacuous)


def test_reference_sums_agree_with_scipy(mhx):
    """tests/pointwise_ref.py's longdouble sums and bounds on a small matrix: they are what the device is held to"""
    rng = np.random.default_rng(12)
    l = rng.normal(size=(5, 63)) * 30.0
    l[1, 0] = -np.inf
    l[2, 7] = np.inf
    l[3, :] = -np.inf
    ref = P.sums(l, 9, 7)
    raw = _raw_sums(mhx, l)
    assert P.same_bits(ref["max"], raw["max"]) and np.array_equal(ref["bad"], raw["bad"]) and np.array_equal(ref["shift"], raw["shift"])
    assert ref["shift"][1] == 0.0 and ref["max"][3] == -np.inf and ref["sumexp"][3] == 0 and np.isnan(ref["max"][2])
    for k in ("sumexp", "s1", "s2"):
        ok, ratio = P.within(raw[k], ref[k], ref["e_" + k])
        assert ok and ratio < 1.0, (k, ratio)                                   # numpy's pairwise float64 sums sit inside the bound
    tab, rt = mhx.pointwise_table(raw), P.table(ref)
    for k in ("lppd", "var", "elpd"):
        assert P.within(tab[k], rt[k], rt["e_" + k])[0], k
    assert P.chain_length(9, 257) == 9 + 9 + 2 * 64
    assert not P.within(np.array([1.0 + 1e-9]), np.array([1.0], dtype=P.LD), np.array([1e-12], dtype=P.LD))[0]
    assert not P.within(np.array([np.nan]), np.array([1.0], dtype=P.LD), np.array([1.0], dtype=P.LD))[0]


def test_entry_points_are_declared_exported_and_guarded(mhx):
    import importlib.util
    hdr = open(os.path.join(ROOT, "include", "mhx.h")).read()
    for name in ("mhx_run_pointwise", "mhx_ctx_pointwise"):
        assert name in mhx.EXPORTS and hasattr(mhx.lib(), name) and ("int %s(" % name) in hdr
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
        assert name not in open(os.path.join(ROOT, "advancedmh.jl_amd", "julia", "AdvancedMHHIP.jl")).read()
    lib = C.CDLL(mhx.LIB_PATH)
    lib.mhx_last_error.restype = C.c_char_p
    z = [None, None, None, C.c_int64(0), C.c_int32(0), None, C.c_size_t(0), C.c_int32(0), None, None, None]
    assert lib.mhx_run_pointwise(*z) == mhx.MHX_EINVAL and lib.mhx_last_error().decode() == "mhx_run_pointwise: handle is NULL"
    z = [None, None, C.c_int64(0), C.c_int32(0), C.c_int64(0), None] + z[2:]
    assert lib.mhx_ctx_pointwise(*z) == mhx.MHX_EINVAL and lib.mhx_last_error().decode() == "mhx_ctx_pointwise: handle is NULL"
    spec = importlib.util.spec_from_file_location("embed_headers", os.path.join(ROOT, "advancedmh.jl_amd", "csrc", "embed_headers.py"))
    eh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(eh)
    assert "mhx_pointwise_kernels.h" in eh.HEADERS
    math_h = open(os.path.join(ROOT, "advancedmh.jl_amd", "csrc", "mhx_device_math.h")).read()
    assert "#define MHX_POINTWISE(x, r, m, d, data, ndata)" in math_h
