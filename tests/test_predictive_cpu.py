"""CPU: the tracer of predictive maps (mhx.trace.draw / trace_predictive) and the reference of their draws (tests/predictive_ref.py,
DESIGN.md section 3.16).  No GPU: the emitted source is read as text, the program is run in numpy, and the reference is held to
known answers with derived bounds."""
import re

import numpy as np
import pytest

import family_restatement as FR
import predictive_ref as P
import mhx
import mhx.trace as T


def test_draw_indices_follow_call_order():
    def fn(t):
        a = T.draw(mhx.Normal(t[0], 1.0))                   # 0
        T.draw(mhx.Gamma(2.5, 2.0))                         # 1: never read, still an index
        b = T.draw(mhx.Exponential(abs(a) + 1.0))           # 2: a parameter that is a draw
        return [b, mhx.Laplace(t[1], 2.0), a + b, mhx.TDist(1)]     # 3 and 4: outputs that are distributions, in output order
    p = T.trace_predictive(fn, 2)
    assert isinstance(p, T.TracedMap) and (p.ndraws, p.nout, p.dim) == (5, 4, 2)
    assert [f for f, _ in p.draws] == [FR.NORMAL, FR.GAMMA, FR.EXPONENTIAL, FR.LAPLACE, FR.CAUCHY]
    assert p.draws[0][1] == (None, 1.0) and p.draws[1][1] == (2.5, 2.0) and p.draws[2][1] == (None, 0.0)
    assert p.draws[3][1] == (None, 2.0) and p.draws[4][1] == (0.0, 1.0)
    calls = re.findall(r"rng\.(draw|gamma)\((\d+), (\d+),", p.source)
    assert [(int(k), int(f)) for _, k, f in calls] == [(0, FR.NORMAL), (2, FR.EXPONENTIAL), (3, FR.LAPLACE), (4, FR.CAUCHY)]     # 1 is dead
    assert p.source.index("rng.draw(0,") < p.source.index("rng.draw(2,")                   # a draw before the draw that reads it
    # the shorthand alone is a complete map, and names work as in trace_map
    q = T.trace_predictive(lambda t: mhx.Normal(t.mu, t.sigma), 2, names=["mu", "sigma"])
    assert (q.ndraws, q.nout) == (1, 1) and "rng.draw(0, 0, t1, t2)" in q.source
    assert T.trace_predictive(lambda t, lp: [lp, mhx.Uniform(0.0, 1.0)], 2, lp=True).lp


def test_emitted_source_is_deterministic_and_names_each_row_once():
    def fn(t):
        s = abs(t[1]) + 0.5
        return [mhx.Normal(t[0], s), mhx.Laplace(t[0], s), T.draw(mhx.Cauchy(t[2], s)) * t[0]]
    a, b = T.trace_predictive(fn, 3), T.trace_predictive(fn, 3)
    assert a.source == b.source and a.source.splitlines()[1] == "MHX_PREDICTIVE(x, rng, y, d, data, ndata)"
    for k in range(3):
        assert a.source.count("x[%d]" % k) == 1
    assert a.source.count("y.set(") == 3 and "MHX_DERIVED" not in a.source
    # the deterministic map's text is what it was
    m = T.trace_map(lambda t: t[1] ** 2, 2)
    assert m.source.splitlines()[1] == "MHX_DERIVED(x, y, d, data, ndata)" and "a map of the draws, 1 outputs" in m.source


@pytest.mark.parametrize("alpha", [2.5, 0.5, 0.1, 1.0, 7.3])
def test_gamma_constants_are_the_tables(alpha, real):
    """d, c and 1 / alpha in the source are those of family_restatement.table (what api_rwmh_create_components derives), compared as
    floats of the width: MHX_RW(fp64 literal, fp32 literal), the shape itself MHX_R(alpha)"""
    p = T.trace_predictive(lambda t: [mhx.Gamma(alpha, t[0]), mhx.InverseGamma(alpha, 2.0)], 1)
    R = np.float64 if real == "f64" else np.float32
    calls = re.findall(r"rng\.gamma\((\d+), (\d+), MHX_R\(([^)]+)\), [^,]+, MHX_RW\(([^,]+), ([^)]+)\), MHX_RW\(([^,]+), ([^)]+)\), "
                       r"MHX_RW\(([^,]+), ([^)]+)\)\)", p.source)
    assert [(int(c[0]), int(c[1])) for c in calls] == [(0, FR.GAMMA), (1, FR.INVERSE_GAMMA)]
    for c, fam in zip(calls, (FR.GAMMA, FR.INVERSE_GAMMA)):
        _, row = FR.table([(fam, alpha, 2.0)])[0]
        pick = 0 if real == "f64" else 1
        got = [R(float.fromhex(c[2]))] + [R(float.fromhex(c[3 + 2 * j + pick])) for j in range(3)]
        want = [row[0], row[2], row[3], row[4]]
        assert all(type(w) is R for w in want)
        assert [g.tobytes() for g in got] == [w.tobytes() for w in want], (alpha, got, want)
        if real == "f32":                                   # the fp32 literal is a float: the suffix the macro appends rounds nothing
            assert all(float(R(float.fromhex(c[4 + 2 * j]))) == float.fromhex(c[4 + 2 * j]) for j in range(3))


def test_refusals():
    tp = T.trace_predictive
    with pytest.raises(T.TraceError, match="shape alpha of Gamma must not depend on the state"):
        tp(lambda t: mhx.Gamma(t[0], 1.0), 1)
    with pytest.raises(T.TraceError, match="shape alpha of InverseGamma must not depend on the state"):
        tp(lambda t: T.draw(mhx.InverseGamma(abs(t[0]) + 1.0, 1.0)), 1)

    class TwoParameterExponential:
        family = FR.EXPONENTIAL

        def __init__(self, a, b):
            self.a, self.b = a, b

        def params(self):
            return self.a, self.b
    with pytest.raises(T.TraceError, match="Exponential has one parameter"):
        tp(lambda t: TwoParameterExponential(1.0, t[0]), 1)
    with pytest.raises(T.TraceError, match=r"TDist\(2\)"):
        tp(lambda t: mhx.TDist(2), 1)

    class Beta:
        family = 7

        def params(self):
            return 1.0, 1.0
    with pytest.raises(T.TraceError, match="not one of the device families"):
        tp(lambda t: T.draw(Beta()), 1)
    with pytest.raises(T.TraceError, match="not one of the device families"):
        tp(lambda t: T.draw(3.0), 1)
    with pytest.raises(T.TraceError, match="finite alpha > 0"):
        tp(lambda t: mhx.Gamma(0.0, t[0]), 1)
    with pytest.raises(T.TraceError, match="draw inside sum_over"):
        tp(lambda t: T.sum_over(np.array([1.0, 2.0]), lambda r: T.draw(mhx.Normal(r, 1.0))), 1)
    # outside a predictive trace: no trace at all, and each of the other tracers
    with pytest.raises(T.TraceError, match="no predictive trace"):
        T.draw(mhx.Normal(0.0, 1.0))
    with pytest.raises(T.TraceError, match="not a predictive trace"):
        T.trace(lambda t: T.draw(mhx.Normal(t[0], 1.0)), 1)
    with pytest.raises(T.TraceError, match="not a predictive trace"):
        T.trace_map(lambda t: T.draw(mhx.Normal(t[0], 1.0)), 1)
    with pytest.raises(T.TraceError, match="not a predictive trace"):
        T.trace_proposal(lambda x: mhx.Normal(T.draw(mhx.Normal(x, 1.0)), 1.0), 1)
    with pytest.raises(T.TraceError, match="not a predictive trace"):
        T.trace_composite([("a", 1, lambda x: mhx.Normal(T.draw(mhx.Normal(x, 1.0)), 1.0))])
    # a distribution is an output of a predictive map only
    with pytest.raises(T.TraceError, match="output 0 of the map"):
        T.trace_map(lambda t: mhx.Normal(t[0], 1.0), 1)


def test_more_than_2_to_the_20_draws_are_refused(monkeypatch):
    assert T.MAX_DRAWS == 1 << 20                           # (draw << 8 | attempt fills the 28 bits of a counter word's block)
    monkeypatch.setattr(T, "MAX_DRAWS", 5)                  # the same check, without a million calls
    T.trace_predictive(lambda t: [mhx.Normal(t[0], 1.0)] * 1 + [T.draw(mhx.Uniform(0.0, 1.0)) for _ in range(4)], 1)
    with pytest.raises(T.TraceError, match=r"more than 2\^20 draws"):
        T.trace_predictive(lambda t: [T.draw(mhx.Uniform(0.0, 1.0)) for _ in range(6)], 1)


def test_evaluate_with_a_supplied_draw_function():
    def make(draw, D):
        def fn(t):
            a = draw(D.Normal(t[0], abs(t[1]) + 0.5))
            g = draw(D.Gamma(2.5, abs(a) + 1.0))
            return [a * g - t[1], D.Laplace(g, 2.0), 3.0]
        return fn
    p = T.trace_predictive(make(T.draw, mhx), 2)
    seen = []

    def draw_fn(k, family, params):
        seen.append((k, family, tuple(float(v) for v in params)))
        return 0.25 * (k + 1) + params[0] - params[1]

    x = [1.5, -2.0]
    got = p.evaluate(x, draw_fn)
    # the callable itself on floats, with the same draws supplied in call order
    count = [0]

    def py_draw(dist):
        k, count[0] = count[0], count[0] + 1
        p0, p1 = dist.params()
        return 0.25 * (k + 1) + p0 - p1
    out = make(py_draw, P)(x)
    want = [out[0], py_draw(out[1]), out[2]]
    assert got.dtype == np.float64 and got.tolist() == want
    assert seen == [(0, FR.NORMAL, (1.5, 2.5)), (1, FR.GAMMA, (2.5, 1.75)), (2, FR.LAPLACE, (1.25, 2.0))] and want == [1.0625, 0.0, 3.0]
    # with lp
    q = T.trace_predictive(lambda t, lp: T.draw(mhx.Normal(lp, 1.0)) + t[0], 1, lp=True)
    assert q.evaluate([2.0], lambda k, f, pr: pr[0] * 10.0, lp=-3.0).tolist() == [-28.0]


N_CHAINS, N_DRAWS, KA_SEED = 64, 512, 20260519


def _pooled(dist):
    """the draws of `dist` (constant parameters) as predictive draw 0 of a 64 x 512 tensor, fp64"""
    return np.array([[float(P.one_draw(dist, KA_SEED, c, t, 0)) for c in range(N_CHAINS)] for t in range(N_DRAWS)])


def test_known_answers_for_the_reference(oracle):
    """The reference itself, on a constant tensor (mu = 1, sigma = 2): 64 chains x 512 draws = 32768 independent draws, seed fixed.
    Each bound is six standard errors of the statistic under the distribution claimed: 6 sd / sqrt(n) for a mean, and
    6 sd^2 sqrt(2 / n) for the variance of a Normal (its sampling variance is 2 sigma^4 / (n - 1))."""
    old = oracle.get_dtype()
    oracle.set_dtype("f64")
    try:
        n = N_CHAINS * N_DRAWS
        y = _pooled(P.Normal(1.0, 2.0))
        assert np.isfinite(y).all() and len(np.unique(y)) == n
        assert abs(y.mean() - 1.0) <= 6 * 2 / np.sqrt(n), y.mean()
        assert abs(y.var() - 4.0) <= 6 * 4 * np.sqrt(2.0 / n), y.var()
        g = _pooled(P.Gamma(2.5, 2.0))                      # mean alpha theta = 5, sd sqrt(alpha) theta
        assert (g > 0).all() and abs(g.mean() - 5.0) <= 6 * np.sqrt(2.5) * 2 / np.sqrt(n), g.mean()
        h = _pooled(P.Gamma(0.5, 1.0))                      # the boosted branch: mean 0.5, sd sqrt(0.5)
        assert (h > 0).all() and abs(h.mean() - 0.5) <= 6 * np.sqrt(0.5) / np.sqrt(n), h.mean()
    finally:
        oracle.set_dtype(old)


def test_salt_and_the_invalid_rule(oracle, real):
    d = P.Normal(1.0, 2.0)
    salted = P.one_draw(d, KA_SEED, 0, 0, 0)
    key = KA_SEED ^ 0x5052454449435421
    # the restatement under the salted key, block 0 of the family stream, normal 0 of its Box-Muller pair
    n = FR.bm_normal(FR.block(key, 0, 0, FR.STREAM_FAMILY, 0))
    assert salted.tobytes() == FR.fma(FR.r(2.0), n, FR.r(1.0)).tobytes() and type(salted) is oracle.real()
    unsalted = P.one_draw(d, KA_SEED, 0, 0, 0, salt=0)
    assert np.isfinite(unsalted) and unsalted != salted
    # every index, chain and saved draw its own number
    assert len({float(P.one_draw(d, KA_SEED, c, t, k)) for c in (0, 1, 2 ** 32) for t in (0, 1) for k in (0, 1)}) == 12
    # invalid parameters: NaN, for every family; a valid neighbour draws
    for bad in (P.Normal(0.0, 0.0), P.Normal(np.inf, 1.0), P.Uniform(1.0, 1.0), P.Laplace(0.0, -1.0), P.Cauchy(np.nan, 1.0),
                P.Exponential(0.0), P.Gamma(2.5, np.inf), P.InverseGamma(0.5, -2.0)):
        assert np.isnan(P.one_draw(bad, KA_SEED, 3, 4, 5)), (bad.family, bad.params())
    for good in (P.Uniform(1.0, 2.0), P.Exponential(0.5), P.InverseGamma(0.5, 2.0), P.Cauchy(0.0, 1.0)):
        assert np.isfinite(P.one_draw(good, KA_SEED, 3, 4, 5))
    s = P.Stream(KA_SEED, 3, 4)
    assert [s(P.Uniform(1.0, 2.0)), s(P.Uniform(1.0, 2.0))] == [P.one_draw(P.Uniform(1.0, 2.0), KA_SEED, 3, 4, k) for k in (0, 1)]
