"""GPU: posterior predictive draws (mhx_run_predict / mhx_ctx_predict / Run.predict / Chains.predict; csrc/mhx_derive_kernels.h,
DESIGN.md sections 3.16 and 6.5.6).  The predictive tensor is compared with tests/predictive_ref.py -- the spec restated from
tests/family_restatement.py and the oracle's primitives, nothing of the engine -- BIT FOR BIT: the positions of NaN agree and every
other value has the same bits.

Shapes, the smallest at which the frame can go wrong: C = 1, 63, 65, 257 (a lone lane, a partial wave, a wave plus a lane, two
blocks with a ragged second); a lane maps 1 draw at a time and a strip is 2 draws, option DERIVE_DRAWS makes that 2, 4 or 8 (strips
of 4, 8, 16), so n_saved = 1, 2, 7, 9: less than a group, a group plus a ragged end, a strip plus one -- for one count or another.
first_chain = 0 and 2^32 - 3: the chain id carries into counter word 1 inside the tensor.  Every reference tensor is computed once
(`_ref`) and shared."""
import ctypes as C

import numpy as np
import pytest

import derived_ref
import hpd_ref
import predictive_ref as P
import mhx.trace as T
from planted import plant, plant_ptr

pytestmark = pytest.mark.gpu

SEED = 0x5EED0FF1CE


def make(draw):
    """d = 3 -> 6 outputs from 9 draw indices: the seven families (Gamma with alpha >= 1, InverseGamma with alpha < 1: the boosted
    branch), a draw that nothing reads, a draw whose parameters are earlier draws, and an output that is arithmetic on a draw.  The
    Cauchy scale x2 + 4.25 is <= 0 where the tensor plants it so; the other scales are |.| + constant, invalid only for NaN / Inf."""
    def fn(x):
        x0, x1, x2 = x[0], x[1], x[2]
        n = draw(P.Normal(x0, abs(x1) + 0.5))
        u = draw(P.Uniform(x0, x0 + abs(x2) + 1.0))
        la = draw(P.Laplace(x2, abs(x1) + 0.5))
        draw(P.Cauchy(0.0, 1.0))                            # index 3: not read
        ca = draw(P.Cauchy(x0, x2 + 4.25))
        e = draw(P.Exponential(abs(x1) + 0.25))
        g = draw(P.Gamma(2.5, abs(x2) + 0.5))
        ig = draw(P.InverseGamma(0.5, abs(x1) + 1.0))
        h = draw(P.Normal(n, 0.5 + e))
        return [n, u - la, ca, e * g, ig, h * h - x0]
    return fn


MAP = T.trace_predictive(make(T.draw), 3)
NOUT = 6


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(bits)[~na], b.view(bits)[~nb])


def _tensor(real, N, nch, seed, edges=True):
    """[N][4][C] draws in (-4, 4); with `edges`, rows 0 .. 2 get a few zeros, infinities and NaNs, and row 2 the values that make the
    Cauchy scale x2 + 4.25 zero and negative"""
    R = np.float64 if real == "f64" else np.float32
    rng = np.random.default_rng(seed)
    x = rng.uniform(-4.0, 4.0, size=(N, 4, nch)).astype(R)
    if edges:
        for row, special in ((0, [np.inf, np.nan]), (1, [0.0, -0.0, -np.inf, np.nan]), (2, [-4.25, -8.0, np.inf, 0.0])):
            flat = x[:, row, :].reshape(-1)
            k = min(len(special), flat.size)
            flat[rng.choice(flat.size, size=k, replace=False)] = np.array(special, dtype=R)[:k]
            x[:, row, :] = flat.reshape(N, nch)
    return np.ascontiguousarray(x)


_REFS = {}


def _ref(real, N, nch, first_chain=0, edges=True, seed=SEED):
    """(source tensor, reference predictive tensor of MAP), computed once per shape; never written to"""
    key = (real, N, nch, first_chain, edges, seed)
    if key not in _REFS:
        x = _tensor(real, N, nch, 17 * N + nch, edges)
        want = P.tensor(make, x, seed, first_chain)
        x.flags.writeable = want.flags.writeable = False
        _REFS[key] = (x, want)
    return _REFS[key]


def _ctx_predict(mhx, run, ptr, shape, first_chain, traced, seed):
    N, d1, nch = shape
    h = C.c_void_p()
    mhx.check(mhx.lib().mhx_ctx_predict(run.ctx.h, ptr, N, d1, nch, first_chain, traced.source.encode(), traced.nout, None, 0, seed, C.byref(h)))
    return mhx.DerivedRun(h, run, traced.nout)


@pytest.mark.parametrize("first_chain", [0, 2 ** 32 - 3])
@pytest.mark.parametrize("nch", [1, 63, 65, 257])
@pytest.mark.parametrize("N", [1, 2, 7, 9])
def test_predictive_tensor_equals_the_reference(mhx, oracle, real, N, nch, first_chain):
    x, want = _ref(real, N, nch, first_chain)
    run, ptr = plant_ptr(mhx, np.array(x))
    # the planted run's own ids start at 0: the other first_chain goes through the caller's-tensor entry
    pre = run.predict(MAP, seed=SEED) if first_chain == 0 else _ctx_predict(mhx, run, ptr, x.shape, first_chain, MAP, SEED)
    try:
        assert isinstance(pre, mhx.DerivedRun) and (pre.dim, pre.n) == (NOUT, nch) and pre.form_name() == "derived"
        got, acc = pre.samples()
        assert acc is None and got.shape == (N, NOUT + 1, nch)
        assert _same_bits(got, want), (N, nch, first_chain, np.argwhere(got.view(np.uint8) != want.view(np.uint8))[:4])
        assert _same_bits(got[:, NOUT, :], x[:, -1, :])                       # the last row is the source's lp row, bit for bit
        if N * nch >= 63:                                                     # the planted values are all there: the NaN rule was exercised
            assert np.isnan(got[:, 2, :]).sum() >= 2 and np.isnan(got[:, 0, :]).sum() >= 2
            assert np.isfinite(got[:, :NOUT, :]).sum() > 0.5 * got[:, :NOUT, :].size
        st = pre.stats()
        assert st["transitions"] == 0 and st["launches"] == 1 and st["dtype"] == real
    finally:
        pre.close()
        run.close()


def test_draws_per_lane_seed_and_repetition(mhx, oracle, real, engine):
    x, want = _ref(real, 9, 65)
    run = plant(mhx, np.array(x))
    try:
        for U in (1, 2, 4, 8):                                                # DERIVE_DRAWS: a grid shape, not a part of the draw
            engine.set("DERIVE_DRAWS", str(U))
            pre = run.predict(MAP, seed=SEED)
            assert _same_bits(pre.samples()[0], want), U
            pre.close()
        engine.delenv("DERIVE_DRAWS")
        a, b, other = run.predict(MAP, seed=SEED), run.predict(MAP, seed=SEED), run.predict(MAP, seed=SEED + 1)
        assert _same_bits(a.samples()[0], want) and _same_bits(b.samples()[0], want)           # the same call twice
        o = other.samples()[0]
        fin = np.isfinite(o[:, :NOUT, :]) & np.isfinite(want[:, :NOUT, :])
        assert fin.sum() > 0.8 * fin.size and (o[:, :NOUT, :][fin] != want[:, :NOUT, :][fin]).mean() > 0.99      # another seed
        # seed=None is the run's own seed (tests/planted.py: 1)
        assert run.seed == 1
        dflt, own = run.predict(MAP), run.predict(MAP, seed=run.seed)
        assert _same_bits(dflt.samples()[0], own.samples()[0]) and not _same_bits(dflt.samples()[0], want)
        assert _same_bits(own.samples()[0], _ref(real, 9, 65, seed=1)[1])
        for r in (a, b, other, dflt, own):
            r.close()
    finally:
        run.close()


def test_a_predictive_run_of_a_derived_run_uses_the_original_ids(mhx, oracle, real):
    x, want = _ref(real, 7, 65, 2 ** 32 - 3)
    run, ptr = plant_ptr(mhx, np.array(x))
    ident = "MHX_DERIVED(x, y, d, data, ndata) { y.set(0, x[0]); y.set(1, x[1]); y.set(2, x[2]); }\n"
    try:
        # a derived run made from a caller's tensor by the predict entry carries first_chain; the identity derive of it inherits it, and
        # the predictive run of that numbers its chains first_chain + c
        first = _ctx_predict(mhx, run, ptr, x.shape, 2 ** 32 - 3, T.trace_predictive(lambda t: [t[0], t[1], t[2]], 3), SEED)
        same = first.derive(mhx.HipMap(ident, 3))
        pre = same.predict(MAP, seed=SEED)
        assert _same_bits(first.samples()[0], x) and _same_bits(same.samples()[0], x)
        assert _same_bits(pre.samples()[0], want)
        # and on a run of ids of its own (0 ..): predict(derive(identity)) == predict(source) == the reference of those ids
        d2 = run.derive(mhx.HipMap(ident, 3))
        p1, p2 = d2.predict(MAP, seed=SEED), run.predict(MAP, seed=SEED)
        assert _same_bits(p1.samples()[0], p2.samples()[0]) and _same_bits(p2.samples()[0], _ref(real, 7, 65, 0)[1])
        for r in (pre, same, first, p1, p2, d2):
            r.close()
    finally:
        run.close()


def test_ctx_form_equals_the_run_form(mhx, oracle, real):
    x, want = _ref(real, 7, 65)
    run, ptr = plant_ptr(mhx, np.array(x))
    try:
        a, b = _ctx_predict(mhx, run, ptr, x.shape, 0, MAP, SEED), run.predict(MAP, seed=SEED)
        assert _same_bits(a.samples()[0], b.samples()[0]) and _same_bits(a.samples()[0], want)
        a.close()
        b.close()
    finally:
        run.close()


def test_statistics_and_refusals_of_a_predictive_run(mhx, oracle, real):
    N, nch = 16, 65
    x, ref = _ref(real, N, nch, edges=False)
    run = plant(mhx, np.array(x))
    pre = run.predict(MAP, seed=SEED)
    try:
        assert _same_bits(pre.samples()[0], ref) and np.isfinite(ref).all()
        S = N * nch
        rows = np.sort(np.moveaxis(ref, 1, 0).reshape(NOUT + 1, -1).astype(np.float64), axis=1)
        j, j1, g = mhx.api.quantile_ranks(S, np.array(mhx.api.DEFAULT_QUANTILE_PROBS))
        assert np.array_equal(pre.quantiles(), mhx.api.quantiles_from_order_statistics(rows[:, j], rows[:, j1], g, top=rows[:, S - 1]))
        lo, hi = pre.hpd(0.05)
        wlo, whi = hpd_ref.hpd_rows(ref, 0.05)
        assert np.array_equal(lo, wlo) and np.array_equal(hi, whi)
        counts, edges, outside = pre.histogram(bins=16, params=[0, 1, 3, 5])
        for k, p in enumerate([0, 1, 3, 5]):
            wc, we = np.histogram(ref[:, p, :].astype(np.float64).ravel(), bins=16)
            assert np.array_equal(counts[k], wc) and np.array_equal(edges[k], we) and outside[k].sum() == 0
        # a second map on the predictive run: a test statistic of y_rep, by the unchanged derive
        t2 = pre.derive(lambda y: y[0] * y[0])
        assert _same_bits(t2.samples()[0][:, 0, :], ref[:, 0, :] * ref[:, 0, :])
        t2.close()
        # what steps or reads sampler state refuses a predictive run as it refuses a derived one
        state = run.save_state()
        for call in (lambda: pre.sample(4), lambda: pre.init(None), lambda: pre.set_params(np.zeros((NOUT, nch))), lambda: pre.save_state(),
                     lambda: pre.load_state(state), lambda: pre.factor(), lambda: pre.step_stats(), lambda: pre.state()):
            with pytest.raises(mhx.MhxError, match="derived") as e:
                call()
            assert e.value.code == mhx.MHX_ESTATE
    finally:
        pre.close()
        run.close()


def test_chains_predict_on_the_readme_model(mhx, oracle, real):
    data = np.random.default_rng(1234).normal(0.0, 1.0, size=30)
    model = mhx.DensityModel(mhx.IIDNormal(data))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(2), 0.25 * mhx.I))
    chain = mhx.sample(model, spl, 200, 256, param_names=["mu", "sigma"], chain_type=mhx.Chains, discard_initial=200,
                       initial_params=np.array([0.0, 1.0]), seed=1234)
    rep = chain.predict(lambda t: mhx.Normal(t.mu, t.sigma), names=["y_rep"])
    try:
        assert rep.names == ["y_rep", "lp"] and rep.value.shape == (200, 2, 256) and isinstance(rep.state, mhx.DerivedRun)
        assert _same_bits(rep["lp"], chain["lp"]) and "y_rep" in rep.describe()
        y, mu = rep["y_rep"].astype(np.float64), chain["mu"].astype(np.float64)
        assert np.isfinite(y).all()                                           # (sigma > 0 on every draw of this posterior)
        # y_rep - mu = sigma * n, n independent of the chain: the difference of the pooled means has variance E sigma^2 / n <=
        # (var y_rep + var mu) / n, the bound formed from the two runs' own variances.  This tests the wiring, not the generator.
        n = y.size
        se = np.sqrt((y.var() + mu.var()) / n)
        print("PREDICT_E2E %s mean(y_rep) - mean(mu) = %.3g, 6 se = %.3g" % (real, y.mean() - mu.mean(), 6 * se))
        assert abs(y.mean() - mu.mean()) <= 6 * se
        # a posterior predictive check is a derive of y_rep away
        t = rep.derive(lambda r: T.where(r.y_rep > 0.0, 1.0, 0.0), names=["positive"])
        assert 0.2 < t.mean("positive") < 0.8
        t.state.close()
    finally:
        rep.state.close()
        chain.state.close()


SRC_HAND = """
MHX_PREDICTIVE(x, rng, y, d, data, ndata)
{
    const mhx_real n = rng.draw(0, MHX_FAMILY_NORMAL, x[0], mhx_abs(x[1]) + MHX_R(0.5));
    y.set(0, n);
    y.set(1, rng.draw(1, MHX_FAMILY_EXPONENTIAL, mhx_abs(n) + data[0], MHX_R(0.0)));
}
"""
SRC_BAD = "MHX_PREDICTIVE(x, rng, y, d, data, ndata) { y.set(0, x[0] +* ); }\n"


def test_hand_written_source_bad_source_and_an_unchanged_derive(mhx, oracle, real):
    x, _ = _ref(real, 7, 65)
    run = plant(mhx, np.array(x))
    sq = "MHX_DERIVED(x, y, d, data, ndata) { y.set(0, x[2] * x[2]); }\n"
    try:
        before = run.derive(mhx.HipMap(sq, 1))
        want_sq = derived_ref.host_map(oracle, sq)(x, 1, None)
        assert _same_bits(before.samples()[0], want_sq) and before.stats()["launches"] == 1
        hand = run.predict(mhx.HipPredictive(SRC_HAND, 2, data=[0.25]), seed=SEED)

        def traced(t):
            n = T.draw(P.Normal(t[0], abs(t[1]) + 0.5))
            return [n, P.Exponential(abs(n) + 0.25)]
        auto = run.predict(traced, seed=SEED)
        got = hand.samples()[0]
        assert _same_bits(got, auto.samples()[0]) and np.isfinite(got).mean() > 0.8
        with pytest.raises(mhx.ArgumentError, match="predictive.hip") as e:
            run.predict(mhx.HipPredictive(SRC_BAD, 1))
        assert "error" in str(e.value) and "does not compile" in str(e.value) and e.value.code == mhx.MHX_EINVAL
        # each kind of map goes to its own entry
        with pytest.raises(mhx.ArgumentError, match="predict"):
            run.predict(mhx.HipMap(sq, 1))
        with pytest.raises(mhx.ArgumentError, match="derive"):
            run.derive(mhx.HipPredictive(SRC_HAND, 2, data=[0.25]))
        with pytest.raises(mhx.ArgumentError, match="cannot be traced"):
            run.derive(traced)                                                # draw outside a predictive trace
        # the derive of before, after: the same module, the same bits, one launch
        counts = run.ctx.jit_counts()
        after = run.derive(mhx.HipMap(sq, 1))
        assert run.ctx.jit_counts() == counts
        assert _same_bits(after.samples()[0], want_sq) and after.stats()["launches"] == 1
        for r in (before, hand, auto, after):
            r.close()
    finally:
        run.close()
