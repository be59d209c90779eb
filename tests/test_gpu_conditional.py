"""GPU: Metropolis-Hastings runs whose proposal is a FUNCTION of the state (conditional proposals, kernel variant 14) against the
test-side restatement of the arithmetic spec (tests/conditional_restatement.py), bit for bit; constant maps against the component
runs of variant 13; the two kernel forms against each other; shards and resume; known answers; the Python API; refusals.
Reference behaviour under test: src/proposal.jl:92-126,195-196; src/mh-core.jl:92-117; test/runtests.jl:190,215-286."""
import ctypes as C

import numpy as np
import pytest

import cases
import conditional_restatement as R
import family_restatement as F
import user_targets

pytestmark = pytest.mark.gpu

KF_FAMILY, KF_COND = 13, 14
REG_MAX_DIM = {"f64": 20, "f32": 32}               # MHX_COND_REG_MAX_DIM (tests/test_conditional_cpu.py reads it from the header)


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    assert a.dtype == b.dtype, "%s: dtypes %s / %s" % (what, a.dtype, b.dtype)
    bad = np.argwhere(cases.bits(a) != cases.bits(b))
    assert len(bad) == 0, "%s: %d mismatches, first at %s: %r vs %r" % (what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


def tracing_namespace(mhx):
    """the namespace a case's parameter map is traced with (the restatement evaluates the same map with R.WIDTH)"""
    T = mhx.trace

    class M:
        log, exp, abs, fma, sum_over = staticmethod(T.log), staticmethod(T.exp), staticmethod(T.abs), staticmethod(T.fma), staticmethod(T.sum_over)
        c = staticmethod(float)
    return M


def dists(mhx, params):
    """[(family, p0, p1)] -> the engine's distribution objects"""
    cls = [mhx.Normal, mhx.Uniform, mhx.Laplace, mhx.Cauchy, mhx.Exponential, mhx.Gamma, mhx.InverseGamma]
    return [cls[f](p0) if f == F.EXPONENTIAL else cls[f](p0, p1) for f, p0, p1 in params]


def function_of(mhx, pmap, d):
    m = tracing_namespace(mhx)
    if d == 1:
        return lambda x: dists(mhx, pmap(m, [x]))[0]
    return lambda x: dists(mhx, pmap(m, x))


def sampler_of(mhx, pmap, d, static, symmetric=False):
    fn = function_of(mhx, pmap, d)
    if static:
        return mhx.MetropolisHastings(mhx.StaticProposal(fn, dim=d, issymmetric=symmetric))
    return mhx.MetropolisHastings(mhx.RandomWalkProposal(fn, issymmetric=symmetric, dim=d))


def _run(mhx, model, spl, C_, N, seed, first_chain=0, flags=0, init=None, ctx=None):
    run = mhx.Run(model, spl, nchains=C_, seed=seed, first_chain=first_chain, flags=flags, ctx=ctx)
    run.init(init)
    run.sample(N, 0, 1, 0)
    value, acc = run.samples()
    return run, value, acc


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit-exact against the restatement
C1, N1, FIRST1 = 70, 12, 3                          # a full wave and a partial one
_restated = {}


def _restatement(oracle, real, name, static, symmetric=False, with_z=True):
    key = (real, name, static, symmetric, with_z)
    if key not in _restated:
        d, pmap, init = R.CASES[name]
        _restated[key] = R.run(oracle.iso_gauss(d), pmap, d, N1, 0xC0D1 + d, FIRST1, C1, init(C1), static=static, symmetric=symmetric,
                               with_z=with_z)
    return _restated[key]


def _compare(mhx, oracle, real, name, static, form, symmetric=False):
    d, pmap, init = R.CASES[name]
    ref = _restatement(oracle, real, name, static, symmetric)
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    run, value, acc = _run(mhx, mhx.DensityModel(mhx.IsoGaussian(d)), sampler_of(mhx, pmap, d, static, symmetric), C1, N1, 0xC0D1 + d,
                           FIRST1, flags, init(C1))
    assert run.stats()["kernel_variant"] == KF_COND and run.stats()["reduce_lanes"] == 1
    _same(value, ref["samples"], "samples")
    _same(acc, ref["accepted"], "accepted")
    x, lp, cnt = run.state()
    _same(x, ref["final_x"], "final x")
    _same(lp, ref["final_lp"], "final lp")
    _same(cnt, ref["accept_counts"], "accept counts")
    assert run.stats()["accepted"] == int(ref["accept_counts"].sum())
    run.close()
    return ref


@pytest.mark.parametrize("form", ["register", "generic"])
@pytest.mark.parametrize("static", [False, True], ids=["walk", "static"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_conditional_runs_bit_exact_against_the_restatement(mhx, oracle, real, name, static, form):
    """Cases (a) - (e) x {walk, static} x {register form, state-in-HBM form}: samples, accept flags, final state and counts equal the
    restatement's.  What keeps a case from hiding a failure is asserted too: the restatement accepts some transitions and rejects
    some, and (cases a - d) leaving Z out of the ratio changes the chain within these 12 samples.  One combination cannot meet
    either condition, by the arithmetic itself: case (c) as a WALK has one-sided components (Exponential, Gamma, InverseGamma),
    whose K(p(y); x - y) is -Inf for every step xi > 0 -- it never accepts, exactly as the reference and the component runs
    behave (tests/test_gpu_families.py: test_a_one_sided_walk_never_accepts).  That combination is compared all the same, its zero
    acceptance asserted, and the walk of case (c) with accepted moves is covered by the declared-symmetric test below."""
    ref = _compare(mhx, oracle, real, name, static, form)
    total = int(ref["accept_counts"].sum())
    if name == "c_every_family" and not static:
        assert total == 0
        return
    assert 0 < total < C1 * (N1 - 1)
    if name != "e_scale_is_the_state":
        noz = _restatement(oracle, real, name, static, with_z=False)
        assert not np.array_equal(cases.bits(noz["samples"]), cases.bits(ref["samples"])), "Z does not matter in this case"
    else:
        # the scale is the state: it must stay positive, and some candidates must have been refused for their parameters alone
        assert (ref["samples"][:, 0, :] > 0).all()


@pytest.mark.parametrize("form", ["register", "generic"])
def test_every_family_walk_declared_symmetric_against_the_restatement(mhx, oracle, real, form):
    """RandomWalkProposal{true}: the ratio is not formed, so the walk of case (c) moves; p(y) is still evaluated and checked"""
    ref = _compare(mhx, oracle, real, "c_every_family", False, form, symmetric=True)
    assert 0 < int(ref["accept_counts"].sum()) < C1 * (N1 - 1)


def test_invalid_candidates_are_rejected_explicitly(mhx, oracle, real):
    """case (e), Normal(0, x): candidates with y <= 0 exist in the restatement and every one of them was rejected; the device chain,
    which equals the restatement (test above), never leaves x > 0"""
    d, pmap, init = R.CASES["e_scale_is_the_state"]
    ref = _restatement(oracle, real, "e_scale_is_the_state", False)
    x0 = init(C1)
    # recompute the candidates of the first transition: some are negative
    negative = 0
    for c in range(C1):
        x = [F.r(x0[0][c]) + F.r(0)]
        xi = F.draw_all(R.rows_of(pmap(R.WIDTH, x)), 0xC0D1 + d, FIRST1 + c, 1, oracle.STREAM_PROPOSAL, F.STREAM_FAMILY)
        if not (x[0] + xi[0] > 0):
            negative += 1
            assert ref["accepted"][1, c] == 0
    assert negative > 0
    run, value, acc = _run(mhx, mhx.DensityModel(mhx.IsoGaussian(1)), sampler_of(mhx, pmap, 1, False), C1, 40, 0xC0D1 + d, FIRST1, 0, x0)
    assert (value[:, 0, :] > 0).all() and 0 < acc[1:].mean() < 1
    run.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. constant maps reproduce the component runs
@pytest.mark.parametrize("form", ["register", "generic"])
@pytest.mark.parametrize("static", [False, True], ids=["walk", "static"])
def test_a_constant_map_reproduces_the_component_run(mhx, real, static, form):
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    if static:
        make = lambda: [mhx.Normal(0, 1), mhx.InverseGamma(2, 3)]
        init = np.abs(np.random.default_rng(3).normal(size=(2, 200))) + 0.25
    else:
        make = lambda: [mhx.Normal(0, 1), mhx.Laplace(0, 2), mhx.Cauchy(0, 0.5)]
        init = np.random.default_rng(3).normal(size=(3, 200))
    d = len(make())
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    P = mhx.StaticProposal if static else mhx.RandomWalkProposal
    r0, v0, a0 = _run(mhx, model, mhx.MetropolisHastings(P(make())), 200, 30, 99, 7, flags, init)
    r1, v1, a1 = _run(mhx, model, mhx.MetropolisHastings(P(lambda x: make(), dim=d)), 200, 30, 99, 7, flags, init)
    assert r0.stats()["kernel_variant"] == KF_FAMILY and r1.stats()["kernel_variant"] == KF_COND
    assert np.array_equal(v0, v1) and np.array_equal(a0, a1)
    _same(v0, v1, "samples")
    assert 0 < a0[1:].mean() < 1
    for got, want, what in zip(r1.state(), r0.state(), ("x", "lp", "accept counts")):
        _same(got, want, what)
    r0.close(), r1.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the two forms give identical bytes at the register form's dimension limit
def _wide_map(d):
    def pmap(m, x):
        out = []
        for k in range(d):
            s = m.c(0.1) + m.c(0.05) * m.abs(x[(k + 1) % d])
            out.append([(F.CAUCHY, m.c(0.01) * x[k], m.c(0.5) * s), (F.LAPLACE, 0.0, s), (F.NORMAL, 0.0, s), (F.UNIFORM, -s, s)][k % 4])
        return out
    return pmap


def test_the_forms_agree_at_the_register_forms_dimension_limit(mhx, real):
    """d = MHX_COND_REG_MAX_DIM: the register form against the state-in-HBM form; one dimension more runs on the state-in-HBM form
    by itself -- on a fresh context exactly one run-time module is compiled either way, and at limit + 1 it is the same module
    MHX_FLAG_GENERIC asks for (no register-form module)"""
    import mhx._lib as L
    dmax = REG_MAX_DIM[real]
    for d in (dmax, dmax + 1):
        pmap = _wide_map(d)
        model = mhx.DensityModel(mhx.IsoGaussian(d))
        init = np.random.default_rng(8).normal(size=(d, 300))
        ctx = L.Context(0, real)
        before = sum(ctx.jit_counts())
        r0, v0, a0 = _run(mhx, model, sampler_of(mhx, pmap, d, False), 300, 25, 5, 0, 0, init, ctx=ctx)
        assert sum(ctx.jit_counts()) - before == 1, d
        r1, v1, a1 = _run(mhx, model, sampler_of(mhx, pmap, d, False), 300, 25, 5, 0, mhx.FLAG_GENERIC, init, ctx=ctx)
        # the state-in-HBM module is new at the limit (the first run compiled the register form) and the SAME at limit + 1
        assert sum(ctx.jit_counts()) - before == (2 if d == dmax else 1), d
        _same(v0, v1, "d = %d: samples" % d)
        _same(a0, a1, "d = %d: accepted" % d)
        assert r0.stats()["kernel_variant"] == KF_COND and 0 < a0[1:].mean() < 1
        r0.close(), r1.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. shards and resume are the whole run
@pytest.mark.parametrize("form", ["register", "generic"])
def test_shards_and_resume_are_the_whole_run(mhx, real, form):
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    d, pmap, _ = R.CASES["b_cross_coordinates"]
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = sampler_of(mhx, pmap, d, True)
    Cn, N = 200, 41
    init = np.random.default_rng(21).normal(size=(d, Cn))
    whole, value, acc = _run(mhx, model, spl, Cn, N, 31, 1000, flags, init)
    a, va, aa = _run(mhx, model, spl, 70, N, 31, 1000, flags, init[:, :70])
    b, vb, ab = _run(mhx, model, spl, Cn - 70, N, 31, 1070, flags, init[:, 70:])
    _same(np.concatenate([va, vb], axis=2), value, "shards: samples")
    _same(np.concatenate([aa, ab], axis=1), acc, "shards: accepted")
    a.close(), b.close()
    first = mhx.Run(model, spl, nchains=Cn, seed=31, first_chain=1000, flags=flags)
    first.init(init)
    first.sample(17, 0, 1, 0)
    v1, a1 = first.samples()
    blob = first.save_state()
    first.close()
    second = mhx.Run(model, spl, nchains=Cn, seed=31, first_chain=1000, flags=flags)
    second.load_state(blob)
    second.sample(N - 17, 1, 1, 0)
    v2, a2 = second.samples()
    _same(np.concatenate([v1, v2], axis=0), value, "resume: samples")
    _same(np.concatenate([a1, a2], axis=0), acc, "resume: accepted")
    for got, want, what in zip(second.state(), whole.state(), ("x", "lp", "accept counts")):
        _same(got, want, "resume: final " + what)
    assert 0 < acc[1:].mean() < 1
    second.close(), whole.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. known answers
def test_symmetric_static_function_proposal_on_the_scalar_normal_model(mhx, real):
    """test/runtests.jl:215-259: target Normal(5, 0.7), SymmetricStaticProposal(x -> Normal(x, 1)); mean and std within 0.05, the
    reference's own tolerance; 4096 chains x 60 recorded after 200 discarded = 245 760 draws (the reference takes 100 000)"""
    model = mhx.DensityModel(mhx.HipLogDensity(user_targets.SHIFTED_GAUSS, 1, [5.0, 0.7]))
    spl = mhx.MetropolisHastings(mhx.SymmetricStaticProposal(lambda x: mhx.Normal(x, 1), dim=1))
    chain = mhx.sample(model, spl, 60, 4096, seed=12, discard_initial=200, initial_params=np.zeros(1), param_names=["x"])
    assert chain.stats["kernel_variant"] == KF_COND
    x = chain["x"].astype(np.float64)
    print("mean %.4f std %.4f acceptance %.3f" % (x.mean(), x.std(), chain.accepted.mean()))
    assert abs(x.mean() - 5.0) < 0.05 and abs(x.std() - 0.7) < 0.05, (x.mean(), x.std())


def test_heteroscedastic_walk_targets_the_standard_normal(mhx, real):
    """RandomWalkProposal(x -> Normal(0, 0.5 + |x|)), not declared symmetric, on N(0, 1): the final states of n = 8192 chains after
    300 transitions.  Bounds derived, not measured: mean within 5 standard errors of 0, 5 / sqrt(n) = 0.055; variance within 5
    standard errors of 1, 5 sqrt(2 / n) = 0.078.  The same walk WITHOUT the ratio (numpy, 200 000 chains, 300 steps) has variance
    0.874 (with it: 1.001), well outside that band: the test sees a missing or wrong ratio."""
    n = 8192
    model = mhx.DensityModel(mhx.IsoGaussian(1))
    spl = mhx.MetropolisHastings(mhx.RandomWalkProposal(lambda x: mhx.Normal(0, 0.5 + abs(x)), dim=1))
    run = mhx.Run(model, spl, nchains=n, seed=2025)
    run.init(np.zeros(1))
    run.sample(1, 300, 1, 0)
    x = run.state()[0][0].astype(np.float64)
    assert run.stats()["kernel_variant"] == KF_COND
    run.close()
    print("mean %.4f var %.4f" % (x.mean(), x.var()))
    assert abs(x.mean()) < 0.055 and abs(x.var() - 1.0) < 0.078, (x.mean(), x.var())


# ---------------------------------------------------------------------------------------------------------------------
# 6. the Python API end to end
def test_sample_returns_chains_for_a_function_proposal(mhx, real):
    model = mhx.DensityModel(mhx.HipLogDensity(user_targets.SHIFTED_GAUSS, 1, [5.0, 0.7]))        # a user log-density and a map: one module
    spl = mhx.MetropolisHastings(mhx.StaticProposal(lambda x: mhx.Normal(x, 1), dim=1))
    chain = mhx.sample(model, spl, 100, 64, seed=3, initial_params=np.full(1, 4.0))
    assert chain.stats["kernel_variant"] == KF_COND and chain.names == ["param_1", "lp"]
    assert chain.value.shape == (100, 2, 64) and 0 < chain.accepted[1:].mean() < 1
    assert np.isfinite(chain.value).all()
    stats = chain.summarystats()
    assert "param_1" in str(stats) or "param_1" in stats
    named = mhx.sample(model, spl, 50, 8, seed=3, initial_params=np.full(1, 4.0), param_names=["mu"])
    assert named.names == ["mu", "lp"] and named["mu"].shape == (50, 8)
    rows = mhx.sample(model, spl, 20, seed=3, initial_params=np.full(1, 4.0), chain_type=dict)
    assert len(rows) == 20 and tuple(rows[0].keys()) == ("param_1", "lp")
    with pytest.raises(mhx.ArgumentError, match="initial_params"):
        mhx.sample(model, spl, 10, 8, seed=3)


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals
def test_refusals(mhx, real):
    import mhx._lib as L
    T = mhx.trace
    model = mhx.DensityModel(mhx.IsoGaussian(2))
    fn = lambda x: [mhx.Normal(0, 0.5 + abs(x[1])), mhx.Laplace(0, T.exp(0.3 * x[0]))]
    spl = mhx.MetropolisHastings(mhx.RandomWalkProposal(fn, dim=2))
    ok_init = np.zeros((2, 8))

    def later_valid_run():
        run = mhx.Run(model, spl, nchains=8, seed=1)
        run.init(ok_init)
        run.sample(5, 0, 1, 0)
        assert run.stats()["kernel_variant"] == KF_COND
        run.close()

    run = mhx.Run(model, spl, nchains=8)
    with pytest.raises(mhx.ArgumentError, match="initial_params"):
        run.init(None)
    with pytest.raises(mhx.ArgumentError, match="initial_params"):                   # the C entry itself
        L.check(L.lib().mhx_run_init(run.h, None))
    run.close()
    later_valid_run()
    with pytest.raises(mhx.ArgumentError, match="NO_JIT"):
        mhx.Run(model, spl, nchains=8, flags=mhx.FLAG_NO_JIT)
    with pytest.raises(mhx.ArgumentError, match="ZIGGURAT"):
        mhx.Run(model, spl, nchains=8, normal_gen="ziggurat")
    with pytest.raises(mhx.ArgumentError, match="reduce_lanes"):
        mhx.Run(model, spl, nchains=8, reduce_lanes=2)
    later_valid_run()
    run = mhx.Run(model, spl, nchains=8)
    run.init(ok_init)
    with pytest.raises(mhx.ArgumentError, match="moments"):
        run.sample(10, 0, 1, 0, save="moments")
    run.sample(3, 0, 1, 0)                                                            # the run is still usable
    run.close()
    with pytest.raises((mhx.ArgumentError, T.TraceError), match="shape"):
        mhx.RandomWalkProposal(lambda x: [mhx.Gamma(1.0 + abs(x[0]), 1.0), mhx.Normal(0, 1)], dim=2)
    with pytest.raises((mhx.ArgumentError, T.TraceError), match="TDist"):
        mhx.RandomWalkProposal(lambda x: [mhx.TDist(3), mhx.Normal(0, 1)], dim=2)
    with pytest.raises((mhx.ArgumentError, T.TraceError), match="must return 2"):
        mhx.RandomWalkProposal(lambda x: [mhx.Normal(0, 1)], dim=2)
    later_valid_run()
    # initial states at which the map gives no distribution: Normal(0, x[0]) at x[0] <= 0 (one chain of eight)
    bad = mhx.MetropolisHastings(mhx.RandomWalkProposal(lambda x: [mhx.Normal(0, x[0]), mhx.Normal(0, 1)], dim=2))
    run = mhx.Run(model, bad, nchains=8)
    init = np.ones((2, 8))
    init[0, 5] = -1.0
    with pytest.raises(mhx.ArgumentError, match="1 of 8 chains"):
        run.init(init)
    with pytest.raises(mhx.MhxError):                                                # not initialised: nothing to sample
        run.sample(3, 0, 1, 0)
    run.init(np.ones((2, 8)))
    run.sample(3, 0, 1, 0)
    with pytest.raises(mhx.ArgumentError, match="1 of 8 chains"):                    # set_params
        run.set_params(init)
    run.close()
    later_valid_run()
    # a source with a syntax error, through the C entry point: the JIT error channel
    ctx = L.Context.default()
    tab = (L.ProposalComponent * 2)(L.ProposalComponent(0, 0, 0.0, 1.0), L.ProposalComponent(0, 0, 0.0, 1.0))
    cfg = L.RwmhCfg(2, 8, 1, 0, 0, 1.0, None, 0, None, 0)
    h = C.c_void_p()
    src = b"MHX_PROPOSAL_PARAMS(x, p, d, data, ndata) { p.set(0, 1, MHX_R(0.5) + mhx_abs(x[1]) }\n"
    rc = L.lib().mhx_rwmh_create_conditional(ctx.h, model.handle(ctx), C.byref(cfg), tab, 2, src, None, 0, C.byref(h))
    assert rc == L.MHX_EJIT
    assert b"proposal_params.hip" in L.lib().mhx_last_error()
    good = src.replace(b"x[1]) }", b"x[1])); }")
    L.check(L.lib().mhx_rwmh_create_conditional(ctx.h, model.handle(ctx), C.byref(cfg), tab, 2, good, None, 0, C.byref(h)))
    L.lib().mhx_run_destroy(h)
    later_valid_run()
