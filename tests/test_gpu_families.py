"""GPU: Metropolis-Hastings runs whose proposal is a vector of univariate family components (kernel variant 13) against the test-side
restatement of the arithmetic spec (tests/family_restatement.py), bit for bit; the two kernel forms against each other; shard /
resume / symmetric-flag invariances; the device draws against their laws; the reference's known answers.
Reference behaviour under test: src/proposal.jl:23-35,41-83,195; src/mh-core.jl:83,92-117; README.md:106-111;
test/runtests.jl:56-74,181-201,215-271."""
import math
import os

import numpy as np
import pytest

import cases
import family_restatement as F
import test_families_cpu as CPU
import user_targets

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KF_FAMILY = 13


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    assert a.dtype == b.dtype, "%s: dtypes %s / %s" % (what, a.dtype, b.dtype)
    bad = np.argwhere(cases.bits(a) != cases.bits(b))
    assert len(bad) == 0, "%s: %d mismatches, first at %s: %r vs %r" % (what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


def readme_data():
    return np.load(os.path.join(GOLD, "c1_normal_data.npy"))[:30]


def _dist(m, fam, p0, p1):
    return {F.NORMAL: lambda: m.Normal(p0, p1), F.UNIFORM: lambda: m.Uniform(p0, p1), F.LAPLACE: lambda: m.Laplace(p0, p1),
            F.CAUCHY: lambda: m.Cauchy(p0, p1), F.EXPONENTIAL: lambda: m.Exponential(p0), F.GAMMA: lambda: m.Gamma(p0, p1),
            F.INVERSE_GAMMA: lambda: m.InverseGamma(p0, p1)}[fam]()


# name -> (components [(family, p0, p1)], static?, engine model, oracle target)
def _case(mhx, oracle, name):
    if name == "static_normal_inversegamma_readme":          # README.md:106: StaticProposal([Normal(0,1), InverseGamma(2,3)])
        data = readme_data()
        return ([(F.NORMAL, 0.0, 1.0), (F.INVERSE_GAMMA, 2.0, 3.0)], True, mhx.DensityModel(mhx.IIDNormal(data)),
                oracle.Target(oracle.TARGET_IID_NORMAL, 2, params=data))
    if name == "walk_laplace_cauchy_normal_uniform_banana":   # a catalogue target at its lane-per-chain reduction shape
        return ([(F.LAPLACE, 0.0, 0.3), (F.CAUCHY, 0.0, 0.1), (F.NORMAL, 0.0, 0.5), (F.UNIFORM, -0.2, 0.2)], False,
                mhx.DensityModel(mhx.Banana(4, 0.03)), oracle.Target(oracle.TARGET_BANANA, 4, params=[0.03]))
    if name == "walk_noncentred_laplace":                     # a ratio that is not zero
        return ([(F.LAPLACE, 0.1, 0.3)], False, mhx.DensityModel(mhx.IsoGaussian(1)), oracle.iso_gauss(1))
    if name == "static_gamma_half_boost":                     # alpha < 1: the alpha + 1 boost
        data = readme_data()
        return ([(F.NORMAL, 0.0, 1.0), (F.GAMMA, 0.5, 1.0)], True, mhx.DensityModel(mhx.IIDNormal(data)),
                oracle.Target(oracle.TARGET_IID_NORMAL, 2, params=data))
    raise KeyError(name)


CASES = ["static_normal_inversegamma_readme", "walk_laplace_cauchy_normal_uniform_banana", "walk_noncentred_laplace",
         "static_gamma_half_boost"]
_restated = {}


def _sampler(mhx, comps, static, symmetric=False):
    dists = [_dist(mhx, *c) for c in comps]
    if static:
        return mhx.MetropolisHastings(mhx.StaticProposal(dists))
    return mhx.MetropolisHastings(mhx.RandomWalkProposal(dists, symmetric))


def _run(mhx, model, spl, C, N, seed, first_chain=0, flags=0, init=None):
    run = mhx.Run(model, spl, nchains=C, seed=seed, first_chain=first_chain, flags=flags)
    run.init(init)
    run.sample(N, 0, 1, 0)
    value, acc = run.samples()
    return run, value, acc


@pytest.mark.parametrize("form", ["specialised", "generic", "no_jit"])
@pytest.mark.parametrize("given_init", [False, True], ids=["drawn", "given"])
@pytest.mark.parametrize("name", CASES)
def test_family_runs_bit_exact_against_the_restatement(mhx, oracle, real, name, given_init, form):
    C, N, seed, first = 40, 30, 0xFA3117 + CASES.index(name), 5
    comps, static, model, target = _case(mhx, oracle, name)
    d = len(comps)
    init = None
    if given_init:
        init = np.abs(np.random.default_rng(11).normal(size=(d, C))).astype(np.float32) + 0.25      # (sigma > 0 for the README model)
    key = (name, given_init, real)
    if key not in _restated:
        _restated[key] = F.run(target, comps, N, seed, first, C, static=static, init=init)
    ref = _restated[key]
    flags = {"specialised": 0, "generic": mhx.FLAG_GENERIC, "no_jit": mhx.FLAG_NO_JIT}[form]
    run, value, acc = _run(mhx, model, _sampler(mhx, comps, static), C, N, seed, first, flags, init)
    assert run.stats()["kernel_variant"] == KF_FAMILY and run.stats()["reduce_lanes"] == 1
    _same(value, ref["samples"], "samples")
    _same(acc, ref["accepted"], "accepted")
    x, lp, cnt = run.state()
    _same(x, ref["final_x"], "final x")
    _same(lp, ref["final_lp"], "final lp")
    _same(cnt, ref["accept_counts"], "accept counts")
    assert run.stats()["accepted"] == int(ref["accept_counts"].sum())
    assert 0 < int(ref["accept_counts"].sum()) < C * (N - 1)            # the case exercises both outcomes
    run.close()


ALL_FAMILIES = [(F.NORMAL, 0.0, 0.5), (F.UNIFORM, -0.3, 0.3), (F.LAPLACE, 0.05, 0.3), (F.CAUCHY, 0.0, 0.1), (F.EXPONENTIAL, 0.7, 0.0),
                (F.GAMMA, 3.0, 0.5), (F.INVERSE_GAMMA, 2.0, 3.0), (F.GAMMA, 0.5, 1.0), (F.NORMAL, 0.3, 1.0), (F.LAPLACE, 0.0, 1.0)]


@pytest.mark.parametrize("static", [True, False], ids=["static", "walk"])
def test_the_two_kernel_forms_give_identical_bytes(mhx, real, static):
    """every family at once, more chains than a block, a user log-density: specialised register form == state-in-HBM form"""
    comps = ALL_FAMILIES if static else [c for c in ALL_FAMILIES if c[0] not in (F.EXPONENTIAL, F.GAMMA, F.INVERSE_GAMMA)]
    d, C, N = len(comps), 1000, 60
    shift = np.concatenate([np.linspace(0.2, 1.5, d), np.full(d, 1.3)])
    models = {"catalogue": mhx.DensityModel(mhx.IsoGaussian(d)), "user": mhx.DensityModel(mhx.HipLogDensity(user_targets.SHIFTED_GAUSS, d, shift))}
    for mname, model in models.items():
        got = {}
        for form, flags in (("specialised", 0), ("generic", mhx.FLAG_GENERIC), ("no_jit", mhx.FLAG_NO_JIT)):
            run, value, acc = _run(mhx, model, _sampler(mhx, comps, static), C, N, 77, 123456789012, flags)
            assert run.stats()["kernel_variant"] == KF_FAMILY
            if mname == "catalogue":
                # both forms report variant 13: which one stepped the chains shows in the context's run-time modules -- on a FRESH
                # context the specialised form compiles (or takes from the disk cache) exactly one, the pre-built form none
                import mhx._lib as L
                ctx = L.Context(0, real)
                before = sum(ctx.jit_counts())
                probe = mhx.Run(model, _sampler(mhx, comps, static), nchains=64, seed=1, flags=flags, ctx=ctx)
                assert sum(ctx.jit_counts()) - before == (1 if form == "specialised" else 0), form
                probe.close()
            got[form] = (value, acc) + run.state()
            run.close()
        for form in ("generic", "no_jit"):
            for a, b, what in zip(got["specialised"], got[form], ("samples", "accepted", "x", "lp", "accept counts")):
                _same(a, b, "%s / %s: %s" % (mname, form, what))
        assert 0 < got["specialised"][1][1:].mean() < 1


def test_the_forms_agree_at_the_register_forms_dimension_limit(mhx, real):
    """d = MHX_FAM_REG_MAX_DIM (32 in fp64, 48 in fp32), the worst family for registers (Cauchy) among the components: the
    specialised form against the state-in-HBM form; one dimension more runs on the state-in-HBM form by itself"""
    import mhx._lib as L
    dmax = 32 if real == "f64" else 48
    for d, jit_modules in ((dmax, 1), (dmax + 1, 0)):
        comps = [[(F.CAUCHY, 0.0, 0.05), (F.LAPLACE, 0.0, 0.1), (F.NORMAL, 0.0, 0.2), (F.UNIFORM, -0.2, 0.2)][k % 4] for k in range(d)]
        model = mhx.DensityModel(mhx.IsoGaussian(d))
        ctx = L.Context(0, real)
        before = sum(ctx.jit_counts())
        probe = mhx.Run(model, _sampler(mhx, comps, False), nchains=64, seed=1, ctx=ctx)
        assert sum(ctx.jit_counts()) - before == jit_modules, d
        probe.close()
        r0, v0, a0 = _run(mhx, model, _sampler(mhx, comps, False), 300, 25, 5, 0, 0)
        r1, v1, a1 = _run(mhx, model, _sampler(mhx, comps, False), 300, 25, 5, 0, mhx.FLAG_GENERIC)
        _same(v0, v1, "d = %d: samples" % d)
        _same(a0, a1, "d = %d: accepted" % d)
        assert r0.stats()["kernel_variant"] == KF_FAMILY and 0 < a0[1:].mean() < 1
        r0.close(), r1.close()


@pytest.mark.parametrize("flags_name", ["specialised", "generic"])
def test_shards_and_resume_are_the_whole_run(mhx, real, flags_name):
    """chains by global id: the union of two shards by first_chain is the whole run; save / load / continue is the uninterrupted
    run, the static proposal's q(x) included"""
    flags = mhx.FLAG_GENERIC if flags_name == "generic" else 0
    comps = [(F.NORMAL, 0.0, 1.0), (F.INVERSE_GAMMA, 2.0, 3.0)]
    model = mhx.DensityModel(mhx.IIDNormal(readme_data()))
    spl = _sampler(mhx, comps, True)
    C, N = 200, 41
    whole, value, acc = _run(mhx, model, spl, C, N, 31, 1000, flags)
    a, va, aa = _run(mhx, model, spl, 70, N, 31, 1000, flags)
    b, vb, ab = _run(mhx, model, spl, C - 70, N, 31, 1070, flags)
    _same(np.concatenate([va, vb], axis=2), value, "shards: samples")
    _same(np.concatenate([aa, ab], axis=1), acc, "shards: accepted")
    for r in (a, b):
        r.close()
    # stop after 17 recorded states, save, load into a fresh run, continue
    first = mhx.Run(model, spl, nchains=C, seed=31, first_chain=1000, flags=flags)
    first.init(None)
    first.sample(17, 0, 1, 0)
    v1, a1 = first.samples()
    blob = first.save_state()
    first.close()
    second = mhx.Run(model, spl, nchains=C, seed=31, first_chain=1000, flags=flags)
    second.load_state(blob)
    second.sample(N - 17, 1, 1, 0)                          # sample 1 of the continuation = the state after one more transition
    v2, a2 = second.samples()
    _same(np.concatenate([v1, v2], axis=0), value, "resume: samples")
    _same(np.concatenate([a1, a2], axis=0), acc, "resume: accepted")
    for got, want, what in zip(second.state(), whole.state(), ("x", "lp", "accept counts")):
        _same(got, want, "resume: final " + what)
    # the same through Group (two members on one device)
    g = mhx.Group([0, 0])
    g.create(model, spl, nchains=C, seed=31, first_chain=1000, flags=flags)
    g.init(None)
    vals, accs = g.sample_to_host(N)
    _same(np.concatenate(vals, axis=2), value, "group: samples")
    _same(np.concatenate(accs, axis=1), acc, "group: accepted")
    assert g.stats()["kernel_variant"] == KF_FAMILY
    g.close()
    second.close()
    whole.close()


def test_sample_and_chains_work_on_a_family_run(mhx, real):
    """mhx.sample (the accept-compacted host path at >= 1024 chains) returns what Run.sample records; names from the dict form"""
    model = mhx.DensityModel(mhx.IIDNormal(readme_data()))
    spl = mhx.MetropolisHastings({"μ": mhx.StaticProposal(mhx.Normal(0, 1)), "σ": mhx.StaticProposal(mhx.InverseGamma(2, 3))})
    chain = mhx.sample(model, spl, 50, 1500, seed=4)
    assert chain.names == ["μ", "σ", "lp"] and chain.stats["kernel_variant"] == KF_FAMILY
    run, value, acc = _run(mhx, model, spl, 1500, 50, 4)
    _same(chain.value, value, "sample vs Run.sample")
    _same(chain.accepted, acc, "accepted")
    assert (chain["σ"] > 0).all()
    run.close()
    # test/runtests.jl:188-193: p2 = StaticProposal([Normal(0,1), InverseGamma(2,3)]) on m2, Vector{NamedTuple} keys
    m2 = mhx.DensityModel(mhx.HipLogDensity(user_targets.SHIFTED_GAUSS.replace("data[k]", "MHX_R(1.0)").replace("data[d + k]", "MHX_R(1.0)"), 2))
    c2 = mhx.sample(m2, mhx.MetropolisHastings(mhx.StaticProposal([mhx.Normal(0, 1), mhx.InverseGamma(2, 3)])), 100, chain_type=dict, seed=1)
    assert len(c2) == 100 and tuple(c2[0].keys()) == ("param_1", "param_2", "lp") and all(s["param_2"] > 0 for s in c2)


def test_a_zero_centred_walk_is_the_same_chain_declared_symmetric_or_not(mhx, real):
    """src/proposal.jl:195: the flag leaves the ratio out; for components symmetric about zero the ratio is exactly 0.0"""
    comps = [(F.LAPLACE, 0.0, 0.3), (F.CAUCHY, 0.0, 0.1), (F.NORMAL, 0.0, 0.5), (F.UNIFORM, -0.2, 0.2)]
    model = mhx.DensityModel(mhx.Banana(4, 0.03))
    for flags in (0, mhx.FLAG_GENERIC):
        r0, v0, a0 = _run(mhx, model, _sampler(mhx, comps, False, False), 300, 40, 9, 0, flags)
        r1, v1, a1 = _run(mhx, model, _sampler(mhx, comps, False, True), 300, 40, 9, 0, flags)
        _same(v1, v0, "samples")
        _same(a1, a0, "accepted")
        assert r0.stats()["kernel_variant"] == r1.stats()["kernel_variant"] == KF_FAMILY and 0 < a0[1:].mean() < 1
        r0.close(), r1.close()


def test_a_one_sided_walk_never_accepts(mhx, real):
    """RandomWalkProposal(Exponential(1)): q(x - y) = -Inf, log alpha = -Inf -- the package's behaviour, not a refusal"""
    model = mhx.DensityModel(mhx.IsoGaussian(1))
    for flags in (0, mhx.FLAG_GENERIC):
        init = np.linspace(-2.0, 2.0, 64).reshape(1, 64)
        run, value, acc = _run(mhx, model, mhx.RWMH(mhx.Exponential(1)), 64, 50, 3, 0, flags, init)
        assert run.stats()["accepted"] == 0 and not acc.any() and not run.state()[2].any()
        assert (value[:, 0, :] == value[0, 0, :]).all() and np.array_equal(value[0, 0, :], init[0].astype(value.dtype))
        run.close()


def test_device_draws_follow_their_laws(mhx, real):
    """initial_params = nothing, 65 536 chains: sample 1 of component k is a draw from family k (the DKW bound of the CPU test)"""
    laws = CPU.LAWS
    n = 65536
    model = mhx.DensityModel(mhx.IsoGaussian(len(laws)))
    spl = mhx.MetropolisHastings(mhx.StaticProposal([_dist(mhx, fam, p0, p1) for _, fam, p0, p1, _ in laws]))
    for flags in (0, mhx.FLAG_GENERIC):
        run, value, _ = _run(mhx, model, spl, n, 1, 2024, 0, flags)
        for k, (name, _, _, _, cdf) in enumerate(laws):
            xs = value[0, k, :].astype(np.float64)
            assert np.isfinite(xs).all(), name
            D = CPU.ks_distance(xs, cdf)
            print("%s [%s] device draw: D_n = %.5f, bound %.5f" % (name, real, D, CPU.dkw_bound(n)))
            assert D <= CPU.dkw_bound(n), (name, real, D, CPU.dkw_bound(n))
        run.close()


def _readme_posterior_means(data):
    """E[mu], E[sigma] under exp(sum logpdf(Normal(mu, sigma), data)) on sigma > 0 (the README model has no prior), by 2-D quadrature"""
    data = np.asarray(data, dtype=np.float64)
    n, m = data.size, data.mean()
    S = ((data - m) ** 2).sum()
    mu = np.linspace(m - 3.0, m + 3.0, 2401)[:, None]
    sg = np.linspace(1e-3, 8.0, 4000)[None, :]
    ll = -n * np.log(sg) - (S + n * (mu - m) ** 2) / (2.0 * sg * sg)
    w = np.exp(ll - ll.max())
    return float((w * mu).sum() / w.sum()), float((w * sg).sum() / w.sum())


def test_static_mh_with_an_inverse_gamma_component_on_the_readme_model(mhx, real):
    """README.md:106-111 on the README model; the tolerance 0.1 of test/runtests.jl:56-74, the sizes of
    test_static_mh_posterior_of_the_readme_model"""
    data = readme_data()
    want_mu, want_sigma = _readme_posterior_means(data)
    model = mhx.DensityModel(mhx.IIDNormal(data))
    chain = mhx.sample(model, mhx.StaticMH([mhx.Normal(0.0, 1.0), mhx.InverseGamma(2, 3)]), 400, 2048, seed=9, discard_initial=200)
    assert chain.stats["kernel_variant"] == KF_FAMILY
    mu, sig = chain.value[:, 0, :].mean(dtype=np.float64), chain.value[:, 1, :].mean(dtype=np.float64)
    print("posterior means: mu %.4f (quadrature %.4f), sigma %.4f (quadrature %.4f)" % (mu, want_mu, sig, want_sigma))
    assert abs(mu - want_mu) < 0.1 and abs(sig - want_sigma) < 0.1, (mu, want_mu, sig, want_sigma)


def test_symmetric_cauchy_walk_on_the_scalar_normal_model(mhx, real):
    """test/runtests.jl:215-259 with RandomWalkProposal{true}(TDist(1)) of :266-271: Normal(5, 0.7), mean and std within 0.05"""
    model = mhx.DensityModel(mhx.HipLogDensity(user_targets.SHIFTED_GAUSS, 1, [5.0, 0.7]))
    spl = mhx.MetropolisHastings(mhx.SymmetricRandomWalkProposal(mhx.TDist(1)))
    chain = mhx.sample(model, spl, 600, 2048, seed=12, discard_initial=200, initial_params=np.zeros(1), param_names=["x"])
    assert chain.stats["kernel_variant"] == KF_FAMILY
    x = chain["x"].astype(np.float64)
    print("mean %.4f std %.4f acceptance %.3f" % (x.mean(), x.std(), chain.accepted.mean()))
    assert abs(x.mean() - 5.0) < 0.05 and abs(x.std() - 0.7) < 0.05, (x.mean(), x.std())


def test_refusals(mhx, real):
    model = mhx.DensityModel(mhx.IsoGaussian(2))
    spl = mhx.RWMH([mhx.Laplace(0, 0.3), mhx.Normal(0, 1)])
    with pytest.raises(mhx.ArgumentError, match="ZIGGURAT"):
        mhx.Run(model, spl, nchains=8, normal_gen="ziggurat")
    with pytest.raises(mhx.ArgumentError, match="reduce_lanes"):
        mhx.Run(model, spl, nchains=8, reduce_lanes=2)
    run = mhx.Run(model, spl, nchains=8)
    run.init(None)
    with pytest.raises(mhx.ArgumentError, match="moments"):
        run.sample(10, 0, 1, 0, save="moments")
    run.sample(3, 0, 1, 0)                                                  # the run is still usable
    run.close()
    with pytest.raises(mhx.ArgumentError, match="dimension"):            # three components for a two-parameter model
        mhx.Run(model, mhx.RWMH([mhx.Laplace(), mhx.Laplace(), mhx.Normal(0, 1)]), nchains=8)
    # the C entry itself: a component count that is not dim, bad parameters, an unknown family
    import ctypes as C
    import mhx._lib as L
    ctx = L.Context.default()

    def create(rows, dim=2, flags=0):
        tab = (L.ProposalComponent * len(rows))(*[L.ProposalComponent(f, 0, a, b) for f, a, b in rows])
        cfg = L.RwmhCfg(dim, 8, 1, 0, 0, 1.0, None, flags, None, 0)
        h = C.c_void_p()
        L.check(L.lib().mhx_rwmh_create_components(ctx.h, model.handle(ctx), C.byref(cfg), tab, len(rows), C.byref(h)))
        L.lib().mhx_run_destroy(h)

    create([(2, 0.0, 0.3), (0, 0.0, 1.0)])
    with pytest.raises(mhx.ArgumentError, match="components"):
        create([(2, 0.0, 0.3)])
    for rows in ([(2, 0.0, 0.0), (0, 0.0, 1.0)], [(1, 1.0, 1.0), (0, 0.0, 1.0)], [(5, -1.0, 1.0), (0, 0.0, 1.0)], [(6, 2.0, 0.0), (0, 0.0, 1.0)],
                 [(4, 0.0, 0.0), (0, 0.0, 1.0)], [(3, math.nan, 1.0), (0, 0.0, 1.0)], [(0, 0.0, math.inf), (0, 0.0, 1.0)]):
        with pytest.raises(mhx.ArgumentError, match="needs"):
            create(rows)
    with pytest.raises(mhx.ArgumentError, match="unknown family"):
        create([(7, 0.0, 1.0), (0, 0.0, 1.0)])
