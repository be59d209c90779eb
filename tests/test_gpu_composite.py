"""GPU: Metropolis-Hastings runs under a COMPOSITE proposal -- a list of proposals or mhx.NamedProposals whose entries mix kinds,
shapes, symmetric flags and functions of their own slice (kernel variant 15) -- against the test-side restatement of the arithmetic
spec (tests/composite_restatement.py), bit for bit; one block against the runs of variants 14 and 13; the spellings against each
other; the initial draw; shards and resume; a known answer; refusals.
Reference behaviour under test: src/proposal.jl:128-175,198-240; src/mh-core.jl:92-117; README.md:92-117."""
import ctypes as C

import numpy as np
import pytest

import cases
import composite_helpers as H
import composite_restatement as CR
import conditional_restatement as R
import family_restatement as F

pytestmark = pytest.mark.gpu

KF_FAMILY, KF_COND, KF_COMPOSITE = 13, 14, 15


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    assert a.dtype == b.dtype, "%s: dtypes %s / %s" % (what, a.dtype, b.dtype)
    bad = np.argwhere(cases.bits(a) != cases.bits(b))
    assert len(bad) == 0, "%s: %d mismatches, first at %s: %r vs %r" % (what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


def _run(mhx, model, spl, C_, N, seed, first_chain=0, flags=0, init=None, ctx=None):
    run = mhx.Run(model, spl, nchains=C_, seed=seed, first_chain=first_chain, flags=flags, ctx=ctx)
    run.init(init)
    run.sample(N, 0, 1, 0)
    value, acc = run.samples()
    return run, value, acc


def _flags(mhx, form):
    return mhx.FLAG_GENERIC if form == "generic" else 0


def _ran_as(run, form):
    """both forms report kernel variant 15 and give the same chain: mhx_stats.register_form says which one stepped the run"""
    st = run.stats()
    assert st["kernel_variant"] == KF_COMPOSITE and st["reduce_lanes"] == 1
    assert st["register_form"] == (0 if form == "generic" else 1), (form, st["register_form"])


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit-exact against the restatement
_restated = {}


def _variant(name, variant):
    d, pos, entries = CR.CASES[name]
    if variant == "walk":
        entries = CR.with_kinds(entries, False)
    elif variant == "static":
        entries = CR.with_kinds(entries, True)
    elif variant == "symmetric laplace":
        entries = CR.with_symmetric(entries, 2, True)
    return d, pos, entries


def _restatement(oracle, real, name, variant="own"):
    key = (real, name, variant)
    if key not in _restated:
        d, pos, entries = _variant(name, variant)
        _restated[key] = CR.run_case(oracle, entries, d, pos)
    return _restated[key]


def _compare(mhx, ref, spl, d, pos, form):
    run, value, acc = _run(mhx, mhx.DensityModel(mhx.IsoGaussian(d)), spl, CR.C, CR.N, CR.seed_of(d), CR.FIRST_CHAIN, _flags(mhx, form),
                           CR.init_of(d, pos))
    _ran_as(run, form)
    _same(value, ref["samples"], "samples")
    _same(acc, ref["accepted"], "accepted")
    x, lp, cnt = run.state()
    _same(x, ref["final_x"], "final x")
    _same(lp, ref["final_lp"], "final lp")
    _same(cnt, ref["accept_counts"], "accept counts")
    assert run.stats()["accepted"] == int(ref["accept_counts"].sum())
    run.close()


@pytest.mark.parametrize("form", ["register", "generic"])
@pytest.mark.parametrize("name", list(CR.CASES))
def test_composite_runs_bit_exact_against_the_restatement(mhx, oracle, real, name, form):
    """Cases A and B x {register form, state-in-HBM form}: samples, accept flags, final state and counts equal the restatement's.
    What keeps a case from hiding a failure is asserted too: some transitions are accepted and some rejected, and the same
    components with every block forced to a walk (never accepts: the one-sided families give -Inf) or to static give other chains
    -- a kernel that ignored the kinds would not pass."""
    d, pos, entries = CR.CASES[name]
    ref = _restatement(oracle, real, name)
    total = int(ref["accept_counts"].sum())
    print("case %s [%s]: %d of %d accepted" % (name, real, total, CR.C * (CR.N - 1)))
    assert 0 < total < CR.C * (CR.N - 1)
    for variant in ("walk", "static"):
        other = _restatement(oracle, real, name, variant)
        assert not np.array_equal(cases.bits(other["samples"]), cases.bits(ref["samples"])), "the kinds do not matter in this case"
    _compare(mhx, ref, H.list_sampler(mhx, entries), d, pos, form)


@pytest.mark.parametrize("form", ["register", "generic"])
def test_a_symmetric_flag_on_the_mapped_block_changes_the_chain_and_is_matched(mhx, oracle, real, form):
    """case A with its Laplace block declared symmetric: its K and Z leave the ratio, p(y) is still evaluated and checked"""
    d, pos, entries = _variant("A", "symmetric laplace")
    ref, own = _restatement(oracle, real, "A", "symmetric laplace"), _restatement(oracle, real, "A")
    assert not np.array_equal(cases.bits(own["samples"]), cases.bits(ref["samples"]))
    assert 0 < int(ref["accept_counts"].sum()) < CR.C * (CR.N - 1)
    _compare(mhx, ref, H.list_sampler(mhx, entries), d, pos, form)


# ---------------------------------------------------------------------------------------------------------------------
# 2. degenerate forms: one block is the conditional run, constant blocks of one kind are the component run
@pytest.mark.parametrize("form", ["register", "generic"])
@pytest.mark.parametrize("static", [False, True], ids=["walk", "static"])
def test_one_block_reproduces_the_conditional_run(mhx, real, static, form):
    d, pmap, init = R.CASES["b_cross_coordinates"]
    fn = lambda x: H.dists(mhx, pmap(H.tracing_namespace(mhx), x))
    P = mhx.StaticProposal if static else mhx.RandomWalkProposal
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    r0, v0, a0 = _run(mhx, model, mhx.MetropolisHastings(P(fn, dim=d)), 200, 30, 99, 7, _flags(mhx, form), init(200))
    r1, v1, a1 = _run(mhx, model, mhx.MetropolisHastings([P(fn, dim=d)]), 200, 30, 99, 7, _flags(mhx, form), init(200))
    assert r0.stats()["kernel_variant"] == KF_COND and r0.stats()["register_form"] == r1.stats()["register_form"]
    _ran_as(r1, form)
    _same(v1, v0, "samples")
    _same(a1, a0, "accepted")
    assert 0 < a0[1:].mean() < 1
    for got, want, what in zip(r1.state(), r0.state(), ("x", "lp", "accept counts")):
        _same(got, want, what)
    r0.close(), r1.close()


@pytest.mark.parametrize("form", ["register", "generic"])
def test_constant_walk_blocks_reproduce_the_component_run(mhx, real, form):
    RW = mhx.RandomWalkProposal
    model = mhx.DensityModel(mhx.IsoGaussian(3))
    init = np.random.default_rng(3).normal(size=(3, 200))
    whole = mhx.MetropolisHastings(RW([mhx.Normal(0, 1), mhx.Laplace(0, 2), mhx.Cauchy(0, 0.5)]))
    parts = mhx.MetropolisHastings([RW([mhx.Normal(0, 1), mhx.Laplace(0, 2)]), RW(mhx.Cauchy(0, 0.5))])
    r0, v0, a0 = _run(mhx, model, whole, 200, 30, 99, 7, _flags(mhx, form), init)
    r1, v1, a1 = _run(mhx, model, parts, 200, 30, 99, 7, _flags(mhx, form), init)
    assert r0.stats()["kernel_variant"] == KF_FAMILY
    _ran_as(r1, form)
    _same(v1, v0, "samples")
    _same(a1, a0, "accepted")
    assert 0 < a0[1:].mean() < 1
    r0.close(), r1.close()


def test_the_register_rule_decides_the_form_and_the_forms_agree_at_its_limit(mhx, real):
    """NamedProposals of d scalar function entries, Cauchy(0.01 x, 0.1 + 0.05 |x|): every component mapped and a block of its own.
    d = 17 is the largest such shape the fp64 rule admits (2 d + d + d / 2 <= 60): the register form, and the same bytes as the
    state-in-HBM form; d = 28 is outside the rule in both widths (98 > 96) and runs the state-in-HBM form by itself."""
    def spl(d):
        return mhx.MetropolisHastings(mhx.NamedProposals(**{"p%d" % k: mhx.RandomWalkProposal(
            lambda x: mhx.Cauchy(0.01 * x, 0.1 + 0.05 * abs(x)), dim=1) for k in range(d)}))
    d = 17
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    init = np.random.default_rng(8).normal(size=(d, 130))
    r0, v0, a0 = _run(mhx, model, spl(d), 130, 20, 5, 0, 0, init)
    r1, v1, a1 = _run(mhx, model, spl(d), 130, 20, 5, 0, mhx.FLAG_GENERIC, init)
    _ran_as(r0, "register"), _ran_as(r1, "generic")
    _same(v0, v1, "samples")
    _same(a0, a1, "accepted")
    assert 0 < a0[1:].mean() < 1
    r0.close(), r1.close()
    d = 28
    r2, v2, a2 = _run(mhx, mhx.DensityModel(mhx.IsoGaussian(d)), spl(d), 70, 5, 5, 0, 0, np.zeros((d, 70)))
    _ran_as(r2, "generic")
    r2.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. locality and the named spelling
def test_named_entries_see_their_own_slice_and_give_the_lists_chain(mhx, oracle, real):
    seen = []

    def b(x):                                                   # the entry's own two parameters, whatever comes before it
        seen.append(("b", len(x)))
        return [mhx.Normal(0.25 * x[1], 0.5 + abs(x[0])), mhx.Laplace(0, 0.5 + abs(x[1]))]

    def c(x):                                                   # a scalar entry gets a scalar
        seen.append(("c", isinstance(x, mhx.trace.Sym)))
        return mhx.Cauchy(0, 0.25 + 0.1 * abs(x))
    spl = mhx.MetropolisHastings(mhx.NamedProposals(a=mhx.StaticProposal([mhx.Normal(0, 1), mhx.Normal(0, 2), mhx.Normal(0, 1)]),
                                                    b=mhx.RandomWalkProposal(b, dim=2), c=mhx.RandomWalkProposal(c, dim=1)))
    assert set(seen) == {("b", 2), ("c", True)}
    assert spl.param_names == ["a[1]", "a[2]", "a[3]", "b[1]", "b[2]", "c"]
    chain = mhx.sample(mhx.DensityModel(mhx.IsoGaussian(6)), spl, 20, 64, seed=3, initial_params=np.zeros(6))
    assert chain.stats["kernel_variant"] == KF_COMPOSITE and chain.names == spl.param_names + ["lp"]
    assert chain["b[2]"].shape == (20, 64) and 0 < chain.accepted[1:].mean() < 1 and np.isfinite(chain.value).all()
    # case A, named: the chain of the list spelling (and of the restatement)
    d, pos, entries = CR.CASES["A"]
    _compare(mhx, _restatement(oracle, real, "A"), H.named_sampler(mhx, entries), d, pos, "register")


# ---------------------------------------------------------------------------------------------------------------------
# 4. the initial draw
def test_a_constant_composite_draws_its_first_state_like_the_component_run(mhx, oracle, real):
    RW, ST = mhx.RandomWalkProposal, mhx.StaticProposal
    comps = [(F.NORMAL, 0.0, 1.0), (F.LAPLACE, 0.0, 2.0), (F.INVERSE_GAMMA, 2.0, 3.0), (F.CAUCHY, 0.0, 0.5)]
    model = mhx.DensityModel(mhx.IsoGaussian(4))
    spl = mhx.MetropolisHastings([RW([mhx.Normal(0, 1), mhx.Laplace(0, 2)]), ST(mhx.InverseGamma(2, 3)), RW(mhx.Cauchy(0, 0.5))])
    r1, v1, a1 = _run(mhx, model, spl, 70, 8, 41, 5)
    r0, v0, a0 = _run(mhx, model, mhx.MetropolisHastings(RW(H.dists(mhx, comps))), 70, 1, 41, 5)
    assert r1.stats()["kernel_variant"] == KF_COMPOSITE and r0.stats()["kernel_variant"] == KF_FAMILY
    _same(v1[0], v0[0], "sample 1: the initial draw")
    ref = CR.run(oracle.iso_gauss(4), lambda m, x: comps, 4, [(0, 2, False, False), (2, 1, True, False), (3, 1, False, False)], 8, 41, 5, 70)
    _same(v1, ref["samples"], "samples")
    _same(a1, ref["accepted"], "accepted")
    assert 0 < int(ref["accept_counts"].sum()) < 70 * 7
    r0.close(), r1.close()
    # with a map there is no distribution to draw from
    import mhx._lib as L
    d, pos, entries = CR.CASES["A"]
    run = mhx.Run(mhx.DensityModel(mhx.IsoGaussian(d)), H.list_sampler(mhx, entries), nchains=8)
    with pytest.raises(mhx.ArgumentError, match="initial_params"):
        run.init(None)
    with pytest.raises(mhx.ArgumentError, match="initial_params"):                   # the C entry itself
        L.check(L.lib().mhx_run_init(run.h, None))
    run.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. shards and resume are the whole run
@pytest.mark.parametrize("form", ["register", "generic"])
def test_shards_and_resume_are_the_whole_run(mhx, real, form):
    flags = _flags(mhx, form)
    d, pos, entries = CR.CASES["B"]
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = H.list_sampler(mhx, entries)
    Cn, N = 70, 41
    init = CR.init_of(d, pos, Cn)
    whole, value, acc = _run(mhx, model, spl, Cn, N, 31, 1000, flags, init)
    a, va, aa = _run(mhx, model, spl, 30, N, 31, 1000, flags, init[:, :30])
    b, vb, ab = _run(mhx, model, spl, Cn - 30, N, 31, 1030, flags, init[:, 30:])
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
    _ran_as(whole, form)
    assert 0 < acc[1:].mean() < 1
    second.close(), whole.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. known answer
def test_readme_model_under_a_walk_on_mu_and_a_static_proposal_on_sigma(mhx, real):
    """The README's model (30 points, default_rng(1234)) under NamedProposals(mu = RandomWalkProposal(Normal(0, .5)), sigma =
    StaticProposal(InverseGamma(2, 3))), the proposal of the reference's README.md:100-117 with one entry a walk: 4096 chains x 1000
    recorded after 200 discarded.  With the flat prior the posterior has E[mu] = ybar and the sigma-marginal
    sigma^-(n-1) exp(-S / 2 sigma^2), S = sum (y - ybar)^2; E[sigma] by quadrature.  Both within 0.1, the tolerance of the
    reference's own tests.  (A float64 numpy simulation of this sampler: 0.0271 / 1.1809 against 0.0268 / 1.1810, acceptance 0.114.)"""
    data = np.random.default_rng(1234).normal(size=30)
    n, ybar = data.size, data.mean()
    S = ((data - ybar) ** 2).sum()
    s = np.linspace(0.3, 6.0, 200001)
    w = np.exp(-(n - 1) * np.log(s) - S / (2 * s * s))
    want_sigma = float((s * w).sum() / w.sum())
    spl = mhx.MetropolisHastings(mhx.NamedProposals(mu=mhx.RandomWalkProposal(mhx.Normal(0, 0.5)), sigma=mhx.StaticProposal(mhx.InverseGamma(2, 3))))
    chain = mhx.sample(mhx.DensityModel(mhx.IIDNormal(data)), spl, 1000, 4096, seed=12, discard_initial=200, initial_params=np.array([0.0, 1.0]))
    assert chain.stats["kernel_variant"] == KF_COMPOSITE and chain.names == ["mu", "sigma", "lp"]
    mu, sigma = chain["mu"].astype(np.float64).mean(), chain["sigma"].astype(np.float64).mean()
    print("E[mu] %.4f (ybar %.4f)  E[sigma] %.4f (quadrature %.4f)  acceptance %.3f" % (mu, ybar, sigma, want_sigma, chain.accepted[1:].mean()))
    assert abs(mu - ybar) < 0.1 and abs(sigma - want_sigma) < 0.1, (mu, ybar, sigma, want_sigma)


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals of the C entry and of Run
def test_refusals(mhx, real):
    import mhx._lib as L
    lib = L.lib()
    model = mhx.DensityModel(mhx.IsoGaussian(3))
    RW, ST = mhx.RandomWalkProposal, mhx.StaticProposal
    spl = mhx.MetropolisHastings([RW(lambda x: [mhx.Normal(0, 0.5 + abs(x[1])), mhx.Laplace(0, 0.5 + abs(x[0]))], dim=2), ST(mhx.Normal(0, 1))])
    ok_init = np.zeros((3, 8))

    def later_valid_run():
        run = mhx.Run(model, spl, nchains=8, seed=1)
        run.init(ok_init)
        run.sample(5, 0, 1, 0)
        assert run.stats()["kernel_variant"] == KF_COMPOSITE
        run.close()

    later_valid_run()
    with pytest.raises(mhx.ArgumentError, match="NO_JIT"):
        mhx.Run(model, spl, nchains=8, flags=mhx.FLAG_NO_JIT)
    with pytest.raises(mhx.ArgumentError, match="ZIGGURAT"):
        mhx.Run(model, spl, nchains=8, normal_gen="ziggurat")
    with pytest.raises(mhx.ArgumentError, match="reduce_lanes"):
        mhx.Run(model, spl, nchains=8, reduce_lanes=2)
    with pytest.raises(mhx.ArgumentError, match="blocks carry"):
        mhx.Run(model, spl, nchains=8, flags=mhx.FLAG_SYMMETRIC_PROPOSAL)
    with pytest.raises(mhx.ArgumentError, match="blocks carry"):
        mhx.Run(model, spl, nchains=8, flags=L.MHX_FLAG_STATIC_PROPOSAL)
    run = mhx.Run(model, spl, nchains=8)
    run.init(ok_init)
    with pytest.raises(mhx.ArgumentError, match="moments"):
        run.sample(10, 0, 1, 0, save="moments")
    run.sample(3, 0, 1, 0)                                                            # the run is still usable
    run.close()
    # the C entry: blocks that do not tile 0 .. dim-1 in order, unknown flags, reserved, masks and sources that do not go together
    ctx = L.Context.default()
    tab = (L.ProposalComponent * 3)(L.ProposalComponent(0, 0, 0.0, 1.0), L.ProposalComponent(5, 0, 2.0, 1.0), L.ProposalComponent(2, 0, 0.0, 1.0))
    cfg = L.RwmhCfg(3, 8, 1, 0, 0, 1.0, None, 0, None, 0)
    src = b"MHX_PROPOSAL_PARAMS(x, p, d, data, ndata) { p.set(0, 1, MHX_R(0.5) + mhx_abs(x[0])); }\n"
    h = C.c_void_p()

    def create(blocks, mapped=None, source=None):
        blk = (L.ProposalBlock * len(blocks))(*[L.ProposalBlock(*b) for b in blocks])
        mk = None if mapped is None else (C.c_int32 * 3)(*mapped)
        return lib.mhx_rwmh_create_composite(ctx.h, model.handle(ctx), C.byref(cfg), tab, 3, blk, len(blocks), mk, source, None, 0, C.byref(h))
    for blocks in ([(0, 2, 0, 0)], [(0, 2, 0, 0), (1, 2, 0, 0)], [(1, 2, 0, 0), (0, 1, 0, 0)], [(0, 2, 0, 0), (2, 2, 0, 0)], [(0, 0, 0, 0), (0, 3, 0, 0)],
                   [(0, 1, 0, 0), (2, 1, 0, 0)]):
        assert create(blocks) == L.MHX_EINVAL and b"tile" in lib.mhx_last_error(), blocks
    assert create([(0, 3, 4, 0)]) == L.MHX_EINVAL and b"flags" in lib.mhx_last_error()
    assert create([(0, 3, 0, 1)]) == L.MHX_EINVAL and b"reserved" in lib.mhx_last_error()
    assert create([(0, 3, 0, 0)], [2, 0, 0], None) == L.MHX_EINVAL and b"without params_src" in lib.mhx_last_error()
    assert create([(0, 3, 0, 0)], [2, 0, 0], b"") == L.MHX_EINVAL
    assert create([(0, 3, 0, 0)], None, src) == L.MHX_EINVAL and b"without a mapped" in lib.mhx_last_error()
    assert create([(0, 3, 0, 0)], [0, 0, 0], src) == L.MHX_EINVAL
    assert create([(0, 3, 0, 0)], [2, 1, 0], src) == L.MHX_EINVAL and b"shape" in lib.mhx_last_error()        # a mapped Gamma shape
    assert create([(0, 3, 0, 0)], [4, 0, 0], src) == L.MHX_EINVAL
    bad = src.replace(b"x[0])); }", b"x[0]) }")
    assert create([(0, 3, 0, 0)], [2, 0, 0], bad) == L.MHX_EJIT and b"proposal_params.hip" in lib.mhx_last_error()
    L.check(create([(0, 1, 0, 0), (1, 2, 3, 0)], [2, 0, 0], src))
    lib.mhx_run_destroy(h)
    L.check(create([(0, 3, 1, 0)], None, b""))                                        # nothing mapped: "" is NULL
    lib.mhx_run_destroy(h)
    later_valid_run()
    # initial states at which the map gives no distribution: Normal(0, x) at x <= 0 (one chain of eight)
    worse = mhx.MetropolisHastings([ST(mhx.Normal(0, 1)), RW(lambda x: mhx.Normal(0, x), dim=1), RW(mhx.Normal(0, 1), issymmetric=True)])
    run = mhx.Run(model, worse, nchains=8)
    init = np.ones((3, 8))
    init[1, 5] = -1.0
    with pytest.raises(mhx.ArgumentError, match="1 of 8 chains"):
        run.init(init)
    with pytest.raises(mhx.MhxError):                                                # not initialised: nothing to sample
        run.sample(3, 0, 1, 0)
    run.init(np.ones((3, 8)))
    run.sample(3, 0, 1, 0)
    with pytest.raises(mhx.ArgumentError, match="1 of 8 chains"):                    # set_params
        run.set_params(init)
    run.close()
    later_valid_run()
