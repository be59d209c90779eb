"""GPU: adaptive random-walk runs (mhx_rwmh_create_adaptive, kernel variant 19) against the test-side restatement of the arithmetic spec
(tests/adaptive_rwmh_restatement.py), bit for bit, in both widths and both kernel forms; the invariances a chain
keeps while it adapts (two calls == one with the seam before, at and after adapt_steps; shards; lp == the target at x; frozen after
adapt_steps; adapt_steps = 0 and c = 0 are the plain run); the refusals; the Python mirror; and the tuning claim on the device's run."""
import ctypes as C

import numpy as np
import pytest

import cases
import test_adaptive_rwmh_cpu as CPU

pytestmark = pytest.mark.gpu

KF_ADAPTIVE = 19
S = CPU.SCHEDULE


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    assert a.dtype == b.dtype, "%s: dtypes %s / %s" % (what, a.dtype, b.dtype)
    bad = np.argwhere(cases.bits(a) != cases.bits(b))
    assert len(bad) == 0, "%s: %d mismatches, first at %s: %r vs %r" % (what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


def _mv(mhx, kind, sigma, d):
    if kind == "iso":
        mv = mhx.MvNormal(mhx.zeros(d), (sigma ** 2) * mhx.I)
        assert mv.kind == 0 and mv.scale == sigma
    else:
        mv = mhx.MvNormal(mhx.zeros(d), np.asarray(sigma, dtype=np.float64) ** 2)
        assert mv.kind == 1 and (np.asarray(mv.vec, dtype=np.float64) == np.asarray(sigma)).all()
    return mv


def _narrow(run, real):
    """proposal_state in the run's width: the widening is exact, so the narrowing gives the device's bits back"""
    ps = run.proposal_state()
    T = np.float32 if real == "f32" else np.float64
    out = {}
    for key in ("lam", "sd", "mean"):
        out[key] = ps[key].astype(T)
        assert (cases.bits(out[key].astype(np.float64)) == cases.bits(ps[key])).all(), key
    out["acc_at_freeze"] = ps["acc_at_freeze"]
    return out


def _forms(form, adapting_fits=True, frozen_fits=True):
    if form == "generic":
        return "adaptive_generic", "adaptive_frozen_generic"
    return ("adaptive_reg" if adapting_fits else "adaptive_generic"), ("adaptive_frozen_reg" if frozen_fits else "adaptive_frozen_generic")


def _check_against(mhx, oracle, real, name, form):
    c = CPU.parity_case(name, real)
    ref = CPU.restated(mhx, oracle, name, real)
    model, _ = CPU.parity_model_and_target(mhx, oracle, c)
    spl = mhx.RWMH(_mv(mhx, c["kind"], c["sigma"], c["d"]), adapt=mhx.ProposalAdaptation(S["adapt_steps"], shape=c["shape"]))
    run = mhx.Run(model, spl, nchains=c["n"], seed=c["seed"], first_chain=c["first"], flags=mhx.FLAG_GENERIC if form == "generic" else 0)
    run.init()
    lim = CPU.register_limits(real)
    adapting, frozen = _forms(form, c["d"] <= (lim[1] if c["shape"] else lim[0]), c["d"] <= lim[2])
    # before any transition: the configured sds themselves, lam = 0, the mean at the first state, and the adapting phase's form
    ps = _narrow(run, real)
    s = np.asarray(CPU.parity_sigma(oracle, c), dtype=oracle.real()) * np.ones(c["d"], dtype=oracle.real())
    _same(ps["sd"], np.repeat(s[:, None], c["n"], axis=1), "sd after init")
    assert (ps["lam"] == 0).all() and (ps["acc_at_freeze"] == 0).all()
    if c["shape"]:
        _same(ps["mean"], run.state()[0], "mean after init")
    else:
        assert np.isnan(ps["mean"]).all()
    assert run.form_name() == adapting and run.stats()["register_form"] == (1 if adapting == "adaptive_reg" else 0)
    run.sample(S["N"], S["discard"], S["thinning"], 0)
    st = run.stats()
    assert st["kernel_variant"] == KF_ADAPTIVE and st["reduce_lanes"] == 1
    assert st["launches"] == 2                                 # one launch per phase: the schedule is split at the seam
    assert run.form_name() == frozen and st["register_form"] == (1 if frozen == "adaptive_frozen_reg" else 0)
    value, acc = run.samples()
    _same(value, ref["samples"], "samples")
    _same(acc, ref["accepted"], "accepted")
    x, lp, cnt = run.state()
    _same(x, ref["final_x"], "final x")
    _same(lp, ref["final_lp"], "final lp")
    _same(cnt, ref["accept_counts"], "accept counts")
    ps = _narrow(run, real)
    _same(ps["lam"], ref["lam"], "lam")
    _same(ps["sd"], ref["sd"], "sd")
    _same(ps["mean"], ref["mean"], "mean")
    _same(ps["acc_at_freeze"], ref["acc_at_freeze"], "acc_at_freeze")
    assert st["accepted"] == int(ref["accept_counts"].sum())
    # lp of every chain is the target at its x
    _same(mhx.logdensity(model, x), lp, "lp == target(x)")
    run.close()


@pytest.mark.parametrize("form", ["register", "generic"])
@pytest.mark.parametrize("name", sorted(CPU.PARITY))
def test_adaptive_runs_bit_exact_against_the_restatement(mhx, oracle, real, name, form):
    _check_against(mhx, oracle, real, name, form)


def test_above_the_register_limit_the_adapting_phase_runs_from_hbm(mhx, oracle, real):
    """d = the limit of the adapting register form with shape + 4: the run reports adaptive_generic while it adapts and
    adaptive_frozen_reg afterwards (that phase has its own, larger limit), and is the restated run"""
    _check_against(mhx, oracle, real, "above_the_register_limit", "register")


def _setup(mhx, d=3, adapt_steps=10, shape=True, kind="diag", **kw):
    model = mhx.DensityModel(mhx.CorrGaussian(np.diag([0.04, 1.0, 9.0, 0.25, 2.25][:d])))
    mv = _mv(mhx, kind, 0.7 if kind == "iso" else [0.3, 1.7, 0.9, 2.4, 0.6][:d], d)
    return model, mhx.RWMH(mv, adapt=mhx.ProposalAdaptation(adapt_steps, shape=shape, **kw))


def _run(mhx, model, spl, n, seed, first=0, flags=0):
    run = mhx.Run(model, spl, nchains=n, seed=seed, first_chain=first, flags=flags)
    run.init()
    return run


def _same_state(a, b, real):
    for u, v in zip(a.state(), b.state()):
        _same(u, v, "final state")
    pa, pb = _narrow(a, real), _narrow(b, real)
    for key in pa:
        _same(pa[key], pb[key], key)


@pytest.mark.parametrize("seam", ["before adapt_steps", "at adapt_steps", "after adapt_steps"])
@pytest.mark.parametrize("form", ["register", "generic"])
def test_two_sample_calls_equal_one(mhx, real, form, seam):
    """7 + 13 samples in two calls == 19 in one; the first call ends after transition 6: with adapt_steps = 10 inside the adaptation
    (lam, m, v, sig and eff cross the seam in memory), with 6 exactly at its end, with 3 after it (the first call holds the seam)"""
    n, seed = 70, 0xAD31
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    steps = {"before adapt_steps": 10, "at adapt_steps": 6, "after adapt_steps": 3}[seam]
    model, spl = _setup(mhx, adapt_steps=steps)
    one = _run(mhx, model, spl, n, seed, flags=flags)
    one.sample(19, 0, 1, 0)
    v1, a1 = one.samples()
    two = _run(mhx, model, spl, n, seed, flags=flags)
    two.sample(7, 0, 1, 0)
    va, aa = two.samples()
    mid = _narrow(two, real)
    two.sample(13, 0, 1, 0)
    vb, ab = two.samples()
    _same(va, v1[:7], "first call")
    _same(vb, v1[6:], "second call")
    _same(aa, a1[:7], "accepted, first call")
    _same(ab, a1[6:], "accepted, second call")
    _same_state(one, two, real)
    end = _narrow(two, real)
    if seam == "before adapt_steps":
        assert (mid["sd"] != end["sd"]).any() and (mid["acc_at_freeze"] == 0).all() and (end["acc_at_freeze"] > 0).any()
    else:
        for key in mid:
            _same(mid[key], end[key], "frozen at the seam: " + key)
    one.close(), two.close()


@pytest.mark.parametrize("form", ["register", "generic"])
def test_a_shard_equals_the_matching_columns_of_the_larger_run(mhx, real, form):
    seed, N = 0xAD32, 16
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    model, spl = _setup(mhx, d=5, adapt_steps=11)
    whole = _run(mhx, model, spl, 128, seed, flags=flags)
    whole.sample(N, 0, 1, 0)
    vw, aw = whole.samples()
    shard = _run(mhx, model, spl, 64, seed, first=64, flags=flags)
    shard.sample(N, 0, 1, 0)
    vs, as_ = shard.samples()
    _same(vs, vw[:, :, 64:], "shard samples")
    _same(as_, aw[:, 64:], "shard accepted")
    pw, psh = _narrow(whole, real), _narrow(shard, real)
    for key in ("lam", "acc_at_freeze"):
        _same(psh[key], pw[key][64:], key)
    for key in ("sd", "mean"):
        _same(psh[key], pw[key][:, 64:], key)
    assert len(np.unique(pw["lam"])) > 64                      # every chain went its own way
    whole.close(), shard.close()


@pytest.mark.parametrize("form", ["register", "generic"])
def test_the_proposal_is_frozen_after_adapt_steps(mhx, real, form):
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    model, spl = _setup(mhx, adapt_steps=10)
    run = _run(mhx, model, spl, 70, 0xAD33, flags=flags)
    run.sample(1, 10, 1, 0)                                    # transitions 1 .. adapt_steps
    at = _narrow(run, real)
    cnt = run.state()[2]
    _same(at["acc_at_freeze"], cnt, "the counters at the seam")
    run.sample(1, 5, 1, 0)                                     # ... adapt_steps + 5
    after = _narrow(run, real)
    for key in at:
        _same(at[key], after[key], key)
    assert (run.state()[2] > cnt).any()
    run.close()


@pytest.mark.parametrize("kind", ["iso", "diag"])
@pytest.mark.parametrize("form", ["register", "generic"])
@pytest.mark.parametrize("how", ["adapt_steps = 0", "c = 0"])
def test_a_run_that_never_moves_its_proposal_is_the_plain_run(mhx, real, form, kind, how):
    """adapt_steps = 0 (shape on: nothing of it ever runs) and c = 0 with shape off (lam stays 0, exp(0) = 1) give the plain run's
    samples, accepts and state: the proposal's standard deviations are the configured ones themselves"""
    d, n, seed, N = 3, 70, 0xAD34, 14
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    kw = dict(adapt_steps=0, shape=True) if how == "adapt_steps = 0" else dict(adapt_steps=9, shape=False, c=0.0)
    model, spl = _setup(mhx, d=d, kind=kind, **kw)
    run = _run(mhx, model, spl, n, seed, first=5, flags=flags)
    run.sample(N, 2, 3, 0)
    plain = _run(mhx, model, mhx.RWMH(spl.proposal.proposal), n, seed, first=5, flags=flags)
    assert plain.stats()["kernel_variant"] != KF_ADAPTIVE
    plain.sample(N, 2, 3, 0)
    for (a, b), what in zip(zip(run.samples(), plain.samples()), ("samples", "accepted")):
        _same(a, b, what)
    for a, b in zip(run.state(), plain.state()):
        _same(a, b, "final state")
    ps = run.proposal_state()
    assert (ps["lam"] == 0).all()
    s = np.full(d, 0.7) if kind == "iso" else np.array([0.3, 1.7, 0.9])
    T = np.float32 if real == "f32" else np.float64
    assert (ps["sd"] == s.astype(T).astype(np.float64)[:, None]).all()
    run.close(), plain.close()


def _refused(mhx, code, words, fn):
    with pytest.raises(mhx.MhxError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def test_refusals_name_their_rule(mhx, real):
    L = mhx._lib
    d = 2
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    iso = mhx.MvNormal(mhx.zeros(d), mhx.I)
    EINVAL, ESTATE = mhx.MHX_EINVAL, mhx.MHX_ESTATE
    nan = float("nan")
    sentinel = 0x5A5A5A5A

    def create(kind=0, scale=1.0, vec=None, mean=None, flags=0, lanes=0, steps=10, shape=0, target_rate=nan, c=nan, kappa=nan, lam_min=nan,
               lam_max=nan):
        """the C entry itself: the Python mirror refuses most of these before the library sees them.  A refusal leaves *out untouched."""
        ctx = L.Context.default()
        v = None if vec is None else ctx.arr(np.asarray(vec))
        m = None if mean is None else ctx.arr(np.asarray(mean))
        cfg = L.RwmhCfg(d, 8, 1, 0, kind, scale, L.fptr(v), flags, L.fptr(m), lanes)
        acfg = L.ProposalAdaptCfg(steps, shape, target_rate, c, kappa, lam_min, lam_max)
        h = C.c_void_p(sentinel)
        rc = L.lib().mhx_rwmh_create_adaptive(ctx.h, model.handle(ctx), C.byref(cfg), C.byref(acfg), C.byref(h))
        if rc != L.MHX_OK:
            assert h.value == sentinel, "a refusal wrote *out"
        L.check(rc)
        L.lib().mhx_run_destroy(h)
    create()                                                # the defaults are accepted
    create(c=0.0, kappa=1.0, steps=0, shape=1)
    create(kind=1, vec=[0.5, 2.0], mean=[0.0, 0.0])          # a zero mean is no mean
    me = "mhx_rwmh_create_adaptive"
    _refused(mhx, EINVAL, [me, "MHX_PROP_DENSE", "ISO or a DIAG"], lambda: create(kind=2, vec=[1.0, 0.0, 1.0]))
    _refused(mhx, EINVAL, [me, "a proposal mean", "zero-mean"], lambda: create(mean=[0.0, 0.5]))
    _refused(mhx, EINVAL, [me, "MHX_FLAG_STATIC_PROPOSAL", "random walk"], lambda: create(flags=L.MHX_FLAG_STATIC_PROPOSAL))
    _refused(mhx, EINVAL, [me, "MHX_FLAG_ZIGGURAT", "Box-Muller"], lambda: create(flags=mhx.FLAG_ZIGGURAT))
    _refused(mhx, EINVAL, [me, "reduce_lanes = 4", "one lane per chain"], lambda: create(lanes=4))
    _refused(mhx, EINVAL, [me, "adapt_steps = -1"], lambda: create(steps=-1))
    _refused(mhx, EINVAL, [me, "kappa = 0.5", "(0.5, 1]"], lambda: create(kappa=0.5))
    _refused(mhx, EINVAL, [me, "kappa = 1.5", "(0.5, 1]"], lambda: create(kappa=1.5))
    _refused(mhx, EINVAL, [me, "c = -1"], lambda: create(c=-1.0))
    _refused(mhx, EINVAL, [me, "target_rate = 0", "(0, 1)"], lambda: create(target_rate=0.0))
    _refused(mhx, EINVAL, [me, "target_rate = 1", "(0, 1)"], lambda: create(target_rate=1.0))
    _refused(mhx, EINVAL, [me, "lam_min", "lam_max"], lambda: create(lam_min=1.0, lam_max=0.0))
    tiny, huge = (1e-14, 1e14) if real == "f32" else (1e-150, 1e150)
    _refused(mhx, EINVAL, [me, "2^-40", "not a normal number"], lambda: create(scale=tiny, shape=1))
    _refused(mhx, EINVAL, [me, "2^40", "not finite"], lambda: create(kind=1, vec=[1.0, huge], shape=1))
    import user_targets
    user = mhx.DensityModel(mhx.HipLogDensity(user_targets.SHIFTED_GAUSS, d, [0.0, 0.0, 1.0, 1.0]))
    adapt = mhx.ProposalAdaptation(10, shape=True)

    def make(m=model, flags=0, ctx=None):
        return mhx.Run(m, mhx.RWMH(iso, adapt=adapt), nchains=8, seed=1, flags=flags, ctx=ctx)
    _refused(mhx, EINVAL, [me, "MHX_FLAG_NO_JIT", "user target"], lambda: make(m=user, flags=mhx.FLAG_NO_JIT))
    # a catalogue target without the run-time compiler: the pre-built state-in-HBM forms
    run = make(flags=mhx.FLAG_NO_JIT)
    assert run.form_name() == "adaptive_generic"
    run.init()
    run.sample(4, 12, 1, 0)
    assert run.form_name() == "adaptive_frozen_generic" and run.proposal_state()["acc_at_freeze"].sum() > 0
    _refused(mhx, ESTATE, ["MHX_SAVE_MOMENTS", "adaptive"], lambda: run.sample(4, save="moments"))
    _refused(mhx, ESTATE, ["mhx_run_sample_to_host", "adaptive"], lambda: run.sample_to_host(4))
    _refused(mhx, ESTATE, ["checkpoint", "adaptive"], lambda: run.save_state())
    _refused(mhx, ESTATE, ["checkpoint", "adaptive"], lambda: run.load_state(b"\0" * 128))
    g = mhx.Group([0])
    other = make(ctx=g.ctxs[0])
    _refused(mhx, ESTATE, ["mhx_group_attach", "adaptive"], lambda: g.attach([other]))
    g.close()
    plain = mhx.Run(model, mhx.RWMH(iso), nchains=8, seed=1)
    _refused(mhx, ESTATE, ["mhx_run_proposal_state", "not an adaptive run"], lambda: plain.proposal_state())
    plain.close(), run.close()


def test_sample_returns_a_chain_with_the_adaptation_table(mhx, real):
    d, n = 3, 70
    model, spl = _setup(mhx, d=d, adapt_steps=40)
    with pytest.raises(mhx.ArgumentError) as ei:
        mhx.sample(model, spl, 10, n, discard_initial=39, seed=3)
    assert "discard_initial = 39 < adapt.steps = 40" in str(ei.value)
    chain = mhx.sample(model, spl, 30, n, discard_initial=40, thinning=2, seed=3, param_names=["a", "b", "c"])
    run = chain.state
    assert run.stats()["kernel_variant"] == KF_ADAPTIVE and chain.value.shape == (30, d + 1, n)
    ps = run.proposal_state()
    t = chain.adaptation
    assert [w["parameter"] for w in t] == ["a", "b", "c"]
    for k, w in enumerate(t):
        assert w["sd_median"] == float(np.median(ps["sd"][k])) and w["sd_min"] == ps["sd"][k].min() and w["sd_max"] == ps["sd"][k].max()
    assert t.lam_median == float(np.median(ps["lam"]))
    frozen = 58                                               # 40 + 29 * 2 transitions, 40 of them adapting
    want = float((run.state()[2].astype(np.int64) - ps["acc_at_freeze"].astype(np.int64)).sum()) / (frozen * n)
    assert t.accept_rate == want and 0.0 < want < 1.0
    assert "median log-scale" in str(t) and "\nb " in str(t)
    # the same chains as the run driven by hand
    by_hand = _run(mhx, model, spl, n, 3)
    by_hand.sample(30, 40, 2, 0)
    _same(chain.value, by_hand.samples()[0], "sample() against Run.sample")
    by_hand.close()


def test_the_adaptation_tunes_the_proposal(mhx, oracle):
    """the tuning claim of DESIGN.md section 3.18 on the device's run, which is the restated run bit for bit: the same windows"""
    t = CPU.TUNING
    with CPU.in_f64(mhx, oracle):
        model = mhx.DensityModel(mhx.CorrGaussian(np.diag(np.square(t["sds"]))))
        spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(4), (t["s"] ** 2) * mhx.I), adapt=mhx.ProposalAdaptation(t["steps"], shape=True))
        run = _run(mhx, model, spl, t["n"], t["seed"])
        run.sample(1, t["steps"] + t["frozen"], 1, 0)
        ps = run.proposal_state()
        cnt = run.state()[2]
        CPU.check_tuning(ps["lam"], ps["sd"], cnt, ps["acc_at_freeze"])
        # the same proposal left fixed
        fixed = _run(mhx, model, mhx.RWMH(spl.proposal.proposal), t["n"], t["seed"])
        fixed.sample(1, t["steps"] + t["frozen"], 1, 0)
        rate = float(fixed.state()[2].sum()) / ((t["steps"] + t["frozen"]) * t["n"])
        print("fixed proposal: acceptance rate %.4f" % rate)
        assert rate < 0.15
        run.close(), fixed.close()
