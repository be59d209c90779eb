"""GPU: tempered runs whose ladders adapt (mhx_rwmh_create_tempered_adaptive, kernel variant 17) against the test-side restatement of
the arithmetic spec (tests/tempered_adaptive_restatement.py), bit for bit, in both widths and both kernel
forms; the invariances a ladder keeps while it adapts (two calls == one, shards, lp == the target at x, frozen after adapt_steps, c = 0
keeps rho0's ladder); the refusals; the Python mirror; and that the adaptation tunes the swap rates."""
import numpy as np
import pytest

import cases
import tempered_adaptive_restatement as A
import test_tempered_adaptive_cpu as CPU
import test_tempered_cpu as FIXED

pytestmark = pytest.mark.gpu

KF_TEMPERED, KF_TEMPERED_ADAPT = 16, 17


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    assert a.dtype == b.dtype, "%s: dtypes %s / %s" % (what, a.dtype, b.dtype)
    bad = np.argwhere(cases.bits(a) != cases.bits(b))
    assert len(bad) == 0, "%s: %d mismatches, first at %s: %r vs %r" % (what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


def _case_sampler(mhx, c):
    if c["kind"] == "iso":
        mv = mhx.MvNormal(mhx.zeros(c["d"]), (c["sigma"] ** 2) * mhx.I)
        assert mv.kind == 0 and mv.scale == c["sigma"]
    else:
        mv = mhx.MvNormal(mhx.zeros(c["d"]), np.asarray(c["sigma"], dtype=np.float64) ** 2)
        assert mv.kind == 1 and (np.asarray(mv.vec, dtype=np.float64) == np.asarray(c["sigma"])).all()
    adapt = mhx.LadderAdaptation(c["adapt_steps"], **{k: c[k] for k in CPU.ADAPT_KEYS if k in c})
    return mhx.Tempered(mhx.RWMH(mv), c["betas"], swap_every=c["swap_every"], adapt=adapt)


def _betas(run, real):
    """ladder_betas in the run's width: the widening is exact, so the narrowing gives the device's bits back"""
    b = run.betas()
    narrow = b.astype(np.float32 if real == "f32" else np.float64)
    assert (narrow.astype(np.float64) == b).all()
    return narrow


@pytest.mark.parametrize("form", ["register", "generic"])
@pytest.mark.parametrize("name", sorted(CPU.PARITY))
def test_adaptive_runs_bit_exact_against_the_restatement(mhx, oracle, real, name, form):
    c = CPU.PARITY[name]
    ref = CPU.restated(mhx, oracle, name, real)
    model, _ = FIXED.parity_model_and_target(mhx, oracle, c)
    n = c["R"] * c["nladders"]
    run = mhx.Run(model, _case_sampler(mhx, c), nchains=n, seed=c["seed"], first_chain=c["first"],
                  flags=mhx.FLAG_GENERIC if form == "generic" else 0)
    run.init()
    # before any transition: the ladder of rho0
    beta0, _ = A.ladder(A.rho0(c["betas"], c.get("rho_min", A.DEFAULTS["rho_min"]), c.get("rho_max", A.default_rho_max(c["R"]))))
    _same(_betas(run, real), np.array([beta0] * c["nladders"], dtype=oracle.real()), "ladder_betas after init")
    run.sample(c["N"], 0, 1, 0)
    st = run.stats()
    assert st["kernel_variant"] == KF_TEMPERED_ADAPT and st["reduce_lanes"] == 1
    assert run.form_name() == ("tempered_adapt_reg" if form == "register" else "tempered_adapt_generic")
    assert st["register_form"] == (1 if form == "register" else 0)
    value, acc = run.samples()
    _same(value, ref["samples"], "samples")
    _same(acc, ref["accepted"], "accepted")
    x, lp, cnt = run.state()
    _same(x, ref["final_x"], "final x")
    _same(lp, ref["final_lp"], "final lp")
    _same(cnt, ref["accept_counts"], "accept counts")
    att, swp = run.swap_stats()
    assert att.tolist() == ref["swap_attempts"].sum(axis=0).tolist() and swp.tolist() == ref["swap_counts"].sum(axis=0).tolist()
    _same(_betas(run, real), ref["betas"], "ladder_betas")
    assert (cases.bits(ref["betas"]) != cases.bits(np.array([beta0] * c["nladders"], dtype=oracle.real()))).any()
    # lp of every slot is the target at its x
    _same(mhx.logdensity(model, x), lp, "lp == target(x)")
    run.close()


def _setup(mhx, R=4, d=2, swap_every=3, adapt_steps=10, ratio=0.45, c=1.0, sigma2=0.81):
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = mhx.Tempered(mhx.RWMH(mhx.MvNormal(mhx.zeros(d), sigma2 * mhx.I)), [ratio ** q for q in range(R)], swap_every=swap_every,
                       adapt=mhx.LadderAdaptation(adapt_steps, c=c))
    return model, spl


def _run(mhx, model, spl, n, seed, first=0, flags=0):
    run = mhx.Run(model, spl, nchains=n, seed=seed, first_chain=first, flags=flags)
    run.init()
    return run


@pytest.mark.parametrize("seam", ["inside the adaptation", "at its end"])
@pytest.mark.parametrize("form", ["register", "generic"])
def test_two_sample_calls_equal_one(mhx, real, form, seam):
    """7 + 13 samples in two calls == 19 in one; the first call ends after transition 6: with adapt_steps = 10 inside the adaptation
    (rho crosses the seam in memory), with adapt_steps = 6 exactly at its end (the second launch derives the frozen ladder from rho)"""
    R, nl, seed = 4, 9, 0xA12
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    model, spl = _setup(mhx, adapt_steps=10 if seam == "inside the adaptation" else 6)
    one = _run(mhx, model, spl, R * nl, seed, flags=flags)
    one.sample(19, 0, 1, 0)
    v1, a1 = one.samples()
    two = _run(mhx, model, spl, R * nl, seed, flags=flags)
    two.sample(7, 0, 1, 0)
    va, aa = two.samples()
    mid = two.betas()
    two.sample(13, 0, 1, 0)
    vb, ab = two.samples()
    _same(va, v1[:7], "first call")
    _same(vb, v1[6:], "second call")
    _same(aa, a1[:7], "accepted, first call")
    _same(ab, a1[6:], "accepted, second call")
    for a, b in zip(one.state(), two.state()):
        _same(a, b, "final state")
    for a, b in zip(one.swap_stats(), two.swap_stats()):
        assert a.tolist() == b.tolist() and a.sum() > 0
    _same(one.betas(), two.betas(), "ladder_betas")
    if seam == "at its end":
        _same(mid, two.betas(), "frozen at the seam")
    else:
        assert (mid != two.betas()).any()
    one.close(), two.close()


@pytest.mark.parametrize("form", ["register", "generic"])
def test_a_shard_equals_the_matching_columns_of_the_larger_run(mhx, real, form):
    R, nl, seed, N = 8, 12, 0x5A4E, 16
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    model, spl = _setup(mhx, R=R, d=3, swap_every=1, adapt_steps=11, ratio=0.6, c=0.5, sigma2=0.64)
    whole = _run(mhx, model, spl, R * nl, seed, flags=flags)
    whole.sample(N, 0, 1, 0)
    vw, aw = whole.samples()
    first, n = 4 * R, 5 * R                                 # ladders 4 .. 8: the shard's waves hold other ladders than the whole run's
    shard = _run(mhx, model, spl, n, seed, first=first, flags=flags)
    shard.sample(N, 0, 1, 0)
    vs, as_ = shard.samples()
    _same(vs, vw[:, :, first:first + n], "shard samples")
    _same(as_, aw[:, first:first + n], "shard accepted")
    _same(shard.betas(), whole.betas()[4:9], "shard ladders")
    assert len(np.unique(whole.betas()[:, 1])) > 1          # every ladder went its own way
    whole.close(), shard.close()


@pytest.mark.parametrize("form", ["register", "generic"])
def test_the_ladder_is_frozen_after_adapt_steps_and_c_zero_keeps_rho0(mhx, oracle, real, form):
    R, nl, seed = 4, 6, 0xF0
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    model, spl = _setup(mhx, adapt_steps=10)
    run = _run(mhx, model, spl, R * nl, seed, flags=flags)
    start = run.betas()
    run.sample(1, 12, 1, 0)                                 # 12 transitions: swap rounds 1 .. 3 adapt (9 <= 10), round 4 does not
    frozen = run.betas()
    assert (frozen != start).any() and (frozen[:, 0] == 1).all() and (np.diff(frozen, axis=1) < 0).all()
    for _ in range(2):
        run.sample(5, 0, 1, 0)
        _same(run.betas(), frozen, "ladder_betas after adapt_steps")
    assert run.swap_stats()[0].sum() > 0
    run.init()                                              # a new start: the ladder and the adaptation begin again
    _same(run.betas(), start, "ladder_betas after a second init")
    run.close()
    model, still = _setup(mhx, adapt_steps=10, c=0.0)
    run = _run(mhx, model, still, R * nl, seed, flags=flags)
    run.sample(13, 0, 1, 0)
    _same(run.betas(), start, "c = 0")
    beta0, _ = A.ladder(A.rho0(still.betas, A.DEFAULTS["rho_min"], A.default_rho_max(R)))
    _same(run.betas(), np.array([beta0] * nl, dtype=np.float64), "c = 0: rho0's ladder")
    run.close()


def _refused(mhx, code, words, fn):
    with pytest.raises(mhx.MhxError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def test_refusals_name_their_rule(mhx, real):
    import ctypes as C
    L = mhx._lib
    d = 2
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    iso = mhx.MvNormal(mhx.zeros(d), mhx.I)
    EINVAL, ESTATE = mhx.MHX_EINVAL, mhx.MHX_ESTATE
    nan = float("nan")

    def create(R=2, n=8, first=0, swap_every=1, betas=(1.0, 0.5), scale=None, flags=0, steps=10, target_rate=nan, c=nan, kappa=nan,
               rho_min=nan, rho_max=nan):
        """the C entry itself: the Python mirror refuses most of these before the library sees them"""
        ctx = L.Context.default()
        b = np.ascontiguousarray(betas, dtype=np.float64)
        s = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
        cfg = L.RwmhCfg(d, n, 1, first, iso.kind, iso.scale, None, flags, None, 0)
        tcfg = L.TemperedCfg(R, swap_every, b.ctypes.data, None if s is None else s.ctypes.data)
        acfg = L.LadderAdaptCfg(steps, target_rate, c, kappa, rho_min, rho_max)
        h = C.c_void_p()
        L.check(L.lib().mhx_rwmh_create_tempered_adaptive(ctx.h, model.handle(ctx), C.byref(cfg), C.byref(tcfg), C.byref(acfg), C.byref(h)))
        L.lib().mhx_run_destroy(h)
    create()                                                # the defaults are accepted
    create(c=0.0, kappa=1.0, steps=0)
    _refused(mhx, EINVAL, ["swap_every = 0", "swap rounds"], lambda: create(swap_every=0))
    _refused(mhx, EINVAL, ["scale[] given", "follow"], lambda: create(scale=(1.0, 1.5)))
    _refused(mhx, EINVAL, ["adapt_steps = -1"], lambda: create(steps=-1))
    _refused(mhx, EINVAL, ["kappa = 0.5", "(0.5, 1]"], lambda: create(kappa=0.5))
    _refused(mhx, EINVAL, ["kappa = 1.5", "(0.5, 1]"], lambda: create(kappa=1.5))
    _refused(mhx, EINVAL, ["c = -1"], lambda: create(c=-1.0))
    _refused(mhx, EINVAL, ["target_rate = 0", "(0, 1)"], lambda: create(target_rate=0.0))
    _refused(mhx, EINVAL, ["target_rate = 1", "(0, 1)"], lambda: create(target_rate=1.0))
    _refused(mhx, EINVAL, ["rho_min", "rho_max"], lambda: create(rho_min=1.0, rho_max=0.0))
    _refused(mhx, EINVAL, ["(R - 1) exp(rho_max)", "> 80", "fp32"], lambda: create(rho_max=4.4))
    _refused(mhx, EINVAL, ["(R - 1) exp(rho_max)"], lambda: create(R=64, n=64, betas=[0.9 ** q for q in range(64)], rho_max=0.25))
    # everything the fixed ladder refuses, by the same checks
    _refused(mhx, EINVAL, ["mhx_rwmh_create_tempered_adaptive", "R = 3", "power of two"], lambda: create(R=3, n=9, betas=(1.0, 0.5, 0.25)))
    _refused(mhx, EINVAL, ["nchains = 9", "multiple of R"], lambda: create(n=9))
    _refused(mhx, EINVAL, ["first_chain = 3", "multiple of R"], lambda: create(first=3))
    _refused(mhx, EINVAL, ["beta[0]", "exactly 1"], lambda: create(betas=(0.9, 0.5)))
    _refused(mhx, EINVAL, ["strictly decreasing"], lambda: create(betas=(1.0, 1.0)))
    _refused(mhx, EINVAL, ["swap_every = -1"], lambda: create(swap_every=-1))
    _refused(mhx, EINVAL, ["MHX_FLAG_ZIGGURAT"], lambda: create(flags=mhx.FLAG_ZIGGURAT))
    user = mhx.DensityModel(FIXED.bimodal, dim=2)
    adapt = mhx.LadderAdaptation(10)

    def make(m=model, flags=0):
        return mhx.Run(m, mhx.Tempered(mhx.RWMH(iso), [1.0, 0.5], adapt=adapt), nchains=8, seed=1, flags=flags)
    _refused(mhx, EINVAL, ["MHX_FLAG_NO_JIT", "user target"], lambda: make(m=user, flags=mhx.FLAG_NO_JIT))
    # a catalogue target without the run-time compiler: the pre-built state-in-HBM form
    run = make(flags=mhx.FLAG_NO_JIT)
    assert run.form_name() == "tempered_adapt_generic"
    run.init()
    run.sample(4, 0, 1, 0)
    assert run.swap_stats()[0].sum() > 0 and run.betas().shape == (4, 2)
    snap = run.rung(0)
    assert snap.n == 4
    snap.close()
    _refused(mhx, ESTATE, ["MHX_SAVE_MOMENTS", "tempered"], lambda: run.sample(4, save="moments"))
    _refused(mhx, ESTATE, ["mhx_run_sample_to_host", "tempered", "swap"], lambda: run.sample_to_host(4))
    _refused(mhx, ESTATE, ["checkpoint", "tempered"], lambda: run.save_state())
    _refused(mhx, ESTATE, ["checkpoint", "tempered"], lambda: run.load_state(b"\0" * 128))
    g = mhx.Group([0])
    other = mhx.Run(model, mhx.Tempered(mhx.RWMH(iso), [1.0, 0.5], adapt=adapt), nchains=8, seed=1, ctx=g.ctxs[0])
    _refused(mhx, ESTATE, ["mhx_group_attach", "tempered"], lambda: g.attach([other]))
    g.close()
    # ladder_betas: a fixed ladder returns its table, a run that is not tempered is refused
    fixed = mhx.Run(model, mhx.Tempered(mhx.RWMH(iso), [1.0, 0.3]), nchains=8, seed=1)
    want = np.array([[1.0, 0.3]] * 4, dtype=np.float32 if real == "f32" else np.float64).astype(np.float64)
    _same(fixed.betas(), want, "a fixed ladder's table")
    assert fixed.stats()["kernel_variant"] in (0, KF_TEMPERED) and fixed.form_name() == "tempered_reg"
    plain = mhx.Run(model, mhx.RWMH(iso), nchains=8, seed=1)
    _refused(mhx, ESTATE, ["mhx_run_ladder_betas", "not a tempered run"], lambda: plain.betas())
    plain.close(), run.close(), fixed.close()


def test_sample_returns_the_cold_chains_and_the_ladder_tables(mhx, oracle, real):
    name = "r8_diag_bimodal_partial_wave"
    c = CPU.PARITY[name]
    ref = CPU.restated(mhx, oracle, name, real)
    model, target = FIXED.parity_model_and_target(mhx, oracle, c)
    spl = _case_sampler(mhx, c)
    with pytest.raises(mhx.ArgumentError) as ei:
        mhx.sample(model, spl, 10, c["nladders"], discard_initial=c["adapt_steps"] - 1)
    assert "discard_initial" in str(ei.value) and "adapt.steps" in str(ei.value)
    # the parity case again under a schedule sample() accepts: the first adapt_steps + 1 transitions discarded
    disc = c["adapt_steps"] + 1
    N = c["N"] - disc
    chain = mhx.sample(model, spl, N, c["nladders"], seed=c["seed"], first_chain=c["first"], discard_initial=disc)
    assert chain.nchains == c["nladders"] and chain.value.shape == (N, c["d"] + 1, c["nladders"])
    _same(chain.value, ref["samples"][disc:, :, 0::c["R"]], "cold chains")
    _same(chain.accepted, ref["accepted"][disc:, 0::c["R"]], "cold accepted")
    b = chain.tempered.betas()
    assert b.shape == (c["nladders"], c["R"]) and b.dtype == np.float64
    _same(b.astype(oracle.real()), ref["betas"], "betas()")
    lad = chain.tempered.ladder()
    assert len(lad) == c["R"] and [w["rung"] for w in lad] == list(range(c["R"]))
    assert [w["beta_median"] for w in lad] == np.median(b, axis=0).tolist()
    assert all(w["beta_min"] <= w["beta_median"] <= w["beta_max"] for w in lad) and lad[0]["beta_min"] == lad[0]["beta_max"] == 1.0
    att, swp = ref["swap_attempts"].sum(axis=0), ref["swap_counts"].sum(axis=0)
    assert [w["rate"] for w in lad[:-1]] == [float(swp[q]) / float(att[q]) for q in range(c["R"] - 1)] and np.isnan(lad[-1]["rate"])
    text = str(lad)
    print(text)
    assert "swap rate" in text.splitlines()[0] and len(text.splitlines()) == c["R"] + 1
    table = chain.tempered.swap_rates()
    assert [w["beta_lo"] for w in table] == np.median(b, axis=0)[:-1].tolist()            # an adaptive run reports the median beta
    assert [w["attempts"] for w in table] == att.tolist() and [w["swaps"] for w in table] == swp.tolist()
    print(table)
    assert np.isfinite(chain.rhat()["rhat"]).all()


# ---- that it tunes
TUNE = dict(R=8, d=4, nladders=256, T=2000, beta_min=1e-3, seed=0x7A7E, sigma=1.0, thin=4)
TARGET = 0.234
# |rate - 0.234| of the restatement's ladders after they froze, the largest over the seven pairs, and the band of the test: that plus
# three binomial standard errors at this test's count of attempts per pair (nladders * T / 2)
TUNE_REFERENCE_OFFSET = 0.0081
TUNE_BAND = 0.0106


def test_the_adaptation_tunes_the_swap_rates(mhx, real):
    """An isotropic Gaussian in d = 4 under geometric_betas(8, 1e-3), 256 ladders, 2000 adapting transitions and 2000 frozen ones, a
    swap round per transition.  The swap rate of every pair over the frozen half (the difference of two swap_stats() calls, pooled over
    the ladders) must lie nearer to 0.234 than the same pair's rate on the fixed starting ladder, and inside a band around 0.234.

    The band is measured on the reference, not on the engine: the restatement (tests/tempered_adaptive_restatement.py, fp64) at this
    configuration and seed on the first 64 of the ladders gave, over its frozen half (64 000 attempts a pair, one binomial standard
    error 0.0017), the rates
        0.2368  0.2421  0.2316  0.2403  0.2361  0.2336  0.2368     (the fixed starting ladder: 0.358 .. 0.365)
    so its largest offset from 0.234 is 0.0081.  Three binomial standard errors at this test's 256 000 attempts a pair are 0.0025:
    the band is 0.0081 + 0.0025 = 0.0106, chosen before the engine was run.  The restated ladders' median betas after freezing:
    1, 0.276, 0.0748, 0.0200, 0.00535, 0.00148, 0.000399, 0.000108; their cold rung's pooled E x^2 is 0.998 +- 0.007."""
    t = TUNE
    R, d, T = t["R"], t["d"], t["T"]
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    rw = mhx.RWMH(mhx.MvNormal(mhx.zeros(d), (t["sigma"] ** 2) * mhx.I))
    start = mhx.geometric_betas(R, t["beta_min"])
    n = R * t["nladders"]
    rates = {}
    for which, spl in (("fixed", mhx.Tempered(rw, start, swap_every=1)),
                       ("adaptive", mhx.Tempered(rw, start, swap_every=1, adapt=mhx.LadderAdaptation(T)))):
        run = mhx.Run(model, spl, nchains=n, seed=t["seed"])
        run.init()
        run.sample(1, T, 1, 0)                              # T transitions: the adaptation, whole
        a1, s1 = run.swap_stats()
        b1 = run.betas()
        run.sample(T // t["thin"] + 1, 0, t["thin"], 0)     # T more, the ladder frozen
        a2, s2 = run.swap_stats()
        _same(run.betas(), b1, "frozen")
        assert ((a2 - a1) == t["nladders"] * T // 2).all()
        rates[which] = (s2 - s1).astype(np.float64) / (a2 - a1).astype(np.float64)
        if which == "adaptive":
            value, _ = run.samples()
            cold = value[:, :d, 0::R].astype(np.float64)
            lad = run.ladder()
        run.close()
    print("fixed   ", np.round(rates["fixed"], 4).tolist())
    print("adaptive", np.round(rates["adaptive"], 4).tolist())
    print(lad)
    se3 = 3.0 * np.sqrt(TARGET * (1.0 - TARGET) / (t["nladders"] * T / 2.0))
    assert abs(TUNE_BAND - (TUNE_REFERENCE_OFFSET + se3)) < 1e-4
    off_a, off_f = np.abs(rates["adaptive"] - TARGET), np.abs(rates["fixed"] - TARGET)
    print("offsets: adaptive", np.round(off_a, 4).tolist(), "fixed", np.round(off_f, 4).tolist(), "band", TUNE_BAND)
    assert (off_a < off_f).all(), (rates["adaptive"], rates["fixed"])
    assert (off_a < TUNE_BAND).all(), (rates["adaptive"], TUNE_BAND)
    # the cold rung still samples N(0, I): E x^2 about the known mean, per ladder, against its own standard error over the ladders (the
    # tolerance of tests/test_tempered_cpu.py's detailed-balance test: five standard errors)
    per_ladder = (cold ** 2).mean(axis=(0, 1))
    mean, se = per_ladder.mean(), per_ladder.std(ddof=1) / np.sqrt(t["nladders"])
    print("cold E x^2 %.4f +- %.4f" % (mean, se))
    assert abs(mean - 1.0) < 5 * se
