"""GPU: anchored tempered runs (mhx_rwmh_create_tempered_anchored, kernel variant 18) against the test-side restatement of the arithmetic
spec (tests/tempered_anchored_restatement.py), bit for bit, in both widths and both kernel forms; the
invariances (two calls == one, shards, unit betas == the plain run, lp == the target at x); mhx_run_evidence against a longdouble
restatement on the tensor the run returns; the known answer; the refusals; the hot rung of a beta = 0 ladder."""
import math

import numpy as np
import pytest

import cases
import tempered_anchored_restatement as A
import test_tempered_anchored_cpu as CPU

pytestmark = pytest.mark.gpu

KF_TEMPERED_ANCHOR = 18
EPS = 2.0 ** -53


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    assert a.dtype == b.dtype, "%s: dtypes %s / %s" % (what, a.dtype, b.dtype)
    bad = np.argwhere(cases.bits(a) != cases.bits(b))
    assert len(bad) == 0, "%s: %d mismatches, first at %s: %r vs %r" % (what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


def _reference(mhx, mean, sd):
    return mhx.MvNormal(np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64) ** 2)


def _case_sampler(mhx, c):
    if c["kind"] == "iso":
        mv = mhx.MvNormal(mhx.zeros(c["d"]), (c["sigma"] ** 2) * mhx.I)
    else:
        mv = mhx.MvNormal(mhx.zeros(c["d"]), np.asarray(c["sigma"], dtype=np.float64) ** 2)
    spl = mhx.Tempered(mhx.RWMH(mv), c["betas"], swap_every=c["swap_every"], scales=c["scales"], reference=_reference(mhx, c["mean"], c["sd"]))
    # the reference's sd as the engine will see it is the restatement's (sqrt of the squared double is exact for these)
    assert spl.ref_sd.tolist() == [float(v) for v in c["sd"]] and spl.ref_mean.tolist() == [float(v) for v in c["mean"]]
    if c["kind"] == "iso":
        assert mv.kind == 0 and mv.scale == c["sigma"]
    return spl


@pytest.mark.parametrize("form", ["register", "generic"])
@pytest.mark.parametrize("name", sorted(CPU.PARITY))
def test_anchored_runs_bit_exact_against_the_restatement(mhx, oracle, real, name, form):
    c = CPU.PARITY[name]
    ref = CPU.restated(mhx, oracle, name, real)
    model, _ = CPU.parity_model_and_target(mhx, oracle, c)
    spl = _case_sampler(mhx, c)
    n = c["R"] * c["nladders"]
    run = mhx.Run(model, spl, nchains=n, seed=c["seed"], first_chain=c["first"], flags=mhx.FLAG_GENERIC if form == "generic" else 0)
    run.init()
    run.sample(c["N"], c["discard"], c["thinning"], 0)
    st = run.stats()
    assert st["kernel_variant"] == KF_TEMPERED_ANCHOR and st["reduce_lanes"] == 1
    assert run.form_name() == ("tempered_anchored_reg" if form == "register" else "tempered_anchored_generic")
    assert st["register_form"] == (1 if form == "register" else 0)
    value, acc = run.samples()
    _same(value, ref["samples"], "samples")
    _same(acc, ref["accepted"], "accepted")
    x, lp, cnt = run.state()
    _same(x, ref["final_x"], "final x")
    _same(lp, ref["final_lp"], "final lp")
    _same(cnt, ref["accept_counts"], "accept counts")
    assert st["accepted"] == int(ref["accept_counts"].sum())
    att, swp = run.swap_stats()
    assert att.tolist() == ref["swap_attempts"].sum(axis=0).tolist() and swp.tolist() == ref["swap_counts"].sum(axis=0).tolist()
    assert (swp > 0).all() and (swp < att).all()
    # the recorded lp stays the UNTEMPERED target at x, for every slot: a swap that moved x without lp (or the reverse) fails here
    _same(mhx.logdensity(model, x), lp, "lp == target(x)")
    _same(run.betas()[0], np.array([float(oracle.real()(b)) for b in c["betas"]]), "ladder betas")
    run.close()


def _run(mhx, model, spl, n, seed, first=0, flags=0, init=None, reduce_lanes=0):
    run = mhx.Run(model, spl, nchains=n, seed=seed, first_chain=first, flags=flags, reduce_lanes=reduce_lanes)
    run.init(init)
    return run


def _ladder(mhx, d, R=4, swap_every=3):
    betas = mhx.power_betas(R, 2.0)
    q = _reference(mhx, np.linspace(-0.5, 0.7, d), np.linspace(1.2, 1.8, d))
    return mhx.Tempered(mhx.RWMH(mhx.MvNormal(mhx.zeros(d), 0.81 * mhx.I)), betas, swap_every=swap_every, scales=np.linspace(1.0, 1.6, R), reference=q)


@pytest.mark.parametrize("form", ["register", "generic"])
def test_two_sample_calls_equal_one(mhx, real, form):
    """7 + 13 samples in two calls == 19 in one: lq is recomputed from x at the start of the second launch, to the same bits"""
    R, nl, d, seed = 4, 9, 2, 0xA12
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = _ladder(mhx, d)
    one = _run(mhx, model, spl, R * nl, seed, flags=flags)
    one.sample(19, 0, 1, 0)
    v1, a1 = one.samples()
    two = _run(mhx, model, spl, R * nl, seed, flags=flags)
    two.sample(7, 0, 1, 0)
    va, aa = two.samples()
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
    one.close(), two.close()


@pytest.mark.parametrize("form", ["register", "generic"])
def test_a_shard_equals_the_matching_columns_of_the_larger_run(mhx, real, form):
    R, nl, d, seed, N = 8, 12, 3, 0x5A4E, 16
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = _ladder(mhx, d, R=8, swap_every=1)
    whole = _run(mhx, model, spl, R * nl, seed, flags=flags)
    whole.sample(N, 0, 1, 0)
    vw, aw = whole.samples()
    first, n = 4 * R, 5 * R                                 # ladders 4 .. 8
    shard = _run(mhx, model, spl, n, seed, first=first, flags=flags)
    shard.sample(N, 0, 1, 0)
    vs, as_ = shard.samples()
    _same(vs, vw[:, :, first:first + n], "shard samples")
    _same(as_, aw[:, first:first + n], "shard accepted")
    whole.close(), shard.close()


@pytest.mark.parametrize("kind", ["iso", "diag"])
@pytest.mark.parametrize("form", ["register", "generic"])
def test_unit_betas_without_swaps_are_the_plain_run(mhx, real, form, kind):
    """whatever the reference: with beta = 1 the reference's share of log a is a zero"""
    d, n, seed, N = 5, 70, 0xB37B, 12
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    mv = mhx.MvNormal(mhx.zeros(d), 0.49 * mhx.I) if kind == "iso" else mhx.MvNormal(mhx.zeros(d), np.linspace(0.3, 1.2, d) ** 2)
    plain = _run(mhx, model, mhx.RWMH(mv), n, seed, first=6, flags=flags, reduce_lanes=1)
    plain.sample(N, 2, 2, 0)
    assert plain.stats()["reduce_lanes"] == 1
    vp, ap = plain.samples()
    q = _reference(mhx, np.linspace(-3.0, 11.0, d), np.linspace(0.01, 3.0, d))
    temp = _run(mhx, model, mhx.Tempered(mhx.RWMH(mv), [1.0, 1.0], swap_every=0, scales=[1.0, 1.0], reference=q), n, seed, first=6, flags=flags)
    temp.sample(N, 2, 2, 0)
    vt, at = temp.samples()
    _same(vt, vp, "samples")
    _same(at, ap, "accepted")
    for a, b in zip(plain.state(), temp.state()):
        _same(a, b, "final state")
    plain.close(), temp.close()


# ---- mhx_run_evidence
def _check_table(got, want, mag, n_saved, what):
    """bad, shift and the maxima bit for bit; the sums within (n_saved + 8) 2^-53 sum |terms| (only the order of summation differs)"""
    for k, name in ((0, "bad"), (1, "shift"), (4, "max_f"), (6, "max_b")):
        _same(got[:, k], want[:, k], "%s: %s" % (what, name))
    worst = 0.0
    for k, name in ((2, "s1"), (3, "s2"), (5, "sumexp_f"), (7, "sumexp_b")):
        bound = (n_saved + 8) * EPS * mag[:, k]
        err = np.abs(got[:, k] - want[:, k])
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        assert (err <= bound).all(), "%s: %s off by %g of its bound at chain %d" % (what, name, (err / bound).max(), int(np.argmax(err - bound)))
    print(what, "largest error / bound %.3f" % worst)


class _Box:
    """uniform on [-2, 2]^2 up to its constant, -inf outside: a bounded support"""
    source = """MHX_LOGDENSITY(x, d, data, ndata) {
    const bool in = x[0] >= MHX_R(-2.0) && x[0] <= MHX_R(2.0) && x[1] >= MHX_R(-2.0) && x[1] <= MHX_R(2.0);
    return in ? MHX_R(-0.125) * (x[0] * x[0] + x[1] * x[1]) : -MHX_INF;
}"""


@pytest.mark.parametrize("n_saved,R,nl", [(1, 2, 33), (17, 8, 40), (40, 2, 33), (40, 8, 40)])
def test_run_evidence_against_the_longdouble_restatement(mhx, oracle, real, n_saved, R, nl):
    d = 2
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    mean, sd = [0.3, -0.2], [1.4, 1.1]
    betas = mhx.power_betas(R, 3.0)
    spl = mhx.Tempered(mhx.RWMH(mhx.MvNormal(mhx.zeros(d), mhx.I)), betas, swap_every=1, scales=np.linspace(1.0, 1.5, R),
                       reference=_reference(mhx, mean, sd))
    run = _run(mhx, model, spl, R * nl, 0xE0 + n_saved)
    run.sample(n_saved, 3, 1, 0)
    value, _ = run.samples()
    u = A.u_of_samples(value, betas, mean, sd)
    want, mag = A.evidence_table(u, betas)
    got, n = run.evidence_table()
    assert n == n_saved and got.shape == (R * nl, 8) and want[:, 0].sum() == 0
    _check_table(got, want, mag, n_saved, "n_saved %d, %d chains [%s]" % (n_saved, R * nl, real))
    # the pair a rung has no use for is neutral
    assert (got[0::R, 4] == -np.inf).all() and (got[0::R, 5] == 0).all() and (got[R - 1::R, 6] == -np.inf).all() and (got[R - 1::R, 7] == 0).all()
    again, _ = run.evidence_table()
    _same(again, got, "two calls")
    ev = run.evidence()
    host = mhx.evidence_from_table(want, run.betas()[0], n_saved)
    for k in ("log_z_ti", "log_z_ss", "log_z_ss_backward"):
        assert ev[k] == pytest.approx(host[k], rel=1e-12, abs=1e-12)
    run.close()


def test_run_evidence_leaves_out_the_draws_outside_a_bounded_support(mhx, oracle, real):
    """chains that start outside the support have lp = -inf: u = -inf is counted in `bad` and left out of every sum.  On the beta = 0
    rung such a chain cannot move (0 * inf is NaN, a reject) until a swap brings it a state; elsewhere its first candidate inside
    the support is accepted"""
    R, nl, d, N = 4, 16, 2, 17
    model = mhx.DensityModel(mhx.HipLogDensity(_Box.source, d))
    mean, sd = [0.0, 0.0], [1.0, 1.0]
    betas = mhx.power_betas(R, 2.0)
    spl = mhx.Tempered(mhx.RWMH(mhx.MvNormal(mhx.zeros(d), mhx.I)), betas, swap_every=2, scales=[1.0, 1.0, 1.0, 1.0], reference=_reference(mhx, mean, sd))
    init = np.random.default_rng(5).uniform(-1.5, 1.5, size=(d, R * nl)).astype(oracle.real())
    init[:, 1::3] += 5.0                                    # every third chain outside, some of them on the beta = 0 rung
    run = _run(mhx, model, spl, R * nl, 0xB0C5, init=init)
    run.sample(N, 0, 1, 0)
    value, _ = run.samples()
    assert np.isneginf(value[:, d, :]).any() and np.isfinite(value[-1, d, 0::R]).all()
    u = A.u_of_samples(value, betas, mean, sd)
    want, mag = A.evidence_table(u, betas)
    got, n = run.evidence_table()
    assert n == N and want[:, 0].sum() > 0 and (want[1::3, 1] == 0.0).all()       # ... whose shift is 0
    _check_table(got, want, mag, N, "bounded support [%s]" % real)
    assert run.evidence()["bad"] == int(want[:, 0].sum())
    # the sums are over the finite draws alone
    c = int(np.argmax(want[:, 0]))
    fin = u[np.isfinite(u[:, c]), c]
    assert got[c, 0] == N - fin.size and got[c, 2] == pytest.approx(float((fin - got[c, 1]).sum()), rel=1e-12, abs=1e-12)
    run.close()


def _refused(mhx, code, words, fn):
    with pytest.raises(mhx.MhxError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def test_run_evidence_refuses_runs_that_carry_no_evidence(mhx, real):
    d = 2
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    iso = mhx.MvNormal(mhx.zeros(d), mhx.I)
    ESTATE = mhx.MHX_ESTATE
    plain = _run(mhx, model, mhx.RWMH(iso), 8, 1)
    plain.sample(4, 0, 1, 0)
    _refused(mhx, ESTATE, ["mhx_run_evidence", "not an anchored"], lambda: mhx.Run.evidence_table(plain))
    fixed = _run(mhx, model, mhx.Tempered(mhx.RWMH(iso), [1.0, 0.5]), 8, 1)
    fixed.sample(4, 0, 1, 0)
    _refused(mhx, ESTATE, ["mhx_run_evidence", "not an anchored"], lambda: fixed.evidence_table())
    q = _reference(mhx, [0.0, 0.0], [1.5, 1.5])
    above = _run(mhx, model, mhx.Tempered(mhx.RWMH(iso), [1.0, 0.5], reference=q), 8, 1)
    _refused(mhx, ESTATE, ["mhx_run_evidence", "sample tensor"], lambda: above.evidence_table())
    above.sample(4, 0, 1, 0)
    _refused(mhx, ESTATE, ["mhx_run_evidence", "last beta is not 0"], lambda: above.evidence_table())
    assert above.swap_stats()[0].sum() > 0 and above.rung(1).n == 4                 # the ladder's other tables work on it
    plain.close(), fixed.close(), above.close()


def test_known_answer_on_the_device(mhx, oracle, real):
    """chain.tempered.evidence() on the CPU test's known-answer case is the host computation from the restated tensor: the chain is
    bit-exact, so it inherits that test's statistical check against the closed form"""
    k = CPU.KNOWN
    res, u, table, mag = CPU.known_restated(mhx, oracle, real)
    model, _ = CPU.known_model_and_target(mhx, oracle)
    spl = mhx.Tempered(mhx.RWMH(mhx.MvNormal(mhx.zeros(2), (k["sigma"] ** 2) * mhx.I)), CPU.known_betas(mhx), swap_every=1,
                       scales=CPU.known_scales(mhx), reference=_reference(mhx, k["m"], [k["t"]] * 2))
    chain = mhx.sample(model, spl, k["N"], k["nladders"], seed=k["seed"], first_chain=k["first"], discard_initial=k["discard"], thinning=k["thinning"])
    _same(chain.value, res["samples"][:, :, 0::k["R"]], "cold chains")
    full, _ = chain.tempered.samples()
    _same(full, res["samples"], "every rung")
    got, n = chain.tempered.evidence_table()
    assert n == k["N"]
    _check_table(got, table, mag, k["N"], "known answer [%s]" % real)
    ev = chain.tempered.evidence()
    host = mhx.evidence_from_table(table, chain.tempered.betas()[0], k["N"])
    print(ev)
    for name in ("log_z_ti", "log_z_ti_coarse", "log_z_ss", "log_z_ss_backward", "se_ti", "se_ss", "se_ss_backward"):
        assert ev[name] == pytest.approx(host[name], rel=1e-11, abs=1e-11), name
    assert ev["bad"] == 0 and abs(ev["log_z_ss"] - k["log_z"]) < 4 * ev["se_ss"]


def test_refusals_name_their_rule(mhx, real):
    d = 2
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    iso = mhx.MvNormal(mhx.zeros(d), mhx.I)
    EINVAL, ESTATE = mhx.MHX_EINVAL, mhx.MHX_ESTATE
    L = mhx._lib
    import ctypes as C

    def create(betas, scales, mean, sd, n=8):
        """the C entry itself: what the Python mirror refuses first is refused by the library too"""
        b = np.asarray(betas, dtype=np.float64)
        s = None if scales is None else np.asarray(scales, dtype=np.float64)
        m = None if mean is None else np.asarray(mean, dtype=np.float64)
        v = None if sd is None else np.asarray(sd, dtype=np.float64)
        run = mhx.Run(model, mhx.RWMH(iso), nchains=n, seed=1)          # (a context and a target handle of the right width)
        cfg = L.RwmhCfg(d, n, 1, 0, 0, 1.0, None, 0, None, 0)
        tcfg = L.TemperedCfg(len(b), 1, b.ctypes.data, None if s is None else s.ctypes.data)
        ref = L.TemperedReference(None if m is None else m.ctypes.data, None if v is None else v.ctypes.data)
        h = C.c_void_p()
        try:
            L.check(L.lib().mhx_rwmh_create_tempered_anchored(run.ctx.h, model.handle(run.ctx), C.byref(cfg), C.byref(tcfg), C.byref(ref), C.byref(h)))
            L.lib().mhx_run_destroy(h)
        finally:
            run.close()
    ok = dict(betas=[1.0, 0.5], scales=None, mean=[0.0, 0.0], sd=[1.0, 2.0])
    create(**ok)
    _refused(mhx, EINVAL, ["reference", "mean is NULL"], lambda: create(**dict(ok, mean=None)))
    _refused(mhx, EINVAL, ["reference", "sd is NULL"], lambda: create(**dict(ok, sd=None)))
    _refused(mhx, EINVAL, ["mean[1]", "not finite"], lambda: create(**dict(ok, mean=[0.0, float("nan")])))
    _refused(mhx, EINVAL, ["sd[0]", "not finite"], lambda: create(**dict(ok, sd=[float("inf"), 1.0])))
    _refused(mhx, EINVAL, ["sd[1] = 0", "positive"], lambda: create(**dict(ok, sd=[1.0, 0.0])))
    _refused(mhx, EINVAL, ["sd[0] = -1", "positive"], lambda: create(**dict(ok, sd=[-1.0, 1.0])))
    _refused(mhx, EINVAL, ["beta[1] = 0", "not the last"], lambda: create(**dict(ok, betas=[1.0, 0.0, 0.5, 0.25], scales=[1, 2, 3, 4])))
    _refused(mhx, EINVAL, ["beta[3] = 0", "without scale[]"], lambda: create(**dict(ok, betas=[1.0, 0.5, 0.25, 0.0])))
    _refused(mhx, EINVAL, ["beta[1]", "positive"], lambda: create(**dict(ok, betas=[1.0, -0.5])))
    create(**dict(ok, betas=[1.0, 0.5, 0.25, 0.0], scales=[1, 1.5, 2, 3]))
    # what a fixed ladder refuses, an anchored one refuses
    q = _reference(mhx, [0.0, 0.0], [1.5, 1.5])

    def make(betas=(1.0, 0.0), n=8, first=0, scales=(1.0, 2.0), flags=0, reduce_lanes=0):
        spl = mhx.Tempered(mhx.RWMH(iso), list(betas), scales=scales, reference=q)
        return mhx.Run(model, spl, nchains=n, seed=1, first_chain=first, flags=flags, reduce_lanes=reduce_lanes)
    _refused(mhx, EINVAL, ["R = 3", "power of two"], lambda: make(betas=(1.0, 0.5, 0.0), scales=(1, 2, 3), n=9))
    _refused(mhx, EINVAL, ["nchains = 9", "multiple of R"], lambda: make(n=9))
    _refused(mhx, EINVAL, ["first_chain = 3", "multiple of R"], lambda: make(first=3))
    _refused(mhx, EINVAL, ["MHX_FLAG_ZIGGURAT"], lambda: make(flags=mhx.FLAG_ZIGGURAT))
    _refused(mhx, EINVAL, ["reduce_lanes = 2"], lambda: make(reduce_lanes=2))
    # a zero beta without a reference is still no ladder
    _refused(mhx, EINVAL, ["beta[1]", "positive"],
             lambda: mhx.Run(model, mhx.Tempered(mhx.RWMH(iso), [1.0, 0.0], scales=[1.0, 2.0]), nchains=8, seed=1))
    run = make(flags=mhx.FLAG_NO_JIT)                       # a catalogue target without the run-time compiler: the pre-built form
    assert run.form_name() == "tempered_anchored_generic"
    run.init()
    run.sample(4, 0, 1, 0)
    assert run.stats()["kernel_variant"] == KF_TEMPERED_ANCHOR and run.stats()["register_form"] == 0
    _refused(mhx, ESTATE, ["MHX_SAVE_MOMENTS", "tempered"], lambda: run.sample(4, save="moments"))
    _refused(mhx, ESTATE, ["mhx_run_sample_to_host", "tempered"], lambda: run.sample_to_host(4))
    _refused(mhx, ESTATE, ["checkpoint", "tempered"], lambda: run.save_state())
    g = mhx.Group([0])
    other = mhx.Run(model, mhx.Tempered(mhx.RWMH(iso), [1.0, 0.0], scales=[1.0, 2.0], reference=q), nchains=8, seed=1, ctx=g.ctxs[0])
    _refused(mhx, ESTATE, ["mhx_group_attach", "tempered"], lambda: g.attach([other]))
    g.close()
    run.close()
    # a dimension above the anchored register form's own limit runs the state-in-HBM form (the fixed ladder's register form reaches it)
    big = {"f64": 46, "f32": 78}[real]
    bm = mhx.DensityModel(mhx.IsoGaussian(big))
    bq = _reference(mhx, np.zeros(big), np.full(big, 1.5))
    wide = mhx.Run(bm, mhx.Tempered(mhx.RWMH(mhx.MvNormal(mhx.zeros(big), mhx.I)), [1.0, 0.0], scales=[1.0, 1.5], reference=bq), nchains=8, seed=1)
    assert wide.form_name() == "tempered_anchored_generic"
    wide.close()


def test_the_hot_rung_of_a_ladder_that_ends_at_zero_samples_the_reference(mhx, real):
    """q = N(0, I) and beta = 0: mean and variance of rung R - 1 within 4 of their Monte-Carlo standard errors of 0 and 1.  The target,
    N((2, 2), 0.25 I), is somewhere else; the errors are those between ladders (independent), of per-ladder means"""
    R, nl, d, N = 4, 512, 2, 64

    def target(x):
        return -2.0 * ((x[0] - 2.0) * (x[0] - 2.0) + (x[1] - 2.0) * (x[1] - 2.0))
    model = mhx.DensityModel(target, dim=d)
    spl = mhx.Tempered(mhx.RWMH(mhx.MvNormal(mhx.zeros(d), 0.36 * mhx.I)), mhx.power_betas(R, 3.0), swap_every=1, scales=[1.0, 1.4, 2.4, 2.8],
                       reference=mhx.MvNormal(mhx.zeros(d), mhx.I))
    run = _run(mhx, model, spl, R * nl, 0x407)
    run.sample(N, 60, 2, 0)
    hot = run.rung(R - 1)
    x, _ = hot.samples()
    x = x[:, :d, :].astype(np.float64)
    assert x.shape == (N, d, nl)
    for k in range(d):
        m_l = x[:, k, :].mean(axis=0)
        v_l = (x[:, k, :] ** 2).mean(axis=0)                 # E x^2 about the known mean 0
        m, se_m = m_l.mean(), m_l.std(ddof=1) / math.sqrt(nl)
        v, se_v = v_l.mean(), v_l.std(ddof=1) / math.sqrt(nl)
        print("param %d: mean %.4f +- %.4f, variance %.4f +- %.4f" % (k, m, se_m, v, se_v))
        assert abs(m) < 4 * se_m and abs(v - 1.0) < 4 * se_v
    att, swp = run.swap_stats()
    assert (swp > 0).all() and (swp < att).all()
    hot.close(), run.close()
