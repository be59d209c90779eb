"""GPU: tempered random-walk Metropolis-Hastings runs (mhx_rwmh_create_tempered, kernel variant 16) against the test-side restatement
of the arithmetic spec (tests/tempered_restatement.py), bit for bit, in both widths and both kernel forms; the
invariances a ladder must keep (two calls == one, shards, unit betas == the plain run, lp == the target at x); the rung snapshot; the
refusals; the Python mirror."""
import ctypes as C

import numpy as np
import pytest

import cases
import tempered_restatement as P
import test_tempered_cpu as CPU

pytestmark = pytest.mark.gpu

KF_TEMPERED = 16


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    assert a.dtype == b.dtype, "%s: dtypes %s / %s" % (what, a.dtype, b.dtype)
    bad = np.argwhere(cases.bits(a) != cases.bits(b))
    assert len(bad) == 0, "%s: %d mismatches, first at %s: %r vs %r" % (what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


def _case_sampler(mhx, c):
    if c["kind"] == "iso":
        mv = mhx.MvNormal(mhx.zeros(c["d"]), (c["sigma"] ** 2) * mhx.I)
    else:
        mv = mhx.MvNormal(mhx.zeros(c["d"]), np.asarray(c["sigma"], dtype=np.float64) ** 2)
    return mhx.Tempered(mhx.RWMH(mv), c["betas"], swap_every=c["swap_every"], scales=c["scales"])


def _proposal_matches(mhx, oracle, c, spl):
    """the MvNormal's scale as the engine will use it is the restatement's sigma (sqrt of the squared double is exact for these)"""
    mv = spl.proposal.proposal
    if c["kind"] == "iso":
        assert mv.kind == 0 and mv.scale == c["sigma"]
    else:
        assert mv.kind == 1
        _same(np.asarray(mv.vec, dtype=oracle.real()), np.asarray(c["sigma"], dtype=oracle.real()), "sigma_k")


@pytest.mark.parametrize("form", ["register", "generic"])
@pytest.mark.parametrize("name", sorted(CPU.PARITY))
def test_tempered_runs_bit_exact_against_the_restatement(mhx, oracle, real, name, form):
    c = CPU.PARITY[name]
    ref = CPU.restated(mhx, oracle, name, real)
    model, _ = CPU.parity_model_and_target(mhx, oracle, c)
    spl = _case_sampler(mhx, c)
    _proposal_matches(mhx, oracle, c, spl)
    n = c["R"] * c["nladders"]
    run = mhx.Run(model, spl, nchains=n, seed=c["seed"], first_chain=c["first"], flags=mhx.FLAG_GENERIC if form == "generic" else 0)
    run.init()
    run.sample(c["N"], c["discard"], c["thinning"], 0)
    st = run.stats()
    assert st["kernel_variant"] == KF_TEMPERED and st["reduce_lanes"] == 1
    assert run.form_name() == ("tempered_reg" if form == "register" else "tempered_generic")
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
    # lp of every slot is the target at its x: a swap that moved x without lp (or the reverse) fails here
    _same(mhx.logdensity(model, x), lp, "lp == target(x)")
    run.close()


def _run(mhx, model, spl, n, seed, first=0, flags=0, init=None, reduce_lanes=0):
    run = mhx.Run(model, spl, nchains=n, seed=seed, first_chain=first, flags=flags, reduce_lanes=reduce_lanes)
    run.init(init)
    return run


@pytest.mark.parametrize("form", ["register", "generic"])
def test_two_sample_calls_equal_one(mhx, real, form):
    """7 + 13 samples in two calls == 19 in one: the swap rounds and their parity come from the global step (swap_every = 3 puts the
    call boundary, after transition 6, between rounds of different parity than a launch-local count would give)"""
    R, nl, d, seed = 4, 9, 2, 0xA11
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = mhx.Tempered(mhx.RWMH(mhx.MvNormal(mhx.zeros(d), 0.81 * mhx.I)), [1.0, 0.5, 0.25, 0.125], swap_every=3)
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
    R, nl, d, seed, N = 8, 12, 3, 0x5A4D, 16
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = mhx.Tempered(mhx.RWMH(mhx.MvNormal(mhx.zeros(d), 0.64 * mhx.I)), mhx.geometric_betas(R, 0.05), swap_every=1)
    whole = _run(mhx, model, spl, R * nl, seed, flags=flags)
    whole.sample(N, 0, 1, 0)
    vw, aw = whole.samples()
    k = 2
    first, n = 2 * R * k, 5 * R                             # ladders 4 .. 8
    shard = _run(mhx, model, spl, n, seed, first=first, flags=flags)
    shard.sample(N, 0, 1, 0)
    vs, as_ = shard.samples()
    _same(vs, vw[:, :, first:first + n], "shard samples")
    _same(as_, aw[:, first:first + n], "shard accepted")
    whole.close(), shard.close()


@pytest.mark.parametrize("kind", ["iso", "diag"])
@pytest.mark.parametrize("form", ["register", "generic"])
def test_unit_betas_without_swaps_are_the_plain_run(mhx, real, form, kind):
    """the plain run at ONE lane per chain (reduce_lanes = 1: the summation order of lp a tempered run has too)"""
    d, n, seed, N = 5, 70, 0xB37A, 12
    flags = mhx.FLAG_GENERIC if form == "generic" else 0
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    mv = mhx.MvNormal(mhx.zeros(d), 0.49 * mhx.I) if kind == "iso" else mhx.MvNormal(mhx.zeros(d), np.linspace(0.3, 1.2, d) ** 2)
    plain = _run(mhx, model, mhx.RWMH(mv), n, seed, first=6, flags=flags, reduce_lanes=1)
    assert plain.stats()["reduce_lanes"] in (0, 1)
    plain.sample(N, 2, 2, 0)
    assert plain.stats()["reduce_lanes"] == 1
    vp, ap = plain.samples()
    temp = _run(mhx, model, mhx.Tempered(mhx.RWMH(mv), [1.0, 1.0], swap_every=0, scales=[1.0, 1.0]), n, seed, first=6, flags=flags)
    temp.sample(N, 2, 2, 0)
    vt, at = temp.samples()
    _same(vt, vp, "samples")
    _same(at, ap, "accepted")
    for a, b in zip(plain.state(), temp.state()):
        _same(a, b, "final state")
    att, swp = temp.swap_stats()
    assert att.sum() == 0 and swp.sum() == 0
    plain.close(), temp.close()


def test_rung_snapshot_and_its_statistics(mhx, real):
    R, nl, d, seed, N = 4, 16, 2, 0x2A6, 64
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = mhx.Tempered(mhx.RWMH(mhx.MvNormal(mhx.zeros(d), mhx.I)), mhx.geometric_betas(R, 0.1), swap_every=2)
    run = _run(mhx, model, spl, R * nl, seed)
    run.sample(N, 10, 1, 0)
    value, _ = run.samples()
    for r in (0, R - 1):
        snap = run.rung(r)
        assert snap.n == nl and snap.form_name() == "derived"
        got, _ = snap.samples()
        _same(got, value[:, :, r::R], "rung %d" % r)
        # the statistics of the snapshot are the ctx forms on the same tensor
        L = mhx._lib
        h, n_saved = C.c_void_p(), C.c_int64()
        L.check(L.lib().mhx_run_device_samples(snap.h, C.byref(h), None, C.byref(n_saved)))
        assert n_saved.value == N
        idx = np.arange(d + 1, dtype=np.int32)
        ip, dp = idx.ctypes.data_as(C.POINTER(C.c_int32)), C.POINTER(C.c_double)
        ranks = np.array([0, (N * nl) // 10, (N * nl) // 2, N * nl - 1], dtype=np.int64)
        out = np.empty((d + 1, len(ranks)), dtype=np.float64)
        L.check(L.lib().mhx_ctx_order_statistics(run.ctx.h, h, N, d + 1, nl, ip, d + 1, ranks.ctypes.data_as(C.POINTER(C.c_int64)), len(ranks),
                                                 out.ctypes.data_as(dp)))
        _same(snap.order_statistics(ranks), out, "order statistics")
        _same(out, np.sort(got.transpose(1, 0, 2).reshape(d + 1, -1).astype(np.float64), axis=1)[:, ranks], "order statistics, host")
        q = snap.quantiles((0.1, 0.5, 0.9))
        assert np.allclose(q, np.quantile(got.transpose(1, 0, 2).reshape(d + 1, -1).astype(np.float64), (0.1, 0.5, 0.9), axis=1).T, rtol=1e-6)
        lower, upper = np.empty(d + 1), np.empty(d + 1)
        L.check(L.lib().mhx_ctx_hpd(run.ctx.h, h, N, d + 1, nl, ip, d + 1, 0.1, lower.ctypes.data_as(dp), upper.ctypes.data_as(dp)))
        lo, up = snap.hpd(0.1)
        _same(lo, lower, "hpd lower")
        _same(up, upper, "hpd upper")
        dg = snap.diagnostics()
        host = got.astype(np.float64)
        assert dg["n_chains"] == nl and dg["n_samples"] == N
        assert np.allclose(dg["mean"], host.mean(axis=(0, 2)), rtol=1e-5, atol=1e-5)
        assert np.allclose(dg["W"], host.var(axis=0, ddof=1).mean(axis=1), rtol=1e-4, atol=1e-5)
        snap.close()
    with pytest.raises(mhx.MhxError) as ei:
        run.rung(R)
    assert ei.value.code == mhx.MHX_EINVAL and "out of range" in str(ei.value)
    fresh = _run(mhx, model, spl, R * nl, seed)
    with pytest.raises(mhx.MhxError) as ei:
        fresh.rung(0)
    assert ei.value.code == mhx.MHX_ESTATE and "sample tensor" in str(ei.value)
    run.close(), fresh.close()


def _refused(mhx, code, words, fn):
    with pytest.raises(mhx.MhxError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def test_refusals_name_their_rule(mhx, real):
    d = 2
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    iso = mhx.MvNormal(mhx.zeros(d), mhx.I)
    EINVAL, ESTATE = mhx.MHX_EINVAL, mhx.MHX_ESTATE

    def make(betas=(1.0, 0.5), n=8, first=0, swap_every=1, scales=None, mv=iso, flags=0, reduce_lanes=0, m=model, sampler=None):
        spl = mhx.Tempered(sampler or mhx.RWMH(mv), list(betas), swap_every=swap_every, scales=scales)
        return mhx.Run(m, spl, nchains=n, seed=1, first_chain=first, flags=flags, reduce_lanes=reduce_lanes)
    _refused(mhx, EINVAL, ["R = 3", "power of two"], lambda: make(betas=(1.0, 0.5, 0.25), n=9))
    _refused(mhx, EINVAL, ["R = 128"], lambda: make(betas=mhx.geometric_betas(128, 0.01), n=128))
    _refused(mhx, EINVAL, ["R = 1"], lambda: make(betas=(1.0,), n=4))
    _refused(mhx, EINVAL, ["nchains = 9", "multiple of R"], lambda: make(n=9))
    _refused(mhx, EINVAL, ["first_chain = 3", "multiple of R"], lambda: make(first=3))
    _refused(mhx, EINVAL, ["beta[0]", "exactly 1"], lambda: make(betas=(0.9, 0.5)))
    _refused(mhx, EINVAL, ["strictly decreasing"], lambda: make(betas=(1.0, 0.5, 0.5, 0.25)))
    _refused(mhx, EINVAL, ["strictly decreasing"], lambda: make(betas=(1.0, 1.0)))               # (equal betas: only without swap rounds)
    _refused(mhx, EINVAL, ["beta[1]", "positive"], lambda: make(betas=(1.0, 0.0)))
    _refused(mhx, EINVAL, ["beta[1]", "positive"], lambda: make(betas=(1.0, -0.5)))
    _refused(mhx, EINVAL, ["scale[0]", "exactly 1"], lambda: make(scales=(1.5, 2.0)))
    _refused(mhx, EINVAL, ["scale[1]", "positive"], lambda: make(scales=(1.0, 0.0)))
    _refused(mhx, EINVAL, ["swap_every = -1"], lambda: make(swap_every=-1))
    _refused(mhx, EINVAL, ["MHX_FLAG_ZIGGURAT"], lambda: make(flags=mhx.FLAG_ZIGGURAT))
    _refused(mhx, EINVAL, ["MHX_FLAG_STATIC_PROPOSAL"], lambda: make(flags=4))
    _refused(mhx, EINVAL, ["proposal mean"], lambda: make(mv=mhx.MvNormal(np.array([0.5, 0.0]), mhx.I)))
    _refused(mhx, EINVAL, ["MHX_PROP_DENSE"], lambda: make(mv=mhx.MvNormal(mhx.zeros(d), np.array([[1.0, 0.3], [0.3, 1.0]]))))
    _refused(mhx, EINVAL, ["reduce_lanes = 2"], lambda: make(reduce_lanes=2))
    user = mhx.DensityModel(CPU.bimodal, dim=2)
    _refused(mhx, EINVAL, ["MHX_FLAG_NO_JIT", "user target"], lambda: make(m=user, flags=mhx.FLAG_NO_JIT))
    # a catalogue target without the run-time compiler: the pre-built state-in-HBM form
    run = make(flags=mhx.FLAG_NO_JIT)
    assert run.form_name() == "tempered_generic"
    run.init()
    _refused(mhx, ESTATE, ["MHX_SAVE_MOMENTS", "tempered"], lambda: run.sample(4, save="moments"))
    _refused(mhx, ESTATE, ["mhx_run_sample_to_host", "tempered", "swap"], lambda: run.sample_to_host(4))
    _refused(mhx, ESTATE, ["checkpoint", "tempered"], lambda: run.save_state())
    _refused(mhx, ESTATE, ["checkpoint", "tempered"], lambda: run.load_state(b"\0" * 128))
    g = mhx.Group([0])
    other = mhx.Run(model, mhx.Tempered(mhx.RWMH(iso), [1.0, 0.5]), nchains=8, seed=1, ctx=g.ctxs[0])
    _refused(mhx, ESTATE, ["mhx_group_attach", "tempered"], lambda: g.attach([other]))
    g.close()
    # not a tempered run
    plain = mhx.Run(model, mhx.RWMH(iso), nchains=8, seed=1)
    _refused(mhx, ESTATE, ["not a tempered run"], lambda: plain.swap_stats())
    _refused(mhx, ESTATE, ["not a tempered run"], lambda: mhx.Run.rung(plain, 0))
    plain.close(), run.close()


def test_sample_returns_the_cold_chains_and_the_swap_table(mhx, oracle, real):
    name = "r8_bimodal_user_scales"
    c = CPU.PARITY[name]
    assert c["first"] % c["R"] == 0
    ref = CPU.restated(mhx, oracle, name, real)
    model, _ = CPU.parity_model_and_target(mhx, oracle, c)
    chain = mhx.sample(model, _case_sampler(mhx, c), c["N"], c["nladders"], seed=c["seed"], first_chain=c["first"], discard_initial=c["discard"],
                       thinning=c["thinning"])
    assert chain.nchains == c["nladders"] and chain.value.shape == (c["N"], c["d"] + 1, c["nladders"])
    _same(chain.value, ref["samples"][:, :, 0::c["R"]], "cold chains")
    _same(chain.accepted, ref["accepted"][:, 0::c["R"]], "cold accepted")
    table = chain.tempered.swap_rates()
    assert [w["attempts"] for w in table] == ref["swap_attempts"].sum(axis=0).tolist()
    assert [w["swaps"] for w in table] == ref["swap_counts"].sum(axis=0).tolist()
    assert "rate" in str(table).splitlines()[0] and len(str(table).splitlines()) == c["R"]
    nT = c["discard"] + (c["N"] - 1) * c["thinning"]
    want = ref["accept_counts"].reshape(-1, c["R"]).mean(axis=0) / nT
    assert np.allclose(chain.tempered.accept_rates(), want, rtol=0, atol=1e-12)
    hot, _ = chain.tempered.rung(c["R"] - 1).samples()
    _same(hot, ref["samples"][:, :, c["R"] - 1::c["R"]], "hot rung")
    # the chain's statistics read the snapshot: they work unchanged
    assert "param_1" in str(chain.describe())
    assert np.isfinite(chain.rhat()["rhat"]).all() and len(chain.rhat("basic")["rhat"]) == c["d"]
    assert len(chain.hpd(0.1)["lower"]) == c["d"]
    host = chain.value[:, :c["d"], :].astype(np.float64)
    assert np.allclose(chain.summarystats()["mean"], host.mean(axis=(0, 2)), rtol=1e-5, atol=1e-5)
