"""Exact chain quantiles on the device (mhx_run / mhx_ctx / mhx_group_order_statistics: a histogram radix select over the
[N][dim+1][C] tensor in place) against numpy's sort of the same draws.  Order statistics are compared EXACTLY, by value
(`np.array_equal(..., equal_nan=True)`: -0.0 == +0.0, NaNs last); quantiles within the rounding of the two interpolation
formulas.  What MCMCChains prints as "Quantiles" for the reference's chains (README.md:65-71)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)


def _ranks(S):
    """the extremes, the middle, and the floor / ceil ranks of the default probs: unsorted, with a repeat"""
    r = {0, min(1, S - 1), max(S // 2 - 1, 0), S // 2, max(S - 2, 0), S - 1}
    for p in PROBS:
        h = (S - 1) * p
        r |= {int(np.floor(h)), min(int(np.floor(h)) + 1, S - 1)}
    r = sorted(r)
    return np.array(r[::-1] + [r[len(r) // 2]], dtype=np.int64)


def _sorted_rows(value):
    """[d1][S] float64: every parameter's draws in ascending order (numpy: NaNs last)"""
    v = np.asarray(value)
    return np.sort(np.moveaxis(v, 1, 0).reshape(v.shape[1], -1).astype(np.float64), axis=1)


def _rwmh_chain(mhx, N, C, seed=5):
    model = mhx.DensityModel(mhx.IsoGaussian(3))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(3), 1.5 * mhx.I))
    init = np.random.default_rng(seed).normal(size=(3, C))
    return mhx.sample(model, spl, N, C, initial_params=init, seed=seed)


# ---- 1. real chains: rejected steps repeat rows (ties), C is not a multiple of the wave; C = 1 with many draws; tiny shapes ----
@pytest.mark.parametrize("N,C", [(33, 67), (1000, 1), (5, 3), (2, 257), (1, 64)])
def test_order_statistics_of_real_chains(mhx, real, N, C):
    chain = _rwmh_chain(mhx, N, C)
    S = N * C
    if N * C >= 500:
        assert 0.0 < chain.accepted[1:].mean() < 1.0        # some rejected steps: repeated draws
    want = _sorted_rows(chain.value)
    ranks = _ranks(S)
    got = chain.state.order_statistics(ranks)               # all dim + 1 rows, lp included
    assert got.shape == (4, len(ranks)) and got.dtype == np.float64
    assert np.array_equal(got, want[:, ranks], equal_nan=True)
    # a subset of the rows, in another order
    got = chain.state.order_statistics([S - 1, 0], params=[3, 1])
    assert np.array_equal(got, want[[3, 1]][:, [S - 1, 0]])
    chain.state.close()


# ---- 2. crafted tensors: each digit position decides alone; every rank asked for (internal batching of ranks) ----
def _crafted(dt, rng, N, C):
    S = N * C
    fi = np.finfo(dt)
    one = dt(1.0)
    steps = [one]
    for _ in range(S // 2):                                  # nextafter steps around 1.0: only the lowest mantissa bits differ
        steps.append(np.nextafter(steps[-1], dt(2.0), dtype=dt))
    lo = one
    while len(steps) < S:
        lo = np.nextafter(lo, dt(0.0), dtype=dt)
        steps.append(lo)
    a = rng.permutation(np.array(steps, dtype=dt))
    sub = np.nextafter(dt(0.0), dt(1.0), dtype=dt)           # the smallest subnormal
    pool = [np.inf, -np.inf, fi.max, -fi.max, fi.tiny, -fi.tiny, sub, -sub, sub * dt(4.0), 0.0, -0.0]
    pool += [s * 2.0 ** k for k in range(-24, 25, 4) for s in (1.0, -1.0)]
    b = rng.choice(np.array(pool, dtype=dt), size=S)
    b[:len(pool)] = np.array(pool, dtype=dt)                 # every one of them at least once
    c = np.full(S, dt(3.25))
    d = rng.normal(size=S).astype(dt)
    d[[5, S // 2, S - 1]] = [np.nan, -np.nan, np.nan]        # both signs of NaN: all of them order last
    d[7] = np.inf
    t = np.stack([rng.permutation(r).reshape(N, C) for r in (a, b, c, d)], axis=1)
    return np.ascontiguousarray(t)                           # [N][4][C]


def _ctx_order_statistics(mhx, ctx, dev_tensor, shape, params, ranks):
    N, d1, Cn = shape
    params = np.ascontiguousarray(params, dtype=np.int32)
    ranks = np.ascontiguousarray(ranks, dtype=np.int64)
    out = np.full((len(params), len(ranks)), -12345.0)
    rc = mhx.lib().mhx_ctx_order_statistics(ctx.h, C.c_void_p(dev_tensor.data_ptr()), N, d1, Cn,
                                            params.ctypes.data_as(C.POINTER(C.c_int32)), len(params),
                                            ranks.ctypes.data_as(C.POINTER(C.c_int64)), len(ranks),
                                            out.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, out


def test_every_rank_of_crafted_tensors(mhx, real):
    import torch
    dt = mhx._lib.NP_DTYPES[real]
    N, d1, Cn = 7, 4, 65
    S = N * Cn
    host = _crafted(dt, np.random.default_rng(11), N, Cn)
    assert np.isnan(host[:, 3, :]).sum() == 3
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    ctx = mhx.Context.default(dtype=real)
    ranks = np.random.default_rng(12).permutation(S)         # all 455 ranks: 15 internal batches of 32
    rc, got = _ctx_order_statistics(mhx, ctx, dev, (N, d1, Cn), [0, 1, 2, 3], ranks)
    mhx.check(rc)
    want = _sorted_rows(host)
    for row, what in enumerate(("lowest mantissa bits", "sign / exponent", "all equal", "three NaNs")):
        assert np.array_equal(got[row], want[row, ranks], equal_nan=True), what
    assert np.isnan(got[3, np.argsort(ranks)][-3:]).all() and not np.isnan(got[3, np.argsort(ranks)][:-3]).any()
    assert np.isfinite(got[0]).all() and len(np.unique(got[0])) == S
    # refusals of this entry point: the name, and nothing written
    for bad_params, bad_ranks in (([0], [S]), ([0], [-1]), ([d1], [0]), ([-1], [0])):
        rc, out = _ctx_order_statistics(mhx, ctx, dev, (N, d1, Cn), bad_params, bad_ranks)
        assert rc == mhx.MHX_EINVAL and "mhx_ctx_order_statistics" in mhx.lib().mhx_last_error().decode()
        assert np.all(out == -12345.0)


@pytest.mark.parametrize("bits", [5, 8, 10])
def test_every_digit_width_selects_the_same_draws(mhx, real, engine, bits):
    """option SELECT_BITS: the other pre-built forms of the kernel (8 and 10 bit digits, 16 groups per launch) and a width that
    leaves a short last digit"""
    chain = _rwmh_chain(mhx, 33, 67)
    ranks = np.arange(0, 33 * 67, 53)                        # 42 ranks: two batches, more groups than one launch holds
    want = chain.state.order_statistics(ranks)
    assert np.array_equal(want, _sorted_rows(chain.value)[:, ranks])
    engine.set("SELECT_BITS", bits)
    assert np.array_equal(chain.state.order_statistics(ranks), want)
    engine.set("SELECT_BITS", 12)
    with pytest.raises(mhx.ArgumentError, match="mhx_run_order_statistics"):
        chain.state.order_statistics(ranks)
    chain.state.close()


# ---- 3. quantiles ----
def test_quantiles_are_numpys(mhx, real):
    chain = _rwmh_chain(mhx, 33, 67)
    S = 33 * 67
    got = chain.state.quantiles()
    assert got.shape == (4, 5) and got.dtype == np.float64
    srt = _sorted_rows(chain.value)
    for p in range(4):
        x64 = chain.value[:, p, :].astype(np.float64).ravel()
        want = np.quantile(x64, PROBS, method="linear")
        for k, pr in enumerate(PROBS):
            j = int(np.floor((S - 1) * pr))
            lo, hi = srt[p, j], srt[p, min(j + 1, S - 1)]
            # at most three rounded float64 operations on operands bounded by 2 max(|lo|, |hi|) in either formula
            bound = 8.0 * 2.0 ** -52 * max(abs(lo), abs(hi))
            err = abs(got[p, k] - want[k])
            print("param %d prob %.3f: |mhx - numpy| = %.3e, bound %.3e" % (p, pr, err, bound))
            assert err <= bound
    ext = chain.state.quantiles((0, 1))
    assert np.array_equal(ext[:, 0], srt[:, 0]) and np.array_equal(ext[:, 1], srt[:, -1])      # exact min and max
    q = chain.quantile()
    assert q["parameters"] == chain.params() and np.array_equal(q["quantiles"], got[:3])       # lp left out
    chain.state.close()


# ---- 4. a group: the union of unequal shards ----
def test_group_order_statistics_pool_all_members(mhx, real):
    d, Cn, N = 3, 67, 21
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(d), 1.5 * mhx.I))
    init = np.random.default_rng(3).normal(size=(d, Cn))
    g = mhx.Group([0, 0, 0])
    g.create(model, spl, nchains=Cn, seed=11, first_chain=5)
    assert sorted(r.n for r in g.runs) == [22, 22, 23]
    g.init(init)
    g.sample(N)
    gathered = np.concatenate([r.samples()[0] for r in g.runs], axis=2)
    S = N * Cn
    ranks = _ranks(S)
    want = _sorted_rows(gathered)
    got = g.order_statistics(ranks)
    assert np.array_equal(got, want[:, ranks])
    whole = mhx.Run(model, spl, nchains=Cn, seed=11, first_chain=5)
    whole.init(init)
    whole.sample(N)
    assert np.array_equal(whole.order_statistics(ranks), got)
    assert np.array_equal(g.quantiles(), whole.quantiles())
    assert np.array_equal(g.order_statistics(np.arange(S), params=[d])[0], want[d])            # every rank of lp
    with pytest.raises(mhx.ArgumentError, match="mhx_group_order_statistics"):
        g.order_statistics([S])
    with pytest.raises(mhx.ArgumentError, match="mhx_group_order_statistics"):
        g.order_statistics([0], params=[d + 1])
    g.close()
    whole.close()


# ---- 5. the two tables of the reference's README ----
def test_describe_prints_both_tables(mhx, real):
    data = np.random.default_rng(1234).normal(0.0, 1.0, size=30)
    model = mhx.DensityModel(mhx.IIDNormal(data))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(2), 0.25 * mhx.I))
    chain = mhx.sample(model, spl, 120, 64, param_names=["mu", "sigma"], discard_initial=50, initial_params=np.array([0.0, 1.0]), seed=1234)
    text = chain.describe()
    lines = text.split("\n")
    assert "Summary Statistics" in lines and "Quantiles" in lines
    st, qt = chain.summarystats(), chain.quantile()
    assert qt["parameters"] == ["mu", "sigma"] == st["parameters"] and qt["quantiles"].shape == (2, 5)
    srt = _sorted_rows(chain.value)
    S = 120 * 64
    for i in range(2):
        x64 = chain.value[:, i, :].astype(np.float64).ravel()
        np.testing.assert_allclose(qt["quantiles"][i], np.quantile(x64, PROBS), rtol=1e-14, atol=0)
        assert srt[i, 0] < qt["quantiles"][i, 0] < qt["quantiles"][i, 2] < qt["quantiles"][i, 4] < srt[i, -1]
    head = lines[lines.index("Summary Statistics") + 1].split()
    assert head == ["parameters", "mean", "std", "naive_se", "mcse", "ess_bulk", "ess_tail", "rhat"]
    qhead = lines[lines.index("Quantiles") + 1].split()
    assert qhead == ["parameters", "2.5%", "25.0%", "50.0%", "75.0%", "97.5%"]
    for i, name in enumerate(["mu", "sigma"]):
        srow = lines[lines.index("Summary Statistics") + 2 + i].split()
        qrow = lines[lines.index("Quantiles") + 2 + i].split()
        assert srow[0] == name and qrow[0] == name
        assert qrow[1:] == ["%.4f" % q for q in qt["quantiles"][i]]
        mcse = st["std"][i] / np.sqrt(st["ess_bulk"][i])
        assert srow[4] == "%.4f" % mcse and srow[3] == "%.4f" % (st["std"][i] / np.sqrt(S))
        assert srow[1] == "%.4f" % st["mean"][i] and srow[2] == "%.4f" % st["std"][i]
    # repr is what it was: the summarystats table, no quantiles
    rep = repr(chain)
    assert "Quantiles" not in rep and "naive_se" not in rep
    rl = rep.split("\n")
    assert rl[1].split() == ["parameters", "mean", "std", "ess_bulk", "ess_tail", "rhat"] and len(rl) == 4
    for i, name in enumerate(["mu", "sigma"]):
        assert rl[2 + i] == "  %-12s %9.4f %9.4f %10.1f %10.1f %9.4f" % (name, st["mean"][i], st["std"][i], st["ess_bulk"][i],
                                                                        st["ess_tail"][i], st["rhat"][i])
    # a container without its live run cannot select anything
    bare = mhx.Chains(chain.value, chain.names, chain.start, chain.thin)
    with pytest.raises(mhx.ArgumentError, match="quantile needs the live run"):
        bare.quantile()
    chain.state.close()


# ---- 6. refusals: an mhx error that names the entry point, nothing written to out ----
def test_refusals(mhx, real):
    chain = _rwmh_chain(mhx, 9, 10)
    run, S, d1 = chain.state, 90, 4
    lib = mhx.lib()

    def call(params, ranks, run=run):
        params, ranks = np.array(params, dtype=np.int32), np.array(ranks, dtype=np.int64)
        out = np.full((len(params), len(ranks)), -12345.0)
        rc = lib.mhx_run_order_statistics(run.h, params.ctypes.data_as(C.POINTER(C.c_int32)), len(params),
                                          ranks.ctypes.data_as(C.POINTER(C.c_int64)), len(ranks), out.ctypes.data_as(C.POINTER(C.c_double)))
        return rc, lib.mhx_last_error().decode(), out

    rc, msg, out = call([0, 1], [0, S - 1])
    assert rc == 0 and not np.any(out == -12345.0)
    for params, ranks in (([0], [3, -1]), ([0], [S]), ([d1], [0])):
        rc, msg, out = call(params, ranks)
        assert rc == mhx.MHX_EINVAL and "mhx_run_order_statistics" in msg, (rc, msg)
        assert np.all(out == -12345.0)
        with pytest.raises(mhx.ArgumentError, match="mhx_run_order_statistics"):
            run.order_statistics(ranks, params=params)
    for bad in (1.5, -0.5, [0.5, 1.5]):
        with pytest.raises(mhx.ArgumentError, match="quantiles: probs must lie in"):
            run.quantiles(bad)
    # moments mode keeps no sample tensor (a run whose kernel keeps running moments: the shape of test_gpu_group.py)
    dm, Cm = 40, 96
    s = float(np.float32(2.38 / dm ** 0.5))
    mom = mhx.Run(mhx.DensityModel(mhx.Funnel(dm)), mhx.RWMH(mhx.MvNormal(mhx.zeros(dm), s * s * mhx.I)), nchains=Cm, seed=2)
    mom.init(np.random.default_rng(8).normal(size=(dm, Cm)))
    mom.sample(10, 5, 5, 0, save="moments")
    rc, msg, out = call([0], [0], run=mom)
    assert rc == mhx.MHX_ESTATE and "mhx_run_order_statistics" in msg and np.all(out == -12345.0)
    with pytest.raises(mhx.MhxError, match="mhx_run_order_statistics"):
        mom.quantiles()
    mom.close()
    # ... nor does save = False; one saved draw is enough
    run.sample(10, save=False)
    with pytest.raises(mhx.MhxError, match="mhx_run_order_statistics"):
        run.order_statistics([0])
    run.sample(1)
    v = run.samples()[0]
    assert np.array_equal(run.order_statistics([0, 9]), _sorted_rows(v)[:, [0, 9]])
    run.close()
