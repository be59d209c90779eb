"""Highest-posterior-density intervals on the device (mhx_run_hpd / mhx_ctx_hpd: thresholds by the radix select, one gather sweep of
the [N][dim+1][C] tensor in place, a sort of the tails only, the first minimum width) against the numpy restatement of MCMCChains'
`_hpd` on the same draws copied back (tests/hpd_ref.py).  The order statistics are exact and the width is the same fp64 subtraction
on both sides, so lower and upper are compared with `==` (signed zeros equal; NaN rows by the rule of the header): no tolerance."""
import ctypes as C

import numpy as np
import pytest

from hpd_ref import hpd_rows, ranks, tail_counts

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
ALPHAS = (0.05, 0.5, 0.9)


def _same(got, want):
    """== with NaN where NaN is wanted"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))


def _rwmh_chain(mhx, N, C, seed=5):
    model = mhx.DensityModel(mhx.IsoGaussian(3))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(3), 1.5 * mhx.I))
    init = np.random.default_rng(seed).normal(size=(3, C))
    return mhx.sample(model, spl, N, C, initial_params=init, seed=seed)


def _ctx_hpd(mhx, ctx, ptr, shape, params, alpha):
    N, d1, Cn = shape
    params = np.ascontiguousarray(params, dtype=np.int32)
    lower, upper = np.full(len(params), SENTINEL), np.full(len(params), SENTINEL)
    dp = C.POINTER(C.c_double)
    rc = mhx.lib().mhx_ctx_hpd(ctx.h, C.c_void_p(ptr), N, d1, Cn, params.ctypes.data_as(C.POINTER(C.c_int32)), len(params), float(alpha),
                               lower.ctypes.data_as(dp), upper.ctypes.data_as(dp))
    return rc, lower, upper


def _run_hpd_raw(mhx, run, params, alpha):
    params = np.ascontiguousarray(params, dtype=np.int32)
    lower, upper = np.full(len(params), SENTINEL), np.full(len(params), SENTINEL)
    dp = C.POINTER(C.c_double)
    rc = mhx.lib().mhx_run_hpd(run.h, params.ctypes.data_as(C.POINTER(C.c_int32)), len(params), float(alpha), lower.ctypes.data_as(dp),
                               upper.ctypes.data_as(dp))
    return rc, mhx.lib().mhx_last_error().decode(), lower, upper


# ---- 1. real chains: rejected steps repeat draws, so ties at the thresholds are the normal case ----
# The quantile tests' shapes, and (17, 241): S = 4097 is the smallest S at which the gather launches two blocks per row in both
# widths -- a block's unrolled sweep is 512 threads x 8 fp32 (x 4 fp64) draws = 4096 (2048), and the grid is ceil(S / sweep) blocks
# per row while that is below 2048 / rows.  The argmin gives a block 1024 candidates: at alpha = 0.5 (m = 2049, cL + cU + 1
# candidates) and at 0.9 (overlapping tails: all m = 3688 are candidates) it launches at least two per row there as well.
@pytest.mark.parametrize("N,C", [(33, 67), (1000, 1), (5, 3), (2, 257), (1, 64), (17, 241)])
def test_hpd_of_real_chains(mhx, real, N, C):
    chain = _rwmh_chain(mhx, N, C)
    S = N * C
    if S >= 500:
        assert 0.0 < chain.accepted[1:].mean() < 1.0        # some rejected steps: repeated draws
    one, all_but_one = 0.5 / S, (S - 1.5) / S
    assert ranks(S, one) == 1 and ranks(S, all_but_one) == S - 1 and mhx.hpd_ranks(S, all_but_one) == S - 1
    if S == 4097:
        for alpha in (0.5, 0.9):
            for p in range(4):
                m, cL, cU = tail_counts(chain.value[:, p, :], alpha)
                assert cL + (1 if cL < m - cU else 0) + (m - max(cL, m - cU)) > 1024       # two argmin blocks in every row
    for alpha in ALPHAS + (one, all_but_one):
        lower, upper = chain.state.hpd(alpha)               # all dim + 1 rows, lp included
        assert lower.shape == upper.shape == (4,) and lower.dtype == upper.dtype == np.float64
        wl, wu = hpd_rows(chain.value, alpha)
        assert _same(lower, wl) and _same(upper, wu), (alpha, lower, wl, upper, wu)
    # a subset of the rows, in another order
    lower, upper = chain.state.hpd(0.5, params=[3, 1])
    wl, wu = hpd_rows(chain.value, 0.5)
    assert _same(lower, wl[[3, 1]]) and _same(upper, wu[[3, 1]])
    chain.state.close()


# ---- 2. crafted tensors through mhx_ctx_hpd on a torch tensor ----
ROWS = ("all equal", "two values", "permutation", "signed zeros", "+inf fills the upper tail", "a few +inf", "a few -inf", "one NaN",
        "ties at both thresholds, cL = cU = 0", "discrete: ties at the thresholds")


def _crafted(dt, rng, N, Cn):
    S = N * Cn
    rows = [np.full(S, 3.25),
            rng.choice([1.0, 2.0], size=S),
            rng.permutation(S).astype(np.float64),
            rng.choice([-0.0, 0.0], size=S),
            np.where(np.arange(S) < (6 * S) // 10, np.inf, rng.normal(size=S)),       # 60 %: +inf reaches a as well at alpha >= 0.5
            np.where(np.arange(S) < S // 10, np.inf, rng.normal(size=S)),
            np.where(np.arange(S) < S // 10, -np.inf, rng.normal(size=S)),
            rng.normal(size=S),
            np.where(np.arange(S) < (4 * S) // 10, -1.0, np.where(np.arange(S) < (8 * S) // 10, 1.0, rng.uniform(-0.5, 0.5, size=S))),
            np.round(rng.normal(size=S) * 2.0) / 2.0]
    rows[7][S // 3] = np.nan
    t = np.stack([rng.permutation(r).astype(dt).reshape(N, Cn) for r in rows], axis=1)
    return np.ascontiguousarray(t)                          # [N][10][C]


@pytest.fixture
def crafted(mhx, real):
    import torch
    dt = mhx._lib.NP_DTYPES[real]
    shape = (7, len(ROWS), 65)
    host = _crafted(dt, np.random.default_rng(11), shape[0], shape[2])
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    yield host, dev, shape, mhx.Context.default(dtype=real)
    del dev


@pytest.mark.parametrize("alpha", [0.05, 0.3, 0.5, 0.9])
def test_hpd_of_crafted_tensors(mhx, real, crafted, alpha):
    host, dev, shape, ctx = crafted
    S = shape[0] * shape[2]
    assert np.isnan(host[:, 7, :]).sum() == 1 and np.isnan(host).sum() == 1
    m = ranks(S, alpha)
    assert tail_counts(host[:, 8, :], alpha)[1:] == (0, 0) or alpha > 0.4      # row 8: nothing strictly beyond either threshold
    if alpha == 0.5:                                       # row 4: b is all +inf and +inf reaches a -- NaN widths, the first of them wins
        y = np.sort(host[:, 4, :].ravel().astype(np.float64))
        assert np.all(np.isinf(y[S - m:])) and np.isinf(y[m - 1])
    rc, lower, upper = _ctx_hpd(mhx, ctx, dev.data_ptr(), shape, np.arange(len(ROWS)), alpha)
    mhx.check(rc)
    wl, wu = hpd_rows(host, alpha)
    for r, what in enumerate(ROWS):
        assert _same(lower[r], wl[r]) and _same(upper[r], wu[r]), (what, alpha, lower[r], wl[r], upper[r], wu[r])
    assert np.isnan(lower[7]) and np.isnan(upper[7]) and not np.isnan(np.delete(lower, 7)).any() and not np.isnan(np.delete(upper, 7)).any()
    assert lower[3] == 0.0 and upper[3] == 0.0              # either zero
    if alpha >= 0.5:
        assert lower[4] == np.inf and upper[4] == np.inf
    # the neighbours of the NaN row answer alone as they do beside it
    rc, lo2, up2 = _ctx_hpd(mhx, ctx, dev.data_ptr(), shape, [6, 8], alpha)
    mhx.check(rc)
    assert _same(lo2, lower[[6, 8]]) and _same(up2, upper[[6, 8]])


# ---- 3. reproducibility; repeated rows in non-ascending order ----
def test_two_calls_return_the_same_bits(mhx, real, crafted):
    host, dev, shape, ctx = crafted
    params = [9, 2, 2, 0, 5, 9, 1]
    rc, lo1, up1 = _ctx_hpd(mhx, ctx, dev.data_ptr(), shape, params, 0.3)
    mhx.check(rc)
    rc, lo2, up2 = _ctx_hpd(mhx, ctx, dev.data_ptr(), shape, params, 0.3)
    mhx.check(rc)
    assert np.array_equal(lo1.view(np.uint64), lo2.view(np.uint64)) and np.array_equal(up1.view(np.uint64), up2.view(np.uint64))
    wl, wu = hpd_rows(host, 0.3)
    assert _same(lo1, wl[params]) and _same(up1, wu[params])


# ---- 4. batching: option HPD_SCRATCH_MB ----
def test_rows_in_batches_give_the_same_intervals(mhx, real, engine):
    """a row in flight holds 4 (m - 1) keys (two tails, each with the buffer it is sorted into); the sort's own space comes on top.
    A budget of 2.6 such rows cannot hold three, so the four rows of the call go in at least two batches; 0.9 rows hold none."""
    chain = _rwmh_chain(mhx, 130, 257)
    S, alpha = 130 * 257, 0.5
    row_mb = 4.0 * (ranks(S, alpha) - 1) * {"f32": 4, "f64": 8}[real] / 2.0 ** 20
    want = chain.state.hpd(alpha)
    wl, wu = hpd_rows(chain.value, alpha)
    assert _same(want[0], wl) and _same(want[1], wu)
    engine.set("HPD_SCRATCH_MB", "%.6f" % (2.6 * row_mb))
    got = chain.state.hpd(alpha)
    assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
    engine.set("HPD_SCRATCH_MB", "%.6f" % (0.9 * row_mb))
    rc, msg, lower, upper = _run_hpd_raw(mhx, chain.state, [0, 1], alpha)
    assert rc == mhx.MHX_EINVAL and "HPD_SCRATCH_MB" in msg and "mhx_run_hpd" in msg, (rc, msg)
    assert np.all(lower == SENTINEL) and np.all(upper == SENTINEL)
    with pytest.raises(mhx.ArgumentError, match="HPD_SCRATCH_MB"):
        chain.state.hpd(alpha)
    engine.set("HPD_SCRATCH_MB", "0")
    with pytest.raises(mhx.ArgumentError, match="HPD_SCRATCH_MB"):
        chain.state.hpd(alpha)
    chain.state.close()


# ---- 5. the Python surface ----
def test_python_surface(mhx, real):
    data = np.random.default_rng(1234).normal(0.0, 1.0, size=30)
    model = mhx.DensityModel(mhx.IIDNormal(data))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(2), 0.25 * mhx.I))
    chain = mhx.sample(model, spl, 120, 64, param_names=["mu", "sigma"], discard_initial=50, initial_params=np.array([0.0, 1.0]), seed=1234)
    run = chain.state
    lower, upper = run.hpd(0.05)
    wl, wu = hpd_rows(chain.value, 0.05)
    assert _same(lower, wl) and _same(upper, wu) and lower.shape == (3,)
    # the ctx entry on the run's own device tensor
    ptr, n_saved = C.c_void_p(), C.c_int64()
    mhx.check(mhx.lib().mhx_run_device_samples(run.h, C.byref(ptr), None, C.byref(n_saved)))
    assert n_saved.value == 120
    rc, cl, cu = _ctx_hpd(mhx, run.ctx, ptr.value, (120, 3, 64), [0, 1, 2], 0.05)
    mhx.check(rc)
    assert np.array_equal(cl, lower) and np.array_equal(cu, upper)
    # the named table: the parameters without lp, the default alpha, the numbers of Run.hpd on the same rows
    t = chain.hpd()
    assert t["parameters"] == ["mu", "sigma"] == chain.params() and t["alpha"] == 0.05
    assert np.array_equal(t["lower"], lower[:2]) and np.array_equal(t["upper"], upper[:2])
    lines = str(t).split("\n")
    assert lines[0] == "HPD (95%)" and lines[1].split() == ["parameters", "lower", "upper"] and len(lines) == 4
    for i, name in enumerate(["mu", "sigma"]):
        assert lines[2 + i].split() == [name, "%.4f" % lower[i], "%.4f" % upper[i]]
    t2 = chain.hpd(alpha=0.5)
    r2 = run.hpd(0.5, params=[0, 1])
    assert np.array_equal(t2["lower"], r2[0]) and np.array_equal(t2["upper"], r2[1]) and np.all(t2["upper"] - t2["lower"] < upper[:2] - lower[:2])
    bare = mhx.Chains(chain.value, chain.names, chain.start, chain.thin)
    with pytest.raises(mhx.ArgumentError, match="hpd needs the live run"):
        bare.hpd()
    run.close()


# ---- 6. refusals: an mhx error that names the entry point, nothing written to lower / upper ----
def test_refusals(mhx, real):
    chain = _rwmh_chain(mhx, 9, 10)
    run, d1 = chain.state, 4
    rc, msg, lower, upper = _run_hpd_raw(mhx, run, [0, 3], 0.2)
    assert rc == 0 and not np.any(lower == SENTINEL) and not np.any(upper == SENTINEL)
    ptr, n_saved = C.c_void_p(), C.c_int64()
    mhx.check(mhx.lib().mhx_run_device_samples(run.h, C.byref(ptr), None, C.byref(n_saved)))
    for alpha in (0.0, 1.0, -0.1, 1.5, float("nan")):
        rc, msg, lower, upper = _run_hpd_raw(mhx, run, [0, 1], alpha)
        assert rc == mhx.MHX_EINVAL and "mhx_run_hpd" in msg, (alpha, rc, msg)
        assert np.all(lower == SENTINEL) and np.all(upper == SENTINEL)
        rc, lower, upper = _ctx_hpd(mhx, run.ctx, ptr.value, (9, d1, 10), [0, 1], alpha)
        assert rc == mhx.MHX_EINVAL and "mhx_ctx_hpd" in mhx.lib().mhx_last_error().decode()
        assert np.all(lower == SENTINEL) and np.all(upper == SENTINEL)
        with pytest.raises(mhx.ArgumentError, match="mhx_run_hpd"):
            run.hpd(alpha)
    for params in ([d1], [0, d1], [-1]):
        rc, msg, lower, upper = _run_hpd_raw(mhx, run, params, 0.05)
        assert rc == mhx.MHX_EINVAL and "mhx_run_hpd" in msg, (params, rc, msg)
        assert np.all(lower == SENTINEL) and np.all(upper == SENTINEL)
        rc, lower, upper = _ctx_hpd(mhx, run.ctx, ptr.value, (9, d1, 10), params, 0.05)
        assert rc == mhx.MHX_EINVAL and np.all(lower == SENTINEL) and np.all(upper == SENTINEL)
    # moments mode keeps no sample tensor (the shape of tests/test_gpu_quantiles.py)
    dm, Cm = 40, 96
    s = float(np.float32(2.38 / dm ** 0.5))
    mom = mhx.Run(mhx.DensityModel(mhx.Funnel(dm)), mhx.RWMH(mhx.MvNormal(mhx.zeros(dm), s * s * mhx.I)), nchains=Cm, seed=2)
    mom.init(np.random.default_rng(8).normal(size=(dm, Cm)))
    mom.sample(10, 5, 5, 0, save="moments")
    rc, msg, lower, upper = _run_hpd_raw(mhx, mom, [0], 0.05)
    assert rc == mhx.MHX_ESTATE and "mhx_run_hpd" in msg and np.all(lower == SENTINEL) and np.all(upper == SENTINEL)
    with pytest.raises(mhx.MhxError, match="mhx_run_hpd"):
        mom.hpd()
    mom.close()
    run.close()
