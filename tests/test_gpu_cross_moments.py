"""Posterior cross moments, covariance and correlation on the device (mhx_ctx / mhx_run / mhx_group_cross_moments: a SYRK over all
draws on the fp64 matrix cores, reading the [N][dim+1][C] tensor in place) against exact sums of the same draws.

The tolerance is derived, not measured (tests/cross_moments_ref.py): |got - exact| <= gamma_K * sum_k |y_ik y_jk| entrywise.
Measured on an MI355X (every case prints its figure before it asserts) the largest error / bound was 0.55 at K = 1 (one rounded
product against gamma_1 = u) and 0.14 over the other shapes; the covariances of the real chains err by 1e-16 against tolerances of
1e-13."""
import ctypes as C

import numpy as np
import pytest

from cross_moments_ref import Moments, shifted_rows

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (5, 4, 3), (33, 4, 67), (2, 16, 257), (3, 17, 64), (7, 48, 130), (2, 113, 70), (2, 1001, 70), (1000, 2, 1)]
DP = C.POINTER(C.c_double)


def _ctx_cross_moments(mhx, ctx, dev_tensor, shape, params, shift):
    N, d1, Cn = shape
    params = np.ascontiguousarray(params, dtype=np.int32)
    m = len(params)
    shift = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    s, x = np.full(m, -12345.0), np.full((m, m), -12345.0)
    rc = mhx.lib().mhx_ctx_cross_moments(ctx.h, C.c_void_p(dev_tensor.data_ptr()), N, d1, Cn, params.ctypes.data_as(C.POINTER(C.c_int32)), m,
                                         None if shift is None else shift.ctypes.data_as(DP), s.ctypes.data_as(DP), x.ctypes.data_as(DP))
    return rc, s, x


def _subset(rng, d1):
    """a permuted subset of the rows with one repeat"""
    k = max(1, (2 * d1) // 3)
    idx = rng.permutation(d1)[:k]
    return np.concatenate([idx, idx[:1]]).astype(np.int32)


def _tensor(kind, dt, rng, shape):
    N, d1, Cn = shape
    if kind == "normal":                                     # scaled per row by 2^+-20, so that a mis-mapped row shows
        t = rng.normal(size=shape) * (2.0 ** rng.integers(-20, 21, size=d1))[None, :, None]
        return np.ascontiguousarray(t.astype(dt))
    t = np.zeros(shape, dtype=dt)
    if kind == "spike_last":
        t[N - 1, d1 - 1, Cn - 1] = 1.0
    elif kind == "spike_first":
        t[0, 0, 0] = 1.0
    else:                                                    # "nonfinite": one row with a NaN, one row with a +Inf
        t = np.ascontiguousarray((rng.normal(size=shape) * (2.0 ** rng.integers(-20, 21, size=d1))[None, :, None]).astype(dt))
        t[N // 2, d1 - 1, Cn // 2] = np.nan
        if d1 > 1:
            t[N - 1, 0, Cn - 1] = np.inf
    return t


# ---- 1. crafted tensors through the raw-tensor entry point ----
@pytest.mark.parametrize("kind", ["normal", "spike_last", "spike_first", "nonfinite"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_crafted_tensors(mhx, real, shape, kind):
    import torch
    dt = mhx._lib.NP_DTYPES[real]
    N, d1, Cn = shape
    rng = np.random.default_rng([N, d1, Cn, len(kind)])
    host = _tensor(kind, dt, rng, shape)
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    ctx = mhx.Context.default(dtype=real)
    every = np.arange(d1, dtype=np.int32)
    sub = _subset(rng, d1)
    for shift in (None, rng.normal(size=d1) * 3.0):
        ref = Moments(shifted_rows(host, every, shift))      # once per shift: a subset's moments are a subset of these
        for params in (every, sub):
            whole = params is every
            label = "%s %s shift=%s rows=%s" % (shape, kind, "0" if shift is None else "random", "all" if whole else list(params[:8]))
            rc, s, x = _ctx_cross_moments(mhx, ctx, dev, shape, params, None if shift is None else shift[params])
            mhx.check(rc)
            assert np.array_equal(x, x.T, equal_nan=True), label + ": cross is not symmetric"
            worst = (ref if whole else ref.subset(params)).check(s, x, label)
            print("%s: largest error / bound %.3e" % (label, worst))
            rc, s2, x2 = _ctx_cross_moments(mhx, ctx, dev, shape, params, None if shift is None else shift[params])
            mhx.check(rc)
            assert np.array_equal(s2, s, equal_nan=True) and np.array_equal(x2, x, equal_nan=True), label + ": not deterministic"
            if shift is None and kind.startswith("spike") and whole:
                want = np.zeros((d1, d1))
                at = d1 - 1 if kind == "spike_last" else 0
                want[at, at] = 1.0
                assert np.array_equal(x, want) and np.array_equal(s, want[at]), label
            if kind == "nonfinite" and whole:
                bad = np.zeros(d1, dtype=bool)
                bad[d1 - 1] = True
                bad[0] |= d1 > 1
                assert np.array_equal(~np.isfinite(s), bad) and np.array_equal(~np.isfinite(x), bad[:, None] | bad[None, :]), label


# ---- 2. real chains ----
def _rwmh_chain(mhx, N, Cn, seed=5):
    model = mhx.DensityModel(mhx.IsoGaussian(3))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(3), 1.5 * mhx.I))
    init = np.random.default_rng(seed).normal(size=(3, Cn))
    return mhx.sample(model, spl, N, Cn, initial_params=init, seed=seed)


def _ensemble_chain(mhx):
    d, W = 3, 10
    Sig = 0.5 * np.eye(d) + 0.5
    init = np.random.default_rng(9).normal(size=(d, W))
    spl = mhx.Ensemble(W, mhx.StretchProposal(mhx.MvNormal(mhx.zeros(d), mhx.I)))
    return mhx.sample(mhx.DensityModel(mhx.CorrGaussian(Sig)), spl, 16, seed=21, initial_params=init)


def _ram_chain(mhx):
    Sig = np.array([[1.0, 0.5], [0.5, 1.0]])
    return mhx.sample(mhx.DensityModel(mhx.CorrGaussian(Sig)), mhx.RobustAdaptiveMetropolis(), 40, 7, seed=42, num_warmup=40,
                      initial_params=np.zeros(2))


@pytest.mark.parametrize("which", ["rwmh-33x67", "rwmh-5x3", "rwmh-2x257", "ensemble", "ram"])
def test_moments_and_covariance_of_real_chains(mhx, real, which):
    if which.startswith("rwmh"):
        N, Cn = map(int, which.split("-")[1].split("x"))
        chain = _rwmh_chain(mhx, N, Cn)
    else:
        chain = _ensemble_chain(mhx) if which == "ensemble" else _ram_chain(mhx)
    N, d1, Cn = chain.value.shape
    d = d1 - 1
    run = chain.state
    n, shift, s, x = run.cross_moments()
    assert n == N * Cn and shift.shape == (d1,) and np.isfinite(shift).all()
    # the default shift: the mean over the chains of saved sample 0
    np.testing.assert_allclose(shift, chain.value[0].astype(np.float64).mean(axis=1), rtol=0, atol=1e-12 * np.abs(chain.value[0]).max())
    ref = Moments(shifted_rows(chain.value, np.arange(d1), shift))
    assert ref.exact
    print("%s: moments, largest error / bound %.3e" % (which, ref.check(s, x, which)))
    assert np.array_equal(x, x.T)
    cov, tol = ref.covariance()
    got = run.cov()
    from fractions import Fraction
    for i in range(d1):
        for j in range(d1):
            err = abs(Fraction(float(got[i, j])) - cov[i][j])
            print("%s cov[%d][%d]: error %.3e, tolerance %.3e" % (which, i, j, err, tol[i][j]))
            assert err <= tol[i][j]
    assert chain.cov().shape == (d, d) and np.array_equal(chain.cov(), got[:d, :d])
    assert chain.cov(include_lp=True).shape == (d1, d1)
    cor = chain.cor()
    assert cor.shape == (d, d) and np.abs(np.diagonal(cor) - 1.0).max() <= 4 * 2.0 ** -53
    assert np.abs(cor).max() <= 1.0 and np.array_equal(np.asarray(cor), np.asarray(cor).T)
    text = str(cor)
    assert text.split("\n")[0] == "Correlation" and all(nm in text for nm in chain.params()) and "lp" not in text
    assert chain.cor(include_lp=True).shape == (d1, d1) and "lp" in str(chain.cor(include_lp=True))
    # an explicit shift, a subset with a repeat
    n2, sh2, s2, x2 = run.cross_moments(params=[d, 0, d], shift=[0.5, -0.25, 0.5])
    assert n2 == n and np.array_equal(sh2, [0.5, -0.25, 0.5])
    Moments(shifted_rows(chain.value, [d, 0, d], sh2)).check(s2, x2, which + " subset")
    assert x2[0, 0] == x2[2, 2] == x2[0, 2] and s2[0] == s2[2]
    run.close()


# ---- 3. the reference's own statement (the RAM docstring) with the covariance taken on the device ----
def test_ram_doctest_covariance_on_the_device(mhx, real):
    Sig = np.array([[1.0, 0.5], [0.5, 1.0]])
    model = mhx.DensityModel(mhx.CorrGaussian(Sig))
    chain = mhx.sample(model, mhx.RobustAdaptiveMetropolis(), 10000, 32, seed=42, num_warmup=10000, initial_params=np.zeros(2))
    cov = chain.cov()
    print("device covariance of 320 000 draws:\n%s" % cov)
    assert cov.shape == (2, 2) and np.abs(cov - Sig).max() < 0.2
    chain.state.close()


# ---- 4. a group: moments about a common shift add ----
def test_group_cross_moments_are_the_sum_of_the_members(mhx, real):
    d, Cn, N = 3, 67, 21
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(d), 1.5 * mhx.I))
    init = np.random.default_rng(3).normal(size=(d, Cn))
    g = mhx.Group([0, 0])
    g.create(model, spl, nchains=Cn, seed=11, first_chain=5)
    g.init(init)
    g.sample(N)
    shift = np.array([0.25, -0.5, 0.125, -2.0])
    n, sh, s, x = g.cross_moments(shift=shift)
    parts = [r.cross_moments(shift=shift) for r in g.runs]
    assert n == N * Cn == sum(p[0] for p in parts)
    assert np.array_equal(s, parts[0][2] + parts[1][2]) and np.array_equal(x, parts[0][3] + parts[1][3])
    gathered = np.concatenate([r.samples()[0] for r in g.runs], axis=2)
    whole = mhx.Run(model, spl, nchains=Cn, seed=11, first_chain=5)
    whole.init(init)
    whole.sample(N)
    assert np.array_equal(whole.samples()[0], gathered)
    ref = Moments(shifted_rows(gathered, np.arange(d + 1), shift))
    ref.check(s, x, "group")
    ref.check(*whole.cross_moments(shift=shift)[2:], "unsharded")
    # the default shift pools sample 0 of all members; cov and cor follow
    n3, sh3, s3, x3 = g.cross_moments()
    np.testing.assert_allclose(sh3, gathered[0].astype(np.float64).mean(axis=1), rtol=0, atol=1e-12 * np.abs(gathered[0]).max())
    Moments(shifted_rows(gathered, np.arange(d + 1), sh3)).check(s3, x3, "group default shift")
    np.testing.assert_allclose(g.cov(), whole.cov(), rtol=1e-10, atol=1e-13)
    assert g.cor().shape == (d + 1, d + 1)
    with pytest.raises(mhx.ArgumentError, match="mhx_group_cross_moments"):
        g.cross_moments(params=[d + 1])
    with pytest.raises(mhx.ArgumentError, match="mhx_group_cross_moments"):
        g.cross_moments(shift=[0.0, np.inf, 0.0, 0.0])
    g.close()
    whole.close()


# ---- 5. refusals: an ArgumentError that names the entry point, nothing written ----
def test_refusals(mhx, real):
    chain = _rwmh_chain(mhx, 9, 10)
    run, d1 = chain.state, 4
    lib = mhx.lib()

    def call(params, shift, run=run):
        params = np.array(params, dtype=np.int32)
        m = len(params)
        shift = None if shift is None else np.array(shift, dtype=np.float64)
        s, x, n = np.full(m, -12345.0), np.full((m, m), -12345.0), C.c_int64(-7)
        rc = lib.mhx_run_cross_moments(run.h, params.ctypes.data_as(C.POINTER(C.c_int32)), m, None if shift is None else shift.ctypes.data_as(DP),
                                       s.ctypes.data_as(DP), x.ctypes.data_as(DP), C.byref(n))
        return rc, lib.mhx_last_error().decode(), s, x, n.value

    rc, msg, s, x, n = call([0, 1], None)
    assert rc == 0 and n == 90 and not np.any(s == -12345.0) and not np.any(x == -12345.0)
    for params, shift in (([d1], None), ([0, -1], None), ([0, 1], [0.0, np.nan]), ([0], [np.inf])):
        rc, msg, s, x, n = call(params, shift)
        assert rc == mhx.MHX_EINVAL and "mhx_run_cross_moments" in msg, (rc, msg)
        assert np.all(s == -12345.0) and np.all(x == -12345.0) and n == -7
        with pytest.raises(mhx.ArgumentError, match="mhx_run_cross_moments"):
            run.cross_moments(params=params, shift=shift)
    with pytest.raises(mhx.ArgumentError, match="mhx_run_cross_moments"):
        run.cross_moments(params=[d1])                       # ... also when the default shift would be asked for first
    # the raw-tensor entry point refuses the same way
    import torch
    dev = torch.zeros((2, 3, 5), dtype=torch.float64 if real == "f64" else torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx = mhx.Context.default(dtype=real)
    for params, shift in (([3], None), ([0], [np.nan])):
        rc, s, x = _ctx_cross_moments(mhx, ctx, dev, (2, 3, 5), params, shift)
        assert rc == mhx.MHX_EINVAL and "mhx_ctx_cross_moments" in lib.mhx_last_error().decode()
        assert np.all(s == -12345.0) and np.all(x == -12345.0)
    # a run that saved nothing holds no tensor
    run.sample(10, save=False)
    rc, msg, s, x, n = call([0], None)
    assert rc == mhx.MHX_ESTATE and "mhx_run_cross_moments" in msg and np.all(x == -12345.0)
    for f in (run.cross_moments, run.cov, run.cor, chain.cov, chain.cor):
        with pytest.raises(mhx.ArgumentError, match="mhx_run_cross_moments"):
            f()
    # one draw: moments exist, a covariance does not
    one = _rwmh_chain(mhx, 1, 1)
    n, sh, s, x = one.state.cross_moments()
    assert n == 1 and np.array_equal(s, np.zeros(4)) and np.array_equal(x, np.zeros((4, 4)))       # the shift is the draw itself
    with pytest.raises(mhx.ArgumentError, match="covariance_from_moments"):
        one.state.cov()
    with pytest.raises(mhx.ArgumentError, match="covariance_from_moments"):
        one.cov()
    one.state.close()
    run.close()
