"""Histograms, pair histograms and densities of the draws on the device (mhx_run_histogram / mhx_run_histogram2d and their ctx and
group forms: one sweep of the [N][dim+1][C] tensor in place, LDS counts, integer atomics) against numpy's own histograms of the draws
copied back and widened to float64, and against the numpy restatement of the definition (tests/histogram_ref.py) where numpy has no
word for it (the outside counts, NaN rows).  Counts are integers and every comparison is `==`; the only tolerance is the derived
binning bound of `density`."""
import ctypes as C
import math

import numpy as np
import pytest

from histogram_ref import histogram2d_rows, histogram_numpy, histogram_rows, kde_direct

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0xDEADBEEFDEADBEEF)
I32P, U64P, DP = C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)


def _rwmh_chain(mhx, N, Cn, seed=5):
    model = mhx.DensityModel(mhx.IsoGaussian(3))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(3), 1.5 * mhx.I))
    init = np.random.default_rng(seed).normal(size=(3, Cn))
    return mhx.sample(model, spl, N, Cn, initial_params=init, seed=seed)


def _raw(fn, handle, tensor, params, edges, nbins, pairs=None):
    """one raw call, the outputs pre-filled with a sentinel: (rc, message, counts, outside)"""
    import mhx
    params = np.ascontiguousarray(params, dtype=np.int32)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    m = len(params)
    args = [handle] + list(tensor) + [params.ctypes.data_as(I32P), m, edges.ctypes.data_as(DP), int(nbins)]
    B = max(int(nbins), 1)
    if pairs is None:
        counts, outside = np.full((m, B), SENTINEL), np.full((m, 3), SENTINEL)
    else:
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        counts, outside = np.full((len(pairs), B, B), SENTINEL), np.full(len(pairs), SENTINEL)
        args += [pairs.ctypes.data_as(I32P), len(pairs)]
    rc = fn(*args, counts.ctypes.data_as(U64P), outside.ctypes.data_as(U64P))
    return rc, mhx.lib().mhx_last_error().decode(), counts, outside


def _untouched(counts, outside):
    return bool(np.all(counts == SENTINEL) and np.all(outside == SENTINEL))


def _wide(chain, name):
    return chain[name].astype(np.float64).ravel()


# ---- 1. real chains: rejected steps repeat draws; the shapes of the quantile and HPD tests.  (17, 241): S = 4097, the smallest S with
# two blocks per row in both widths (a block's unrolled sweep is 512 threads x 8 fp32 / 4 fp64 draws); (3, 700): more chains than a
# block has threads, where the lane-to-chain step has 512 / C == 0 ----
SHAPES = [(33, 67), (1000, 1), (5, 3), (2, 257), (1, 64), (17, 241), (3, 700)]


@pytest.mark.parametrize("N,Cn", SHAPES)
def test_histograms_of_real_chains(mhx, real, N, Cn):
    chain = _rwmh_chain(mhx, N, Cn)
    run, S, names = chain.state, N * Cn, chain.names
    assert len(names) == 4 and names[3] == "lp"
    for bins in (1, 2, 7, 64, 2048):
        for rng_ in (None, (-0.75, 1.25)):
            for name in names:
                counts, edges = chain.histogram(name, bins=bins, range=rng_)
                want, wedges = np.histogram(_wide(chain, name), bins, rng_)
                assert counts.dtype == np.int64 and counts.shape == (bins,) and edges.dtype == np.float64
                assert np.array_equal(edges, wedges) and np.array_equal(counts, want), (name, bins, rng_)
            # all rows in one sweep, and the totals
            counts, edges, outside = run.histogram(bins=bins, range=rng_)
            assert counts.shape == (4, bins) and edges.shape == (4, bins + 1) and outside.shape == (4, 3)
            assert np.array_equal(counts.sum(axis=1) + outside.sum(axis=1), np.full(4, S))
            wc, wo = histogram_rows(chain.value, range(4), edges)
            assert np.array_equal(counts, wc) and np.array_equal(outside, wo)
            if rng_ is None:
                assert not outside.any()
    # a subset of the rows in another order with one repeat
    rows = [3, 1, 1, 0]
    counts, edges, outside = run.histogram(bins=7, params=rows)
    for k, p in enumerate(rows):
        want, wedges = np.histogram(_wide(chain, names[p]), 7)
        assert np.array_equal(counts[k], want) and np.array_equal(edges[k], wedges)
    run.close()


@pytest.mark.parametrize("N,Cn", SHAPES)
def test_pair_histograms_and_corner_of_real_chains(mhx, real, N, Cn):
    chain = _rwmh_chain(mhx, N, Cn)
    run, S, names = chain.state, N * Cn, chain.names
    for bins in (1, 5, 128):
        H, xe, ye = chain.histogram2d(names[0], names[2], bins=bins)
        want, wx, wy = np.histogram2d(_wide(chain, names[0]), _wide(chain, names[2]), bins)
        assert H.dtype == np.int64 and np.array_equal(H, want.astype(np.int64)) and np.array_equal(xe, wx) and np.array_equal(ye, wy)
        given = [(-0.75, 1.25), (-1.5, 0.5)]
        H, xe, ye = chain.histogram2d(names[1], names[3], bins=bins, range=given)
        want, wx, wy = np.histogram2d(_wide(chain, names[1]), _wide(chain, names[3]), bins, given)
        assert np.array_equal(H, want.astype(np.int64)) and np.array_equal(xe, wx) and np.array_equal(ye, wy)
        # every pair of all rows, and the totals
        counts, edges, outside, pairs = run.histogram2d(bins=bins, range=(-0.75, 1.25))
        assert counts.shape == (6, bins, bins) and outside.shape == (6,) and [tuple(p) for p in pairs] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        assert np.array_equal(counts.sum(axis=(1, 2)) + outside, np.full(6, S))
        wc, wo = histogram2d_rows(chain.value, range(4), edges, pairs)
        assert np.array_equal(counts, wc) and np.array_equal(outside, wo)
        # corner: the parameters without lp, each row between its own minimum and maximum
        cn = chain.corner(bins=bins)
        assert cn.names == chain.params() == names[:3] and sorted(cn.joint) == [(names[0], names[1]), (names[0], names[2]), (names[1], names[2])]
        for a in cn.names:
            want, wedges = np.histogram(_wide(chain, a), bins)
            assert np.array_equal(cn.marginal[a], want) and np.array_equal(cn.edges[a], wedges) and not cn.outside[a].any()
        for (a, b), Hab in cn.joint.items():
            want, _, _ = np.histogram2d(_wide(chain, a), _wide(chain, b), bins)
            assert np.array_equal(Hab, want.astype(np.int64)) and cn.outside[(a, b)] == 0 and Hab.sum() == S
            assert np.array_equal(Hab.sum(axis=1), cn.marginal[a]) and np.array_equal(Hab.sum(axis=0), cn.marginal[b])
    text = repr(chain.corner(names=[names[1], "lp"], bins=5))
    assert text.split("\n")[0] == "Corner (2 parameters, 5 bins): 2 marginal [5], 1 joint [5][5]" and text.count("%d draws" % S) == 3
    # a subset in another order with a repeat, pairs given
    rows, pr = [3, 1, 1, 0], [(0, 3), (2, 1), (3, 3)]
    counts, edges, outside, pairs = run.histogram2d(params=rows, pairs=pr, bins=5)
    wc, wo = histogram2d_rows(chain.value, rows, edges, pr)
    assert np.array_equal(counts, wc) and np.array_equal(outside, wo) and np.array_equal(pairs, pr)
    assert np.array_equal(np.diag(counts[2]), histogram_numpy(chain.value[:, 0, :], edges[3])[0])      # a row against itself: the diagonal
    bare = mhx.Chains(chain.value, chain.names, chain.start, chain.thin)
    for call, what in ((lambda: bare.histogram(names[0]), "histogram"), (lambda: bare.histogram2d(names[0], names[1]), "histogram2d"),
                       (lambda: bare.corner(), "corner"), (lambda: bare.density(names[0]), "density")):
        with pytest.raises(mhx.ArgumentError, match="%s needs the live run" % what):
            call()
    run.close()


# ---- 2. crafted tensors through mhx_ctx_histogram / mhx_ctx_histogram2d on a torch tensor ----
ROWS = ("all equal", "two values", "on every edge and one ulp to either side", "signed zeros, an edge at 0", "infinities and NaNs of both signs",
        "1e4 +- 0.01", "exp(8 normal), log-spaced edges", "edges with repeats", "edges fp32 cannot represent", "clean")
B0 = 16


def _nan(dt, negative):
    bits = {np.float32: (np.uint32, 0x7FC00000, 0x80000000), np.float64: (np.uint64, 0x7FF8000000000000, 0x8000000000000000)}[dt]
    return np.array([bits[1] | (bits[2] if negative else 0)], dtype=bits[0]).view(dt)[0]


def _crafted(dt, rng, N, Cn):
    """([N][10][C] tensor, [10][B0 + 1] edges)"""
    S = N * Cn
    fill = lambda v: np.resize(np.asarray(v, dtype=dt), S)
    rows, edges = [], []
    rows.append(np.full(S, 3.25, dtype=dt)); edges.append(np.histogram_bin_edges([], B0, (3.25, 3.25)))
    rows.append(rng.choice([1.0, 2.0], size=S).astype(dt)); edges.append(np.histogram_bin_edges([], B0, (1.0, 2.0)))
    e = np.linspace(-2.0, 2.0, B0 + 1)                      # multiples of 1/4: representable in both widths
    on = e.astype(dt)
    rows.append(fill(np.concatenate([on, np.nextafter(on, dt(np.inf)), np.nextafter(on, dt(-np.inf))]))); edges.append(e)
    rows.append(rng.choice([-0.0, 0.0], size=S).astype(dt)); edges.append(np.linspace(-1.0, 1.0, B0 + 1))
    r = rng.normal(size=S).astype(dt)
    r[:5], r[5:9], r[9], r[10] = np.inf, -np.inf, _nan(dt, True), _nan(dt, False)
    rows.append(r); edges.append(np.histogram_bin_edges([], B0, (-1.0, 1.0)))
    r = (1e4 + rng.choice([-0.01, 0.0, 0.01], size=S)).astype(dt)
    rows.append(r); edges.append(np.histogram_bin_edges([], B0, (float(r.min()), float(r.max()))))
    rows.append(np.exp(8.0 * rng.normal(size=S)).astype(dt)); edges.append(np.geomspace(1e-8, 1e8, B0 + 1))
    rows.append(rng.choice([-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 3.5, 4.0, 5.0, 5.5], size=S).astype(dt))
    edges.append(np.repeat([0.0, 1.0, 2.0, 3.0, 4.0, 5.0], [2, 3, 2, 4, 3, 3]))
    e = 0.1 * np.arange(B0 + 1)                             # 0.1, 0.3, ...: no fp32 number equals them
    near = e.astype(dt)                                     # fp32: the nearest float, on either side of the edge; fp64: the edge itself
    rows.append(fill(np.concatenate([near, np.nextafter(near, dt(np.inf)), np.nextafter(near, dt(-np.inf))]))); edges.append(e)
    rows.append(rng.normal(size=S).astype(dt)); edges.append(np.histogram_bin_edges([], B0, (-2.5, 2.5)))
    t = np.stack([rng.permutation(r).reshape(N, Cn) for r in rows], axis=1)
    assert t.dtype == dt and all(len(e) == B0 + 1 for e in edges)
    return np.ascontiguousarray(t), np.stack(edges)


@pytest.fixture(params=[(7, 65), (2, 257)], ids=["7x65", "2x257"])
def crafted(request, mhx, real):
    import torch
    dt = mhx._lib.NP_DTYPES[real]
    N, Cn = request.param
    host, edges = _crafted(dt, np.random.default_rng([N, Cn]), N, Cn)
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    ctx = mhx.Context.default(dtype=real)
    yield host, edges, (N, len(ROWS), Cn), ctx, [ctx.h, C.c_void_p(dev.data_ptr()), N, len(ROWS), Cn]
    del dev


def test_histograms_of_crafted_tensors(mhx, real, crafted):
    host, edges, shape, ctx, handle = crafted
    S, every = shape[0] * shape[2], np.arange(len(ROWS))
    dt = host.dtype.type
    assert np.isnan(host[:, 4, :]).sum() == 2 and np.signbit(host[:, 4, :][np.isnan(host[:, 4, :])]).sum() == 1 and np.isnan(host).sum() == 2
    if dt is np.float32:
        assert not np.any(np.isin(host[:, 8, :].astype(np.float64), edges[8][[1, 3]]))     # no fp32 draw equals the edges 0.1 and 0.3
    rc, msg, counts, outside = _raw(mhx.lib().mhx_ctx_histogram, handle[0], handle[1:], every, edges, B0)
    assert rc == 0, msg
    counts, outside = counts.view(np.int64), outside.view(np.int64)
    wc, wo = histogram_rows(host, every, edges)
    for r, what in enumerate(ROWS):
        assert np.array_equal(counts[r], wc[r]) and np.array_equal(outside[r], wo[r]), (what, counts[r], wc[r], outside[r], wo[r])
        assert counts[r].sum() + outside[r].sum() == S, what
        if r != 4:                                          # numpy agrees wherever it has an answer
            assert np.array_equal(counts[r], np.histogram(host[:, r, :].astype(np.float64).ravel(), bins=edges[r])[0]), what
    assert counts[0][B0 // 2] == S and counts[3][B0 // 2] == S                         # a constant row; both zeros in the bin that starts at 0.0
    assert outside[4][0] >= 4 and outside[4][1] >= 5 and outside[4][2] == 2           # -inf below, +inf above, both NaNs
    assert outside[2][0] >= 1 and outside[2][1] >= 1 and outside[2][2] == 0           # one ulp below e[0] and above e[B]: outside
    assert np.all(counts[7][[0, 2, 3, 5, 7, 8, 9, 11, 12, 14]] == 0) and np.all(counts[7][[1, 4, 6, 10, 13, 15]] > 0)      # of equal edges the last takes the draws
    # the rows answer alone, in another order and repeated, as they do side by side
    sub = [9, 4, 2, 2, 6]
    rc, msg, c2, o2 = _raw(mhx.lib().mhx_ctx_histogram, handle[0], handle[1:], sub, edges[sub], B0)
    assert rc == 0 and np.array_equal(c2.view(np.int64), counts[sub]) and np.array_equal(o2.view(np.int64), outside[sub]), msg
    # 2048 log-spaced bins for the heavy-tailed row: the bisection, far from any uniform guess
    fine = np.geomspace(1e-30, 1e30, 2049)
    rc, msg, c3, o3 = _raw(mhx.lib().mhx_ctx_histogram, handle[0], handle[1:], [6, 9], np.stack([fine, np.linspace(-3.0, 3.0, 2049)]), 2048)
    w3c, w3o = histogram_rows(host, [6, 9], [fine, np.linspace(-3.0, 3.0, 2049)])
    assert rc == 0 and np.array_equal(c3.view(np.int64), w3c) and np.array_equal(o3.view(np.int64), w3o), msg
    # outside NULL: only the counts are wanted
    params = np.array([9], dtype=np.int32)
    only = np.full((1, B0), SENTINEL)
    e9 = np.ascontiguousarray(edges[9:10])
    mhx.check(mhx.lib().mhx_ctx_histogram(*handle, params.ctypes.data_as(I32P), 1, e9.ctypes.data_as(DP), B0, only.ctypes.data_as(U64P), None))
    assert np.array_equal(only.view(np.int64)[0], counts[9])


def test_pair_histograms_of_crafted_tensors(mhx, real, crafted):
    host, edges, shape, ctx, handle = crafted
    S, every = shape[0] * shape[2], np.arange(len(ROWS))
    pairs = [(4, 9), (9, 4), (2, 8), (0, 1), (6, 7), (3, 5), (9, 9)]
    rc, msg, counts, outside = _raw(mhx.lib().mhx_ctx_histogram2d, handle[0], handle[1:], every, edges, B0, pairs)
    assert rc == 0, msg
    counts, outside = counts.view(np.int64), outside.view(np.int64)
    wc, wo = histogram2d_rows(host, every, edges, pairs)
    assert np.array_equal(counts, wc) and np.array_equal(outside, wo)
    assert np.array_equal(counts.sum(axis=(1, 2)) + outside, np.full(len(pairs), S))
    assert np.array_equal(counts[0], counts[1].T) and outside[0] == outside[1]
    # the NaN row beside the clean row: what it has no bin for is outside, and the clean row's own counts are what they are alone
    c1, o1 = histogram_rows(host, [4, 9], edges[[4, 9]])
    assert outside[0] >= o1[0].sum() and outside[0] <= o1[0].sum() + o1[1].sum()
    rc, msg, alone, oa = _raw(mhx.lib().mhx_ctx_histogram, handle[0], handle[1:], [9], edges[9:10], B0)
    rc2, msg2, beside, ob = _raw(mhx.lib().mhx_ctx_histogram, handle[0], handle[1:], [4, 9], edges[[4, 9]], B0)
    assert rc == 0 and rc2 == 0 and np.array_equal(alone[0], beside[1]) and np.array_equal(oa[0], ob[1]) and np.array_equal(alone.view(np.int64)[0], c1[1])
    assert np.array_equal(np.diag(counts[6]), c1[1]) and counts[6].sum() == np.trace(counts[6])


# ---- 3. refusals: the entry point's name in the message, nothing written ----
def test_refusals(mhx, real):
    chain = _rwmh_chain(mhx, 9, 10)
    run, d1 = chain.state, 4
    lib = mhx.lib()
    ptr, n_saved = C.c_void_p(), C.c_int64()
    mhx.check(lib.mhx_run_device_samples(run.h, C.byref(ptr), None, C.byref(n_saved)))
    tensor = [ptr, 9, d1, 10]
    g = mhx.Group([0])
    g.create(mhx.DensityModel(mhx.IsoGaussian(3)), mhx.RWMH(mhx.MvNormal(mhx.zeros(3), 1.5 * mhx.I)), nchains=10, seed=5)
    g.init(np.random.default_rng(5).normal(size=(3, 10)))
    g.sample(9)
    good = np.tile(np.linspace(-1.0, 1.0, 5), (2, 1))
    forms = [("mhx_run_histogram", lib.mhx_run_histogram, run.h, [], None, 2048), ("mhx_ctx_histogram", lib.mhx_ctx_histogram, run.ctx.h, tensor, None, 2048),
             ("mhx_group_histogram", lib.mhx_group_histogram, g.h, [], None, 2048),
             ("mhx_run_histogram2d", lib.mhx_run_histogram2d, run.h, [], [(0, 1)], 128), ("mhx_ctx_histogram2d", lib.mhx_ctx_histogram2d, run.ctx.h, tensor, [(0, 1)], 128),
             ("mhx_group_histogram2d", lib.mhx_group_histogram2d, g.h, [], [(0, 1)], 128)]
    for name, fn, h, t, pairs, limit in forms:
        rc, msg, counts, outside = _raw(fn, h, t, [0, 3], good, 4, pairs)
        assert rc == 0 and not np.any(counts == SENTINEL) and not np.any(outside == SENTINEL), (name, msg)
        bad = []
        for params in ([0, d1], [-1, 0]):                   # a row outside [0, dim]
            bad.append((params, good, 4, pairs))
        bad.append(([0, 3], good, 0, pairs))                # nbins < 1, and above the limit
        bad.append(([0, 3], np.tile(np.linspace(-1.0, 1.0, limit + 2), (2, 1)), limit + 1, pairs))
        for k, v in ((2, np.nan), (4, np.inf), (0, -np.inf)):       # an edge that is not finite
            e = good.copy()
            e[1, k] = v
            bad.append(([0, 3], e, 4, pairs))
        e = good.copy()
        e[1, 3] = e[1, 2] - 0.25                            # edges that decrease
        bad.append(([0, 3], e, 4, pairs))
        if pairs is not None:                               # a pair slot outside [0, nparams)
            bad += [([0, 3], good, 4, [(0, 2)]), ([0, 3], good, 4, [(0, 1), (-1, 1)])]
        for params, e, nbins, pr in bad:
            rc, msg, counts, outside = _raw(fn, h, t, params, e, nbins, pr)
            assert rc == mhx.MHX_EINVAL and name in msg and _untouched(counts, outside), (name, params, nbins, pr, rc, msg)
    with pytest.raises(mhx.ArgumentError, match="mhx_run_histogram"):
        run.histogram(bins=4, range=(0.0, 1.0), params=[d1])
    with pytest.raises(mhx.ArgumentError, match="mhx_run_histogram2d"):
        run.histogram2d(bins=129, range=(0.0, 1.0))
    with pytest.raises(mhx.ArgumentError, match="histogram_edges"):
        run.histogram(bins=0, range=(0.0, 1.0))
    # moments mode keeps no sample tensor (the shape of tests/test_gpu_quantiles.py)
    dm, Cm = 40, 96
    s = float(np.float32(2.38 / dm ** 0.5))
    mom = mhx.Run(mhx.DensityModel(mhx.Funnel(dm)), mhx.RWMH(mhx.MvNormal(mhx.zeros(dm), s * s * mhx.I)), nchains=Cm, seed=2)
    mom.init(np.random.default_rng(8).normal(size=(dm, Cm)))
    mom.sample(10, 5, 5, 0, save="moments")
    for name, fn, pairs in (("mhx_run_histogram", lib.mhx_run_histogram, None), ("mhx_run_histogram2d", lib.mhx_run_histogram2d, [(0, 1)])):
        rc, msg, counts, outside = _raw(fn, mom.h, [], [0, 3], good, 4, pairs)
        assert rc == mhx.MHX_ESTATE and name in msg and _untouched(counts, outside), (name, rc, msg)
    with pytest.raises(mhx.MhxError, match="mhx_run_histogram"):
        mom.histogram(bins=4, range=(0.0, 1.0))
    with pytest.raises(mhx.MhxError):
        mom.histogram(bins=4)
    mom.close()
    g.close()
    run.close()


class _TensorDraws:
    """the two things the automatic range asks of a run (its draws' count and order statistics), over a caller's device tensor"""

    def __init__(self, mhx, handle, shape):
        self.mhx, self.handle, self.shape = mhx, handle, shape

    def _n_draws(self):
        return self.shape[0] * self.shape[2]

    def order_statistics(self, ranks, params):
        params, ranks = np.ascontiguousarray(params, dtype=np.int32), np.ascontiguousarray(ranks, dtype=np.int64)
        out = np.empty((len(params), len(ranks)))
        self.mhx.check(self.mhx.lib().mhx_ctx_order_statistics(*self.handle, params.ctypes.data_as(I32P), len(params),
                                                               ranks.ctypes.data_as(C.POINTER(C.c_int64)), len(ranks), out.ctypes.data_as(DP)))
        return out


def test_a_row_with_a_nan_or_an_infinity_needs_a_range(mhx, real, crafted):
    """range None takes each row's minimum and maximum from one order-statistics call; an end that is not finite is an ArgumentError
    (a ValueError, as numpy's) that names the row"""
    host, edges, shape, ctx, handle = crafted
    draws = _TensorDraws(mhx, handle, shape)
    rows = np.array([9, 0, 5], dtype=np.int32)
    e = mhx.api._histogram_edges(draws, rows, 7, None, None, "histogram")
    for k, r in enumerate(rows):
        assert np.array_equal(e[k], np.histogram(host[:, r, :].astype(np.float64).ravel(), 7)[1])
    with pytest.raises(ValueError, match="histogram: the range of row 4"):
        mhx.api._histogram_edges(draws, np.array([9, 4], dtype=np.int32), 7, None, None, "histogram")
    with pytest.raises(mhx.ArgumentError, match="row 9"):
        mhx.api._histogram_edges(draws, rows, 7, [(0.0, np.inf), (0.0, 1.0), (0.0, 1.0)], None, "histogram")


# ---- 4. reproducibility ----
def test_two_calls_return_the_same_arrays(mhx, real):
    chain = _rwmh_chain(mhx, 17, 241)
    run = chain.state
    a = run.histogram(bins=2048, params=[2, 0, 0, 3])
    b = run.histogram(bins=2048, params=[2, 0, 0, 3])
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[0][1], a[0][2])
    a = run.histogram2d(bins=128)
    b = run.histogram2d(bins=128)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    run.close()


# ---- 5. a group: integer counts add over the shards ----
def test_group_histograms_equal_the_unsharded_run(mhx, real):
    d, Cn, N = 3, 67, 21
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(d), 1.5 * mhx.I))
    init = np.random.default_rng(3).normal(size=(d, Cn))
    g = mhx.Group([0, 0, 0])
    g.create(model, spl, nchains=Cn, seed=11, first_chain=5)
    assert sorted(r.n for r in g.runs) == [22, 22, 23]
    g.init(init)
    g.sample(N)
    whole = mhx.Run(model, spl, nchains=Cn, seed=11, first_chain=5)
    whole.init(init)
    whole.sample(N)
    gathered = np.concatenate([r.samples()[0] for r in g.runs], axis=2)
    assert np.array_equal(whole.samples()[0], gathered)
    ranges = [(-3.0, 3.0), (-2.0, 1.0), (0.0, 0.5), (-10.0, 0.0)]              # edges fixed up front
    for bins in (7, 64, 2048):
        got, want = g.histogram(bins=bins, range=ranges), whole.histogram(bins=bins, range=ranges)
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
        wc, wo = histogram_rows(gathered, range(d + 1), got[1])
        assert np.array_equal(got[0], wc) and np.array_equal(got[2], wo) and np.array_equal(wc.sum(axis=1) + wo.sum(axis=1), np.full(d + 1, N * Cn))
        parts = [r.histogram(bins=bins, range=ranges) for r in g.runs]
        assert np.array_equal(got[0], sum(p[0] for p in parts)) and np.array_equal(got[2], sum(p[2] for p in parts))
    for bins in (5, 128):
        got, want = g.histogram2d(bins=bins, range=ranges), whole.histogram2d(bins=bins, range=ranges)
        assert all(np.array_equal(x, y) for x, y in zip(got, want)) and got[0].shape == (6, bins, bins)
        wc, wo = histogram2d_rows(gathered, range(d + 1), got[1], got[3])
        assert np.array_equal(got[0], wc) and np.array_equal(got[2], wo)
    # the automatic range pools the members' minima and maxima (the group's order statistics)
    got, want = g.histogram(bins=64), whole.histogram(bins=64)
    assert all(np.array_equal(x, y) for x, y in zip(got, want)) and not got[2].any()
    with pytest.raises(mhx.ArgumentError, match="mhx_group_histogram"):
        g.histogram(bins=4, range=(0.0, 1.0), params=[d + 1])
    g.close()
    whole.close()


# ---- 6. density: the device's counts under a Gaussian kernel against the direct sum over the draws themselves ----
def test_density_within_the_binning_bound(mhx, real):
    """every draw moves by at most half a cell delta / 2 to its bin's centre, so |density - exact| <= delta / (2 h^2 sqrt(2 pi e)); the
    float64 sums of at most 2211 positive terms on either side add at most 2211 x 1.1e-16 < 1e-12 of the largest density"""
    chain = _rwmh_chain(mhx, 33, 67)
    run, S = chain.state, 33 * 67
    for name, npoints in ((chain.names[0], 2048), (chain.names[3], 300)):
        row = chain.names.index(name)
        x64 = _wide(chain, name)
        # the bandwidth density() itself used, from the same device calls; numpy's agrees to rounding
        std = math.sqrt(run.cov([row])[0, 0])
        q25, q75 = run.quantiles([0.25, 0.75], [row])[0]
        h = mhx.silverman_bandwidth(std, q25, q75, S)
        n25, n75 = np.quantile(x64, [0.25, 0.75])
        assert abs(h - mhx.silverman_bandwidth(np.std(x64, ddof=1), n25, n75, S)) <= 1e-10 * h
        for bw in (None, h, 0.05):
            hh = h if bw is None else bw
            grid, dens = chain.density(name, npoints=npoints, bandwidth=bw)
            e = mhx.histogram_edges(x64.min() - 4.0 * hh, x64.max() + 4.0 * hh, npoints)
            assert grid.shape == dens.shape == (npoints,) and np.array_equal(grid, 0.5 * (e[:-1] + e[1:]))
            exact = kde_direct(x64, grid, hh)
            bound = mhx.density_binning_bound(e, hh)
            assert bound == (e[-1] - e[0]) / npoints / (2.0 * hh * hh * math.sqrt(2.0 * math.pi * math.e))
            err = np.abs(dens - exact).max()
            print("%s npoints %d h %.4g: |density - exact| max %.3e, bound %.3e" % (name, npoints, hh, err, bound))
            assert err <= bound + 1e-12 * exact.max()
            # and it IS the host sum over the device's own counts
            counts, _, outside = run.histogram(params=[row], edges=e)
            assert not outside.any() and np.array_equal(dens, mhx.density_from_counts(counts[0], e, hh)[1])
    with pytest.raises(mhx.ArgumentError, match="density: the bandwidth"):
        chain.density(chain.names[0], bandwidth=0.0)
    run.close()
