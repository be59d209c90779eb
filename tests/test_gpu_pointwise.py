"""GPU: the pointwise log-likelihood sums (mhx_run_pointwise / mhx_ctx_pointwise, Run.pointwise, Group.pointwise, Chains.pointwise /
waic / dic; csrc/mhx_pointwise_kernels.h) against tests/pointwise_ref.py: the same MHX_POINTWISE text compiled for
the host gives l[i, s] bit for bit, and from it -- in 80-bit arithmetic -- the five arrays with a bound for each, derived there.

  exact     max, bad, the returned shift and T equal the reference bit for bit; with integer draws and rows and l = x[0] + r[0], s1 and
            s2 are sums of integers below 2^53, exact in any order, and equal numpy's
  bounded   sumexp, s1, s2, lppd, var, elpd within MARGIN x bound on EVERY row of every case; each test prints the largest
            |error| / bound it met (DESIGN.md section 6.5.7 records them)

Shapes: the smallest at which the frame can go wrong.  C = 1, 63, 65, 257: a lone lane, a partial wave, a wave plus one lane, a block plus
one lane.  A lane takes one draw at a time and a strip is 16 draws, so n_saved = 1, 3, 17, 35: one draw, fewer than a strip, a strip plus
one, two strips and a ragged end -- at 35 draws of 257 chains there are 2 x 3 partials per row, merged one after the other.  A tile is
R = 8 rows in fp64 and 4 in fp32, so nrows = 1, 3, 5, 7, 9, 17 (R - 1, R + 1 and 2R + 1 of both); rowlen = 1 and 3; d = 1 and 5 with a source that names row d - 1 only.  The planted shapes go
through the ctx form on ONE device buffer per width (a run's sample buffer, large enough for the largest case).  Four sources per
width: SRC_LOG, SRC_INT, the README's Normal line (traced), and one that does not compile."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.special import logsumexp

import mhx.trace as T
import pointwise_ref as P
from planted import plant_ptr

pytestmark = pytest.mark.gpu

# l = r[0] log(v - r[1]) + r[m - 1], v = x[d - 1]: names one row of the draw whatever d is, and with rowlen 1 every r[j] is r[0] (the
# clamp).  v == r[1] makes l -inf (r[0] > 0) or +inf (r[0] < 0); v < r[1] makes it NaN.
SRC_LOG = """
MHX_POINTWISE(x, r, m, d, data, ndata)
{
    return mhx_fma(r[0], mhx_log(x[d - 1] - r[1]), r[m - 1]);
}
"""
SRC_INT = "MHX_POINTWISE(x, r, m, d, data, ndata) { return x[0] + r[0]; }\n"
SRC_BAD = "MHX_POINTWISE(x, r, m, d, data, ndata) { return x[0] +* ; }\n"
LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)
CAP = (40, 6, 257)                      # the planted buffer: every case's tensor fits
RATIOS = {}                             # (width, quantity) -> largest |error| / bound met


def normal_ll(t, y):
    return -0.5 * ((y - t.mu) / t.sigma) ** 2 - T.log(t.sigma) - LOG_SQRT_2PI


_BUF = {}


@pytest.fixture(scope="module", autouse=True)
def _buffers():
    yield
    for run, _ in _BUF.values():
        run.close()
    _BUF.clear()
    for k in sorted(RATIOS):
        print("pointwise ratio %s %-7s %.4f" % (k[0], k[1], RATIOS[k]))


def _buffer(mhx, real):
    if real not in _BUF:
        _BUF[real] = plant_ptr(mhx, np.zeros(CAP, dtype=np.float64 if real == "f64" else np.float32))
    return _BUF[real]


def _ctx_pointwise(mhx, real, x, source, rows, data=None, shift=None):
    """mhx_ctx_pointwise on x [N][d + 1][C], copied into the width's device buffer"""
    run, ptr = _buffer(mhx, real)
    R = run.real
    x = np.ascontiguousarray(x, dtype=R)
    assert x.size <= CAP[0] * CAP[1] * CAP[2]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(ptr, x.ctypes.data_as(C.c_void_p), x.nbytes, 1) == 0
    rr = np.ascontiguousarray(rows, dtype=R)
    rr = rr.reshape(rr.shape[0], -1)
    dat = None if data is None else np.ascontiguousarray(data, dtype=R).ravel()
    nrows = rr.shape[0]
    sh = np.full(nrows, 123.0) if shift is None else np.array(shift, dtype=np.float64)
    out, T_ = np.full((5, nrows), 77.0), C.c_int64(-1)
    dp = C.POINTER(C.c_double)
    rc = mhx.lib().mhx_ctx_pointwise(run.ctx.h, ptr, x.shape[0], x.shape[1], x.shape[2], source.encode(), mhx._lib.rptr(rr), nrows, rr.shape[1],
                                     mhx._lib.rptr(dat), 0 if dat is None else dat.size, 0 if shift is None else 1, sh.ctypes.data_as(dp),
                                     out.ctypes.data_as(dp), C.byref(T_))
    if rc:
        return rc, out, sh, T_.value
    return mhx.PointwiseSums(max=out[0], sumexp=out[1], s1=out[2], s2=out[3], bad=out[4], shift=sh, T=int(T_.value))


def _note(real, name, ratio):
    RATIOS[(real, name)] = max(RATIOS.get((real, name), 0.0), ratio)


def _check(mhx, real, got, ref, tag):
    """the exact parts bit for bit, the bounded parts (and the table's columns) within MARGIN x bound on every row"""
    assert got["T"] == ref["T"], tag
    for k in ("max", "bad", "shift"):
        assert P.same_bits(got[k], ref[k]), (tag, k, got[k], ref[k])
    for k in ("sumexp", "s1", "s2"):
        ok, ratio = P.within(got[k], ref[k], ref["e_" + k])
        _note(real, k, ratio)
        assert ok, (tag, k, ratio, got[k], ref[k])
    tab, rt = mhx.pointwise_table(got), P.table(ref)
    for k in ("lppd", "var", "elpd"):
        ok, ratio = P.within(tab[k], rt[k], rt["e_" + k])
        _note(real, k, ratio)
        assert ok, (tag, k, ratio, tab[k], rt[k])


def _draws(real, N, d, nch, seed):
    """[N][d + 1][C]: draws in (2, 6)"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.uniform(2.0, 6.0, size=(N, d + 1, nch)).astype(np.float64 if real == "f64" else np.float32))


def _rows(real, nrows, rowlen, seed):
    """r[0] in (0.5, 2), r[1] in (-1, 1), r[2] in (-3, 3); with rowlen 1 the one entry serves as all three: in (0.5, 1)"""
    rng = np.random.default_rng(seed)
    if rowlen == 1:
        r = rng.uniform(0.5, 1.0, size=(nrows, 1))
    else:
        r = np.stack([rng.uniform(0.5, 2.0, nrows), rng.uniform(-1.0, 1.0, nrows), rng.uniform(-3.0, 3.0, nrows)], axis=1)
    return r.astype(np.float64 if real == "f64" else np.float32)


@pytest.mark.parametrize("nch", [1, 63, 65, 257])
def test_sums_of_every_shape_are_within_the_reference_bound(mhx, oracle, real, nch):
    host = P.host_matrix(oracle, SRC_LOG)
    for N in (1, 3, 17, 35):
        for d in (1, 5):
            x = _draws(real, N, d, nch, 100 * N + d + nch)
            for rowlen in (1, 3):
                rows = _rows(real, 17, rowlen, N + d + rowlen)
                l = host(x, rows)
                for nrows in (1, 3, 5, 7, 9, 17):
                    got = _ctx_pointwise(mhx, real, x, SRC_LOG, rows[:nrows])
                    assert isinstance(got, dict), got
                    _check(mhx, real, got, P.sums(l[:nrows], N, nch), (N, d, nch, rowlen, nrows))
    print("ratios so far:", {k: round(v, 4) for k, v in RATIOS.items() if k[0] == real})


def test_integer_sums_are_exact(mhx, real):
    rng = np.random.default_rng(8)
    N, nch, nrows = 35, 257, 9
    xi = rng.integers(-50, 51, size=(N, 2, nch))
    ri = rng.integers(-20, 21, size=nrows)
    x = xi.astype(np.float64 if real == "f64" else np.float32)
    got = _ctx_pointwise(mhx, real, x, SRC_INT, ri.astype(x.dtype))
    li = xi[:, 0, :].reshape(1, -1) + ri.reshape(-1, 1)                         # [nrows][T] integers
    sh = li[:, 0]
    assert got["T"] == N * nch and np.array_equal(got["shift"], sh.astype(np.float64)) and not got["bad"].any()
    assert np.array_equal(got["max"], li.max(axis=1).astype(np.float64))
    assert np.array_equal(got["s1"], (li - sh[:, None]).sum(axis=1).astype(np.float64))
    assert np.array_equal(got["s2"], ((li - sh[:, None]) ** 2).sum(axis=1).astype(np.float64))
    _check(mhx, real, got, P.sums(li.astype(np.float64), N, nch), "integers")    # (l is exact in both widths: no host compile needed)
    # a supplied shift is used: s1 and s2 follow it exactly here, and it is returned untouched
    mine = np.arange(nrows, dtype=np.float64) - 4.0
    again = _ctx_pointwise(mhx, real, x, SRC_INT, ri.astype(x.dtype), shift=mine)
    assert np.array_equal(again["shift"], mine)
    assert np.array_equal(again["s1"], (li - mine[:, None]).sum(axis=1)) and np.array_equal(again["s2"], ((li - mine[:, None]) ** 2).sum(axis=1))
    assert P.same_bits(again["max"], got["max"]) and P.same_bits(again["sumexp"], got["sumexp"])


def _edge_case(real):
    """63 chains (a partial wave) x 17 draws, d = 1; v = 1.5 exactly in draw 0 of chain 0 (the shift), in the last lane (chain 62, draw
    9), and in a few more; rows of 3.  The edges are switched on by the ROWS (r[1] = 1.5 / 1.75 / 7), so that the tensor, and with it
    every other row, is the same with and without them."""
    x = _draws(real, 17, 1, 63, 5)
    for t, c in ((0, 0), (9, 62), (16, 31), (3, 7)):
        x[t, 0, c] = 1.5
    plain = _rows(real, 12, 3, 77)
    edged = plain.copy()
    edged[1] = (2.0, 1.5, 0.25)          # -inf at the four planted draws, the shift among them
    edged[3] = (-2.0, 1.5, 0.25)         # +inf there
    edged[4] = (1.0, 1.75, 0.0)          # NaN there (log of -0.25)
    edged[6] = (1.0, 7.0, 0.0)           # NaN at every draw
    edged[8] = (100.0, 1.5 - 2.0 ** -11, 0.0)    # l = -762.5 at the planted draws, -70 .. 150 elsewhere: l - max below exp's underflow
    edged[10] = (1.0, 0.0, -745.0)       # every l near -745
    return x, plain, edged


def test_edges_follow_the_rules_and_leave_the_other_rows_alone(mhx, oracle, real):
    x, plain, edged = _edge_case(real)
    host = P.host_matrix(oracle, SRC_LOG)
    base = _ctx_pointwise(mhx, real, x, SRC_LOG, plain)
    got = _ctx_pointwise(mhx, real, x, SRC_LOG, edged)
    l = host(x, edged)
    assert np.isneginf(l[1]).sum() == 4 and np.isposinf(l[3]).sum() == 4 and np.isnan(l[4]).sum() == 4 and np.isnan(l[6]).all()
    assert l[8].min() < -760 and l[8].max() > -80 and -745.0 < l[10].min() and l[10].max() < -743.0
    _check(mhx, real, base, P.sums(host(x, plain), 17, 63), "plain")
    _check(mhx, real, got, P.sums(l, 17, 63), "edged")
    T_ = 17 * 63
    # -inf: counted, left out of the sums, adds nothing to sumexp; the shift (draw 0 of chain 0 is one of them) is 0
    assert got["bad"][1] == 4 and got["shift"][1] == 0.0 and np.isfinite(got["max"][1]) and np.isfinite(got["sumexp"][1])
    assert got["sumexp"][1] == pytest.approx(np.exp(l[1][np.isfinite(l[1])] - got["max"][1]).sum(), rel=1e-12)
    # +inf and NaN: counted, left out of s1 and s2 (which stay finite), max and sumexp NaN
    for i in (3, 4):
        assert got["bad"][i] == 4 and np.isnan(got["max"][i]) and np.isnan(got["sumexp"][i]) and np.isfinite(got["s1"][i]) and np.isfinite(got["s2"][i])
    assert got["bad"][6] == T_ and np.isnan(got["max"][6]) and got["s1"][6] == 0.0 and got["s2"][6] == 0.0 and got["shift"][6] == 0.0
    # below exp's underflow and near -745: finite everywhere, as the reference (checked above), nothing counted
    assert got["bad"][8] == 0 and got["bad"][10] == 0 and got["sumexp"][8] >= 1.0 and got["sumexp"][10] >= 1.0
    # no other row is affected: the same bits as without the edges
    for i in (0, 2, 5, 7, 9, 11):
        for k in ("max", "sumexp", "s1", "s2", "bad", "shift"):
            assert P.same_bits(got[k][i], base[k][i]), (i, k)
    # every draw -inf: max -inf, sumexp 0, every draw counted
    const = np.full((3, 2, 63), 1.5, dtype=x.dtype)
    allinf = _ctx_pointwise(mhx, real, const, SRC_LOG, edged[:2])
    assert allinf["max"][1] == -np.inf and allinf["sumexp"][1] == 0.0 and allinf["bad"][1] == 3 * 63 and allinf["s1"][1] == 0.0
    assert np.isneginf(mhx.pointwise_table(allinf)["lppd"][1])
    _check(mhx, real, allinf, P.sums(host(const, edged[:2]), 3, 63), "all -inf")


def test_two_calls_give_the_same_bits_and_every_tile_size_agrees(mhx, oracle, real):
    N, nch = 35, 257
    x = _draws(real, N, 5, nch, 21)
    rows = _rows(real, 17, 3, 22)
    ref = P.sums(P.host_matrix(oracle, SRC_LOG)(x, rows), N, nch)
    first = _ctx_pointwise(mhx, real, x, SRC_LOG, rows)
    second = _ctx_pointwise(mhx, real, x, SRC_LOG, rows)
    for k in ("max", "sumexp", "s1", "s2", "bad", "shift"):
        assert P.same_bits(first[k], second[k]), k
    run, _ = _buffer(mhx, real)
    try:
        for R in (2, 4, 8, 16):
            run.ctx.set_option("POINTWISE_ROWS", str(R))
            got = _ctx_pointwise(mhx, real, x, SRC_LOG, rows)
            _check(mhx, real, got, ref, "POINTWISE_ROWS=%d" % R)                 # (max, bad and shift bit for bit in there)
        run.ctx.set_option("POINTWISE_ROWS", "3")
        rc, out, sh, T_ = _ctx_pointwise(mhx, real, x, SRC_LOG, rows)
        assert rc == mhx.MHX_EINVAL and "POINTWISE_ROWS" in mhx.lib().mhx_last_error().decode()
    finally:
        run.ctx.set_option("POINTWISE_ROWS", None)


def test_refusals_write_nothing(mhx, real):
    x = _draws(real, 3, 1, 5, 1)
    rows = _rows(real, 2, 1, 1)
    rc, out, sh, T_ = _ctx_pointwise(mhx, real, x, SRC_BAD, rows)
    msg = mhx.lib().mhx_last_error().decode()
    assert rc == mhx.MHX_EINVAL and "pointwise.hip" in msg and "does not compile" in msg
    assert np.all(out == 77.0) and np.all(sh == 123.0) and T_ == -1
    run, ptr = _buffer(mhx, real)
    dp = C.POINTER(C.c_double)
    args = lambda nrows, rowlen: (run.ctx.h, ptr, 3, 2, 5, SRC_INT.encode(), mhx._lib.rptr(rows), nrows, rowlen, None, 0, 0,      # noqa: E731
                                  sh.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(C.c_int64()))
    for nrows, rowlen in ((0, 1), (2, 0), (-1, 1), (1 << 20, 1 << 12)):
        assert mhx.lib().mhx_ctx_pointwise(*args(nrows, rowlen)) == mhx.MHX_EINVAL
        assert np.all(out == 77.0) and np.all(sh == 123.0)
    # a second call with the same source compiles nothing
    _ctx_pointwise(mhx, real, x, SRC_INT, rows)
    before = run.ctx.jit_counts()
    _ctx_pointwise(mhx, real, x, SRC_INT, rows)
    assert run.ctx.jit_counts() == before


def _readme_model(mhx):
    data = np.random.default_rng(1234).normal(0.0, 1.0, size=30)
    model = mhx.DensityModel(mhx.IIDNormal(data))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(2), mhx.I))
    return data, model, spl


def test_readme_model_waic_and_dic_end_to_end(mhx, oracle, real):
    """257 chains x 200 draws, 30 data rows: chain.waic and chain.dic against scipy and numpy on run.samples() in float64, at the bounds
    of pointwise_ref (whose l is the engine's own arithmetic on the same samples); a derived run is a source; the entries that need a
    sampler still refuse it"""
    data, model, spl = _readme_model(mhx)
    chain = mhx.sample(model, spl, 200, 257, param_names=["mu", "sigma"], chain_type=mhx.Chains, discard_initial=100,
                       initial_params=np.array([0.0, 1.0]), seed=1234)
    run = chain.state
    x, _ = run.samples()
    tp = T.trace_pointwise(normal_ll, 2, data, names=["mu", "sigma"])
    ref = P.sums(P.host_matrix(oracle, tp.source)(x, data), 200, 257)
    sums = run.pointwise(normal_ll, data, names=["mu", "sigma"])
    _check(mhx, real, sums, ref, "readme")
    w, rt = chain.waic(normal_ll, data), P.table(ref)
    assert w["pointwise"]["T"] == 200 * 257 and "WAIC" in str(w) and "lppd" in str(chain.pointwise(normal_ll, data))
    e_total = float((P.MARGIN * rt["e_elpd"]).sum())
    assert abs(w["elpd_waic"] - float(rt["elpd"].sum())) <= e_total + 1e-15 * 30 * abs(w["elpd_waic"])
    # ... and against scipy / numpy on the samples in float64: libm's log against the engine's in l, so at the engine-against-libm
    # bound of the CPU tests per term (1e-12 / 2e-5 relative to max(1, |l|)) carried through the sums
    xs = x.astype(np.float64)
    mu, sigma = xs[:, 0, :].ravel(), xs[:, 1, :].ravel()
    with np.errstate(all="ignore"):
        l64 = -0.5 * ((data[:, None] - mu[None, :]) / sigma[None, :]) ** 2 - np.log(sigma)[None, :] - LOG_SQRT_2PI
    assert np.isfinite(l64).all()
    tol = {"f64": 1e-12, "f32": 2e-5}[real] * max(1.0, float(np.abs(l64).max()))
    lppd = logsumexp(l64, axis=1) - math.log(l64.shape[1])
    var = l64.var(axis=1, ddof=1)
    tab = w["pointwise"]
    assert np.all(np.abs(tab["lppd"] - lppd) <= tol + P.MARGIN * rt["e_lppd"].astype(np.float64))
    spread = 2.0 * np.sqrt(var) + tol                                           # |d var| <= (2 mean|l - mean| + tol) tol <= (2 sd + tol) tol
    assert np.all(np.abs(tab["var"] - var) <= tol * spread + P.MARGIN * rt["e_var"].astype(np.float64) + 1e-13)
    assert w["waic"] == -2.0 * w["elpd_waic"] and w["p_waic"] == pytest.approx(var.sum(), abs=30 * tol * float(spread.max()) + 1e-9)
    dic = chain.dic(normal_ll, data)
    theta = np.array([chain.mean("mu"), chain.mean("sigma")])
    d_bar = -2.0 * l64.mean(axis=1).sum()
    d_hat = -2.0 * float(np.sum(-0.5 * ((data - theta[0]) / theta[1]) ** 2 - math.log(theta[1]) - LOG_SQRT_2PI))
    assert dic["d_bar"] == pytest.approx(d_bar, abs=60 * tol + 1e-9) and dic["d_hat"] == pytest.approx(d_hat, rel=1e-12)
    assert dic["dic"] == pytest.approx(2 * d_bar - d_hat, abs=120 * tol + 1e-9) and dic["p_d"] > 0
    with pytest.raises(mhx.ArgumentError, match="no host evaluator"):
        chain.dic(mhx.HipPointwise(tp.source, data))
    # a hand-written source gives the same bits as the traced one it restates
    hand = run.pointwise(mhx.HipPointwise(tp.source, data))
    for k in ("max", "sumexp", "s1", "s2", "bad", "shift"):
        assert P.same_bits(hand[k], sums[k])
    # a derived run is a source: (mu, sigma) -> (mu, 2 sigma)
    der = run.derive(lambda t: [t.mu, 2.0 * t.sigma], names=["mu", "sigma"])
    try:
        xd, _ = der.samples()
        got = der.pointwise(tp)
        _check(mhx, real, got, P.sums(P.host_matrix(oracle, tp.source)(xd, data), 200, 257), "derived run")
        with pytest.raises(mhx.MhxError, match="derived run"):
            der.init(None)
        with pytest.raises(mhx.MhxError, match="derived run"):
            der.sample(1, 0, 1, 0)
    finally:
        der.close()
    run.close()


def test_group_of_two_members_equals_the_unsharded_call(mhx, oracle, real):
    data, model, spl = _readme_model(mhx)
    init = np.tile(np.array([[0.0], [1.0]]), (1, 130))
    whole = mhx.Run(model, spl, nchains=130, seed=11, first_chain=5)
    whole.init(init)
    whole.sample(40, 10, 1, 0)
    g = mhx.Group([0, 0])
    try:
        g.create(model, spl, nchains=130, seed=11, first_chain=5)
        g.init(init)
        g.sample(40, 10, 1, 0)
        x, _ = whole.samples()
        tp = T.trace_pointwise(normal_ll, 2, data, names=["mu", "sigma"])
        ref = P.sums(P.host_matrix(oracle, tp.source)(x, data), 40, 130)
        one = whole.pointwise(tp)
        both = g.pointwise(tp)
        _check(mhx, real, one, ref, "unsharded")
        _check(mhx, real, both, ref, "group")                                   # max, bad, shift and T bit for bit in there
        assert both["T"] == one["T"] == 40 * 130 and P.same_bits(both["max"], one["max"]) and P.same_bits(both["bad"], one["bad"])
    finally:
        g.close()
        whole.close()
