"""GPU: PSIS-LOO per data row (mhx_run_psis / mhx_ctx_psis, Run.psis, Chains.loo; csrc/mhx_psis_kernels.h)
against tests/psis_ref.py: the same MHX_POINTWISE text compiled for the host gives l[i, s] bit for bit, and from it -- in 80-bit
arithmetic -- the definitions of include/mhx.h with a bound of the device's computation for every inexact column, derived there.

  exact     tau, lmin, n_below, bad, T, M and the tails equal the reference bit for bit
  bounded   elpd_loo, khat, sigma and B within MARGIN x bound on EVERY row of every case; the module prints the largest |error| / bound
            it met per width and column (DESIGN.md section 6.5.8 records them)

Shapes: the smallest that cross a wave, a block, a strip and a row tile -- C = 1, 63, 65, 257; n_saved = 1, 3, 17, 35 (a strip is 16
draws); nrows = 1, 9, 17 (a tile is 4 rows); rowlen = 1, 3.  They include T = 1, 3, 17 (M < 5: khat = +inf, raw weights) and T = 189 (M = 37,
the 0.2 T branch).  The planted tensor: mu ~ N(0.1, 0.2^2), sigma = |N(1, 0.15^2)| + 0.2, the README's Normal line, rows y ~ N(0, 1) and
one row y = 4 (khat above 1)."""
import ctypes as C
import math

import numpy as np
import pytest

import mhx.trace as T
import pointwise_ref as P
import psis_ref as R
from planted import plant_ptr

pytestmark = pytest.mark.gpu

# the README's Normal line on (mu, sigma) = (x[0], x[1]); y is the LAST entry of the row, so that rows of 3 differ from rows of 1
SRC_NORMAL = """
MHX_POINTWISE(x, r, m, d, data, ndata)
{
    const mhx_real z = (r[m - 1] - x[0]) / x[1];
    return MHX_R(-0.5) * z * z - mhx_log(x[1]) - MHX_R(0.9189385332046727);
}
"""
SRC_INT = "MHX_POINTWISE(x, r, m, d, data, ndata) { return x[0] + r[0]; }\n"
SRC_BAD = "MHX_POINTWISE(x, r, m, d, data, ndata) { return x[0] +* ; }\n"
# as tests/test_gpu_pointwise.py: -inf, +inf and NaN are switched on by the ROWS (r[1] against the planted v = 1.5)
SRC_LOG = """
MHX_POINTWISE(x, r, m, d, data, ndata)
{
    return mhx_fma(r[0], mhx_log(x[d - 1] - r[1]), r[m - 1]);
}
"""
LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)
CAP = (40, 3, 257)                      # the planted buffer: every case's tensor fits
RATIOS = {}                             # (width, column) -> largest |error| / bound met
COLS = ("elpd_loo", "khat", "sigma", "tau", "lmin", "body", "n_below", "bad")


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
        print("psis ratio %s %-8s %.4f" % (k[0], k[1], RATIOS[k]))


def _buffer(mhx, real):
    if real not in _BUF:
        _BUF[real] = plant_ptr(mhx, np.zeros(CAP, dtype=np.float64 if real == "f64" else np.float32))
    return _BUF[real]


def _ctx_psis(mhx, real, x, source, rows, reff=1.0, data=None, tails=True):
    """mhx_ctx_psis on x [N][d + 1][C], copied into the width's device buffer: a dict, or (rc, out8, tails, T, M) of a refusal"""
    run, ptr = _buffer(mhx, real)
    x = np.ascontiguousarray(x, dtype=run.real)
    assert x.size <= CAP[0] * CAP[1] * CAP[2]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(ptr, x.ctypes.data_as(C.c_void_p), x.nbytes, 1) == 0
    rr = np.ascontiguousarray(rows, dtype=run.real)
    rr = rr.reshape(rr.shape[0], -1)
    dat = None if data is None else np.ascontiguousarray(data, dtype=run.real).ravel()
    nrows = rr.shape[0]
    M = R.tail_length(x.shape[0] * x.shape[2], reff) if reff > 0 and math.isfinite(reff) else 0
    out, tl, T_, M_ = np.full((8, nrows), 77.0), np.full((nrows, M), 55.0), C.c_int64(-1), C.c_int64(-1)
    dp = C.POINTER(C.c_double)
    rc = mhx.lib().mhx_ctx_psis(run.ctx.h, ptr, x.shape[0], x.shape[1], x.shape[2], source.encode(), mhx._lib.rptr(rr), nrows, rr.shape[1],
                                mhx._lib.rptr(dat), 0 if dat is None else dat.size, reff, out.ctypes.data_as(dp),
                                tl.ctypes.data_as(dp) if tails else None, C.byref(T_), C.byref(M_))
    if rc:
        return rc, out, tl, T_.value, M_.value
    res = {k: out[j] for j, k in enumerate(COLS)}
    res.update(T=int(T_.value), M=int(M_.value), tails=tl)
    return res


def _same(a, b):
    for k in COLS + ("tails",):
        if not P.same_bits(a[k], b[k]):
            return k
    return None if (a["T"], a["M"]) == (b["T"], b["M"]) else "T, M"


def _check(real, got, ref, tag):
    """the exact parts bit for bit, the bounded parts within MARGIN x bound on every row"""
    assert isinstance(got, dict), (tag, got[0])
    assert got["T"] == ref["T"] and got["M"] == ref["M"], (tag, got["T"], got["M"], ref["T"], ref["M"])
    for k in R.EXACT + ("tails",):
        assert P.same_bits(got[k], ref[k]), (tag, k, got[k], ref[k])
    for k in R.BOUNDED:
        ok, ratio = P.within(got[k], ref[k], ref["e_" + k])
        print("  %s %s %s ratio %.4g" % (tag, real, k, ratio))
        RATIOS[(real, k)] = max(RATIOS.get((real, k), 0.0), ratio)
        assert ok, (tag, k, ratio, got[k], ref[k].astype(np.float64), ref["e_" + k].astype(np.float64))


def _planted(real, N, nch, seed):
    """[N][3][C]: mu ~ N(0.1, 0.2^2), sigma = |N(1, 0.15^2)| + 0.2, and an lp row nothing reads"""
    rng = np.random.default_rng(seed)
    x = np.zeros((N, 3, nch))
    x[:, 0, :] = rng.normal(0.1, 0.2, size=(N, nch))
    x[:, 1, :] = np.abs(rng.normal(1.0, 0.15, size=(N, nch))) + 0.2
    return np.ascontiguousarray(x.astype(np.float64 if real == "f64" else np.float32))


def _planted_rows(real, rowlen, seed=3):
    """17 rows: y ~ N(0, 1), y = 4 in row 8; y is the last entry, the others (rowlen 3) are decoys"""
    rng = np.random.default_rng(seed)
    rows = rng.normal(size=(17, rowlen)) * 10.0
    rows[:, -1] = rng.normal(size=17)
    rows[8, -1] = 4.0
    return rows.astype(np.float64 if real == "f64" else np.float32)


@pytest.mark.parametrize("nch", [1, 63, 65, 257])
def test_every_shape_is_within_the_reference_bound(mhx, oracle, real, nch):
    host = P.host_matrix(oracle, SRC_NORMAL)
    for N in (1, 3, 17, 35):
        x = _planted(real, N, nch, 100 * N + nch)
        for rowlen in (1, 3):
            rows = _planted_rows(real, rowlen)
            l = host(x, rows)
            for nrows in (1, 9, 17):
                got = _ctx_psis(mhx, real, x, SRC_NORMAL, rows[:nrows])
                ref = R.reference(l[:nrows], N, nch)
                _check(real, got, ref, "C%d N%d rows%dx%d" % (nch, N, nrows, rowlen))
                if ref["M"] == 0:
                    assert np.all(np.isposinf(got["khat"])) and np.all(np.isnan(got["sigma"])) and np.all(got["n_below"] == 0)
    if nch == 63:
        assert R.tail_length(3 * 63) == 37                                      # T = 189: the 0.2 T branch
    if nch == 257:                                                              # both classes of the printout occur at T = 8995
        assert ref["khat"][8] > 1.0 and np.all(ref["khat"][:8] < 0.7), ref["khat"]


def _int_case(real, kind):
    """35 x 257 integer draws, l = x[0] + r[0] exact in both widths.  T = 8995, M = 285.
    levels   40 levels: n_below < M, copies of tau in the tail
    repeat   more than M draws at the lowest level: a tail of one repeated value
    quarter  185 distinct values below a level that holds thousands: 100 >= floor(M / 4 + 1 / 2) of the x_j are 0, x* among them"""
    rng = np.random.default_rng(41)
    N, nch = 35, 257
    xi = rng.integers(1, 21, size=N * nch)
    if kind == "levels":
        xi = rng.integers(-20, 20, size=N * nch)
    elif kind == "repeat":
        xi[rng.permutation(N * nch)[:5000]] = 0
    else:
        where = rng.permutation(N * nch)
        xi[where[:4000]] = 0
        xi[where[4000:4185]] = -np.arange(1, 186)
    x = np.zeros((N, 2, nch))
    x[:, 0, :] = xi.reshape(N, nch)
    return x.astype(np.float64 if real == "f64" else np.float32), xi


@pytest.mark.parametrize("kind", ["levels", "repeat", "quarter"])
def test_ties(mhx, real, kind):
    x, xi = _int_case(real, kind)
    ri = np.array([0, -3, 7, 2, 11])
    l = (xi[None, :] + ri[:, None]).astype(np.float64)
    got = _ctx_psis(mhx, real, x, SRC_INT, ri.astype(x.dtype))
    ref = R.reference(l, 35, 257)
    assert ref["M"] == 285
    _check(real, got, ref, kind)
    if kind == "levels":
        assert np.all(got["n_below"] < 285) and np.all(got["tails"][:, -1] == got["tau"]) and np.all(np.isfinite(got["elpd_loo"]))
    else:
        assert np.all(np.isposinf(got["khat"])) and np.all(np.isnan(got["sigma"])) and np.all(np.isfinite(got["elpd_loo"]))
        assert np.all(got["n_below"] == (0 if kind == "repeat" else 185))


def _edge_case(real):
    """63 chains (a partial wave) x 17 draws; v = 1.5 exactly in draw 0 of chain 0, in the last lane (chain 62, draw 9) and in two more;
    the edges are switched on by the rows, so the tensor, and every other row, is the same with and without them"""
    rng = np.random.default_rng(5)
    dt = np.float64 if real == "f64" else np.float32
    x = np.ascontiguousarray(rng.uniform(2.0, 6.0, size=(17, 2, 63)).astype(dt))
    for t, c in ((0, 0), (9, 62), (16, 31), (3, 7)):
        x[t, 0, c] = 1.5
    plain = np.stack([rng.uniform(0.5, 2.0, 10), rng.uniform(-1.0, 1.0, 10), rng.uniform(-3.0, 3.0, 10)], axis=1).astype(dt)
    edged = plain.copy()
    edged[1] = (2.0, 1.5, 0.25)          # -inf at the four planted draws
    edged[3] = (-2.0, 1.5, 0.25)         # +inf there
    edged[4] = (1.0, 1.75, 0.0)          # NaN there
    edged[6] = (1.0, 7.0, 0.0)           # NaN at every draw
    return x, plain, edged


def test_non_finite_draws_poison_their_row_only(mhx, oracle, real):
    x, plain, edged = _edge_case(real)
    host = P.host_matrix(oracle, SRC_LOG)
    base = _ctx_psis(mhx, real, x, SRC_LOG, plain)
    got = _ctx_psis(mhx, real, x, SRC_LOG, edged)
    l = host(x, edged)
    assert np.isneginf(l[1]).sum() == 4 and np.isposinf(l[3]).sum() == 4 and np.isnan(l[4]).sum() == 4 and np.isnan(l[6]).all()
    _check(real, base, R.reference(host(x, plain), 17, 63), "plain")
    _check(real, got, R.reference(l, 17, 63), "edged")
    for i, n in ((1, 4), (3, 4), (4, 4), (6, 17 * 63)):
        assert got["bad"][i] == n and np.isnan(got["tails"][i]).all()
        for k in COLS[:7]:
            assert np.isnan(got[k][i]), (i, k)
    for i in (0, 2, 5, 7, 8, 9):
        for k in COLS + ("tails",):
            assert P.same_bits(got[k][i], base[k][i]), (i, k)


def _threshold_mb(mhx, real, run, x, rows):
    """the smallest PSIS_SCRATCH_MB (to 1e-6 MiB) the call accepts: by bisection between a refusal and a success"""
    lo, hi = 1e-4, 64.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        run.ctx.set_option("PSIS_SCRATCH_MB", repr(mid))
        ok = isinstance(_ctx_psis(mhx, real, x, SRC_NORMAL, rows), dict)
        lo, hi = (lo, mid) if ok else (mid, hi)
        if hi - lo < 1e-6:
            break
    return lo, hi


def test_same_bits_under_repetition_and_options(mhx, real):
    N, nch = 35, 257
    x = _planted(real, N, nch, 21)
    rows = _planted_rows(real, 3)
    first = _ctx_psis(mhx, real, x, SRC_NORMAL, rows)
    second = _ctx_psis(mhx, real, x, SRC_NORMAL, rows)
    assert _same(first, second) is None
    run, _ = _buffer(mhx, real)
    try:
        for bits in (8, 10, 11):
            run.ctx.set_option("SELECT_BITS", str(bits))
            assert _same(_ctx_psis(mhx, real, x, SRC_NORMAL, rows), first) is None, bits
        run.ctx.set_option("SELECT_BITS", None)
        for tile in (1, 2, 8):
            run.ctx.set_option("PSIS_ROWS", str(tile))
            assert _same(_ctx_psis(mhx, real, x, SRC_NORMAL, rows), first) is None, tile
        run.ctx.set_option("PSIS_ROWS", None)
        # the smallest budget that is accepted holds one row and not two: 17 batches of one row
        lo, hi = _threshold_mb(mhx, real, run, x, rows)
        run.ctx.set_option("PSIS_SCRATCH_MB", repr(hi))
        assert _same(_ctx_psis(mhx, real, x, SRC_NORMAL, rows), first) is None
        run.ctx.set_option("PSIS_SCRATCH_MB", repr(lo))
        rc, out, tl, T_, M_ = _ctx_psis(mhx, real, x, SRC_NORMAL, rows)
        assert rc == mhx.MHX_EINVAL and "PSIS_SCRATCH_MB" in mhx.lib().mhx_last_error().decode()
        assert np.all(out == 77.0) and np.all(tl == 55.0) and (T_, M_) == (-1, -1)
    finally:
        for name in ("SELECT_BITS", "PSIS_ROWS", "PSIS_SCRATCH_MB"):
            run.ctx.set_option(name, None)


def test_reff_and_refusals(mhx, oracle, real):
    N, nch = 35, 65
    x = _planted(real, N, nch, 9)
    rows = _planted_rows(real, 1)[:9]
    l = P.host_matrix(oracle, SRC_NORMAL)(x, rows)
    assert R.tail_length(N * nch, 0.5) == math.ceil(3 * math.sqrt(N * nch / 0.5)) != R.tail_length(N * nch, 1.0)
    _check(real, _ctx_psis(mhx, real, x, SRC_NORMAL, rows, reff=0.5), R.reference(l, N, nch, reff=0.5), "reff 0.5")
    no_tails = _ctx_psis(mhx, real, x, SRC_NORMAL, rows, tails=False)            # tail_out = NULL
    assert np.all(no_tails["tails"] == 55.0)
    _check(real, dict(no_tails, tails=R.reference(l, N, nch)["tails"]), R.reference(l, N, nch), "no tails")
    for reff in (0.0, -1.0, math.inf, math.nan):
        rc, out, tl, T_, M_ = _ctx_psis(mhx, real, x, SRC_NORMAL, rows, reff=reff)
        assert rc == mhx.MHX_EINVAL and "reff" in mhx.lib().mhx_last_error().decode()
        assert np.all(out == 77.0) and (T_, M_) == (-1, -1)
    rc, out, tl, T_, M_ = _ctx_psis(mhx, real, x, SRC_BAD, rows)
    msg = mhx.lib().mhx_last_error().decode()
    assert rc == mhx.MHX_EINVAL and "pointwise.hip" in msg and "does not compile" in msg
    assert np.all(out == 77.0) and np.all(tl == 55.0) and (T_, M_) == (-1, -1)
    run, ptr = _buffer(mhx, real)
    dp = C.POINTER(C.c_double)
    for nrows, rowlen in ((0, 1), (2, 0), (-1, 1), (1 << 20, 1 << 12)):
        rc = mhx.lib().mhx_ctx_psis(run.ctx.h, ptr, 3, 3, 5, SRC_INT.encode(), mhx._lib.rptr(rows), nrows, rowlen, None, 0, 1.0,
                                    out.ctypes.data_as(dp), None, None, None)
        assert rc == mhx.MHX_EINVAL and np.all(out == 77.0)
    # a second call with the same source compiles nothing
    _ctx_psis(mhx, real, x, SRC_INT, rows)
    before = run.ctx.jit_counts()
    _ctx_psis(mhx, real, x, SRC_INT, rows)
    assert run.ctx.jit_counts() == before


def _readme_model(mhx, data):
    model = mhx.DensityModel(mhx.IIDNormal(data))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(2), mhx.I))
    return model, spl


def test_readme_model_loo_end_to_end(mhx, oracle, real):
    """257 chains x 200 draws, 30 data rows: chain.loo against psis_ref on the draws copied to the host; a HipPointwise and a derived run
    are sources; mhx.compare orders the model and a deliberately worse one (sigma doubled)"""
    data = np.random.default_rng(1234).normal(0.0, 1.0, size=30)
    model, spl = _readme_model(mhx, data)
    chain = mhx.sample(model, spl, 200, 257, param_names=["mu", "sigma"], chain_type=mhx.Chains, discard_initial=100,
                       initial_params=np.array([0.0, 1.0]), seed=1234)
    run = chain.state
    x, _ = run.samples()
    tp = T.trace_pointwise(normal_ll, 2, data, names=["mu", "sigma"])
    host = P.host_matrix(oracle, tp.source)
    ref = R.reference(host(x, data), 200, 257)
    got = run.psis(normal_ll, data, names=["mu", "sigma"], tails=True)
    assert isinstance(got, mhx.PsisResult) and got["reff"] == 1.0
    _check(real, got, ref, "readme")
    loo = chain.loo(normal_ll, data)
    tab = loo["pointwise"]
    assert P.same_bits(tab["elpd_loo"], got["elpd_loo"]) and P.same_bits(tab["khat"], got["khat"])
    e_total = float((P.MARGIN * ref["e_elpd_loo"]).sum())
    assert abs(loo["elpd_loo"] - float(ref["elpd_loo"].sum())) <= e_total + 1e-15 * 30 * abs(loo["elpd_loo"])
    assert loo["looic"] == -2.0 * loo["elpd_loo"] and 0.0 < loo["p_loo"] < 10.0 and sum(loo["khat_counts"]) == 30
    assert loo["khat_threshold"] == min(1 - 1 / math.log10(200 * 257), 0.7) and "PSIS-LOO" in str(loo) and "khat" in str(tab)
    w = chain.waic(normal_ll, data)
    assert abs(loo["elpd_loo"] - w["elpd_waic"]) < 0.1                          # (a well-specified model: the two estimators agree)
    hand = run.psis(mhx.HipPointwise(tp.source, data), tails=True)
    assert _same(hand, got) is None
    der = run.derive(lambda t: [t.mu, 2.0 * t.sigma], names=["mu", "sigma"])
    try:
        xd, _ = der.samples()
        worse = der.psis(tp, tails=True)
        _check(real, worse, R.reference(host(xd, data), 200, 257), "derived run")
        loo_worse = mhx.loo_from_table(mhx.loo_table(worse, der.pointwise(tp)))
        cmp_ = mhx.compare({"doubled": loo_worse, "readme": loo, "readme waic": w})
        assert [r["name"] for r in cmp_][-1] == "doubled" and cmp_[0]["elpd_diff"] == 0.0 and cmp_[-1]["elpd_diff"] < -2 * cmp_[-1]["se_diff"] < 0
    finally:
        der.close()
    run.close()
