"""Autocovariance sums on the device (mhx_run_autocovariance and its ctx and group forms: a centre pass, then lag tiles that keep
a window of the series in registers) and what the host makes of them (Chains.autocor, Chains.autocorr_time), against the
extended-precision reference tests/acf_ref.py at MARGIN = 4 times the reference's own error bounds.  Crafted tensors are planted
in a run's device sample buffer; integers (nvalid, window, truncated) are compared with `==`."""
import ctypes as C

import numpy as np
import pytest

import acf_ref as A
import diag_ref as R
from planted import plant_ptr as _plant

pytestmark = pytest.mark.gpu
K = R.MARGIN
SENT_D, SENT_I = -12345.678, -987654321
I32P, I64P, DP = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
NONFINITE = (R.R_NAN, R.R_NEG_NAN, R.R_PINF, R.R_NINF)
MODES = (("un", "acov", False), ("nm", "nacov", True))


def _raw(fn, head, params, lags, chains, normalise, acov_null=False, nlags=None):
    """one raw call, the outputs pre-filled with a sentinel: (rc, message, acov, nvalid).  chains None: the group form"""
    import mhx
    params = np.ascontiguousarray(params, dtype=np.int32)
    lags = np.ascontiguousarray(lags, dtype=np.int32)
    nl = len(lags) if nlags is None else nlags
    acov, nvalid = np.full((len(params), max(len(lags), 1)), SENT_D), np.full(len(params), SENT_I, dtype=np.int64)
    args = list(head) + [params.ctypes.data_as(I32P), len(params), lags.ctypes.data_as(I32P), nl]
    if chains is not None:
        args += [int(chains[0]), int(chains[1])]
    rc = fn(*args, int(normalise), None if acov_null else acov.ctypes.data_as(DP), nvalid.ctypes.data_as(I64P))
    return rc, mhx.lib().mhx_last_error().decode(), acov, nvalid


def _untouched(acov, nvalid):
    return bool(np.all(acov == SENT_D) and np.all(nvalid == SENT_I))


_worst = {}


def _near(got, want, bound, width, what, where, k=K):
    """|got - want| <= k bound, entry by entry (NaN: on both sides); prints the largest ratio"""
    got, want, bound = np.atleast_1d(got), np.atleast_1d(want), np.atleast_1d(bound)
    wf = want.astype(np.float64)
    nan = np.isnan(wf)
    assert np.array_equal(np.isnan(got), nan), "%s %s: NaN pattern, got %r, reference %r" % (what, where, got, wf)
    if nan.all():
        return
    err = np.abs(got[~nan].astype(R.LD) - want[~nan])
    b = bound[~nan]
    ratio = np.where(b > 0, err / np.where(b > 0, b, 1), np.where(err == 0, 0.0, np.inf)).astype(np.float64)
    worst = float(ratio.max())
    _worst[(width, what)] = max(_worst.get((width, what), 0.0), worst)
    print("ACF_RATIO %s %s %.3g   %s" % (width, what, worst, where))
    i = int(ratio.argmax())
    assert worst <= k, "%s %s: entry %d got %.17g, reference %.17g, error %.3g = %.3g x bound %.3g" % (
        what, where, i, float(got[~nan][i]), float(want[~nan][i]), float(err[i]), worst, float(b[i]))


def _check_sums(got, nvalid, st, rows, pick, width, where):
    """both modes' sums of the rows `rows` (reference entries `pick` of each row's dense reference) and nvalid"""
    for (mode, key, _), (acov, nv) in zip(MODES, zip(got, nvalid)):
        for i, r in enumerate(rows):
            s = st[r]
            w = "%s row %d (%s)" % (where, r, R.ROWS[r])
            _near(acov[i], s[key][pick], s["b_" + key][pick], width, key, w)
            assert nv[i] == s["nvalid"], (w, mode, nv[i], s["nvalid"])


def _check_windows(got, st, rows, width, where):
    """tau, window and truncated of rows whose lags are 0..N-1, wherever the window margins admit the row (acf_ref.admitted)"""
    import mhx
    for (mode, key, _), acov in zip(MODES, got):
        rho = mhx.autocorrelation(acov)
        for i, r in enumerate(rows):
            s = st[r]
            w = "%s row %d (%s) %s" % (where, r, R.ROWS[r], mode)
            if not s["finite"] or not s[key][0] > 0:
                assert np.isnan(rho[i]).all(), w
                tau, M, trunc = mhx.integrated_time(rho[i])
                assert np.isnan(tau) and trunc and M == len(rho[i]) - 1, w
                continue
            _near(rho[i], s[mode]["rho"], s[mode]["b_rho"], width, "rho_" + mode, w)
            if A.admitted(s, mode):
                tau, M, trunc = mhx.integrated_time(rho[i])
                assert (M, trunc) == (s[mode]["window"], s[mode]["truncated"]), (w, M, trunc, s[mode]["window"])
                _near(tau, s[mode]["tau"], s[mode]["b_tau"], width, "tau_" + mode, w)


def _both(run, lags, params=None, chains=None):
    a = [run.autocovariance(lags, params=params, chains=chains, normalise=nm) for _, _, nm in MODES]
    return [x[0] for x in a], [x[1] for x in a]


def _lag_sets(mhx, real, N):
    Rt = mhx.ACF_TILE[real]
    sets = [[0], [N - 1]]
    if N > 50:
        sets.append([1, 5, 10, 50])
    if N > 2 * Rt:
        sets.append([Rt - 1, Rt, Rt + 1, 2 * Rt])       # straddles tile edges ...
    if N > 4 * Rt:
        sets.append([Rt - 1, 3 * Rt, 3 * Rt + 1])       # ... and leaves a tile in between that is not launched
    return sets


def _crafted_case(mhx, real, N, nch, seed, rows=None):
    rows = list(range(len(R.ROWS))) if rows is None else list(rows)
    x, st = A.reference(N, nch, real, seed, np.arange(N), rows=rows)
    where = "N%d-C%d" % (N, nch)
    run, _ = _plant(mhx, np.ascontiguousarray(x))
    try:
        got, nv = _both(run, np.arange(N), params=rows)
        sparse = [(lg, _both(run, lg, params=rows)) for lg in _lag_sets(mhx, real, N)]
        finite = [r for r in rows if r not in NONFINITE]
        alone = _both(run, np.arange(N), params=finite)
    finally:
        run.close()
    _check_sums(got, nv, st, rows, slice(None), real, where + " all lags")
    _check_windows(got, st, rows, real, where)
    for lg, (g, n) in sparse:
        _check_sums(g, n, st, rows, np.array(lg), real, where + " lags %s" % lg)
    # the rows with a NaN or an infinity are NaN at every lag and leave the others as a call without them gives them: bit for bit
    # where at most two atomics meet in a sum (their order cannot matter then), else within the bounds
    for m in range(2):
        for r in NONFINITE:
            if r in rows:
                assert np.isnan(got[m][rows.index(r)]).all() and nv[m][rows.index(r)] == 0, (where, r)
        sub = got[m][[rows.index(r) for r in finite]]
        if ((nch + 63) // 64) * ((N + A.CHUNK - 1) // A.CHUNK) <= 2:
            assert np.array_equal(sub, alone[0][m]), where
        assert np.array_equal(nv[m][[rows.index(r) for r in finite]], alone[1][m]), where
    _check_sums(alone[0], alone[1], st, finite, slice(None), real, where + " finite rows alone")


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_crafted_tensor_matches_the_reference(mhx, real, case):
    _crafted_case(mhx, real, case[0], case[1], case[5])


@pytest.mark.parametrize("which", ["2", "R", "R+1", "2R+1"])
def test_series_as_short_as_a_tile(mhx, real, which):
    Rt = mhx.ACF_TILE[real]
    N = {"2": 2, "R": Rt, "R+1": Rt + 1, "2R+1": 2 * Rt + 1}[which]
    _crafted_case(mhx, real, N, 65, 3)


def test_one_long_chain_all_lags(mhx, real):
    """N = 4099, C = 1, lags 0..4098: five time chunks, one live lane, more tiles than one block has waves"""
    _crafted_case(mhx, real, 4099, 1, 5, rows=(2, 5, R.R_NAN))


RANGES = [None, (3, 70), (256, 1), (64, 0)]


def test_chain_ranges(mhx, real):
    """C = 257: a range that begins and ends mid-wave, the last chain alone, count 0 = to the last chain.  The -inf stretch of row
    neg_inf sits in chain 256: a range without that chain reads a finite row."""
    N, nch, seed = 97, 257, 2
    x = A.tensor(N, nch, real, seed)
    rows = [0, 5, 9, R.R_CONST_PC, R.R_NINF]
    lags = [0, 1, 5, 10, 50]
    run, _ = _plant(mhx, np.ascontiguousarray(x))
    try:
        got = {rg: _both(run, lags, params=rows, chains=rg) for rg in RANGES}
    finally:
        run.close()
    for rg in RANGES:
        st = {r: A.acf_stats(x[:, r, :], real, lags, chains=rg) for r in rows}
        _check_sums(got[rg][0], got[rg][1], st, rows, slice(None), real, "N97-C257 chains %s" % (rg,))
        assert st[R.R_NINF]["finite"] == (rg == (3, 70))
        assert st[R.R_CONST_PC]["nvalid"] == 0 and not got[rg][0][0][3].any()


def test_one_constant_chain_is_left_out_and_counted_out(mhx, real):
    N, nch, seed = 97, 65, 2
    x = np.array(A.tensor(N, nch, real, seed))
    x[:, 0, 7] = x[0, 0, 7]
    run, _ = _plant(mhx, x)
    try:
        got, nv = _both(run, np.arange(N), params=[0])
    finally:
        run.close()
    st = {0: A.acf_stats(x[:, 0, :], real, np.arange(N))}
    assert st[0]["nvalid"] == nch - 1
    _check_sums(got, nv, st, [0], slice(None), real, "one constant chain")
    _check_windows(got, st, [0], real, "one constant chain")


def test_ctx_form_on_the_same_pointer(mhx, real):
    """one block of chains and one time chunk: a single atomic per sum, so both forms return the same bits"""
    N, nch, seed = 97, 64, 1
    x = A.tensor(N, nch, real, seed)
    run, ptr = _plant(mhx, np.ascontiguousarray(x))
    lib = mhx.lib()
    rows, lags = [9, 0, 0, R.R_NAN, R.R_CONST], np.arange(N)
    try:
        for nm in (0, 1):
            rc, msg, a_run, n_run = _raw(lib.mhx_run_autocovariance, [run.h], rows, lags, (0, 0), nm)
            assert rc == 0, msg
            rc, msg, a_ctx, n_ctx = _raw(lib.mhx_ctx_autocovariance, [run.ctx.h, ptr, N, x.shape[1], nch], rows, lags, (0, 0), nm)
            assert rc == 0, msg
            assert np.array_equal(a_run, a_ctx, equal_nan=True) and np.array_equal(n_run, n_ctx)
            assert np.array_equal(a_run[1], a_run[2]) and np.isnan(a_run[3]).all() and not a_run[4].any()
            assert list(n_run) == [A.acf_stats(x[:, r, :], real, [0])["nvalid"] for r in rows] and n_run[1] == nch
    finally:
        run.close()


def test_group_sums_equal_the_unsharded_run(mhx, real):
    d, Cn, N = 3, 67, 21
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(d), 1.5 * mhx.I))
    init = np.random.default_rng(3).normal(size=(d, Cn))
    g = mhx.Group([0, 0, 0])
    g.create(model, spl, nchains=Cn, seed=11, first_chain=5)
    g.init(init)
    g.sample(N)
    whole = mhx.Run(model, spl, nchains=Cn, seed=11, first_chain=5)
    whole.init(init)
    whole.sample(N)
    shards = [r.samples()[0] for r in g.runs]
    assert np.array_equal(whole.samples()[0], np.concatenate(shards, axis=2))
    lags = np.arange(N)
    u64 = R.U["f64"]
    for mode, key, nm in MODES:
        got, nv = g.autocovariance(lags, normalise=nm)
        want, wnv = whole.autocovariance(lags, normalise=nm)
        assert got.shape == (d + 1, N) and np.array_equal(nv, wnv)
        for r in range(d + 1):
            parts = [A.acf_stats(s[:, r, :], real, lags) for s in shards]
            ref = sum(p[key] for p in parts)
            bound = sum(p["b_" + key] for p in parts) + len(parts) * u64 * sum(np.abs(p[key]) for p in parts)
            _near(got[r], ref, bound, real, "group_" + key, "row %d" % r)
            _near(want[r], ref, bound, real, key, "unsharded row %d" % r)
            assert nv[r] == sum(p["nvalid"] for p in parts)
    with pytest.raises(mhx.ArgumentError, match="autocovariance"):
        g.autocovariance([0, N])
    whole.close()
    g.close()


SHAPES = [(33, 67), (1000, 1), (5, 3), (2, 257), (1, 64), (17, 241), (3, 700)]       # tests/test_gpu_histogram.py::SHAPES


@pytest.mark.parametrize("N,Cn", SHAPES)
def test_autocor_of_real_chains(mhx, real, N, Cn):
    model = mhx.DensityModel(mhx.IsoGaussian(3))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(3), 1.5 * mhx.I))
    chain = mhx.sample(model, spl, N, Cn, initial_params=np.random.default_rng(5).normal(size=(3, Cn)), seed=5)
    run = chain.state
    try:
        if N < 2:
            with pytest.raises(mhx.MhxError, match="mhx_run_autocovariance"):
                chain.autocor(lags=[0])
            return
        lags = [k for k in (1, 5, 10, 50) if k < N]
        with pytest.raises(mhx.ArgumentError, match="autocor: lag %d" % N):
            chain.autocor(lags=lags + [N])
        for moc in (False, True):
            key = "nacov" if moc else "acov"
            for rg in (None, (Cn - 1, 1)):
                tab = chain.autocor(lags=lags, mean_of_chains=moc, chains=rg)
                assert tab["parameters"] == chain.params() and tab["lags"] == lags and tab["autocor"].shape == (3, len(lags))
                assert str(tab).startswith("Autocorrelation")
                for i in range(3):
                    s = A.acf_stats(chain.value[:, i, :], real, [0] + lags, chains=rg)
                    if not s[key][0] > 0:                                  # no chain of the range ever moved
                        assert np.isnan(tab["autocor"][i]).all()
                        continue
                    rho, b = A.ratio(s[key], s["b_" + key])
                    _near(tab["autocor"][i], rho[1:], b[1:], real, "autocor", "N%d-C%d %s %s row %d" % (N, Cn, key, rg, i))
        shown = chain.autocor(lags=[0] + lags)
        assert shown["lags"] == [0] + lags and np.all(shown["autocor"][:, 0] == 1.0)
    finally:
        run.close()


def test_autocorr_time_of_one_ensemble(mhx, real):
    """3 ensembles of 8 walkers: ensemble=1 is chains [8, 16) -- the walkers of one ensemble, never those of another"""
    d, W, E, N = 2, 8, 3, 200
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = mhx.Ensemble(W, mhx.StretchProposal(mhx.MvNormal(mhx.zeros(d), mhx.I)))
    chain = mhx.sample(model, spl, mhx.MCMCThreads(), N, E, seed=3)
    run = chain.state
    try:
        assert chain.value.shape == (N, d + 1, W * E) and run.n_ensembles == E
        at = chain.autocorr_time(ensemble=1)
        acov, nv = run.autocovariance(np.arange(N), params=[0, 1], chains=(W, W), normalise=True)
        assert np.array_equal(nv, [W, W]) and np.array_equal(at["nvalid"], nv)
        for i in range(d):
            st = A.acf_stats(chain.value[:, i, :], real, np.arange(N), chains=(W, W))
            _near(acov[i], st["nacov"], st["b_nacov"], real, "nacov", "ensemble 1 row %d" % i)
            tau, M, trunc = mhx.integrated_time(mhx.autocorrelation(acov[i]))
            if A.admitted(st, "nm"):
                assert (at["window"][i], bool(at["truncated"][i])) == (M, trunc) == (st["nm"]["window"], st["nm"]["truncated"])
                _near(at["tau"][i], st["nm"]["tau"], st["nm"]["b_tau"], real, "tau_nm", "ensemble 1 row %d" % i)
                assert bool(at["converged"][i]) == (N >= 50 * at["tau"][i])
        assert at["parameters"] == chain.params()
        capped = chain.autocorr_time(max_lag=3, ensemble=1)             # a window that is not reached within the lags computed
        assert np.all(capped["window"] <= 3)
        for bad in (3, -1):
            with pytest.raises(mhx.ArgumentError, match="autocorr_time: ensemble"):
                chain.autocorr_time(ensemble=bad)
        with pytest.raises(mhx.ArgumentError, match="autocorr_time: max_lag"):
            chain.autocorr_time(max_lag=N)
    finally:
        run.close()


def test_refusals(mhx, real):
    N, nch, d1 = 9, 10, 4
    model = mhx.DensityModel(mhx.IsoGaussian(3))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(3), 1.5 * mhx.I))
    init = np.random.default_rng(5).normal(size=(3, nch))
    chain = mhx.sample(model, spl, N, nch, initial_params=init, seed=5)
    run = chain.state
    lib = mhx.lib()
    ptr, n_saved = C.c_void_p(), C.c_int64()
    mhx.check(lib.mhx_run_device_samples(run.h, C.byref(ptr), None, C.byref(n_saved)))
    g = mhx.Group([0])
    g.create(model, spl, nchains=nch, seed=5)
    g.init(init)
    g.sample(N)
    forms = [("mhx_run_autocovariance", lib.mhx_run_autocovariance, [run.h], (0, 0)),
             ("mhx_ctx_autocovariance", lib.mhx_ctx_autocovariance, [run.ctx.h, ptr, N, d1, nch], (0, 0)),
             ("mhx_group_autocovariance", lib.mhx_group_autocovariance, [g.h], None)]
    for name, fn, head, rg in forms:
        rc, msg, acov, nvalid = _raw(fn, head, [0, 3], [0, 2, 8], rg, 0)
        assert rc == 0 and not np.any(acov == SENT_D) and not np.any(nvalid == SENT_I), (name, msg)
        bad = [dict(lags=[0, 5, 3]), dict(lags=[0, 3, 3]), dict(lags=[0, N]), dict(lags=[-1, 2]), dict(lags=[0, 2], nlags=0),
               dict(params=[0, d1]), dict(params=[-1, 0]), dict(acov_null=True)]
        if rg is not None:
            bad += [dict(chains=(0, nch + 1)), dict(chains=(nch, 0)), dict(chains=(4, 7)), dict(chains=(-1, 2))]
        for kw in bad:
            rc, msg, acov, nvalid = _raw(fn, head, kw.get("params", [0, 3]), kw.get("lags", [0, 2, 8]), kw.get("chains", rg), 1,
                                         acov_null=kw.get("acov_null", False), nlags=kw.get("nlags"))
            assert rc == mhx.MHX_EINVAL and "autocovariance" in msg and _untouched(acov, nvalid), (name, kw, rc, msg)
            if rg is not None:
                assert name in msg, (name, kw, msg)
        # the offending entry is named
    rc, msg, _, _ = _raw(lib.mhx_run_autocovariance, [run.h], [0], [0, 5, 3], (0, 0), 0)
    assert "entry 2" in msg and "3 after 5" in msg, msg
    with pytest.raises(mhx.ArgumentError, match="mhx_run_autocovariance"):
        run.autocovariance([0, 1], chains=(0, nch + 1))
    # moments mode keeps no sample tensor (the shape of tests/test_gpu_histogram.py)
    dm, Cm = 40, 96
    s = float(np.float32(2.38 / dm ** 0.5))
    mom = mhx.Run(mhx.DensityModel(mhx.Funnel(dm)), mhx.RWMH(mhx.MvNormal(mhx.zeros(dm), s * s * mhx.I)), nchains=Cm, seed=2)
    mom.init(np.random.default_rng(8).normal(size=(dm, Cm)))
    mom.sample(10, 5, 5, 0, save="moments")
    rc, msg, acov, nvalid = _raw(lib.mhx_run_autocovariance, [mom.h], [0, 3], [0, 2], (0, 0), 0)
    assert rc == mhx.MHX_ESTATE and "mhx_run_autocovariance" in msg and _untouched(acov, nvalid), (rc, msg)
    with pytest.raises(mhx.MhxError, match="mhx_run_autocovariance"):
        mom.autocovariance([0, 1])
    mom.close()
    # a single saved draw: no autocovariance
    one = mhx.Run(model, spl, nchains=nch, seed=5)
    one.init(init)
    one.sample(1)
    rc, msg, acov, nvalid = _raw(lib.mhx_run_autocovariance, [one.h], [0], [0], (0, 0), 0)
    assert rc == mhx.MHX_ESTATE and "mhx_run_autocovariance" in msg and _untouched(acov, nvalid), (rc, msg)
    one.close()
    g.close()
    run.close()


def test_largest_ratios_are_reported():
    """not a check: prints the largest |error| / bound per quantity and width seen by the tests above"""
    for (width, what), v in sorted(_worst.items()):
        print("ACF_WORST %s %s %.3g" % (width, what, v))
