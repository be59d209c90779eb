"""GPU: derived quantities (mhx_run_derive / Run.derive / Chains.derive; csrc/mhx_derive_kernels.h).  The
derived tensor is compared with the same MHX_DERIVED source compiled for the host (tests/derived_ref.py: g++, no contraction, log and
exp from the oracle) BIT FOR BIT: the positions of NaN agree and every other value has the same bits (the payload and sign of a NaN
an operation makes are the processor's, not the engine's).  The statistics of a derived run are the statistics of a run whose tensor
is the host reference, planted (tests/planted.py): the same kernels on the same bytes -- bit for bit wherever the order of the
statistic's additions is fixed, and at the statistic's own test's bound where fp64 atomics of several blocks meet in one word.

Shapes: the smallest at which the frame can go wrong.  C = 1, 63, 65, 257: a lone lane, a partial wave, a wave plus one lane, a block
plus one lane.  A lane maps 4 draws together and a strip is 8 draws (2 groups), so n_saved = 1, 2, 7 and 9: one draw, fewer than a
group, a group plus a ragged end, a strip plus one.  d = 1 and 5 with nout = 7, 3 and 1.  Five map sources per width, and one that does not compile."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import derived_ref
import diag_ref as R
import hpd_ref
import rank_rhat_ref as F
import mhx.trace as T
from planted import plant

pytestmark = pytest.mark.gpu

# d = 5 -> 3 outputs, fewer than inputs: reads row d - 1 and lp only (traced: compile-time indices)
MAP_LAST = T.trace_map(lambda t, lp: [t[4] ** 2, T.where(t[4] > 0, 1.0, 0.0), lp + t[4]], 5, lp=True)
# d = 1 -> 7 outputs, more than inputs: NaN where log / sqrt have no value, +-inf at 0, and output 6 never set
SRC_EDGES = """
MHX_DERIVED(x, y, d, data, ndata)
{
    const mhx_real v = x[0];
    y.set(0, v);
    y.set(1, -v);
    y.set(2, v * v);
    y.set(3, mhx_exp(v));
    y.set(4, mhx_log(v));
    y.set(5, MHX_R(1.0) / mhx_sqrt(v));
    y.set(7, v);
    y.set(-1, v);
}
"""
# run-time loop over d and a data block: d = 5 -> 1 output
SRC_LOOP = """
MHX_DERIVED(x, y, d, data, ndata)
{
    mhx_real s = data[d];
    for (int k = 0; k < d; ++k) s = mhx_fma(data[k], x[k], s);
    y.set(0, ndata == d + 1 ? s : MHX_NAN);
}
"""
LOOP_DATA = np.array([0.5, -1.25, 2.0, 0.0, 3.5, -0.75])
MAP_SIGMA2 = lambda t: t.sigma ** 2                          # noqa: E731  (the README's line; also x[1] ** 2 of any run with d >= 2)
SRC_BAD = "MHX_DERIVED(x, y, d, data, ndata) { y.set(0, x[0] +* ); }\n"


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(bits)[~na], b.view(bits)[~nb])


def _tensor(real, N, d, nch, seed, edges=True):
    """[N][d + 1][C] draws in (-4, 4), with zeros of both signs, infinities and NaNs planted in row d - 1 and in lp"""
    R = np.float64 if real == "f64" else np.float32
    rng = np.random.default_rng(seed)
    x = rng.uniform(-4.0, 4.0, size=(N, d + 1, nch)).astype(R)
    if edges:
        special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0], dtype=R)
        for row in (d - 1, d):
            flat = x[:, row, :].reshape(-1)
            k = min(len(special), flat.size)
            pos = rng.choice(flat.size, size=k, replace=False)
            flat[pos] = special[rng.permutation(len(special))[:k]]
            x[:, row, :] = flat.reshape(N, nch)
    return np.ascontiguousarray(x)


def _host(oracle, source, x, nout, data=None):
    return derived_ref.host_map(oracle, source)(x, nout, data)


@pytest.mark.parametrize("nch", [1, 63, 65, 257])
@pytest.mark.parametrize("N", [1, 2, 7, 9])
def test_derived_tensor_equals_the_host_compiled_map(mhx, oracle, real, N, nch):
    x5, x1 = _tensor(real, N, 5, nch, 11 * N + nch), _tensor(real, N, 1, nch, 13 * N + nch)
    src5, src1 = plant(mhx, x5), plant(mhx, x1)
    try:
        cases = [(src5, x5, MAP_LAST, MAP_LAST.source, 3, None),
                 (src1, x1, mhx.HipMap(SRC_EDGES, 7), SRC_EDGES, 7, None),
                 (src5, x5, mhx.HipMap(SRC_LOOP, 1, data=LOOP_DATA), SRC_LOOP, 1, LOOP_DATA)]
        for run, x, m, source, nout, data in cases:
            der = run.derive(m)
            try:
                assert isinstance(der, mhx.DerivedRun) and (der.dim, der.n) == (nout, nch) and der.form_name() == "derived"
                got, acc = der.samples()
                want = _host(oracle, source, x, nout, data)
                assert acc is None and got.shape == (N, nout + 1, nch)
                assert _same_bits(got, want), (source, N, nch, np.argwhere(got.view(np.uint8) != want.view(np.uint8))[:4])
                assert _same_bits(got[:, nout, :], x[:, -1, :])               # the last row is the source's lp row
                if nout == 7:
                    assert np.isnan(got[:, 6, :]).all()                       # an output that is never set
                    assert np.array_equal(np.isnan(got[:, 4, :]), np.isnan(x[:, 0, :]) | (x[:, 0, :] < 0))
                    assert np.array_equal(np.isinf(got[:, 5, :]), x[:, 0, :] == 0)
                st = der.stats()
                assert st["transitions"] == 0 and st["accepted"] == 0 and st["dtype"] == real
            finally:
                der.close()
    finally:
        src5.close()
        src1.close()


def test_a_map_that_yields_nan_on_some_draws_orders_them_last(mhx, oracle, real):
    x = _tensor(real, 9, 1, 65, 5, edges=False)
    run = plant(mhx, x)
    der = run.derive(mhx.HipMap(SRC_EDGES, 7))
    try:
        got, _ = der.samples()
        nan = int(np.isnan(got[:, 4, :]).sum())
        S = 9 * 65
        assert 0 < nan < S and nan == int((x[:, 0, :] < 0).sum())            # log of the negative draws: stored as NaN
        srt = np.sort(got[:, 4, :].astype(np.float64).ravel())               # numpy: NaNs last
        os_ = der.order_statistics([0, S - nan - 1, S - nan, S - 1], params=[4])
        assert np.array_equal(os_[0, :2], srt[[0, S - nan - 1]]) and np.isnan(os_[0, 2:]).all()
        q = der.quantiles(params=[4, 2])
        assert np.isnan(q[0]).all() and np.isfinite(q[1]).all()               # a row that holds a NaN has NaN quantiles, as numpy's
    finally:
        der.close()
        run.close()


def _default_rank_diagnostics_within_the_reference_bound(der, twin, ref, real, N):
    """.rank_diagnostics() as it is called by default (split chains, max_lag = a quarter of the draws, ess_chains = 256) of the derived
    run and of its planted twin: each within MARGIN x the reference's own bound of the extended-precision reference on the reference
    tensor (tests/rank_rhat_ref.py, tests/diag_ref.py: the bound and the margin of tests/test_gpu_rank_rhat.py and
    tests/test_gpu_diagnostics.py), hence within twice that of each other.  The continuous rows: x4^2, lp + x4 and lp.  Measured on
    the MI355X, largest |error| / bound (bound, not MARGIN x bound): 0.024 in fp64 (ess_bulk), 7e-4 in fp32."""
    K = R.MARGIN
    max_lag = max(2, (N // 2) // 2)
    got = [der.rank_diagnostics(), twin.rank_diagnostics()]
    assert got[0].keys() == got[1].keys()
    for p in (0, 2, 3):
        row = np.ascontiguousarray(ref[:, p, :])
        fr = F.rank_rhat(row, real, True)
        bt = R.bulk_tail(row, real, max_lag, 256, True)
        assert bt["margin"] > K                             # the input is fit for a comparison at K bounds (tests/diag_ref.py)
        lo, hi = R.tail_interval(bt, K)
        for who, rd in zip(("derived", "twin"), got):
            for part, k in (("bulk", "rhat_bulk"), ("tail", "rhat_tail")):
                err = abs(R.LD(rd[k][p]) - fr[part]["rhat"])
                print("DIAG_RATIO %s %s %.3g   %s row %d" % (real, k, float(err / fr[part]["b_rhat"]), who, p))
                assert np.isfinite(rd[k][p]) and err <= K * fr[part]["b_rhat"], (who, k, p, rd[k][p], float(fr[part]["rhat"]))
            assert rd["rhat"][p] == max(rd["rhat_bulk"][p], rd["rhat_tail"][p])
            err = abs(R.LD(rd["ess_bulk"][p]) - bt["ess_bulk"])
            print("DIAG_RATIO %s ess_bulk %.3g   %s row %d" % (real, float(err / bt["b_ess_bulk"]), who, p))
            assert err <= K * bt["b_ess_bulk"], (who, p, rd["ess_bulk"][p], float(bt["ess_bulk"]))
            assert bool(rd["bulk_truncated"][p]) == bool(bt["bulk_truncated"]), (who, p)
            assert lo <= R.LD(rd["ess_tail"][p]) <= hi, (who, p, rd["ess_tail"][p], float(lo), float(hi))


def test_statistics_of_a_derived_run_are_those_of_the_reference_tensor(mhx, oracle, real):
    N, nch = 64, 257
    x = _tensor(real, N, 5, nch, 77, edges=False)
    run = plant(mhx, x)
    der = run.derive(MAP_LAST)
    ref = _host(oracle, MAP_LAST.source, x, 3)
    twin = plant(mhx, ref)                                                    # a run whose tensor IS the reference tensor
    try:
        assert _same_bits(der.samples()[0], ref)
        S = N * nch
        # the quantiles' CPU reference: numpy's sort of the reference tensor and the project's own host half of the quantile (ranks
        # and interpolation: mhx.api.quantile_ranks / quantiles_from_order_statistics, pinned against numpy.quantile in
        # tests/test_quantiles_cpu.py); tests/compact_ref.py holds nothing for quantiles
        rows = np.sort(np.moveaxis(ref, 1, 0).reshape(4, -1).astype(np.float64), axis=1)
        probs = np.array(mhx.api.DEFAULT_QUANTILE_PROBS)
        j, j1, g = mhx.api.quantile_ranks(S, probs)
        want_q = mhx.api.quantiles_from_order_statistics(rows[:, j], rows[:, j1], g, top=rows[:, S - 1])
        assert np.array_equal(der.quantiles(), want_q)
        lo, hi = der.hpd(0.05)
        wlo, whi = hpd_ref.hpd_rows(ref, 0.05)
        assert np.array_equal(lo, wlo) and np.array_equal(hi, whi)
        counts, edges, outside = der.histogram(bins=16, params=[0, 2, 3])
        for k, p in enumerate([0, 2, 3]):
            wc, we = np.histogram(ref[:, p, :].astype(np.float64).ravel(), bins=16)
            assert np.array_equal(counts[k], wc) and np.array_equal(edges[k], we) and outside[k].sum() == 0
        a, b = der.diagnostics(), twin.diagnostics()
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
        # rank_diagnostics, bit for bit where the order of the additions is fixed: whole chains (ONE launch per sum, and the two chain
        # blocks of C = 257 add their partial sums to 0 in either order with the same bits) and ess_chains = 64 (the autocovariance
        # sums of the ESS are one block of 64 chains: one atomic per word).  With the defaults neither holds -- split chains launch
        # once per half (four partial sums per word) and ess_chains = 256 is four blocks of the autocovariance kernel, split or not
        # -- so two calls on the SAME run may differ in the last bits in fp64 (tests/test_gpu_rank_rhat.py and
        # tests/test_gpu_diagnostics.py say so of their own comparisons); the default call follows below, at those tests' bound.
        a, b = der.rank_diagnostics(split=False, ess_chains=64), twin.rank_diagnostics(split=False, ess_chains=64)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
        assert np.isfinite(a["rhat"]).all() and np.isfinite(a["ess_bulk"][[0, 2, 3]]).all()
        _default_rank_diagnostics_within_the_reference_bound(der, twin, ref, real, N)
        assert np.array_equal(der.cov(), twin.cov())
    finally:
        twin.close()
        der.close()
        run.close()


def _readme_chain(mhx, N=40, nch=64):
    data = np.random.default_rng(1234).normal(0.0, 1.0, size=30)
    model = mhx.DensityModel(mhx.IIDNormal(data))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(2), 0.25 * mhx.I))
    return mhx.sample(model, spl, N, nch, param_names=["mu", "sigma"], chain_type=mhx.Chains, discard_initial=20,
                      initial_params=np.array([0.0, 1.0]), seed=1234)


def test_chains_derive_on_the_readme_model(mhx, oracle, real):
    chain = _readme_chain(mhx)
    dch = chain.derive(MAP_SIGMA2, names=["sigma2"])
    two = chain.state.derive(lambda t: [t.sigma ** 2, t.mu], names=["mu", "sigma"])
    try:
        assert dch.names == ["sigma2", "lp"] and dch.params() == ["sigma2"] and (dch.start, dch.thin) == (chain.start, chain.thin)
        assert isinstance(dch.state, mhx.DerivedRun) and dch.value.shape == (40, 2, 64) and dch.value.dtype == chain.value.dtype
        assert _same_bits(dch.value, dch.state.samples()[0])
        mu, sig, lp = chain["mu"], chain["sigma"], chain["lp"]
        assert _same_bits(dch["sigma2"], sig * sig) and _same_bits(dch["lp"], lp)
        text = dch.describe()
        assert "sigma2" in text and "Quantiles" in text and "sigma2" in repr(dch)
        assert dch.hpd()["parameters"] == ["sigma2"] and dch.rhat(kind="rank")["rhat"].shape == (1,)
        assert dch.mean("sigma2") == float(np.mean(sig * sig, dtype=np.float64))
        assert (two.dim, two.n) == (2, 64) and _same_bits(two.samples()[0], np.stack([sig * sig, mu, lp], axis=1))
        # a derived run as a source: the README's source text again, on the derived run's own rows (its x[1] is mu), nothing compiled anew
        before = chain.state.ctx.jit_counts()
        again = two.derive(MAP_SIGMA2, names=["sigma2", "sigma"])
        try:
            assert chain.state.ctx.jit_counts() == before
            assert _same_bits(again.samples()[0], np.stack([mu * mu, lp], axis=1))
        finally:
            again.close()
        # a second identical derive compiles nothing and loads nothing
        twice = chain.state.derive(MAP_SIGMA2, names=["mu", "sigma"])
        try:
            assert chain.state.ctx.jit_counts() == before
            # a snapshot: sampling the source again does not change the derived tensor
            snap = twice.samples()[0].copy()
            chain.state.sample(40, 0, 1, 0)
            assert not _same_bits(chain.state.samples(False)[0][:, 1, :], sig)
            assert _same_bits(twice.samples()[0], snap) and _same_bits(dch.state.samples()[0], dch.value)
        finally:
            twice.close()
    finally:
        two.close()
        dch.state.close()
        chain.state.close()


def test_ctx_form_on_a_callers_tensor(mhx, oracle, real):
    x = _tensor(real, 7, 5, 65, 21)
    run = plant(mhx, x)
    try:
        ptr, n = C.c_void_p(), C.c_int64()
        mhx.check(mhx.lib().mhx_run_device_samples(run.h, C.byref(ptr), None, C.byref(n)))
        dat = run.ctx.arr(LOOP_DATA)
        h = C.c_void_p()
        mhx.check(mhx.lib().mhx_ctx_derive(run.ctx.h, ptr, 7, 6, 65, SRC_LOOP.encode(), 1, mhx._lib.rptr(dat), dat.size, C.byref(h)))
        der = mhx.DerivedRun(h, run, 1)
        try:
            assert _same_bits(der.samples()[0], _host(oracle, SRC_LOOP, x, 1, LOOP_DATA))
        finally:
            der.close()
    finally:
        run.close()


def test_refusals(mhx, oracle, real):
    x = _tensor(real, 7, 5, 63, 3, edges=False)
    run = plant(mhx, x)
    der = run.derive(MAP_LAST)
    try:
        state = run.save_state()
        calls = [lambda: der.sample(4), lambda: der.init(None), lambda: der.set_params(np.zeros((3, 63))), lambda: der.save_state(),
                 lambda: der.load_state(state), lambda: der.factor(), lambda: der.step_stats(), lambda: der.state()]
        for call in calls:
            with pytest.raises(mhx.MhxError, match="derived") as e:
                call()
            assert e.value.code == mhx.MHX_ESTATE
        with pytest.raises(mhx.ArgumentError, match="derived"):
            der.samples(want_accepted=True)
        # the arguments of the call itself
        h = C.c_void_p()
        lib, src = mhx.lib(), MAP_LAST.source.encode()
        assert lib.mhx_run_derive(run.h, src, 0, None, 0, C.byref(h)) == mhx.MHX_EINVAL and not h.value
        assert lib.mhx_run_derive(run.h, src, -3, None, 0, C.byref(h)) == mhx.MHX_EINVAL and not h.value
        assert lib.mhx_run_derive(run.h, None, 3, None, 0, C.byref(h)) == mhx.MHX_EINVAL and not h.value
        assert lib.mhx_run_derive(run.h, src, 3, None, 4, C.byref(h)) == mhx.MHX_EINVAL and not h.value
        with pytest.raises(mhx.ArgumentError, match="nout"):
            run.derive(MAP_LAST, nout=2)
        # a source that does not compile: MHX_EINVAL with the compiler's log; a good derive works afterwards
        with pytest.raises(mhx.ArgumentError, match="derived.hip") as e:
            run.derive(mhx.HipMap(SRC_BAD, 1))
        assert "error" in str(e.value) and "does not compile" in str(e.value)
        # a run in moments mode (the shape of tests/test_gpu_quantiles.py), and a run that saved nothing, hold no draws to map
        dm, Cm = 40, 96
        s = float(np.float32(2.38 / dm ** 0.5))
        mom = mhx.Run(mhx.DensityModel(mhx.Funnel(dm)), mhx.RWMH(mhx.MvNormal(mhx.zeros(dm), s * s * mhx.I)), nchains=Cm, seed=2)
        mom.init(np.random.default_rng(8).normal(size=(dm, Cm)))
        mom.sample(10, 5, 5, 0, save="moments")
        with pytest.raises(mhx.MhxError, match="no device sample tensor") as e:
            mom.derive(mhx.HipMap(SRC_LOOP, 1, data=LOOP_DATA))
        assert e.value.code == mhx.MHX_ESTATE
        mom.close()
        run.sample(5, 0, 1, 0, save=False)
        with pytest.raises(mhx.MhxError, match="no device sample tensor"):
            run.derive(MAP_LAST)
        # both runs remain usable: the derived run kept its snapshot, the source samples and derives again
        assert _same_bits(der.samples()[0], _host(oracle, MAP_LAST.source, x, 3))
        run.sample(7, 0, 1, 0)
        der2 = run.derive(MAP_LAST)
        assert _same_bits(der2.samples()[0], _host(oracle, MAP_LAST.source, run.samples(False)[0], 3))
        der2.close()
    finally:
        der.close()
        run.close()


def _refuse_list():
    """the entry points include/mhx.h lists under `refuse` at mhx_run_derive, written out: "mhx_run_init, _sample, ...; mhx_ram_..." """
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mhx.h")).read()
    text = re.search(r"refuse\s+with MHX_ESTATE[^:]*looked at:(.*?)\(and with them", hdr, flags=re.S).group(1)
    names = []
    for family in text.split(";"):
        for w in re.findall(r"(?:mhx)?_\w+", family):
            names.append(w if w.startswith("mhx_") else re.match(r"mhx_[a-z]+", names[-1]).group(0) + w)
    return names


def test_every_entry_on_the_headers_refuse_list_refuses_a_derived_run(mhx, real):
    """Raw ctypes, the derived run's handle and every other argument zero: the header promises the guard runs "before anything else is
    looked at", so NULL pointers and 0 sizes are within the contract.  MHX_ESTATE, "derived" and the entry's own name in the message."""
    names = _refuse_list()
    assert len(names) == len(set(names)) == 22
    assert [sum(n.startswith(p) for n in names) for p in ("mhx_run_", "mhx_ram_", "mhx_emcee_")] == [8, 8, 6]
    x = _tensor(real, 7, 3, 63, 5, edges=False)
    run = plant(mhx, x)
    der = run.derive(mhx.HipMap("MHX_DERIVED(x, y, d, data, ndata) { y.set(0, x[0] * x[0]); }\n", 1))
    try:
        lib = mhx.lib()
        for name in names:
            fn = getattr(lib, name)
            zeros = [None if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer) else 0 for t in fn.argtypes[1:]]
            assert fn(der.h, *zeros) == mhx.MHX_ESTATE, name
            msg = lib.mhx_last_error().decode()
            assert "derived" in msg and msg.startswith(name + ":"), (name, msg)
        # the source run is untouched by all that: it still samples
        run.sample(7, 0, 1, 0)
        assert run.samples(False)[0].shape == (7, 4, 63)
    finally:
        der.close()
        run.close()
