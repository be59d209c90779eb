"""GPU: the rank-normalised split R-hat of the device (mhx_run_rank_diagnostics, mhx_run_rank_scores; csrc/mhx_diag_kernels.h:
mhx_diag_fold_rank) against tests/rank_rhat_ref.py, on the crafted tensors of tests/diag_ref.py, on rows built where the fold can go
wrong and on rows that have no answer (include/mhx.h).

The scores are compared element by element -- which pins every rank, bulk and folded -- and the two R-hat values at MARGIN = 4 times
the reference's own bounds.  The tensors are planted in the sample buffer of a run of their shape, as tests/test_gpu_diagnostics.py
does.  Every comparison of an R-hat prints `DIAG_RATIO <width> rhat_bulk|rhat_tail <|error| / bound>`; the largest per width are
tabulated in DESIGN.md 6.5."""
import re

import numpy as np
import pytest

import diag_ref as R
import rank_rhat_ref as F
from planted import plant as _plant

pytestmark = pytest.mark.gpu
K = R.MARGIN
EXTRA_KEYS = [("extras",) + s for s in F.EXTRA_SHAPES]
SUBSET = np.array([R.R_NINF, 9, 2, 2, 0, R.R_NAN, R.R_CONST], dtype=np.int32)         # a subset, out of order, one row twice


def _id(key):
    return key if isinstance(key, str) else ("extras-N%d-C%d" % key[1:] if key[0] == "extras" else R.case_id(key))


def _near(got, want, bound, width, what, where):
    """|got - want| <= K bound (NaN and inf: the same on both sides); prints the ratio"""
    want_f = float(want)
    if not np.isfinite(want_f):
        assert (np.isnan(got) and np.isnan(want_f)) or got == want_f, "%s %s: got %r, reference %r" % (what, where, got, want_f)
        return
    assert np.isfinite(got), "%s %s: got %r, reference %r" % (what, where, got, want_f)
    err = abs(R.LD(got) - want)
    ratio = float(err / bound) if bound > 0 else (0.0 if err == 0 else np.inf)
    print("DIAG_RATIO %s %s %.3g   %s" % (width, what, ratio, where))
    assert ratio <= K, "%s %s: got %.17g, reference %.17g, error %.3g = %.3g x bound %.3g" % (
        what, where, got, want_f, float(err), ratio, float(bound))


_device_cache = {}


def _device(mhx, key, width):
    """everything the tests of one tensor read of the device, taken once per process: the two score arrays of every row, the full
    rank_diagnostics call and (crafted tensors) ess_bulk_tail and the subset call of the same run"""
    k = (key, width)
    if k not in _device_cache:
        x, split, _ = F.reference(key, width)
        lag = dict(max_lag=key[2], ess_chains=key[3]) if key in F.CASES else dict(max_lag=3, ess_chains=0)
        run = _plant(mhx, x)
        try:
            out = dict(rd=run.rank_diagnostics(split=split, **lag),
                       z={r: run.rank_scores(r) for r in range(x.shape[1])},
                       zf={r: run.rank_scores(r, folded=True) for r in range(x.shape[1])})
            if key in F.CASES:
                out.update(et=run.ess_bulk_tail(split=split, **lag), sub=run.rank_diagnostics(params=SUBSET, split=split, **lag),
                           rhat_only=run.rank_diagnostics(split=split, ess=False, **lag),
                           ess_only=run.rank_diagnostics(split=split, rhat=False, **lag))
            else:
                out["et"] = run.ess_bulk_tail(split=split, **lag)
        finally:
            run.close()
        _device_cache[k] = out
    return _device_cache[k]


def _score_pairs(key, width, dev):
    """(where, device scores, reference scores, reference ranks) of every row and fold that has ranks"""
    x, _, ref = F.reference(key, width)
    for r, rr in ref.items():
        for name, zk, rk in (("bulk", "z", "ranks"), ("folded", "zf", "ranks_f")):
            got = dev[zk][r]
            assert got.dtype == x.dtype and got.shape == (x.shape[0], x.shape[2])
            where = "%s row %d %s" % (_id(key), r, name)
            if rr["nan"] or rr[zk] is None:
                assert np.isnan(got).all(), where                  # a NaN in the row / a median that is not finite: no scores
                continue
            yield where, got, rr[zk], rr[rk].reshape(got.shape)


@pytest.mark.parametrize("key", F.CASES + EXTRA_KEYS + ["no_answer"], ids=_id)
def test_scores_carry_the_reference_ranks(mhx, real, key):
    """every score, mapped back through Phi, lands on the reference's tie-averaged rank -- bulk and folded, finite, +-inf and constant
    rows, signed zeros and draws equal to the median.  (rank - 3/8) / (S + 1/4) moves by 1 / (2 S + 1/2) per half rank; what a score
    that is SCORE_ULPS ulp off moves it by is at most phi(z) |z| SCORE_ULPS 2^-23 < 1.2e-7 in fp32: under a hundredth of that step (2e-5) at
    the largest S here, 24929.)"""
    from scipy.special import ndtr
    S = None
    for where, got, _, ranks in _score_pairs(key, real, _device(mhx, key, real)):
        S = got.size
        back = ndtr(got.astype(np.float64)) * (S + 0.25) + 0.375
        assert np.array_equal(np.round(2.0 * back) / 2.0, ranks), where
    assert S is not None


@pytest.mark.parametrize("key", F.CASES + EXTRA_KEYS + ["no_answer"], ids=_id)
def test_scores_match_the_reference(mhx, real, key):
    """rank_scores(p, folded) within SCORE_ULPS ulp (of the width, at the reference's value) of the reference's scores, element by
    element.  Measured on the MI355X: 0 ulp everywhere in fp32; in fp64 at most 1 ulp (S = 4, 15), 3 ulp (S = 315, 6208, 6305) and
    4 ulp (S = 24929).  This holds because the new entries evaluate the score where it is well conditioned (csrc/mhx_api_diag.inc:
    diag_normal_score); the evaluation of k_diag_rank_scores -- p = (rank - 3/8) / (S + 1/4) rounded in double, then inverted -- was
    measured at 24 ulp (S = 315), 1.5e3 ulp (S = 6208) and 4.7e3 ulp (S = 24929) at the score nearest zero, as scipy's ndtri of the
    same double p is on the CPU: the absolute rounding error of p comes back times 1 / phi(z)."""
    worst, lines = 0.0, []
    for where, got, want, _ in _score_pairs(key, real, _device(mhx, key, real)):
        err = np.abs(got.astype(R.LD) - want.astype(R.LD))
        ulps = err / np.spacing(np.abs(want)).astype(R.LD)
        i = np.unravel_index(int(np.argmax(ulps)), ulps.shape)
        lines.append("SCORE_ULPS %s %.3g   %s at %s: got %.17g, reference %.17g, largest absolute error of the row %.3g" % (
            real, float(ulps.max()), where, i, got[i], want[i], float(err.max())))
        print(lines[-1])
        worst = max(worst, float(ulps.max()))
    print("SCORE_ULPS_MAX %s %.3g   %s" % (real, worst, _id(key)))
    assert worst <= R.SCORE_ULPS, "\n".join(ln for ln in lines if float(ln.split()[2]) > R.SCORE_ULPS)


@pytest.mark.parametrize("key", F.CASES + EXTRA_KEYS, ids=_id)
def test_rhat_matches_the_reference(mhx, real, key):
    _, _, ref = F.reference(key, real)
    rd = _device(mhx, key, real)["rd"]
    assert np.array_equal(rd["params"], np.arange(len(ref)))
    for r, rr in ref.items():
        where = "%s row %d" % (_id(key), r)
        if rr["nan"]:
            assert np.isnan(rd["rhat_bulk"][r]) and np.isnan(rd["rhat_tail"][r]) and np.isnan(rd["rhat"][r]), where
            continue
        for part, k in (("bulk", "rhat_bulk"), ("tail", "rhat_tail")):
            _near(rd[k][r], rr[part]["rhat"], rr[part]["b_rhat"], real, k, where)
        both = np.array([rd["rhat_bulk"][r], rd["rhat_tail"][r]])
        if np.isnan(both).all():
            assert np.isnan(rd["rhat"][r]), where
        else:
            assert rd["rhat"][r] == np.nanmax(both), where                  # the larger of the two, NaN only if both are
    if key in F.CASES:
        # the crafted rows without an answer (include/mhx.h): W == 0 with and without a spread of the chain means, one chain
        one = key[1] * (2 if key[4] else 1) == 1
        for k in ("rhat_bulk", "rhat_tail"):
            assert np.isnan(rd[k][R.R_CONST]), k
            assert np.isnan(rd[k][R.R_CONST_PC]) if key[1] == 1 else np.isposinf(rd[k][R.R_CONST_PC]), k
            if one:
                assert np.isnan(rd[k]).all(), k


@pytest.mark.parametrize("key", F.CASES, ids=R.case_id)
def test_ess_of_the_same_call_is_that_of_ess_bulk_tail(mhx, real, key):
    """within MARGIN x bound, not bit for bit: the fp64 atomics may arrive in another order, and the bulk scores of the new entry differ
    from those of ess_bulk_tail in their last bits (include/mhx.h); so do the calls that ask for one half only"""
    _, _, bt = R.reference(key, real)
    dev = _device(mhx, key, real)
    rd, et = dev["rd"], dev["et"]
    for other in (rd, dev["ess_only"]):
        for r in range(len(R.ROWS)):
            for k in ("ess_bulk", "ess_tail"):
                a, f = other[k][r], et[k][r]
                assert (np.isnan(a) and np.isnan(f)) or abs(R.LD(a) - R.LD(f)) <= K * bt[r]["b_" + k], (k, r, a, f)
            assert other["bulk_truncated"][r] == et["bulk_truncated"][r], r
            if "lo" in bt[r] and bt[r]["lo"]["truncated"] == bt[r]["hi"]["truncated"]:
                assert other["tail_truncated"][r] == et["tail_truncated"][r], r
    assert "rhat" not in dev["ess_only"] and "ess_bulk" not in dev["rhat_only"]
    _, _, ref = F.reference(key, real)
    for r in F.RANKED:
        for part, k in (("bulk", "rhat_bulk"), ("tail", "rhat_tail")):
            _near(dev["rhat_only"][k][r], ref[r][part]["rhat"], ref[r][part]["b_rhat"], real, k, "%s row %d (R-hat only)" % (R.case_id(key), r))


@pytest.mark.parametrize("key", F.CASES, ids=R.case_id)
def test_a_subset_a_repeated_row_and_another_order_give_the_numbers_of_the_full_call(mhx, real, key):
    _, _, ref = F.reference(key, real)
    _, _, bt = R.reference(key, real)
    dev = _device(mhx, key, real)
    sub, rd = dev["sub"], dev["rd"]
    assert np.array_equal(sub["params"], SUBSET)
    for i, r in enumerate(SUBSET):
        where = "%s subset slot %d row %d" % (R.case_id(key), i, r)
        for k in ("ess_bulk", "ess_tail"):
            a, f = sub[k][i], rd[k][r]
            assert (np.isnan(a) and np.isnan(f)) or abs(R.LD(a) - R.LD(f)) <= K * bt[r]["b_" + k], (where, k, a, f)
        if ref[r]["nan"]:
            assert np.isnan(sub["rhat_bulk"][i]) and np.isnan(sub["rhat_tail"][i]), where
            continue
        for part, k in (("bulk", "rhat_bulk"), ("tail", "rhat_tail")):
            _near(sub[k][i], ref[r][part]["rhat"], ref[r][part]["b_rhat"], real, k, where)


def test_rows_without_an_answer(mhx, real):
    """include/mhx.h, one row each: a NaN -> NaN everywhere; a median that is not finite (half of the draws +inf; -inf and +inf as the
    middle pair) -> rhat_tail = NaN and the other three as the reference and ess_bulk_tail give them; infinite draws around a finite
    median are ranked like any other; W == 0 -> NaN (Vm == 0) or +inf (Vm > 0)"""
    _, _, ref = F.reference("no_answer", real)
    dev = _device(mhx, "no_answer", real)
    rd, et = dev["rd"], dev["et"]
    for k in ("ess_bulk", "ess_tail", "rhat_bulk", "rhat_tail", "rhat"):
        assert np.isnan(rd[k][F.NO_NAN]), k
    assert np.isnan(dev["z"][F.NO_NAN]).all() and np.isnan(dev["zf"][F.NO_NAN]).all()
    for r in (F.NO_HALF_INF, F.NO_INF_PAIR):
        where = "no_answer row %d" % r
        assert np.isnan(rd["rhat_tail"][r]) and np.isnan(dev["zf"][r]).all() and not np.isnan(dev["z"][r]).any(), where
        _near(rd["rhat_bulk"][r], ref[r]["bulk"]["rhat"], ref[r]["bulk"]["b_rhat"], real, "rhat_bulk", where)
        assert rd["rhat"][r] == rd["rhat_bulk"][r]
        bt = R.bulk_tail(F.no_answer(real)[:, r, :], real, 3, 0, True)
        for k in ("ess_bulk", "ess_tail"):
            a, f = rd[k][r], et[k][r]
            assert (np.isnan(a) and np.isnan(f)) or abs(R.LD(a) - R.LD(f)) <= K * bt["b_" + k], (where, k, a, f)
    where = "no_answer row %d" % F.NO_FEW_INF
    for part, k in (("bulk", "rhat_bulk"), ("tail", "rhat_tail")):
        assert np.isfinite(rd[k][F.NO_FEW_INF])
        _near(rd[k][F.NO_FEW_INF], ref[F.NO_FEW_INF][part]["rhat"], ref[F.NO_FEW_INF][part]["b_rhat"], real, k, where)
    for k in ("rhat_bulk", "rhat_tail", "rhat"):
        assert np.isnan(rd[k][F.NO_CONST]) and np.isposinf(rd[k][F.NO_CONST_PC]), k


def _real_chain(mhx):
    """examples/readme_model.py cut to 16 chains x 100 draws"""
    data = np.random.default_rng(1234).normal(0.0, 1.0, size=30)
    model = mhx.DensityModel(mhx.IIDNormal(data))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(2), mhx.I))
    return mhx.sample(model, spl, 100, 16, param_names=["mu", "sigma"], chain_type=mhx.Chains, discard_initial=50,
                      initial_params=np.array([0.0, 1.0]), seed=1234)


def test_chains_rhat_and_describe_on_a_real_run(mhx, real):
    chain = _real_chain(mhx)
    x = np.ascontiguousarray(chain.value)
    assert x.shape == (100, 3, 16) and chain.params() == ["mu", "sigma"]
    rd = chain.state.rank_diagnostics(params=[0, 1], split=True)
    ref = [F.rank_rhat(np.ascontiguousarray(x[:, p, :]), real, True) for p in (0, 1)]
    kinds = {"rank": "rhat", "bulk": "rhat_bulk", "tail": "rhat_tail"}
    for kind, col in kinds.items():
        got = chain.rhat(kind=kind)
        assert got["parameters"] == ["mu", "sigma"] and got["kind"] == kind
        for p in (0, 1):
            parts = [q for q in ("bulk", "tail") if kind in ("rank", q)]
            want = max(ref[p][q]["rhat"] for q in parts)
            bound = max(ref[p][q]["b_rhat"] for q in parts)
            for v in (got["rhat"][p], rd[col][p]):
                _near(v, want, bound, real, col, "real run %s %s" % (kind, got["parameters"][p]))
    basic = chain.rhat(kind="basic")
    dg = chain.state.diagnostics(max_lag=0, split=True)
    st = R.series_stats
    for p in (0, 1):
        s = st(x[:, p, :], real, 0, 0, True)
        _near(basic["rhat"][p], s["rhat"], s["b_rhat"], real, "rhat", "real run basic %d" % p)
        _near(dg["rhat"][p], s["rhat"], s["b_rhat"], real, "rhat", "real run diagnostics %d" % p)
    with pytest.raises(mhx.ArgumentError):
        chain.rhat(kind="split")
    # the rhat column of describe(rhat_kind="rank") is rank_diagnostics' rhat, printed to four places
    text = chain.describe(rhat_kind="rank")
    rows = [ln.split() for ln in text.split("Quantiles")[0].splitlines() if re.match(r"\s+(mu|sigma)\s", ln)]
    assert [rw[0] for rw in rows] == ["mu", "sigma"]
    for p, rw in enumerate(rows):
        want = max(ref[p]["bulk"]["rhat"], ref[p]["tail"]["rhat"])
        bound = max(ref[p]["bulk"]["b_rhat"], ref[p]["tail"]["b_rhat"])
        assert abs(R.LD(float(rw[-1])) - want) <= 0.5e-4 + K * bound, (rw, float(want))
    st_rank = chain.summarystats(rhat_kind="rank")
    for p in (0, 1):
        want = max(ref[p]["bulk"]["rhat"], ref[p]["tail"]["rhat"])
        _near(st_rank["rhat"][p], want, max(ref[p]["bulk"]["b_rhat"], ref[p]["tail"]["b_rhat"]), real, "rhat", "real run summarystats %d" % p)


def test_describe_by_default_is_the_basic_kind(mhx, real):
    chain = _real_chain(mhx)
    assert chain.describe() == chain.describe(rhat_kind="basic")
    assert repr(chain) == chain.__repr__(rhat_kind="basic")
    assert chain.summarystats().keys() == chain.summarystats(rhat_kind="basic").keys()
    with pytest.raises(mhx.ArgumentError):
        chain.describe(rhat_kind="folded")
