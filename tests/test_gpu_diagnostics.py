"""GPU: R-hat sums, Geyer ESS, bulk and tail ESS of the device (csrc/mhx_diag_kernels.h, csrc/mhx_api_diag.inc) against the
extended-precision reference tests/diag_ref.py on crafted tensors, at MARGIN = 4 times the reference's own error bounds, and the
answers of rows that have none (include/mhx.h: constant rows, NaN of either sign, +-inf).

The crafted [N][16][C] tensor is planted in the sample buffer of a run of that shape (mhx_run_device_samples hands out the device
pointer); tests/test_diagnostics_cpu.py asserts, on the reference alone, that every planted input keeps the truncation index of
the Geyer sum MARGIN bounds away from a step.  Bad rows sit in the same tensor as the finite ones, so every comparison of a
finite row is also the statement that no bad row changes another row's numbers.

Every comparison prints `DIAG_RATIO <width> <quantity> <|error| / bound>`; the largest per width are tabulated in DESIGN.md 6.5."""
import numpy as np
import pytest

import diag_ref as R
from planted import plant as _plant

pytestmark = pytest.mark.gpu
K = R.MARGIN


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


def _check_plain(dg, st, rows, width, where, check_ess=True):
    for r in rows:
        s = st[r]
        w = "%s row %d (%s)" % (where, r, R.ROWS[r] if len(st) > 2 else "ar1")
        for k in ("sum_m", "sum_m2", "sum_v"):
            _near(dg[k][r], s[k], s["b_" + k], width, k, w)
        if "rhat" in dg:
            _near(dg["rhat"][r], s["rhat"], s["b_rhat"], width, "rhat", w)
        if check_ess:
            _near(dg["ess_geyer"][r], s["ess"], s["b_ess"], width, "ess_geyer", w)
            assert bool(dg["ess_geyer_truncated"][r]) == bool(s["truncated"]), w


def _check_bulk_tail(et, idx, bt, width, where):
    for i, r in enumerate(idx):
        b = bt[r]
        w = "%s row %d (%s)" % (where, r, R.ROWS[r])
        _near(et["ess_bulk"][i], b["ess_bulk"], b["b_ess_bulk"], width, "ess_bulk", w)
        assert bool(et["bulk_truncated"][i]) == bool(b["bulk_truncated"]), w
        if not np.isfinite(float(b["ess_tail"])):
            assert np.isnan(et["ess_tail"][i]), w
            continue
        lo, hi = R.tail_interval(b, K)
        got = R.LD(et["ess_tail"][i])
        side = b["lo"] if b["lo"]["ess"] < b["hi"]["ess"] else b["hi"]
        print("DIAG_RATIO %s ess_tail %.3g   %s" % (width, float(abs(got - side["ess"]) / side["b_ess"]), w))
        assert lo <= got <= hi, "ess_tail %s: got %.17g outside [%.17g, %.17g]" % (w, float(got), float(lo), float(hi))
        if b["lo"]["truncated"] == b["hi"]["truncated"]:
            assert bool(et["tail_truncated"][i]) == bool(side["truncated"]), w


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_crafted_tensor_matches_the_reference(mhx, real, case):
    N, nch, max_lag, ess_chains, split, _ = case
    x, st, bt = R.reference(case, real)
    where = R.case_id(case)
    run = _plant(mhx, x)
    try:
        dg = run.diagnostics(max_lag=max_lag, ess_chains=ess_chains, split=split)
        again = run.diagnostics(max_lag=max_lag, ess_chains=ess_chains, split=split)
        et = run.ess_bulk_tail(max_lag=max_lag, ess_chains=ess_chains, split=split)
        some = np.array([R.R_NINF, 9, 2, 2, 0, R.R_NAN, R.R_CONST], dtype=np.int32)      # a subset, out of order, one row twice
        sub = run.ess_bulk_tail(params=some, max_lag=max_lag, ess_chains=ess_chains, split=split)
    finally:
        run.close()
    parts = 2 if split else 1
    assert dg["n_chains"] == nch * parts and dg["n_samples"] == N // parts
    # ---- finite rows
    _check_plain(dg, st, R.FINITE, real, where)
    _check_bulk_tail(et, list(range(len(R.ROWS))), bt, real, where)
    # the fp64 atomics may arrive in another order: a second call agrees within the bound, not bit for bit
    for r in R.FINITE:
        for k in ("sum_m", "sum_m2", "sum_v"):
            assert abs(R.LD(dg[k][r]) - R.LD(again[k][r])) <= K * st[r]["b_" + k], (k, r)
        if np.isfinite(float(st[r]["ess"])):
            assert abs(R.LD(dg["ess_geyer"][r]) - R.LD(again["ess_geyer"][r])) <= K * st[r]["b_ess"], r
    # a subset of the rows, a repeated row, another order: the numbers of the full call
    _check_bulk_tail(sub, list(some), bt, real, where + " subset")
    for i, r in enumerate(some):
        for k, b in (("ess_bulk", "b_ess_bulk"), ("ess_tail", "b_ess_tail")):
            a, f = sub[k][i], et[k][r]
            assert (np.isnan(a) and np.isnan(f)) or abs(R.LD(a) - R.LD(f)) <= K * bt[r][b], (k, r, a, f)
    assert sub["ess_bulk"][2] == sub["ess_bulk"][3] or abs(sub["ess_bulk"][2] - sub["ess_bulk"][3]) <= K * float(bt[2]["b_ess_bulk"])
    # ---- rows without an answer (include/mhx.h)
    for r in (R.R_CONST, R.R_CONST_PC):
        assert np.isnan(dg["ess_geyer"][r]) and not dg["ess_geyer_truncated"][r], (r, dg["ess_geyer"][r])
        assert np.isnan(et["ess_tail"][r]) and np.isnan(et["ess_bulk"][r]), (r, et["ess_bulk"][r], et["ess_tail"][r])
        assert dg["sum_v"][r] == 0.0
        _near(dg["sum_m"][r], st[r]["sum_m"], st[r]["b_sum_m"], real, "sum_m", "%s row %d" % (where, r))
    if "rhat" in dg:
        assert np.isnan(dg["rhat"][R.R_CONST])
        assert np.isposinf(dg["rhat"][R.R_CONST_PC])
    for r in (R.R_NAN, R.R_NEG_NAN, R.R_PINF, R.R_NINF):
        for k in ("sum_m", "sum_m2", "sum_v", "ess_geyer"):
            assert np.isnan(dg[k][r]), (k, r, dg[k][r])
        if "rhat" in dg:
            assert np.isnan(dg["rhat"][r])
    for r in (R.R_NAN, R.R_NEG_NAN):
        assert np.isnan(et["ess_bulk"][r]) and np.isnan(et["ess_tail"][r]), (r, et["ess_bulk"][r], et["ess_tail"][r])
    if N >= 97:                                            # ranks are defined: the reference gives the (finite) value, checked above
        for r in (R.R_PINF, R.R_NINF):
            assert np.isfinite(et["ess_bulk"][r]) and np.isfinite(et["ess_tail"][r]), (r, et["ess_bulk"][r], et["ess_tail"][r])


def test_more_lags_than_one_launch_holds(mhx, real):
    """dim = 1, one chain of 131073 draws, max_lag = 65600: 65600 lags, more than the 65535 blocks grid.z takes.  The lags are
    launched in slices; the answer is the reference's (which stops at the truncating pair: nothing behind it enters tau)."""
    N, nch, max_lag, ess_chains, split, _ = R.LONG_CASE
    x, st, _ = R.reference(R.LONG_CASE, real, bulk=False)
    assert R.nlag_rule(max_lag, N) == 65600
    run = _plant(mhx, x)
    try:
        dg = run.diagnostics(max_lag=max_lag, ess_chains=ess_chains, split=split)
    finally:
        run.close()
    _check_plain(dg, st, [0, 1], real, R.case_id(R.LONG_CASE))
