"""GPU: different post-run statistics back to back on ONE context.  The select, the histograms and the autocovariance carve the same
scratch block of the context, HPD holds its own block across the select passes inside it, and the cross moments have a third
(csrc/mhx_api.hip: scratch_carve): a block that one call resized or left full of its own data must not
disturb the next.  Every result of the sequence is compared, bit for bit, with the same call made first thing on a fresh run.

The tensor is acf_ref.tensor(97, 64, .): one block of chains and one time chunk for the autocovariance, so a single atomic per sum
and reproducible bits (as in tests/test_gpu_acf.py: test_ctx_form_on_the_same_pointer); S = 6208 draws per row give the select and
the histograms more than one block per row in both widths."""
import numpy as np
import pytest

import acf_ref as A
import diag_ref as R
from planted import plant

pytestmark = pytest.mark.gpu
N, NCH, SEED = 97, 64, 1
S = N * NCH
FINITE4 = [9, 0, 5, 2]                                      # rows whose minimum and maximum can be edges
WITH_NAN = FINITE4 + [R.R_NAN]
RANKS = [0, S // 2, S - 1]


def _edges(x, rows, bins):
    return np.stack([np.linspace(x[:, r, :].astype(np.float64).min(), x[:, r, :].astype(np.float64).max(), bins + 1) for r in rows])


def _calls(x):
    """(name, call on a run, result arrays that may hold a NaN) in the order of the sequence: the select block's need goes
    small, large, small, (HPD: small again, from inside), -, middling, small"""
    e1, e2 = _edges(x, FINITE4, 2048), _edges(x, FINITE4, 128)
    return [
        ("order statistics", lambda run: [run.order_statistics(RANKS)]),
        ("histogram", lambda run: [a for a in run.histogram(params=FINITE4, edges=e1)]),
        ("autocovariance", lambda run: [a for a in run.autocovariance(np.arange(N), params=WITH_NAN)]),
        ("hpd", lambda run: [a for a in run.hpd(0.05, params=FINITE4)]),
        ("cross moments", lambda run: [np.asarray(a) for a in run.cross_moments(params=FINITE4, shift=np.zeros(len(FINITE4)))]),
        ("pair histogram", lambda run: [a for a in run.histogram2d(params=FINITE4, bins=128, edges=e2)]),
        ("order statistics again", lambda run: [run.order_statistics(RANKS)]),
    ]


def test_a_block_resized_by_one_statistic_does_not_disturb_the_next(mhx, real):
    x = np.ascontiguousarray(A.tensor(N, NCH, real, SEED))
    assert x.shape == (N, len(R.ROWS), NCH) and np.isfinite(x[:, FINITE4, :]).all() and np.isnan(x[:, R.R_NAN, :]).any()
    calls = _calls(x)
    fresh = []
    for name, call in calls[:-1]:                           # (the last call is the first one again)
        run = plant(mhx, x)
        try:
            fresh.append(call(run))
        finally:
            run.close()
    fresh.append(fresh[0])
    run = plant(mhx, x)
    try:
        got = [call(run) for _, call in calls]
    finally:
        run.close()
    for (name, _), g, w in zip(calls, got, fresh):
        assert len(g) == len(w), name
        for k, (a, b) in enumerate(zip(g, w)):
            a, b = np.asarray(a), np.asarray(b)
            assert a.dtype == b.dtype and a.shape == b.shape, (name, k)
            nan_ok = a.dtype.kind == "f"
            assert np.array_equal(a, b, equal_nan=True) if nan_ok else np.array_equal(a, b), "%s: result %d differs from a fresh run's" % (name, k)
    # the sequence did compute something: NaNs order last in the NaN row and make its autocovariance NaN, and no other row has one
    assert np.isnan(got[0][0][R.R_NAN][-1]) and not np.isnan(got[0][0][FINITE4]).any()
    assert np.isnan(got[2][0][-1]).all() and got[2][1][-1] == 0 and not np.isnan(got[2][0][:-1]).any()
    assert got[1][0].sum() + got[1][2].sum() == len(FINITE4) * S
