"""The reference of the rank-normalised split R-hat (tests/rank_rhat_ref.py) on its own: the device's route to the folded ranks --
searches in the two monotone halves of the one sorted array, no second sort -- gives the ranks of the definition on every input
tests/test_gpu_rank_rhat.py plants; every finite row has scores with within-chain variance; and a known answer."""
import numpy as np
import pytest

import diag_ref as R
import rank_rhat_ref as F

WIDTHS = ["f32", "f64"]
KEYS = F.CASES + [("extras",) + s for s in F.EXTRA_SHAPES] + ["no_answer"]


def _id(key):
    return key if isinstance(key, str) else ("extras-N%d-C%d" % key[1:] if key[0] == "extras" else R.case_id(key))


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("key", KEYS, ids=_id)
def test_fold_by_search_gives_the_ranks_of_the_folded_draws(key, width):
    """less / leq counted by searchsorted on each side of the split point == average_ranks(|x - m|), rank for rank, also where the
    rounded subtraction collapses distinct draws onto one fold value (exp8 in fp32) and where -0.0, +0.0 and the median tie"""
    x, _, ref = F.reference(key, width)
    n = 0
    for r, rr in ref.items():
        if rr["nan"] or rr["ranks_f"] is None:
            continue
        flat = x[:, r, :].reshape(-1)
        assert np.array_equal(F.fold_ranks_by_search(flat), rr["ranks_f"]), (key, r)
        n += 1
    assert n >= 3


def test_the_fold_collapses_distinct_draws_in_fp32():
    """what makes exp8 a test of the tie handling: distinct draws, fewer distinct fold values"""
    x = F.extras(97, 65, "f32")[:, F.EXTRA_ROWS.index("exp8"), :].reshape(-1)
    g = F.fold(x)
    assert len(np.unique(g)) < len(np.unique(x))


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("key", F.CASES + [("extras",) + s for s in F.EXTRA_SHAPES], ids=_id)
def test_every_finite_row_has_within_chain_variance(key, width):
    """R-hat = sqrt(var+ / W) is continuous in the three sums wherever W > 0: no margin of the kind the Geyer truncation needs"""
    x, split, ref = F.reference(key, width)
    rows = R.FINITE if key in F.CASES else range(len(F.EXTRA_ROWS))
    for r in rows:
        for part in ("bulk", "tail"):
            s = ref[r][part]
            assert s["W"] > 0, (key, r, part)
            if s["M"] > 1:
                assert np.isfinite(float(s["rhat"])) and s["b_rhat"] < 1e-3 * s["rhat"], (key, r, part, s["rhat"], s["b_rhat"])
            else:
                assert np.isnan(float(s["rhat"]))


def test_rows_without_an_answer():
    x, split, ref = F.reference("no_answer", "f64")
    assert ref[F.NO_NAN]["nan"]
    for r in (F.NO_HALF_INF, F.NO_INF_PAIR):
        assert ref[r]["tail"] is None and np.isfinite(float(ref[r]["bulk"]["rhat"]))
    assert np.isposinf(F.median(x[:, F.NO_HALF_INF, :].reshape(-1))) and np.isnan(F.median(x[:, F.NO_INF_PAIR, :].reshape(-1)))
    few = ref[F.NO_FEW_INF]
    assert np.isfinite(float(few["bulk"]["rhat"])) and np.isfinite(float(few["tail"]["rhat"]))
    assert few["ranks_f"].max() == 31.5 and (few["ranks_f"] == 31.5).sum() == 2          # the two infinite draws fold onto +inf
    for part in ("bulk", "tail"):
        assert np.isnan(float(ref[F.NO_CONST][part]["rhat"])) and (ref[F.NO_CONST]["z" if part == "bulk" else "zf"] == 0).all()
        assert np.isposinf(float(ref[F.NO_CONST_PC][part]["rhat"]))


def test_chains_that_differ_in_scale_only_show_in_the_folded_rhat():
    """8 chains of 1000 normal draws about 0, every other one three times as wide (seed 5), split: the classic split R-hat of the
    draws is 0.9995 and that of the bulk scores 0.9996 -- both blind to it -- while the folded scores give 1.1564."""
    rng = np.random.default_rng(5)
    x = rng.normal(size=(1000, 8)) * np.where(np.arange(8) % 2 == 0, 1.0, 3.0)[None, :]
    basic = float(R.series_stats(x, "f64", 0, 0, True)["rhat"])
    rr = F.rank_rhat(x, "f64", True)
    bulk, tail = float(rr["bulk"]["rhat"]), float(rr["tail"]["rhat"])
    print("basic %.4f bulk %.4f tail %.4f" % (basic, bulk, tail))
    assert abs(basic - 1) < 0.01 and abs(bulk - 1) < 0.01
    assert tail > 1.1 and tail > bulk + 0.1
