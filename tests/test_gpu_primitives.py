"""GPU: every elementary function of the arithmetic spec (mhx_device_math.h), probed on the device at its edges, bit for bit.

The probe is a user log-density (tests/primitive_probes.py: PROBE) evaluated by mhx.logdensity: one compile per width returns any
device function of the header at any argument.  References: the oracle's exports for log / exp / sincos2pi / u01; the device's own
mhx_log AND the oracle for mhx_log_sel; np.sqrt and a / b -- IEEE, correctly rounded, which is what the shortened sequences
mhx_sqrt_normal and mhx_div_normal claim -- for those two; compositions of the above, rounded step by step in the width, for
mhx_normal_pair and the Cauchy quotient.  Every comparison is on bit patterns and the sign of zero counts; two NaNs compare equal
whatever their payload or sign.  The inputs are described, and checked without a GPU, in tests/primitive_probes.py and
tests/test_primitives_cpu.py."""
import numpy as np
import pytest

import cases
import primitive_probes as P

pytestmark = pytest.mark.gpu

_models = {}
_refs = {}


def probe(mhx, fn, x, ctx=None):
    """device function `fn` of the probe at the columns of x [d][n]"""
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=cases.R())
    key = (mhx.get_default_dtype(), fn, x.shape[0], ctx)
    if key not in _models:
        _models[key] = mhx.DensityModel(mhx.HipLogDensity(P.PROBE, x.shape[0], data=[float(fn)]))
    return mhx.logdensity(_models[key], x, ctx=ctx)


def probe_words(mhx, fn, words, second=False):
    return probe(mhx, fn, P.words_to_x(words, 1.0 if second else 0.0))


def ref(key, make):
    """a reference computed once and shared by the tests that need it"""
    if key not in _refs:
        _refs[key] = make()
        if isinstance(_refs[key], np.ndarray):
            _refs[key].setflags(write=False)
    return _refs[key]


def same(got, want, what, x=None):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == cases.R(), (what, got.shape, want.shape, got.dtype, want.dtype)
    both_nan = np.isnan(got) & np.isnan(want)
    bad = np.flatnonzero((cases.bits(got) != cases.bits(want)) & ~both_nan)
    if len(bad):
        i = bad[0]
        at = "" if x is None else " at x = %s" % (np.asarray(x)[..., i].tolist(),)
        raise AssertionError("%s: %d of %d results differ (%d NaN pairs taken as equal); first, index %d%s: device %r (%#x), reference %r (%#x)" % (
            what, len(bad), got.size, int(both_nan.sum()), i, at, got[i], int(cases.bits(got)[i]), want[i], int(cases.bits(want)[i])))
    return int(both_nan.sum())


# ---- log -------------------------------------------------------------------------------------------------------------------------
def _log_ref(dt):
    return ref(("log", dt), lambda: P.orc_map("orc_log", P.log_inputs(dt), dt))


def test_log_matches_the_oracle(mhx, oracle, real):
    x = P.log_inputs(real)
    nn = same(probe(mhx, P.F_LOG, x), _log_ref(real), "mhx_log", x)
    assert nn == 5                                                       # -inf, -tiny, -1 and the two NaNs


def test_log_sel_is_log_for_every_input(mhx, oracle, real):
    x = P.log_inputs(real)
    sel = probe(mhx, P.F_LOG_SEL, x)
    same(sel, probe(mhx, P.F_LOG, x), "mhx_log_sel against the device's mhx_log", x)
    same(sel, _log_ref(real), "mhx_log_sel against the oracle", x)


def test_log_pos_matches_the_oracle_on_positive_normals(mhx, oracle, real):
    x = P.log_inputs(real)
    W = P.Width(real)
    keep = (W.to_bits(x) >= W.tiny) & (W.to_bits(x) < W.inf)
    assert same(probe(mhx, P.F_LOG_POS, x[keep]), _log_ref(real)[keep], "mhx_log_pos", x[keep]) == 0


# ---- exp -------------------------------------------------------------------------------------------------------------------------
def test_exp_matches_the_oracle(mhx, oracle, real):
    x = P.exp_inputs(real)
    want = ref(("exp", real), lambda: P.orc_map("orc_exp", x, real))
    assert same(probe(mhx, P.F_EXP, x), want, "mhx_exp", x) == 2


def test_log_and_exp_edges_under_the_product_compiler(mhx, oracle, product_jit, tmp_path, monkeypatch):
    """the same probe through the product's default compiler for run-time kernels (the suite's default tier compiles with hiprtc):
    fp64, the edge lists of log and exp"""
    monkeypatch.setenv("MHX_CACHE_DIR", str(tmp_path / "jit"))
    mhx.set_default_dtype("f64")
    oracle.set_dtype("f64")
    ctx = mhx.Context(0, "f64")
    x = P.log_inputs("f64", 0)
    same(probe(mhx, P.F_LOG, x, ctx), P.orc_map("orc_log", x, "f64"), "mhx_log", x)
    same(probe(mhx, P.F_LOG_SEL, x, ctx), P.orc_map("orc_log", x, "f64"), "mhx_log_sel", x)
    x = P.exp_inputs("f64", 0)
    same(probe(mhx, P.F_EXP, x, ctx), P.orc_map("orc_exp", x, "f64"), "mhx_exp", x)
    cid, ext = ctx.jit_compiler()
    comp, _ = ctx.jit_counts()
    assert comp >= 1 and (ext == comp if cid else ext == 0), (cid, comp, ext)
    for k in [k for k in _models if k[3] is ctx]:
        del _models[k]


# ---- sqrt ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binade", [0, 1])
def test_sqrt_normal_fp32_is_correctly_rounded_on_every_mantissa(mhx, oracle, binade):
    """all 2^23 floats of [1, 2) and of [2, 4): both exponent parities, every mantissa.  (Measured over these 2^24 arguments: the
    hardware estimate is the rounded root 14241764 times, one ulp below it 2534470 times and one ulp above it 982 times; the upper
    residual x - s+ s is exactly zero twice, at 1 + 2^-23 and 4 - 2^-22, so `0.0f < rp` must stay strict; the lower residual
    x - s- s is never zero, so on this hardware `0.0f >= rm` and `0.0f > rm` select the same root for every normal argument
    whose residuals do not underflow.)"""
    mhx.set_default_dtype("f32")
    x = P.sqrt_f32_binade(binade)
    assert same(probe(mhx, P.F_SQRT_NORMAL, x), np.sqrt(x), "mhx_sqrt_normal", x) == 0


def test_sqrt_normal_is_correctly_rounded(mhx, oracle, real):
    """near-midpoint arguments of both exponent parities across the domain the header claims, the ends of the Box-Muller domain,
    the neighbours of 1 in four binades, +-0 (fp32, whose sequence claims them), and in fp64 2^22 random arguments.  The fp32
    sequence is also evaluated below its domain, at the smallest normal numbers, where its residuals underflow (sqrt(FLT_MIN)
    comes out one ulp low): counted, not asserted -- nothing sends them."""
    xm, wm = P.sqrt_midpoint_arrays(real, P.SQRT_MIDPOINT_SCALES[real])
    assert same(probe(mhx, P.F_SQRT_NORMAL, xm), wm, "mhx_sqrt_normal near midpoints", xm) == 0
    xe = P.sqrt_extras(real)
    same(probe(mhx, P.F_SQRT_NORMAL, xe), np.sqrt(xe), "mhx_sqrt_normal at the edges", xe)
    if real == "f32":
        xn = P.sqrt_f32_non_members()
        wrong = cases.bits(probe(mhx, P.F_SQRT_NORMAL, xn)) != cases.bits(np.sqrt(xn))
        print("fp32 mhx_sqrt_normal below its domain, misrounded:", xn[wrong].tolist(), "of", xn.tolist())
    if real == "f64":
        xr = P.sqrt_f64_random()
        same(probe(mhx, P.F_SQRT_NORMAL, xr), np.sqrt(xr), "mhx_sqrt_normal on [2.2e-16, 74]", xr)


# ---- division (fp64 only: the fp32 spec has none of its own) ---------------------------------------------------------------------
def test_div_normal_is_correctly_rounded(mhx, oracle):
    """Near-midpoint quotients at every exponent pair of primitive_probes.DIV_MEMBERS -- the domain the header claims -- and random
    operands of mhx_log_core's own ranges.  DIV_NON_MEMBERS are finite normal operands with a normal quotient OUTSIDE that domain
    (1 / b subnormal, or the residual a - b q inexact), and so is a == -0 (it gives +0): evaluated and counted, not asserted --
    nothing sends them.  (Measured: of 300 near-midpoint quotients per exponent pair, none misrounded while |a| >= 2^-969 and
    |b| < 2^1023; 1 at |a| ~ 2^-970, 47 at 2^-975, about half from 2^-1000 down; 8 at |b| >= 2^1023.)"""
    mhx.set_default_dtype("f64")
    for eb, eq in P.DIV_MEMBERS:
        a, b, q = P.div_midpoint_arrays("f64", 500, eb, eq, seed=(eb + 1100) * 4096 + eq + 1100)
        assert np.array_equal(cases.bits(a / b), cases.bits(q))
        for sa, sb in ((1, 1), (-1, 1), (1, -1)):
            same(probe(mhx, P.F_DIV_NORMAL, np.stack([sa * a, sb * b])), (sa * sb) * q, "mhx_div_normal, b ~ 2^%d, quotient ~ 2^%d" % (eb, eq),
                 np.stack([sa * a, sb * b]))
    rng = np.random.default_rng(20269)
    b = rng.uniform(1.7, 2.42, 2 ** 20)
    a = np.concatenate([rng.uniform(-0.3, 0.42, 2 ** 19), rng.uniform(-1, 1, 2 ** 19) * np.exp2(rng.integers(-53, 0, 2 ** 19))])
    ab = np.concatenate([np.stack([a, b]), np.array([[0.0, 0.0, 0.0], [2.0, 2.42, 1.75]])], axis=1)
    same(probe(mhx, P.F_DIV_NORMAL, ab), ab[0] / ab[1], "mhx_div_normal on mhx_log_core's ranges", ab)
    wrong = {}
    for eb, eq in P.DIV_NON_MEMBERS:
        a, b, q = P.div_midpoint_arrays("f64", 500, eb, eq, seed=(eb + 1100) * 4096 + eq + 1100)
        got = probe(mhx, P.F_DIV_NORMAL, np.stack([a, b]))
        wrong[(eb, eq)] = int((cases.bits(got) != cases.bits(q)).sum())
    print("mhx_div_normal outside its domain, misrounded of 500 per (exponent of b, of the quotient):", wrong)
    print("mhx_div_normal(-0.0, 2.0) =", probe(mhx, P.F_DIV_NORMAL, np.array([[-0.0], [2.0]]))[0])


def test_log_core_division_is_correctly_rounded(mhx, oracle):
    """f / (2 + f), f = m - 1, for 2^22 random mantissas m of mhx_log_core's interval, its ends, 1 and the neighbours of each"""
    mhx.set_default_dtype("f64")
    m = P.log_core_div_inputs()
    f = m - 1.0
    assert same(probe(mhx, P.F_LOG_CORE_DIV, m), f / (2.0 + f), "mhx_div_normal(f, 2 + f)", m) == 0


# ---- sincos, uniforms, Box-Muller, the Cauchy quotient -----------------------------------------------------------------------------
def _angle_words(dt):
    return np.concatenate([P.angle_edge_words(dt), P.angle_random_words(dt)])


def test_sincos2pi_matches_the_oracle(mhx, oracle, real):
    a = _angle_words(real)
    s, c = ref(("sincos", real), lambda: P.orc_sincos(a, real))
    w = P.split_angle(real, a)
    assert same(probe_words(mhx, P.F_SINCOS, w), s, "sin of mhx_sincos2pi", a) == 0
    assert same(probe_words(mhx, P.F_SINCOS, w, second=True), c, "cos of mhx_sincos2pi", a) == 0


def test_uniforms_match_the_oracle(mhx, oracle, real):
    w = P.uniform_words(real)
    for fn, which in ((P.F_U01_OPEN, "open"), (P.F_U01_HALF, "half")):
        want = P.orc_u01(which, w, real)
        assert same(probe_words(mhx, fn, w), want, "mhx_u01_" + which, w) == 0
    # the second uniform of a family block: words (z, w) / word z
    blk = np.zeros((4, w.shape[1]), dtype=np.uint64)
    blk[2:2 + w.shape[0]] = w
    assert same(probe_words(mhx, P.F_FAM_U_OPEN2, blk), P.orc_u01("open", w, real), "mhx_fam_u_open2", blk) == 0
    open_ = P.orc_u01("open", w, real)
    assert (open_ > 0).all() and (open_ <= 1).all() and ((open_ < 1).all() or real == "f32")


def test_normal_pair_matches_the_composition_of_the_spec(mhx, oracle, real):
    blk = P.block_words(real)
    n0, n1 = P.normal_pair_reference(real, blk)
    w = blk if real == "f64" else blk[:2]
    same(probe_words(mhx, P.F_NORMAL_PAIR, w), n0, "n0 of mhx_normal_pair", w)
    same(probe_words(mhx, P.F_NORMAL_PAIR, w, second=True), n1, "n1 of mhx_normal_pair", w)


def test_cauchy_quotient_matches_the_oracle(mhx, oracle, real):
    blk = P.block_words(real)
    assert same(probe_words(mhx, P.F_CAUCHY_QUOTIENT, blk), P.cauchy_quotient_reference(real, blk), "s / c of mhx_fam_phase", blk) == 0
    # at the four quarter turns the draw of family_restatement: fma(1, s / c, 0) = 0, -inf, 0, -inf
    import family_restatement as FR
    q = np.zeros((4, 4), dtype=np.uint64)
    q[2:2 + (2 if real == "f64" else 1)] = P.split_angle(real, P.quarter_turn_words(real))
    got = probe_words(mhx, P.F_CAUCHY_QUOTIENT, q)
    for i in range(4):
        s, c = FR.phase([int(v) for v in q[:, i]])
        with np.errstate(all="ignore"):
            want = s / c
        assert cases.bits(got[i:i + 1])[0] == cases.bits(np.array([want]))[0], (i, got[i], want)
    assert got.tolist() == [0.0, -np.inf, 0.0, -np.inf]


# ---- the pre-built kernels: the same header compiled ahead of time ----------------------------------------------------------------
def test_funnel_at_the_cut_offs_of_exp(mhx, oracle, real):
    """mhx.Funnel takes mhx_exp(-x[0]) (mhx_targets.h): x[0] at minus each cut-off and 6 neighbours on each side, +-inf, NaN"""
    W = P.Width(real)
    v = -np.concatenate([W.neighbours(W.exp_hi, 6), W.neighbours(W.exp_lo, 6), P.exp_specials(real)])
    d = 3
    x = np.concatenate([np.stack([v, np.full_like(v, 0.5), np.full_like(v, -0.25)]), np.stack([v, np.zeros_like(v), np.zeros_like(v)])], axis=1)
    lp = mhx.logdensity(mhx.DensityModel(mhx.Funnel(d)), x)
    ot = oracle.Target(oracle.TARGET_FUNNEL, d)
    same(lp, np.array([ot(x[:, i]) for i in range(x.shape[1])], dtype=cases.R()), "Funnel", x)


def test_iid_normal_at_the_edges_of_log(mhx, oracle, real):
    """mhx.IIDNormal takes mhx_log(sigma): sigma subnormal, the smallest normal, max, +inf, -0.0, NaN"""
    W = P.Width(real)
    sigma = W.from_bits([1, 1000, W.tiny - 1, W.tiny, W.inf - 1, W.inf, W.sign, W.qnan])
    th = np.stack([np.full_like(sigma, 0.25), sigma])
    data = np.array([0.5, -1.25, 2.0])
    lp = mhx.logdensity(mhx.DensityModel(mhx.IIDNormal(data)), th)
    ot = oracle.Target(oracle.TARGET_IID_NORMAL, 2, params=data)
    same(lp, np.array([ot(th[:, i]) for i in range(th.shape[1])], dtype=cases.R()), "IIDNormal", th)
