"""CPU: the inputs of tests/test_gpu_primitives.py are what they claim to be, and the oracle holds the suite's accuracy bound at them.

The near-midpoint generators are checked in exact integer arithmetic (Python ints / fractions), and numpy's sqrt and / are shown to
round every one of their cases the way the integers say: that is what makes np.sqrt and a / b legitimate references for the device's
shortened sequences.  The oracle's log / exp / sincos are compared with mpmath (fp64) and float64 (fp32) at the edge lists."""
import fractions
import math

import numpy as np
import pytest

import primitive_probes as P

WIDTHS = ["f32", "f64"]


# ---- generators ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 9, -7, 1593, -1599])
def test_hensel_roots_are_the_four_square_roots(r):
    for k in (3, 4, 25, 55):
        roots = P.sqrt_roots_mod_pow2(r, k)
        assert len(set(roots)) == 4 and all(0 <= m < 2 ** k and (m * m - r) % 2 ** k == 0 for m in roots)
    brute = [m for m in range(2 ** 12) if (m * m - r) % 2 ** 12 == 0]
    assert brute == P.sqrt_roots_mod_pow2(r, 12)


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("dt", WIDTHS)
def test_sqrt_midpoint_cases_are_near_midpoints(dt, parity):
    W = P.Width(dt)
    p = W.p
    cases = P.sqrt_midpoint_cases(p, parity)
    assert len(cases) >= 200
    assert len(set(cases)) == len(cases)
    for M, r in cases:
        assert M % 2 == 1 and M.bit_length() == p + 1 and r % 8 == 1 and 0 < abs(r) < 1600
        X4 = M * M - r                                                   # 4 X
        assert X4 % 4 == 0
        X = X4 // 4
        sh = X.bit_length() - p
        assert X.bit_length() == 2 * p - 1 + parity and X % (1 << sh) == 0          # a p-bit significand: x is representable
        # sqrt(X) is strictly between the neighbouring significands (M - 1) / 2 and (M + 1) / 2, on the side of M / 2 that r says
        assert (M - 1) ** 2 < 4 * X < (M + 1) ** 2 and (4 * X < M * M) == (r > 0)
        # distance to the midpoint in ulp (ulp of the root = 1 here): M / 2 - sqrt(X) = r / (4 (M / 2 + sqrt(X))) ~ r / (4 M)
        root2 = math.isqrt(4 * X)                                          # floor(2 sqrt(X)): M - 1 or M
        assert root2 in (M - 1, M)
        dist = fractions.Fraction(abs(r), 2 * (M + root2))                 # >= the true distance |r| / (2 (M + 2 sqrt(X)))
        assert dist < fractions.Fraction(1, 2 ** 10)


@pytest.mark.parametrize("dt", WIDTHS)
def test_numpy_sqrt_rounds_the_midpoint_cases_correctly(dt):
    W = P.Width(dt)
    x, want = P.sqrt_midpoint_arrays(dt, P.SQRT_MIDPOINT_SCALES[dt])
    assert x.dtype == W.real and len(x) >= 400 * len(P.SQRT_MIDPOINT_SCALES[dt])
    # the arrays hold the integers of the cases exactly: x and the rounded root as fractions
    p = W.p
    i = 0
    for parity in (0, 1):
        for M, r in P.sqrt_midpoint_cases(p, parity):
            for k in P.SQRT_MIDPOINT_SCALES[dt]:
                assert fractions.Fraction(float(x[i])) == fractions.Fraction(M * M - r, 4) * fractions.Fraction(4) ** (1 - p + k)
                Y = (M - 1) // 2 if r > 0 else (M + 1) // 2
                assert fractions.Fraction(float(want[i])) == Y * fractions.Fraction(2) ** (1 - p + k)
                i += 1
    assert i == len(x)
    lo, hi = (2.0 ** -52, 74.0) if dt == "f64" else (2.0 ** -80, 2.0 ** 122)     # the domains of the two mhx_sqrt_normal
    assert lo <= x.min() and x.max() < hi
    if dt == "f32":                                                                # ... and the Box-Muller domain inside it
        assert ((x >= 1.19e-7) & (x <= 46)).sum() >= 3 * 400
    assert np.array_equal(P.Width(dt).to_bits(np.sqrt(x)), P.Width(dt).to_bits(want))


@pytest.mark.parametrize("dt", WIDTHS)
def test_div_midpoint_cases_are_near_midpoints_and_numpy_divides_them_correctly(dt):
    W = P.Width(dt)
    p = W.p
    cases = P.div_midpoint_cases(p, 2000)
    assert len(cases) == 2000
    for A, B, M, r in cases:
        assert A.bit_length() == p and B.bit_length() == p and B % 2 == 1 and M % 2 == 1 and M.bit_length() == p + 1
        assert r % 2 == 1 and abs(r) < 100
        q = fractions.Fraction(A, B) * 2 ** p                              # the quotient in ulp of [1/2, 1)
        assert abs(q - fractions.Fraction(M, 2)) == fractions.Fraction(abs(r), 2 * B) <= fractions.Fraction(abs(r), 2 ** p)
        assert (q < fractions.Fraction(M, 2)) == (r > 0)
    a, b, want = P.div_midpoint_arrays(dt, 2000, 1, -2)
    for (A, B, M, r), av, bv, qv in zip(cases, a, b, want):
        assert fractions.Fraction(float(av)) / fractions.Fraction(float(bv)) == fractions.Fraction(A, B) / 2      # (quotient exponent -2: A / B in [1/2, 1) halved)
        Q = (M - 1) // 2 if r > 0 else (M + 1) // 2
        assert fractions.Fraction(float(qv)) == Q * fractions.Fraction(2) ** (-2 - (p - 1))
    assert np.array_equal(W.to_bits(a / b), W.to_bits(want))


def test_div_domain_table():
    for eb, eq in P.DIV_MEMBERS:
        assert P.div_member(eb, eq), (eb, eq)
    for eb, eq in P.DIV_NON_MEMBERS:
        assert not P.div_member(eb, eq), (eb, eq)
    W = P.Width("f64")
    for eb, eq in P.DIV_MEMBERS + P.DIV_NON_MEMBERS:                       # finite normal operands, normal quotient -- all of them
        a, b, q = P.div_midpoint_arrays("f64", 50, eb, eq)
        for v in (a, b, q):
            bits = W.to_bits(np.abs(v))
            assert ((bits >= W.tiny) & (bits < W.inf)).all(), (eb, eq)
        assert np.array_equal(W.to_bits(a / b), W.to_bits(q)), (eb, eq)
        assert (np.frexp(b)[1] - 1 == eb).all() and (np.frexp(q)[1] - 1 == eq).all()


@pytest.mark.parametrize("dt", WIDTHS)
def test_edge_lists_hold_what_they_name(dt):
    W = P.Width(dt)
    R = W.real
    fi = np.finfo(R)
    le = P.log_edges(dt)
    assert le.dtype == R and (le > 0).all() and np.isfinite(le).all()
    for k in (1, 2, 3, 5, 1000):
        assert R(k) * R(fi.smallest_subnormal) in le
    for v in (fi.tiny, np.nextafter(R(fi.tiny), R(0)), np.nextafter(R(fi.tiny), R(1)), fi.max, R(1)):
        assert v in le
    one = R(1)
    up = dn = one
    for _ in range(8):
        up, dn = np.nextafter(up, R(2)), np.nextafter(dn, R(0))
        assert up in le and dn in le
    split = W.from_bits([W.log_split])[0]
    assert abs(float(split) - (math.sqrt(0.5) if dt == "f64" else 2.0 / 3.0)) < 1e-7
    for s in (R(1), R(2), R(2.0 ** -40)):
        for v in (split * s, np.nextafter(split * s, R(0)), np.nextafter(split * s, R(np.inf))):
            assert v in le
    ls = P.log_specials(dt)
    assert np.isnan(ls).sum() == 2 and np.isposinf(ls).sum() == 1 and np.isneginf(ls).sum() == 1
    assert (W.to_bits(ls) == 0).sum() == 1 and (W.to_bits(ls) == W.sign).sum() == 1 and R(-1) in ls and -R(fi.tiny) in ls
    lr = P.log_random(dt, 2 ** 10)
    assert (lr > 0).all() and np.isfinite(lr).all() and (lr < fi.tiny).any() == (dt == "f32")   # (2^-9 of the fp32 patterns are subnormal)
    pn = P.positive_normal(dt, P.log_inputs(dt, 2 ** 10))
    assert (pn >= fi.tiny).all() and np.isfinite(pn).all() and fi.max in pn and fi.tiny in pn
    # exp: the cut-offs are the literals of the device header and of the oracle
    for path in (P.DEVICE_MATH_H, P.ROOT + "/oracle/mhx_oracle.c"):
        txt = open(path).read()
        for lit in (W.exp_hi_text, W.exp_lo_text):
            assert lit + ("f)" if dt == "f32" else ")") in txt, (path, lit)
    ee = P.exp_edges(dt)
    for c in (W.exp_hi, W.exp_lo):
        v = lo = hi = R(c)
        assert float(v) == c
        for _ in range(6):
            lo, hi = np.nextafter(lo, R(-np.inf)), np.nextafter(hi, R(np.inf))
            assert lo in ee and hi in ee
    with np.errstate(all="ignore"):
        sub = ee[(ee > W.exp_lo) & (ee < R(np.log(float(fi.tiny))))]
    assert len(sub) >= 2 ** 12 - 2
    n = np.rint(ee.astype(np.float64) * W.log2e)
    near0 = np.abs(ee) < 3
    assert set(n[near0].astype(int)) >= set(range(-3, 4))                                  # both parities, both signs


def test_funnel_takes_exp_of_minus_its_first_coordinate():
    """tests/test_gpu_primitives.py puts x[0] at -(cut-off of mhx_exp): the factor is read here"""
    assert "const mhx_real ev = mhx_exp(-v);" in open(P.TARGETS_H).read()


def test_words_to_x_round_trips():
    w = np.array([[0, 1, 0xffffffff, 0x12345678], [0xffff0000, 0x0000ffff, 0x80000000, 7]], dtype=np.uint64)
    x = P.words_to_x(w, selector=1.0)
    assert x.shape == (5, 4) and (x[4] == 1.0).all() and (x[:4] == x[:4].astype(np.float32)).all() and x[:4].max() <= 65535
    back = (x[0::2][:2].astype(np.uint64) << np.uint64(16)) | x[1::2].astype(np.uint64)
    assert np.array_equal(back, w)


# ---- the oracle at the edges -----------------------------------------------------------------------------------------------------
def _ulp_errors(got, want_mp, W, mp):
    """|got - want| in ulp of want, the ulp of a subnormal taken as the subnormal spacing; an infinite result is read as 2^emax, the
    value after the largest finite number, and so is any exact value beyond it (where infinity is the only rounded answer)"""
    emax = 1024 if W.dt == "f64" else 128
    out = []
    for g, w in zip(got.tolist(), want_mp):
        w = min(w, mp.mpf(2) ** emax)
        gm = mp.mpf(2) ** emax * (1 if g > 0 else -1) if math.isinf(g) else mp.mpf(g)
        ex = max(int(mp.floor(mp.log(abs(w), 2))), W.emin) if w != 0 else W.emin
        ex = min(ex, emax - 1)
        out.append(float(abs(gm - w) / mp.mpf(2) ** (ex - W.mant)))
    return np.array(out)


@pytest.mark.parametrize("dt", WIDTHS)
def test_oracle_log_at_the_edges_against_mpmath(oracle, dt):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    W = P.Width(dt)
    x = np.concatenate([P.log_edges(dt), P.log_random(dt, 2 ** 11)])
    got = P.orc_map("orc_log", x, dt)
    err = _ulp_errors(got, [mp.log(mp.mpf(float(v))) for v in x], W, mp)
    assert err.max() < 1.0, (err.max(), x[err.argmax()])
    sp = P.orc_map("orc_log", P.log_specials(dt), dt)
    assert sp[0] == np.inf and np.isnan(sp[1]) and sp[2] == -np.inf and sp[3] == -np.inf and np.isnan(sp[4:]).all()


@pytest.mark.parametrize("dt", WIDTHS)
def test_oracle_exp_at_the_edges_against_mpmath(oracle, dt):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    W = P.Width(dt)
    x = np.concatenate([P.exp_edges(dt), P.exp_random(dt, 2 ** 11)])
    got = P.orc_map("orc_exp", x, dt)
    err = _ulp_errors(got, [mp.exp(mp.mpf(float(v))) for v in x], W, mp)
    assert err.max() < 1.0, (err.max(), x[err.argmax()])
    # beyond the cut-offs exactly inf / +0, at them still finite
    R = W.real
    hi, lo = R(W.exp_hi), R(W.exp_lo)
    at = P.orc_map("orc_exp", [hi, np.nextafter(hi, R(np.inf)), lo, np.nextafter(lo, R(-np.inf))], dt)
    assert np.isfinite(at[0]) and at[1] == np.inf and np.isfinite(at[2]) and at[3] == 0 and not np.signbit(at[3])
    sp = P.orc_map("orc_exp", P.exp_specials(dt), dt)
    assert sp[0] == np.inf and sp[1] == 0 and np.isnan(sp[2:]).all()


def test_oracle_fp32_log_exp_at_the_edges_against_float64(oracle):
    """the whole fp32 lists, the 2^20 random arguments included, against numpy's float64 (its own error, 1e-16 relative, is
    2e-9 ulp of a float)"""
    W = P.Width("f32")
    fi = np.finfo(np.float32)

    def ulp_err(got, want):
        with np.errstate(all="ignore"):
            want = np.minimum(want, 2.0 ** 128)                             # (as in _ulp_errors)
            ex = np.clip(np.floor(np.log2(np.abs(want))), W.emin, 127)
            ex = np.where(want == 0, W.emin, ex)
            g = got.astype(np.float64)
            g = np.where(np.isinf(g), np.sign(g) * 2.0 ** 128, g)
            return np.abs(g - want) / 2.0 ** (ex - W.mant)

    x = np.concatenate([P.log_edges("f32"), P.log_random("f32")])
    err = ulp_err(P.orc_map("orc_log", x, "f32"), np.log(x.astype(np.float64)))
    assert err.max() < 1.0, (err.max(), x[err.argmax()])
    x = np.concatenate([P.exp_edges("f32"), P.exp_random("f32")])
    err = ulp_err(P.orc_map("orc_exp", x, "f32"), np.exp(x.astype(np.float64)))
    assert err.max() < 1.0, (err.max(), x[err.argmax()])
    assert fi.smallest_subnormal > 0


@pytest.mark.parametrize("dt", WIDTHS)
def test_oracle_sincos_at_the_boundary_words_against_mpmath(oracle, dt):
    """the bounds of test_f64_sincos_accuracy (0.75 ulp of the spec's angle) / test_sincos_accuracy (2e-7 absolute), and exact
    0 / +-1 at the quarter turns"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    W = P.Width(dt)
    words = [int(a) for a in P.angle_edge_words(dt)]
    s, c = P.orc_sincos(words, dt)
    if dt == "f64":
        worst = 0.0
        for a, sv, cv in zip(words, s.tolist(), c.tolist()):
            kk = (a + 2 ** 61) % 2 ** 64                                  # the spec's angle: quadrant + 52-bit residual
            q, t = kk >> 62, ((kk & (2 ** 62 - 1)) - 2 ** 61) >> 10
            ang = 2 * mp.pi * (mp.mpf(q) / 4 + mp.mpf(t) * mp.mpf(2) ** -54)
            for g, w in ((sv, mp.sin(ang)), (cv, mp.cos(ang))):
                if abs(w) > mp.mpf("1e-30"):
                    worst = max(worst, float(_ulp_errors(np.array([g]), [w], W, mp)[0]))
        assert worst < 0.75, worst
    else:
        for a, sv, cv in zip(words, s.tolist(), c.tolist()):
            ang = 2 * mp.pi * mp.mpf(a) / 2 ** 32
            assert abs(mp.mpf(sv) - mp.sin(ang)) < 2e-7 and abs(mp.mpf(cv) - mp.cos(ang)) < 2e-7, a
    s, c = P.orc_sincos(P.quarter_turn_words(dt), dt)
    assert s.tolist() == [0.0, 1.0, 0.0, -1.0] and c.tolist() == [1.0, 0.0, -1.0, 0.0]
    # the signs of the zeros, as the quadrant's sign rule leaves them: the Cauchy quotient s / c is -inf at both odd quarter turns
    assert np.signbit(s).tolist() == [False, False, True, True] and np.signbit(c).tolist() == [False, True, True, False]
    with np.errstate(all="ignore"):
        t = s / c
    assert t[1] == -np.inf and t[3] == -np.inf and t[0] == 0 and t[2] == 0
