"""Derived quantities without a GPU (mhx.trace.trace_map, MHX_DERIVED): the recorded map equals the Python
callable on floats, the emitted source compiles for the host (tests/derived_ref.py) and equals the recorded program in both widths,
what cannot be traced says so, and the two entry points are declared and exported.

Agreement is exact where no log or exp occurs: the inputs are small dyadic numbers, so every product and sum of those maps is exact
in fp32 as well.  With log / exp the bound is the one tests/test_trace_cpu.py uses for the host-compiled log-densities
(libm's functions against the engine's): 1e-12 (fp64) / 2e-5 (fp32), relative to max(1, |value|)."""
import math
import os
import re

import numpy as np
import pytest

import mhx.trace as T
import derived_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X_ROWS = np.array([[0.5, 1.0], [1.5, 0.25], [-2.0, 0.5], [3.0, 2.0]])           # (x_i, w_i) of the fitted mean


def _fitted(t):
    return T.sum_over(X_ROWS, lambda r: (t[0] + t[1] * r[0]) * r[1])


# name -> (callable, dim, names, lp, uses log / exp)
MAPS = {
    "sigma2": (lambda t: t.sigma ** 2, 2, ["mu", "sigma"], False, False),        # the README model's variance
    "contrast": (lambda t: t[1] - t[0], 3, None, False, False),
    "indicator": (lambda t: [T.where(t[0] > 0, 1.0, 0.0), T.where((t[0] > 0) & (t[1] <= 0.5), t[0], -1.0)], 2, None, False, False),
    "fitted": (lambda t: [_fitted(t), T.fma(t[0], t[1], 1.0), T.maximum(t[0], t[1]), T.minimum(t[0], 0.0)], 2, None, False, False),
    "with_lp": (lambda t, lp: [lp, t[0] + lp, abs(lp)], 2, None, True, False),
    "constants": (lambda t: [1.5, -2.0, 3], 2, None, False, False),
    "explog": (lambda t: [T.exp(t[0]), T.log(abs(t[1]) + 1.0), T.sqrt(t[1] * t[1] + 1.0)], 2, None, False, True),
}
TOL = {"f64": 1e-12, "f32": 2e-5}


def _draws(dim, n=24, seed=3):
    """dyadic draws [n][dim + 1]: multiples of 1/16 in [-4, 4), the last column the lp"""
    rng = np.random.default_rng(seed)
    return rng.integers(-64, 64, size=(n, dim + 1)).astype(np.float64) / 16.0


def _call(f, names, lp, row, dim):
    theta = T.NamedVec(list(row[:dim]), names) if names else T.Vec(list(row[:dim]))
    out = f(theta, float(row[dim])) if lp else f(theta)
    out = list(out.items) if isinstance(out, T.Vec) else (list(out) if isinstance(out, (list, tuple)) else [out])
    return np.array([float(v) for v in out])


@pytest.mark.parametrize("name", sorted(MAPS))
def test_traced_map_equals_the_callable(name):
    f, dim, names, lp, transcendental = MAPS[name]
    m = T.trace_map(f, dim, names=names, lp=lp)
    assert m.dim == dim and m.lp == lp and "MHX_DERIVED(x, y, d, data, ndata)" in m.source
    for row in _draws(dim):
        want = _call(f, names, lp, row, dim)
        got = m.evaluate(row)
        assert got.shape == (m.nout,) == want.shape
        if transcendental:
            assert np.all(np.abs(got - want) <= TOL["f64"] * np.maximum(1.0, np.abs(want))), (name, row, got, want)
        else:
            assert np.array_equal(got, want), (name, row, got, want)
        if lp:
            assert np.array_equal(m.evaluate(row[:dim], lp=row[dim]), got)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_emitted_source_compiles_for_the_host_and_agrees(name, dt):
    from oracle import oracle as O
    old = O.get_dtype()
    O.set_dtype(dt)
    try:
        f, dim, names, lp, transcendental = MAPS[name]
        m = T.trace_map(f, dim, names=names, lp=lp)
        rows = _draws(dim, n=12)
        x = np.ascontiguousarray(rows.reshape(4, 3, dim + 1).transpose(0, 2, 1))         # [N = 4][dim + 1][C = 3]
        got = derived_ref.host_map(O, m.source)(x, m.nout, data=m.data)
        assert got.dtype == O.real() and got.shape == (4, m.nout + 1, 3)
        assert np.array_equal(got[:, m.nout, :], x[:, dim, :].astype(O.real()))            # the lp row, copied
        for t in range(4):
            for c in range(3):
                want = m.evaluate(x[t, :, c])
                have = got[t, :m.nout, c].astype(np.float64)
                if transcendental:
                    assert np.all(np.abs(have - want) <= TOL[dt] * np.maximum(1.0, np.abs(want))), (name, dt, have, want)
                else:
                    assert np.array_equal(have, want), (name, dt, have, want)
    finally:
        O.set_dtype(old)


def test_outputs_and_names_are_checked():
    m = T.trace_map(MAPS["fitted"][0], 2)
    assert m.nout == 4 and "y.set(3, " in m.source and "y.set(4, " not in m.source
    assert m.data is not None and np.array_equal(m.data, X_ROWS.ravel())                  # the rows of the sum_over loop
    assert m.source.count("for (int k = 0; k < 4; ++k)") == 1
    assert T.trace_map(lambda t: t[0], 1).nout == 1
    assert T.trace_map(lambda t: T.Vec([t[0], t[1]]), 2).nout == 2                        # a Vec is a list of outputs
    assert T.trace_map(lambda t: t * 2.0, 3).nout == 3
    one = T.trace_map(lambda t: t.b, 2, names=["a", "b"])
    assert "x[1]" in one.source and "x[0]" not in one.source                             # a row that is not named is not read
    assert "x[2]" in T.trace_map(lambda t, lp: lp, 2, lp=True).source                     # x[d] is the draw's lp
    with pytest.raises(T.TraceError, match="names"):
        T.trace_map(lambda t: t[0], 2, names=["a"])
    with pytest.raises(T.TraceError, match="dim"):
        T.trace_map(lambda t: 1.0, 0)
    with pytest.raises(T.TraceError, match="evaluate"):
        T.trace_map(lambda t, lp: lp, 2, lp=True).evaluate([1.0, 2.0])


def test_what_cannot_be_traced_raises():
    with pytest.raises(T.TraceError, match="output 0"):
        T.trace_map(lambda t: "sigma", 2)                                                 # a wrong return type
    with pytest.raises(T.TraceError, match="where"):
        T.trace_map(lambda t: [t[0], t[0] > 0], 2)                                        # a condition is not a number
    with pytest.raises(T.TraceError, match="at least one"):
        T.trace_map(lambda t: [], 2)
    other = []
    T.trace_map(lambda t: other.append(t[0]) or t[0], 1)
    with pytest.raises(T.TraceError, match="another trace"):
        T.trace_map(lambda t: other[0], 1)                                                # a value of another trace
    with pytest.raises(T.TraceError, match="where"):
        T.trace_map(lambda t: t[0] if t[0] > 0 else -math.inf, 1)                         # a branch on a parameter value


def test_the_entry_points_are_declared_and_exported():
    import mhx
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mhx.h")).read(), flags=re.S)
    flat = " ".join(hdr.split())
    assert ("int mhx_run_derive(const mhx_run *src, const char *source, int32_t nout, const void *data, size_t ndata, "
            "mhx_run **out);") in flat
    assert ("int mhx_ctx_derive(mhx_ctx *ctx, const void *d_tensor, int64_t n_samples, int32_t dim1, int64_t nchains, "
            "const char *source, int32_t nout, const void *data, size_t ndata, mhx_run **out);") in flat
    lib = mhx.lib()
    for name in ("mhx_run_derive", "mhx_ctx_derive"):
        assert name in mhx.EXPORTS and hasattr(lib, name)
    assert len(lib.mhx_run_derive.argtypes) == 6 and len(lib.mhx_ctx_derive.argtypes) == 10
    assert mhx.HipMap("MHX_DERIVED(x, y, d, data, ndata) {}", 2, data=[1, 2]).nout == 2 and issubclass(mhx.DerivedRun, mhx.Run)
