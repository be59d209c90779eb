"""The numpy restatement the device histograms are held to (tests/histogram_ref.py) against numpy's own histograms, the host half of
the histogram / density surface (mhx/api.py: histogram_edges, silverman_bandwidth, density_from_counts) and the six new entry points
in the header, the ctypes mirror and the library alike.  No device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from histogram_ref import histogram2d_numpy, histogram_numpy, kde_direct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases(rng):
    """draws as float64: fine and coarse scales, ties, fp32-representable values"""
    n = int(rng.integers(1, 400))
    kind = int(rng.integers(0, 5))
    if kind == 0:
        return rng.normal(size=n) * 10.0 ** rng.integers(-6, 7)
    if kind == 1:
        return np.round(rng.normal(size=n) * 3.0) / 4.0                 # ties
    if kind == 2:
        return rng.normal(size=n).astype(np.float32).astype(np.float64)
    if kind == 3:
        return 1e4 + rng.choice([-0.01, 0.0, 0.01], size=n)
    return rng.choice([-0.0, 0.0, 1.0, 2.5], size=n)


def test_restatement_equals_numpy_histogram_in_both_forms():
    import mhx
    rng = np.random.default_rng(20)
    for case in range(300):
        x = _cases(rng)
        bins = int(rng.choice([1, 2, 7, 64, 2048]))
        lo, hi = float(x.min()), float(x.max())
        if case % 3 == 1:                                   # a range inside the data: draws below and above
            lo, hi = lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo)
        e = mhx.histogram_edges(lo, hi, bins)
        want_r, edges_r = np.histogram(x, bins=bins, range=(lo, hi))
        assert np.array_equal(e, edges_r) and np.array_equal(e, np.histogram_bin_edges([], bins, (lo, hi)))
        want_e, _ = np.histogram(x, bins=e)
        counts, outside = histogram_numpy(x, e)
        assert np.array_equal(counts, want_r) and np.array_equal(counts, want_e), (case, bins)
        assert counts.sum() + outside.sum() == x.size and outside[2] == 0
        if case % 3 != 1:
            assert np.array_equal(counts, np.histogram(x, bins)[0]) and outside.sum() == 0      # the automatic range


def test_restatement_equals_numpy_histogram2d():
    rng = np.random.default_rng(21)
    for case in range(60):
        x, y = _cases(rng), None
        y = np.resize(_cases(rng), x.size)
        B = int(rng.choice([1, 5, 32, 128]))
        ex = np.histogram_bin_edges([], B, (x.min(), x.max()))
        ey = np.histogram_bin_edges([], B, (y.min() + 0.1 * (y.max() - y.min()), y.max()))
        want, wx, wy = np.histogram2d(x, y, bins=[ex, ey])
        H, outside = histogram2d_numpy(x, y, ex, ey)
        assert np.array_equal(H, want.astype(np.int64)) and H.sum() + outside == x.size, case
        want2, _, _ = np.histogram2d(x, y, bins=B, range=[(ex[0], ex[-1]), (ey[0], ey[-1])])
        assert np.array_equal(H, want2.astype(np.int64)), case
        assert np.array_equal(H.sum(axis=1), histogram_numpy(x[(y >= ey[0]) & (y <= ey[-1])], ex)[0])


def test_edges_of_a_constant_row_repeated_edges_and_draws_at_every_edge():
    import mhx
    # lo == hi: numpy widens by half to either side, and the restatement puts the draws where numpy does
    e = mhx.histogram_edges(3.25, 3.25, 4)
    assert np.array_equal(e, [2.75, 3.0, 3.25, 3.5, 3.75]) and np.array_equal(e, np.histogram(np.full(9, 3.25), 4)[1])
    assert np.array_equal(histogram_numpy(np.full(9, 3.25), e)[0], np.histogram(np.full(9, 3.25), 4)[0])
    assert np.array_equal(histogram_numpy(np.full(9, 3.25), e)[0], [0, 0, 9, 0])
    # repeated edges: of a run of equal edges the last takes the draw; at the very end the closed last bin does
    e = np.array([0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0])
    x = np.array([0.0, -0.0, 0.5, 1.0, 1.0, 1.5, 2.0, 2.0, 2.0, np.nextafter(2.0, 3.0), np.nextafter(0.0, -1.0)])
    counts, outside = histogram_numpy(x, e)
    assert np.array_equal(counts, np.histogram(x, bins=e)[0]) and np.array_equal(counts, [0, 3, 0, 0, 3, 3])
    assert np.array_equal(outside, [1, 1, 0])
    assert np.array_equal(histogram_numpy([1.0, 1.0], [1.0, 1.0, 1.0])[0], [0, 2])
    # draws exactly on every edge and one ulp to either side, in both widths' ulps
    for dt in (np.float32, np.float64):
        e = np.linspace(-2.0, 2.0, 33)                      # multiples of 1/8: representable in both widths
        on = e.astype(dt)
        x = np.concatenate([on, np.nextafter(on, dt(np.inf)), np.nextafter(on, dt(-np.inf))]).astype(np.float64)
        counts, outside = histogram_numpy(x, e)
        assert np.array_equal(counts, np.histogram(x, bins=e)[0]) and np.array_equal(counts, np.histogram(x, 32, (-2.0, 2.0))[0])
        want = np.full(32, 3)
        want[-1] = 4                                        # a bin holds its edge, the edge's upper neighbour and the next edge's lower one;
                                                            # the last bin also e[B] itself
        assert np.array_equal(counts, want) and np.array_equal(outside, [1, 1, 0])
    # infinities and NaNs of either sign
    x = np.array([np.inf, -np.inf, -np.inf, np.nan, -np.nan, 0.5])
    counts, outside = histogram_numpy(x, [0.0, 1.0])
    assert np.array_equal(counts, [1]) and np.array_equal(outside, [2, 1, 2])
    H, out2 = histogram2d_numpy(x, np.full(6, 0.5), [0.0, 1.0], [0.0, 1.0])
    assert H[0, 0] == 1 and out2 == 5


def test_histogram_edges_refusals():
    import mhx
    assert mhx.histogram_edges is mhx.api.histogram_edges
    for lo, hi, bins in ((0.0, 1.0, 0), (1.0, 0.0, 4), (float("nan"), 1.0, 4), (0.0, float("inf"), 4)):
        with pytest.raises(mhx.ArgumentError, match="histogram_edges"):
            mhx.histogram_edges(lo, hi, bins)
    assert isinstance(mhx.ArgumentError(0, ""), ValueError)     # where numpy raises ValueError


def test_silverman_bandwidth_as_kerneldensity_applies_it():
    import mhx
    S = 1000
    assert mhx.silverman_bandwidth(2.0, -1.0, 1.0, S) == 0.9 * min(2.0, 2.0 / 1.34) * S ** -0.2
    assert mhx.silverman_bandwidth(0.5, -1.0, 1.0, S) == 0.9 * 0.5 * S ** -0.2
    assert mhx.silverman_bandwidth(0.5, 1.0, 1.0, S) == 0.9 * 0.5 * S ** -0.2         # IQR 0: the std takes its place
    assert mhx.silverman_bandwidth(0.0, 1.0, 1.0, S) == 0.9 * S ** -0.2               # both 0: width 1
    assert mhx.silverman_bandwidth(0.0, 0.0, 0.0, 1) == 0.9


@pytest.mark.parametrize("npoints", [64, 700, 2048])
def test_density_from_counts_within_the_binning_bound_of_the_direct_sum(npoints):
    """every draw moves by at most half a cell, so |binned - exact| <= delta / (2 h^2 sqrt(2 pi e)); on top, the rounding of a float64
    sum of at most 2048 terms: 1e-12 x the largest density"""
    import mhx
    rng = np.random.default_rng(22)
    x = np.concatenate([rng.normal(-2.0, 0.5, size=1500), rng.normal(1.0, 1.0, size=700)])
    S = x.size
    q25, q75 = np.quantile(x, [0.25, 0.75])
    h = mhx.silverman_bandwidth(np.std(x, ddof=1), q25, q75, S)
    e = mhx.histogram_edges(x.min() - 4.0 * h, x.max() + 4.0 * h, npoints)
    counts, outside = histogram_numpy(x, e)
    assert outside.sum() == 0
    grid, dens = mhx.density_from_counts(counts, e, h)
    assert grid.shape == dens.shape == (npoints,) and np.array_equal(grid, 0.5 * (e[:-1] + e[1:]))
    exact = kde_direct(x, grid, h)
    delta = (e[-1] - e[0]) / npoints
    bound = delta / (2.0 * h * h * math.sqrt(2.0 * math.pi * math.e))
    assert bound == mhx.density_binning_bound(e, h)
    err = np.abs(dens - exact).max()
    print("npoints %d: |binned - exact| max %.3e, bound %.3e" % (npoints, err, bound))
    assert err <= bound + 1e-12 * exact.max()
    assert abs(dens.sum() * delta - 1.0) < 1e-3             # a density: the grid reaches 4 h beyond the draws


CT = {"mhx_run *": C.c_void_p, "mhx_ctx *": C.c_void_p, "mhx_group *": C.c_void_p, "const void *": C.c_void_p,
      "const int32_t *": C.POINTER(C.c_int32), "int32_t": C.c_int32, "int64_t": C.c_int64, "const double *": C.POINTER(C.c_double),
      "uint64_t *": C.POINTER(C.c_uint64)}


def test_the_new_entry_points_in_header_mirror_and_library():
    import mhx
    import mhx._lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mhx.h")).read(), flags=re.S)
    protos = {}
    for name, args in re.findall(r"\bint (mhx_\w+)\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S):
        protos[name] = [re.sub(r"\s*\w+$", "", a.strip()).strip() for a in " ".join(args.split()).split(",")]
    lib = mhx.lib()
    one = ["const int32_t *", "int32_t", "const double *", "int32_t", "uint64_t *", "uint64_t *"]
    two = ["const int32_t *", "int32_t", "const double *", "int32_t", "const int32_t *", "int32_t", "uint64_t *", "uint64_t *"]
    tensor = ["const void *", "int64_t", "int32_t", "int64_t"]
    want = {"mhx_run_histogram": ["mhx_run *"] + one, "mhx_ctx_histogram": ["mhx_ctx *"] + tensor + one,
            "mhx_group_histogram": ["mhx_group *"] + one, "mhx_run_histogram2d": ["mhx_run *"] + two,
            "mhx_ctx_histogram2d": ["mhx_ctx *"] + tensor + two, "mhx_group_histogram2d": ["mhx_group *"] + two}
    for name, args in want.items():
        assert name in L.EXPORTS and name in protos and hasattr(lib, name), name
        assert protos[name] == args, (name, protos[name])
        assert list(getattr(lib, name).argtypes) == [CT[t] for t in args], name
    assert (mhx.api.HISTOGRAM_MAX_BINS, mhx.api.HISTOGRAM2D_MAX_BINS) == (2048, 128)
    src = open(os.path.join(ROOT, "advancedmh.jl_amd", "csrc", "mhx_hist_kernels.h")).read()
    assert "#define MHX_HIST_MAX_BINS 2048" in src and "#define MHX_HIST2D_MAX_BINS 128" in src
