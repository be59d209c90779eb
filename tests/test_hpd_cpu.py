"""The host half of the HPD intervals (mhx/api.py: hpd_ranks), the numpy restatement the GPU tests are held to (tests/hpd_ref.py)
against hand-worked examples, and the two new entry points in the header, the ctypes mirror and the library alike.  No device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from hpd_ref import hpd_numpy, hpd_rows, ranks, tail_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hpd_ranks_at_the_boundaries():
    import mhx
    import mhx.api as api
    assert api.hpd_ranks is mhx.hpd_ranks
    # alpha S an exact integer (alpha a binary fraction: the product is exact)
    assert api.hpd_ranks(64, 0.25) == 16 and api.hpd_ranks(100, 0.5) == 50 and api.hpd_ranks(8, 0.125) == 1
    # alpha S just above one, and just above an integer
    assert api.hpd_ranks(21, 0.05) == 2 and api.hpd_ranks(65, 0.25) == 17
    assert api.hpd_ranks(2 ** 20, 1.0 / 2 ** 20 + 2.0 ** -40) == 2
    # m = 1: alpha S below one, and a single draw
    assert api.hpd_ranks(10, 0.05) == 1 and api.hpd_ranks(1, 0.99) == 1 and api.hpd_ranks(10 ** 9, 1e-12) == 1
    # m = S - 1 and m = S
    assert api.hpd_ranks(10, 0.85) == 9 and api.hpd_ranks(455, (455 - 1.5) / 455) == 454 and api.hpd_ranks(10, 0.95) == 10
    # the definition itself, in double, for shapes and alphas the GPU tests use -- no 2^32 limit
    for S in (1, 2, 15, 64, 455, 1000, 2211, 4097, 2 ** 40 + 3):
        for alpha in (0.05, 0.3, 0.5, 0.9, 0.5 / S, (S - 0.5) / S if S > 1 else 0.5):
            assert api.hpd_ranks(S, alpha) == max(1, int(math.ceil(alpha * float(S)))) == ranks(S, alpha)
            assert 1 <= api.hpd_ranks(S, alpha) <= S
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(mhx.ArgumentError, match="hpd: alpha"):
            api.hpd_ranks(10, bad)
    with pytest.raises(mhx.ArgumentError, match="hpd: no draws"):
        api.hpd_ranks(0, 0.05)


def test_restatement_on_hand_worked_examples():
    # S = 6, alpha = 0.34: m = ceil(2.04) = 3; a = [0, 5, 6], b = [7, 8, 20]; widths [7, 3, 14] -> i = 1
    x = np.array([8.0, 0.0, 20.0, 6.0, 5.0, 7.0])
    assert ranks(6, 0.34) == 3 and hpd_numpy(x, 0.34) == (5.0, 8.0)
    assert hpd_numpy(x.astype(np.float32), 0.34) == (5.0, 8.0)
    # ties: S = 8, alpha = 0.5: m = 4; a = [1, 1, 2, 2], b = [2, 3, 3, 9]; widths [1, 2, 1, 7] -> the FIRST minimum, i = 0
    t = np.array([3.0, 1.0, 2.0, 9.0, 2.0, 1.0, 3.0, 2.0])
    assert hpd_numpy(t, 0.5) == (1.0, 2.0)
    assert tail_counts(t, 0.5) == (4, 2, 3)                 # y = 1 1 2 2 2 3 3 9: tL = y[3] = 2, two below; tU = y[4] = 2, three above
    # m = 1: the whole range; m = S: every width is zero, the first candidate wins
    assert hpd_numpy(x, 0.1) == (0.0, 20.0) and hpd_numpy(x, 0.99) == (0.0, 0.0)
    # a NaN width (inf - inf) is smaller than every number: S = 5, m = 3, a = [1, 2, inf], b = [inf, inf, inf]
    assert hpd_numpy([np.inf, 1.0, np.inf, 2.0, np.inf], 0.5) == (np.inf, np.inf)
    lo, up = hpd_rows(np.array([[[1.0, 4.0], [np.nan, 1.0]], [[2.0, 8.0], [0.0, 1.0]]]), 0.5)      # [N = 2][d1 = 2][C = 2]
    assert (lo[0], up[0]) == (1.0, 4.0) and np.isnan(lo[1]) and np.isnan(up[1])


CT = {"mhx_run *": C.c_void_p, "mhx_ctx *": C.c_void_p, "const void *": C.c_void_p, "const int32_t *": C.POINTER(C.c_int32),
      "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "double *": C.POINTER(C.c_double)}


def test_the_new_entry_points_in_header_mirror_and_library():
    import mhx
    import mhx._lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mhx.h")).read(), flags=re.S)
    protos = {}
    for name, args in re.findall(r"\bint (mhx_\w+)\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S):
        protos[name] = [re.sub(r"\s*\w+$", "", a.strip()).strip() for a in " ".join(args.split()).split(",")]
    lib = mhx.lib()
    for name in ("mhx_run_hpd", "mhx_ctx_hpd"):
        assert name in L.EXPORTS and name in protos and hasattr(lib, name)
        assert list(getattr(lib, name).argtypes) == [CT[t] for t in protos[name]], (name, protos[name])
    assert protos["mhx_run_hpd"] == ["mhx_run *", "const int32_t *", "int32_t", "double", "double *", "double *"]
    assert protos["mhx_ctx_hpd"] == ["mhx_ctx *", "const void *", "int64_t", "int32_t", "int64_t", "const int32_t *", "int32_t", "double",
                                     "double *", "double *"]
    assert "HPD_SCRATCH_MB" in open(os.path.join(ROOT, "include", "mhx.h")).read()
