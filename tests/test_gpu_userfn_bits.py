"""GPU: the four statistics that compile a caller's text -- derive, predict, pointwise, psis -- bit for bit against
tests/golden/userfn_bits.json, on tensors made on the host.

The file pins the DOCUMENTED ORDER OF OPERATIONS of these kernels (csrc/mhx_pointwise_kernels.h, mhx_psis_kernels.h,
mhx_derive_kernels.h; DESIGN.md sections 6.5.5 - 6.5.8): which draws a lane sums, the butterfly over the wave, the waves in wave order,
the partials in index order, the fit's lane-strided sums.  It was recorded with the library as it stood before the shared frame of these
kernels was factored out, and it is regenerated only by a change that MEANS to alter that order:

    python tests/test_gpu_userfn_bits.py --record        (MHX_LIB=<another build's libmhx.so> records with that build)

Inputs (seeded numpy generator, uploaded with hipMemcpy and passed to the mhx_ctx_* forms; no sampler): d = 2; N = 37 saved draws (a
ragged last strip of 16 and a ragged last group of 4); C = 1, 65, 257 (one lane, a partial second wave, a partial second block); 5 data
rows of 3 reals (a ragged last tile at every tile size); a data block of 1 real; in data row 3 one draw gives l = -inf and one gives NaN.
Recorded per (width, C) as hex floats: the pointwise out5 and shift; the PSIS out8, T, M and the tails at reff = 1 (M = 7, 148, 293).
The derived tensor (two outputs) and the predictive tensor (one Normal and one Gamma draw, seed 0xC0FFEE) are up to 28 527 reals each --
as hex floats they alone would make the file some 2 MB --, so they are recorded as the SHA-256 of their bytes, which is equality to the
last bit, beside the hex floats of the first and last draw of chain 0 and of the last chain for a readable difference.

Pointwise is also asserted to give the recorded bits at every POINTWISE_ROWS in {2, 4, 8, 16}: at these shapes the three strips of a
chain block go to three slots whatever the tile is, so the order of every sum is the same."""
import ctypes as C
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "userfn_bits.json")
N, D, NROWS, ROWLEN = 37, 2, 5, 3
CHAINS = (1, 65, 257)
SEED = 0xC0FFEE
PSIS_COLS = ("elpd_loo", "khat", "sigma", "tau", "lmin", "body", "n_below", "bad")

# l = -data[0] (r[0] - x[0])^2 / 2 + r[1] log(x[1] - r[2]): -inf where x[1] == r[2], NaN where x[1] < r[2]
SRC_POINTWISE = """
MHX_POINTWISE(x, r, m, d, data, ndata)
{
    const mhx_real z = r[0] - x[0];
    return mhx_fma(r[1], mhx_log(x[d - 1] - r[m - 1]), MHX_R(-0.5) * data[0] * z * z);
}
"""
SRC_DERIVED = """
MHX_DERIVED(x, y, d, data, ndata)
{
    y.set(0, mhx_fma(x[0], x[0], data[0]));
    y.set(1, mhx_exp(x[0]) + mhx_log(x[1]));
}
"""
# mhx.trace_predictive of [Normal(x0, |x1| + 1/2), Gamma(5/2, |x0| + 1/2)], kept as text so that the tracer may change
SRC_PREDICTIVE = """
MHX_PREDICTIVE(x, rng, y, d, data, ndata)
{
    const mhx_real t1 = x[0];
    const mhx_real t2 = x[1];
    const mhx_real t3 = mhx_abs(t2);
    const mhx_real t5 = t3 + MHX_R(0x1.0000000000000p-1);
    const mhx_real t6 = mhx_abs(t1);
    const mhx_real t7 = t6 + MHX_R(0x1.0000000000000p-1);
    const mhx_real t8 = rng.draw(0, 0, t1, t5);
    const mhx_real t10 = rng.gamma(1, 5, MHX_R(0x1.4000000000000p+1), t7, MHX_RW(0x1.1555555555555p+1, 0x1.1555560000000p+1), MHX_RW(0x1.cfc7da32a9212p-3, 0x1.cfc7da0000000p-3), MHX_RW(0x1.999999999999ap-2, 0x1.99999a0000000p-2));
    y.set(0, t8);
    y.set(1, t10);
}
"""


def _inputs(real, nch):
    """x [N][3][C]: x0 ~ N(0.1, 0.5^2), x1 ~ U(2, 6), an lp row; rows (y, a, b) with b < 2 except row 3, whose b = 1.5 meets one planted
    x1 = 1.5 (-inf) and one planted x1 = 1.0 (NaN); data = (0.75)"""
    dt = np.float64 if real == "f64" else np.float32
    rng = np.random.default_rng(1000 + nch)
    x = np.zeros((N, D + 1, nch))
    x[:, 0, :] = rng.normal(0.1, 0.5, size=(N, nch))
    x[:, 1, :] = rng.uniform(2.0, 6.0, size=(N, nch))
    x[:, 2, :] = rng.normal(-3.0, 1.0, size=(N, nch))
    x[5, 1, nch - 1] = 1.5
    x[33, 1, nch // 2] = 1.0
    rows = np.stack([rng.normal(0.0, 1.0, NROWS), rng.uniform(0.5, 2.0, NROWS), rng.uniform(-1.0, 0.5, NROWS)], axis=1)
    rows[3, 2] = 1.5
    return np.ascontiguousarray(x.astype(dt)), np.ascontiguousarray(rows.astype(dt)), np.array([0.75], dtype=dt)


class _Device:
    """a device copy of a host array, freed on exit"""
    hip = None

    def __init__(self, a):
        if _Device.hip is None:
            hip = _Device.hip = C.CDLL("libamdhip64.so")
            hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            hip.hipFree.argtypes = [C.c_void_p]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.p = C.c_void_p()
        assert _Device.hip.hipMalloc(C.byref(self.p), a.nbytes) == 0
        assert _Device.hip.hipMemcpy(self.p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0

    def __enter__(self):
        return self.p

    def __exit__(self, *exc):
        _Device.hip.hipFree(self.p)


def _tensor_of(mhx, h, shape, dtype):
    """the sample tensor of the derived run `h`, copied to the host; the run is destroyed"""
    try:
        ptr, n = C.c_void_p(), C.c_int64()
        mhx.check(mhx.lib().mhx_run_device_samples(h, C.byref(ptr), None, C.byref(n)))
        assert n.value == shape[0]
        out = np.empty(shape, dtype=dtype)
        assert _Device.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), ptr, out.nbytes, 2) == 0
        return out
    finally:
        mhx.lib().mhx_run_destroy(h)


def _hex(a):
    """the values as hex floats in one string; the mantissa's trailing zeros are dropped (float.fromhex gives the same bits back)"""
    return " ".join(re.sub(r"\.?0*p", "p", float(v).hex()) for v in np.asarray(a, dtype=np.float64).ravel())


def _tensor_record(t):
    ends = [0, t.shape[2] - 1] if t.shape[2] > 1 else [0]                        # chain 0 and the last chain
    return dict(sha256=hashlib.sha256(t.tobytes()).hexdigest(), first_draw=_hex(t[0][:, ends]), last_draw=_hex(t[-1][:, ends]))


def _pointwise(mhx, ctx, ptr, nch, rows, data):
    out, sh, T_ = np.full((5, NROWS), 77.0), np.full(NROWS, 123.0), C.c_int64(-1)
    dp = C.POINTER(C.c_double)
    mhx.check(mhx.lib().mhx_ctx_pointwise(ctx.h, ptr, N, D + 1, nch, SRC_POINTWISE.encode(), mhx._lib.rptr(rows), NROWS, ROWLEN, mhx._lib.rptr(data),
                                          data.size, 0, sh.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(T_)))
    assert T_.value == N * nch
    return dict(out5=_hex(out), shift=_hex(sh))


def compute(mhx, real, nch):
    """the record of one (width, C): every statistic on the same tensor, through the mhx_ctx_* forms"""
    x, rows, data = _inputs(real, nch)
    ctx = mhx.Context(0, real)
    dp = C.POINTER(C.c_double)
    lib = mhx.lib()
    try:
        with _Device(x) as ptr:
            rec = dict(pointwise=_pointwise(mhx, ctx, ptr, nch, rows, data), pointwise_rows={})
            for tile in (2, 4, 8, 16):
                ctx.set_option("POINTWISE_ROWS", str(tile))
                rec["pointwise_rows"][str(tile)] = _pointwise(mhx, ctx, ptr, nch, rows, data)
            ctx.set_option("POINTWISE_ROWS", None)
            T_, M_ = C.c_int64(-1), C.c_int64(-1)
            M = min(int(0.2 * N * nch), int(np.ceil(3.0 * np.sqrt(N * nch))))
            out8, tails = np.full((8, NROWS), 77.0), np.full((NROWS, M), 55.0)
            mhx.check(lib.mhx_ctx_psis(ctx.h, ptr, N, D + 1, nch, SRC_POINTWISE.encode(), mhx._lib.rptr(rows), NROWS, ROWLEN, mhx._lib.rptr(data),
                                       data.size, 1.0, out8.ctypes.data_as(dp), tails.ctypes.data_as(dp), C.byref(T_), C.byref(M_)))
            assert M_.value == M >= 5 and T_.value == N * nch
            rec["psis"] = dict(out8=_hex(out8), tails=_hex(tails), T=int(T_.value), M=int(M_.value))
            h = C.c_void_p()
            mhx.check(lib.mhx_ctx_derive(ctx.h, ptr, N, D + 1, nch, SRC_DERIVED.encode(), 2, mhx._lib.rptr(data), data.size, C.byref(h)))
            rec["derive"] = _tensor_record(_tensor_of(mhx, h, (N, 3, nch), x.dtype))
            h = C.c_void_p()
            mhx.check(lib.mhx_ctx_predict(ctx.h, ptr, N, D + 1, nch, 0, SRC_PREDICTIVE.encode(), 2, None, 0, SEED, C.byref(h)))
            rec["predict"] = _tensor_record(_tensor_of(mhx, h, (N, 3, nch), x.dtype))
    finally:
        ctx.close()
    return rec


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("nch", CHAINS)
def test_bits_match_the_recorded_order_of_operations(mhx, real, golden, nch):
    want = golden[real][str(nch)]
    got = compute(mhx, real, nch)
    # one draw of -inf and one of NaN in row 3: counted, sumexp NaN; the PSIS row is NaN with bad = 2
    bad = [float.fromhex(v) for v in want["pointwise"]["out5"].split()][4 * NROWS:]
    assert bad == [0.0, 0.0, 0.0, 2.0, 0.0] and float.fromhex(want["psis"]["out8"].split()[7 * NROWS + 3]) == 2.0
    for tile, rec in got["pointwise_rows"].items():
        assert rec == want["pointwise"], ("POINTWISE_ROWS", tile)
    for stat in ("pointwise", "psis", "derive", "predict"):
        for k in want[stat]:
            assert got[stat][k] == want[stat][k], (real, nch, stat, k)
        assert set(got[stat]) == set(want[stat])


def record(path=GOLDEN):
    sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "advancedmh.jl_amd")]
    import mhx
    out = {}
    for real in ("f32", "f64"):
        out[real] = {}
        for nch in CHAINS:
            rec = compute(mhx, real, nch)
            assert all(r == rec["pointwise"] for r in rec.pop("pointwise_rows").values()), "pointwise differs between tiles"
            out[real][str(nch)] = rec
    with open(path, "w") as f:                                                  # one line per (width, C, statistic)
        f.write("{\n" + ",\n".join(' "%s": {\n%s\n }' % (real, ",\n".join('  "%s": {\n%s\n  }' % (
            nch, ",\n".join('   "%s": %s' % (stat, json.dumps(rec, sort_keys=True)) for stat, rec in sorted(cases[nch].items())))
            for nch in sorted(cases, key=int))) for real, cases in sorted(out.items())) + "\n}\n")
    print("recorded %s with %s" % (path, mhx._lib._lib_path))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--record"]:
        record(*sys.argv[2:3])
    else:
        sys.exit("usage: test_gpu_userfn_bits.py --record [OUT.json]")
