"""The pointwise log-likelihood sums of mhx_run_pointwise (include/mhx.h) from first principles.

The same MHX_POINTWISE text is compiled for the host the way tests/derived_ref.py compiles a map -- g++, -ffp-contract=off, log and exp
from the oracle -- and looped over draws and rows: the matrix l[i, s] in the engine's own arithmetic, bit for bit, widened to float64.
From it, in numpy's 80-bit longdouble (as acf_ref.py and diag_ref.py), the five arrays, the derived columns, and for each a running
error bound of the DEVICE's computation, derived here from its order of operations and not tuned to it:

  u = 2^-53 in both widths (every accumulator is fp64).  L = the longest chain of operations one term can pass through: the draws of
  one lane (at most N), 6 butterfly steps over the wave, 3 merges over the block's waves, and the partials of a row merged one after the
  other (at most ceil(C / 256) x 64 of them, the cap of mhx_pointwise_kernels.h).
  sumexp  a term enters as exp(-(|l - m|)) for a running maximum m: the subtraction rounds once (u |l - m| in the argument is a relative
          u |l - m| in the value) and the engine's exp is within 0.90 ulp, so (0.90 + D) u with D = max - min of the
          row's finite l, capped at 746 (beyond it both the engine's exp and the true value are below 2^-1075).  Every later step either adds
          (one rounding) or rescales by such an exp and adds (one rounding and (0.90 + D) u more).  All terms are positive, so
          |error| <= gamma_{L + 1}((1.90 + D) u) x sumexp, plus T x 2^-1021 for terms in the subnormal range.
  s1      y = l - shift rounds once, then L additions: gamma_{L + 1}(u) x sum |y|.
  s2      y^2 carries 2 u from y, the fma rounds once, then L additions: gamma_{L + 3}(u) x sum y^2.
  lppd    max is exact; log is 1-Lipschitz in relative terms: -log1p(-e_sumexp / sumexp); plus the host's float64 roundings, 4 u of the
          magnitudes added.
  var     (s2 - s1^2 / n) / (n - 1): (e_s2 + (2 |s1| e_s1 + e_s1^2) / n) / (n - 1) -- the cancellation is in the bound through the
          magnitudes of s2 and s1^2 / n, not of their difference -- plus 4 u (|s2| + s1^2 / n) / (n - 1) for the host's roundings.
  elpd    the sum of the two, plus u of the magnitudes.
Comparisons run at diag_ref.MARGIN x bound."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

import diag_ref
import user_targets

ROOT = user_targets.ROOT
LD = np.longdouble
U = LD(2) ** -53
MARGIN = diag_ref.MARGIN
THREADS, MAX_SLOTS = 256, 64            # MHX_POINTWISE_THREADS, MHX_POINTWISE_MAX_SLOTS

_HOST_FRAME = r"""
#define MHX_POINTWISE(x, r, m, d, data, ndata) \
    template <class MHX_X, class MHX_ROW> static inline mhx_real mhx_user_pointwise(const MHX_X& x, const MHX_ROW& r, const int m, const int d, const mhx_real* data, const int ndata)
struct host_draw {
    const mhx_real* p; long ld; int d;
    mhx_real operator[](int k) const { const int kk = k < 0 ? 0 : (k > d ? d : k); return p[(long)kk * ld]; }
};
struct host_row {
    const mhx_real* p; int m;
    mhx_real operator[](int j) const { return p[j < 0 ? 0 : (j >= m ? m - 1 : j)]; }
};
"""

_HOST_LOOP = r"""
// src [N][d + 1][C], rows [nrows][rowlen] -> out [nrows][N * C] doubles, draw s = t * C + c
extern "C" void pointwise_matrix(const mhx_real* src, long N, int d, long C, const mhx_real* rows, long nrows, int rowlen,
                                 const mhx_real* data, int ndata, double* out)
{
    for (long i = 0; i < nrows; ++i) {
        const host_row r = {rows + i * rowlen, rowlen};
        for (long t = 0; t < N; ++t)
            for (long c = 0; c < C; ++c) {
                const host_draw x = {src + t * (long)(d + 1) * C + c, C, d};
                out[(i * N + t) * C + c] = (double)mhx_user_pointwise(x, r, rowlen, d, data, ndata);
            }
    }
}
"""


def host_matrix(oracle, source, cache_dir=os.path.join(ROOT, "oracle", "_user_targets")):
    """fn(tensor [N][d + 1][C], rows [nrows][rowlen], data=None) -> l [nrows][N * C] float64 (the oracle's current width, widened)"""
    oracle.build()
    os.makedirs(cache_dir, exist_ok=True)
    f64 = oracle.get_dtype() == "f64"
    text = user_targets._PRELUDE + _HOST_FRAME + source + _HOST_LOOP
    tag = hashlib.sha1(text.encode()).hexdigest()[:16] + ("_f64" if f64 else "_f32")
    so = os.path.join(cache_dir, "pointwise_%s.so" % tag)
    if not os.path.exists(so):
        cpp = os.path.join(cache_dir, "pointwise_%s.cpp" % tag)
        open(cpp, "w").write(text)
        odir = os.path.join(ROOT, "oracle")
        tmp = "%s.%d.tmp" % (so, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                               "-mfma", "-mavx2", "-DMHX_REAL64=%d" % (1 if f64 else 0), "-o", tmp, cpp, "-L" + odir,
                               "-lmhx_oracle64" if f64 else "-lmhx_oracle", "-Wl,-rpath," + odir])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.pointwise_matrix.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_long, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.pointwise_matrix.restype = None
    R = np.float64 if f64 else np.float32

    def fn(tensor, rows, data=None):
        x = np.ascontiguousarray(tensor, dtype=R)
        rr = np.ascontiguousarray(rows, dtype=R)
        rr = rr.reshape(rr.shape[0], -1)
        N, d1, nch = x.shape
        out = np.empty((rr.shape[0], N * nch), dtype=np.float64)
        dat = None if data is None else np.ascontiguousarray(data, dtype=R).ravel()
        lib.pointwise_matrix(x.ctypes.data, N, d1 - 1, nch, rr.ctypes.data, rr.shape[0], rr.shape[1],
                             None if dat is None else dat.ctypes.data, 0 if dat is None else dat.size, out.ctypes.data)
        return out

    fn._keep = lib
    return fn


def gamma(k, u):
    ku = LD(k) * LD(u)
    assert ku < LD(0.5)
    return ku / (1 - ku)


def chain_length(N, nch):
    """L of the module's text for a tensor of N draws x nch chains"""
    return int(N) + 6 + 3 + ((int(nch) + THREADS - 1) // THREADS) * MAX_SLOTS


def sums(l, N, nch, shift=None):
    """dict of the five arrays and the shift (float64, as the device returns them: max and shift exact) and their longdouble values
    and bounds, from l [nrows][N * nch] float64.  shift None: l[i, 0] where finite, else 0 (draw 0 of chain 0 is s = 0)."""
    l = np.asarray(l, dtype=np.float64)
    nrows, T = l.shape
    assert T == N * nch
    L = chain_length(N, nch)
    if shift is None:
        shift = np.where(np.isfinite(l[:, 0]), l[:, 0], 0.0)
    shift = np.asarray(shift, dtype=np.float64)
    out = {k: np.zeros(nrows, dtype=LD) for k in ("sumexp", "s1", "s2", "e_sumexp", "e_s1", "e_s2")}
    out["max"], out["bad"], out["shift"], out["T"] = np.zeros(nrows), np.zeros(nrows), shift, T
    with np.errstate(all="ignore"):
        for i in range(nrows):
            li = l[i]
            fin = np.isfinite(li)
            out["bad"][i] = float(T - int(fin.sum()))
            poisoned = bool(np.any(np.isnan(li) | (li == np.inf)))
            lf = li[fin].astype(LD)
            y = lf - LD(shift[i])
            out["s1"][i], out["s2"][i] = y.sum(), (y * y).sum()
            out["e_s1"][i] = gamma(L + 1, U) * np.abs(y).sum()
            out["e_s2"][i] = gamma(L + 3, U) * (y * y).sum()
            if poisoned:
                out["max"][i] = np.nan
                out["sumexp"][i] = out["e_sumexp"][i] = LD(np.nan)
            elif lf.size == 0:
                out["max"][i] = -np.inf                     # every l is -inf: sumexp 0, exactly
            else:
                m = li[fin].max()
                out["max"][i] = m
                se = np.exp(lf - LD(m)).sum()
                D = min(float(m - li[fin].min()), 746.0)
                out["sumexp"][i] = se
                out["e_sumexp"][i] = gamma(L + 1, (LD(1.90) + LD(D)) * U) * se + LD(T) * LD(2) ** -1021
    return out


def table(ref):
    """the columns of mhx.pointwise_table in longdouble with their bounds: dict(lppd, mean, var, elpd, e_lppd, e_var, e_elpd)"""
    T = ref["T"]
    n = LD(T) - ref["bad"].astype(LD)
    with np.errstate(all="ignore"):
        mx = ref["max"].astype(LD)
        lppd = mx + np.log(ref["sumexp"]) - np.log(LD(T))
        e_lppd = -np.log1p(-ref["e_sumexp"] / ref["sumexp"]) + 4 * U * (np.abs(mx) + np.abs(np.log(ref["sumexp"])) + np.log(LD(T)))
        s1, s2, e1, e2 = ref["s1"], ref["s2"], ref["e_s1"], ref["e_s2"]
        mean = ref["shift"].astype(LD) + s1 / n
        var = np.where(n >= 2, (s2 - s1 * s1 / n) / (n - 1), LD(np.nan))
        e_var = (e2 + (2 * np.abs(s1) * e1 + e1 * e1) / n) / (n - 1) + 4 * U * (np.abs(s2) + s1 * s1 / n) / (n - 1)
        elpd = lppd - var
        e_elpd = e_lppd + e_var + U * (np.abs(lppd) + np.abs(var))
    return dict(lppd=lppd, mean=mean, var=var, elpd=elpd, e_lppd=e_lppd, e_var=e_var, e_elpd=e_elpd)


def same_bits(a, b):
    """float64 arrays equal bit for bit, NaNs matching NaNs"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def within(got, want, bound, k=MARGIN):
    """(ok, largest |error| / bound): every entry within k x bound of the reference; NaN only where the reference is NaN; an infinite
    reference equalled exactly"""
    got, want, bound = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD), np.asarray(bound, dtype=LD)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False, np.inf
    inf = np.isinf(want)
    if not np.array_equal(got[inf], want[inf]):
        return False, np.inf
    ok = ~nan & ~inf
    if not ok.any():
        return True, 0.0
    err = np.abs(got[ok] - want[ok])
    b = bound[ok]
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, LD(0), np.where(b > 0, err / b, LD(np.inf)))      # (an exact entry has ratio 0 whatever its bound)
    return bool(np.all(err <= k * b)), float(ratio.max())
