"""A map of the draws (MHX_DERIVED source: mhx_run_derive) compiled for the host the way
tests/user_targets.py compiles a log-density -- g++, -ffp-contract=off, log and exp from the oracle -- and applied to a whole tensor:
the expected derived tensor in the engine's own arithmetic, bit for bit."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

import user_targets

ROOT = user_targets.ROOT

_HOST_FRAME = r"""
#define MHX_DERIVED(x, y, d, data, ndata) \
    template <class MHX_X, class MHX_Y> static inline void mhx_user_derived(const MHX_X& x, const MHX_Y& y, const int d, const mhx_real* data, const int ndata)
// one draw of one chain: x[k] is row k (clamped to [0, d] as on the device), y.set(j, v) output j < K
struct host_draw {
    const mhx_real* p; long ld; int d;
    mhx_real operator[](int k) const { const int kk = k < 0 ? 0 : (k > d ? d : k); return p[(long)kk * ld]; }
};
struct host_out {
    mhx_real* p; int K;
    void set(int j, mhx_real v) const { if ((unsigned)j < (unsigned)K) p[j] = v; }
};
"""

_HOST_LOOP = r"""
// src [N][d + 1][C] -> dst [N][K + 1][C]: the outputs (NaN where the map sets none), then the lp row
extern "C" void derive_tensor(const mhx_real* src, mhx_real* dst, long N, int d, long C, int K, const mhx_real* data, int ndata)
{
    mhx_real y[512];
    for (long t = 0; t < N; ++t)
        for (long c = 0; c < C; ++c) {
            for (int j = 0; j < K; ++j) y[j] = MHX_NAN;
            const host_draw x = {src + t * (long)(d + 1) * C + c, C, d};
            const host_out o = {y, K};
            mhx_user_derived(x, o, d, data, ndata);
            for (int j = 0; j < K; ++j) dst[(t * (long)(K + 1) + j) * C + c] = y[j];
            dst[(t * (long)(K + 1) + K) * C + c] = x[d];
        }
}
"""


def host_map(oracle, source, cache_dir=os.path.join(ROOT, "oracle", "_user_targets")):
    """fn(tensor [N][d + 1][C], nout, data=None) -> [N][nout + 1][C] in the oracle's current width"""
    oracle.build()
    os.makedirs(cache_dir, exist_ok=True)
    f64 = oracle.get_dtype() == "f64"
    text = user_targets._PRELUDE + _HOST_FRAME + source + _HOST_LOOP
    tag = hashlib.sha1(text.encode()).hexdigest()[:16] + ("_f64" if f64 else "_f32")
    so = os.path.join(cache_dir, "derived_%s.so" % tag)
    if not os.path.exists(so):
        cpp = os.path.join(cache_dir, "derived_%s.cpp" % tag)
        open(cpp, "w").write(text)
        odir = os.path.join(ROOT, "oracle")
        tmp = "%s.%d.tmp" % (so, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                               "-mfma", "-mavx2", "-DMHX_REAL64=%d" % (1 if f64 else 0), "-o", tmp, cpp, "-L" + odir,
                               "-lmhx_oracle64" if f64 else "-lmhx_oracle", "-Wl,-rpath," + odir])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.derive_tensor.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_long, C.c_int, C.c_void_p, C.c_int]
    lib.derive_tensor.restype = None
    R = np.float64 if f64 else np.float32

    def fn(tensor, nout, data=None):
        x = np.ascontiguousarray(tensor, dtype=R)
        assert x.ndim == 3 and 1 <= nout <= 512
        N, d1, nch = x.shape
        out = np.empty((N, nout + 1, nch), dtype=R)
        dat = None if data is None else np.ascontiguousarray(data, dtype=R).ravel()
        lib.derive_tensor(x.ctypes.data, out.ctypes.data, N, d1 - 1, nch, nout, None if dat is None else dat.ctypes.data,
                          0 if dat is None else dat.size)
        return out

    fn._keep = lib
    return fn
