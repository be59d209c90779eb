#!/usr/bin/env python3
"""Rate of the derived-quantity map (mhx_run_derive) on the tensor bench.py's flagship workload leaves on the
device: C2 -- RWMH on the 100-dim isotropic Gaussian, 65 536 chains, 250 saved draws each, [250][101][65536] -- in fp64 and fp32.

Three maps, each at 1, 2, 4 and 8 draws per lane (option DERIVE_DRAWS; the library's default is marked):
  identity   2 rows in, 2 out:    y0 = x0, y1 = x1
  sumsq      100 rows in, 1 out:  y0 = x0^2 + ... + x99^2
  explog     2 rows in, 1 out:    y0 = exp(x0) + log(|x1| + 1)
Per form: the KERNEL time of the map's one launch from HIP events (mhx_run_stats.kernel_ms of the derived run), median over REPEATS
rounds in which the forms alternate, with minimum and maximum; the algorithmic bytes -- (rows named + lp) read and (nout + 1) rows
written, each n_saved x nchains reals --; the rate bytes / time; and, as the yardstick, hipMemcpyDtoDAsync of bytes / 2 in the same
process and the same rounds (a copy of n bytes reads n and writes n: the same bytes cross the memory interface), from HIP events
too.  `of_copy` = the map's rate over the copy's.
Last, once per width: the wall time of chain.derive(identity).describe() -- map, tensor of 3 rows to the host, the two tables with ESS
and R-hat on the device -- against run.samples() + numpy (the whole tensor to the host, then mean, std and the five quantiles of the
two rows: no ESS, no R-hat), same process.
Nothing here gates anything: the tests do.

    derive_rate.py [OUT.json]        default OUT: profiles/derive_rate.json      env: C, INNER, REPEATS, E2E=0 skips the last part"""
import ctypes as C_
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402
import mhx.trace as T  # noqa: E402

D, C, INNER, REPEATS = 100, int(os.environ.get("C", 65536)), int(os.environ.get("INNER", 250)), int(os.environ.get("REPEATS", 7))
DRAWS = (1, 2, 4, 8)
DEFAULT_DRAWS = 4
MAPS = {
    "identity": (lambda t: [t[0], t[1]], 2),
    "sumsq": (lambda t: sum(t[k] * t[k] for k in range(D)), D),
    "explog": (lambda t: T.exp(t[0]) + T.log(abs(t[1]) + 1.0), 2),
}

hip = C_.CDLL("libamdhip64.so")
hip.hipMalloc.argtypes = [C_.POINTER(C_.c_void_p), C_.c_size_t]
hip.hipFree.argtypes = [C_.c_void_p]
hip.hipMemcpyDtoDAsync.argtypes = [C_.c_void_p, C_.c_void_p, C_.c_size_t, C_.c_void_p]
hip.hipEventCreate.argtypes = [C_.POINTER(C_.c_void_p)]
hip.hipEventRecord.argtypes = [C_.c_void_p, C_.c_void_p]
hip.hipEventSynchronize.argtypes = [C_.c_void_p]
hip.hipEventElapsedTime.argtypes = [C_.POINTER(C_.c_float), C_.c_void_p, C_.c_void_p]


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: hipError %d" % (what, rc))


def copy_ms(dst, src, nbytes, ev):
    _ok(hip.hipEventRecord(ev[0], None), "hipEventRecord")
    _ok(hip.hipMemcpyDtoDAsync(dst, src, nbytes, None), "hipMemcpyDtoDAsync")
    _ok(hip.hipEventRecord(ev[1], None), "hipEventRecord")
    _ok(hip.hipEventSynchronize(ev[1]), "hipEventSynchronize")
    ms = C_.c_float()
    _ok(hip.hipEventElapsedTime(C_.byref(ms), ev[0], ev[1]), "hipEventElapsedTime")
    return float(ms.value)


def stat(t):
    t = np.array(t)
    return dict(ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))


def measure(dt, e2e):
    s = float(np.float32(2.38 / D ** 0.5))
    ctx = mhx.Context.default(dtype=dt)
    run = mhx.Run(mhx.DensityModel(mhx.IsoGaussian(D)), mhx.RWMH(mhx.MvNormal(mhx.zeros(D), s * s * mhx.I)), nchains=C, seed=0xC0FFEE,
                  ctx=ctx, reduce_lanes=2)
    run.init(None)
    run.sample(INNER, 1, 1, 0)
    size = 8 if dt == "f64" else 4
    row_bytes = INNER * C * size
    traced = {k: T.trace_map(f, D) for k, (f, _) in MAPS.items()}
    nbytes = {k: (MAPS[k][1] + 1 + traced[k].nout + 1) * row_bytes for k in MAPS}

    def derive_ms(name, u):
        ctx.set_option("DERIVE_DRAWS", u)
        try:
            der = run.derive(traced[name])
        finally:
            ctx.set_option("DERIVE_DRAWS", None)
        ms = der.stats()["kernel_ms"]
        der.close()
        return ms

    src, n_saved = C_.c_void_p(), C_.c_int64()
    mhx.check(mhx.lib().mhx_run_device_samples(run.h, C_.byref(src), None, C_.byref(n_saved)))
    dst = C_.c_void_p()
    _ok(hip.hipMalloc(C_.byref(dst), max(nbytes.values()) // 2), "hipMalloc")
    ev = [C_.c_void_p(), C_.c_void_p()]
    for e in ev:
        _ok(hip.hipEventCreate(C_.byref(e)), "hipEventCreate")
    forms = {}
    for name in MAPS:
        for u in DRAWS:
            forms["%s_u%d" % (name, u)] = lambda name=name, u=u: derive_ms(name, u)
        forms["copy_%s" % name] = lambda name=name: copy_ms(dst, src, nbytes[name] // 2, ev)
    # the maps compute what numpy computes: a few chains of the default form of each, before anything is timed
    host = None
    if C * INNER <= 1 << 22:
        host = run.samples(want_accepted=False)[0].astype(np.float64)
    for f in forms.values():                                # warm-up: every module compiled and loaded
        f()
    times = {k: [] for k in forms}
    for _ in range(REPEATS):
        for k, f in forms.items():
            times[k].append(f())
    out = dict(row_bytes=row_bytes, maps={})
    for name in MAPS:
        cp = stat(times["copy_%s" % name])
        cp.update(bytes=nbytes[name], TBps=nbytes[name] / (cp["ms"] * 1e-3) / 1e12)
        m = dict(rows_in=MAPS[name][1], rows_out=traced[name].nout, bytes=nbytes[name], copy=cp, draws={})
        for u in DRAWS:
            st = stat(times["%s_u%d" % (name, u)])
            st.update(TBps=nbytes[name] / (st["ms"] * 1e-3) / 1e12)
            st["of_copy"] = st["TBps"] / cp["TBps"]
            m["draws"][str(u)] = st
        out["maps"][name] = m
    if host is not None:                                    # (small shapes only: a rehearsal's check of the whole path)
        der = run.derive(traced["sumsq"])
        got = der.samples()[0]
        der.close()
        assert np.allclose(got[:, 0, :], (host[:, :D, :] ** 2).sum(axis=1), rtol=1e-4 if dt == "f32" else 1e-12)
    if e2e:
        names = ["x%d" % k for k in range(D)] + ["lp"]
        chain = mhx.Chains(np.empty((INNER, 0, 0), dtype=run.real), names, 1, 1, state=run)
        t0 = time.perf_counter()
        dch = chain.derive(MAPS["identity"][0], names=["x0", "x1"])
        text = dch.describe()
        t_dev = time.perf_counter() - t0
        dch.state.close()
        t0 = time.perf_counter()
        value = run.samples(want_accepted=False)[0]
        t_copy = time.perf_counter() - t0
        rows = [value[:, k, :].astype(np.float64).ravel() for k in (0, 1)]
        table = [(r.mean(), r.std(ddof=1), np.quantile(r, [0.025, 0.25, 0.5, 0.75, 0.975])) for r in rows]
        t_host = time.perf_counter() - t0
        del value, rows
        out["end_to_end"] = dict(derive_describe_s=t_dev, samples_numpy_s=t_host, of_which_samples_s=t_copy, speedup=t_host / t_dev,
                                 describe_lines=len(text.splitlines()), numpy_means=[float(t[0]) for t in table])
    hip.hipFree(dst)
    run.close()
    print(json.dumps({dt: out}), flush=True)
    return out


def main(out):
    result = dict(dim=D, nchains=C, saved_draws=INNER, repeats=REPEATS, default_draws_per_lane=DEFAULT_DRAWS,
                  unit="kernel milliseconds from HIP events; bytes = (rows named + lp + nout + 1) x n_saved x nchains x sizeof(real); "
                       "copy = hipMemcpyDtoDAsync of bytes / 2")
    for dt in ("f64", "f32"):
        result[dt] = measure(dt, os.environ.get("E2E", "1") != "0")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "derive_rate.json"))
