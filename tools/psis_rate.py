#!/usr/bin/env python3
"""Time of PSIS-LOO on the device (mhx_run_psis) on the tensor bench.py's flagship workload leaves there: C2 --
RWMH on the 100-dim isotropic Gaussian, 65 536 chains, 250 saved draws each, [250][101][65536] -- in fp64 and fp32, as
tools/pointwise_rate.py times the pointwise pass.

Function: the README's Normal log-likelihood with mu = x[0] and sigma = |x[1]| + 0.5 (pointwise_rate.py says why).  Rows: nrows = 30 and
2 000.  Per (width, nrows): the wall time of the BLOCKING CALL, median of REPEATS rounds in which the forms alternate, with minimum and
maximum; split by phase -- the select passes, the gather, the sort, the fit -- through option PSIS_STOP_AFTER = 1 | 2 | 3 of the tools
build (a second context on the same device tensor, so that the run's own context stays untainted).  The yardstick, in the same rounds:
mhx_run_pointwise at the same shape, which is ONE evaluation sweep; every phase is reported as a multiple of it.  Beside the times: the
registers, waves per SIMD and instruction counts of the three kernels as hipcc emits them for gfx950 from the same source and options.
Nothing here gates anything: the tests do.

    psis_rate.py [OUT.json]        default OUT: profiles/psis_rate.json      env: C, INNER, REPEATS, NROWS (comma-separated)"""
import ctypes
import json
import math
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402
import mhx.trace as T  # noqa: E402

D, C, INNER, REPEATS = 100, int(os.environ.get("C", 65536)), int(os.environ.get("INNER", 250)), int(os.environ.get("REPEATS", 7))
NROWS = tuple(int(n) for n in os.environ.get("NROWS", "30,2000").split(","))
CSRC = os.path.join(ROOT, "advancedmh.jl_amd", "csrc")
LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)
KERNELS = ("mhx_jit_psis_hist", "mhx_jit_psis_gather", "mhx_jit_psis_fit", "mhx_jit_pointwise")


def normal_ll(t, y):
    sigma = abs(t[1]) + 0.5
    return -0.5 * ((y - t[0]) / sigma) ** 2 - T.log(sigma) - LOG_SQRT_2PI


def kernel_table(source, f64):
    """per kernel of the module: VGPRs, SGPRs, LDS bytes, scratch bytes, waves per SIMD and instructions, from the cross-compiler"""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "psis.hip"), os.path.join(tmp, "psis.s")
        open(src, "w").write('#include "mhx_device_math.h"\n' + source + '\n#define MHX_HAVE_POINTWISE 1\n#include "mhx_pointwise_kernels.h"\n'
                             '#define MHX_HAVE_PSIS 1\n#include "mhx_psis_kernels.h"\n')
        cmd = [hipcc, "-x", "hip", "--offload-device-only", "--no-gpu-bundle-output", "-S", "-DMHX_JIT_BUILD=1", "-I" + CSRC,
               "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-DMHX_REAL64=%d" % (1 if f64 else 0),
               "-DMHX_XW_LINE=64", "-DMHX_JIT_PSIS_ROWS=4", "-DMHX_JIT_POINTWISE_ROWS=%d" % (8 if f64 else 4), "-o", out, src]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if done.returncode:
            raise RuntimeError(done.stdout[-2000:])
        text = open(out).read()
    table = {}
    for k in KERNELS:
        body = text[text.index("\n%s:" % k):]
        end = body.index(".end_amdhsa_kernel")
        code, desc, tail = body[:body.index("s_endpgm")], body[body.index("s_endpgm"):end], body[end:end + 4000]
        ins = [x.split()[0] for x in code.split("\n") if x.startswith("\t") and x.strip() and not x.strip().startswith((".", ";"))]
        occ = re.search(r"; Occupancy: (\d+)", tail)
        table[k] = dict(vgprs=int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)),
                        sgprs=int(re.search(r"\.amdhsa_next_free_sgpr (\d+)", desc).group(1)),
                        lds_bytes=int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1)),
                        scratch_bytes=int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)),
                        waves_per_simd=int(occ.group(1)) if occ else None, instructions=len(ins),
                        valu=sum(1 for m in ins if m.startswith("v_")), lds_ops=sum(1 for m in ins if m.startswith("ds_")))
    return table


def stat(t):
    t = np.array(t)
    return dict(ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))


def measure(dt):
    s = float(np.float32(2.38 / D ** 0.5))
    ctx = mhx.Context.default(dtype=dt)
    run = mhx.Run(mhx.DensityModel(mhx.IsoGaussian(D)), mhx.RWMH(mhx.MvNormal(mhx.zeros(D), s * s * mhx.I)), nchains=C, seed=0xC0FFEE,
                  ctx=ctx, reduce_lanes=2)
    run.init(None)
    run.sample(INNER, 1, 1, 0)
    ptr, n = ctypes.c_void_p(), ctypes.c_int64()
    mhx.check(mhx.lib().mhx_run_device_samples(run.h, ctypes.byref(ptr), None, ctypes.byref(n)))
    rng = np.random.default_rng(1234)
    rows = {k: rng.normal(0.0, 1.0, size=k) for k in NROWS}
    traced = {k: T.trace_pointwise(normal_ll, D, rows[k]) for k in NROWS}
    tctx = mhx.Context(0, dt)                                # the phases: a context of its own, which the probe option taints
    dp = ctypes.POINTER(ctypes.c_double)

    def phase_ms(k, stop):
        rr = tctx.arr(rows[k].reshape(-1, 1))
        out = np.zeros((8, k))
        tctx.set_option("PSIS_STOP_AFTER", stop)
        t0 = time.perf_counter()
        mhx.check(mhx.lib().mhx_ctx_psis(tctx.h, ptr, INNER, D + 1, C, traced[k].source.encode(), mhx._lib.rptr(rr), k, 1, None, 0, 1.0,
                                         out.ctypes.data_as(dp), None, None, None))
        return (time.perf_counter() - t0) * 1e3

    def timed(f):
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3

    forms = {}
    for k in NROWS:
        forms["n%d_psis" % k] = lambda k=k: timed(lambda: run.psis(traced[k]))
        forms["n%d_pointwise" % k] = lambda k=k: timed(lambda: run.pointwise(traced[k]))
        for stop in (1, 2, 3, 0):
            forms["n%d_stop%d" % (k, stop)] = lambda k=k, stop=stop: phase_ms(k, stop)
    for name, f in forms.items():                           # warm-up: every module compiled and loaded, the scratch grown
        print("# %s warm-up %s" % (dt, name), file=sys.stderr, flush=True)
        f()
    times = {k: [] for k in forms}
    for rnd in range(REPEATS):
        print("# %s round %d" % (dt, rnd), file=sys.stderr, flush=True)
        for k, f in forms.items():
            times[k].append(f())
    draws = INNER * C
    out = dict(draws=draws, tail=mhx.psis_tail_length(draws), key_passes=6 if dt == "f64" else 3, rows={})
    for k in NROWS:
        call, sweep = stat(times["n%d_psis" % k]), stat(times["n%d_pointwise" % k])
        med = {s_: float(np.median(times["n%d_stop%d" % (k, s_)])) for s_ in (1, 2, 3, 0)}
        ph = dict(select=med[1], gather=med[2] - med[1], sort=med[3] - med[2], fit=med[0] - med[3], call_of_the_tools_build=med[0])
        res = run.psis(traced[k])
        out["rows"][str(k)] = dict(call=call, pointwise_call=sweep, call_over_pointwise=call["ms"] / sweep["ms"], phases_ms=ph,
                                   phases_over_pointwise={p: ph[p] / sweep["ms"] for p in ("select", "gather", "sort", "fit")},
                                   select_pass_over_pointwise=ph["select"] / out["key_passes"] / sweep["ms"],
                                   evals_per_s_of_a_select_pass=draws * k / (ph["select"] / out["key_passes"] * 1e-3),
                                   evals_per_s_of_the_pointwise_call=draws * k / (sweep["ms"] * 1e-3),
                                   khat_range=[float(np.nanmin(res["khat"])), float(np.nanmax(res["khat"]))],
                                   elpd_loo=float(np.sum(res["elpd_loo"])))
    out["kernels"] = kernel_table(traced[NROWS[0]].source, dt == "f64")
    tctx.close()
    run.close()
    print(json.dumps({dt: out}), flush=True)
    return out


def main(out):
    mhx.use_library(mhx.TOOLS_LIB_PATH)                      # one library for every form, so that the times compare
    result = dict(dim=D, nchains=C, saved_draws=INNER, repeats=REPEATS,
                  unit="wall milliseconds of the blocking call, median [min, max]; phases by PSIS_STOP_AFTER of the tools build, differences of "
                       "medians; *_over_pointwise = multiples of the mhx_run_pointwise call at the same shape in the same rounds")
    for dt in ("f64", "f32"):
        result[dt] = measure(dt)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "psis_rate.json"))
