#!/usr/bin/env python3
"""Rate of the pointwise log-likelihood pass (mhx_run_pointwise) on the tensor bench.py's flagship workload
leaves on the device: C2 -- RWMH on the 100-dim isotropic Gaussian, 65 536 chains, 250 saved draws each, [250][101][65536] -- in fp64
and fp32.

Function: the README's Normal log-likelihood, log Normal(y | mu, sigma) with mu = x[0] and sigma = |x[1]| + 0.5 (the tensor's second
row is a standard normal, not a scale: the README's line needs a positive one, and a NaN l would take the cheap branch of the frame).
Rows: nrows = 30 and 2 000.  Per (nrows, POINTWISE_ROWS = 2, 4, 8, 16; the library's default is marked): the time of the BLOCKING
CALL, wall clock -- upload of the rows, the shift launch, the sweep, the merge, the copy back; the library hands out no event pair
for a call that returns no run, so the fixed part is measured beside it as the same call on ONE saved draw of the same tensor and
reported as `overhead_ms` -- median over REPEATS rounds in which the forms alternate, with minimum and maximum.  Quoted as (draw, row)
evaluations per second and as a share of the VALU issue rate: the instructions of the sweep's draw loop per evaluation, counted in
the ISA that hipcc emits for gfx950 from the same source and options and priced by class with the cycles tools/ubench/valu_rates.hip
measured (tools/isa_mix.py: group_cycles), over 1024 SIMDs x 2.4 GHz.
Yardstick, at nrows = 30, interleaved in the same rounds, wall clock: what exists without this pass -- derive with 30 outputs (the l of
every row as a derived run), samples() of that run over PCIe, then scipy.special.logsumexp and numpy.var on the host.
Nothing here gates anything: the tests do.

    pointwise_rate.py [OUT.json]        default OUT: profiles/pointwise_rate.json      env: C, INNER, REPEATS, YARDSTICK=0 skips it"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mhx  # noqa: E402
import mhx.trace as T  # noqa: E402
import isa_mix  # noqa: E402

D, C, INNER, REPEATS = 100, int(os.environ.get("C", 65536)), int(os.environ.get("INNER", 250)), int(os.environ.get("REPEATS", 7))
TILES = (2, 4, 8, 16)
DEFAULT_TILE = {"f64": 8, "f32": 4}          # MHX_POINTWISE_ROWS_DEFAULT
NROWS = (30, 2000)
CSRC = os.path.join(ROOT, "advancedmh.jl_amd", "csrc")
LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)


def normal_ll(t, y):
    sigma = abs(t[1]) + 0.5
    return -0.5 * ((y - t[0]) / sigma) ** 2 - T.log(sigma) - LOG_SQRT_2PI


_ISA = {}


def loop_cycles(source, f64, tile):
    key = (source, f64, tile)
    if key not in _ISA:
        _ISA[key] = _loop_cycles(source, f64, tile)
    return _ISA[key]


def _loop_cycles(source, f64, tile):
    """(VALU instructions, class-weighted issue cycles) per (draw, row) of the sweep's draw loop -- the largest loop of mhx_jit_pointwise
    in the ISA -- and the kernel's VGPRs, from the cross-compiler; None where hipcc is not there"""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "pw.hip"), os.path.join(tmp, "pw.s")
        open(src, "w").write('#include "mhx_device_math.h"\n' + source + '#define MHX_HAVE_POINTWISE 1\n#include "mhx_pointwise_kernels.h"\n')
        cmd = [hipcc, "-x", "hip", "--offload-device-only", "--no-gpu-bundle-output", "-S", "-DMHX_JIT_BUILD=1", "-I" + CSRC,
               "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-DMHX_REAL64=%d" % (1 if f64 else 0),
               "-DMHX_JIT_POINTWISE_ROWS=%d" % tile, "-o", out, src]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if done.returncode:
            raise RuntimeError(done.stdout[-2000:])
        text = open(out).read()
    body = text[text.index("mhx_jit_pointwise:"):]
    end = body.index(".end_amdhsa_kernel")
    descriptor, tail = body[body.index("s_endpgm"):end], body[end:end + 4000]
    body = body[:body.index("s_endpgm")]
    lines = body.split("\n")
    labels = {ln.split(":")[0]: n for n, ln in enumerate(lines) if ln.startswith(".LBB")}
    best = []
    for n, ln in enumerate(lines):
        m = re.search(r"s_cbranch_\w+ (\.LBB\w+)", ln)
        if m and labels.get(m.group(1), n) < n:
            seg = [x.split()[0] for x in lines[labels[m.group(1)]:n + 1] if x.startswith("\t") and not x.strip().startswith((".", ";"))]
            if len(seg) > len(best):
                best = seg
    cyc = isa_mix.group_cycles()
    valu = [m for m in best if m.startswith("v_")]
    occ = re.search(r"; Occupancy: (\d+)", tail)
    return dict(loop_instructions=len(best), valu_per_eval=len(valu) / tile, cycles_per_eval=sum(cyc[isa_mix.cost_group(m)] for m in valu) / tile,
                global_loads_in_loop=sum(1 for m in best if m.startswith("global_load")),
                vgprs=int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", descriptor).group(1)), waves_per_simd=int(occ.group(1)) if occ else None)


def stat(t):
    t = np.array(t)
    return dict(ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))


def measure(dt, yardstick):
    s = float(np.float32(2.38 / D ** 0.5))
    ctx = mhx.Context.default(dtype=dt)
    run = mhx.Run(mhx.DensityModel(mhx.IsoGaussian(D)), mhx.RWMH(mhx.MvNormal(mhx.zeros(D), s * s * mhx.I)), nchains=C, seed=0xC0FFEE,
                  ctx=ctx, reduce_lanes=2)
    run.init(None)
    run.sample(INNER, 1, 1, 0)
    rng = np.random.default_rng(1234)
    rows = {n: rng.normal(0.0, 1.0, size=n) for n in NROWS}
    traced = {n: T.trace_pointwise(normal_ll, D, rows[n]) for n in NROWS}
    one = mhx.Run(mhx.DensityModel(mhx.IsoGaussian(D)), mhx.RWMH(mhx.MvNormal(mhx.zeros(D), s * s * mhx.I)), nchains=C, seed=0xC0FFEE,
                  ctx=ctx, reduce_lanes=2)
    one.init(None)
    one.sample(1, 1, 1, 0)                                  # ONE saved draw of the same chains: the call's fixed part

    def call_ms(r, n, tile):
        ctx.set_option("POINTWISE_ROWS", tile)
        try:
            t0 = time.perf_counter()
            res = r.pointwise(traced[n])
            ms = (time.perf_counter() - t0) * 1e3
        finally:
            ctx.set_option("POINTWISE_ROWS", None)
        return ms, res

    def yardstick_ms():
        t0 = time.perf_counter()
        der = run.derive(lambda t: [normal_ll(t, float(y)) for y in rows[30]])
        t1 = time.perf_counter()
        l = der.samples()[0][:, :30, :]
        t2 = time.perf_counter()
        from scipy.special import logsumexp
        l = np.moveaxis(l, 1, 0).reshape(30, -1).astype(np.float64)
        lppd = logsumexp(l, axis=1) - math.log(l.shape[1])
        var = np.var(l, axis=1, ddof=1)
        t3 = time.perf_counter()
        der.close()
        return dict(total=(t3 - t0) * 1e3, derive=(t1 - t0) * 1e3, samples=(t2 - t1) * 1e3, host=(t3 - t2) * 1e3), lppd, var

    forms = {}
    for n in NROWS:
        for tile in TILES:
            forms["n%d_r%d" % (n, tile)] = lambda n=n, tile=tile: call_ms(run, n, tile)[0]
            forms["n%d_r%d_one" % (n, tile)] = lambda n=n, tile=tile: call_ms(one, n, tile)[0]
    if yardstick:
        forms["yardstick"] = lambda: yardstick_ms()[0]["total"]
    for f in forms.values():                                # warm-up: every module compiled and loaded
        f()
    times = {k: [] for k in forms}
    parts = []
    for rnd in range(REPEATS):
        print("# %s round %d" % (dt, rnd), file=sys.stderr, flush=True)
        for k, f in forms.items():
            if k == "yardstick":
                p, _, _ = yardstick_ms()
                parts.append(p)
                times[k].append(p["total"])
            else:
                times[k].append(f())
    draws = INNER * C
    out = dict(draws=draws, rows={})
    for n in NROWS:
        per = {}
        for tile in TILES:
            st = stat(times["n%d_r%d" % (n, tile)])
            st["overhead_ms"] = float(np.median(times["n%d_r%d_one" % (n, tile)]))
            st["evals_per_s"] = draws * n / (st["ms"] * 1e-3)
            isa = loop_cycles(traced[n].source, dt == "f64", tile)
            if isa:
                st.update(isa)
                st["valu_issue_share"] = st["evals_per_s"] / 64.0 * isa["cycles_per_eval"] / (isa_mix.SIMDS * isa_mix.CLOCK_HZ)
            per[str(tile)] = st
        out["rows"][str(n)] = per
    # the pass computes what the yardstick computes
    _, res = call_ms(run, 30, DEFAULT_TILE[dt])
    tab = mhx.pointwise_table(res)
    if yardstick:
        _, lppd, var = yardstick_ms()
        tol = 1e-9 if dt == "f64" else 1e-3
        assert np.allclose(tab["lppd"], lppd, rtol=tol, atol=tol) and np.allclose(tab["var"], var, rtol=tol, atol=tol)
        y = stat(times["yardstick"])
        y.update({k + "_ms": float(np.median([p[k] for p in parts])) for k in ("derive", "samples", "host")})
        y["speedup_at_default"] = y["ms"] / out["rows"]["30"][str(DEFAULT_TILE[dt])]["ms"]
        out["yardstick_30_rows"] = y
    one.close()
    run.close()
    print(json.dumps({dt: out}), flush=True)
    return out


def main(out):
    result = dict(dim=D, nchains=C, saved_draws=INNER, repeats=REPEATS, default_rows_per_tile=DEFAULT_TILE,
                  unit="wall milliseconds of the blocking call; evals = saved_draws x nchains x nrows; valu_issue_share = evals/s / 64 lanes x "
                       "class-weighted cycles per evaluation / (1024 SIMDs x 2.4 GHz)")
    for dt in ("f64", "f32"):
        result[dt] = measure(dt, os.environ.get("YARDSTICK", "1") != "0")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pointwise_rate.json"))
