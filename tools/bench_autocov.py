#!/usr/bin/env python3
"""Time of the device autocovariance sums (mhx_run_autocovariance) on the tensor bench.py's flagship workload
leaves on the device: C2 -- RWMH on the 100-dim isotropic Gaussian, 65 536 chains, 250 saved draws each, [250][101][65536] -- in fp64
and fp32.

What is timed is the HOST WALL time of one blocking call (both kernels, the copies, the host's checks), after a warm-up of every
form; the forms are timed in turn (interleaved), REPEATS rounds, and the median of each is reported with its minimum and maximum.
  per_lag_K        the yardstick: the per-lag kernel of mhx_run_diagnostics over ALL chains, Run.diagnostics(max_lag=K, ess_chains=0)
                   minus Run.diagnostics(max_lag=0) (the moments, which both calls take) -- lags 0..K as well (nlag = K + 1, even)
  tiled_K_R        Run.autocovariance of lags 0..K, all 101 rows, all chains, with R lags per tile (option ACF_R), K = 63 and 255;
                   `over_per_lag` = its time / the yardstick's, `sweeps` = its time over the time of reading the tensor once at the
                   copy ceiling of DESIGN.md section 7
  tiled_default    the four lags (1, 5, 10, 50) of Chains.autocor with lag 0, the shipped R: a sparse tile list
  normalised_63    lags 0..63 with normalise = 1, the shipped R
Nothing here gates anything: the tests do.

    bench_autocov.py [OUT.json]        default OUT: profiles/autocov_bench.json      env: C, INNER, REPEATS"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402

D, C, INNER, REPEATS = 100, int(os.environ.get("C", 65536)), int(os.environ.get("INNER", 250)), int(os.environ.get("REPEATS", 5))
CEILING = 6.3e12
TILES = (8, 16, 32)
LAGS = (63, 255)


def measure(dt):
    s = float(np.float32(2.38 / D ** 0.5))
    ctx = mhx.Context.default(dtype=dt)
    run = mhx.Run(mhx.DensityModel(mhx.IsoGaussian(D)), mhx.RWMH(mhx.MvNormal(mhx.zeros(D), s * s * mhx.I)), nchains=C, seed=0xC0FFEE,
                  ctx=ctx, reduce_lanes=2)
    run.init(None)
    run.sample(INNER, 1, 1, 0)
    tensor_bytes = INNER * (D + 1) * C * (8 if dt == "f64" else 4)
    lags = sorted({min(k, INNER - 1) for k in LAGS})       # a record of 250 draws has lags 0..249: K = 255 becomes 249

    def wall(f):
        t0 = time.perf_counter()
        out = f()
        return (time.perf_counter() - t0) * 1e3, out

    def tiled(K, R, normalise=False):
        ctx.set_option("ACF_R", R)
        try:
            ms, (acov, nvalid) = wall(lambda: run.autocovariance(np.arange(K + 1), normalise=normalise))
        finally:
            ctx.set_option("ACF_R", None)
        assert np.isfinite(acov).all() and np.all(nvalid == C)
        return ms, acov

    def default():
        ms, (acov, _) = wall(lambda: run.autocovariance([0, 1, 5, 10, 50]))
        assert np.isfinite(acov).all()
        return ms

    forms = {"moments": lambda: wall(lambda: run.diagnostics(max_lag=0))[0], "tiled_default": default,
             "normalised_63": lambda: tiled(min(63, INNER - 1), None, True)[0]}
    for K in lags:
        forms["diagnostics_%d" % K] = lambda K=K: wall(lambda: run.diagnostics(max_lag=K, ess_chains=0))[0]
        for R in TILES:
            forms["tiled_%d_R%d" % (K, R)] = lambda K=K, R=R: tiled(K, R)[0]
    # the three tile widths compute the same sums, up to the order of the additions
    ref = tiled(lags[0], TILES[0])[1]
    for R in TILES[1:]:
        assert np.allclose(tiled(lags[0], R)[1], ref, rtol=1e-4 if dt == "f32" else 1e-10, atol=0.0)
    for f in forms.values():                                # warm-up: the context's scratch is allocated and kept
        f()
    times = {k: [] for k in forms}
    for _ in range(REPEATS):
        for k, f in forms.items():
            times[k].append(f())

    def stat(t):
        t = np.array(t)
        return dict(ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))

    row = dict(tensor_bytes=tensor_bytes, one_sweep_ms=tensor_bytes / CEILING * 1e3, forms={k: stat(t) for k, t in times.items()})
    f = row["forms"]
    for K in lags:
        per_lag = f["diagnostics_%d" % K]["ms"] - f["moments"]["ms"]
        f["per_lag_%d" % K] = dict(ms=per_lag, sweeps=per_lag / row["one_sweep_ms"])
        for R in TILES:
            k = "tiled_%d_R%d" % (K, R)
            f[k].update(over_per_lag=f[k]["ms"] / per_lag, sweeps=f[k]["ms"] / row["one_sweep_ms"])
    run.close()
    print(json.dumps({dt: row}), flush=True)
    return row


def main(out):
    result = dict(dim=D, nchains=C, saved_draws=INNER, repeats=REPEATS, copy_ceiling_TBps=CEILING / 1e12,
                  shipped_tile=dict(mhx.ACF_TILE), unit="wall milliseconds of one blocking call")
    for dt in ("f64", "f32"):
        result[dt] = measure(dt)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "autocov_bench.json"))
