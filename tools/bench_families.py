#!/usr/bin/env python3
"""Throughput of the proposal-family kernels (kernel variant 13) beside the register kernel they sit next to.

d = 16 and d = 32 (the register form's dimension limit in fp64), 65 536 chains, 250 recorded steps per timed call, isotropic Gaussian target, one lane per chain, fp64 and fp32:
  (a) the DIAG register kernel (an MvNormal random walk, reduce_lanes = 1)
  (b) the specialised family kernel with d Normal components   -- (a)'s draws plus the two ratio sums
  (c) the specialised family kernel with d Laplace components  -- a logarithm and a sign bit per component instead of Box-Muller
  (d) the state-in-HBM form on (c)
Rates are chain-steps per second of kernel time (mhx_stats.kernel_ms, device events).  Every configuration is warmed up (its kernel
is compiled and loaded, the chains leave their start), then the configurations are timed in turn, REPEATS rounds, and the median
of each is reported with its spread.

    bench_families.py [OUT.json]        default OUT: profiles/families_bench.json"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402

DIMS = [int(v) for v in os.environ.get("DIMS", "16,32").split(",")]      # 32: the register form's dimension limit in fp64
C, STEPS, REPEATS = int(os.environ.get("C", 65536)), int(os.environ.get("STEPS", 250)), 7


def component_walk(comps):
    rw = mhx.RandomWalkProposal(comps[0] if not isinstance(comps[0], mhx.Normal) else mhx.Laplace())
    rw.proposal = mhx.ComponentProposal(comps)       # (an all-Normal vector would otherwise lower to an MvNormal: that is (a))
    return mhx.MetropolisHastings(rw)


def measure(D):
    s = float(np.float32(2.38 / D ** 0.5))
    th = float(np.float32(s / 2 ** 0.5))                 # Laplace(0, theta) of the same variance
    configs = [("a_diag_register", mhx.RWMH(mhx.MvNormal(mhx.zeros(D), np.full(D, s * s))), 0),
               ("b_family_normal", component_walk([mhx.Normal(0.0, s)] * D), 0),
               ("c_family_laplace", component_walk([mhx.Laplace(0.0, th)] * D), 0),
               ("d_family_laplace_hbm", component_walk([mhx.Laplace(0.0, th)] * D), mhx.FLAG_GENERIC)]
    result = dict(dim=D, nchains=C, recorded_steps=STEPS, repeats=REPEATS, target="IsoGaussian", unit="chain-steps per second of kernel time")
    for dt in ("f64", "f32"):
        model = mhx.DensityModel(mhx.IsoGaussian(D))
        runs = {}
        for name, spl, flags in configs:
            run = mhx.Run(model, spl, nchains=C, seed=1, flags=flags, reduce_lanes=1, dtype=dt)
            run.init(np.zeros(D))
            run.sample(STEPS, 50, 1, 0)                   # warm-up: same shape as the timed call
            runs[name] = run
        rates = {name: [] for name in runs}
        for _ in range(REPEATS):
            for name, run in runs.items():
                run.sample(STEPS, 1, 1, 0)
                st = run.stats()
                rates[name].append(st["transitions"] / (st["kernel_ms"] * 1e-3))
        row = {}
        for name, run in runs.items():
            st = run.stats()
            r = np.array(rates[name])
            row[name] = dict(steps_per_s=float(np.median(r)), min=float(r.min()), max=float(r.max()), kernel_variant=st["kernel_variant"],
                             acceptance=st["accepted"] / st["transitions"])
            run.close()
        med = {k: v["steps_per_s"] for k, v in row.items()}
        # ratios of TIME per step (family / baseline): above 1 = slower than the baseline
        row["b_over_a"] = med["a_diag_register"] / med["b_family_normal"]
        row["c_over_a"] = med["a_diag_register"] / med["c_family_laplace"]
        row["d_over_c"] = med["c_family_laplace"] / med["d_family_laplace_hbm"]
        result[dt] = row
        print(json.dumps({"d": D, dt: row}), flush=True)
    return result


def main(out):
    result = {"d%d" % D: measure(D) for D in DIMS}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "families_bench.json"))
