#!/usr/bin/env python3
"""Throughput of the conditional-proposal kernels (kernel variant 14) beside the family kernel they are built from.

65 536 chains, d = 8, isotropic Gaussian target, one lane per chain, fp64 and fp32:
  (a) the register form of a walk with Normal(0, 0.5 + |x_k|) per component
  (b) the state-in-HBM form of the same walk
  (c) the floor: the family register kernel (variant 13) with [Normal(0, 1)] * 8 -- no map, no normalisers, one pass of log-kernels
Rates are chain-steps per second of kernel time (mhx_stats.kernel_ms: device events around the launches of one sampling call).  A
timed call records two states THIN transitions apart, so it is one long launch and no record traffic; THIN is doubled until the
call takes at least 0.25 s.  The configurations are timed in turn, REPEATS rounds, and the median of each is reported.

    bench_conditional.py [OUT.json]        default OUT: profiles/conditional_bench.json"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402

D, C, REPEATS, MIN_MS = int(os.environ.get("D", 8)), int(os.environ.get("C", 65536)), int(os.environ.get("REPEATS", 5)), 250.0


def timed(run, thin):
    run.sample(2, 1, thin, 0)
    st = run.stats()
    return st["kernel_ms"], st["transitions"] / (st["kernel_ms"] * 1e-3), st


def measure(dt):
    walk = mhx.RandomWalkProposal(lambda x: [mhx.Normal(0, 0.5 + abs(x[k])) for k in range(D)], dim=D)
    floor = mhx.RandomWalkProposal(mhx.Laplace())
    floor.proposal = mhx.ComponentProposal([mhx.Normal(0.0, 1.0)] * D)      # (an all-Normal vector would otherwise lower to an MvNormal)
    configs = [("a_conditional_register", mhx.MetropolisHastings(walk), 0), ("b_conditional_hbm", mhx.MetropolisHastings(walk), mhx.FLAG_GENERIC),
               ("c_family_floor", mhx.MetropolisHastings(floor), 0)]
    model = mhx.DensityModel(mhx.IsoGaussian(D))
    runs, thin = {}, {}
    for name, spl, flags in configs:
        run = mhx.Run(model, spl, nchains=C, seed=1, flags=flags, dtype=dt)
        run.init(np.zeros(D))
        t = 256
        while True:                                          # also the warm-up: the kernel is compiled, the chains leave their start
            ms, _, _ = timed(run, t)
            if ms >= MIN_MS or t >= 32768:
                break
            t *= 2
        runs[name], thin[name] = run, t
    rates = {name: [] for name in runs}
    for _ in range(REPEATS):
        for name, run in runs.items():
            rates[name].append(timed(run, thin[name])[1])
    row = {}
    for name, run in runs.items():
        ms, _, st = timed(run, thin[name])
        r = np.array(rates[name])
        row[name] = dict(steps_per_s=float(np.median(r)), min=float(r.min()), max=float(r.max()), kernel_variant=st["kernel_variant"],
                         transitions_per_call=thin[name] + 1, call_ms=ms, acceptance=st["accepted"] / st["transitions"])
        run.close()
    row["floor_over_register"] = row["c_family_floor"]["steps_per_s"] / row["a_conditional_register"]["steps_per_s"]
    row["register_over_hbm"] = row["a_conditional_register"]["steps_per_s"] / row["b_conditional_hbm"]["steps_per_s"]
    print(json.dumps({dt: row}), flush=True)
    return row


def main(out):
    result = dict(dim=D, nchains=C, repeats=REPEATS, target="IsoGaussian", unit="chain-steps per second of kernel time")
    for dt in ("f64", "f32"):
        result[dt] = measure(dt)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "conditional_bench.json"))
