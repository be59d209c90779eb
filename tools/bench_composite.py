#!/usr/bin/env python3
"""Throughput of the composite-proposal kernel (kernel variant 15) beside the two kernels it degenerates to.

65 536 chains, isotropic Gaussian target, one lane per chain, fp64 and fp32, everything the register form (asserted:
mhx_stats.register_form).  Each older form at the shape its own tool measures (bench_conditional.py: d = 8, bench_families.py: d = 16):
  (a) variant 14, d = 8: a walk with Normal(0, 0.5 + |x_k|) per component (one function of the whole state)
  (b) variant 15, d = 8: the same walk as a ONE-BLOCK composite -- the same chain as (a), bit for bit
  (c) variant 13, d = 16: [Laplace(0, 1)] * 16 as one random walk
  (d) variant 15, d = 16: the same components as eight constant walk blocks of two -- an all-constant one-kind composite
  (e) variant 15, d = 8: a mixed composite: a symmetric walk of two Normals | a static block Normal, InverseGamma | four mapped
      Laplace walks of one component each
Rates are chain-steps per second of kernel time (mhx_stats.kernel_ms: device events around the launches of one sampling call).  A
timed call records two states THIN transitions apart, so it is one long launch and no record traffic; THIN is doubled until the
call takes at least 0.25 s or THIN is 32 768 (these kernels reach the cap: calls of 50 - 150 ms).  The configurations are timed in turn (interleaved), REPEATS rounds; the median of each is reported
with its minimum and maximum, so the spread between repeated runs of the older forms stands next to the difference to the new one.

    bench_composite.py [OUT.json]        default OUT: profiles/composite_bench.json"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402

D, D13, C, REPEATS, MIN_MS = 8, 16, int(os.environ.get("C", 65536)), int(os.environ.get("REPEATS", 5)), 250.0


def timed(run, thin):
    run.sample(2, 1, thin, 0)
    st = run.stats()
    return st["kernel_ms"], st["transitions"] / (st["kernel_ms"] * 1e-3), st


def measure(dt):
    RW, ST = mhx.RandomWalkProposal, mhx.StaticProposal
    walk = lambda: RW(lambda x: [mhx.Normal(0, 0.5 + abs(x[k])) for k in range(D)], dim=D)
    mixed = [RW([mhx.Normal(0, 0.5), mhx.Normal(0, 0.7)], issymmetric=True), ST([mhx.Normal(0, 1), mhx.InverseGamma(2, 3)])]
    mixed += [RW(lambda x: mhx.Laplace(0, 0.4 + 0.2 * abs(x)), dim=1) for _ in range(4)]
    configs = [("a_conditional", mhx.MetropolisHastings(walk()), 14, D),
               ("b_composite_one_block", mhx.MetropolisHastings([walk()]), 15, D),
               ("c_family", mhx.MetropolisHastings(RW([mhx.Laplace(0, 1)] * D13)), 13, D13),
               ("d_composite_constant", mhx.MetropolisHastings([RW([mhx.Laplace(0, 1)] * 2) for _ in range(D13 // 2)]), 15, D13),
               ("e_composite_mixed", mhx.MetropolisHastings(mixed), 15, D)]
    runs, thin = {}, {}
    for name, spl, variant, dim in configs:
        run = mhx.Run(mhx.DensityModel(mhx.IsoGaussian(dim)), spl, nchains=C, seed=1, dtype=dt)
        run.init(np.ones(dim))
        t = 256
        while True:                                          # also the warm-up: the kernel is compiled, the chains leave their start
            ms, _, st = timed(run, t)
            if ms >= MIN_MS or t >= 32768:
                break
            t *= 2
        assert st["kernel_variant"] == variant and st["register_form"] == 1, (name, st["kernel_variant"], st["register_form"])
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
                         dim=run.dim, transitions_per_call=thin[name] + 1, call_ms=ms, acceptance=st["accepted"] / st["transitions"])
        run.close()
    row["one_block_over_conditional"] = row["b_composite_one_block"]["steps_per_s"] / row["a_conditional"]["steps_per_s"]
    row["constant_over_family"] = row["d_composite_constant"]["steps_per_s"] / row["c_family"]["steps_per_s"]
    print(json.dumps({dt: row}), flush=True)
    return row


def main(out):
    result = dict(dim=D, dim_family=D13, nchains=C, repeats=REPEATS, target="IsoGaussian", unit="chain-steps per second of kernel time")
    for dt in ("f64", "f32"):
        result[dt] = measure(dt)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "composite_bench.json"))
