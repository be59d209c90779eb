#!/usr/bin/env python3
"""Cost of the tempering frame and of a swap round on the register form (kernel variant 16) beside the plain register kernel.

d = 8, 65 536 chains (8 192 ladders of R = 8), 250 recorded steps per timed call, isotropic Gaussian target, ISO proposal, one lane per
chain, fp64 and fp32:
  (a) the plain register kernel (mhx_rwmh_create, reduce_lanes = 1)
  (b) the tempered register form with every beta and every scale 1 and swap_every = 0   -- (a)'s chains bit for bit: the frame's cost
  (c) the tempered register form on a geometric ladder, swap_every = 0
  (d) the same ladder with swap_every = 1                                               -- (d) - (c): the cost of a swap round
Rates are chain-steps per second of kernel time (mhx_stats.kernel_ms, device events).  Every configuration is warmed up (its kernel
is compiled and loaded, the chains leave their start), then the configurations are timed in turn, REPEATS rounds, and the median
of each is reported with its spread.  Each width runs in a child process of its own under a time limit; a width that fails ends the
run.

    bench_tempered.py [OUT.json]        default OUT: profiles/tempered_bench.json"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))

D, R = int(os.environ.get("D", 8)), int(os.environ.get("R", 8))
C, STEPS, REPEATS = int(os.environ.get("C", 65536)), int(os.environ.get("STEPS", 250)), 7
STEP_LIMIT_S = 240


def measure(dt):
    import mhx
    s = float(np.float32(2.38 / D ** 0.5))
    mv = mhx.MvNormal(mhx.zeros(D), (s * s) * mhx.I)
    ladder = mhx.geometric_betas(R, 0.05)
    configs = [("a_plain_register", mhx.RWMH(mv)),
               ("b_tempered_unit_noswap", mhx.Tempered(mhx.RWMH(mv), [1.0] * R, swap_every=0, scales=[1.0] * R)),
               ("c_tempered_ladder_noswap", mhx.Tempered(mhx.RWMH(mv), ladder, swap_every=0)),
               ("d_tempered_ladder_swap1", mhx.Tempered(mhx.RWMH(mv), ladder, swap_every=1))]
    model = mhx.DensityModel(mhx.IsoGaussian(D))
    runs = {}
    for name, spl in configs:
        run = mhx.Run(model, spl, nchains=C, seed=1, reduce_lanes=1, dtype=dt)
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
                         form=run.form_name(), acceptance=st["accepted"] / st["transitions"])
    att, swp = runs["d_tempered_ladder_swap1"].swap_stats()
    row["d_tempered_ladder_swap1"]["swap_rate"] = float(swp.sum()) / float(att.sum())
    for run in runs.values():
        run.close()
    med = {k: v["steps_per_s"] for k, v in row.items()}
    # ratios of TIME per step: above 1 = slower than what it is compared with
    row["frame_b_over_a"] = med["a_plain_register"] / med["b_tempered_unit_noswap"]
    row["swap_d_over_c"] = med["c_tempered_ladder_noswap"] / med["d_tempered_ladder_swap1"]
    # a swap round per step: its time per chain-step, in nanoseconds of kernel time
    row["swap_round_ns_per_chain_step"] = (1.0 / med["d_tempered_ladder_swap1"] - 1.0 / med["c_tempered_ladder_noswap"]) * 1e9
    return row


def main(out):
    result = dict(dim=D, R=R, nchains=C, recorded_steps=STEPS, repeats=REPEATS, target="IsoGaussian", unit="chain-steps per second of kernel time")
    for dt in ("f64", "f32"):
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", dt], stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT_S)
        if done.returncode != 0:
            print("bench_tempered: the %s step ended with status %d; nothing more is started" % (dt, done.returncode), flush=True)
            return done.returncode
        result[dt] = json.loads(done.stdout.strip().splitlines()[-1])
        print(json.dumps({dt: result[dt]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        print(json.dumps(measure(sys.argv[2])), flush=True)
        sys.exit(0)
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tempered_bench.json")))
