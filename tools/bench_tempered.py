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

    bench_tempered.py [OUT.json]        default OUT: profiles/tempered_bench.json

--adapt measures the adaptive ladder (kernel variant 17) at the same shape instead, in milliseconds of kernel time per step of all
chains, the three configurations timed in turn as above:
  (fixed)    the geometric ladder with swap_every = 1: (d) above
  (adapting) the same start, LadderAdaptation over more transitions than the run makes: every swap round moves rho and derives the ladder
  (frozen)   LadderAdaptation(0): the adaptive kernel on the ladder of rho0, which is (fixed)'s up to rounding, never adapting
--lib PATH adds (fixed) measured on another build of the library (the parent commit's, say), in child processes of its own that
alternate with children that time (fixed) alone on this build: the fixed ladder's code path must not have moved.

    bench_tempered.py --adapt [--lib OTHER/libmhx.so] [OUT.json]        default OUT: profiles/tempered_adaptive_bench.json

--anchor measures the anchored ladder (kernel variant 18) at the same shape, in the same unit, (fixed) and (anchored) timed in turn:
  (fixed)    the geometric ladder with swap_every = 1: (d) above
  (anchored) the same ladder and scales with a reference density N(0.25, 1.5^2 I): lq beside the target in every transition and swap
--lib PATH adds (fixed) measured on another build of the library (the parent commit's) in a child process of its own.

    bench_tempered.py --anchor [--lib OTHER/libmhx.so] [OUT.json]       default OUT: profiles/tempered_anchored_bench.json"""
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


def measure_adapt(dt, lib=None):
    """lib None: the three configurations on this build; a path, or "-" for this build: (fixed) alone, the A/B children"""
    import mhx
    if lib and lib != "-":
        mhx.use_library(lib)
    s = float(np.float32(2.38 / D ** 0.5))
    rw = mhx.RWMH(mhx.MvNormal(mhx.zeros(D), (s * s) * mhx.I))
    ladder = mhx.geometric_betas(R, 0.05)
    configs = [("fixed", mhx.Tempered(rw, ladder, swap_every=1))]
    if not lib:
        configs += [("adapting", mhx.Tempered(rw, ladder, swap_every=1, adapt=mhx.LadderAdaptation(1 << 20))),
                    ("frozen", mhx.Tempered(rw, ladder, swap_every=1, adapt=mhx.LadderAdaptation(0)))]
    model = mhx.DensityModel(mhx.IsoGaussian(D))
    runs = {}
    for name, spl in configs:
        run = mhx.Run(model, spl, nchains=C, seed=1, reduce_lanes=1, dtype=dt)
        run.init(np.zeros(D))
        run.sample(STEPS, 50, 1, 0)
        runs[name] = run
    ms = {name: [] for name in runs}
    for _ in range(REPEATS):
        for name, run in runs.items():
            run.sample(STEPS, 1, 1, 0)
            st = run.stats()
            ms[name].append(st["kernel_ms"] / (st["transitions"] / C))
    row = {}
    for name, run in runs.items():
        st = run.stats()
        v = np.array(ms[name])
        att, swp = run.swap_stats()
        row[name] = dict(ms_per_step=float(np.median(v)), min=float(v.min()), max=float(v.max()), kernel_variant=st["kernel_variant"],
                         form=run.form_name(), swap_rate=float(swp.sum()) / float(att.sum()))
        run.close()
    return row


def measure_anchor(dt, lib=None):
    """lib None: (fixed) and (anchored) on this build; a path: (fixed) alone on that build"""
    import mhx
    if lib:
        mhx.use_library(lib)
    s = float(np.float32(2.38 / D ** 0.5))
    rw = mhx.RWMH(mhx.MvNormal(mhx.zeros(D), (s * s) * mhx.I))
    ladder = mhx.geometric_betas(R, 0.05)
    configs = [("fixed", mhx.Tempered(rw, ladder, swap_every=1))]
    if not lib:
        configs.append(("anchored", mhx.Tempered(rw, ladder, swap_every=1, reference=mhx.MvNormal(np.full(D, 0.25), 2.25 * mhx.I))))
    model = mhx.DensityModel(mhx.IsoGaussian(D))
    runs = {}
    for name, spl in configs:
        run = mhx.Run(model, spl, nchains=C, seed=1, reduce_lanes=1, dtype=dt)
        run.init(np.zeros(D))
        run.sample(STEPS, 50, 1, 0)
        runs[name] = run
    ms = {name: [] for name in runs}
    for _ in range(REPEATS):
        for name, run in runs.items():
            run.sample(STEPS, 1, 1, 0)
            st = run.stats()
            ms[name].append(st["kernel_ms"] / (st["transitions"] / C))
    row = {}
    for name, run in runs.items():
        st = run.stats()
        v = np.array(ms[name])
        att, swp = run.swap_stats()
        row[name] = dict(ms_per_step=float(np.median(v)), min=float(v.min()), max=float(v.max()), kernel_variant=st["kernel_variant"],
                         form=run.form_name(), swap_rate=float(swp.sum()) / float(att.sum()))
        run.close()
    return row


def main_anchor(out, lib):
    result = dict(dim=D, R=R, nchains=C, recorded_steps=STEPS, repeats=REPEATS, target="IsoGaussian",
                  unit="milliseconds of kernel time per step of all chains")
    for dt in ("f64", "f32"):
        row = child(["--one-anchor", dt])
        if row is None:
            return 1
        row["anchored_over_fixed"] = row["anchored"]["ms_per_step"] / row["fixed"]["ms_per_step"]
        if lib:
            other = child(["--one-anchor", dt, lib])
            if other is None:
                return 1
            row["fixed_other_build"] = other["fixed"]
            row["anchored_over_fixed_other_build"] = row["anchored"]["ms_per_step"] / other["fixed"]["ms_per_step"]
            row["fixed_this_over_other"] = row["fixed"]["ms_per_step"] / other["fixed"]["ms_per_step"]
        result[dt] = row
        print(json.dumps({dt: row}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


def child(args):
    done = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT_S)
    if done.returncode != 0:
        print("bench_tempered: the step %s ended with status %d; nothing more is started" % (args, done.returncode), flush=True)
        return None
    return json.loads(done.stdout.strip().splitlines()[-1])


def main_adapt(out, lib):
    result = dict(dim=D, R=R, nchains=C, recorded_steps=STEPS, repeats=REPEATS, target="IsoGaussian",
                  unit="milliseconds of kernel time per step of all chains")
    for dt in ("f64", "f32"):
        row = child(["--one-adapt", dt])
        if row is None:
            return 1
        if lib:
            # the other build and this one in turn, a child process each that times (fixed) ALONE -- the same process on both sides,
            # not (fixed) between two other kernels on one of them: medians of the children's medians
            other, this = [], []
            for i in range(3):
                a, b = child(["--one-adapt", dt, lib]), child(["--one-adapt", dt, "-"])
                if a is None or b is None:
                    return 1
                other.append(a["fixed"]["ms_per_step"])
                this.append(b["fixed"]["ms_per_step"])
            row["fixed_other_build"] = dict(ms_per_step=float(np.median(other)), runs=other)
            row["fixed_this_build"] = dict(ms_per_step=float(np.median(this)), runs=this)
            row["fixed_this_over_other"] = float(np.median(this) / np.median(other))
        row["adapting_over_fixed"] = row["adapting"]["ms_per_step"] / row["fixed"]["ms_per_step"]
        row["frozen_over_fixed"] = row["frozen"]["ms_per_step"] / row["fixed"]["ms_per_step"]
        # an adapting round per step: its time per chain-step, in nanoseconds of kernel time
        row["adapting_round_ns_per_chain_step"] = (row["adapting"]["ms_per_step"] - row["frozen"]["ms_per_step"]) * 1e6 / C
        result[dt] = row
        print(json.dumps({dt: row}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


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
    if len(sys.argv) > 2 and sys.argv[1] == "--one-adapt":
        print(json.dumps(measure_adapt(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)), flush=True)
        sys.exit(0)
    if len(sys.argv) > 2 and sys.argv[1] == "--one-anchor":
        print(json.dumps(measure_anchor(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)), flush=True)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--anchor":
        rest = sys.argv[2:]
        lib = None
        if rest and rest[0] == "--lib":
            lib, rest = os.path.abspath(rest[1]), rest[2:]
        sys.exit(main_anchor(rest[0] if rest else os.path.join(ROOT, "profiles", "tempered_anchored_bench.json"), lib))
    if len(sys.argv) > 1 and sys.argv[1] == "--adapt":
        rest = sys.argv[2:]
        lib = None
        if rest and rest[0] == "--lib":
            lib, rest = os.path.abspath(rest[1]), rest[2:]
        sys.exit(main_adapt(rest[0] if rest else os.path.join(ROOT, "profiles", "tempered_adaptive_bench.json"), lib))
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tempered_bench.json")))
