#!/usr/bin/env python3
"""Rates of the adaptive random walk (kernel variant 19) beside the plain lane-per-chain run it becomes once its proposal is frozen.

d = 100 (or D of the environment), 65 536 chains, isotropic Gaussian target, DIAG proposal 2.38 / sqrt(d) in every coordinate, one
lane per chain, every state recorded, fp64 and fp32; milliseconds of kernel time per step of all chains (mhx_stats.kernel_ms, device
events):
  (plain)          mhx_rwmh_create with the DIAG proposal, reduce_lanes = 1: the yardstick
  (frozen)         ProposalAdaptation(0): the frozen phase from the first transition on -- (plain)'s chains bit for bit
  (adapting)       ProposalAdaptation(2^20): every timed transition moves lam and eff
  (adapting_shape) ... with shape=True: m, v and sig as well
Every configuration is warmed up (its kernel is compiled and loaded, the chains leave their start), then the configurations are timed
in turn, REPEATS rounds, and the median of each is reported with its spread.  Each width runs in a child process of its own under a
time limit; a width that fails ends the run.
--lib PATH adds (plain) measured on another build of the library (the parent commit's), in a child process of its own.

    bench_adaptive.py [--lib OTHER/libmhx.so] [OUT.json]        default OUT: profiles/adaptive_bench.json"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))

D = int(os.environ.get("D", 100))
C, STEPS, REPEATS = int(os.environ.get("C", 65536)), int(os.environ.get("STEPS", 100)), 7
STEP_LIMIT_S = 240


def measure(dt, lib=None):
    """lib None: the four configurations on this build; a path: (plain) alone on that build"""
    import mhx
    if lib:
        mhx.use_library(lib)
    s = float(np.float32(2.38 / D ** 0.5))
    mv = mhx.MvNormal(mhx.zeros(D), np.full(D, s * s))
    configs = [("plain", mhx.RWMH(mv))]
    if not lib:
        configs += [("frozen", mhx.RWMH(mv, adapt=mhx.ProposalAdaptation(0))),
                    ("adapting", mhx.RWMH(mv, adapt=mhx.ProposalAdaptation(1 << 20))),
                    ("adapting_shape", mhx.RWMH(mv, adapt=mhx.ProposalAdaptation(1 << 20, shape=True)))]
    model = mhx.DensityModel(mhx.IsoGaussian(D))
    runs = {}
    for name, spl in configs:
        run = mhx.Run(model, spl, nchains=C, seed=1, reduce_lanes=1, dtype=dt)
        run.init(np.zeros(D))
        run.sample(STEPS, 50, 1, 0)                   # warm-up: same shape as the timed call
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
        row[name] = dict(ms_per_step=float(np.median(v)), min=float(v.min()), max=float(v.max()), kernel_variant=st["kernel_variant"],
                         form=run.form_name(), steps_per_s=C / (float(np.median(v)) * 1e-3), acceptance=st["accepted"] / st["transitions"])
        run.close()
    if not lib:
        for name in ("frozen", "adapting", "adapting_shape"):                  # ratios of TIME per step: above 1 = slower than (plain)
            row[name + "_over_plain"] = row[name]["ms_per_step"] / row["plain"]["ms_per_step"]
    return row


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        print("RESULT " + json.dumps(measure(args[1], args[2] if len(args) > 2 else None)), flush=True)
        return
    lib = None
    if args and args[0] == "--lib":
        lib, args = os.path.abspath(args[1]), args[2:]
    out = args[0] if args else os.path.join(ROOT, "profiles", "adaptive_bench.json")
    res = dict(shape=dict(d=D, chains=C, steps_per_call=STEPS, repeats=REPEATS, target="IsoGaussian", proposal="DIAG", reduce_lanes=1))
    for dt in ("f64", "f32"):
        for key, extra in ((dt, []), (dt + "_other_build", [lib])):
            if extra == [None]:
                continue
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", dt] + extra, stdout=subprocess.PIPE, text=True,
                                  timeout=STEP_LIMIT_S)
            if done.returncode != 0:
                sys.exit("bench_adaptive: the %s child ended with status %d" % (key, done.returncode))
            line = [ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            res[key] = json.loads(line[len("RESULT "):])
        if lib:
            res[dt]["plain_over_other_build"] = res[dt]["plain"]["ms_per_step"] / res[dt + "_other_build"]["plain"]["ms_per_step"]
            res[dt]["frozen_over_other_build"] = res[dt]["frozen"]["ms_per_step"] / res[dt + "_other_build"]["plain"]["ms_per_step"]
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    for dt in ("f64", "f32"):
        r = res[dt]
        print("%s d=%d: plain %.4f ms/step [%s]  frozen x%.3f [%s]  adapting x%.3f [%s]  adapting+shape x%.3f [%s]%s" % (
            dt, D, r["plain"]["ms_per_step"], r["plain"]["form"], r["frozen_over_plain"], r["frozen"]["form"], r["adapting_over_plain"],
            r["adapting"]["form"], r["adapting_shape_over_plain"], r["adapting_shape"]["form"],
            "  frozen over the other build's plain x%.3f" % r["frozen_over_other_build"] if lib else ""))


if __name__ == "__main__":
    main()
