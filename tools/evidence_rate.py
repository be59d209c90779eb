#!/usr/bin/env python3
"""The evidence sweep (mhx_run_evidence) beside the first pass of the radix select on the same tensor.

An anchored tempered run, d = 8, R = 8, isotropic Gaussian target, power ladder to beta = 0, INNER = 250 saved draws, at 65 536 chains
and at 4 096 (where the strip slots are what fills the device), fp64 and fp32:
  evidence     wall time of one blocking mhx_run_evidence call: the sweep of all d + 1 rows, the merge, the copy of [nchains][8] doubles
  first_pass   the yardstick: ONE first pass of the select at 11 bits over the same d + 1 rows (mhx_run_select_histogram, one group per
               row), which reads the same bytes
Both as the median of REPEATS alternating calls after a warm-up, in milliseconds and in bytes of the tensor per second.  Each width
runs in a child process of its own under a time limit; a width that fails ends the run.

    evidence_rate.py [OUT.json]        default OUT: profiles/evidence_rate.json"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))

D, R, INNER, REPEATS = 8, 8, int(os.environ.get("INNER", 250)), int(os.environ.get("REPEATS", 7))
CHAINS = (65536, 4096)
STEP_LIMIT_S = 240


def measure(dt):
    import mhx
    out = {}
    for C in CHAINS:
        s = float(np.float32(2.38 / D ** 0.5))
        spl = mhx.Tempered(mhx.RWMH(mhx.MvNormal(mhx.zeros(D), (s * s) * mhx.I)), mhx.power_betas(R, 3.0), swap_every=1,
                           scales=np.linspace(1.0, 2.0, R), reference=mhx.MvNormal(np.full(D, 0.25), 2.25 * mhx.I))
        run = mhx.Run(mhx.DensityModel(mhx.IsoGaussian(D)), spl, nchains=C, seed=0xE71D, dtype=dt)
        run.init(None)
        run.sample(INNER, 1, 1, 0)
        rows = np.arange(D + 1, dtype=np.int32)
        keybits = 64 if dt == "f64" else 32
        nbytes = INNER * (D + 1) * C * (keybits // 8)

        def first_pass():
            pf, ng = np.zeros(D + 1, dtype=np.uint64), np.ones(D + 1, dtype=np.int32)
            hist = np.zeros((D + 1, 1 << 11), dtype=np.uint64)
            i32p, u64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)
            t0 = time.perf_counter()
            mhx.check(mhx.lib().mhx_run_select_histogram(run.h, rows.ctypes.data_as(i32p), D + 1, pf.ctypes.data_as(u64p), ng.ctypes.data_as(i32p),
                                                         1, keybits - 11, 11, hist.ctypes.data_as(u64p)))
            ms = (time.perf_counter() - t0) * 1e3
            assert np.all(hist.sum(axis=1) == INNER * C)
            return ms

        def evidence():
            t0 = time.perf_counter()
            table, n = run.evidence_table()
            ms = (time.perf_counter() - t0) * 1e3
            assert n == INNER and table[:, 0].sum() == 0
            return ms
        forms = dict(evidence=evidence, first_pass=first_pass)
        for f in forms.values():                            # warm-up: the context's scratch is allocated and kept
            f()
        t = {k: [] for k in forms}
        for _ in range(REPEATS):
            for k, f in forms.items():
                t[k].append(f())
        row = {}
        for k, v in t.items():
            v = np.array(v)
            row[k] = dict(ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), TBps=nbytes / (float(np.median(v)) * 1e-3) / 1e12)
        row["evidence_over_first_pass"] = row["evidence"]["ms"] / row["first_pass"]["ms"]
        row["tensor_bytes"] = nbytes
        row["log_z_ss"] = run.evidence()["log_z_ss"]
        out["chains_%d" % C] = row
        run.close()
    return out


def main(out):
    result = dict(dim=D, R=R, saved_draws=INNER, repeats=REPEATS, unit="wall milliseconds of one blocking call; TBps: bytes of the tensor per second")
    for dt in ("f64", "f32"):
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", dt], stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT_S)
        if done.returncode != 0:
            print("evidence_rate: the %s step ended with status %d; nothing more is started" % (dt, done.returncode), flush=True)
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
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "evidence_rate.json")))
