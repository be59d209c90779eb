#!/usr/bin/env python3
"""Time of the exact quantiles (mhx_run_order_statistics: histogram radix select) on the tensor bench.py's
flagship workload leaves on the device: C2 -- RWMH on the 100-dim isotropic Gaussian, 65 536 chains, 250 saved draws each,
[250][101][65536] -- in fp64 and fp32.

One call = Run.quantiles() of the 100 parameters at the default five probs (eleven distinct ranks per parameter -- j and j + 1 of
every prob and the top rank -- one batch).  The
call is blocking and host-driven (one synchronisation and one bucket scan on the host per pass), so its time is the wall time of
the call: kernels, the copies of the histograms and the scans together.  After one warm-up call the digit widths are timed in
turn (interleaved), REPEATS rounds; the median of each is reported with its minimum and maximum.
  implied bandwidth = passes x tensor bytes / time, passes = ceil(key bits / digit bits), as a fraction of the 6.3 TB/s copy
  ceiling of DESIGN.md section 7 (the floor model of a memory-bound pass, not the peak).  This is a LOWER bound of the bytes
  read: a form that holds fewer groups per launch than the ranks asked for (11 bits: 8) launches a pass twice for the parameters
  whose ranks have parted into more groups, and the second launch reads their rows again -- at most every pass but the first
  (`max_sweeps`, `max_implied_bandwidth_TBps`).
  The first pass alone (one group of all draws: sign and top exponent bits, where nearly all draws of a wave meet in a few bins)
  is timed through the per-pass building block mhx_run_select_histogram (`top_pass_ms`).
Times are host wall times, not HIP events: the call synchronises and scans on the host once per pass, and that is part of what
a caller waits for.
Context, not a bar: ess_bulk_tail of the same 100 parameters -- the rocPRIM sort per parameter that was the only device route to a
quantile before -- timed once after a warm-up on 2 parameters, in THIS build of the library (the select leaves its code as the
commit before it had it).

    bench_quantiles.py [OUT.json]        default OUT: profiles/quantiles_bench.json      env: C, INNER, REPEATS, WIDTHS"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402

D, C, INNER, REPEATS = 100, int(os.environ.get("C", 65536)), int(os.environ.get("INNER", 250)), int(os.environ.get("REPEATS", 5))
WIDTHS = [int(w) for w in os.environ.get("WIDTHS", "8,10,11").split(",")]
CEILING = 6.3e12
GROUPS_PER_LAUNCH = {8: 16, 10: 16, 11: 8}                   # the pre-built forms (csrc/mhx_api_diag.inc)


def measure(dt):
    s = float(np.float32(2.38 / D ** 0.5))
    ctx = mhx.Context.default(dtype=dt)
    run = mhx.Run(mhx.DensityModel(mhx.IsoGaussian(D)), mhx.RWMH(mhx.MvNormal(mhx.zeros(D), s * s * mhx.I)), nchains=C, seed=0xC0FFEE,
                  ctx=ctx, reduce_lanes=2)
    run.init(None)
    run.sample(INNER, 1, 1, 0)
    params = np.arange(D, dtype=np.int32)
    keybits = 64 if dt == "f64" else 32
    tensor_bytes = INNER * (D + 1) * C * (keybits // 8)

    def call(width):
        ctx.set_option("SELECT_BITS", width)
        t0 = time.perf_counter()
        q = run.quantiles(params=params)
        return (time.perf_counter() - t0) * 1e3, q

    _, ref = call(WIDTHS[-1])                                # warm-up: the context's scratch and page-locked landing buffer are allocated and kept
    times = {w: [] for w in WIDTHS}
    for _ in range(REPEATS):
        for w in WIDTHS:
            ms, q = call(w)
            assert np.array_equal(q, ref), "digit width %d selects other draws" % w
            times[w].append(ms)
    ctx.set_option("SELECT_BITS", None)

    def top_pass(width):
        """the first pass alone: one group per parameter, the top `width` bits of the key"""
        pf, ng = np.zeros(D, dtype=np.uint64), np.ones(D, dtype=np.int32)
        hist = np.zeros((D, 1 << width), dtype=np.uint64)
        i32p, u64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)
        t0 = time.perf_counter()
        mhx.check(mhx.lib().mhx_run_select_histogram(run.h, params.ctypes.data_as(i32p), D, pf.ctypes.data_as(u64p), ng.ctypes.data_as(i32p),
                                                     1, keybits - width, width, hist.ctypes.data_as(u64p)))
        ms = (time.perf_counter() - t0) * 1e3
        assert np.all(hist.sum(axis=1) == INNER * C)
        return ms, int(np.count_nonzero(hist[0]))

    nranks = 2 * len(mhx.api.DEFAULT_QUANTILE_PROBS) + 1
    row = dict(tensor_bytes=tensor_bytes, draws_per_parameter=INNER * C, quantiles_of_parameter_0=[float(x) for x in ref[0]], widths={})
    for w in WIDTHS:
        t = np.array(times[w])
        passes = -(-keybits // w)
        bw = passes * tensor_bytes / (float(np.median(t)) * 1e-3)
        max_sweeps = passes + (passes - 1) * (-(-nranks // GROUPS_PER_LAUNCH.get(w, 16)) - 1)
        top_pass(w)
        top = [top_pass(w) for _ in range(3)]
        row["widths"][str(w)] = dict(ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), passes=passes,
                                     implied_bandwidth_TBps=bw / 1e12, fraction_of_copy_ceiling=bw / CEILING, max_sweeps=max_sweeps,
                                     max_implied_bandwidth_TBps=bw / 1e12 * max_sweeps / passes,
                                     top_pass_ms=float(np.median([m for m, _ in top])), top_pass_bins_in_use=top[0][1],
                                     top_pass_TBps=tensor_bytes / (float(np.median([m for m, _ in top])) * 1e-3) / 1e12)
    run.ess_bulk_tail(params=params[:2])                     # warm-up of the sort route
    t0 = time.perf_counter()
    run.ess_bulk_tail(params=params)
    row["ess_bulk_tail_ms"] = (time.perf_counter() - t0) * 1e3
    best = min(WIDTHS, key=lambda w: row["widths"][str(w)]["ms"])
    row["fastest_width"] = best
    row["ess_bulk_tail_over_quantiles"] = row["ess_bulk_tail_ms"] / row["widths"][str(best)]["ms"]
    run.close()
    print(json.dumps({dt: row}), flush=True)
    return row


def main(out):
    result = dict(dim=D, nchains=C, saved_draws=INNER, repeats=REPEATS, probs=list(mhx.api.DEFAULT_QUANTILE_PROBS),
                  copy_ceiling_TBps=CEILING / 1e12, unit="wall milliseconds of one blocking Run.quantiles() call on 100 parameters")
    for dt in ("f64", "f32"):
        result[dt] = measure(dt)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "quantiles_bench.json"))
