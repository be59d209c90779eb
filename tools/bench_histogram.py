#!/usr/bin/env python3
"""Time of the device histograms (mhx_run_histogram / mhx_run_histogram2d) on the tensor bench.py's flagship
workload leaves on the device: C2 -- RWMH on the 100-dim isotropic Gaussian, 65 536 chains, 250 saved draws each, [250][101][65536]
-- in fp64 and fp32.

What is timed is the HOST WALL time of one blocking call (kernel, copies of the edges and of the counters, the host's checks), after
a warm-up of every form; the forms are timed in turn (interleaved), REPEATS rounds, and the median of each is reported with its
minimum and maximum.  Edges are fixed up front (numpy's edges between each row's minimum and maximum, from one order-statistics call),
so a call is the sweep alone; `auto` is Run.histogram(range=None), which takes the minima and maxima itself first.
  first_pass        the yardstick, as old as the select: ONE first pass of the radix select at 11 bits over the same 101 rows
                    (mhx_run_select_histogram, shift = key bits - 11, one group per row) -- the same sweep with one LDS add per draw
                    and no bin search.  `over_first_pass` = histogram / first pass.
  hist_64, hist_2048   Run.histogram of all 101 rows at 64 and at 2048 uniform bins
  hist_64_one_bin   the 64-bin call over edges 64 times as wide as each row's range: ALL draws of ALL 101 rows in bin 0, so every lane of
                    every wave adds to one LDS counter -- the contention case at its worst; `one_bin_over_spread` = its time / hist_64's
  hist_64_const     the same 64-bin call after row 0 was overwritten with a constant on the device: every lane of every wave of
                    that row's blocks adds to ONE LDS counter (the contention case); `const_over_spread` = its time / hist_64's
  hist2d_32, hist2d_128   Run.histogram2d of the 45 pairs of rows 0..9; bytes = m (m - 1) rows = 90 rows, as TB/s against the
                    6.3 TB/s copy ceiling of DESIGN.md section 7
Nothing here gates anything: the exact tests do.

    bench_histogram.py [OUT.json]        default OUT: profiles/histogram_bench.json      env: C, INNER, REPEATS"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402

D, C, INNER, REPEATS = 100, int(os.environ.get("C", 65536)), int(os.environ.get("INNER", 250)), int(os.environ.get("REPEATS", 7))
CEILING = 6.3e12
PAIR_ROWS = 10


def overwrite_row_with_zero(run, row, width_bytes):
    """row `row` of the run's [INNER][D + 1][C] device tensor := 0.0, through the HIP runtime the library already loaded"""
    ptr = ctypes.c_void_p()
    mhx.check(mhx.lib().mhx_run_device_samples(run.h, ctypes.byref(ptr), None, None))
    hip = ctypes.CDLL(None)
    hip.hipMemset2D.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t]
    hip.hipDeviceSynchronize.argtypes = []
    pitch, width = (D + 1) * C * width_bytes, C * width_bytes
    rc = hip.hipMemset2D(ctypes.c_void_p(ptr.value + row * width), pitch, 0, width, INNER)      # the last byte: (INNER - 1) pitch + (row + 1) width
    return rc == 0 and hip.hipDeviceSynchronize() == 0


def measure(dt):
    s = float(np.float32(2.38 / D ** 0.5))
    ctx = mhx.Context.default(dtype=dt)
    run = mhx.Run(mhx.DensityModel(mhx.IsoGaussian(D)), mhx.RWMH(mhx.MvNormal(mhx.zeros(D), s * s * mhx.I)), nchains=C, seed=0xC0FFEE,
                  ctx=ctx, reduce_lanes=2)
    run.init(None)
    run.sample(INNER, 1, 1, 0)
    rows = np.arange(D + 1, dtype=np.int32)
    keybits = 64 if dt == "f64" else 32
    row_bytes = INNER * C * (keybits // 8)
    S = INNER * C
    ends = run.order_statistics([0, S - 1])
    edges = {b: np.stack([mhx.histogram_edges(lo, hi, b) for lo, hi in ends]) for b in (32, 64, 128, 2048)}

    def first_pass():
        pf, ng = np.zeros(D + 1, dtype=np.uint64), np.ones(D + 1, dtype=np.int32)
        hist = np.zeros((D + 1, 1 << 11), dtype=np.uint64)
        i32p, u64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)
        t0 = time.perf_counter()
        mhx.check(mhx.lib().mhx_run_select_histogram(run.h, rows.ctypes.data_as(i32p), D + 1, pf.ctypes.data_as(u64p), ng.ctypes.data_as(i32p),
                                                     1, keybits - 11, 11, hist.ctypes.data_as(u64p)))
        ms = (time.perf_counter() - t0) * 1e3
        assert np.all(hist.sum(axis=1) == S)
        return ms

    wide = np.stack([mhx.histogram_edges(lo, lo + 64.5 * (hi - lo), 64) for lo, hi in ends])

    def hist(bins, auto=False, one_bin=False):
        t0 = time.perf_counter()
        counts, _, outside = run.histogram(bins=bins) if auto else run.histogram(edges=wide if one_bin else edges[bins])
        ms = (time.perf_counter() - t0) * 1e3
        assert np.all(counts.sum(axis=1) + outside.sum(axis=1) == S) and (not one_bin or np.all(counts[:, 0] == S))
        return ms

    def hist2d(bins):
        t0 = time.perf_counter()
        counts, _, outside, pairs = run.histogram2d(params=rows[:PAIR_ROWS], bins=bins, edges=edges[bins][:PAIR_ROWS])
        ms = (time.perf_counter() - t0) * 1e3
        assert len(pairs) == PAIR_ROWS * (PAIR_ROWS - 1) // 2 and np.all(counts.sum(axis=(1, 2)) + outside == S)
        return ms

    forms = dict(first_pass=first_pass, hist_64=lambda: hist(64), hist_2048=lambda: hist(2048), hist_64_auto=lambda: hist(64, True),
                 hist_64_one_bin=lambda: hist(64, one_bin=True),
                 hist2d_32=lambda: hist2d(32), hist2d_128=lambda: hist2d(128))
    for f in forms.values():                                # warm-up: the context's scratch is allocated and kept
        f()
    times = {k: [] for k in forms}
    for _ in range(REPEATS):
        for k, f in forms.items():
            times[k].append(f())
    # the contention case: row 0 constant, the same edges, beside the spread rows -- in rounds of its own with the spread form
    spread, const = [], []
    before = run.histogram(params=[0, 1], edges=edges[64][:2])[0]
    if overwrite_row_with_zero(run, 0, keybits // 8):
        after = run.histogram(params=[0, 1], edges=edges[64][:2])[0]
        assert np.count_nonzero(after[0]) == 1 and after[0].sum() == S and np.array_equal(after[1], before[1])
        hist(64)
        for _ in range(REPEATS):
            const.append(hist(64))
        # one row alone, constant against spread: the slowdown of the blocks that meet the contention, not diluted by 100 other rows
        one = {}
        for name, r in (("const", 0), ("spread", 1)):
            run.histogram(params=[r], edges=edges[64][r:r + 1])
            ts = []
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                run.histogram(params=[r], edges=edges[64][r:r + 1])
                ts.append((time.perf_counter() - t0) * 1e3)
            one[name] = float(np.median(ts))
    else:
        one = None

    def stat(t):
        t = np.array(t)
        return dict(ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))

    row = dict(tensor_bytes=(D + 1) * row_bytes, row_bytes=row_bytes, draws_per_row=S, forms={k: stat(t) for k, t in times.items()})
    fp = row["forms"]["first_pass"]["ms"]
    for k in ("hist_64", "hist_2048", "hist_64_auto", "hist_64_one_bin"):
        row["forms"][k]["over_first_pass"] = row["forms"][k]["ms"] / fp
        row["forms"][k]["TBps"] = (D + 1) * row_bytes / (row["forms"][k]["ms"] * 1e-3) / 1e12
    row["forms"]["hist_64_one_bin"]["one_bin_over_spread"] = row["forms"]["hist_64_one_bin"]["ms"] / row["forms"]["hist_64"]["ms"]
    row["forms"]["first_pass"]["TBps"] = (D + 1) * row_bytes / (fp * 1e-3) / 1e12
    for k in ("hist2d_32", "hist2d_128"):
        bw = PAIR_ROWS * (PAIR_ROWS - 1) * row_bytes / (row["forms"][k]["ms"] * 1e-3)
        row["forms"][k].update(rows_read=PAIR_ROWS * (PAIR_ROWS - 1), TBps=bw / 1e12, fraction_of_copy_ceiling=bw / CEILING)
    if const:
        row["forms"]["hist_64_const"] = stat(const)
        row["forms"]["hist_64_const"]["const_over_spread"] = row["forms"]["hist_64_const"]["ms"] / row["forms"]["hist_64"]["ms"]
        row["one_row_64_bins_ms"] = dict(one, const_over_spread=one["const"] / one["spread"])
    else:
        row["forms"]["hist_64_const"] = "NOT MEASURED"
    run.close()
    print(json.dumps({dt: row}), flush=True)
    return row


def main(out):
    result = dict(dim=D, nchains=C, saved_draws=INNER, repeats=REPEATS, copy_ceiling_TBps=CEILING / 1e12, pair_rows=PAIR_ROWS,
                  unit="wall milliseconds of one blocking call")
    for dt in ("f64", "f32"):
        result[dt] = measure(dt)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "histogram_bench.json"))
