#!/usr/bin/env python3
"""Time of the rank-normalised R-hat (mhx_run_rank_diagnostics: bulk and folded scores from ONE sort) next to
the call it extends, on the tensor bench.py's flagship workload leaves on the device: C2 -- RWMH on the 100-dim isotropic Gaussian,
65 536 chains -- with bench.py's ESS window (256 saved draws, rows 0, 50 and 99, max_lag 126, 512 chains for the autocovariances,
split chains) and with a larger buffer of the same run (1024 saved draws: 2^26 draws per row), in fp64 and fp32.

Three blocking calls on one run per shape, timed in turn (interleaved) REPEATS times after one warm-up round; the median of each is
reported with its minimum and maximum:
  rank_all   rank_diagnostics, all four outputs
  rank_ess   rank_diagnostics, the two ESS outputs only (the R-hat pointers NULL)
  ess        ess_bulk_tail, whose code is that of the commit before mhx_run_rank_diagnostics -- the yardstick
`rhat_extra_over_ess` = (rank_all - rank_ess) / ess: what the two R-hat outputs add, in units of one ess_bulk_tail call of the same
rows.  Below 1, the searches in the sorted array beat running the whole pipeline a second time on folded draws.
Times are host wall times of blocking calls (each ends in device synchronisations), not HIP events.

    bench_rank_diag.py [OUT.json]        default OUT: profiles/rank_diag_bench.json      env: C, DRAWS, REPEATS, DTYPES"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402

D, C, REPEATS = 100, int(os.environ.get("C", 65536)), int(os.environ.get("REPEATS", 7))
DRAWS = [int(n) for n in os.environ.get("DRAWS", "256,1024").split(",")]
DTYPES = os.environ.get("DTYPES", "f64,f32").split(",")
ROWS = sorted(set([0, D // 2, D - 1]))


def measure(dt, n_draws):
    s = float(np.float32(2.38 / D ** 0.5))
    run = mhx.Run(mhx.DensityModel(mhx.IsoGaussian(D)), mhx.RWMH(mhx.MvNormal(mhx.zeros(D), s * s * mhx.I)), nchains=C, seed=0xC0FFEE,
                  ctx=mhx.Context.default(dtype=dt), reduce_lanes=2)
    run.init(None)
    thin = max(1, int(round(40 * (D / 0.3) / 256)))          # bench.py's ESS window: draws `thin` transitions apart
    run.sample(n_draws, thin, thin, 0, save=True)
    kw = dict(params=ROWS, max_lag=n_draws // 2 - 2, ess_chains=512, split=True)
    calls = dict(rank_all=lambda: run.rank_diagnostics(**kw), rank_ess=lambda: run.rank_diagnostics(rhat=False, **kw),
                 ess=lambda: run.ess_bulk_tail(**kw))
    last = {k: f() for k, f in calls.items()}                # warm-up: code objects, rocPRIM's choice of kernels
    times = {k: [] for k in calls}
    for _ in range(REPEATS):
        for k, f in calls.items():
            t0 = time.perf_counter()
            last[k] = f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    run.close()
    for k in ("rank_all", "rank_ess"):                       # the same numbers up to the order of the fp64 atomics
        assert np.allclose(last[k]["ess_bulk"], last["ess"]["ess_bulk"], rtol=1e-6), (k, last[k]["ess_bulk"], last["ess"]["ess_bulk"])
    row = dict(draws=n_draws, chains=C, draws_per_row=n_draws * C, rows=ROWS, thin=thin)
    for k, t in times.items():
        t = np.array(t)
        row[k] = dict(ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))
    row["rhat_extra_ms"] = row["rank_all"]["ms"] - row["rank_ess"]["ms"]
    row["rhat_extra_over_ess"] = row["rhat_extra_ms"] / row["ess"]["ms"]
    row["rank_ess_over_ess"] = row["rank_ess"]["ms"] / row["ess"]["ms"]
    for k in ("rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail"):
        row[k] = [float(v) for v in last["rank_all"][k]]
    print(json.dumps({"%s_%d" % (dt, n_draws): row}), flush=True)
    return row


def main(out):
    result = dict(dim=D, nchains=C, repeats=REPEATS, unit="wall milliseconds of one blocking call on %d rows" % len(ROWS))
    for dt in DTYPES:
        for n in DRAWS:
            result["%s_%d" % (dt, n)] = measure(dt, n)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rank_diag_bench.json"))
