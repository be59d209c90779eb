#!/usr/bin/env python3
"""Time of the device cross moments (mhx_ctx_cross_moments: SYRK over all draws on the fp64 matrix cores) at
the shape bench.py's flagship workload leaves on the device -- [250][101][65536], all 101 rows -- on an fp64 and an fp32 tensor of
standard normals, beside the only other device-side route a user has: torch.einsum('npc,nqc->pq') in fp64 on the same tensor, in the
same process, interleaved.

One call of either is timed two ways: HIP events recorded on torch's stream before and after (the mhx call is blocking -- it ends in
a device synchronise and the copy of 101 x 102 doubles -- so both events are taken on an idle device and span exactly the call), and
the host clock around the call plus a synchronise.  After one warm-up of each (the context's scratch is allocated and kept; the
library picks its algorithm) REPEATS rounds alternate the two; medians with minimum and maximum are reported.
  bytes          the tensor once: 13.24 GB (fp64), 6.62 GB (fp32)
  GB/s           bytes / time, and its fraction of the 6.3 TB/s copy ceiling of DESIGN.md section 7
  MFMA           v_mfma_f64_16x16x4_f64 issued: tile pairs (28 at 7 row tiles) x K / 4; at 64 cycles each per SIMD (2048 flop; the
                 part's 78.6 TFLOP/s fp64 matrix peak over 1024 SIMDs at 2.4 GHz) the least time the matrix pipes need
Small m: the same call on the first m rows, m = 1, 2, 4, 8, 16, 17, 32, 48, 64 (what a crossover to a lane-reduction form would be
judged by).

    bench_cross_moments.py [OUT.json]      default OUT: profiles/cross_moments_bench.json      env: N, C, REPEATS"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402

D1, C, N, REPEATS = 101, int(os.environ.get("C", 65536)), int(os.environ.get("N", 250)), int(os.environ.get("REPEATS", 5))
CEILING, SIMDS, CLOCK, MFMA_CYCLES = 6.3e12, 1024, 2.4e9, 64
SMALL_M = (1, 2, 4, 8, 16, 17, 32, 48, 64)
DP = ctypes.POINTER(ctypes.c_double)


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    ms = np.asarray(ms)
    return dict(ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()))


def measure(torch, dt):
    tdt = torch.float64 if dt == "f64" else torch.float32
    ctx = mhx.Context.default(dtype=dt)
    gen = torch.Generator(device="cuda:0").manual_seed(1234)
    t = torch.empty((N, D1, C), dtype=tdt, device="cuda:0")
    for n in range(N):                                       # sample by sample: no second tensor of that size
        t[n] = torch.randn((D1, C), generator=gen, dtype=tdt, device="cuda:0")
    torch.cuda.synchronize()
    nbytes, K = t.numel() * t.element_size(), N * C

    def moments(m=D1):
        params = np.arange(m, dtype=np.int32)
        s, x = np.empty(m), np.empty((m, m))
        mhx.check(mhx.lib().mhx_ctx_cross_moments(ctx.h, ctypes.c_void_p(t.data_ptr()), N, D1, C, params.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                  m, None, s.ctypes.data_as(DP), x.ctypes.data_as(DP)))
        return s, x

    def einsum():
        a = t if dt == "f64" else t.double()                 # fp64 sums of an fp32 tensor: the conversion is part of the route
        return torch.einsum("npc,nqc->pq", a, a)

    (_, x0), ref = moments(), einsum()                       # warm-up of both
    torch.cuda.synchronize()
    rel = float((torch.from_numpy(x0).to("cuda:0") - ref).abs().max() / ref.abs().max())
    ours, base = [], []
    for _ in range(REPEATS):
        ours.append(timed(torch, moments)[:2])
        base.append(timed(torch, einsum)[:2])
    tiles = (D1 + 15) // 16
    n_mfma = tiles * (tiles + 1) // 2 * (K // 4)
    o_ev, o_wall, b_ev, b_wall = stats([a for a, _ in ours]), stats([b for _, b in ours]), stats([a for a, _ in base]), stats([b for _, b in base])
    row = dict(tensor_bytes=nbytes, draws=K, rows=D1,
               cross_moments=dict(hip_events=o_ev, host_clock=o_wall, GBps=nbytes / (o_ev["ms"] * 1e-3) / 1e9,
                                  fraction_of_copy_ceiling=nbytes / (o_ev["ms"] * 1e-3) / CEILING, mfma_f64_16x16x4=n_mfma,
                                  mfma_floor_ms=n_mfma * MFMA_CYCLES / (SIMDS * CLOCK) * 1e3,
                                  fraction_of_mfma_issue_rate=n_mfma * MFMA_CYCLES / (SIMDS * CLOCK) * 1e3 / o_ev["ms"]),
               einsum_fp64=dict(hip_events=b_ev, host_clock=b_wall, GBps=nbytes / (b_ev["ms"] * 1e-3) / 1e9),
               einsum_over_cross_moments=b_ev["ms"] / o_ev["ms"], max_abs_difference_over_max_abs=rel, small_m={})
    for m in SMALL_M:
        moments(m)
        ms = [timed(torch, lambda: moments(m))[0] for _ in range(3)]
        row["small_m"][str(m)] = dict(ms=float(np.median(ms)), GBps_of_the_rows_read=nbytes * m / D1 / (float(np.median(ms)) * 1e-3) / 1e9)
    del t, ref
    torch.cuda.empty_cache()
    print(json.dumps({dt: row}), flush=True)
    return row


def main(out):
    import torch
    result = dict(shape=[N, D1, C], repeats=REPEATS, copy_ceiling_TBps=CEILING / 1e12,
                  unit="milliseconds of one blocking mhx_ctx_cross_moments call on all rows / of one torch.einsum('npc,nqc->pq') in fp64")
    for dt in ("f64", "f32"):
        result[dt] = measure(torch, dt)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cross_moments_bench.json"))
