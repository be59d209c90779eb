#!/usr/bin/env python3
"""Time of the HPD intervals (mhx_run_hpd: radix select of the thresholds, one gather sweep, a sort of the tails only, the first
minimum width) on the tensor bench.py's flagship workload leaves on the device: C2 -- RWMH on the 100-dim
isotropic Gaussian, 65 536 chains, 250 saved draws each, [250][101][65536] -- in fp64 and fp32, alpha = 0.05, all 101 rows.

  call        one blocking Run.hpd() between two HIP events (torch.cuda.Event on the current stream: the call synchronises its own
              stream before it returns, so the span is what a caller waits for), median of REPEATS with minimum and maximum
  torch route the only other device route, in the same process, interleaved call by call: per row torch.sort of the flattened row,
              then the same widths and argmin in torch (fp64 of the widened ends); one copy of the 2 x 101 results at the end
  phases      the tools build of the library (option HPD_STOP_AFTER = 1 | 2 | 3: return after the select / the gather / the sort)
              on the same tensor through mhx_ctx_hpd; a phase is the difference of two medians.  Every phase ends in a
              synchronisation of its own in the full call as well, so the differences add up to the call.
  byte model  the select's passes (6 fp64, 3 fp32) plus the gather sweep over the tensor, against the call time

    bench_hpd.py [OUT.json]        default OUT: profiles/hpd_bench.json      env: C, INNER, REPEATS, ALPHA"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402

D, C, INNER, REPEATS = 100, int(os.environ.get("C", 65536)), int(os.environ.get("INNER", 250)), int(os.environ.get("REPEATS", 5))
ALPHA = float(os.environ.get("ALPHA", 0.05))


class _DeviceView:
    """a caller's device tensor for torch.as_tensor (no copy)"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2)


def _events(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def _stat(t):
    t = np.array(t, dtype=np.float64)
    return dict(ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))


def measure(dt):
    import torch
    s = float(np.float32(2.38 / D ** 0.5))
    ctx = mhx.Context.default(dtype=dt)
    run = mhx.Run(mhx.DensityModel(mhx.IsoGaussian(D)), mhx.RWMH(mhx.MvNormal(mhx.zeros(D), s * s * mhx.I)), nchains=C, seed=0xC0FFEE,
                  ctx=ctx, reduce_lanes=2)
    run.init(None)
    run.sample(INNER, 1, 1, 0)
    d1, S = D + 1, INNER * C
    m = mhx.hpd_ranks(S, ALPHA)
    keybytes = 8 if dt == "f64" else 4
    tensor_bytes = INNER * d1 * C * keybytes
    ptr, n_saved = ctypes.c_void_p(), ctypes.c_int64()
    mhx.check(mhx.lib().mhx_run_device_samples(run.h, ctypes.byref(ptr), None, ctypes.byref(n_saved)))
    assert n_saved.value == INNER
    try:                                                     # the run's own tensor, in place
        t = torch.as_tensor(_DeviceView(ptr.value, (INNER, d1, C), "<f8" if dt == "f64" else "<f4"), device="cuda:0")
        assert t.data_ptr() == ptr.value
    except Exception:                                        # ... or a copy of it through the host
        t = torch.from_numpy(run.samples()[0]).to("cuda:0")
    assert tuple(t.shape) == (INNER, d1, C)

    def torch_route():
        lo, up = [], []
        for p in range(d1):
            y = torch.sort(t[:, p, :].reshape(-1))[0]
            a, b = y[:m].double(), y[S - m:].double()
            i = torch.argmin(b - a)
            lo.append(a[i])
            up.append(b[i])
        return torch.stack(lo).cpu().numpy(), torch.stack(up).cpu().numpy()

    ref = run.hpd(ALPHA)                                     # warm-up: the context's scratch is allocated and kept
    tref = torch_route()
    torch.cuda.synchronize()
    ours, theirs = [], []
    for _ in range(REPEATS):
        ms, got = _events(torch, lambda: run.hpd(ALPHA))
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        ours.append(ms)
        ms, _ = _events(torch, torch_route)
        theirs.append(ms)
    row = dict(tensor_bytes=tensor_bytes, draws_per_row=S, rows=d1, alpha=ALPHA, m=m, tail_keys_bound_per_row=2 * (m - 1),
               scratch_mb_of_one_row=4.0 * (m - 1) * keybytes / 2.0 ** 20, hpd_of_row_0=[float(ref[0][0]), float(ref[1][0])],
               call=_stat(ours), torch_route=_stat(theirs),
               torch_route_gives_the_same_intervals=bool(np.array_equal(tref[0], ref[0]) and np.array_equal(tref[1], ref[1])))
    row["torch_route_over_call"] = row["torch_route"]["ms"] / row["call"]["ms"]
    sweeps = (6 if dt == "f64" else 3) + 1
    row["byte_model"] = dict(sweeps=sweeps, bytes=sweeps * tensor_bytes, implied_TBps_of_the_call=sweeps * tensor_bytes / (row["call"]["ms"] * 1e-3) / 1e12)

    # the phases: the tools build on the same device tensor
    mhx.use_library(mhx.TOOLS_LIB_PATH)
    try:
        tctx = mhx.Context(0, dt)
        params = np.arange(d1, dtype=np.int32)
        lower, upper = np.empty(d1), np.empty(d1)
        dp, i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)

        def upto(k):
            tctx.set_option("HPD_STOP_AFTER", k)
            mhx.check(mhx.lib().mhx_ctx_hpd(tctx.h, ptr, INNER, d1, C, params.ctypes.data_as(i32p), d1, ALPHA, lower.ctypes.data_as(dp),
                                            upper.ctypes.data_as(dp)))

        upto(0)                                              # warm-up of this context's scratch
        assert np.array_equal(lower, ref[0]) and np.array_equal(upper, ref[1])
        times = {k: [] for k in (1, 2, 3, 0)}
        for _ in range(REPEATS):
            for k in times:
                ms, _ = _events(torch, lambda: upto(k))
                times[k].append(ms)
        med = {k: float(np.median(v)) for k, v in times.items()}
        row["phases_ms"] = dict(select=med[1], gather=med[2] - med[1], sort=med[3] - med[2], argmin=med[0] - med[3], call_of_the_tools_build=med[0])
        tctx.close()
    finally:
        mhx.use_library()
    del t
    run.close()
    ctx.close()
    print(json.dumps({dt: row}), flush=True)
    return row


def main(out):
    result = dict(dim=D, nchains=C, saved_draws=INNER, repeats=REPEATS, alpha=ALPHA,
                  unit="milliseconds between two HIP events around one blocking call, median of `repeats`")
    for dt in ("f64", "f32"):
        result[dt] = measure(dt)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hpd_bench.json"))
