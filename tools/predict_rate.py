#!/usr/bin/env python3
"""Rate of predictive maps (mhx_run_predict, DESIGN.md sections 3.16 and 6.5.6) on the tensor bench.py's flagship workload leaves on
the device: C2 -- RWMH on the 100-dim isotropic Gaussian, 65 536 chains, 250 saved draws each, [250][101][65536] -- in fp64 and fp32
(the tensor of tools/derive_rate.py).

Four maps, each at 1, 2 and 4 draws per lane (option DERIVE_DRAWS; the library's default for predictive maps is marked):
  normal1    2 rows in, 1 out:    Normal(x0, |x1| + 0.5)
  normal8    16 rows in, 8 out:   Normal(x_k, |x_{k+8}| + 0.5), k = 0 .. 7
  gamma25    1 row in, 1 out:     Gamma(2.5, |x0| + 0.5)
  gamma05    1 row in, 1 out:     Gamma(0.5, |x0| + 0.5)       (the boosted branch: one more log and exp per draw)
Per form: the KERNEL time of the map's one launch from HIP events (mhx_run_stats.kernel_ms of the predictive run), median over
REPEATS rounds in which the forms alternate, with minimum and maximum; outputs per second (nout x n_saved x nchains / time); the
algorithmic bytes as derive counts them and their rate; and `of_identity`: the time of the identity `derive` of the same output
count (y_j = x_j: the same rows written, as many read -- the frame at a device copy's rate) over the map's time, same process, same
rounds.  What `of_identity` falls short of 1 by is the generator's arithmetic.
Nothing here gates anything: the tests do.

    predict_rate.py [OUT.json]        default OUT: profiles/predict_rate.json      env: C, INNER, REPEATS"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402
import mhx.trace as T  # noqa: E402

D, C, INNER, REPEATS = 100, int(os.environ.get("C", 65536)), int(os.environ.get("INNER", 250)), int(os.environ.get("REPEATS", 5))
DRAWS = (1, 2, 4)
DEFAULT_DRAWS = 1
MAPS = {        # name: (function, rows named)
    "normal1": (lambda t: mhx.Normal(t[0], abs(t[1]) + 0.5), 2),
    "normal8": (lambda t: [mhx.Normal(t[k], abs(t[k + 8]) + 0.5) for k in range(8)], 16),
    "gamma25": (lambda t: mhx.Gamma(2.5, abs(t[0]) + 0.5), 1),
    "gamma05": (lambda t: mhx.Gamma(0.5, abs(t[0]) + 0.5), 1),
}


def stat(t):
    t = np.array(t)
    return dict(ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))


def measure(dt):
    s = float(np.float32(2.38 / D ** 0.5))
    ctx = mhx.Context.default(dtype=dt)
    run = mhx.Run(mhx.DensityModel(mhx.IsoGaussian(D)), mhx.RWMH(mhx.MvNormal(mhx.zeros(D), s * s * mhx.I)), nchains=C, seed=0xC0FFEE,
                  ctx=ctx, reduce_lanes=2)
    run.init(None)
    run.sample(INNER, 1, 1, 0)
    size = 8 if dt == "f64" else 4
    row_bytes = INNER * C * size
    traced = {k: T.trace_predictive(f, D) for k, (f, _) in MAPS.items()}
    ident = {n: T.trace_map(lambda t, n=n: [t[k] for k in range(n)], D) for n in sorted({m.nout for m in traced.values()})}

    def kernel_ms(call, u=None):
        ctx.set_option("DERIVE_DRAWS", u)
        try:
            r = call()
        finally:
            ctx.set_option("DERIVE_DRAWS", None)
        ms = r.stats()["kernel_ms"]
        r.close()
        return ms

    forms = {}
    for name in MAPS:
        for u in DRAWS:
            forms["%s_u%d" % (name, u)] = lambda name=name, u=u: kernel_ms(lambda: run.predict(traced[name]), u)
    for n in ident:
        forms["identity%d" % n] = lambda n=n: kernel_ms(lambda: run.derive(ident[n]))
    if C * INNER <= 1 << 22:                                # (small shapes only: a rehearsal's check of the whole path)
        pre = run.predict(traced["normal1"])
        y = pre.samples()[0][:, 0, :].astype(np.float64)
        x = run.samples(want_accepted=False)[0].astype(np.float64)
        pre.close()
        z = (y - x[:, 0, :]) / (np.abs(x[:, 1, :]) + 0.5)
        assert np.isfinite(z).all() and abs(z.mean()) < 6 / np.sqrt(z.size) and abs(z.var() - 1) < 6 * np.sqrt(2 / z.size)
    for f in forms.values():                                # warm-up: every module compiled and loaded
        f()
    times = {k: [] for k in forms}
    for _ in range(REPEATS):
        for k, f in forms.items():
            times[k].append(f())
    out = dict(row_bytes=row_bytes, maps={}, identity={str(n): stat(times["identity%d" % n]) for n in ident})
    for name in MAPS:
        nout = traced[name].nout
        nbytes = (MAPS[name][1] + 1 + nout + 1) * row_bytes
        idn = out["identity"][str(nout)]
        m = dict(rows_in=MAPS[name][1], rows_out=nout, draws_per_output=1, bytes=nbytes, draws={})
        for u in DRAWS:
            st = stat(times["%s_u%d" % (name, u)])
            st.update(outputs_per_s=nout * INNER * C / (st["ms"] * 1e-3), TBps=nbytes / (st["ms"] * 1e-3) / 1e12, of_identity=idn["ms"] / st["ms"])
            m["draws"][str(u)] = st
        out["maps"][name] = m
    run.close()
    print(json.dumps({dt: out}), flush=True)
    return out


def main(out):
    result = dict(dim=D, nchains=C, saved_draws=INNER, repeats=REPEATS, default_draws_per_lane=DEFAULT_DRAWS,
                  unit="kernel milliseconds from HIP events; outputs_per_s = nout x n_saved x nchains / time; bytes = (rows named + lp + "
                       "nout + 1) x n_saved x nchains x sizeof(real); of_identity = time of the identity derive of nout outputs / time")
    for dt in ("f64", "f32"):
        result[dt] = measure(dt)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "predict_rate.json"))
