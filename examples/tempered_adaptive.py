#!/usr/bin/env python3
"""The bimodal posterior of examples/tempered_bimodal.py from a deliberately poor ladder -- and what the adaptive ladder makes of it.

The ladder 1, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 1e-4 crowds seven temperatures near the cold end and leaves one gap that no swap crosses: the
hottest rung, the only one that moves freely between the modes, is cut off, and the cold chains stay where they started.  With
`adapt=mhx.LadderAdaptation(steps)` every ladder moves its temperatures during the first `steps` transitions until each pair swaps at
about the target rate (0.234), inside the step kernel, and is frozen afterwards; the draws of those transitions are discarded.  (The
last gap is wider than the largest the adaptation allows, log beta apart by exp(rho_max) = 16 / 7: the adaptive run starts it there.)
On one MI355X the rank-normalised R-hat of the 256 cold chains goes from 1.126 (every chain still in the mode it started in) to 1.021
(every chain spends 30 % to 70 % of its draws in each mode).

    python examples/tempered_adaptive.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402
import mhx.trace as T  # noqa: E402

A = 4.0


def density(x):
    a = -0.5 * ((x[0] - A) ** 2 + (x[1] - A) ** 2)
    b = -0.5 * ((x[0] + A) ** 2 + (x[1] + A) ** 2)
    m = T.maximum(a, b)
    return m + T.log(T.exp(a - m) + T.exp(b - m))


model = mhx.DensityModel(density, dim=2)
spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(2), mhx.I))
NL, N, R, WARM = 256, 2000, 8, 2000
rng = np.random.default_rng(7)
start = np.where(rng.random(NL) < 0.5, -A, A)[None, :] + rng.normal(size=(2, NL))       # half the chains in each mode
ladder_start = np.repeat(start, R, axis=1)
poor = [1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 1e-4]

results = {}
for name, adapt in (("fixed", None), ("adaptive", mhx.LadderAdaptation(WARM))):
    results[name] = mhx.sample(model, mhx.Tempered(spl, poor, swap_every=2, adapt=adapt), N, NL, initial_params=ladder_start,
                               discard_initial=WARM, seed=11, param_names=["x", "y"])

print("the poor ladder, kept fixed: swaps between neighbouring temperatures")
print(results["fixed"].tempered.swap_rates())
print("\nthe same start, adapted over the first %d transitions (the rates include them):" % WARM)
print(results["adaptive"].tempered.swap_rates())
print("\nthe adapted ladders (temperatures over the %d ladders):" % NL)
print(results["adaptive"].tempered.ladder())
print("\nrank-normalised R-hat     fixed    adaptive")
for pname, a, b in zip(results["fixed"].rhat()["parameters"], results["fixed"].rhat()["rhat"], results["adaptive"].rhat()["rhat"]):
    print("%-22s %8.3f %11.3f" % (pname, a, b))
for name, chain in results.items():
    share = (chain["x"] > 0).mean(axis=0)
    print("%-9s share of the draws in the upper mode per cold chain: min %.2f max %.2f" % (name, share.min(), share.max()))
