#!/usr/bin/env python3
"""A bimodal posterior, where a random walk stays in the mode it started in -- and what parallel tempering does about it.

The target is an equal mixture of N((-4, -4), I) and N((+4, +4), I), written as a closure and traced into kernel source.  256 plain
RWMH chains start around both modes and never cross: the device R-hat says so.  The same 256 chains as the cold rungs of 256 ladders
of 8 temperatures (mhx.Tempered: what MCMCTempering.jl wraps around AdvancedMH's samplers) exchange states with their hotter
neighbours inside the step kernel, and every cold chain visits both modes.

    python examples/tempered_bimodal.py
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
NL, N, R = 256, 2000, 8
rng = np.random.default_rng(7)
start = np.where(rng.random(NL) < 0.5, -A, A)[None, :] + rng.normal(size=(2, NL))       # half the chains in each mode

plain = mhx.sample(model, spl, N, NL, initial_params=start, discard_initial=500, seed=11, param_names=["x", "y"])

betas = mhx.geometric_betas(R, 0.02)
ladder_start = np.repeat(start, R, axis=1)                                             # every rung of a ladder starts where its cold chain does
tempered = mhx.sample(model, mhx.Tempered(spl, betas, swap_every=2), N, NL, initial_params=ladder_start, discard_initial=500, seed=11,
                      param_names=["x", "y"])

print("plain RWMH, %d chains:" % NL)
print(plain.describe(rhat_kind="rank"))
print("\ntempered, the cold rungs of %d ladders of %d temperatures:" % (NL, R))
print(tempered.describe(rhat_kind="rank"))
print("\nrank-normalised R-hat     plain    tempered")
for name, a, b in zip(plain.rhat()["parameters"], plain.rhat()["rhat"], tempered.rhat()["rhat"]):
    print("%-22s %8.3f %11.3f" % (name, a, b))
print("\nshare of the draws in the upper mode per chain: plain min %.2f max %.2f, tempered min %.2f max %.2f" % (
    (plain["x"] > 0).mean(axis=0).min(), (plain["x"] > 0).mean(axis=0).max(),
    (tempered["x"] > 0).mean(axis=0).min(), (tempered["x"] > 0).mean(axis=0).max()))
print("\nswaps between neighbouring temperatures:")
print(tempered.tempered.swap_rates())
print("\nacceptance rate per temperature:", np.round(tempered.tempered.accept_rates(), 3))
hot = tempered.tempered.rung(R - 1)
print("the hottest rung (beta = %.3g) as a run of its own: quantiles of x" % betas[-1], np.round(hot.quantiles((0.05, 0.5, 0.95), params=[0])[0], 2))
