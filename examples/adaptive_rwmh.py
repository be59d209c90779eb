#!/usr/bin/env python3
"""A Gaussian whose four coordinates have standard deviations 0.1, 1, 10 and 100, sampled by a random walk whose proposal is a guess
(unit steps in every coordinate) -- and by the same random walk with `adapt=mhx.ProposalAdaptation(steps, shape=True)`.

The guess is rejected on the narrow coordinate and barely moves on the wide one.  With `adapt`, every chain tunes its own proposal
during the first `steps` transitions, inside the step kernel: a log-scale driven towards an acceptance rate of 0.234 and a standard
deviation per coordinate that follows the chain's own running variance; afterwards the proposal is frozen and the chain is a plain
random walk.  The draws of the adapting transitions are discarded.  On one MI355X (256 chains, 4000 draws each after 2000 adapting
transitions) the acceptance rate goes from 0.102 to 0.229 and the bulk ESS of the widest coordinate from 554 to 70 408; the learned
standard deviations have medians 0.143, 1.40, 14.2 and 142 over the chains.

    python examples/adaptive_rwmh.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402

SDS = np.array([0.1, 1.0, 10.0, 100.0])
model = mhx.DensityModel(mhx.CorrGaussian(np.diag(SDS ** 2)))
guess = mhx.MvNormal(mhx.zeros(4), mhx.I)
NCHAINS, N, WARM = 256, 4000, 2000

for name, adapt in (("fixed", None), ("adapted", mhx.ProposalAdaptation(WARM, shape=True))):
    run = mhx.Run(model, mhx.RWMH(guess, adapt=adapt), nchains=NCHAINS, seed=11)
    run.init()
    run.sample(N, WARM, 1, 0)
    if adapt is None:
        rate = run.stats()["accepted"] / run.stats()["transitions"]
    else:
        table = run.adaptation(["x1", "x2", "x3", "x4"])
        rate = table.accept_rate
        print("the proposal every chain froze at (true sds %s; the optimal scale of a 4-d random walk is 2.38 / sqrt(4) = 1.19 of them):" % SDS.tolist())
        print(table)
    ess = run.ess_bulk_tail(params=[3])["ess_bulk"][0]
    print("%-8s acceptance rate %.3f, ess_bulk of the widest coordinate %.0f of %d draws\n" % (name, rate, ess, NCHAINS * N))
    run.close()
