#!/usr/bin/env python3
"""The log marginal likelihood (evidence) of two regression models from anchored tempering ladders, beside the closed form.

Data y_i = theta_0 + theta_1 x_i + noise, noise ~ N(0, sigma^2), prior theta ~ N(0, tau^2 I).  Model A has intercept and slope, model B
the intercept alone.  Both are linear-Gaussian, so the evidence is known: y ~ N(0, sigma^2 I + tau^2 X X').

`mhx.Tempered(..., reference=prior)` tempers from the posterior (beta = 1) to the prior itself (beta = 0): rung r samples
joint^beta * prior^(1 - beta), and the path integrates to log Z.  `chain.tempered.evidence()` returns thermodynamic integration over
the ladder (with ptemcee's every-other-rung check of the discretisation) and both stepping-stone estimates, each with its standard
error between the independent ladders; `mhx.bayes_factor` compares two models.

    python examples/tempered_evidence.py
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advancedmh.jl_amd"))
import mhx  # noqa: E402

SIGMA, TAU, NOBS = 0.5, 2.0, 24
rng = np.random.default_rng(3)
xs = np.linspace(-1.0, 1.0, NOBS)
ys = 0.7 + 0.4 * xs + SIGMA * rng.normal(size=NOBS)


def log_joint(columns):
    """log likelihood + log prior of the model whose design matrix has these columns, as a function the tracer reads"""
    d = len(columns)
    const = -NOBS * math.log(SIGMA * math.sqrt(2 * math.pi)) - d * math.log(TAU * math.sqrt(2 * math.pi))

    def f(theta):
        q = 0.0
        for i in range(NOBS):
            r = float(ys[i])
            for k in range(d):
                r = r - theta[k] * float(columns[k][i])
            q = q + r * r
        p = 0.0
        for k in range(d):
            p = p + theta[k] * theta[k]
        return const - (0.5 / SIGMA ** 2) * q - (0.5 / TAU ** 2) * p
    return f


def exact_log_evidence(columns):
    X = np.stack(columns, axis=1)
    S = SIGMA ** 2 * np.eye(NOBS) + TAU ** 2 * X @ X.T
    return -0.5 * (NOBS * math.log(2 * math.pi) + np.linalg.slogdet(S)[1] + ys @ np.linalg.solve(S, ys))


R, NL, N, WARM = 16, 256, 1000, 500
betas = mhx.power_betas(R, 3.0)
results = {}
for name, columns in (("A: intercept + slope", [np.ones(NOBS), xs]), ("B: intercept", [np.ones(NOBS)])):
    d = len(columns)
    X = np.stack(columns, axis=1)
    # the rung's own spread: posterior precision beta X'X / sigma^2 + I / tau^2, per parameter, relative to the cold rung
    prec = np.array([b * np.diag(X.T @ X) / SIGMA ** 2 + 1.0 / TAU ** 2 for b in betas])
    scales = np.sqrt(prec[0].mean() / prec.mean(axis=1))
    scales[0] = 1.0
    step = 2.4 / math.sqrt(d * prec[0].mean())
    spl = mhx.Tempered(mhx.RWMH(mhx.MvNormal(mhx.zeros(d), step * step * mhx.I)), betas, swap_every=1, scales=scales,
                       reference=mhx.MvNormal(mhx.zeros(d), TAU * TAU * mhx.I))
    chain = mhx.sample(mhx.DensityModel(log_joint(columns), dim=d), spl, N, NL, discard_initial=WARM, thinning=2, seed=5)
    ev = chain.tempered.evidence()
    results[name] = (ev, exact_log_evidence(columns))
    print("model %s" % name)
    print(ev)
    print("closed form            %.5f\n" % results[name][1])

(a, ea), (b, eb) = results["A: intercept + slope"], results["B: intercept"]
bf = mhx.bayes_factor(a, b)
print("log Bayes factor A over B: %.4f +- %.4f   closed form %.4f" % (bf["log_bf"], bf["se"], ea - eb))
