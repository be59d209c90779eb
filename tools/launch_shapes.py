"""One tiny run per launch arm of the step kernels, in both widths, through the public Python API only.

    rocprofv3 --kernel-trace -d OUT -- python tools/launch_shapes.py [path/to/libmhx.so]

The kernel trace of this script lists kernel name, grid and workgroup of every launch, and a library built with tools/launch_log.h
logs the dynamic LDS bytes of each beside it (MHX_LAUNCH_LOG=file): two builds of the library whose device code is the same compute
the same chains exactly when those lists are equal (tools/launch_trace.py joins and compares them; the pair of
profiles/launch_record/ was taken this way).  Chain counts leave a partial last wave and a partial last block; where a grid is rounded
to whole rounds of 8 blocks the unrounded count is no multiple of 8.  The script prints one line per arm: the form the run took and
its launch count -- an arm a width does not have says why."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "advancedmh.jl_amd"), os.path.join(ROOT, "tests")]
import mhx  # noqa: E402
import user_targets  # noqa: E402

if len(sys.argv) > 1:
    mhx.use_library(os.path.abspath(sys.argv[1]))

RW, ST, MH = mhx.RandomWalkProposal, mhx.StaticProposal, mhx.MetropolisHastings


def ar1(d, rho):
    return rho ** np.abs(np.subtract.outer(np.arange(d), np.arange(d)))


def spd(d):
    """a covariance whose precision factor has no zero below the diagonal"""
    A = np.random.default_rng(d).normal(size=(d, d)) / d ** 0.5
    return A @ A.T + np.eye(d)


def iso(d, s=0.5, mean=None):
    return MH(RW(mhx.MvNormal(mhx.zeros(d) if mean is None else mean, s * s * mhx.I)))


def user(d):
    return mhx.HipLogDensity(user_targets.SHIFTED_GAUSS, d, data=np.r_[np.zeros(d), np.ones(d)])


def user_grad(d):
    return mhx.HipLogDensity(user_targets.SHIFTED_GAUSS_WITH_GRADIENT, d, data=np.r_[np.zeros(d), np.ones(d)])


def ens(d, W):
    return mhx.Ensemble(W, mhx.StretchProposal(mhx.MvNormal(mhx.zeros(d), mhx.I)))


FAM = [mhx.Normal(0, 1), mhx.Laplace(0, 2), mhx.Cauchy(0, 0.5)]
COND = lambda x: [mhx.Normal(0, 0.5 + abs(x[1])), mhx.Laplace(0, 0.5 + abs(x[0]))]       # noqa: E731
G, ZIG = mhx.FLAG_GENERIC, dict(normal_gen="ziggurat")
DATA = np.linspace(-1.0, 2.0, 16)
RAM = mhx.RobustAdaptiveMetropolis


def arms(real):
    """(name, target spec, sampler, chains, Run keywords, options, needs an initial state, save mode)"""
    f64 = real == "f64"
    big = 64 if f64 else 32                              # lanes per chain of the pre-built d = 1000 kernels
    lean = 330 if f64 else 512
    A = []

    def arm(name, spec, spl, C, kw=None, opts=None, init=False, save=True):
        A.append((name, spec, spl, C, kw or {}, opts or {}, init, save))
    # ---- RWMH
    arm("rwmh wave K=4", mhx.IIDNormal(DATA), iso(2), 5, dict(reduce_lanes=64), {"WAVE_K": 4})
    arm("rwmh wave K=8", mhx.IIDNormal(DATA), iso(2), 5, dict(reduce_lanes=64), {"WAVE_K": 8})
    arm("rwmh coop pre-built", mhx.IsoGaussian(100), iso(100, 0.2), 130, dict(reduce_lanes=2))
    arm("rwmh coop pre-built L>=32", mhx.Funnel(1000), iso(1000, 0.05), 20, dict(reduce_lanes=big))
    arm("rwmh coop run-time L=1", mhx.IsoGaussian(8), iso(8, 0.5, np.full(8, 0.1)), 130, dict(reduce_lanes=1))
    arm("rwmh coop run-time L=2", mhx.IsoGaussian(40), iso(40, 0.3), 130, dict(reduce_lanes=2))
    arm("rwmh coop run-time L=32", mhx.IsoGaussian(128), iso(128, 0.2), 20, dict(reduce_lanes=32))
    arm("rwmh coop ziggurat, pairs pre-built", mhx.IsoGaussian(100), iso(100, 0.2), 130, dict(reduce_lanes=2, **ZIG), {"COOP_PAIRS": 1})
    arm("rwmh coop ziggurat, pairs run-time", mhx.IsoGaussian(100), iso(100, 0.2), 130, dict(reduce_lanes=2, **ZIG), {"COOP_PAIRS": 1, "NO_PREBUILT": 1})
    arm("rwmh coop ziggurat, one wave", mhx.IsoGaussian(100), iso(100, 0.2), 130, dict(reduce_lanes=2, **ZIG), {"COOP_PAIRS": 0})
    arm("rwmh moments twin pre-built", mhx.Funnel(1000), iso(1000, 0.05), 20, dict(reduce_lanes=big), save="moments")
    arm("rwmh moments twin run-time", mhx.IsoGaussian(40), iso(40, 0.3), 130, dict(reduce_lanes=2), save="moments")
    arm("rwmh moments twin run-time of a pre-built kernel", mhx.IsoGaussian(100), iso(100, 0.2), 130, dict(reduce_lanes=2), save="moments")
    arm("rwmh moments twin of wave pairs", mhx.IsoGaussian(100), iso(100, 0.2), 130, dict(reduce_lanes=2, **ZIG), {"COOP_PAIRS": 1}, save="moments")
    arm("rwmh matrix-core resident", mhx.CorrGaussian(ar1(32, 0.6)), iso(32, 0.3), 65)
    arm("rwmh matrix-core streamed", mhx.CorrGaussian(ar1(200, 0.6)), MH(RW(mhx.MvNormal(mhx.zeros(200), 0.01 * ar1(200, 0.4)))), 65, dict(reduce_lanes=4))
    arm("rwmh dense cooperative", mhx.CorrGaussian(ar1(70, 0.6)), iso(70, 0.2), 33, dict(reduce_lanes=8))
    arm("rwmh register pre-built", mhx.IIDNormal(DATA), iso(2), 130, dict(reduce_lanes=1))
    arm("rwmh register run-time", mhx.IsoGaussian(7), iso(7), 130, dict(reduce_lanes=1))
    arm("rwmh register run-time, state tail in LDS", mhx.IsoGaussian(150), iso(150, 0.2), 130, dict(reduce_lanes=1))
    arm("rwmh register ziggurat", mhx.CorrGaussian(ar1(8, 0.6)), iso(8), 130, ZIG)
    arm("rwmh generic", mhx.IsoGaussian(7), iso(7), 300, dict(flags=G))
    arm("rwmh generic moments", mhx.IsoGaussian(7), iso(7), 300, dict(flags=G), save="moments")
    arm("rwmh user generic", user(5), iso(5), 300, dict(flags=G))
    # ---- family, conditional, composite proposals
    arm("family register", mhx.IsoGaussian(3), MH(RW(FAM)), 130)
    arm("family generic", mhx.IsoGaussian(3), MH(RW(FAM)), 300, dict(flags=G))
    arm("family user generic", user(3), MH(RW(FAM)), 300, dict(flags=G))
    arm("conditional register", mhx.IsoGaussian(2), MH(RW(COND, dim=2)), 130, init=True)
    arm("conditional generic", mhx.IsoGaussian(2), MH(RW(COND, dim=2)), 300, dict(flags=G), init=True)
    arm("composite register", mhx.IsoGaussian(3), MH([RW(COND, dim=2), ST(mhx.Normal(0, 1))]), 130, init=True)
    arm("composite generic", mhx.IsoGaussian(3), MH([RW(COND, dim=2), ST(mhx.Normal(0, 1))]), 300, dict(flags=G), init=True)
    # ---- MALA
    arm("mala generic", mhx.IsoGaussian(5), mhx.MALA(0.3), 300, dict(flags=G), init=True)
    arm("mala user generic", user_grad(5), mhx.MALA(0.3), 300, dict(flags=G), init=True)
    arm("mala register", mhx.IsoGaussian(5), mhx.MALA(0.3), 300, init=True)
    arm("mala register split", mhx.IsoGaussian(60), mhx.MALA(0.05), 130, dict(reduce_lanes=1), init=True)
    arm("mala register ziggurat", mhx.IsoGaussian(5), mhx.MALA(0.3), 130, ZIG, init=True)
    arm("mala cooperative", mhx.IsoGaussian(60), mhx.MALA(0.05), 130, dict(reduce_lanes=4), init=True)
    arm("mala matrix-core resident", mhx.CorrGaussian(ar1(32, 0.6)), mhx.MALA(0.1), 65, dict(reduce_lanes=4), init=True)
    arm("mala matrix-core streamed", mhx.CorrGaussian(ar1(200, 0.6)), mhx.MALA(0.02), 65, dict(reduce_lanes=4), init=True)
    arm("mala matrix-core lean", mhx.CorrGaussian(ar1(lean, 0.6)), mhx.MALA(0.01), 65, dict(reduce_lanes=4), init=True)
    # ---- RAM: a wave holds 4 chains at d = 6 (5 waves: 8 blocks), one at d = 40 and in the deferred form
    arm("ram sweep", mhx.IsoGaussian(6), RAM(), 20)
    arm("ram sweep, dense target", mhx.CorrGaussian(ar1(40, 0.6)), RAM(), 13)
    arm("ram sweep, user target", user(6), RAM(), 20)
    arm("ram deferred", mhx.IsoGaussian(6), RAM(deferred_factor=True), 13)
    arm("ram sweep with RAM_LDS_PAD", mhx.IsoGaussian(6), RAM(), 20, opts={"RAM_LDS_PAD": 70000})
    arm("ram sweep with RAM_G", mhx.IsoGaussian(6), RAM(), 20, opts={"RAM_G": 32})
    # ---- ensembles (`chains` = ensembles of 130 walkers)
    one_half = {"EMCEE_FUSED": 0, "EMCEE_PERSIST": 0}
    arm("emcee sequential", mhx.IsoGaussian(5), ens(5, 130), 1, dict(flags=mhx.FLAG_EMCEE_SEQUENTIAL))
    arm("emcee sequential, user target, 3 ensembles", user(5), ens(5, 130), 3, dict(flags=mhx.FLAG_EMCEE_SEQUENTIAL))
    arm("emcee half steps, pre-built", mhx.IsoGaussian(5), ens(5, 130), 1, dict(flags=G))
    arm("emcee half steps, lane per walker", mhx.IsoGaussian(5), ens(5, 130), 1, opts=one_half)
    arm("emcee half steps, lane per walker, preloaded", mhx.IsoGaussian(5), ens(5, 130), 1, opts=dict(one_half, EMCEE_PRELOAD=1))
    arm("emcee half steps, lane per walker, 3 ensembles", mhx.IsoGaussian(5), ens(5, 130), 3, opts=one_half)
    arm("emcee half steps, cooperative (band)", mhx.CorrGaussian(ar1(12, 0.6)), ens(12, 130), 1, opts=one_half)
    arm("emcee half steps, cooperative (dense)", mhx.CorrGaussian(spd(12)), ens(12, 130), 1, opts=dict(one_half, EMCEE_SCALAR=0, EMCEE_MFMA=0))
    arm("emcee half steps, scalar-factor", mhx.CorrGaussian(spd(12)), ens(12, 130), 1, opts=dict(one_half, EMCEE_MFMA=0))
    arm("emcee half steps, matrix-core", mhx.CorrGaussian(spd(12)), ens(12, 130), 1, opts=dict(one_half, EMCEE_MFMA=1))
    arm("emcee sweep, lane per walker", mhx.IsoGaussian(5), ens(5, 130), 1, opts={"EMCEE_FUSED": 1, "EMCEE_PERSIST": 0})
    arm("emcee sweep, cooperative (band)", mhx.CorrGaussian(ar1(12, 0.6)), ens(12, 130), 1, opts={"EMCEE_FUSED": 1})
    arm("emcee sweep, scalar-factor", mhx.CorrGaussian(spd(12)), ens(12, 130), 1, opts={"EMCEE_FUSED": 1, "EMCEE_MFMA": 0})
    arm("emcee sweep, matrix-core, 3 ensembles", mhx.CorrGaussian(spd(12)), ens(12, 130), 3, opts={"EMCEE_FUSED": 1, "EMCEE_MFMA": 1})
    arm("emcee persistent block", mhx.IsoGaussian(5), ens(5, 130), 1)
    arm("emcee persistent block, 3 ensembles", mhx.IsoGaussian(5), ens(5, 130), 3)
    return A


def main():
    for real in ("f64", "f32"):
        for name, spec, spl, C, kw, opts, init, save in arms(real):
            mhx.clear_options()
            for k, v in opts.items():
                mhx.set_option(k, v)
            try:
                run = mhx.Run(mhx.DensityModel(spec), spl, nchains=C, seed=11, first_chain=3, dtype=real, **kw)
                run.init(0.1 * np.random.default_rng(5).normal(size=(run.dim, run.n)) if init else None)
                run.sample(5, 1, 2, 0, save=save)               # 9 transitions, 5 records
                st = run.stats()
                print("%s | %-52s | %-14s variant %2d, %2d lane(s), %s, %d launch(es)" % (
                    real, name, run.form_name(), st["kernel_variant"], st["reduce_lanes"], "ziggurat" if st["normal_gen"] else "box-muller", st["launches"]), flush=True)
                run.close()
            except mhx.MhxError as e:
                print("%s | %-52s | not in this width: %s" % (real, name, str(e)[:150]), flush=True)
    mhx.clear_options()


if __name__ == "__main__":
    main()
