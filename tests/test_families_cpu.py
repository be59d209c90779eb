"""CPU (no GPU): the arithmetic spec of the proposal families as restated in tests/family_restatement.py
-- the draws follow their laws, the log-kernels are logpdf minus a constant -- and the host lowering of
RandomWalkProposal / StaticProposal over univariate components (src/proposal.jl:23-35; README.md:106; test/runtests.jl:188-189,
:266-271)."""
import math

import numpy as np
import pytest

import family_restatement as F
import mhx

# Dvoretzky-Kiefer-Wolfowitz (Massart's constant): P(sup |F_n - F| > e) <= 2 exp(-2 n e^2), so with probability 1 - DELTA the
# Kolmogorov distance of n exact draws is below sqrt(ln(2 / DELTA) / (2 n)).  Derived, not tuned; the seed is fixed.
DELTA = 1e-9
N_DRAWS = 4000
SEED = 0x5EEDFA11


def dkw_bound(n):
    return math.sqrt(math.log(2.0 / DELTA) / (2.0 * n))


def ks_distance(xs, cdf):
    xs = np.sort(np.asarray(xs, dtype=np.float64))
    n = xs.size
    Fx = np.array([cdf(float(x)) for x in xs])
    i = np.arange(1, n + 1)
    return max(float(np.max(i / n - Fx)), float(np.max(Fx - (i - 1) / n)))


def poisson_tail(a, z):
    """sum_{j < a} e^-z z^j / j! for integer a: 1 - CDF of Gamma(a, 1) at z"""
    return math.exp(-z) * sum(z ** j / math.factorial(j) for j in range(int(a)))


# (family, p0, p1, closed-form CDF)
LAWS = [
    ("normal", F.NORMAL, 0.4, 1.7, lambda x: 0.5 * math.erfc(-((x - 0.4) / 1.7) / math.sqrt(2.0))),
    ("uniform", F.UNIFORM, -0.2, 0.5, lambda x: min(1.0, max(0.0, (x + 0.2) / 0.7))),
    ("laplace", F.LAPLACE, 0.1, 0.3, lambda x: 0.5 * math.exp((x - 0.1) / 0.3) if x < 0.1 else 1.0 - 0.5 * math.exp(-(x - 0.1) / 0.3)),
    ("cauchy", F.CAUCHY, -1.0, 0.25, lambda x: 0.5 + math.atan((x + 1.0) / 0.25) / math.pi),
    ("exponential", F.EXPONENTIAL, 2.5, 0.0, lambda x: 1.0 - math.exp(-x / 2.5) if x > 0 else 0.0),
    ("gamma(3, 0.5)", F.GAMMA, 3.0, 0.5, lambda x: 1.0 - poisson_tail(3, x / 0.5) if x > 0 else 0.0),
    ("gamma(1, 2)", F.GAMMA, 1.0, 2.0, lambda x: 1.0 - poisson_tail(1, x / 2.0) if x > 0 else 0.0),
    ("inverse gamma(2, 3)", F.INVERSE_GAMMA, 2.0, 3.0, lambda x: poisson_tail(2, 3.0 / x) if x > 0 else 0.0),
    # the boost alpha < 1: Gamma(1/2, theta) is theta chi^2_1 / 2, CDF erf(sqrt(x / theta))
    ("gamma(1/2, 1)", F.GAMMA, 0.5, 1.0, lambda x: math.erf(math.sqrt(x)) if x > 0 else 0.0),
]


@pytest.mark.parametrize("name,fam,p0,p1,cdf", LAWS, ids=[l[0] for l in LAWS])
def test_draws_follow_their_law(real, name, fam, p0, p1, cdf):
    """component 0 of N_DRAWS chains at step 1, transition streams; and the initial-draw streams at step 0"""
    rows = F.table([(fam, p0, p1)])
    for step, nstream, sbase in ((1, 0, F.STREAM_FAMILY), (0, 2, F.STREAM_FAMILY_INIT)):
        n = N_DRAWS if step else N_DRAWS // 4
        xs = [float(F.draw_all(rows, SEED, cid, step, nstream, sbase)[0]) for cid in range(n)]
        assert all(math.isfinite(x) for x in xs)
        D = ks_distance(xs, cdf)
        print("%s [%s] step %d: D_n = %.4f, bound %.4f" % (name, real, step, D, dkw_bound(n)))
        assert D <= dkw_bound(n), (name, real, D, dkw_bound(n))


def test_draws_are_pure_functions_of_their_counters(real):
    """component index and stream enter the counter: two components of one family differ, and so do transition and initial draw"""
    rows = F.table([(F.LAPLACE, 0.0, 1.0), (F.LAPLACE, 0.0, 1.0), (F.GAMMA, 2.0, 1.0), (F.GAMMA, 2.0, 1.0)])
    a = F.draw_all(rows, 7, 3, 5, 0, F.STREAM_FAMILY)
    assert a == F.draw_all(rows, 7, 3, 5, 0, F.STREAM_FAMILY)
    assert a[0] != a[1] and a[2] != a[3]
    b = F.draw_all(rows, 7, 3, 5, 2, F.STREAM_FAMILY_INIT)
    assert all(x != y for x, y in zip(a, b))
    assert a != F.draw_all(rows, 7, 4, 5, 0, F.STREAM_FAMILY) and a != F.draw_all(rows, 7, 3, 6, 0, F.STREAM_FAMILY)


def _logpdf_terms(fam, p0, p1, v):
    """the terms of logpdf that depend on v (in double, from the width's parameters), or None outside the support"""
    if fam == F.NORMAL:
        return [-0.5 * ((v - p0) / p1) ** 2]
    if fam == F.UNIFORM:
        return [0.0] if p0 <= v <= p1 else None
    if fam == F.LAPLACE:
        return [-abs(v - p0) / p1]
    if fam == F.CAUCHY:
        return [-math.log1p(((v - p0) / p1) ** 2)]
    if fam == F.EXPONENTIAL:
        return [-v / p0] if v >= 0 else None
    if fam == F.GAMMA:
        return [(p0 - 1.0) * math.log(v), -v / p1] if v > 0 else None
    return [-(p0 + 1.0) * math.log(v), -p1 / v] if v > 0 else None


@pytest.mark.parametrize("fam,p0,p1", [(F.NORMAL, 0.3, 1.5), (F.UNIFORM, -0.25, 0.75), (F.LAPLACE, 0.1, 0.3), (F.CAUCHY, 0.0, 0.1),
                                       (F.EXPONENTIAL, 1.5, 0.0), (F.GAMMA, 2.5, 0.7), (F.GAMMA, 0.5, 1.0), (F.INVERSE_GAMMA, 2.0, 3.0)])
def test_log_kernels_are_logpdf_minus_a_constant(real, fam, p0, p1):
    """on a grid: within a few ulp of the closed form (each operation rounds to half an ulp, log to one: 8 ulp of the terms' size
    covers the two or three operations of every kernel), and -Inf outside the support"""
    rt = np.float64 if real == "f64" else np.float32
    eps = float(np.finfo(rt).eps)
    row = F.table([(fam, p0, p1)])[0]
    q0, q1 = float(row[1][0]), float(row[1][1])
    grid = [float(rt(v)) for v in np.concatenate([np.linspace(-3.0, 3.0, 61), [1e-3, 17.0, 250.0, -40.0]])]
    seen_out = False
    for v in grid:
        got = float(F.logk(row, v))
        terms = _logpdf_terms(fam, q0, q1, v)
        if terms is None:
            assert got == -math.inf, (fam, v, got)
            seen_out = True
            continue
        want = sum(terms)
        if fam == F.CAUCHY:            # 1 + t^2 is rounded before the logarithm: half an ulp of ITS size
            tol = 8 * eps * (1.0 + abs(want))
        else:
            tol = 8 * eps * sum(abs(t) for t in terms)
        assert abs(got - want) <= tol, (fam, v, got, want, tol)
    assert seen_out == (fam in (F.UNIFORM, F.EXPONENTIAL, F.GAMMA, F.INVERSE_GAMMA))
    assert math.isnan(float(F.logk(row, math.nan))) or float(F.logk(row, math.nan)) == -math.inf


def test_the_ratio_of_a_zero_centred_symmetric_component_is_exactly_zero(real):
    rows = F.table([(F.LAPLACE, 0.0, 0.3), (F.CAUCHY, 0.0, 0.1), (F.UNIFORM, -0.2, 0.2), (F.NORMAL, 0.0, 0.5)])
    rng = np.random.default_rng(1)
    for _ in range(50):
        x = [F.r(v) for v in rng.normal(size=4)]
        y = [x[k] + F.r(v) for k, v in enumerate(rng.uniform(-0.15, 0.15, size=4))]     # (inside the Uniform component's support)
        qb, qf = F.qsum(rows, [x[k] - y[k] for k in range(4)]), F.qsum(rows, [y[k] - x[k] for k in range(4)])
        assert float(qb - qf) == 0.0
    one_sided = F.table([(F.EXPONENTIAL, 1.0, 0.0)])
    assert float(F.qsum(one_sided, [F.r(-0.5)])) == -math.inf and float(F.qsum(one_sided, [F.r(0.5)])) == -0.5


# ---- host lowering ----------------------------------------------------------------------------------------------------

def test_mixed_vectors_lower_to_the_component_table():
    p = mhx.StaticProposal([mhx.Normal(0, 1), mhx.InverseGamma(2, 3)])                 # README.md:106, src/mh-core.jl:22-23
    assert isinstance(p.proposal, mhx.ComponentProposal) and p.proposal.dim == 2
    assert p.proposal.table() == [(0, 0.0, 1.0), (6, 2.0, 3.0)]
    rw = mhx.RandomWalkProposal(mhx.Laplace())                                       # a scalar parameter
    assert rw.proposal.table() == [(2, 0.0, 1.0)] and not rw.issymmetric
    spl = mhx.MetropolisHastings({"a": mhx.StaticProposal(mhx.Normal(0, 1)), "b": mhx.StaticProposal(mhx.InverseGamma(2, 3))})
    assert isinstance(spl.proposal, mhx.StaticProposal) and spl.param_names == ["a", "b"]      # test/runtests.jl:189
    assert spl.proposal.proposal.table() == [(0, 0.0, 1.0), (6, 2.0, 3.0)]
    every = mhx.RWMH([mhx.Normal(1, 2), mhx.Uniform(-1, 3), mhx.Laplace(0.1, 0.3), mhx.Cauchy(0, 0.1), mhx.Exponential(2),
                      mhx.Gamma(0.5, 1), mhx.InverseGamma(2, 3), mhx.TDist(1)])
    assert every.proposal.proposal.table() == [(0, 1.0, 2.0), (1, -1.0, 3.0), (2, 0.1, 0.3), (3, 0.0, 0.1), (4, 2.0, 0.0), (5, 0.5, 1.0),
                                               (6, 2.0, 3.0), (3, 0.0, 1.0)]
    assert mhx.SymmetricRandomWalkProposal([mhx.Cauchy(0, 0.1), mhx.Laplace(0, 2), mhx.Uniform(-1, 1), mhx.Normal(0, 1)]).issymmetric


def test_all_normal_forms_still_lower_to_mvnormal():
    mv = mhx.RWMH([mhx.Normal(0, 2.0), mhx.Normal(0, 0.5)]).proposal.proposal
    assert isinstance(mv, mhx.MvNormal) and mv.kind == 1 and np.allclose(mv.vec, [2.0, 0.5]) and not mv.mean.any()
    mv = mhx.StaticMH(mhx.Normal(0.5, 3.0)).proposal.proposal
    assert isinstance(mv, mhx.MvNormal) and mv.dim == 1 and mv.kind == 1 and mv.vec[0] == 3.0 and mv.mean[0] == 0.5
    spl = mhx.MetropolisHastings({"μ": mhx.StaticProposal(mhx.Normal(0, 1)), "σ": mhx.StaticProposal(mhx.Normal(0.5, 2.0))})
    assert isinstance(spl.proposal.proposal, mhx.MvNormal) and np.allclose(spl.proposal.proposal.vec, [1.0, 2.0])
    assert isinstance(mhx.RWMH(3).proposal.proposal, mhx.MvNormal)


def test_refusals_of_the_host_lowering():
    with pytest.raises(mhx.ArgumentError, match="TDist"):
        mhx.RandomWalkProposal(mhx.TDist(3))
    for bad in (mhx.Laplace(0, 0), mhx.Cauchy(0, -1), mhx.Exponential(0), mhx.Gamma(-1, 1), mhx.Gamma(1, 0), mhx.InverseGamma(0, 3),
                mhx.Uniform(1, 1), mhx.Uniform(2, 1), mhx.Laplace(math.inf, 1), mhx.Cauchy(0, math.nan)):
        with pytest.raises(mhx.ArgumentError, match="bad parameters"):
            mhx.StaticProposal(bad)
        with pytest.raises(mhx.ArgumentError, match="bad parameters"):
            mhx.RandomWalkProposal([mhx.Normal(0, 1), bad])
    with pytest.raises(mhx.ArgumentError, match="bad parameters"):
        mhx.RandomWalkProposal([mhx.Normal(0, -1), mhx.Laplace()])
    with pytest.raises(mhx.ArgumentError):
        mhx.RandomWalkProposal([mhx.Normal(0, 1), "laplace"])
    with pytest.raises(mhx.ArgumentError, match="not symmetric"):                    # src/proposal.jl:195 is a promise of the caller
        mhx.SymmetricRandomWalkProposal(mhx.Exponential(1))
    with pytest.raises(mhx.ArgumentError, match="not symmetric"):
        mhx.SymmetricRandomWalkProposal(mhx.Laplace(0.1, 0.3))
    # the refusals that were there before still hold, with their messages
    with pytest.raises(mhx.ArgumentError, match="every entry"):
        mhx.MetropolisHastings({"a": mhx.RandomWalkProposal(mhx.Laplace()), "b": mhx.StaticProposal(mhx.Normal(0, 1))})
    with pytest.raises(mhx.ArgumentError, match="one scalar Normal"):
        mhx.MetropolisHastings({"a": mhx.StaticProposal([mhx.Normal(0, 1), mhx.InverseGamma(2, 3)])})
    with pytest.raises(mhx.ArgumentError):
        mhx.MetropolisHastings("static")


def test_host_rand_of_the_new_distributions():
    rng = np.random.default_rng(3)
    for dist, lo, hi in ((mhx.Uniform(-1, 3), -1, 3), (mhx.Exponential(2), 0, math.inf), (mhx.Gamma(2, 3), 0, math.inf),
                         (mhx.Laplace(0, 1), -math.inf, math.inf), (mhx.Cauchy(0, 1), -math.inf, math.inf), (mhx.TDist(4), -math.inf, math.inf)):
        xs = [dist.rand(rng) for _ in range(200)]
        assert all(lo <= x <= hi for x in xs)
    assert mhx.ComponentProposal([mhx.Uniform(0, 1), mhx.Normal(0, 1)]).rand(rng).shape == (2,)


def test_component_struct_mirrors_the_header():
    """mhx_proposal_component, mhx_family and the symmetric flag: header, ctypes mirror and Julia glue agree"""
    import ctypes as C
    import os
    import re
    import mhx._lib as L
    import test_abi_mirrors as A
    hs = A.header_structs()
    want = [(n, A.CT[t]) for n, t in hs["mhx_proposal_component"]]
    assert list(L.ProposalComponent._fields_) == want and C.sizeof(L.ProposalComponent) == 24
    js = A.julia_structs()
    assert js["ProposalComponent"] == [(n, A.JT[t]) for n, t in hs["mhx_proposal_component"]]
    fam = dict(re.findall(r"(MHX_FAMILY_\w+)\s*=\s*(\d+)", A.HDR))
    assert [int(fam["MHX_FAMILY_" + n]) for n in ("NORMAL", "UNIFORM", "LAPLACE", "CAUCHY", "EXPONENTIAL", "GAMMA", "INVERSE_GAMMA")] == \
        [L.FAMILY_NORMAL, L.FAMILY_UNIFORM, L.FAMILY_LAPLACE, L.FAMILY_CAUCHY, L.FAMILY_EXPONENTIAL, L.FAMILY_GAMMA, L.FAMILY_INVERSE_GAMMA]
    assert [F.NORMAL, F.UNIFORM, F.LAPLACE, F.CAUCHY, F.EXPONENTIAL, F.GAMMA, F.INVERSE_GAMMA] == list(range(7))
    assert re.search(r"#define\s+MHX_FLAG_SYMMETRIC_PROPOSAL\s+128\b", A.HDR) and L.FLAG_SYMMETRIC_PROPOSAL == 128
    math_h = open(os.path.join(A.ROOT, "advancedmh.jl_amd", "csrc", "mhx_device_math.h")).read()
    for name, val in fam.items():
        assert re.search(r"#define\s+%s\s+%s\b" % (name, val), math_h), name
    assert "mhx_rwmh_create_components" in A.JL


def test_gamma_boost_is_decided_once_on_the_rounded_alpha(real):
    """an alpha just below 1 that rounds to 1 in the run's width: table (d from alpha or alpha + 1) and draw (times u^(1/alpha) iff
    the row's alpha < 1) must take the same side, else the draw is silently Gamma(alpha + 1)"""
    for alpha in (1.0 - 2.0 ** -30, 1.0 - 2.0 ** -60, 0.999, 1.0, 1.0 + 2.0 ** -30):
        fam, p = F.table([(F.GAMMA, alpha, 1.0)])[0]
        boosted = bool(p[0] < F.r(1))
        want_d = (float(p[0]) + 1.0 if boosted else float(p[0])) - 1.0 / 3.0
        assert float(p[2]) == float(F.r(want_d)), (real, alpha)
        assert float(p[4]) == float(F.r(1.0 / float(p[0]))) and float(p[5]) == float(F.r(float(p[0]) - 1.0))
    if real == "f32":
        assert not bool(F.table([(F.GAMMA, 1.0 - 2.0 ** -30, 1.0)])[0][1][0] < F.r(1))      # rounds to 1: no boost, d = 2/3


def test_register_form_compiles_without_scratch_at_its_dimension_limit(real, tmp_path):
    """the specialised kernel at d = MHX_FAM_REG_MAX_DIM, cross-compiled for gfx950 with the options of the run-time build: no
    scratch memory (x and y in registers) for the family that needs the most registers (Cauchy) and for a mix of all seven"""
    import os
    import re
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "advancedmh.jl_amd", "csrc")
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the build needs it too"
    hdr = open(os.path.join(csrc, "mhx_rwmh_family_kernels.h")).read()
    m = re.search(r"#define\s+MHX_FAM_REG_MAX_DIM\s+\(MHX_REAL64 \? (\d+) : (\d+)\)", hdr)
    assert m, "MHX_FAM_REG_MAX_DIM not found"
    d = int(m.group(1) if real == "f64" else m.group(2))
    assert "d <= MHX_FAM_REG_MAX_DIM" in open(os.path.join(csrc, "mhx_api.hip")).read()
    src = tmp_path / "fam.hip"
    src.write_text('#include "mhx_device_math.h"\n#include "mhx_rwmh_family_kernels.h"\n')
    for name, fams, static in (("cauchy walk", [F.CAUCHY] * d, 0), ("mixed walk", [k % 7 for k in range(d)], 0), ("mixed static", [k % 7 for k in range(d)], 1)):
        out = tmp_path / "k.s"
        cmd = [hipcc, "-x", "hip", "--offload-device-only", "--no-gpu-bundle-output", "-S", "-DMHX_JIT_BUILD=1", "-I" + csrc,
               "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
               "-mllvm", "-pragma-unroll-threshold=4000000", "-mllvm", "-amdgpu-unroll-threshold-private=100000",
               "-DMHX_REAL64=%d" % (1 if real == "f64" else 0), "-DMHX_JIT_FAM_REG=1", "-DMHX_JIT_DIM=%d" % d, "-DMHX_JIT_TK=0",
               "-DMHX_JIT_FAM_LIST=" + ",".join(str(f) for f in fams), "-DMHX_JIT_FAM_STATIC=%d" % static, "-DMHX_JIT_FAM_SYM=0",
               "-o", str(out), str(src)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert done.returncode == 0, done.stdout[-2000:]
        assert "not unrolled" not in done.stdout, done.stdout[-2000:]
        sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", out.read_text())
        assert sizes and all(int(v) == 0 for v in sizes), "%s, d = %d [%s]: %s bytes of scratch" % (name, d, real, sizes)
