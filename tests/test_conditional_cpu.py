"""CPU: the tracer of function proposals (mhx.trace.trace_proposal), the yardstick of the GPU tests (tests/conditional_restatement.py)
and the register budget of the conditional-proposal kernel.  No GPU.
Reference behaviour under test: src/proposal.jl:92-126."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import conditional_restatement as R
import family_restatement as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "advancedmh.jl_amd", "csrc")


def _host_eval(source, x, table, data=None):
    """run the p.set lines of a traced MHX_PROPOSAL_PARAMS source on Python floats: a tiny interpreter of the emitter's own output
    (one assignment per line, hexadecimal literals)"""
    env = {"x": list(x), "data": [] if data is None else list(data), "MHX_INF": math.inf, "MHX_NAN": math.nan,
           "mhx_log": lambda v: math.log(v) if v > 0 else (-math.inf if v == 0 else math.nan), "mhx_exp": math.exp,
           "mhx_abs": abs, "mhx_sqrt": math.sqrt, "MHX_R": float}
    out = [[p0, p1] for _, p0, p1 in table]
    for line in source.splitlines():
        line = line.strip()
        m = re.match(r"const mhx_real (t\d+) = (.*);$", line)
        if m:
            rhs = re.sub(r"MHX_R\(([^)]*)\)", lambda h: repr(float.fromhex(h.group(1))), m.group(2))
            assert "?" not in rhs and "mhx_fma" not in rhs, "the maps of this test use neither where() nor fma()"
            env[m.group(1)] = eval(rhs, {"__builtins__": {}}, env)       # noqa: S307 (the emitter's own arithmetic lines)
            continue
        m = re.match(r"p\.set\((\d+), (\d+), (.*)\);$", line)
        if m:
            v = m.group(3)
            out[int(m.group(1))][int(m.group(2))] = env[v] if v in env else float.fromhex(re.match(r"MHX_R\((.*)\)", v).group(1))
    return [tuple(r) for r in out]


def test_trace_proposal_source_evaluates_to_the_callables_values(mhx):
    T = mhx.trace
    f1 = lambda x: mhx.Normal(0, 0.5 + abs(x))
    f2 = lambda x: [mhx.Normal(0.5 * x[1], 1), mhx.Laplace(0, T.exp(0.3 * x[0])), mhx.Gamma(0.7, 1.5 + x[2] * x[2])]
    for fn, d, points in ((f1, 1, ([0.3], [-1.25])), (f2, 3, ([0.1, -0.4, 2.0], [1.5, 0.25, -0.5]))):
        fams, table, source = T.trace_proposal(fn, d)
        tp = T.trace_proposal(fn, d)
        assert source.startswith("// traced by mhx.trace") and "MHX_PROPOSAL_PARAMS(x, p, d, data, ndata)" in source
        assert "0x" in source                                               # hexadecimal floating-point literals
        for x in points:
            got = fn(x[0]) if d == 1 else fn(x)
            want = [tuple(float(v) for v in g.params()) for g in (got if isinstance(got, list) else [got])]
            assert _host_eval(source, x, table) == want, (x, source)
            assert tp.evaluate(x) == want
    # unset entries fall back to the table: the constants are there, the traced entries are p.set lines and nothing else is
    fams, table, source = T.trace_proposal(f2, 3)
    assert fams == [0, 2, 5]
    assert table[0][2] == 1.0 and table[1][1] == 0.0 and table[2][1] == 0.7
    assert re.findall(r"p\.set\((\d+), (\d+),", source) == [("0", "0"), ("1", "1"), ("2", "1")]
    # a map of constants sets nothing
    fams, table, source = T.trace_proposal(lambda x: [mhx.Normal(0, 1), mhx.InverseGamma(2, 3)], 2)
    assert "p.set" not in source and table == [(0, 0.0, 1.0), (6, 2.0, 3.0)]
    # TDist(1) is Cauchy(0, 1); a closed-over array travels in the data block
    assert T.trace_proposal(lambda x: mhx.TDist(1), 1).table == [(3, 0.0, 1.0)]
    w = np.array([0.5, 0.25])
    tp = T.trace_proposal(lambda x: mhx.Normal(0, 1.0 + T.sum_over(w, lambda wi: wi * abs(x))), 1)
    assert np.array_equal(tp.data, w) and "data[" in tp.source
    assert tp.evaluate([2.0]) == [(0.0, 1.0 + (0.0 + 0.5 * 2.0 + 0.25 * 2.0))]


def test_the_constructors_hold_traced_parameters(mhx):
    p = mhx.RandomWalkProposal(lambda x: mhx.Normal(0, 0.5 + abs(x)), dim=1)
    assert isinstance(p.proposal, mhx.ConditionalProposal) and p.proposal.dim == 1 and not p.issymmetric
    assert mhx.SymmetricRandomWalkProposal(lambda x: mhx.Normal(0, 0.5 + abs(x)), dim=1).issymmetric
    s = mhx.SymmetricStaticProposal(lambda x: mhx.Normal(x, 1), dim=1)
    assert isinstance(s, mhx.StaticProposal) and s.issymmetric and not mhx.StaticProposal(lambda x: mhx.Normal(x, 1), dim=1).issymmetric
    spl = mhx.MetropolisHastings(mhx.StaticProposal(lambda x: [mhx.Normal(x[1], 1), mhx.Uniform(x[0] - 1, x[0] + 1)], dim=2))
    assert spl.proposal.proposal.table() == [(0, 0.0, 1.0), (1, 0.0, 1.0)]
    assert not mhx.StaticProposal(mhx.Normal(0, 1)).issymmetric                     # the fixed forms are what they were


def test_refusals_that_need_no_device(mhx):
    T = mhx.trace
    err = (mhx.ArgumentError, T.TraceError)
    with pytest.raises(err, match="shape"):
        T.trace_proposal(lambda x: mhx.Gamma(1.0 + abs(x), 1.0), 1)
    with pytest.raises(err, match="shape"):
        mhx.StaticProposal(lambda x: mhx.InverseGamma(2.0 + x * x, 1.0), dim=1)
    with pytest.raises(err, match="TDist"):
        T.trace_proposal(lambda x: mhx.TDist(3), 1)
    with pytest.raises(err, match="must return 3"):
        T.trace_proposal(lambda x: [mhx.Normal(0, 1), mhx.Normal(0, 1)], 3)
    with pytest.raises(err, match="device families"):
        T.trace_proposal(lambda x: [mhx.Normal(0, 1), mhx.MvNormal(mhx.zeros(2), mhx.I)], 2)
    with pytest.raises(err, match="branch"):
        T.trace_proposal(lambda x: mhx.Normal(0, 1.0 if x > 0 else 2.0), 1)
    with pytest.raises(mhx.ArgumentError, match="dim"):
        mhx.RandomWalkProposal(lambda x: mhx.Normal(0, 1))
    with pytest.raises(mhx.ArgumentError, match="bad parameters"):                 # a constant of the map, checked like any component's
        mhx.RandomWalkProposal(lambda x: mhx.Normal(x, -1.0), dim=1)
    with pytest.raises(mhx.ArgumentError, match="function"):                       # StaticProposal{true} of a fixed distribution
        mhx.SymmetricStaticProposal(mhx.Normal(0, 1))
    with pytest.raises(mhx.ArgumentError, match="function proposals"):
        mhx.MetropolisHastings({"a": mhx.RandomWalkProposal(lambda x: mhx.Normal(0, 0.5 + abs(x)), dim=1)})


def _dists(mhx, params):
    cls = [mhx.Normal, mhx.Uniform, mhx.Laplace, mhx.Cauchy, mhx.Exponential, mhx.Gamma, mhx.InverseGamma]
    return [cls[f](p0) if f == F.EXPONENTIAL else cls[f](p0, p1) for f, p0, p1 in params]


def test_the_restatements_heteroscedastic_walk_has_the_right_variance(mhx, oracle, real):
    """the yardstick itself: Normal(0, 0.5 + |x|) on N(0, 1) through R.run with the ratio; 24 chains x 250 recorded states after 50.
    The bounds, derived: steps of scale >= 0.5 accepted more than half the time decorrelate within about ten transitions, so the
    6 000 states are worth at least 600 independent ones -- standard error of the mean 1 / sqrt(600) = 0.041, of the variance
    sqrt(2 / 600) = 0.058; the bands are 5 and 4 of those (0.2, 0.75 .. 1.25).  That is too loose to tell the walk without the ratio
    apart (its variance is 0.874: tests/test_gpu_conditional.py does that with 8192 chains); what is checked here is that the
    restated chain samples N(0, 1) at all."""
    d, pmap, _ = R.CASES["a_scalar_scale_abs"]
    ref = R.run(oracle.iso_gauss(1), pmap, 1, 300, 77, 0, 24, np.zeros((1, 24), dtype=np.float32))
    x = ref["samples"][50:, 0, :].astype(np.float64)
    rate = ref["accepted"][1:].mean()
    print("restatement [%s]: mean %.3f var %.3f acceptance %.3f" % (real, x.mean(), x.var(), rate))
    assert abs(x.mean()) < 0.2 and 0.75 < x.var() < 1.25 and 0.2 < rate < 0.9
    # the one callable does both jobs: traced, its program gives at the chain's states the parameters the restatement used (one abs
    # and one add, both exact to compare: a double sum of two floats rounds to the float sum)
    class M:
        abs, c = staticmethod(mhx.trace.abs), staticmethod(float)
    tp = mhx.trace.trace_proposal(lambda s: _dists(mhx, pmap(M, [s]))[0], 1)
    for v in ref["samples"][::37, 0, 0]:
        want = pmap(R.WIDTH, [F.r(v)])[0]
        assert F.r(tp.evaluate([float(v)])[0][1]) == want[2] and tp.evaluate([float(v)])[0][0] == want[1]


def test_the_restatement_with_constant_parameters_is_the_family_restatement(mhx, oracle, real):
    """Z - Z = +0: a constant map through R.run gives the chain of F.run, walk and static; traced, such a map is its table alone"""
    for static, comps, init in ((False, [(F.NORMAL, 0.0, 1.0), (F.LAPLACE, 0.0, 2.0), (F.CAUCHY, 0.0, 0.5)], np.zeros((3, 6))),
                                (True, [(F.NORMAL, 0.0, 1.0), (F.INVERSE_GAMMA, 2.0, 3.0)], np.ones((2, 6)))):
        d = len(comps)
        a = R.run(oracle.iso_gauss(d), lambda m, x: comps, d, 15, 5, 2, 6, init.astype(np.float32), static=static)
        b = F.run(oracle.iso_gauss(d), comps, 15, 5, 2, 6, static=static, init=init.astype(np.float32))
        assert np.array_equal(a["samples"], b["samples"]) and np.array_equal(a["accepted"], b["accepted"])
        assert 0 < int(a["accept_counts"].sum()) < 6 * 14
        fams, table, source = mhx.trace.trace_proposal(lambda x: _dists(mhx, comps), d)
        assert table == comps and "p.set" not in source


def _worst_map(mhx, fams):
    d = len(fams)
    cls = [mhx.Normal, mhx.Uniform, mhx.Laplace, mhx.Cauchy, mhx.Exponential, mhx.Gamma, mhx.InverseGamma]

    def fn(x):
        out = []
        for k, f in enumerate(fams):
            loc, sc = 0.5 * x[(k + 1) % d], 0.5 + abs(x[k])
            if f == F.UNIFORM:
                out.append(mhx.Uniform(loc - sc, loc + sc))
            elif f == F.EXPONENTIAL:
                out.append(mhx.Exponential(sc))
            elif f in (F.GAMMA, F.INVERSE_GAMMA):
                out.append(cls[f](0.7 if f == F.GAMMA else 2.0, sc))
            else:
                out.append(cls[f](loc, sc))
        return out
    return fn


def test_register_form_compiles_without_scratch_at_its_dimension_limit(mhx, real, tmp_path):
    """the register kernel at d = MHX_COND_REG_MAX_DIM, cross-compiled for gfx950 with the options of the run-time build and a map
    that sets every parameter from the state: no scratch memory for the family that needs the most registers (Cauchy), static,
    and for a mix of all seven, walk; at the next size tried (MHX_COND_REG_NEXT_DIM_TRIED) the Cauchy kernel needs scratch.  Read
    from the code object's metadata."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the build needs it too"
    hdr = open(os.path.join(CSRC, "mhx_rwmh_cond_kernels.h")).read()
    m = re.search(r"#define\s+MHX_COND_REG_MAX_DIM\s+\(MHX_REAL64 \? (\d+) : (\d+)\)", hdr)
    n = re.search(r"#define\s+MHX_COND_REG_NEXT_DIM_TRIED\s+\(MHX_REAL64 \? (\d+) : (\d+)\)", hdr)
    assert m and n, "MHX_COND_REG_MAX_DIM / MHX_COND_REG_NEXT_DIM_TRIED not found"
    dmax, dnext = (int(g.group(1) if real == "f64" else g.group(2)) for g in (m, n))
    assert "d <= MHX_COND_REG_MAX_DIM" in open(os.path.join(CSRC, "mhx_api_cond.inc")).read()

    def scratch_bytes(name, fams, static):
        d = len(fams)
        tp = mhx.trace.trace_proposal(_worst_map(mhx, fams), d)
        src = tmp_path / "cond.hip"
        src.write_text('#include "mhx_device_math.h"\n' + tp.source + '#define MHX_HAVE_PROPOSAL_PARAMS 1\n#include "mhx_rwmh_cond_kernels.h"\n')
        out = tmp_path / "k.s"
        cmd = [hipcc, "-x", "hip", "--offload-device-only", "--no-gpu-bundle-output", "-S", "-DMHX_JIT_BUILD=1", "-I" + CSRC,
               "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
               "-mllvm", "-pragma-unroll-threshold=4000000", "-mllvm", "-amdgpu-unroll-threshold-private=100000",
               "-DMHX_REAL64=%d" % (1 if real == "f64" else 0), "-DMHX_JIT_COND_REG=1", "-DMHX_JIT_DIM=%d" % d, "-DMHX_JIT_TK=0",
               "-DMHX_JIT_FAM_LIST=" + ",".join(str(f) for f in fams), "-DMHX_JIT_FAM_STATIC=%d" % static, "-DMHX_JIT_FAM_SYM=0",
               "-o", str(out), str(src)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert done.returncode == 0, done.stdout[-2000:]
        assert "not unrolled" not in done.stdout, done.stdout[-2000:]
        sizes = re.findall(r"\.name:\s*(\w+)\s|\.private_segment_fixed_size:\s*(\d+)", out.read_text())
        names = [a for a, _ in sizes if a.startswith("mhx_jit_")]
        vals = [int(b) for _, b in sizes if b]
        assert "mhx_jit_cond_reg" in names and vals, (name, sizes)
        return max(vals)

    assert scratch_bytes("cauchy static", [F.CAUCHY] * dmax, 1) == 0
    assert scratch_bytes("mixed walk", [k % 7 for k in range(dmax)], 0) == 0
    assert scratch_bytes("cauchy static, next size", [F.CAUCHY] * dnext, 1) > 0
