"""CPU: the tracer of composite proposals (mhx.trace.trace_composite), the two spellings of the Python API, the yardstick of the GPU
tests (tests/composite_restatement.py) and the register budget of the composite kernel.  No GPU.
Reference behaviour under test: src/proposal.jl:128-175,198-240; README.md:92-117."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import composite_helpers as H
import composite_restatement as CR
import conditional_restatement as R
import family_restatement as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "advancedmh.jl_amd", "csrc")


# ---------------------------------------------------------------------------------------------------------------------
# the tracer
def test_trace_composite_remaps_slices_to_global_indices(mhx):
    T = mhx.trace
    entries = [("a", 1, [mhx.Normal(0, 1)]),
               ("b", 2, lambda x: [mhx.Normal(0.5 * x[1], 1), mhx.Laplace(0, 0.5 + abs(x[0]))]),
               ("c", 1, lambda x: mhx.Cauchy(0, T.exp(0.3 * x))),
               ("d", 1, mhx.InverseGamma(2, 3))]
    tc = T.trace_composite(entries)
    table, mapped, source, data = tc
    assert tc.families == [0, 0, 2, 3, 6] and mapped == [0, 1, 2, 2, 0] and data is None
    assert table[0] == (0, 0.0, 1.0) and table[4] == (6, 2.0, 3.0) and table[1][2] == 1.0 and table[2][1] == 0.0
    assert re.findall(r"p\.set\((\d+), (\d+),", source) == [("1", "0"), ("2", "1"), ("3", "1")]
    # entry b's x[1] is the global x[2], its x[0] the global x[1]; entry c's scalar is x[3]; x[0] and x[4] are read by nobody
    assert set(re.findall(r"x\[(\d+)\]", source)) == {"1", "2", "3"}
    x = [9.0, 0.25, -1.5, 2.0, 7.0]
    got = tc.evaluate(x)
    assert got[1] == (0.5 * -1.5, 1.0) and got[2] == (0.0, 0.5 + 0.25) and got[3] == (0.0, float(np.exp(0.3 * 2.0))) and got[0] == (0.0, 1.0)
    # nothing mapped: no source at all
    tc = T.trace_composite([("a", 2, [mhx.Normal(0, 1), mhx.Laplace(0, 2)]), ("b", 1, lambda x: mhx.Uniform(-1, 1))])
    assert tc.source == "" and tc.mapped == [0, 0, 0] and tc.table == [(0, 0.0, 1.0), (2, 0.0, 2.0), (1, -1.0, 1.0)]
    # a closed-over array travels in the one data block
    w = np.array([0.5, 0.25])
    tc = T.trace_composite([("a", 1, [mhx.Normal(0, 1)]), ("b", 1, lambda x: mhx.Normal(0, 1.0 + T.sum_over(w, lambda wi: wi * abs(x))))])
    assert np.array_equal(tc.data, w) and "data[" in tc.source and tc.evaluate([5.0, 2.0])[1] == (0.0, 1.0 + (0.0 + 0.5 * 2.0 + 0.25 * 2.0))


def test_trace_composite_refusals_name_the_entry(mhx):
    T = mhx.trace
    err = (mhx.ArgumentError, T.TraceError)
    ok = ("a", 1, [mhx.Normal(0, 1)])
    with pytest.raises(err, match=r"entry 'b'.*must return 2"):
        T.trace_composite([ok, ("b", 2, lambda x: [mhx.Normal(x[0], 1)])])
    with pytest.raises(err, match=r"entry 'g'.*component 1.*shape"):
        T.trace_composite([ok, ("g", 1, lambda x: mhx.Gamma(1.0 + abs(x), 1.0))])
    with pytest.raises(err, match=r"entry 'c'.*branch"):
        T.trace_composite([ok, ("c", 1, lambda x: mhx.Normal(0, 1.0 if x > 0 else 2.0))])
    with pytest.raises(err, match=r"entry 't'.*TDist"):
        T.trace_composite([ok, ("t", 1, lambda x: mhx.TDist(3))])
    with pytest.raises(err, match=r"entry 2.*device families"):
        T.trace_composite([ok, (2, 2, lambda x: [mhx.Normal(0, 1), mhx.MvNormal(mhx.zeros(2), mhx.I)])])
    # trace_proposal's own messages are what they were
    with pytest.raises(err, match="^component 0: the shape"):
        T.trace_proposal(lambda x: mhx.Gamma(1.0 + abs(x), 1.0), 1)


# ---------------------------------------------------------------------------------------------------------------------
# the spellings
def _same_lowering(a, b):
    pa, pb = a.proposal, b.proposal
    assert type(pa) is type(pb) and pa.issymmetric == pb.issymmetric and type(pa.proposal) is type(pb.proposal)
    if hasattr(pa.proposal, "table"):
        assert pa.proposal.table() == pb.proposal.table()
    else:
        assert pa.proposal.kind == pb.proposal.kind and np.array_equal(pa.proposal.mean, pb.proposal.mean)
        assert np.array_equal(pa.proposal.vec, pb.proposal.vec) and pa.proposal.scale == pb.proposal.scale


def test_homogeneous_scalars_fold_as_the_mapping_form_does(mhx):
    RW, ST = mhx.RandomWalkProposal, mhx.StaticProposal
    for make in (lambda: dict(mu=RW(mhx.Normal(0, 0.5)), sigma=RW(mhx.Normal(0.1, 2.0))),
                 lambda: dict(mu=ST(mhx.Normal(0, 1)), sigma=ST(mhx.InverseGamma(2, 3))),
                 lambda: dict(a=RW(mhx.Laplace(0, 1), issymmetric=True), b=RW(mhx.Normal(0, 1), issymmetric=True))):
        mapping = mhx.MetropolisHastings(make())
        named = mhx.MetropolisHastings(mhx.NamedProposals(**make()))
        listed = mhx.MetropolisHastings(list(make().values()))
        tupled = mhx.MetropolisHastings(tuple(make().values()))
        for other in (named, listed, tupled):
            assert not isinstance(other.proposal, mhx.CompositeProposal)
            _same_lowering(mapping, other)
        assert named.param_names == mapping.param_names == list(make())
        assert listed.param_names is None and tupled.param_names is None


def test_anything_else_is_a_composite_with_the_right_blocks_and_names(mhx):
    import mhx._lib as L
    RW, ST = mhx.RandomWalkProposal, mhx.StaticProposal
    spl = mhx.MetropolisHastings(mhx.NamedProposals(
        mu=RW(mhx.Normal(0, 0.5)), a=ST([mhx.Normal(0, 1), mhx.InverseGamma(2, 3)]),
        w=RW(mhx.MvNormal(mhx.zeros(2), np.array([0.25, 4.0])), issymmetric=True), i=RW(mhx.MvNormal([0.5, 0.0], 4.0 * mhx.I)),
        f=ST(lambda x: [mhx.Normal(x[1], 1), mhx.Uniform(x[0] - 1, x[0] + 1)], dim=2, issymmetric=True), s=RW(lambda x: mhx.Laplace(0, 0.5 + abs(x)), dim=1)))
    cp = spl.proposal
    assert isinstance(cp, mhx.CompositeProposal) and cp.proposal is cp and cp.dim == 10
    assert spl.param_names == ["mu", "a[1]", "a[2]", "w[1]", "w[2]", "i[1]", "i[2]", "f[1]", "f[2]", "s"]
    assert cp.blocks == [(0, 1, 0), (1, 2, L.BLOCK_STATIC), (3, 2, L.BLOCK_SYMMETRIC), (5, 2, 0), (7, 2, L.BLOCK_STATIC | L.BLOCK_SYMMETRIC), (9, 1, 0)]
    assert cp.table()[:7] == [(0, 0.0, 0.5), (0, 0.0, 1.0), (6, 2.0, 3.0), (0, 0.0, 0.5), (0, 0.0, 2.0), (0, 0.5, 2.0), (0, 0.0, 2.0)]
    assert cp.mapped == [0] * 7 + [1, 3, 2]
    assert re.findall(r"p\.set\((\d+), (\d+),", cp.source) == [("7", "0"), ("8", "0"), ("8", "1"), ("9", "1")]
    assert set(re.findall(r"x\[(\d+)\]", cp.source)) == {"7", "8", "9"}            # every map reads its own slice, by global index
    # a list: the same composite without names; mixed kinds of scalars and a one-entry symmetric flag are composites too
    lst = mhx.MetropolisHastings([RW(mhx.Normal(0, 0.5)), ST(mhx.InverseGamma(2, 3))])
    assert isinstance(lst.proposal, mhx.CompositeProposal) and lst.param_names is None and lst.proposal.blocks == [(0, 1, 0), (1, 1, 1)]
    one = mhx.MetropolisHastings([RW([mhx.Normal(0, 1), mhx.Laplace(0, 1)], issymmetric=True), RW(mhx.Cauchy(0, 1))])
    assert one.proposal.blocks == [(0, 2, L.BLOCK_SYMMETRIC), (2, 1, 0)]


def test_refusals_of_the_spellings(mhx):
    RW, ST = mhx.RandomWalkProposal, mhx.StaticProposal
    dense = mhx.MvNormal(mhx.zeros(2), np.array([[1.0, 0.5], [0.5, 1.0]]))
    with pytest.raises(mhx.ArgumentError, match=r"entry 'w'.*dense"):
        mhx.MetropolisHastings(mhx.NamedProposals(a=ST(mhx.Normal(0, 1)), w=RW(dense)))
    with pytest.raises(mhx.ArgumentError, match=r"entry 2.*dense"):
        mhx.MetropolisHastings([RW(mhx.Normal(0, 1)), RW(dense)])
    with pytest.raises(mhx.ArgumentError, match=r"entry 2.*not a RandomWalkProposal"):
        mhx.MetropolisHastings([RW(mhx.Normal(0, 1)), mhx.Normal(0, 1)])
    with pytest.raises(mhx.ArgumentError, match=r"entry 'b'.*not a RandomWalkProposal"):
        mhx.MetropolisHastings(mhx.NamedProposals(a=RW(mhx.Normal(0, 1)), b=3))
    with pytest.raises(mhx.ArgumentError, match="empty"):
        mhx.MetropolisHastings([])
    with pytest.raises(mhx.ArgumentError, match="empty"):
        mhx.NamedProposals()
    with pytest.raises((mhx.ArgumentError, mhx.trace.TraceError), match=r"entry 'f'.*must return 2"):
        mhx.MetropolisHastings(mhx.NamedProposals(a=ST(mhx.Normal(0, 1)), f=_unchecked_function(mhx, lambda x: [mhx.Normal(x[0], 1)], 2)))
    # the mapping form is exactly what it was: its three refusals still raise
    with pytest.raises(mhx.ArgumentError, match="every entry"):
        mhx.MetropolisHastings({"a": RW(mhx.Normal(0, 1)), "b": ST(mhx.Normal(0, 1))})
    with pytest.raises(mhx.ArgumentError, match="one scalar Normal"):
        mhx.MetropolisHastings({"a": RW([mhx.Normal(0, 1), mhx.Normal(0, 1)]), "b": RW(mhx.Normal(0, 1))})
    with pytest.raises(mhx.ArgumentError, match="function proposals"):
        mhx.MetropolisHastings({"a": RW(lambda x: mhx.Normal(0, 0.5 + abs(x)), dim=1)})


def _unchecked_function(mhx, fn, dim):
    """a RandomWalkProposal that holds `fn` without the constructor's own trace (which would refuse the wrong count first)"""
    p = mhx.RandomWalkProposal(lambda x: [mhx.Normal(x[0], 1)] * dim, dim=dim)
    p.proposal.fn = fn
    return p


def test_the_case_entries_become_the_expected_composites(mhx, oracle):
    import mhx._lib as L
    d, pos, entries = CR.CASES["A"]
    for spl in (H.list_sampler(mhx, entries), H.named_sampler(mhx, entries)):
        cp = spl.proposal
        assert cp.blocks == [(0, 2, L.BLOCK_SYMMETRIC), (2, 2, L.BLOCK_STATIC), (4, 1, 0)] and cp.mapped == [0, 0, 0, 0, 2]
        assert cp.table()[:4] == [(0, 0.0, 0.5), (0, 0.0, 0.7), (0, 0.0, 1.0), (6, 2.0, 3.0)] and cp.table()[4][0] == F.LAPLACE
    assert H.named_sampler(mhx, entries).param_names == ["a[1]", "a[2]", "b[1]", "b[2]", "c"]
    d, pos, entries = CR.CASES["B"]
    cp = H.list_sampler(mhx, entries).proposal
    assert cp.blocks == [(0, 2, 0), (2, 2, 0), (4, 3, L.BLOCK_STATIC)] and cp.mapped == [3, 3, 2, 2, 1, 2, 2]
    # traced, the program gives the parameters the restatement uses (operations that are exact in double at these points)
    x = [0.5, -0.25, 1.0, 2.0, 0.75, 1.5, 0.125]
    oracle.set_dtype("f64")                                                   # (the width fixture restores it; evaluate() is float64)
    want = CR.pmap_of(entries)(R.WIDTH, [np.float64(v) for v in x])
    got = cp.traced.evaluate(x)
    for (f, p0, p1), g in zip(want, got):
        assert g[0] == float(p0) and (f == F.EXPONENTIAL or g[1] == float(p1))


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
def test_one_block_is_the_conditional_and_the_family_restatement(oracle, real):
    """a single block reproduces tests/conditional_restatement.py, and tests/family_restatement.py when constant, in bits"""
    for name, static, n in (("b_cross_coordinates", False, 6), ("b_cross_coordinates", True, 6), ("d_data_block", False, 6)):
        d, pmap, init = R.CASES[name]
        x0 = init(n)
        a = CR.run(oracle.iso_gauss(d), pmap, d, [(0, d, static, False)], 15, 5, 2, n, x0)
        b = R.run(oracle.iso_gauss(d), pmap, d, 15, 5, 2, n, x0, static=static)
        assert np.array_equal(a["samples"], b["samples"]) and np.array_equal(a["accepted"], b["accepted"])
        assert 0 < int(a["accept_counts"].sum()) < n * 14
    for static, comps, init in ((False, [(F.NORMAL, 0.0, 1.0), (F.LAPLACE, 0.0, 2.0), (F.CAUCHY, 0.0, 0.5)], np.zeros((3, 6))),
                                (True, [(F.NORMAL, 0.0, 1.0), (F.INVERSE_GAMMA, 2.0, 3.0)], np.ones((2, 6))),
                                (False, [(F.NORMAL, 0.0, 1.0), (F.LAPLACE, 0.0, 2.0), (F.CAUCHY, 0.0, 0.5)], None)):
        d = len(comps)
        x0 = None if init is None else init.astype(np.float32)
        a = CR.run(oracle.iso_gauss(d), lambda m, x: comps, d, [(0, d, static, False)], 15, 5, 2, 6, x0)
        b = F.run(oracle.iso_gauss(d), comps, 15, 5, 2, 6, static=static, init=x0)
        assert np.array_equal(a["samples"], b["samples"]) and np.array_equal(a["accepted"], b["accepted"])
        assert 0 < int(a["accept_counts"].sum()) < 6 * 14


def test_the_cases_have_the_expected_counts_and_need_their_kinds_and_flags(oracle, real):
    """the accept counts of the cases are pinned; forcing one kind on every block or moving a symmetric flag changes what it must
    change"""
    expected = {("A", "f64"): 219, ("A", "f32"): 219, ("B", "f64"): 107, ("B", "f32"): 112}
    for name, (d, pos, entries) in CR.CASES.items():
        ref = CR.run_case(oracle, entries, d, pos)
        assert int(ref["accept_counts"].sum()) == expected[name, real]
        walk = CR.run_case(oracle, CR.with_kinds(entries, False), d, pos)
        stat = CR.run_case(oracle, CR.with_kinds(entries, True), d, pos)
        assert int(walk["accept_counts"].sum()) == 0                          # the one-sided families give -Inf
        assert not np.array_equal(stat["samples"], ref["samples"]) and int(stat["accept_counts"].sum()) > 0
    d, pos, entries = CR.CASES["A"]
    ref = CR.run_case(oracle, entries, d, pos)
    same = CR.run_case(oracle, CR.with_symmetric(entries, 0, False), d, pos)      # zero-mean Normals: their ratio is +-0 anyway
    assert np.array_equal(same["samples"], ref["samples"]) and np.array_equal(same["accepted"], ref["accepted"])
    other = CR.run_case(oracle, CR.with_symmetric(entries, 2, True), d, pos)      # the Laplace block's Z matters
    assert not np.array_equal(other["samples"], ref["samples"])


def test_the_draws_do_not_depend_on_the_grouping(oracle, real):
    """regrouping A's five components leaves the draws of step 1 unchanged, bit for bit (every entry of A maps at most its own
    coordinate, so any contiguous grouping keeps the maps inside their blocks)"""
    d, pos, entries = CR.CASES["A"]
    ref = CR.run_case(oracle, entries, d, pos, nchains=8, n_samples=2)
    for sizes in ((5,), (1, 1, 1, 1, 1), (3, 2), (1, 4)):
        alt = CR.run_case(oracle, CR.regrouped(entries, sizes), d, pos, nchains=8, n_samples=2)
        assert np.array_equal(alt["first_xi"].view(np.uint8), ref["first_xi"].view(np.uint8)), sizes


# ---------------------------------------------------------------------------------------------------------------------
# the register budget
def _rule(hdr, real):
    """the admission rule of the register form, read from the headers"""
    cond = open(os.path.join(CSRC, "mhx_rwmh_cond_kernels.h")).read()
    fam = open(os.path.join(CSRC, "mhx_rwmh_family_kernels.h")).read()
    i = 1 if real == "f64" else 2
    cmax = int(re.search(r"#define\s+MHX_COND_REG_MAX_DIM\s+\(MHX_REAL64 \? (\d+) : (\d+)\)", cond).group(i))
    fmax = int(re.search(r"#define\s+MHX_FAM_REG_MAX_DIM\s+\(MHX_REAL64 \? (\d+) : (\d+)\)", fam).group(i))
    assert re.search(r"#define\s+MHX_COMPOSITE_REG_COST_MAX\s+\(3 \* MHX_COND_REG_MAX_DIM\)", hdr)
    inc = open(os.path.join(CSRC, "mhx_api_composite.inc")).read()
    assert "nmapped ? 2 * d + nmapped + nzblocks / 2 <= MHX_COMPOSITE_REG_COST_MAX : d <= MHX_FAM_REG_MAX_DIM" in inc
    return (lambda d, nm, zb: (2 * d + nm + zb // 2 <= 3 * cmax) if nm else d <= fmax), cmax, fmax


def _shape(mhx, d, nmapped, kind):
    """(entries for trace_composite, families, static list, block list, symmetric list): `nmapped` of the d components, spread evenly,
    get both parameters from two coordinates of their block.  kind "cauchy": Cauchy throughout in one static block (the worst
    family); "own static" / "own walk": Cauchy throughout, every component a block of its own; "mix": the seven families in turn,
    the kind alternating per component, every component a block of its own"""
    cls = [mhx.Normal, mhx.Uniform, mhx.Laplace, mhx.Cauchy, mhx.Exponential, mhx.Gamma, mhx.InverseGamma]
    is_mapped = [False] * d
    for i in range(nmapped):
        is_mapped[(i * d) // nmapped] = True
    fams = [k % 7 for k in range(d)] if kind == "mix" else [F.CAUCHY] * d

    def comp(f, mapped, xk, xn):
        loc, sc = (0.5 * xn, 0.5 + abs(xk)) if mapped else (0.0, 1.0)
        if f == F.UNIFORM:
            return mhx.Uniform(loc - sc, loc + sc)
        if f == F.EXPONENTIAL:
            return mhx.Exponential(sc)
        if f in (F.GAMMA, F.INVERSE_GAMMA):
            return cls[f](0.7 if f == F.GAMMA else 2.0, sc)
        return cls[f](loc, sc)
    if kind == "cauchy":
        entries = [("all", d, lambda x: [comp(fams[k], is_mapped[k], x[k], x[(k + 1) % d]) for k in range(d)])]
        return entries, fams, [1] * d, [0] * d, [0]
    entries = [(k, 1, lambda x, k=k: comp(fams[k], is_mapped[k], x, x)) for k in range(d)]
    stat = [k % 2 for k in range(d)] if kind == "mix" else [1 if kind == "own static" else 0] * d
    return entries, fams, stat, list(range(d)), [0] * d


def test_register_form_compiles_without_scratch_at_the_admission_rules_limit(mhx, real, tmp_path):
    """the register kernel at the largest dimension the rule admits with none, half and all of the components mapped, cross-compiled
    for gfx950 with the options of the run-time build: no scratch memory -- Cauchy throughout in one block, Cauchy throughout with
    every component a block of its own (static and walk: every mapped block carries a Z pair), and the seven families mixed with
    the kind alternating.  Two shapes the rule rejects need scratch in fp64: d = 25 with 12 mapped in one block, and d = 20 with
    everything mapped in blocks of their own (the same shape in ONE block is admitted and clean); in fp32 the rule is the same
    expression and stops short of the first shape found to need scratch (d = 44, 22 mapped).  Read from the code object's
    metadata."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the build needs it too"
    hdr = open(os.path.join(CSRC, "mhx_rwmh_composite_kernels.h")).read()
    admits, cmax, fmax = _rule(hdr, real)

    def largest(mapped_of, own):
        return max(d for d in range(1, fmax + 1) if admits(d, mapped_of(d), mapped_of(d) if own else min(1, mapped_of(d))))
    one = tuple(largest(m, False) for m in (lambda d: 0, lambda d: d // 2, lambda d: d))
    own = tuple(largest(m, True) for m in (lambda d: 0, lambda d: d // 2, lambda d: d))
    assert one == ((32, 24, 20) if real == "f64" else (48, 38, 32)) and own == ((32, 22, 17) if real == "f64" else (48, 35, 27))
    assert not admits(one[0] + 1, 0, 0) and not admits(one[1] + 1, (one[1] + 1) // 2, 1) and not admits(one[2] + 1, one[2] + 1, 1)
    assert not admits(fmax, 1, 1) and admits(fmax - 3, 2, 1)                  # one mapped component ends the nothing-mapped regime
    assert admits(one[2], one[2], 1) and not admits(one[2], one[2], one[2])   # the Z pairs count

    def scratch_bytes(shape):
        d, nmapped, kind = shape
        entries, fams, stat, blk, sym = _shape(mhx, d, nmapped, kind)
        tc = mhx.trace.trace_composite(entries)
        assert sum(1 for m in tc.mapped if m) == nmapped
        work = tmp_path / ("%s_%d_%d" % (kind.replace(" ", "_"), d, nmapped))
        work.mkdir()
        src = work / "composite.hip"
        src.write_text('#include "mhx_device_math.h"\n' + (tc.source or "MHX_PROPOSAL_PARAMS(x, p, d, data, ndata) {}\n") +
                       '#define MHX_HAVE_PROPOSAL_PARAMS 1\n#include "mhx_rwmh_composite_kernels.h"\n')
        out = work / "k.s"
        j = lambda l: ",".join(str(v) for v in l)
        cmd = [hipcc, "-x", "hip", "--offload-device-only", "--no-gpu-bundle-output", "-S", "-DMHX_JIT_BUILD=1", "-I" + CSRC,
               "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
               "-mllvm", "-pragma-unroll-threshold=4000000", "-mllvm", "-amdgpu-unroll-threshold-private=100000",
               "-DMHX_REAL64=%d" % (1 if real == "f64" else 0), "-DMHX_JIT_COMPOSITE_REG=1", "-DMHX_JIT_DIM=%d" % d, "-DMHX_JIT_TK=0",
               "-DMHX_JIT_FAM_LIST=" + j(fams), "-DMHX_JIT_CMP_STATIC_LIST=" + j(stat), "-DMHX_JIT_CMP_BLOCK_LIST=" + j(blk),
               "-DMHX_JIT_CMP_MAPPED_LIST=" + j(tc.mapped), "-DMHX_JIT_CMP_SYM_LIST=" + j(sym), "-o", str(out), str(src)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert done.returncode == 0, done.stdout[-2000:]
        assert "not unrolled" not in done.stdout, done.stdout[-2000:]
        sizes = re.findall(r"\.name:\s*(\w+)\s|\.private_segment_fixed_size:\s*(\d+)", out.read_text())
        names = [a for a, _ in sizes if a.startswith("mhx_jit_")]
        vals = [int(b) for _, b in sizes if b]
        assert "mhx_jit_composite_reg" in names and vals, (d, nmapped, kind, sizes)
        return max(vals)

    mapped = lambda t: (0, t[1] // 2, t[2])
    limit = [(d, nm, "cauchy") for d, nm in zip(one, mapped(one))]
    limit += [(d, nm, kind) for kind in ("own static", "own walk", "mix") for d, nm in list(zip(own, mapped(own)))[1:]] + [(own[0], 0, "mix")]
    rejected = [(25, 12, "cauchy"), (20, 20, "own walk")] if real == "f64" else [(44, 22, "cauchy")]
    assert not admits(rejected[0][0], rejected[0][1], 1) and (real == "f32" or not admits(20, 20, 20))
    with ThreadPoolExecutor(6) as pool:                                        # (the compilations are child processes)
        got = list(pool.map(scratch_bytes, limit + rejected))
    for shape, nbytes in zip(limit, got):
        assert nbytes == 0, (shape, nbytes)
    for shape, nbytes in zip(rejected, got[len(limit):]):
        assert nbytes > 0, (shape, nbytes)
