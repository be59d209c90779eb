"""CPU (no GPU): the restatement of the adaptive temperature ladder (tests/tempered_adaptive_restatement.py)
pinned to the fixed-ladder restatement and to hand-computed values, the inputs of the GPU parity cases (tests/test_gpu_tempered_adaptive.py
shares them and their restated chains), the adaptive register kernel at the register form's dimension limit, and the guards of the new
entry points."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases
import tempered_adaptive_restatement as A
import tempered_restatement as P
import test_tempered_cpu as FIXED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "advancedmh.jl_amd", "csrc")


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    assert a.dtype == b.dtype, "%s: dtypes %s / %s" % (what, a.dtype, b.dtype)
    bad = np.argwhere(cases.bits(a) != cases.bits(b))
    assert len(bad) == 0, "%s: %d mismatches, first at %s: %r vs %r" % (what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


# ---- c = 0: the ladder never moves, and the chains are the fixed-ladder restatement's on the ladder rho0 defines
@pytest.mark.parametrize("kind", ["iso", "diag"])
def test_with_c_zero_the_chains_are_the_fixed_ladders(oracle, real, kind):
    """The fixed-ladder restatement forms the proposal scale as ONE product in double, scales[r] * sigma_k, rounded once; the adaptive
    spec forms s[r] * sigma_k in the width.  With s[r] and sigma_k values of the width (sigma_k chosen representable in fp32) the
    double product of the two is exact in fp32's case and the same operation in fp64's, so the two scales are the same number and the
    chains agree bit for bit -- no rounding to excuse, everything is compared."""
    O = oracle
    R, nl, d, seed, first, N = 4, 3, 2, 0xC0, 8, 14
    sigma = 0.875 if kind == "iso" else np.array([0.75, 1.25], dtype=O.real())
    pk = O.PROP_ISO if kind == "iso" else O.PROP_DIAG
    start = [1.0, 0.5, 0.2, 0.05]
    got = A.run(O.iso_gauss(d), pk, sigma, start, N, seed, first, R * nl, adapt_steps=9, swap_every=2, c=0.0)
    beta, s = A.ladder(A.rho0(start, A.DEFAULTS["rho_min"], A.default_rho_max(R)))
    _same(got["betas"], np.array([beta] * nl, dtype=O.real()), "betas stay rho0's")
    assert (cases.bits(got["betas_rounds"]) == cases.bits(got["betas"])[None]).all()
    # rho0's ladder is the starting ladder up to the roundings of log log, exp and exp
    assert np.allclose(np.array(beta, dtype=np.float64), start, rtol=1e-5 if real == "f32" else 1e-13)
    ref = P.run(O.iso_gauss(d), pk, sigma, [float(b) for b in beta], N, seed, first, R * nl, swap_every=2, scales=[float(v) for v in s])
    for k in ("samples", "accepted", "final_x", "final_lp", "accept_counts", "swap_attempts", "swap_counts"):
        _same(got[k], ref[k], k)
    assert 0 < int(ref["swap_counts"].sum()) < int(ref["swap_attempts"].sum())


# ---- the scan's order, by hand
def test_scan_order_against_a_hand_computed_ladder_of_four(oracle):
    """fp32, gaps chosen so that the order of the additions shows: h = [0, g0, g1, g2] -> off 1: [0, g0, g1 + g0, g2 + g1] -> off 2:
    [0, g0, g1 + g0, (g2 + g1) + g0].  A serial prefix sum would give (g0 + g1) + g2 in the last place, a different float here."""
    oracle.set_dtype("f32")
    f = np.float32
    g0, g1, g2 = f(1.0), f(2.0 ** -24), f(2.0 ** -24)
    assert (g2 + g1) + g0 == f(1.0 + 2.0 ** -23) and (g0 + g1) + g2 == f(1.0)      # the two orders differ
    h = A.scan([f(0), g0, g1, g2])
    assert [float(v) for v in h] == [0.0, 1.0, 1.0, float(f(1.0 + 2.0 ** -23))]
    # and the whole derivation: exp(log g) is not g in general, so the gaps are taken from the restatement's own g
    rho = [f(0.25), f(-1.5), f(-0.75)]
    g = [A.exp(v) for v in rho]
    want_h = [f(0), g[0], g[1] + g[0], (g[2] + g[1]) + g[0]]
    beta, s = A.ladder(rho)
    assert beta[0] == f(1) and s[0] == f(1)
    for i in (1, 2, 3):
        assert beta[i] == A.exp(-want_h[i]) and s[i] == A.exp(f(0.5) * want_h[i])
    # R = 8: off = 4 adds the scanned h[i - 4]
    h8 = A.scan([f(i) for i in range(8)])
    assert [float(v) for v in h8] == [float(sum(range(i + 1))) for i in range(8)]


def test_rho0_and_the_step_sizes_are_the_host_formulas(oracle, real):
    r_ = oracle.real()
    b = [1.0, 0.5, 0.2, 0.05]
    got = A.rho0(b, -10.0, A.default_rho_max(4))
    assert [float(v) for v in got] == [float(r_(math.log(math.log(b[q] / b[q + 1])))) for q in range(3)]
    assert float(A.rho0([1.0, 1e-30], -10.0, 1.0)[0]) == 1.0 and float(A.rho0([1.0, 1.0 - 1e-9], -10.0, 1.0)[0]) == -10.0     # clamped
    assert [float(v) for v in A.gammas(0.5, 0.75, 3)] == [float(r_(0.5 * math.pow(s, -0.75))) for s in (1, 2, 3)]
    assert A.default_rho_max(64) == math.log(16.0 / 63.0)


# ---- the GPU parity cases: inputs here, chains restated once per width and shared with tests/test_gpu_tempered_adaptive.py
def _geometric(R, ratio):
    return [ratio ** q for q in range(R)]


# name -> dict(R, nladders, d, swap_every, adapt_steps, N (discard 0, thinning 1: N - 1 transitions), kind, sigma, betas, seed, first,
#              target, and the adaptation's parameters where they are not the defaults)
PARITY = {
    "r2_no_odd_pairs": dict(R=2, nladders=3, d=1, swap_every=2, adapt_steps=21, N=41, kind="iso", sigma=1.5, betas=[1.0, 0.3],
                            seed=0xAD01, first=2, target="iso_gauss"),
    "r4_every_third": dict(R=4, nladders=9, d=2, swap_every=3, adapt_steps=25, N=37, kind="iso", sigma=0.9, betas=_geometric(4, 0.45),
                           seed=0xAD02, first=8, target="iso_gauss"),
    "r8_diag_bimodal_partial_wave": dict(R=8, nladders=5, d=2, swap_every=2, adapt_steps=27, N=41, kind="diag", sigma=[0.8, 1.3],
                                         betas=_geometric(8, 0.6), seed=0xAD03, first=16, target="bimodal", c=0.5),
    "r32_two_ladders_share_a_wave": dict(R=32, nladders=4, d=1, swap_every=2, adapt_steps=29, N=41, kind="iso", sigma=1.2,
                                         betas=_geometric(32, 0.7), seed=0xAD04, first=96, target="iso_gauss", c=0.25, kappa=0.75, rho_max=0.9,
                                         target_rate=0.5),
    "r64_scan_crosses_the_rows": dict(R=64, nladders=2, d=2, swap_every=2, adapt_steps=31, N=41, kind="iso", sigma=1.0,
                                      betas=_geometric(64, 0.5), seed=0xAD05, first=0, target="iso_gauss", c=0.25, rho_max=0.2,
                                      target_rate=0.3),
}
ADAPT_KEYS = ("target_rate", "c", "kappa", "rho_min", "rho_max")
_restated = {}


def restated(mhx, oracle, name, real):
    """the restated chains of a parity case in the current width (computed once per session)"""
    key = (name, real)
    if key not in _restated:
        c = PARITY[name]
        _, target = FIXED.parity_model_and_target(mhx, oracle, c)
        _restated[key] = A.run(target, oracle.PROP_ISO if c["kind"] == "iso" else oracle.PROP_DIAG, FIXED.parity_sigma(oracle, c), c["betas"],
                               c["N"], c["seed"], c["first"], c["R"] * c["nladders"], adapt_steps=c["adapt_steps"], swap_every=c["swap_every"],
                               **{k: c[k] for k in ADAPT_KEYS if k in c})
    return _restated[key]


@pytest.mark.parametrize("name", sorted(PARITY))
def test_parity_inputs_exercise_both_outcomes_of_every_pair_and_move_every_rho(mhx, oracle, real, name):
    """a GPU parity test on these inputs cannot pass with swaps never or always taken, with accepts never or always taken, with a rho
    that never moves or with a rho that only sits at a clamp; beta stays strictly decreasing from beta[0] == 1 after every round"""
    c = PARITY[name]
    assert 20 <= c["N"] - 1 <= 40 and 0 < c["adapt_steps"] < c["N"] - 1 and c["adapt_steps"] % c["swap_every"] != 0
    ref = restated(mhx, oracle, name, real)
    att, swp = ref["swap_attempts"].sum(axis=0), ref["swap_counts"].sum(axis=0)
    print(name, real, "attempts", att.tolist(), "swaps", swp.tolist())
    assert att.shape == (c["R"] - 1,)
    assert (swp > 0).all() and (swp < att).all(), (att, swp)
    nT = c["N"] - 1
    per_rung = ref["accept_counts"].reshape(-1, c["R"]).sum(axis=0)
    assert (per_rung > 0).all() and (per_rung < nT * c["nladders"]).all(), per_rung
    lo, hi = c.get("rho_min", A.DEFAULTS["rho_min"]), c.get("rho_max", A.default_rho_max(c["R"]))
    start = np.array(A.rho0(c["betas"], lo, hi), dtype=oracle.real())
    assert (start > oracle.real()(lo)).all() and (start < oracle.real()(hi)).all(), "rho0 sits at a clamp"
    assert (ref["rho"] != start[None, :]).all(), "a rho never moved"
    assert (ref["rho"] > oracle.real()(lo)).all() and (ref["rho"] < oracle.real()(hi)).all(), "a rho ends at a clamp"
    rounds = ref["betas_rounds"]
    assert rounds.shape == (nT // c["swap_every"], c["nladders"], c["R"])
    assert (rounds[:, :, 0] == 1).all() and (np.diff(rounds, axis=2) < 0).all() and (rounds > 0).all()
    # frozen after adapt_steps: the rounds past it repeat the last adapting round's ladder
    last = c["adapt_steps"] // c["swap_every"]
    assert (cases.bits(rounds[last:]) == cases.bits(rounds[last - 1])[None]).all()
    assert (cases.bits(rounds[last - 1]) != cases.bits(rounds[0])).any()
    _same(ref["betas"], rounds[-1], "betas at the end")


# ---- the register form at its limit
def _compile_reg(real, d, pk, R, tmp_path, adapt):
    """tests/test_tempered_cpu.py's _compile_reg with the adaptive switch: (scratch bytes, VGPRs, AGPRs, SGPRs, assembly)"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the build needs it too"
    src = tmp_path / "tempered.hip"
    src.write_text('#include "mhx_device_math.h"\n#include "mhx_rwmh_tempered_kernels.h"\n')
    out = tmp_path / ("k_%d_%d_%d_%d.s" % (d, pk, R, adapt))
    cmd = [hipcc, "-x", "hip", "--offload-device-only", "--no-gpu-bundle-output", "-S", "-DMHX_JIT_BUILD=1", "-I" + CSRC,
           "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
           "-mllvm", "-pragma-unroll-threshold=4000000", "-mllvm", "-amdgpu-unroll-threshold-private=100000",
           "-DMHX_REAL64=%d" % (1 if real == "f64" else 0), "-DMHX_JIT_TEMPERED_REG=1", "-DMHX_JIT_DIM=%d" % d, "-DMHX_JIT_TK=0",
           "-DMHX_JIT_PK=%d" % pk, "-DMHX_JIT_R=%d" % R] + (["-DMHX_JIT_ADAPT=1"] if adapt else []) + ["-o", str(out), str(src)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-2000:]
    assert "not unrolled" not in done.stdout, done.stdout[-2000:]
    text = out.read_text()
    fig = [max(int(v) for v in re.findall(r"\.%s:\s*(\d+)" % key, text)) for key in
           ("private_segment_fixed_size", "vgpr_count", "agpr_count", "sgpr_count")]
    return fig + [text]


def _reg_max_dim(real):
    hdr = open(os.path.join(CSRC, "mhx_rwmh_tempered_kernels.h")).read()
    m = re.search(r"#define\s+MHX_TEMPERED_REG_MAX_DIM\s+\(MHX_REAL64 \? (\d+) : (\d+)\)", hdr)
    assert m, "MHX_TEMPERED_REG_MAX_DIM not found"
    return int(m.group(1) if real == "f64" else m.group(2))


# what the fixed-ladder register kernel compiled to before the adaptive variant shared its header, at MHX_TEMPERED_REG_MAX_DIM, R = 64:
# (width, proposal kind) -> (scratch bytes, VGPRs, AGPRs, SGPRs)
FIXED_FIGURES = {("f32", 0): (0, 414, 158, 66), ("f32", 1): (0, 493, 237, 66), ("f64", 0): (0, 414, 158, 106), ("f64", 1): (0, 512, 256, 106)}


@pytest.mark.parametrize("pk", [0, 1])
def test_adaptive_register_form_compiles_without_scratch_at_the_dimension_limit(real, tmp_path, pk):
    """d = MHX_TEMPERED_REG_MAX_DIM, R = 64, cross-compiled for gfx950 with the options of the run-time build: the adaptive kernel has
    no scratch memory and holds the scan's cross-row fetches; the fixed-ladder kernel of the same header has the figures it had"""
    d = _reg_max_dim(real)
    scratch, vgpr, agpr, sgpr, text = _compile_reg(real, d, pk, 64, tmp_path, True)
    print("adaptive", real, pk, scratch, vgpr, agpr, sgpr)
    assert scratch == 0, "d = %d, proposal kind %d [%s]: %d bytes of scratch" % (d, pk, real, scratch)
    assert "mhx_jit_tempered_adapt_reg" in text and not re.search(r"^mhx_jit_tempered_reg:", text, flags=re.M)
    words = 2 if real == "f64" else 1
    # the exchange of x and lp as in the fixed kernel, and beyond it the scan: the fetch of g and six steps by ds_bpermute (R = 64
    # crosses the rows), the odd partner's beta -- at launch start and again in the adapting round
    assert len(re.findall(r"ds_bpermute_b32", text)) >= words * (d + 1) + 2 * words * 8
    fixed = _compile_reg(real, d, pk, 64, tmp_path, False)
    assert tuple(fixed[:4]) == FIXED_FIGURES[(real, pk)], fixed[:4]
    assert "mhx_jit_tempered_adapt_reg" not in fixed[4]


def test_a_ladder_inside_a_row_scans_by_dpp_row_shifts(real, tmp_path):
    """R = 8: the fetch of g and the three steps of the scan are row_shr DPP moves, one per 32-bit word, and no step beyond R is emitted"""
    _, _, _, _, text = _compile_reg(real, 3, 0, 8, tmp_path, True)
    words = 2 if real == "f64" else 1
    for off, times in ((1, 2), (2, 1), (4, 1)):
        n = len(re.findall(r"v_mov_b32_dpp .*row_shr:%d\b" % off, text))
        assert n >= 2 * words * times and n % (words * times) == 0, (off, n)      # launch start and the adapting round
    assert not re.search(r"row_shr:8\b", text)


# ---- declared, exported, bound, guarded
def test_entry_points_are_declared_exported_and_guarded(mhx):
    hdr = open(os.path.join(ROOT, "include", "mhx.h")).read()
    for name in ("mhx_rwmh_create_tempered_adaptive", "mhx_run_ladder_betas"):
        assert name in mhx.EXPORTS and hasattr(mhx.lib(), name) and ("int %s(" % name) in hdr
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
        assert name not in open(os.path.join(ROOT, "advancedmh.jl_amd", "julia", "AdvancedMHHIP.jl")).read()
    assert "mhx_ladder_adapt_cfg" in hdr
    want = [("adapt_steps", C.c_int32)] + [(n, C.c_double) for n in ("target_rate", "c", "kappa", "rho_min", "rho_max")]
    assert list(mhx._lib.LadderAdaptCfg._fields_) == want
    for name in ("betas", "ladder"):
        assert hasattr(mhx.Run, name)
    lib = C.CDLL(mhx.LIB_PATH)
    lib.mhx_last_error.restype = C.c_char_p
    assert lib.mhx_rwmh_create_tempered_adaptive(None, None, None, None, None, None) == mhx.MHX_EINVAL
    assert lib.mhx_last_error().decode() == "mhx_rwmh_create_tempered_adaptive: handle is NULL"
    assert lib.mhx_run_ladder_betas(None, None) == mhx.MHX_EINVAL and lib.mhx_last_error().decode() == "mhx_run_ladder_betas: handle is NULL"
    api = open(os.path.join(CSRC, "mhx_api.hip")).read()
    assert "KF_TEMPERED_ADAPT = 17" in api and '"tempered_adapt_reg" : "tempered_adapt_generic"' in api
    assert "k_tempered_adapt_generic" in open(os.path.join(CSRC, "mhx_api_tempered.inc")).read()
    # the switch enters the run-time kernel key as a define of its own; the fixed ladder's list of defines is untouched
    inc = open(os.path.join(CSRC, "mhx_api_tempered.inc")).read()
    assert 'if (ac) rdefs.push_back("MHX_JIT_ADAPT=1")' in inc and 'if (ac) gdefs.push_back("MHX_JIT_ADAPT=1")' in inc


def test_python_mirror_refuses_what_it_can_without_a_device(mhx):
    rw = mhx.RWMH(mhx.MvNormal(mhx.zeros(2), mhx.I))
    b = mhx.geometric_betas(4, 0.05)
    a = mhx.LadderAdaptation(100)
    assert (a.steps, a.target_rate, a.c, a.kappa, a.rho_min, a.rho_max) == (100, 0.234, 1.0, 0.6, None, None)
    cfg = a.cfg()
    assert cfg.adapt_steps == 100 and cfg.c == 1.0 and math.isnan(cfg.rho_min) and math.isnan(cfg.rho_max)
    assert mhx.LadderAdaptation(5, rho_min=-3.0, rho_max=0.5).cfg().rho_max == 0.5
    t = mhx.Tempered(rw, b, swap_every=2, adapt=a)
    assert t.adapt is a and mhx.Tempered(rw, b).adapt is None
    for words, make in ((["steps"], lambda: mhx.LadderAdaptation(-1)),
                        (["kappa", "(0.5, 1]"], lambda: mhx.LadderAdaptation(10, kappa=0.5)),
                        (["kappa", "(0.5, 1]"], lambda: mhx.LadderAdaptation(10, kappa=1.25)),
                        (["c ="], lambda: mhx.LadderAdaptation(10, c=-0.1)),
                        (["target_rate", "(0, 1)"], lambda: mhx.LadderAdaptation(10, target_rate=1.0)),
                        (["target_rate", "(0, 1)"], lambda: mhx.LadderAdaptation(10, target_rate=0.0)),
                        (["rho_min", "rho_max"], lambda: mhx.LadderAdaptation(10, rho_min=1.0, rho_max=0.0)),
                        (["scales", "follow"], lambda: mhx.Tempered(rw, b, scales=[1.0, 1.5, 2.0, 3.0], adapt=a)),
                        (["swap_every = 0"], lambda: mhx.Tempered(rw, b, swap_every=0, adapt=a)),
                        (["LadderAdaptation"], lambda: mhx.Tempered(rw, b, adapt=100))):
        with pytest.raises(mhx.ArgumentError) as ei:
            make()
        for w in words:
            assert w in str(ei.value), str(ei.value)
    # sample() names its rule before it touches a device
    model = mhx.DensityModel(mhx.IsoGaussian(2))
    with pytest.raises(mhx.ArgumentError) as ei:
        mhx.sample(model, t, 10, 4, discard_initial=99)
    assert "discard_initial" in str(ei.value) and "adapt.steps = 100" in str(ei.value)
    table = mhx.LadderTable([dict(rung=0, beta_median=1.0, beta_min=1.0, beta_max=1.0, rate=0.25),
                             dict(rung=1, beta_median=0.5, beta_min=0.4, beta_max=0.6, rate=float("nan"))])
    assert "swap rate" in str(table).splitlines()[0] and "0.250" in str(table) and len(str(table).splitlines()) == 3
