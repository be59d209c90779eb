"""CPU (no GPU): the restatement of the anchored-ladder arithmetic (tests/tempered_anchored_restatement.py)
pinned to the oracle, the detailed balance of its swap where a forgotten lq shows, the log evidence of a Gaussian path against its
closed form, the inputs of the GPU cases (tests/test_gpu_tempered_anchored.py shares them and their restated chains), the register
form's own dimension limit, and the guards of the new entry points."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases
import tempered_anchored_restatement as A
import test_tempered_adaptive_cpu as ADAPT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "advancedmh.jl_amd", "csrc")


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    assert a.dtype == b.dtype, "%s: dtypes %s / %s" % (what, a.dtype, b.dtype)
    bad = np.argwhere(cases.bits(a) != cases.bits(b))
    assert len(bad) == 0, "%s: %d mismatches, first at %s: %r vs %r" % (what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


# ---- the cold rung is the oracle's plain chain whatever the reference: loga degenerates exactly
@pytest.mark.parametrize("kind", ["iso", "diag"])
def test_restatement_with_unit_betas_and_no_swaps_is_the_oracles_rwmh(oracle, real, kind):
    O = oracle
    d, Cn, N, seed, first = 3, 6, 14, 0xA7C, 4
    vec = np.linspace(0.4, 1.1, d).astype(O.real())
    prop = O.Proposal(O.PROP_ISO, 0.7) if kind == "iso" else O.Proposal(O.PROP_DIAG, vec=vec)
    for sched, init in ((O.schedule(N), None), (O.schedule(N, 3, 2), np.random.default_rng(2).normal(size=(d, Cn)).astype(O.real()))):
        ref = O.rwmh(O.iso_gauss(d), prop, sched, seed, first, Cn, init=init)
        got = A.run(O.iso_gauss(d), O.PROP_ISO if kind == "iso" else O.PROP_DIAG, 0.7 if kind == "iso" else vec, [1.0, 1.0],
                    [0.3, -2.0, 11.0], [0.5, 3.0, 0.01], N, seed, first, Cn, swap_every=0, scales=[1.0, 1.0],
                    discard_initial=sched.discard_initial, thinning=sched.thinning, init=init)
        for k in ("samples", "accepted", "final_x", "final_lp", "accept_counts"):
            _same(got[k], ref[k], k)
        assert 0 < int(ref["accept_counts"].sum()) < Cn * (sched.discard_initial + (N - 1) * sched.thinning)


# ---- the Gaussian path: f = exp(-|x - a|^2 / (2 s^2)), q = N(m, t^2 I); rung beta is N(mu_beta, I / P_beta)
def path_moments(beta, a, s, m, t):
    """(P_beta, mu_beta, E_beta[u]) with u = log f - log q"""
    a, m = np.asarray(a, dtype=np.float64), np.asarray(m, dtype=np.float64)
    d = a.size
    P = beta / s ** 2 + (1.0 - beta) / t ** 2
    mu = (beta * a / s ** 2 + (1.0 - beta) * m / t ** 2) / P
    eu = -(d / P + ((mu - a) ** 2).sum()) / (2 * s ** 2) + (d / P + ((mu - m) ** 2).sum()) / (2 * t ** 2) + d * math.log(t) + 0.5 * d * math.log(2 * math.pi)
    return P, mu, eu


# ---- detailed balance of the anchored swap; a swap that forgets lq does not keep it
def _pooled(oracle, swap_lq):
    O = oracle
    nl, burn, N = 256, 40, 160
    a, s, m, t, betas = [0.0], 1.0, [3.0], 2.0, [1.0, 0.25]
    res = A.run(O.iso_gauss(1), O.PROP_ISO, 2.4, betas, m, [t], N, 0xDB2, 0, 2 * nl, swap_every=1, scales=[1.0, 1.5],
                discard_initial=burn, swap_lq=swap_lq)
    x = res["samples"][:, 0, :].astype(np.float64)
    out = []
    for rung in (0, 1):
        P, mu, _ = path_moments(betas[rung], a, s, m, t)
        per_ladder = ((x[:, rung::2] - mu[0]) ** 2).mean(axis=0)       # E (x - mu)^2 about the known mean: unbiased for a stationary chain
        out.append((per_ladder.mean(), per_ladder.std(ddof=1) / np.sqrt(nl), 1.0 / P))
    return out, res


def test_detailed_balance_of_the_anchored_swap_and_that_a_forgotten_lq_fails_it(oracle):
    oracle.set_dtype("f64")
    (cold, hot), res = _pooled(oracle, True)
    print("cold %.4f +- %.4f (%.4f), hot %.4f +- %.4f (%.4f), swaps %d of %d" % (cold + hot + (res["swap_counts"].sum(), res["swap_attempts"].sum())))
    assert abs(cold[0] - cold[2]) < 5 * cold[1] and abs(hot[0] - hot[2]) < 5 * hot[1]
    assert 0 < res["swap_counts"].sum() < res["swap_attempts"].sum()
    (coldf, hotf), _ = _pooled(oracle, False)
    print("lq forgotten: cold %.4f +- %.4f, hot %.4f +- %.4f" % (coldf[:2] + hotf[:2]))
    assert not (abs(coldf[0] - coldf[2]) < 5 * coldf[1] and abs(hotf[0] - hotf[2]) < 5 * hotf[1])


# ---- the known answer, shared with the GPU test
def offset_gauss(x):
    """log f(x) = -|x - a|^2 / (2 s^2), a = (1, -0.5), s = 0.8 (1 / s^2 = 1.5625 exactly), unnormalised: log Z = log(2 pi s^2)"""
    return -0.5 * (((x[0] - 1.0) * (x[0] - 1.0) + (x[1] + 0.5) * (x[1] + 0.5)) * 1.5625)


KNOWN = dict(a=[1.0, -0.5], s=0.8, m=[0.4, 0.1], t=1.5, R=8, nladders=32, N=120, discard=60, thinning=2, seed=0xE71D, first=0, sigma=1.2)
KNOWN["log_z"] = math.log(2 * math.pi * KNOWN["s"] ** 2)
_known = {}


def known_betas(mhx):
    return mhx.power_betas(KNOWN["R"], 3.0)


def known_scales(mhx):
    """the rung's own standard deviation over the cold rung's: the walk keeps its acceptance rate down the ladder"""
    k = KNOWN
    P1 = path_moments(1.0, k["a"], k["s"], k["m"], k["t"])[0]
    return [1.0] + [math.sqrt(P1 / path_moments(float(b), k["a"], k["s"], k["m"], k["t"])[0]) for b in known_betas(mhx)[1:]]


def known_model_and_target(mhx, oracle):
    import user_targets
    model = mhx.DensityModel(offset_gauss, dim=2)
    return model, user_targets.host_target(oracle, model.traced.source, 2, data=model.traced.data)


def known_restated(mhx, oracle, real):
    """(restated run, u [N][C], evidence table, magnitudes) of the known-answer case in the current width, once per session"""
    if real not in _known:
        k = KNOWN
        _, target = known_model_and_target(mhx, oracle)
        b = known_betas(mhx)
        res = A.run(target, oracle.PROP_ISO, k["sigma"], b, k["m"], [k["t"]] * 2, k["N"], k["seed"], k["first"], k["R"] * k["nladders"],
                    swap_every=1, scales=known_scales(mhx), discard_initial=k["discard"], thinning=k["thinning"])
        u = A.u_of_samples(res["samples"], b, k["m"], [k["t"]] * 2)
        table, mag = A.evidence_table(u, b)
        _known[real] = (res, u, table, mag)
    return _known[real]


def test_log_evidence_of_a_gaussian_path_against_its_closed_form(mhx, oracle, real):
    k = KNOWN
    res, u, table, _ = known_restated(mhx, oracle, real)
    R, nl = k["R"], k["nladders"]
    betas = np.array([float(oracle.real()(b)) for b in known_betas(mhx)])
    ev = mhx.evidence_from_table(table, betas, k["N"])
    print(ev)
    att, swp = res["swap_attempts"].sum(axis=0), res["swap_counts"].sum(axis=0)
    assert (swp > 0).all() and (swp < att).all(), (att, swp)
    exact_u = np.array([path_moments(b, k["a"], k["s"], k["m"], k["t"])[2] for b in betas])
    per_ladder = u.mean(axis=0).reshape(nl, R)
    for r_ in range(R):
        mean, se = per_ladder[:, r_].mean(), per_ladder[:, r_].std(ddof=1) / math.sqrt(nl)
        print("rung %d beta %.5f  mean u %.5f +- %.5f  exact %.5f" % (r_, betas[r_], mean, se, exact_u[r_]))
        assert abs(mean - exact_u[r_]) < 4 * se
        assert abs(ev["rungs"][r_]["mean_u"] - mean) < 1e-9 * max(1.0, abs(mean)) and ev["rungs"][r_]["n"] == nl * k["N"]
    ti_exact = float(((betas[:-1] - betas[1:]) * 0.5 * (exact_u[:-1] + exact_u[1:])).sum())
    print("exact log Z %.5f, trapezoid of the exact rung means %.5f" % (k["log_z"], ti_exact))
    assert abs(ev["log_z_ti"] - ti_exact) < 4 * ev["se_ti"]
    assert abs(ev["log_z_ss"] - k["log_z"]) < 4 * ev["se_ss"]
    assert abs(ev["log_z_ss_backward"] - k["log_z"]) < 4 * ev["se_ss_backward"]
    lo, hi = sorted((ev["log_z_ss"], ev["log_z_ss_backward"]))
    assert lo <= k["log_z"] <= hi or hi - lo <= ev["se_ss"] + ev["se_ss_backward"]
    for name in ("se_ti", "se_ss", "se_ss_backward"):
        assert 0 < ev[name] <= 0.05, (name, ev[name])
    assert ev["bad"] == 0 and math.isfinite(ev["log_z_ti_coarse"])
    bf = mhx.bayes_factor(ev, ev)
    assert bf["log_bf"] == 0.0 and bf["se"] == pytest.approx(math.sqrt(2) * ev["se_ss"])
    assert "stepping stone" in str(ev) and len(str(ev).splitlines()) == 4 + R


def test_evidence_of_two_rungs_has_no_coarse_rule_and_one_ladder_no_standard_error(mhx):
    t = np.zeros((2, 8))
    t[:, 1], t[:, 2], t[:, 3] = [1.0, 3.0], [0.5, -0.5], [2.0, 2.0]
    t[0, 4:] = [-np.inf, 0.0, -1.0, 5.0]
    t[1, 4:] = [3.0, 5.0, -np.inf, 0.0]
    ev = mhx.evidence_from_table(t, [1.0, 0.0], 5)
    assert math.isnan(ev["log_z_ti_coarse"]) and math.isnan(ev["se_ss"]) and math.isnan(ev["se_ti"])
    assert ev["log_z_ti"] == pytest.approx(0.5 * (1.1 + 2.9)) and ev["log_z_ss"] == pytest.approx(3.0) and ev["log_z_ss_backward"] == pytest.approx(1.0)


# ---- the register form at its own limit
def _anchored_max_dim(real):
    hdr = open(os.path.join(CSRC, "mhx_rwmh_tempered_kernels.h")).read()
    m = re.search(r"#define\s+MHX_TEMPERED_ANCHORED_REG_MAX_DIM\s+\(MHX_REAL64 \? (\d+) : (\d+)\)", hdr)
    assert m, "MHX_TEMPERED_ANCHORED_REG_MAX_DIM not found"
    return int(m.group(1) if real == "f64" else m.group(2))


def _compile_anchored(real, d, pk, tmp_path):
    """the anchored register kernel as the run-time build compiles it: (scratch bytes, VGPRs, AGPRs, SGPRs, assembly), read as
    tests/test_tempered_adaptive_cpu.py reads them"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the build needs it too"
    src = tmp_path / "tempered.hip"
    src.write_text('#include "mhx_device_math.h"\n#include "mhx_rwmh_tempered_kernels.h"\n')
    out = tmp_path / ("k_%d_%d.s" % (d, pk))
    cmd = [hipcc, "-x", "hip", "--offload-device-only", "--no-gpu-bundle-output", "-S", "-DMHX_JIT_BUILD=1", "-I" + CSRC,
           "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
           "-mllvm", "-pragma-unroll-threshold=4000000", "-mllvm", "-amdgpu-unroll-threshold-private=100000",
           "-DMHX_REAL64=%d" % (1 if real == "f64" else 0), "-DMHX_JIT_TEMPERED_REG=1", "-DMHX_JIT_DIM=%d" % d, "-DMHX_JIT_TK=0",
           "-DMHX_JIT_PK=%d" % pk, "-DMHX_JIT_R=64", "-DMHX_JIT_ANCHOR=1", "-o", str(out), str(src)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-2000:]
    assert "not unrolled" not in done.stdout, done.stdout[-2000:]
    text = out.read_text()
    fig = [max(int(v) for v in re.findall(r"\.%s:\s*(\d+)" % key, text)) for key in
           ("private_segment_fixed_size", "vgpr_count", "agpr_count", "sgpr_count")]
    return fig + [text]


@pytest.mark.parametrize("pk", [0, 1])
def test_anchored_register_form_compiles_without_scratch_at_its_limit_and_not_above(real, tmp_path, pk):
    """d = MHX_TEMPERED_ANCHORED_REG_MAX_DIM, R = 64, cross-compiled for gfx950 with the options of the run-time build: no scratch
    memory, ISO and DIAG; at the next size tried (the fixed ladder's limit, which the header must not lower) DIAG spills"""
    d = _anchored_max_dim(real)
    assert d < ADAPT._reg_max_dim(real) == {"f64": 48, "f32": 80}[real]
    inc = open(os.path.join(CSRC, "mhx_api_tempered.inc")).read()
    assert "(ref ? d <= MHX_TEMPERED_ANCHORED_REG_MAX_DIM : d <= MHX_TEMPERED_REG_MAX_DIM)" in inc
    scratch, vgpr, agpr, sgpr, text = _compile_anchored(real, d, pk, tmp_path)
    print("anchored", real, pk, d, scratch, vgpr, agpr, sgpr)
    assert scratch == 0, "d = %d, proposal kind %d [%s]: %d bytes of scratch" % (d, pk, real, scratch)
    assert "mhx_jit_tempered_anchored_reg" in text and not re.search(r"^mhx_jit_tempered_reg:", text, flags=re.M)
    words = 2 if real == "f64" else 1
    # the exchange: x[0..d), u, and under the swap's mask lp and lq, each a DPP move (even rounds) and a ds_bpermute (odd rounds) per word
    assert len(re.findall(r"v_mov_b32_dpp .*quad_perm:\[1,0,3,2\]", text)) >= words * (d + 3)
    assert len(re.findall(r"ds_bpermute_b32", text)) >= words * (d + 3)
    if pk == 1:
        nxt = ADAPT._reg_max_dim(real)
        scratch, vgpr = _compile_anchored(real, nxt, 1, tmp_path)[:2]
        print("anchored", real, pk, nxt, scratch, vgpr)
        assert scratch > 0, "d = %d [%s] compiles without scratch: the limit can move up" % (nxt, real)


# ---- declared, exported, bound, guarded
def test_entry_points_are_declared_exported_and_guarded(mhx):
    hdr = open(os.path.join(ROOT, "include", "mhx.h")).read()
    for name in ("mhx_rwmh_create_tempered_anchored", "mhx_run_evidence"):
        assert name in mhx.EXPORTS and hasattr(mhx.lib(), name) and ("int %s(" % name) in hdr
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
        assert name not in open(os.path.join(ROOT, "advancedmh.jl_amd", "julia", "AdvancedMHHIP.jl")).read()
    assert "mhx_tempered_reference" in hdr
    assert list(mhx._lib.TemperedReference._fields_) == [("mean", C.c_void_p), ("sd", C.c_void_p)]
    # mhx_tempered_cfg is public and mirrored: it stays what it was
    assert list(mhx._lib.TemperedCfg._fields_) == [("R", C.c_int32), ("swap_every", C.c_int32), ("beta", C.c_void_p), ("scale", C.c_void_p)]
    for name in ("evidence", "evidence_table"):
        assert hasattr(mhx.Run, name)
    assert not hasattr(mhx.Group, "evidence")
    lib = C.CDLL(mhx.LIB_PATH)
    lib.mhx_last_error.restype = C.c_char_p
    assert lib.mhx_rwmh_create_tempered_anchored(None, None, None, None, None, None) == mhx.MHX_EINVAL
    assert lib.mhx_last_error().decode() == "mhx_rwmh_create_tempered_anchored: handle is NULL"
    assert lib.mhx_run_evidence(None, None, None) == mhx.MHX_EINVAL and lib.mhx_last_error().decode() == "mhx_run_evidence: handle is NULL"
    api = open(os.path.join(CSRC, "mhx_api.hip")).read()
    assert "KF_TEMPERED_ANCHOR = 18" in api and '"tempered_anchored_reg" : "tempered_anchored_generic"' in api
    inc = open(os.path.join(CSRC, "mhx_api_tempered.inc")).read()
    assert "k_tempered_anchored_generic" in inc
    # the switch enters the run-time kernel key as a define of its own; the other ladders' lists of defines are untouched
    assert 'if (ref) rdefs.push_back("MHX_JIT_ANCHOR=1")' in inc and 'if (ref) gdefs.push_back("MHX_JIT_ANCHOR=1")' in inc
    assert 'if (ac) rdefs.push_back("MHX_JIT_ADAPT=1")' in inc


def test_python_mirror_refuses_what_it_can_without_a_device(mhx):
    rw = mhx.RWMH(mhx.MvNormal(mhx.zeros(2), mhx.I))
    q = mhx.MvNormal(np.array([0.5, -1.0]), np.array([4.0, 0.25]))
    t = mhx.Tempered(rw, [1.0, 0.5, 0.1, 0.0], scales=[1.0, 1.2, 2.0, 3.0], reference=q)
    assert t.reference is q and t.ref_mean.tolist() == [0.5, -1.0] and t.ref_sd.tolist() == [2.0, 0.5]
    iso = mhx.Tempered(rw, [1.0, 0.5], reference=mhx.MvNormal(mhx.zeros(2), 2.25 * mhx.I))
    assert iso.ref_sd.tolist() == [1.5, 1.5] and mhx.Tempered(rw, [1.0, 0.5]).reference is None
    for words, make in ((["reference", "adapt"], lambda: mhx.Tempered(rw, [1.0, 0.5], reference=q, adapt=mhx.LadderAdaptation(10))),
                        (["dense"], lambda: mhx.Tempered(rw, [1.0, 0.5], reference=mhx.MvNormal(mhx.zeros(2), np.array([[1.0, 0.3], [0.3, 1.0]])))),
                        (["MvNormal"], lambda: mhx.Tempered(rw, [1.0, 0.5], reference=(0.0, 1.0))),
                        (["betas[1] = 0", "not the last"], lambda: mhx.Tempered(rw, [1.0, 0.0, 0.5, 0.25], scales=[1, 2, 3, 4], reference=q)),
                        (["betas[3] = 0", "without scales"], lambda: mhx.Tempered(rw, [1.0, 0.5, 0.1, 0.0], reference=q))):
        with pytest.raises(mhx.ArgumentError) as ei:
            make()
        for w in words:
            assert w in str(ei.value), str(ei.value)


def test_power_betas_endpoints_are_exact(mhx):
    for R, p in ((2, 3.0), (8, 3.0), (64, 5.0), (16, 0.5)):
        b = mhx.power_betas(R, p)
        assert b.dtype == np.float64 and b.shape == (R,) and b[0] == 1.0 and b[-1] == 0.0 and (np.diff(b) < 0).all()
        assert np.allclose(b, ((R - 1 - np.arange(R)) / (R - 1.0)) ** p, rtol=1e-15, atol=0)
    assert mhx.power_betas(8)[1] == (6.0 / 7.0) ** 3.0
    for bad in (lambda: mhx.power_betas(1), lambda: mhx.power_betas(8, 0.0)):
        with pytest.raises(mhx.ArgumentError):
            bad()


# ---- the GPU parity cases: inputs here, chains restated once per width and shared with tests/test_gpu_tempered_anchored.py
# name -> dict(R, nladders, d, swap_every, discard, thinning, N, kind, sigma, betas, scales, mean, sd, seed, first, target)
PARITY = {
    # no odd rounds, a partial wave, a DIAG proposal; the ladder ends above 0
    "r2_diag_partial_wave": dict(R=2, nladders=33, d=3, swap_every=1, discard=0, thinning=1, N=12, kind="diag", sigma=[0.8, 1.3, 0.5],
                                 betas=[1.0, 0.3], scales=None, mean=[1.5, -1.0, 0.5], sd=[0.7, 1.6, 0.9], seed=0xA701, first=2,
                                 target="iso_gauss"),
    "r4_thinned_shard": dict(R=4, nladders=19, d=5, swap_every=3, discard=3, thinning=2, N=20, kind="iso", sigma=0.9,
                             betas=[1.0, 0.6, 0.3, 0.1], scales=None, mean=[1.0, -1.0, 0.5, 0.0, -0.5], sd=[0.8, 1.2, 0.6, 1.5, 1.0],
                             seed=0xA702, first=8, target="iso_gauss"),
    # every row boundary of the wave; equal steps in beta and a reference far from the target keep both outcomes alive at all 63 pairs
    "r64_every_row_boundary": dict(R=64, nladders=2, d=1, swap_every=1, discard=0, thinning=1, N=64, kind="iso", sigma=1.5,
                                   betas=[1.0 - r_ / 64.0 for r_ in range(64)], scales=[1.0] * 64, mean=[40.0], sd=[1.0], seed=0xA703,
                                   first=0, target="iso_gauss"),
    # the evidence ladder: last beta exactly 0, user scales, a traced target; 320 chains are two 256-thread blocks of the state-in-HBM form
    "r8_to_zero_user_scales": dict(R=8, nladders=40, d=2, swap_every=2, discard=0, thinning=1, N=24, kind="iso", sigma=1.0,
                                   betas=[((7 - r_) / 7.0) ** 3.0 for r_ in range(8)], scales=[1.0, 1.1, 1.25, 1.5, 1.75, 2.0, 2.25, 2.5],
                                   mean=[0.4, 0.1], sd=[1.5, 1.2], seed=0xA704, first=16, target="offset_gauss"),
}
_restated = {}


def parity_model_and_target(mhx, oracle, case):
    if case["target"] == "iso_gauss":
        return mhx.DensityModel(mhx.IsoGaussian(case["d"])), oracle.iso_gauss(case["d"])
    return known_model_and_target(mhx, oracle)


def parity_sigma(oracle, case):
    return case["sigma"] if case["kind"] == "iso" else np.asarray(case["sigma"], dtype=oracle.real())


def restated(mhx, oracle, name, real):
    """the restated chains of a parity case in the current width (computed once per session)"""
    key = (name, real)
    if key not in _restated:
        c = PARITY[name]
        _, target = parity_model_and_target(mhx, oracle, c)
        _restated[key] = A.run(target, oracle.PROP_ISO if c["kind"] == "iso" else oracle.PROP_DIAG, parity_sigma(oracle, c), c["betas"],
                               c["mean"], c["sd"], c["N"], c["seed"], c["first"], c["R"] * c["nladders"], swap_every=c["swap_every"],
                               scales=c["scales"], discard_initial=c["discard"], thinning=c["thinning"])
    return _restated[key]


@pytest.mark.parametrize("name", sorted(PARITY))
def test_parity_inputs_exercise_both_outcomes_of_every_pair(mhx, oracle, real, name):
    """a GPU parity test on these inputs cannot pass with swaps never or always taken, nor with accepts never or always taken"""
    ref = restated(mhx, oracle, name, real)
    att, swp = ref["swap_attempts"].sum(axis=0), ref["swap_counts"].sum(axis=0)
    print(name, real, "attempts", att.tolist(), "swaps", swp.tolist())
    c = PARITY[name]
    assert att.shape == (c["R"] - 1,)
    assert (swp > 0).all() and (swp < att).all(), (att, swp)
    nT = c["discard"] + (c["N"] - 1) * c["thinning"]
    per_rung = ref["accept_counts"].reshape(-1, c["R"]).sum(axis=0)
    assert (per_rung > 0).all() and (per_rung < nT * c["nladders"]).all(), per_rung
