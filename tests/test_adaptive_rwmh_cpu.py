"""CPU (no GPU): the restatement of the adaptive random-walk arithmetic (tests/adaptive_rwmh_restatement.py)
against an independent transcription and against the oracle's plain chain where nothing adapts, the inputs of the GPU parity cases
(tests/test_gpu_adaptive_rwmh.py shares them and their restated chains), the tuning claim, the register forms' dimension limits, the
Python mirror's checks and the guards of the new entry points."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_rwmh_restatement as A
import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "advancedmh.jl_amd", "csrc")


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    assert a.dtype == b.dtype, "%s: dtypes %s / %s" % (what, a.dtype, b.dtype)
    bad = np.argwhere(cases.bits(a) != cases.bits(b))
    assert len(bad) == 0, "%s: %d mismatches, first at %s: %r vs %r" % (what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


# ---- an independent scalar transcription of DESIGN.md section 3.18 for ONE chain: the spec's sentences in their order, nothing shared
# with the restatement but the oracle's primitives and libm's fma
def _transcription(O, target, s, steps, adapt_steps, shape, seed, cid, target_rate, c, kappa, lam_min, lam_max):
    T = O.real()
    d = len(s)
    s = [T(v) for v in s]
    n0 = O.normals(seed, cid, 0, O.STREAM_INIT, d)
    x = np.array([A.fma(s[k], n0[k], T(0)) for k in range(d)], dtype=T)
    lp = T(target(x))
    lam = T(0)
    sig, eff = np.array(s, dtype=T), np.array(s, dtype=T)
    m, v = x.copy(), np.array([s[k] * s[k] for k in range(d)], dtype=T)
    nacc, frz = 0, 0
    with np.errstate(all="ignore"):
        for t in range(1, steps + 1):
            n = O.normals(seed, cid, t, O.STREAM_PROPOSAL, d)
            y = np.array([A.fma(eff[k], n[k], x[k]) for k in range(d)], dtype=T)
            lpy = T(target(y))
            loga = T(lpy - lp)
            if T(O.accept_logu(seed, cid, t)) < loga:
                x, lp, nacc = y, lpy, nacc + 1
            if t <= adapt_steps:
                if math.isnan(float(loga)):
                    p = T(0)
                elif loga >= 0:
                    p = T(1)
                else:
                    p = T(O.exp(loga)[0])
                g = T(min(1.0, c * math.pow(float(t), -kappa)))
                lam = A.fma(g, T(p - T(target_rate)), lam)
                lam = T(lam_min) if lam < T(lam_min) else (T(lam_max) if lam > T(lam_max) else lam)
                if shape:
                    for k in range(d):
                        delta = T(x[k] - m[k])
                        m1 = A.fma(g, delta, m[k])
                        v1 = A.fma(g, A.fma(delta, delta, T(-v[k])), v[k])
                        vlo, vhi = T(float(s[k]) ** 2 * 2.0 ** -40), T(float(s[k]) ** 2 * 2.0 ** 40)
                        v1 = vlo if v1 < vlo else (vhi if v1 > vhi else v1)
                        if math.isfinite(float(m1)) and math.isfinite(float(v1)):
                            m[k], v[k], sig[k] = m1, v1, np.sqrt(T(v1))
                el = T(O.exp(lam)[0])
                eff = np.array([T(sig[k] * el) for k in range(d)], dtype=T)
            if t == adapt_steps:
                frz = nacc
    return dict(x=x, lp=lp, nacc=nacc, lam=lam, sd=eff, mean=m, var=v, frz=frz)


@pytest.mark.parametrize("shape", [False, True])
def test_restatement_against_an_independent_scalar_transcription(oracle, real, shape):
    O = oracle
    d, steps, adapt_steps, seed, cid = 3, 40, 25, 0xAD01, 11
    sig = np.array([0.6, 1.4, 2.2])
    Sigma = np.diag([0.25, 4.0, 30.0])
    target = O.corr_gauss_from_cov(Sigma)
    ref = A.run(target, O.PROP_DIAG, np.asarray(sig, dtype=O.real()), steps + 1, seed, cid, 1, adapt_steps, shape=shape, c=0.8, kappa=0.7,
                target_rate=0.3, lam_min=-0.5, lam_max=0.25)
    t = _transcription(O, target, np.asarray(sig, dtype=O.real()), steps, adapt_steps, shape, seed, cid, 0.3, 0.8, 0.7, -0.5, 0.25)
    _same(ref["final_x"][:, 0], t["x"], "x")
    _same(ref["final_lp"][:1], np.array([t["lp"]], dtype=O.real()), "lp")
    assert int(ref["accept_counts"][0]) == t["nacc"] and 0 < t["nacc"] < steps
    assert int(ref["acc_at_freeze"][0]) == t["frz"]
    _same(ref["lam"][:1], np.array([t["lam"]], dtype=O.real()), "lam")
    _same(ref["sd"][:, 0], t["sd"], "sd")
    if shape:
        _same(ref["mean"][:, 0], t["mean"], "mean")
        _same(ref["var"][:, 0], t["var"], "var")
    else:
        assert np.isnan(ref["mean"]).all()
    # the run exercised both clamps of lam, or at least moved it
    assert float(ref["lam"][0]) != 0.0


@pytest.mark.parametrize("kind", ["iso", "diag"])
def test_restatement_with_no_adapting_transition_is_the_oracles_rwmh(oracle, real, kind):
    """adapt_steps = 0: eff is the configured s itself for the whole run, so the chains are the oracle's plain random walk"""
    O = oracle
    d, n, N = 5, 3, 12
    sigma = 0.7 if kind == "iso" else np.array([0.5, 0.9, 1.3, 0.2, 2.0], dtype=O.real())
    target = O.iso_gauss(d)
    ref = A.run(target, O.PROP_ISO if kind == "iso" else O.PROP_DIAG, sigma, N, 0xAD02, 5, n, 0, shape=(kind == "diag"), discard_initial=2, thinning=3)
    prop = O.Proposal(O.PROP_ISO, scale=sigma) if kind == "iso" else O.Proposal(O.PROP_DIAG, vec=sigma)
    want = O.rwmh(target, prop, O.schedule(N, 2, 3), 0xAD02, 5, n)
    for key in ("samples", "accepted", "final_x", "final_lp", "accept_counts"):
        _same(ref[key], want[key], key)
    assert (ref["acc_at_freeze"] == 0).all() and (ref["lam"] == 0).all()


# ---- the GPU parity cases (tests/test_gpu_adaptive_rwmh.py), restated once per session and width
# N = 24, adapt_steps = 10, discard_initial = 2, thinning = 3: records at transitions 2, 5, 8, 11, ... fall on both sides of the seam
SCHEDULE = dict(N=24, adapt_steps=10, discard=2, thinning=3)
_DIAG = {1: [0.45], 2: [0.8, 0.35], 3: [0.3, 1.7, 0.9], 5: [0.3, 1.7, 0.9, 2.4, 0.6]}
PARITY = {
    "d1_partial_wave_iso": dict(d=1, n=70, first=0, kind="iso", sigma=1.8, shape=False, seed=0xAD10, target="scaled_gauss"),
    "d3_shard_diag_shape": dict(d=3, n=130, first=7, kind="diag", sigma=_DIAG[3], shape=True, seed=0xAD11, target="scaled_gauss"),
    "d5_partial_wave_iso_shape": dict(d=5, n=70, first=0, kind="iso", sigma=0.4, shape=True, seed=0xAD12, target="scaled_gauss"),
    "d5_shard_diag": dict(d=5, n=130, first=7, kind="diag", sigma=_DIAG[5], shape=False, seed=0xAD13, target="scaled_gauss"),
    "d1_shard_diag_shape": dict(d=1, n=130, first=7, kind="diag", sigma=_DIAG[1], shape=True, seed=0xAD14, target="scaled_gauss"),
    "d3_partial_wave_iso": dict(d=3, n=70, first=0, kind="iso", sigma=2.5, shape=False, seed=0xAD15, target="scaled_gauss"),
    "user_target_diag_shape": dict(d=3, n=70, first=0, kind="diag", sigma=_DIAG[3], shape=True, seed=0xAD16, target="user_shifted"),
    "bounded_support_iso_shape": dict(d=2, n=70, first=0, kind="iso", sigma=1.5, shape=True, seed=0xAD17, target="user_nig"),
}
_restated = {}


def register_limits(real):
    """(adapting, adapting with shape, frozen) limits of the register forms in the width, from the kernels' header"""
    hdr = open(os.path.join(CSRC, "mhx_rwmh_adaptive_kernels.h")).read()
    out = []
    for name in ("MHX_ADAPT_REG_MAX_DIM", "MHX_ADAPT_SHAPE_REG_MAX_DIM", "MHX_ADAPT_FROZEN_REG_MAX_DIM"):
        m = re.search(r"#define\s+%s\s+\(MHX_REAL64 \? (\d+) : (\d+)\)" % name, hdr)
        assert m, "%s not found" % name
        out.append(int(m.group(1) if real == "f64" else m.group(2)))
    return tuple(out)


def parity_case(name, real):
    if name == "above_the_register_limit":
        # shape on, d = the adapting register form's limit + 4: that phase must run from HBM (the frozen one still fits its own limit)
        d = register_limits(real)[1] + 4
        return dict(d=d, n=70, first=0, kind="iso", sigma=0.3, shape=True, seed=0xAD18, target="iso_gauss")
    return PARITY[name]


def _scaled_cov(d):
    return np.diag(([0.04, 1.0, 9.0, 0.25, 2.25])[:d])


def parity_model_and_target(mhx, oracle, case):
    """(engine model, restatement target) of a parity case"""
    import user_targets
    d = case["d"]
    if case["target"] == "iso_gauss":
        return mhx.DensityModel(mhx.IsoGaussian(d)), oracle.iso_gauss(d)
    if case["target"] == "scaled_gauss":
        if d == 1:
            return mhx.DensityModel(mhx.IsoGaussian(1)), oracle.iso_gauss(1)
        return mhx.DensityModel(mhx.CorrGaussian(_scaled_cov(d))), oracle.corr_gauss_from_cov(_scaled_cov(d))
    if case["target"] == "user_shifted":
        data = [0.5, -1.0, 2.0, 0.2, 1.0, 3.0]
        return (mhx.DensityModel(mhx.HipLogDensity(user_targets.SHIFTED_GAUSS, d, data)),
                user_targets.host_target(oracle, user_targets.SHIFTED_GAUSS, d, data=data))
    return (mhx.DensityModel(mhx.HipLogDensity(user_targets.NIG_UNTRANSFORMED, 2)),
            user_targets.host_target(oracle, user_targets.NIG_UNTRANSFORMED, 2))


def parity_sigma(oracle, case):
    return case["sigma"] if case["kind"] == "iso" else np.asarray(case["sigma"], dtype=oracle.real())


def restated(mhx, oracle, name, real):
    """the restated chains of a parity case in the current width (computed once per session)"""
    key = (name, real)
    if key not in _restated:
        c = parity_case(name, real)
        _, target = parity_model_and_target(mhx, oracle, c)
        _restated[key] = A.run(target, oracle.PROP_ISO if c["kind"] == "iso" else oracle.PROP_DIAG, parity_sigma(oracle, c), SCHEDULE["N"],
                               c["seed"], c["first"], c["n"], SCHEDULE["adapt_steps"], shape=c["shape"],
                               discard_initial=SCHEDULE["discard"], thinning=SCHEDULE["thinning"])
    return _restated[key]


@pytest.mark.parametrize("name", sorted(PARITY))
def test_parity_inputs_exercise_accepts_rejects_and_the_adaptation(mhx, oracle, real, name):
    """a GPU parity test on these inputs cannot pass with accepts never or always taken, with lam or (shape) the sds left where they
    began; the bounded-support case rejects candidates outright (loga = -inf, p = 0)"""
    ref = restated(mhx, oracle, name, real)
    c = PARITY[name]
    nT = SCHEDULE["discard"] + (SCHEDULE["N"] - 1) * SCHEDULE["thinning"]
    total = int(ref["accept_counts"].sum())
    print(name, real, "accepted", total, "of", nT * c["n"], "at the seam", int(ref["acc_at_freeze"].sum()))
    assert 0 < total < nT * c["n"]
    assert 0 < int(ref["acc_at_freeze"].sum()) < total
    assert (ref["lam"] != 0).all() and len(np.unique(ref["lam"])) > c["n"] // 2
    s = np.asarray(parity_sigma(oracle, c), dtype=np.float64) * np.ones(c["d"])
    assert (ref["sd"] != s[:, None]).any()
    if c["shape"]:
        assert np.isfinite(ref["mean"]).all() and (ref["var"] > 0).all()
        assert (np.abs(ref["sd"] / np.exp(ref["lam"].astype(np.float64))[None, :] / s[:, None] - 1.0) > 1e-3).any()
    if c["target"] == "user_nig":
        # chains outside the support (lp = -inf: a candidate outside it too gives loga = NaN, p = 0) and chains inside it (a candidate
        # that leaves it gives loga = -inf, p = 0)
        lp0 = ref["samples"][0, c["d"], :]
        assert np.isneginf(lp0).any() and np.isfinite(lp0).any()


# ---- the tuning claim, on the restatement: what the device must reproduce bit for bit
TUNING = dict(sds=(0.1, 1.0, 10.0, 100.0), s=1.0, n=64, steps=1500, frozen=1000, seed=0xAD20)
_tuned = {}


def tuning_reference(oracle):
    """fp64: the 4-d Gaussian with sds (0.1, 1, 10, 100), s = 1, 64 chains, 1500 adapting transitions with shape, then 1000 frozen;
    the run's final state only (N = 1).  Computed once per session."""
    assert oracle.get_dtype() == "f64"
    if "ref" not in _tuned:
        t = TUNING
        target = oracle.corr_gauss_from_cov(np.diag(np.square(t["sds"])))
        _tuned["ref"] = A.run(target, oracle.PROP_ISO, t["s"], 1, t["seed"], 0, t["n"], t["steps"], shape=True,
                              discard_initial=t["steps"] + t["frozen"])
    return _tuned["ref"]


def check_tuning(lam, sd, acc_total, acc_at_freeze):
    """the windows of the claim: pooled frozen acceptance rate in [0.17, 0.30]; per coordinate the median over chains of
    sqrt(v_k) / true sd_k = sd_k / exp(lam) / true sd_k in [0.75, 1.25]"""
    t = TUNING
    rate = float((acc_total.astype(np.int64) - acc_at_freeze.astype(np.int64)).sum()) / (t["frozen"] * t["n"])
    ratios = [float(np.median(sd[k] / np.exp(lam) / t["sds"][k])) for k in range(4)]
    print("frozen acceptance rate %.4f, median sqrt(v) / true sd %s" % (rate, ["%.3f" % v for v in ratios]))
    assert 0.17 <= rate <= 0.30, rate
    for k, v in enumerate(ratios):
        assert 0.75 <= v <= 1.25, (k, v)
    return rate, ratios


class in_f64:
    """the engine's default dtype and the oracle's build in fp64 for the duration of a block (a test that runs in one width only)"""

    def __init__(self, mhx, oracle):
        self.m, self.O = mhx, oracle

    def __enter__(self):
        self.old = self.m.get_default_dtype(), self.O.get_dtype()
        self.m.set_default_dtype("f64")
        self.O.set_dtype("f64")

    def __exit__(self, *exc):
        self.m.set_default_dtype(self.old[0])
        self.O.set_dtype(self.old[1])


def test_tuning_claim_on_the_restatement(mhx, oracle):
    O = oracle
    with in_f64(mhx, O):
        ref = tuning_reference(O)
        lam, sd = ref["lam"].astype(np.float64), ref["sd"].astype(np.float64)
        # sqrt(v) directly, too: sd / exp(lam) is it up to two roundings
        direct = [float(np.median(np.sqrt(ref["var"][k].astype(np.float64)) / TUNING["sds"][k])) for k in range(4)]
        _, ratios = check_tuning(lam, sd, ref["accept_counts"], ref["acc_at_freeze"])
        assert np.allclose(direct, ratios, rtol=1e-12)
        # the same proposal left fixed: the oracle's plain chain over the same 2500 transitions
        t = TUNING
        target = O.corr_gauss_from_cov(np.diag(np.square(t["sds"])))
        fixed = O.rwmh(target, O.Proposal(O.PROP_ISO, scale=t["s"]), O.schedule(1, t["steps"] + t["frozen"], 1), t["seed"], 0, t["n"], save=False)
        fixed_rate = float(fixed["accept_counts"].sum()) / ((t["steps"] + t["frozen"]) * t["n"])
        print("fixed proposal: acceptance rate %.4f" % fixed_rate)
        assert fixed_rate < 0.15


# ---- the register forms at their limits
def _compile_reg(real, phase, d, perk, shape, tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the build needs it too"
    src = tmp_path / "adaptive.hip"
    src.write_text('#include "mhx_device_math.h"\n#include "mhx_rwmh_adaptive_kernels.h"\n')
    out = tmp_path / ("k_%s_%d_%d_%d.s" % (phase, d, perk, shape))
    cmd = [hipcc, "-x", "hip", "--offload-device-only", "--no-gpu-bundle-output", "-S", "-DMHX_JIT_BUILD=1", "-I" + CSRC,
           "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
           "-mllvm", "-pragma-unroll-threshold=4000000", "-mllvm", "-amdgpu-unroll-threshold-private=100000",
           "-DMHX_REAL64=%d" % (1 if real == "f64" else 0),
           "-DMHX_JIT_ADAPTIVE_REG=1" if phase == "adapting" else "-DMHX_JIT_ADAPTIVE_FROZEN_REG=1", "-DMHX_JIT_DIM=%d" % d, "-DMHX_JIT_TK=0",
           "-DMHX_JIT_PERK=%d" % perk, "-DMHX_JIT_SHAPE=%d" % shape, "-o", str(out), str(src)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-2000:]
    assert "not unrolled" not in done.stdout, done.stdout[-2000:]
    text = out.read_text()
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)]
    assert sizes
    return max(sizes)


# the next size tried above each limit (the header's comment): (adapting, adapting with shape, frozen)
NEXT_TRIED = {"f64": (64, 24, 56), "f32": (112, 40, 88)}


@pytest.mark.parametrize("which", ["adapting", "adapting with shape", "frozen"])
def test_register_forms_compile_without_scratch_at_their_limits_and_not_above(real, which, tmp_path):
    """each phase's specialised kernel at its limit, cross-compiled for gfx950 with the options of the run-time build: no scratch
    memory, with a row of eff per coordinate and with one; at the next size tried it spills"""
    i = ["adapting", "adapting with shape", "frozen"].index(which)
    d = register_limits(real)[i]
    api = open(os.path.join(CSRC, "mhx_api_adaptive.inc")).read()
    for name in ("d <= MHX_ADAPT_REG_MAX_DIM", "d <= MHX_ADAPT_SHAPE_REG_MAX_DIM", "d <= MHX_ADAPT_FROZEN_REG_MAX_DIM"):
        assert name in api
    phase, shape = ("frozen", 0) if which == "frozen" else ("adapting", 1 if which == "adapting with shape" else 0)
    for perk in ((1,) if shape else (1, 0)):
        scratch = _compile_reg(real, phase, d, perk, shape, tmp_path)
        assert scratch == 0, "%s, d = %d, perk %d [%s]: %d bytes of scratch" % (which, d, perk, real, scratch)
    nxt = NEXT_TRIED[real][i]
    assert nxt > d
    scratch = _compile_reg(real, phase, nxt, 1, shape, tmp_path)
    assert scratch > 0, "%s, d = %d [%s] compiles without scratch: the limit can move up" % (which, nxt, real)


# ---- declared, exported, bound, guarded
def test_entry_points_are_declared_exported_and_guarded(mhx):
    hdr = open(os.path.join(ROOT, "include", "mhx.h")).read()
    for name in ("mhx_rwmh_create_adaptive", "mhx_run_proposal_state"):
        assert name in mhx.EXPORTS and hasattr(mhx.lib(), name) and ("int %s(" % name) in hdr
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
        assert name not in open(os.path.join(ROOT, "advancedmh.jl_amd", "julia", "AdvancedMHHIP.jl")).read()       # left out on purpose
    assert not hasattr(mhx.Group, "proposal_state")                                   # left out on purpose
    assert hasattr(mhx.Run, "proposal_state")
    lib = C.CDLL(mhx.LIB_PATH)
    lib.mhx_last_error.restype = C.c_char_p
    assert lib.mhx_rwmh_create_adaptive(None, None, None, None, None) == mhx.MHX_EINVAL
    assert lib.mhx_last_error().decode() == "mhx_rwmh_create_adaptive: handle is NULL"
    assert lib.mhx_run_proposal_state(None, None, None, None, None) == mhx.MHX_EINVAL
    assert lib.mhx_last_error().decode() == "mhx_run_proposal_state: handle is NULL"
    import mhx._lib as L
    assert [f[0] for f in L.ProposalAdaptCfg._fields_] == ["adapt_steps", "shape", "target_rate", "c", "kappa", "lam_min", "lam_max"]
    assert re.search(r"int32_t adapt_steps;\s*int32_t shape;\s*double target_rate, c, kappa, lam_min, lam_max;\s*} mhx_proposal_adapt_cfg;", hdr)
    import importlib.util
    spec = importlib.util.spec_from_file_location("embed_headers", os.path.join(CSRC, "embed_headers.py"))
    eh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(eh)
    assert "mhx_rwmh_adaptive_kernels.h" in eh.HEADERS


def test_python_mirror_validates_and_defaults_without_a_device(mhx):
    a = mhx.ProposalAdaptation(100)
    assert (a.steps, a.target_rate, a.c, a.kappa, a.shape, a.lam_min, a.lam_max) == (100, 0.234, 1.0, 0.6, False, None, None)
    cfg = a.cfg()
    assert cfg.adapt_steps == 100 and cfg.shape == 0 and cfg.target_rate == 0.234 and cfg.c == 1.0 and cfg.kappa == 0.6
    assert math.isnan(cfg.lam_min) and math.isnan(cfg.lam_max)                          # NaN = the library's default (-20, 20)
    cfg = mhx.ProposalAdaptation(5, shape=True, lam_min=-3, lam_max=2, c=0.0).cfg()
    assert (cfg.shape, cfg.lam_min, cfg.lam_max, cfg.c) == (1, -3.0, 2.0, 0.0)
    for bad in (dict(steps=-1), dict(steps=1, kappa=0.5), dict(steps=1, kappa=1.01), dict(steps=1, c=-0.1), dict(steps=1, c=float("inf")),
                dict(steps=1, target_rate=0.0), dict(steps=1, target_rate=1.0), dict(steps=1, lam_min=1.0, lam_max=0.0)):
        with pytest.raises(mhx.ArgumentError):
            mhx.ProposalAdaptation(**bad)
    iso = mhx.MvNormal(mhx.zeros(2), 0.25 * mhx.I)
    assert mhx.RWMH(iso).adapt is None and mhx.MetropolisHastings(mhx.RandomWalkProposal(iso)).adapt is None
    assert mhx.RWMH(iso, adapt=a).adapt is a
    assert mhx.RWMH(mhx.MvNormal(mhx.zeros(2), np.array([1.0, 4.0])), adapt=a).adapt is a
    with pytest.raises(mhx.ArgumentError):
        mhx.RWMH(iso, adapt=mhx.LadderAdaptation(3))
    for refused in (lambda: mhx.RWMH(mhx.MvNormal(mhx.zeros(2), np.array([[1.0, 0.3], [0.3, 1.0]])), adapt=a),     # dense
                    lambda: mhx.RWMH(mhx.MvNormal([0.5, 0.0], mhx.I), adapt=a),                                   # a proposal mean
                    lambda: mhx.MetropolisHastings(mhx.StaticProposal(iso), adapt=a),                             # static
                    lambda: mhx.RWMH([mhx.Laplace(0, 1)], adapt=a),                                               # a family component
                    lambda: mhx.Tempered(mhx.RWMH(iso, adapt=a), [1.0, 0.5])):
        with pytest.raises(mhx.ArgumentError):
            refused()
    t = mhx.AdaptationTable([dict(parameter="mu", sd_median=0.5, sd_min=0.25, sd_max=1.0)])
    t.lam_median, t.accept_rate = -0.125, 0.231
    assert "mu" in str(t) and "0.231" in str(t) and "-0.1250" in str(t)
