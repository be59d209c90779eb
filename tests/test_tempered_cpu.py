"""CPU (no GPU): the restatement of the parallel-tempering arithmetic (tests/tempered_restatement.py) pinned to
the oracle, its detailed balance where a sign error shows, the inputs of the GPU parity cases (tests/test_gpu_tempered.py shares
them and their restated chains), the register form's dimension limit, and the guards of the new entry points."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases
import tempered_restatement as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "advancedmh.jl_amd", "csrc")


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    assert a.dtype == b.dtype, "%s: dtypes %s / %s" % (what, a.dtype, b.dtype)
    bad = np.argwhere(cases.bits(a) != cases.bits(b))
    assert len(bad) == 0, "%s: %d mismatches, first at %s: %r vs %r" % (what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


# ---- the restatement is the oracle's plain chain where the ladder does nothing
@pytest.mark.parametrize("d", [1, 5])
@pytest.mark.parametrize("kind", ["iso", "diag"])
def test_restatement_with_unit_betas_and_no_swaps_is_the_oracles_rwmh(oracle, real, kind, d):
    O = oracle
    Cn, N, seed, first = 6, 14, 0x7E3 + d, 4
    vec = np.linspace(0.4, 1.1, d).astype(O.real())
    prop = O.Proposal(O.PROP_ISO, 0.7) if kind == "iso" else O.Proposal(O.PROP_DIAG, vec=vec)
    for sched, init in ((O.schedule(N), None), (O.schedule(N, 3, 2), np.random.default_rng(2).normal(size=(d, Cn)).astype(O.real()))):
        ref = O.rwmh(O.iso_gauss(d), prop, sched, seed, first, Cn, init=init)
        got = P.run(O.iso_gauss(d), O.PROP_ISO if kind == "iso" else O.PROP_DIAG, 0.7 if kind == "iso" else vec, [1.0, 1.0], N, seed, first,
                    Cn, swap_every=0, scales=[1.0, 1.0], discard_initial=sched.discard_initial, thinning=sched.thinning, init=init)
        for k in ("samples", "accepted", "final_x", "final_lp", "accept_counts"):
            _same(got[k], ref[k], k)
        assert 0 < int(ref["accept_counts"].sum()) < Cn * (sched.discard_initial + (N - 1) * sched.thinning)
        assert got["swap_attempts"].sum() == 0 and got["swap_counts"].sum() == 0


# ---- detailed balance: the cold rung samples N(0, 1), the hot rung N(0, 1 / beta); a swap ratio of the wrong sign does not
def _pooled_variances(oracle, swap_sign):
    O = oracle
    nl, burn, N = 256, 40, 160
    res = P.run(O.iso_gauss(1), O.PROP_ISO, 2.4, [1.0, 0.25], N, 0xDB, 0, 2 * nl, swap_every=1, discard_initial=burn, swap_sign=swap_sign)
    x = res["samples"][:, 0, :].astype(np.float64)
    out = []
    for rung in (0, 1):
        per_ladder = (x[:, rung::2] ** 2).mean(axis=0)             # E x^2 about the known mean 0: unbiased for a stationary chain
        out.append((per_ladder.mean(), per_ladder.std(ddof=1) / np.sqrt(nl)))
    return out, res


def test_detailed_balance_of_the_swap_and_that_a_flipped_sign_fails_it(oracle):
    oracle.set_dtype("f64")
    (cold, hot), res = _pooled_variances(oracle, +1)
    print("cold %.4f +- %.4f, hot %.4f +- %.4f, swaps %d of %d" % (cold + hot + (res["swap_counts"].sum(), res["swap_attempts"].sum())))
    assert abs(cold[0] - 1.0) < 5 * cold[1] and abs(hot[0] - 4.0) < 5 * hot[1]
    assert 0 < res["swap_counts"].sum() < res["swap_attempts"].sum()
    (coldf, hotf), _ = _pooled_variances(oracle, -1)
    print("flipped: cold %.4f +- %.4f, hot %.4f +- %.4f" % (coldf + hotf))
    assert not (abs(coldf[0] - 1.0) < 5 * coldf[1] and abs(hotf[0] - 4.0) < 5 * hotf[1])


# ---- the GPU parity cases: inputs here, chains restated once per width and shared with tests/test_gpu_tempered.py
def bimodal(x):
    """an equal mixture of N((+2.5, +2.5), I) and N((-2.5, -2.5), I), up to its constant"""
    import mhx.trace as T
    a = -0.5 * ((x[0] - 2.5) * (x[0] - 2.5) + (x[1] - 2.5) * (x[1] - 2.5))
    b = -0.5 * ((x[0] + 2.5) * (x[0] + 2.5) + (x[1] + 2.5) * (x[1] + 2.5))
    m = T.maximum(a, b)
    return m + T.log(T.exp(a - m) + T.exp(b - m))


def _geometric(R, ratio):
    return [ratio ** r for r in range(R)]


# name -> dict(R, nladders, d, swap_every, discard, thinning, N, kind, sigma, betas, scales, seed, first, target)
PARITY = {
    "r4_partial_wave_iso": dict(R=4, nladders=19, d=5, swap_every=3, discard=3, thinning=2, N=20, kind="iso", sigma=0.9,
                                betas=_geometric(4, 0.45), scales=None, seed=0x7E01, first=8, target="iso_gauss"),
    "r64_every_row_boundary": dict(R=64, nladders=2, d=1, swap_every=1, discard=0, thinning=1, N=48, kind="iso", sigma=1.5,
                                   betas=_geometric(64, 0.55), scales=None, seed=0x7E02, first=0, target="iso_gauss"),
    "r2_diag": dict(R=2, nladders=33, d=3, swap_every=1, discard=0, thinning=1, N=12, kind="diag", sigma=[0.8, 1.3, 0.5],
                    betas=[1.0, 0.3], scales=None, seed=0x7E03, first=2, target="iso_gauss"),
    "r8_bimodal_user_scales": dict(R=8, nladders=8, d=2, swap_every=2, discard=0, thinning=1, N=40, kind="iso", sigma=1.0,
                                   betas=_geometric(8, 0.5), scales=[1.0, 1.25, 1.5, 2.0, 2.5, 3.0, 4.0, 5.5], seed=0x7E04, first=16,
                                   target="bimodal"),
}
_restated = {}


def parity_model_and_target(mhx, oracle, case):
    """(engine model, restatement target) of a parity case"""
    import user_targets
    if case["target"] == "iso_gauss":
        return mhx.DensityModel(mhx.IsoGaussian(case["d"])), oracle.iso_gauss(case["d"])
    model = mhx.DensityModel(bimodal, dim=2)
    return model, user_targets.host_target(oracle, model.traced.source, 2, data=model.traced.data)


def parity_sigma(oracle, case):
    return case["sigma"] if case["kind"] == "iso" else np.asarray(case["sigma"], dtype=oracle.real())


def restated(mhx, oracle, name, real):
    """the restated chains of a parity case in the current width (computed once per session)"""
    key = (name, real)
    if key not in _restated:
        c = PARITY[name]
        _, target = parity_model_and_target(mhx, oracle, c)
        _restated[key] = P.run(target, oracle.PROP_ISO if c["kind"] == "iso" else oracle.PROP_DIAG, parity_sigma(oracle, c), c["betas"],
                               c["N"], c["seed"], c["first"], c["R"] * c["nladders"], swap_every=c["swap_every"], scales=c["scales"],
                               discard_initial=c["discard"], thinning=c["thinning"])
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


# ---- the register form at its limit
def _compile_reg(real, d, pk, R, tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the build needs it too"
    src = tmp_path / "tempered.hip"
    src.write_text('#include "mhx_device_math.h"\n#include "mhx_rwmh_tempered_kernels.h"\n')
    out = tmp_path / ("k_%d_%d.s" % (d, pk))
    cmd = [hipcc, "-x", "hip", "--offload-device-only", "--no-gpu-bundle-output", "-S", "-DMHX_JIT_BUILD=1", "-I" + CSRC,
           "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
           "-mllvm", "-pragma-unroll-threshold=4000000", "-mllvm", "-amdgpu-unroll-threshold-private=100000",
           "-DMHX_REAL64=%d" % (1 if real == "f64" else 0), "-DMHX_JIT_TEMPERED_REG=1", "-DMHX_JIT_DIM=%d" % d, "-DMHX_JIT_TK=0",
           "-DMHX_JIT_PK=%d" % pk, "-DMHX_JIT_R=%d" % R, "-o", str(out), str(src)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-2000:]
    assert "not unrolled" not in done.stdout, done.stdout[-2000:]
    text = out.read_text()
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)]
    assert sizes
    return max(sizes), text


def test_register_form_compiles_without_scratch_at_its_dimension_limit_and_not_above(real, tmp_path):
    """the specialised kernel at d = MHX_TEMPERED_REG_MAX_DIM, cross-compiled for gfx950 with the options of the run-time build: no
    scratch memory, ISO and DIAG, with the exchange instructions in it; at the next size tried (the header's comment) DIAG spills"""
    hdr = open(os.path.join(CSRC, "mhx_rwmh_tempered_kernels.h")).read()
    m = re.search(r"#define\s+MHX_TEMPERED_REG_MAX_DIM\s+\(MHX_REAL64 \? (\d+) : (\d+)\)", hdr)
    assert m, "MHX_TEMPERED_REG_MAX_DIM not found"
    d = int(m.group(1) if real == "f64" else m.group(2))
    assert "d <= MHX_TEMPERED_REG_MAX_DIM" in open(os.path.join(CSRC, "mhx_api_tempered.inc")).read()
    for pk in (0, 1):
        scratch, text = _compile_reg(real, d, pk, 64, tmp_path)
        assert scratch == 0, "d = %d, proposal kind %d [%s]: %d bytes of scratch" % (d, pk, real, scratch)
        words = 2 if real == "f64" else 1
        # the exchange: a DPP move (even rounds) and a ds_bpermute (odd rounds) per 32-bit word of x[0..d) and of lp
        assert len(re.findall(r"v_mov_b32_dpp .*quad_perm:\[1,0,3,2\]", text)) >= words * (d + 1)
        assert len(re.findall(r"ds_bpermute_b32", text)) >= words * (d + 1)
    nxt = {"f64": 56, "f32": 88}[real]
    scratch, _ = _compile_reg(real, nxt, 1, 64, tmp_path)
    assert scratch > 0, "d = %d [%s] compiles without scratch: the limit can move up" % (nxt, real)


# ---- declared, exported, bound, guarded
def test_entry_points_are_declared_exported_and_guarded(mhx):
    hdr = open(os.path.join(ROOT, "include", "mhx.h")).read()
    names = ("mhx_rwmh_create_tempered", "mhx_run_swap_stats", "mhx_run_rung")
    for name in names:
        assert name in mhx.EXPORTS and hasattr(mhx.lib(), name) and ("int %s(" % name) in hdr
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
        assert name not in open(os.path.join(ROOT, "advancedmh.jl_amd", "julia", "AdvancedMHHIP.jl")).read()
    assert not hasattr(mhx.Group, "swap_rates")                                   # left out on purpose
    for name in ("swap_stats", "swap_rates", "rung", "accept_rates"):
        assert hasattr(mhx.Run, name)
    lib = C.CDLL(mhx.LIB_PATH)
    lib.mhx_last_error.restype = C.c_char_p
    assert lib.mhx_rwmh_create_tempered(None, None, None, None, None) == mhx.MHX_EINVAL
    assert lib.mhx_last_error().decode() == "mhx_rwmh_create_tempered: handle is NULL"
    assert lib.mhx_run_swap_stats(None, None, None) == mhx.MHX_EINVAL and lib.mhx_last_error().decode() == "mhx_run_swap_stats: handle is NULL"
    assert lib.mhx_run_rung(None, C.c_int32(0), None) == mhx.MHX_EINVAL and lib.mhx_last_error().decode() == "mhx_run_rung: handle is NULL"
    import importlib.util
    spec = importlib.util.spec_from_file_location("embed_headers", os.path.join(CSRC, "embed_headers.py"))
    eh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(eh)
    assert "mhx_rwmh_tempered_kernels.h" in eh.HEADERS
    # the stream tag of the swap uniforms is no other stream's: 0 .. 3, their retry twins | 4, the family streams 8 .. 10 and 12 .. 14
    math_h = open(os.path.join(CSRC, "mhx_device_math.h")).read()
    tags = {int(v) for v in re.findall(r"#define MHX_STREAM_(?:PROPOSAL|ACCEPT|INIT|EMCEE)\s+(\d+)u", math_h)}
    assert tags == {0, 1, 2, 3}
    fam = {int(v) for v in re.findall(r"#define MHX_STREAM_FAMILY(?:_INIT)?\s+(\d+)u", math_h)}
    used = tags | {t | 4 for t in tags} | {f + k for f in fam for k in range(3)}
    swap = int(re.search(r"#define MHX_STREAM_SWAP (\d+)u", open(os.path.join(CSRC, "mhx_rwmh_tempered_kernels.h")).read()).group(1))
    assert swap == P.STREAM_SWAP and swap < 16 and swap not in used


def test_python_mirror_checks_what_it_can_without_a_device(mhx):
    b = mhx.geometric_betas(8, 0.01)
    assert b[0] == 1.0 and b[-1] == 0.01 and (np.diff(b) < 0).all() and np.allclose(b[1:] / b[:-1], 0.01 ** (1 / 7))
    with pytest.raises(mhx.ArgumentError):
        mhx.geometric_betas(1, 0.5)
    with pytest.raises(mhx.ArgumentError):
        mhx.Tempered(mhx.StaticMH(mhx.MvNormal(mhx.zeros(2), mhx.I)), b)
    with pytest.raises(mhx.ArgumentError):
        mhx.Tempered(mhx.RWMH([mhx.Laplace(0, 1)]), b)
    t = mhx.Tempered(mhx.RWMH(mhx.MvNormal(mhx.zeros(2), mhx.I)), b, swap_every=3)
    assert t.R == 8 and t.swap_every == 3 and t.scales is None
    table = mhx.SwapTable([dict(pair=(0, 1), beta_lo=1.0, beta_hi=0.5, attempts=10, swaps=4, rate=0.4)])
    assert "0-1" in str(table) and "0.400" in str(table)
