"""GPU parity of the cooperative RWMH kernel as generator / consumer wave pairs (option COOP_PAIRS = 1; csrc/mhx_rwmh_kernels.h,
mhx_rwmh_coop_pairs_body): fp64, d = 100, two lanes per chain, the ziggurat generator -- the shape of the headline, where the
one-wave body runs one wave per SIMD.  A block of 512 threads splits the step by role (waves 0-3 generate the normals of the next step,
waves 4-7 consume the current one) and hands the slab over through block-wide barriers only; the chains must be the one-wave body's
and the oracle's bit for bit: samples, accept flags, final state, lp and accept counts.
Reference behaviour under test: src/mh-core.jl:76-117 (one transition), through the spec's ziggurat normals."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

D = 100
S = float(np.float32(0.238))
SEED, FIRST = 0x9A1125, 3


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    bad = np.argwhere(cases.bits(a) != cases.bits(b))
    assert len(bad) == 0, "%s: %d mismatches, first at %s: %r vs %r" % (what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


@pytest.fixture
def f64(mhx, oracle):
    old_m, old_o = mhx.get_default_dtype(), oracle.get_dtype()
    mhx.set_default_dtype("f64")
    oracle.set_dtype("f64")
    yield
    mhx.set_default_dtype(old_m)
    oracle.set_dtype(old_o)


def _device(mhx, d, C, sched, save, lanes=2):
    """one call on a fresh run of the default context (whose COOP_PAIRS option the caller has set)"""
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(d), S * S * mhx.I))
    run = mhx.Run(model, spl, nchains=C, seed=SEED, first_chain=FIRST, reduce_lanes=lanes, normal_gen="ziggurat")
    run.init(None)
    run.sample(*sched, save=save)
    out = dict(form=run.form_name(), stats=run.stats())
    if save:
        out["samples"], out["accepted"] = run.samples()
    out["x"], out["lp"], out["cnt"] = run.state()
    run.close()
    return out


def _check(got, ref, save, what):
    if save:
        _same(got["samples"], ref["samples"], what + ": samples")
        _same(got["accepted"], ref["accepted"], what + ": accepted")
    _same(got["x"], ref["final_x"], what + ": final x")
    _same(got["lp"], ref["final_lp"], what + ": final lp")
    _same(got["cnt"], ref["accept_counts"], what + ": accept counts")
    assert got["stats"]["accepted"] == int(ref["accept_counts"].astype(np.uint64).sum()), what + ": stats accepted"


@pytest.mark.parametrize("save", [True, False], ids=["thinned_record", "no_record"])
@pytest.mark.parametrize("N", [1, 2, 7])
@pytest.mark.parametrize("C", [32, 33, 128, 160])
def test_pairs_equal_the_oracle_and_the_one_wave_body(mhx, oracle, f64, engine, C, N, save):
    """32 chains: one pair alive, three idle pairs that must keep the barrier count; 33: a partial wave; 128: one full block; 160: a
    partial second block.  schedule(N, 2, 3): unsaved steps between the saved ones, 2 + 3 (N - 1) transitions."""
    sched = (N, 2, 3, 0)
    ref = oracle.rwmh(oracle.iso_gauss(D, reduce_lanes=2), oracle.Proposal(oracle.PROP_ISO, S, normal_gen=1), oracle.schedule(*sched),
                      SEED, FIRST, C, save=save)
    engine.set("COOP_PAIRS", "1")
    pairs = _device(mhx, D, C, sched, save)
    assert pairs["form"] == "coop_pairs" and pairs["stats"]["kernel_variant"] == 3 and pairs["stats"]["reduce_lanes"] == 2
    assert pairs["stats"]["normal_gen"] == 1 and pairs["stats"]["dtype"] == "f64"
    _check(pairs, ref, save, "pairs against the oracle")
    engine.set("COOP_PAIRS", "0")
    one = _device(mhx, D, C, sched, save)
    assert one["form"] == "coop" and one["stats"]["kernel_variant"] == 3
    _check(one, ref, save, "one-wave body against the oracle")
    for k in (("samples", "accepted") if save else ()) + ("x", "lp", "cnt"):
        _same(pairs[k], one[k], "pairs against the one-wave body: " + k)
    assert pairs["stats"]["accepted"] == one["stats"]["accepted"]


def test_two_calls_on_one_run_hand_the_state_back(mhx, oracle, f64, engine):
    """Two consecutive sample calls: the consumer waves write state, lp, counts and the last accept flag back, the next call starts
    from them; and the host keeps the acceptance total of the previous call instead of reading it again -- stats()["accepted"] of
    each call is the oracle's count over that call's transitions."""
    C, N1, N2 = 160, 6, 5
    engine.set("COOP_PAIRS", "1")
    model = mhx.DensityModel(mhx.IsoGaussian(D))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(D), S * S * mhx.I))
    run = mhx.Run(model, spl, nchains=C, seed=SEED, first_chain=FIRST, reduce_lanes=2, normal_gen="ziggurat")
    assert run.form_name() == "coop_pairs"
    run.init(None)
    run.sample(N1)
    first, acc1 = run.samples()
    st1 = run.stats()
    run.sample(N2)
    second, acc2 = run.samples()
    st2 = run.stats()
    x, lp, cnt = run.state()
    run.close()
    ref = oracle.rwmh(oracle.iso_gauss(D, reduce_lanes=2), oracle.Proposal(oracle.PROP_ISO, S, normal_gen=1),
                      oracle.schedule(N1 + N2 - 1), SEED, FIRST, C)
    _same(first, ref["samples"][:N1], "first call")
    _same(acc1[1:], ref["accepted"][1:N1], "first call: accepted")
    _same(second, ref["samples"][N1 - 1:], "second call (slot 0 = the state the first call ended in)")
    _same(acc2, ref["accepted"][N1 - 1:], "second call: accepted (slot 0 = the flag of the first call's last transition)")
    _same(x, ref["final_x"], "final x")
    _same(lp, ref["final_lp"], "final lp")
    _same(cnt, ref["accept_counts"], "accept counts")
    assert st1["transitions"] == (N1 - 1) * C and st2["transitions"] == (N2 - 1) * C
    assert st1["accepted"] == int(ref["accepted"][1:N1].sum()), "first call: stats accepted"
    assert st2["accepted"] == int(ref["accepted"][N1:].sum()), "second call: stats accepted (previous total kept on the host)"


def test_fixup_queue_windows_inside_a_generator_wave(mhx, oracle, f64, tools_engine):
    """ZIG_FORCE_FAIL of the tools build (as in test_gpu_ziggurat.test_fixup_queue_windows) sends every third slot through the
    fix-up queue: several 64-entry windows per wave-step, all inside a generator wave; the refinement re-derives the same normals,
    so the chains stay the oracle's.  The run-time compiled twin of the pairs kernel (NO_PREBUILT)."""
    tools_engine.set("ZIG_FORCE_FAIL", "3")
    tools_engine.set("NO_PREBUILT", "1")
    tools_engine.set("COOP_PAIRS", "1")
    C, N = 70, 9
    model = mhx.DensityModel(mhx.IsoGaussian(D))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(D), S * S * mhx.I))
    chain = mhx.sample(model, spl, N, C, seed=SEED, first_chain=FIRST, reduce_lanes=2, normal_gen="ziggurat", allow_tainted=True)
    assert chain.stats["kernel_variant"] == 4 and chain.stats["tainted"] == 1 and chain.state.form_name() == "coop_jit_pairs"
    ref = oracle.rwmh(oracle.iso_gauss(D, reduce_lanes=2), oracle.Proposal(oracle.PROP_ISO, S, normal_gen=1), oracle.schedule(N),
                      SEED, FIRST, C)
    _same(chain.value, ref["samples"], "samples")
    _same(chain.accepted, ref["accepted"], "accepted")


def test_a_shape_at_two_waves_per_simd_keeps_the_one_wave_body(mhx, oracle, f64, engine):
    """d = 52 with two lanes per chain: 7 blocks per lane, two waves per SIMD already -- COOP_PAIRS = 1 does not apply."""
    engine.set("COOP_PAIRS", "1")
    d, C, sched = 52, 96, (4, 0, 1, 0)
    got = _device(mhx, d, C, sched, True)
    assert got["form"] in ("coop", "coop_jit") and got["stats"]["kernel_variant"] in (3, 4) and got["stats"]["reduce_lanes"] == 2
    ref = oracle.rwmh(oracle.iso_gauss(d, reduce_lanes=2), oracle.Proposal(oracle.PROP_ISO, S, normal_gen=1), oracle.schedule(*sched),
                      SEED, FIRST, C)
    _check(got, ref, True, "d = 52")
