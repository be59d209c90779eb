"""The generator wave of the fp64 generator / consumer wave pairs (csrc/mhx_rwmh_kernels.h, mhx_rwmh_coop_pairs_body): ONE Philox call
per lane-half in the last block where lane-half 1's own last block is padding altogether (MHX_GEN_SHARE_LAST: d <= 4 (2 (NBL - 1) + 1),
i.e. d = 73 .. 76 at 10 blocks per lane and 97 .. 100 at 13).  There lane-half 1 draws the second call of lane-half 0's block, stores
its pair into the owner's column of the slab and hands its two failure notes across the halves; the generator has one step loop for
these shapes and one for the others.  Every value is made by the same function on the same inputs: the chains must stay the oracle's
bit for bit -- samples, accept flags, final state, lp and accept counts -- and equal to the one-wave body (COOP_PAIRS = 0) of the same
build.
Reference behaviour under test: src/mh-core.jl:76-117 (one transition), through the spec's ziggurat normals."""
import numpy as np
import pytest

import cases
from test_gpu_zig_fixup_lanes import _candidate, _zig_table

S = float(np.float32(0.238))
SEED, FIRST = 0x9A1125, 3
SCHED = (3, 2, 3, 0)                       # 2 + 3 x 2 = 8 transitions, unsaved steps between the saved ones
# chosen on the CPU with the oracle (test_the_seed_fails_in_the_shared_block asserts it): among the 8 x 130 x 4 candidates of the shared
# block of this run (d = 100: n = 96 .. 99) enough leave their rectangles, in either lane-half's share
FIX_SEED, FIX_FIRST, FIX_C, FIX_NSAVE = 0x21F1B, 3, 130, 9
gpu = pytest.mark.gpu


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


_REF = {}


def _ref(oracle, d, C, sched=SCHED, seed=SEED, first=FIRST):
    """the oracle's chains with a record, computed once per shape and shared (never modified): a run without a record ends in the
    same state"""
    key = (d, C, sched, seed, first)
    if key not in _REF:
        _REF[key] = oracle.rwmh(oracle.iso_gauss(d, reduce_lanes=2), oracle.Proposal(oracle.PROP_ISO, S, normal_gen=1),
                                oracle.schedule(*sched), seed, first, C, save=True)
    return _REF[key]


def _device(mhx, d, C, sched=SCHED, save=True, seed=SEED, first=FIRST):
    """one call on a fresh run of the default context (whose options the caller has set)"""
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(d), S * S * mhx.I))
    run = mhx.Run(model, spl, nchains=C, seed=seed, first_chain=first, reduce_lanes=2, normal_gen="ziggurat")
    run.init(None)
    run.sample(*sched, save=save)
    out = dict(form=run.form_name(), stats=run.stats())
    if save:
        out["samples"], out["accepted"] = run.samples()
    out["x"], out["lp"], out["cnt"] = run.state()
    run.close()
    return out


KEYS = ("samples", "accepted", "x", "lp", "cnt")


def _check(got, ref, save, what):
    if save:
        _same(got["samples"], ref["samples"], what + ": samples")
        _same(got["accepted"], ref["accepted"], what + ": accepted")
    _same(got["x"], ref["final_x"], what + ": final x")
    _same(got["lp"], ref["final_lp"], what + ": final lp")
    _same(got["cnt"], ref["accept_counts"], what + ": accept counts")
    assert got["stats"]["accepted"] == int(ref["accept_counts"].astype(np.uint64).sum()), what + ": stats accepted"


def _equal(a, b, save, what):
    for k in KEYS if save else KEYS[2:]:
        _same(a[k], b[k], what + ": " + k)
    assert a["stats"]["accepted"] == b["stats"]["accepted"], what


# ---- the oracle's side: the failed candidates of the shared block ---------------------------------------------------------------------
def shared_block_failures(oracle, seed, first, C, d, steps):
    """{n: failed candidates} over the normals n of block (d - 1) // 4 of chains first .. first + C - 1, steps 1 .. steps (the way of
    classify_exits in test_gpu_zig_fixup_lanes.py: the candidate from its Philox words and the layer table)"""
    x = _zig_table()
    key = (seed & 0xffffffff, seed >> 32)
    b = (d - 1) // 4
    out = {n: 0 for n in range(4 * b, 4 * b + 4)}
    for step in range(1, steps + 1):
        for c in range(C):
            cid = first + c
            for h2 in range(2):
                w = oracle.philox((cid & 0xffffffff, cid >> 32, step, 2 * b + h2), key)
                for h in range(2):
                    n = 4 * b + 2 * h2 + h
                    if n < d and not _candidate(x, w[2 * h], w[2 * h + 1])[2]:
                        out[n] += 1
    return out


def test_the_seed_fails_in_the_shared_block(oracle, f64):
    """d = 100, 130 chains, 8 transitions: at least 8 failed candidates among n = 98, 99 (drawn by lane-half 1 for the owner: their
    failure notes cross the halves, the fix-up repairs them in the owner's column) and at least 4 among n = 96, 97 (lane-half 0's
    call) -- so the parity run below cannot pass with a shared block that never reaches the fix-up"""
    got = shared_block_failures(oracle, FIX_SEED, FIX_FIRST, FIX_C, 100, FIX_NSAVE - 1)
    print(got)
    assert got[98] + got[99] >= 8 and got[96] + got[97] >= 4, got


# ---- the device ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("save", [True, False], ids=["record", "no_record"])
@pytest.mark.parametrize("C", [33, 160])
@pytest.mark.parametrize("d", [73, 74, 76, 77, 97, 98, 100, 101, 104])
def test_pairs_equal_the_oracle_and_the_one_wave_body(mhx, oracle, f64, engine, d, C, save):
    """d = 73 .. 76 (10 blocks per lane) and 97 .. 100 (13) take the shared last block: 73 and 97 leave one live dimension in it, 74
    and 98 make the second call pure padding; 77, 101 and 104 have live dimensions in lane-half 1's last block and keep two calls per
    lane.  33 chains: a partial wave; 160: a partial second block."""
    ref = _ref(oracle, d, C)
    engine.set("COOP_PAIRS", "1")
    pairs = _device(mhx, d, C, save=save)
    assert pairs["form"] in ("coop_pairs", "coop_jit_pairs") and pairs["stats"]["reduce_lanes"] == 2, pairs["form"]
    assert pairs["stats"]["normal_gen"] == 1 and pairs["stats"]["dtype"] == "f64"
    _check(pairs, ref, save, "pairs against the oracle")
    engine.set("COOP_PAIRS", "0")
    one = _device(mhx, d, C, save=save)
    assert one["form"] in ("coop", "coop_jit"), one["form"]
    _check(one, ref, save, "one-wave body against the oracle")
    _equal(pairs, one, save, "pairs against the one-wave body")


@gpu
def test_failures_of_the_shared_block_are_repaired(mhx, oracle, f64, engine):
    """the run whose shared block test_the_seed_fails_in_the_shared_block counts"""
    sched = (FIX_NSAVE, 0, 1, 0)
    ref = _ref(oracle, 100, FIX_C, sched, FIX_SEED, FIX_FIRST)
    engine.set("COOP_PAIRS", "1")
    pairs = _device(mhx, 100, FIX_C, sched, True, FIX_SEED, FIX_FIRST)
    assert pairs["form"] == "coop_pairs"
    _check(pairs, ref, True, "pairs against the oracle")
    engine.set("COOP_PAIRS", "0")
    one = _device(mhx, 100, FIX_C, sched, True, FIX_SEED, FIX_FIRST)
    assert one["form"] == "coop"
    _equal(pairs, one, True, "pairs against the one-wave body")


def _twin(mhx, tools_engine, d, C, defs, force_fail):
    """the run-time twin of the pairs kernel from the tools build, the generator's form chosen by defines"""
    tools_engine.set("NO_PREBUILT", "1")
    tools_engine.set("COOP_PAIRS", "1")
    tools_engine.set("JIT_DEFS", defs)
    tools_engine.set("ZIG_FORCE_FAIL", str(force_fail))
    got = _device(mhx, d, C)
    assert got["form"] == "coop_jit_pairs" and got["stats"]["tainted"] == 1
    return got


@gpu
@pytest.mark.parametrize("d", [100, 74])
@pytest.mark.parametrize("every", [3, 40])
def test_forced_failures_in_the_shared_block(mhx, oracle, f64, tools_engine, d, every):
    """ZIG_FORCE_FAIL sends slot s of owner lane o through the fix-up when (s + o) % every == 0 although its candidate is inside its
    rectangle (the refinement returns the fast-path value for it).  every = 3: in every lane of the shared block one or two of the
    four slots, noted by either lane-half; 40: the second call's slots of three owners only (their notes cross the halves) beside
    the queue's further windows.  The shared form must give what the two-calls-per-lane form of the same build gives, and the oracle's chains."""
    C = 70
    ref = _ref(oracle, d, C)
    shared = _twin(mhx, tools_engine, d, C, "MHX_GEN_SHARE_LAST=1", every)
    parent = _twin(mhx, tools_engine, d, C, "MHX_GEN_SHARE_LAST=0", every)
    _check(shared, ref, True, "shared last block against the oracle")
    _check(parent, ref, True, "two calls per lane against the oracle")
    _equal(shared, parent, True, "shared last block against two calls per lane")
