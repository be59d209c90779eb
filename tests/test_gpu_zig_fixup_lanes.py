"""The fp64 ziggurat fix-up of the generator / consumer wave pairs with TWO lanes per failed candidate (csrc/mhx_device_math.h,
mhx_zig_refine2; csrc/mhx_rwmh_kernels.h, mhx_zig_fixup<L, FIX2>): one Philox call and one exponential per lane where
mhx_zig_refine runs two of each, windows of 32 queue entries where the one-lane form has 64.  Every value is made by the same function
on the same inputs, so the chains must stay the oracle's bit for bit, and equal to the ONE-lane form of the same build (the run-time twin of the tools
build with MHX_ZIG_FIX2=0).
Reference behaviour under test: src/mh-core.jl:76-117 (one transition), through the spec's ziggurat normals."""
import os
import re

import numpy as np
import pytest

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "advancedmh.jl_amd", "csrc")
D = 100
S = float(np.float32(0.238))
# chosen on the CPU with the oracle (test_the_seed_reaches_every_exit_of_the_refinement asserts it): the 8 x 130 x 100 normals of this
# run contain every exit of mhx_zig_refine
SEED, FIRST, NSAVE = 0x21F1B, 3, 9         # 9 saved states = 8 transitions
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


def _ref(oracle, d, C, n=NSAVE):
    """the oracle's chains, computed once per shape and shared (never modified)"""
    if (d, C, n) not in _REF:
        _REF[(d, C, n)] = oracle.rwmh(oracle.iso_gauss(d, reduce_lanes=2), oracle.Proposal(oracle.PROP_ISO, S, normal_gen=1),
                                      oracle.schedule(n), SEED, FIRST, C)
    return _REF[(d, C, n)]


def _device(mhx, d, C, n=NSAVE, **kw):
    model = mhx.DensityModel(mhx.IsoGaussian(d))
    spl = mhx.RWMH(mhx.MvNormal(mhx.zeros(d), S * S * mhx.I))
    chain = mhx.sample(model, spl, n, C, seed=SEED, first_chain=FIRST, reduce_lanes=2, normal_gen="ziggurat", **kw)
    return dict(samples=chain.value, accepted=chain.accepted, form=chain.state.form_name(), stats=chain.stats)


def _check(got, ref, what):
    _same(got["samples"], ref["samples"], what + ": samples")
    _same(got["accepted"], ref["accepted"], what + ": accepted")


# ---- the oracle's side: which exit of the refinement each failed candidate of the run takes -------------------------------------------
def _zig_table():
    text = open(os.path.join(CSRC, "mhx_zig_table.h")).read()
    body = text[text.index("#define MHX_ZIG_TABLE {"):]
    body = body[body.index("{") + 1:body.index("}")]
    x = np.array([float.fromhex(t) for t in re.findall(r"-?0x[0-9a-fA-F.]+p[-+]?\d+", body)])
    assert len(x) == 1025 and x[1024] == 0.0
    return x


def _candidate(x, hi, lo):
    """zig_try of the oracle: (signed candidate, layer, inside its rectangle)"""
    layer = lo & 1023
    k = (((lo >> 11) & 0xfffff) << 32) | hi
    ax = (k * 2.0 ** -52) * x[layer]                       # both products exact / rounded once, as in the oracle
    return (-ax if lo >> 31 else ax), layer, ax < x[layer + 1]


def classify_exits(oracle, seed, first, C, d, steps):
    """counts of {tail, wedge_accept, second_candidate, slow_at_2} over the normals n < d of chains first .. first + C - 1, steps 1 .. steps;
    every classified normal is checked against orc_zig_normal's value"""
    x = _zig_table()
    key = (seed & 0xffffffff, seed >> 32)
    out = dict(tail=0, wedge_accept=0, second_candidate=0, slow_at_2=0, failed=0)
    for step in range(1, steps + 1):
        for c in range(C):
            cid = first + c
            z = None
            for p in range((d + 1) // 2):
                w = oracle.philox((cid & 0xffffffff, cid >> 32, step, p), key)
                for h in range(2):
                    n = 2 * p + h
                    if n >= d:
                        continue
                    x0, layer, inside = _candidate(x, w[2 * h], w[2 * h + 1])
                    if inside:
                        continue
                    if z is None:
                        z = oracle.zig_normals(seed, cid, step, 0, d)
                    out["failed"] += 1
                    if layer == 0:
                        out["tail"] += 1
                        assert abs(z[n]) > x[1]
                        continue
                    v = oracle.philox((cid & 0xffffffff, cid >> 32, step, (4 << 28) | (n << 8) | 1), key)
                    x2, _, inside2 = _candidate(x, v[0], v[1])
                    if z[n] == x0:
                        out["wedge_accept"] += 1
                    elif inside2:
                        out["second_candidate"] += 1
                        assert z[n] == x2
                    else:
                        out["slow_at_2"] += 1
    return out


def test_the_seed_reaches_every_exit_of_the_refinement(oracle, f64):
    """the 8 x 130 x 100 normals of the runs below contain a layer-0 failure (the tail: mhx_zig_slow from attempt 1), a wedge that
    accepts, a wedge rejection settled by attempt 1's fresh candidate, and one whose fresh candidate left its rectangle too
    (mhx_zig_slow from attempt 2) -- so a passing parity run has gone through all exits of mhx_zig_refine2"""
    got = classify_exits(oracle, SEED, FIRST, 130, D, NSAVE - 1)
    print(got)
    assert got["tail"] >= 1 and got["wedge_accept"] >= 1 and got["second_candidate"] >= 1 and got["slow_at_2"] >= 1, got


# ---- the device ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", [128, 130])
def test_two_lane_pairs_and_the_one_wave_body_equal_the_oracle(mhx, oracle, f64, engine, C):
    """128 chains: one full block; 130: a second block whose lanes are mostly idle and shadow the last chain.  The pre-built pairs
    kernel (two lanes per failed candidate) and the one-wave body (one lane per failed candidate)."""
    ref = _ref(oracle, D, C)
    engine.set("COOP_PAIRS", "1")
    pairs = _device(mhx, D, C)
    assert pairs["form"] == "coop_pairs" and pairs["stats"]["kernel_variant"] == 3
    _check(pairs, ref, "pairs against the oracle")
    engine.set("COOP_PAIRS", "0")
    one = _device(mhx, D, C)
    assert one["form"] == "coop"
    _check(one, ref, "one-wave body against the oracle")


def _twin(mhx, tools_engine, d, C, fix2, force_fail=None, n=NSAVE):
    """the run-time twin of the pairs kernel from the tools build, with the fix-up's form chosen by a define"""
    tools_engine.set("NO_PREBUILT", "1")
    tools_engine.set("COOP_PAIRS", "1")
    tools_engine.set("JIT_DEFS", "MHX_ZIG_FIX2=%d" % fix2)
    if force_fail:
        tools_engine.set("ZIG_FORCE_FAIL", str(force_fail))
    got = _device(mhx, d, C, n=n, allow_tainted=True)
    assert got["form"] == "coop_jit_pairs" and got["stats"]["tainted"] == 1
    return got


@gpu
def test_two_lanes_equal_one_lane_of_the_same_build(mhx, oracle, f64, tools_engine):
    ref = _ref(oracle, D, 130)
    two = _twin(mhx, tools_engine, D, 130, 1)
    one = _twin(mhx, tools_engine, D, 130, 0)
    _check(two, ref, "two lanes against the oracle")
    _check(one, ref, "one lane against the oracle")
    _same(two["samples"], one["samples"], "two lanes against one lane")


@gpu
@pytest.mark.parametrize("every", [80, 40, 3])
def test_window_overflow(mhx, oracle, f64, tools_engine, every):
    """ZIG_FORCE_FAIL sends slot s of lane l through the queue when (s + l) % every == 0 although its candidate is inside its rectangle
    (the refinement returns the fast-path value for it).  Per wave-step of 52 x 64 slots, on top of the ~14 real failures:
    every = 80: 36 forced (more than one window of 32, less than 64), 40: 77 (more than 64: a third and fourth window of 32, a second
    of 64), 3: a third of all slots (dozens of windows).  The two-lane form's further windows must give what the one-lane form gives."""
    C, n = 70, 4
    ref = _ref(oracle, D, C, n)
    two = _twin(mhx, tools_engine, D, C, 1, every, n)
    one = _twin(mhx, tools_engine, D, C, 0, every, n)
    _check(two, ref, "two lanes against the oracle")
    _same(two["samples"], one["samples"], "two lanes against one lane")
    _same(two["accepted"], one["accepted"], "two lanes against one lane: accepted")


@gpu
@pytest.mark.parametrize("d,form", [(98, "coop_pairs"), (77, "coop_pairs"), (37, "coop")])
def test_other_shapes(mhx, oracle, f64, engine, d, form):
    """d = 98: 13 blocks per lane, the last block of lane 0 has two padding dimensions and lane 1's is padding altogether; d = 77: 10
    blocks per lane (the smallest pairs shape), three padding dimensions in lane 1: the two-lane fix-up against the oracle (equal to
    the one-lane form through the oracle: test_two_lanes_equal_one_lane_of_the_same_build compares the forms directly at d = 100).
    d = 37: 5 blocks per lane, padding in both lanes -- not a pairs shape: the one-wave body with the one-lane fix-up, NONE of the new
    code; it only pins that the shape the issue names still takes that body and stays the oracle's."""
    C = 70
    engine.set("COOP_PAIRS", "1")
    got = _device(mhx, d, C, n=5)
    assert got["form"] in (form, form.replace("coop", "coop_jit")), got["form"]
    _check(got, _ref(oracle, d, C, 5), "d = %d" % d)


# ---- no GPU needed ------------------------------------------------------------------------------------------------------------------
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_lds_bytes_of_the_launch_record(tmp_path):
    """The dynamic LDS of the cooperative ziggurat kernel (one-wave body and pairs alike: this change leaves it alone) for 4, 7 and 13
    blocks per lane in fp64, evaluated BY THE COMPILER from the macros of mhx_rwmh_kernels.h and from the very expression the launch
    record of mhx_api.hip is filled with.  Expected bytes, from the layout the header describes -- table (1024 + 1) x 8 rounded up to
    16 = 8 208; per wave KS x (NBL x 4 x 64 x 8 + 512) + 128 with KS the steps per fix-up group that fit (NBL = 4, two waves per SIMD:
    (81 920 - 8 208 - 512) / (4 x 8 736) = 2; NBL = 7: 1; NBL = 13, one wave per SIMD: 1); four waves per block:
        NBL = 4:  8 208 + 4 x (2 x 8 704 + 128) =  78 352
        NBL = 7:  8 208 + 4 x (14 848 + 128)    =  68 112
        NBL = 13: 8 208 + 4 x (27 136 + 128)    = 117 264   (the pairs' 512-thread block: one slab per pair, the same bytes)"""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the build needs it too"
    m = re.findall(r"size_t coop_lds = ([^;]+);", _src("mhx_api.hip"))
    assert len(m) == 1, "the cooperative kernel's launch record takes its LDS from one expression"
    expect = {4: (78352, 2), 7: (68112, 1), 13: (117264, 1)}
    lines = ['#include <hip/hip_runtime.h>', '#include "mhx_rwmh_kernels.h"',
             "template <int NBL> constexpr long record_lds() { constexpr bool zig = true; return (long)(%s); }" % m[0]]
    for nbl, (nbytes, ks) in expect.items():
        lines.append('static_assert(MHX_ZIG_LDS_BYTES(%d) == %d, "macro, NBL = %d");' % (nbl, nbytes, nbl))
        lines.append('static_assert(MHX_ZIG_KS(%d) == %d, "steps per fix-up group, NBL = %d");' % (nbl, ks, nbl))
        lines.append('static_assert(record_lds<%d>() == %d, "launch record, NBL = %d");' % (nbl, nbytes, nbl))
    lines.append('static_assert(MHX_ZIG_LDS_BYTES(13) <= 163840, "one block per CU");')
    src = tmp_path / "lds.hip"
    src.write_text("\n".join(lines) + "\n")
    done = subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-fsyntax-only", "-std=c++17", "-DMHX_REAL64=1", "-I" + CSRC, str(src)],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-3000:]
    # the pairs' record is the one-wave body's with a 512-thread block: nothing else of it is reassigned
    assert re.search(r"if \(r->coop_pairs\) r->step\.block = 512;", _src("mhx_api.hip"))


def test_the_release_library_embeds_the_new_text(tmp_path):
    """the run-time twin is compiled from the headers the library carries: the generated text is what embed_headers.py makes of the
    tree's headers now (`make` leaves no diff), and it holds the two-lane refinement"""
    import subprocess
    import sys
    out = tmp_path / "embed.inc"
    subprocess.run([sys.executable, os.path.join(CSRC, "embed_headers.py"), "--release", str(out)], check=True)
    text = out.read_text()
    assert "mhx_zig_refine2" in text and "MHX_ZIG_FIX2" in text and "MHX_TOOLS_BUILD" not in text
    built = os.path.join(CSRC, "mhx_jit_embed.inc")
    if os.path.exists(built):
        assert open(built).read() == text, "mhx_jit_embed.inc is stale: run make"
    lib = os.path.join(os.path.dirname(CSRC), "libmhx.so")
    if os.path.exists(lib):
        assert b"mhx_zig_refine2" in open(lib, "rb").read(), "libmhx.so carries the headers of another tree"
