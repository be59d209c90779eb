"""The production loop of the radix select (mhx_select_hist_body, csrc/mhx_diag_kernels.h): whole block sweeps of UNROLL loads per
thread, then the rest of the chunk one element at a time.  A block enters the unrolled loop only when its chunk holds at least
512 * UNROLL draws, and the host gives a parameter up to ceil(2048 / parameters) blocks -- so a small tensor asked for a few
parameters never gets there.  Here 100 parameter slots (repeated rows) share 21 blocks each and every chunk holds several
sweeps and a partial one: the running offset (src += step, the carry of c past C into the next draw) and the hand-over into
the tail loop run in both widths.  Exact comparison with numpy's sort, as in test_gpu_quantiles.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "advancedmh.jl_amd", "csrc", "mhx_diag_kernels.h")
SLOTS = 100


def _loop_constants(real):
    src = open(HEADER).read()
    threads = int(re.search(r"#define MHX_SELECT_THREADS (\d+)", src).group(1))
    u64, u32 = (int(u) for u in re.findall(r"#define MHX_SELECT_UNROLL (\d+)", src))     # the fp64 branch comes first
    return threads, u64 if real == "f64" else u32


def _chunks(S, P, threads, unroll):
    """the host's chunking rule (select_hist_pass, csrc/mhx_api_diag.inc): [(sweeps, tail elements)] of every block"""
    sweep = threads * unroll
    nblk = max(min(-(-2048 // P), -(-S // sweep)), 1, -(-S // 2 ** 31))
    chunk = -(-S // nblk)
    out = []
    for b in range(nblk):
        n = min(chunk, S - b * chunk)
        if n > 0:
            out.append((n // sweep, n % sweep))
    return out


# C above the block width and no multiple or divisor of it; C below it (several draws per block row); the single chain
@pytest.mark.parametrize("N,Cn", [(100, 2051), (3001, 67), (200003, 1)])
def test_unrolled_sweeps_and_their_tail(mhx, real, N, Cn):
    import torch
    threads, unroll = _loop_constants(real)
    S = N * Cn
    blocks = _chunks(S, SLOTS, threads, unroll)
    # what this test is for: every block runs whole sweeps AND hands a partial sweep over to the tail loop; the last block's
    # chunk is shorter than the others'
    assert len(blocks) > 1 and all(s >= 2 and t > 0 for s, t in blocks), blocks
    assert blocks[-1] != blocks[0]
    assert Cn == 1 or (threads % Cn != 0 and Cn % threads != 0)

    dt = mhx._lib.NP_DTYPES[real]
    rng = np.random.default_rng(N + Cn)
    host = np.full((N, 4, Cn), np.nan, dtype=dt)             # rows 1 and 3 stay NaN: a walk that strays off its row meets them
    host[:, 0, :] = rng.permutation(S).reshape(N, Cn)        # every draw distinct (exact in fp32: S < 2^24): order statistic r is r
    host[:, 2, :] = np.round(rng.normal(size=(N, Cn)) * 64.0) / 64.0 - 7.0     # many ties, both signs of the exponent
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()

    probs = (0.025, 0.25, 0.5, 0.75, 0.975)
    r = {0, 1, S - 2, S - 1} | {int((S - 1) * p) + k for p in probs for k in (0, 1)} | set(range(7, S, S // 29))
    ranks = rng.permutation(np.array(sorted(r), dtype=np.int64))      # more than one batch of 32, more groups than one launch holds
    assert len(ranks) > 32
    params = np.ascontiguousarray(np.tile(np.array([0, 2], dtype=np.int32), SLOTS // 2))
    out = np.full((SLOTS, len(ranks)), -12345.0)
    ctx = mhx.Context.default(dtype=real)
    mhx.check(mhx.lib().mhx_ctx_order_statistics(ctx.h, C.c_void_p(dev.data_ptr()), N, 4, Cn,
                                                 params.ctypes.data_as(C.POINTER(C.c_int32)), SLOTS,
                                                 ranks.ctypes.data_as(C.POINTER(C.c_int64)), len(ranks),
                                                 out.ctypes.data_as(C.POINTER(C.c_double))))
    want = np.sort(np.moveaxis(host, 1, 0).reshape(4, S).astype(np.float64), axis=1)
    assert np.array_equal(want[0], np.arange(S, dtype=np.float64))
    assert np.array_equal(out[0], ranks.astype(np.float64))
    assert np.array_equal(out[1], want[2, ranks])
    # every slot of a row selects the same draws
    assert np.array_equal(out[0::2], np.broadcast_to(out[0], (SLOTS // 2, len(ranks))))
    assert np.array_equal(out[1::2], np.broadcast_to(out[1], (SLOTS // 2, len(ranks))))
