"""Test-side restatement of the composite-proposal arithmetic: the Metropolis-Hastings step of a run whose
proposal is an ordered list of blocks of univariate components, each block with its own kind (walk or static), its own symmetric
flag and, optionally, parameters that depend on the block's own slice of the state.  Plain Python with numpy scalars of the run's
width.

It is composed from tests/family_restatement.py (`draw_all`, `r`), tests/conditional_restatement.py (`rows_of`, `valid`, `K`, `Z`,
`WIDTH`) and the oracle's primitives only, and imports nothing from the engine.

A case is a list of ENTRIES (name, count, static, symmetric, emap): `emap(m, xs) -> [(family, p0, p1)] * count` is written once
against the namespace `m` of conditional_restatement and sees ONLY the entry's own slice xs (a list of `count` numbers).  The GPU
test traces it into the engine's proposals entry by entry; `run` below evaluates it with WIDTH.  Z_b is formed for every block that
is not symmetric: for a block of constants it is Z - Z = +0, which changes no comparison (the kernels may leave it out)."""
import numpy as np

import conditional_restatement as R
import family_restatement as F
from oracle import oracle as O


def blocks_of(entries):
    """[(first, count, static, symmetric)]"""
    out, first = [], 0
    for _, n, static, symmetric, _ in entries:
        out.append((first, n, bool(static), bool(symmetric)))
        first += n
    return out


def pmap_of(entries):
    """the map over the WHOLE state: every entry's map over its own slice, one after the other"""
    def pmap(m, x):
        out, first = [], 0
        for _, n, _, _, emap in entries:
            out += list(emap(m, list(x[first:first + n])))
            first += n
        return out
    return pmap


def with_kinds(entries, static):
    """the same entries, every block forced to one kind"""
    return [(name, n, static, sym, emap) for name, n, _, sym, emap in entries]


def with_symmetric(entries, index, symmetric):
    return [(name, n, st, symmetric if i == index else sym, emap) for i, (name, n, st, sym, emap) in enumerate(entries)]


def regrouped(entries, sizes, static=False, symmetric=False):
    """the same components under another grouping: blocks of the given sizes, all of one kind (for the draws, which depend on
    neither)"""
    pmap = pmap_of(entries)
    d = sum(n for _, n, _, _, _ in entries)
    assert sum(sizes) == d
    out, first = [], 0
    for i, n in enumerate(sizes):
        # (a regrouped entry reads its slice out of a whole state whose other coordinates it must not need: only used with maps
        # that are constant or stay inside the new block)
        def emap(m, xs, first=first, n=n):
            x = [m.c(0.0)] * d
            x[first:first + n] = xs
            return pmap(m, x)[first:first + n]
        out.append(("g%d" % i, n, static, symmetric, emap))
        first += n
    return out


def run(target, pmap, d, blocks, n_samples, seed, first_chain, nchains, init=None):
    """The chains of `n_samples` recorded states (sample 1 = the initial state, one transition between samples) under the composite
    proposal (pmap, blocks); blocks = [(first, count, static, symmetric)], contiguous, in order, covering 0 .. d-1.  init [d][nchains],
    or None = a bare draw x = 0 + xi from the (then constant) components, streams INIT / FAMILY_INIT, step 0."""
    assert [b[0] for b in blocks] == list(np.cumsum([0] + [b[1] for b in blocks[:-1]])) and sum(b[1] for b in blocks) == d
    static_of = [st for _, n, st, _ in blocks for _ in range(n)]
    N, Cn = n_samples, nchains
    samples = np.empty((N, d + 1, Cn), dtype=O.real())
    accepted = np.zeros((N, Cn), dtype=np.uint8)
    fx = np.empty((d, Cn), dtype=O.real())
    flp = np.empty(Cn, dtype=O.real())
    cnt = np.zeros(Cn, dtype=np.uint32)
    first_xi = np.empty((d, Cn), dtype=O.real())                # the draws of step 1, for the tests of the grouping
    with np.errstate(all="ignore"):
        for c in range(Cn):
            cid = first_chain + c
            if init is not None:
                x = [F.r(init[k][c]) + F.r(0) for k in range(d)]
            else:
                rows0 = R.rows_of(pmap(R.WIDTH, [F.r(0)] * d))
                x = [F.r(0) + xi for xi in F.draw_all(rows0, seed, cid, 0, O.STREAM_INIT, F.STREAM_FAMILY_INIT)]
            lp = F.r(target(np.array(x, dtype=O.real())))
            rx = R.rows_of(pmap(R.WIDTH, x))
            assert R.valid(rx), "the initial state of chain %d has invalid parameters" % c
            samples[0, :d, c], samples[0, d, c] = x, lp
            for step in range(1, N):
                xi = F.draw_all(rx, seed, cid, step, O.STREAM_PROPOSAL, F.STREAM_FAMILY)
                if step == 1:
                    first_xi[:, c] = xi
                y = [xi[k] if static_of[k] else x[k] + xi[k] for k in range(d)]
                ry = R.rows_of(pmap(R.WIDTH, y))
                ok = R.valid(ry)
                lpy = F.r(target(np.array(y, dtype=O.real())))
                acc = False
                if ok:                                      # an invalid p(y) is rejected by a branch of its own
                    ratio = None
                    for first, n, static, symmetric in blocks:
                        if symmetric:
                            continue
                        ks = range(first, first + n)
                        bx, by = rx[first:first + n], ry[first:first + n]
                        if static:
                            kk = R.K(by, [x[k] for k in ks]) - R.K(bx, [y[k] for k in ks])
                        else:
                            kk = R.K(by, [x[k] - y[k] for k in ks]) - R.K(bx, [y[k] - x[k] for k in ks])
                        rb = kk + (R.Z(by) - R.Z(bx))
                        ratio = rb if ratio is None else ratio + rb
                    loga = (lpy - lp) if ratio is None else (lpy - lp) + ratio
                    acc = bool(F.r(O.accept_logu(seed, cid, step)) < loga)
                if acc:
                    x, lp, rx = y, lpy, ry
                    cnt[c] += 1
                samples[step, :d, c], samples[step, d, c] = x, lp
                accepted[step, c] = 1 if acc else 0
            fx[:, c], flp[c] = x, lp
    return dict(samples=samples, accepted=accepted, final_x=fx, final_lp=flp, accept_counts=cnt, first_xi=first_xi)


# ---------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_composite.py.  Every target is the isotropic standard Gaussian of the case's dimension.
C, N, FIRST_CHAIN = 70, 12, 3                       # a full wave and a partial one


def seed_of(d):
    return 0xC0D1 + d


def init_of(d, pos, nchains=C):
    """default_rng(1234 + d) normals; rows from `pos` on |z| + 0.25 (the support of the one-sided families); as float32"""
    z = np.random.default_rng(1234 + d).normal(size=(d, nchains))
    z[pos:] = np.abs(z[pos:]) + 0.25
    return z.astype(np.float32)


_s = R._scale                                       # s(x) = 0.4 + 0.2 |x|

# A: d = 5 -- a walk of two Normals declared symmetric | a static block Normal, InverseGamma | a walk with a map
CASE_A = [
    ("a", 2, False, True, lambda m, xs: [(F.NORMAL, 0.0, 0.5), (F.NORMAL, 0.0, 0.7)]),
    ("b", 2, True, False, lambda m, xs: [(F.NORMAL, 0.0, 1.0), (F.INVERSE_GAMMA, 2.0, 3.0)]),
    ("c", 1, False, False, lambda m, xs: [(F.LAPLACE, 0.0, _s(m, xs[0]))]),
]
# B: d = 7 -- every component mapped, every map inside its own block
CASE_B = [
    ("a", 2, False, False, lambda m, xs: [(F.NORMAL, m.c(0.1) * xs[1], _s(m, xs[0])), (F.UNIFORM, -_s(m, xs[1]), _s(m, xs[1]))]),
    ("b", 2, False, False, lambda m, xs: [(F.LAPLACE, 0.0, _s(m, xs[0])), (F.CAUCHY, 0.0, m.c(0.5) * _s(m, xs[1]))]),
    ("c", 3, True, False, lambda m, xs: [(F.EXPONENTIAL, _s(m, xs[0]), 0.0), (F.GAMMA, 0.7, _s(m, xs[1])), (F.INVERSE_GAMMA, 2.0, _s(m, xs[2]))]),
]
CASES = {"A": (5, 3, CASE_A), "B": (7, 4, CASE_B)}


def run_case(oracle, entries, d, pos, nchains=C, n_samples=N, first_chain=FIRST_CHAIN):
    return run(oracle.iso_gauss(d), pmap_of(entries), d, blocks_of(entries), n_samples, seed_of(d), first_chain, nchains,
               init_of(d, pos, C)[:, :nchains])
