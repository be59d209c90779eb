"""What tests/test_composite_cpu.py and tests/test_gpu_composite.py share: the engine's proposals made from the entries of
tests/composite_restatement.py (the same `emap` callables the restatement evaluates, traced)."""
import family_restatement as F


def tracing_namespace(mhx):
    """the namespace an entry's parameter map is traced with (the restatement evaluates the same map with conditional_restatement.WIDTH)"""
    T = mhx.trace

    class M:
        log, exp, abs, fma, sum_over = staticmethod(T.log), staticmethod(T.exp), staticmethod(T.abs), staticmethod(T.fma), staticmethod(T.sum_over)
        c = staticmethod(float)
    return M


def dists(mhx, params):
    """[(family, p0, p1)] -> the engine's distribution objects"""
    cls = [mhx.Normal, mhx.Uniform, mhx.Laplace, mhx.Cauchy, mhx.Exponential, mhx.Gamma, mhx.InverseGamma]
    return [cls[f](p0) if f == F.EXPONENTIAL else cls[f](p0, p1) for f, p0, p1 in params]


def entry_function(mhx, entry):
    """the entry's map as the engine takes it: a function of the entry's own slice (a scalar for one parameter)"""
    _, n, _, _, emap = entry
    m = tracing_namespace(mhx)
    if n == 1:
        return lambda x: dists(mhx, emap(m, [x]))[0]
    return lambda x: dists(mhx, emap(m, list(x)))


def entry_proposal(mhx, entry, as_function=False):
    """RandomWalkProposal / StaticProposal of one entry: a fixed distribution (or list) when the map is constant, else a function"""
    name, n, static, symmetric, emap = entry
    fn = entry_function(mhx, entry)
    P = mhx.StaticProposal if static else mhx.RandomWalkProposal
    if as_function or any(mhx.trace.trace_composite([(name, n, fn)]).mapped):
        return P(fn, dim=n, issymmetric=symmetric)
    comps = dists(mhx, emap(tracing_namespace(mhx), [0.0] * n))
    what = comps[0] if n == 1 else comps
    assert not (static and symmetric), "a fixed static proposal cannot be declared symmetric"
    return P(what) if static else P(what, issymmetric=symmetric)


def list_sampler(mhx, entries):
    return mhx.MetropolisHastings([entry_proposal(mhx, e) for e in entries])


def named_sampler(mhx, entries):
    return mhx.MetropolisHastings(mhx.NamedProposals(**{e[0]: entry_proposal(mhx, e) for e in entries}))
