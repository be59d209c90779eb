"""Host mirror of the AdvancedMH.jl API surface for the GPU hot path.

Same names and keyword meaning as the reference so that its tests read the same:

    model   = DensityModel(IsoGaussian(100))                      # src/AdvancedMH.jl:52-54
    spl     = RWMH(MvNormal(zeros(100), 0.238**2 * I))            # src/mh-core.jl:50-51
    chain   = sample(model, spl, 1000, 65536; discard_initial=1000)  # AbstractMCMC.sample (re-export, src/AdvancedMH.jl:30)

Every call goes through the C ABI of libmhx.so (include/mhx.h); nothing here computes a sample on
the CPU.  A Python callable cannot be lowered to the device: DensityModel takes one of the
catalogue log-densities below or HipLogDensity(source) (hiprtc-compiled, inlined per lane).
"""
import ctypes as C
import math

import numpy as np

from . import _lib as L
from . import trace as _trace

# ------------------------------------------------------------------------------------------------
# distributions (the subset of Distributions.jl the GPU path accepts)


class _Identity:
    """LinearAlgebra.I; supports `s * I`."""

    def __init__(self, scale=1.0):
        self.scale = float(scale)

    def __rmul__(self, s):
        return _Identity(self.scale * float(s))

    __mul__ = __rmul__


I = _Identity()


def zeros(d):
    return np.zeros(int(d))


def _param(v):
    """a distribution's parameter: a number, or -- inside a function proposal being traced (mhx.trace.trace_proposal) -- a traced one"""
    return v if isinstance(v, _trace.Sym) else float(v)


class Normal:
    family = L.FAMILY_NORMAL

    def __init__(self, mu=0.0, sigma=1.0):
        self.mu, self.sigma = _param(mu), _param(sigma)

    def rand(self, rng):
        return self.mu + self.sigma * rng.standard_normal()

    def params(self):
        return self.mu, self.sigma


class InverseGamma:
    family = L.FAMILY_INVERSE_GAMMA

    def __init__(self, shape=1.0, scale=1.0):
        self.shape, self.scale = _param(shape), _param(scale)

    def rand(self, rng):
        return self.scale / rng.gamma(self.shape)

    def params(self):
        return self.shape, self.scale


# The other univariate families a proposal component may be (src/proposal.jl:23-35 with a vector of Distributions univariates;
# test/runtests.jl:188-189,266-271), parameters as in Distributions.jl.  `rand` is the host draw (ensemble initialisation); as a
# component of a RandomWalkProposal / StaticProposal they are drawn on the device.
class Uniform:
    family = L.FAMILY_UNIFORM

    def __init__(self, a=0.0, b=1.0):
        self.a, self.b = _param(a), _param(b)

    def rand(self, rng):
        return self.a + (self.b - self.a) * rng.random()

    def params(self):
        return self.a, self.b


class Laplace:
    family = L.FAMILY_LAPLACE

    def __init__(self, mu=0.0, theta=1.0):
        self.mu, self.theta = _param(mu), _param(theta)

    def rand(self, rng):
        return rng.laplace(self.mu, self.theta)

    def params(self):
        return self.mu, self.theta


class Cauchy:
    family = L.FAMILY_CAUCHY

    def __init__(self, mu=0.0, sigma=1.0):
        self.mu, self.sigma = _param(mu), _param(sigma)

    def rand(self, rng):
        return self.mu + self.sigma * rng.standard_cauchy()

    def params(self):
        return self.mu, self.sigma


class Exponential:
    family = L.FAMILY_EXPONENTIAL

    def __init__(self, theta=1.0):
        self.theta = _param(theta)

    def rand(self, rng):
        return rng.exponential(self.theta)

    def params(self):
        return self.theta, 0.0


class Gamma:
    family = L.FAMILY_GAMMA

    def __init__(self, alpha=1.0, theta=1.0):
        self.alpha, self.theta = _param(alpha), _param(theta)

    def rand(self, rng):
        return rng.gamma(self.alpha, self.theta)

    def params(self):
        return self.alpha, self.theta


class TDist:
    """TDist(nu).  As a proposal component only nu = 1 is lowered: it IS Cauchy(0, 1)."""

    def __init__(self, nu):
        self.nu = float(nu)

    def rand(self, rng):
        return rng.standard_t(self.nu)


_UNIVARIATES = (Normal, Uniform, Laplace, Cauchy, Exponential, Gamma, InverseGamma)


def _lower_univariate(dist):
    """a univariate of one of the device families, checked: TDist(1) -> Cauchy(0, 1); bad parameters raise"""
    if isinstance(dist, TDist):
        if dist.nu != 1.0:
            raise L.ArgumentError(L.MHX_EINVAL, "TDist(%g): only TDist(1) = Cauchy(0, 1) is lowered to the device; any other number of "
                                  "degrees of freedom has no device sampler" % dist.nu)
        return Cauchy(0.0, 1.0)
    if not isinstance(dist, _UNIVARIATES):
        return None
    p0, p1 = dist.params()
    name = type(dist).__name__
    ok = math.isfinite(p0) and math.isfinite(p1)
    if isinstance(dist, Uniform):
        ok = ok and p0 < p1
    elif isinstance(dist, Exponential):
        ok = ok and p0 > 0
    elif isinstance(dist, (Gamma, InverseGamma)):
        ok = ok and p0 > 0 and p1 > 0
    else:
        ok = ok and p1 > 0
    if not ok:
        raise L.ArgumentError(L.MHX_EINVAL, "%s%r: bad parameters (scale and shape parameters must be positive, Uniform needs a < b, "
                              "everything finite)" % (name, dist.params() if not isinstance(dist, Exponential) else (p0,)))
    return dist


class ComponentProposal:
    """A proposal distribution made of independent univariate components, at least one of them not Normal: what
    RandomWalkProposal / StaticProposal hold for `[Normal(0, 1), InverseGamma(2, 3)]`, `Laplace()`, ... (an all-Normal vector is an
    MvNormal, as before).  `table()` is the component table of mhx_rwmh_create_components."""

    def __init__(self, comps):
        self.comps = list(comps)
        self.dim = len(self.comps)

    def table(self):
        return [(c.family,) + tuple(c.params()) for c in self.comps]

    def symmetric_about_zero(self):
        def sym(c):
            if isinstance(c, (Normal, Laplace, Cauchy)):
                return c.params()[0] == 0
            return isinstance(c, Uniform) and c.a == -c.b
        return all(sym(c) for c in self.comps)

    def rand(self, rng):
        return np.array([c.rand(rng) for c in self.comps])


class MvNormal:
    """MvNormal(mean, cov): cov may be `s*I`, a vector of variances (diagonal) or a dense PD matrix."""

    def __init__(self, mean, cov=I):
        self.mean = np.asarray(mean, dtype=np.float64)
        self.dim = int(self.mean.size)
        if isinstance(cov, _Identity):
            self.kind, self.scale, self.vec = L.PROP_ISO, math.sqrt(cov.scale), None
        else:
            cov = np.asarray(cov, dtype=np.float64)
            if cov.ndim == 1:
                if cov.size != self.dim:
                    raise L.ArgumentError(L.MHX_EINVAL, "MvNormal: mean and covariance dimensions differ")
                self.kind, self.scale, self.vec = L.PROP_DIAG, 1.0, np.sqrt(cov)
            else:
                if cov.shape != (self.dim, self.dim):
                    raise L.ArgumentError(L.MHX_EINVAL, "MvNormal: mean and covariance dimensions differ")
                try:
                    chol = np.linalg.cholesky(cov)
                except np.linalg.LinAlgError as e:
                    raise L.PosDefException(L.MHX_ENOTPD, "MvNormal: covariance is not positive definite") from e
                self.kind, self.scale, self.vec = L.PROP_DENSE, 1.0, pack_lower(chol)

    def rand(self, rng):
        z = rng.standard_normal(self.dim)
        if self.kind == L.PROP_ISO:
            return self.mean + self.scale * z
        if self.kind == L.PROP_DIAG:
            return self.mean + self.vec * z
        return self.mean + unpack_lower(self.vec, self.dim) @ z


def pack_lower(M):
    M = np.asarray(M)
    return np.concatenate([M[i, :i + 1] for i in range(M.shape[0])]).astype(np.float64)


def unpack_lower(p, d):
    M = np.zeros((d, d), dtype=np.asarray(p).dtype)
    o = 0
    for i in range(d):
        M[i, :i + 1] = p[o:o + i + 1]
        o += i + 1
    return M


def _as_mvnormal(dist):
    """RWMH accepts MvNormal, a vector of univariate Normals (src/proposal.jl:26-28) or an Int."""
    if isinstance(dist, (int, np.integer)):
        return MvNormal(zeros(dist), I)                           # src/mh-core.jl:51
    if isinstance(dist, MvNormal):
        return dist
    if isinstance(dist, Normal):                                      # scalar parameter: RandomWalkProposal(Normal(0, 1))
        return MvNormal([dist.mu], np.array([dist.sigma ** 2]))
    if isinstance(dist, (list, tuple)) and all(isinstance(p, Normal) for p in dist):
        mv = MvNormal([p.mu for p in dist], np.array([p.sigma ** 2 for p in dist]))
        return mv
    raise L.ArgumentError(L.MHX_EINVAL, "the GPU path supports MvNormal / vector-of-Normal proposals here; "
                          "got %r" % (dist,))


class ConditionalProposal:
    """What a RandomWalkProposal / StaticProposal holds for a FUNCTION of the state (src/proposal.jl:92-126): `fn(x)` returns one
    univariate (dim = 1, x a scalar) or a list of `dim` univariates whose parameters may depend on x.  It is traced once
    (mhx.trace.trace_proposal): `.table()` is the component table, `.source` / `.data` the parameter map of
    mhx_rwmh_create_conditional."""

    def __init__(self, fn, dim):
        if dim is None:
            raise L.ArgumentError(L.MHX_EINVAL, "a function proposal needs dim=: the number of parameters its function takes")
        self.fn, self.dim = fn, int(dim)
        self.traced = _trace.trace_proposal(fn, self.dim)
        self.source, self.data = self.traced.source, self.traced.data
        for fam, p0, p1 in self.traced.table:                 # the constants, checked like any component's
            _lower_univariate(_UNIVARIATES[fam](p0) if fam == L.FAMILY_EXPONENTIAL else _UNIVARIATES[fam](p0, p1))

    def table(self):
        return list(self.traced.table)


class NamedProposals:
    """NamedProposals(a=p1, b=p2, ...): the reference's NamedTuple of proposals `(a = ..., b = ...)` (src/proposal.jl:163-175) in its
    full form -- each entry a RandomWalkProposal or StaticProposal of any kind, scalar or vector, fixed or a function of the entry's
    OWN slice of the state.  The keys name the parameters; a vector entry `a` of length n names `a[1] .. a[n]`."""

    def __init__(self, **entries):
        if not entries:
            raise L.ArgumentError(L.MHX_EINVAL, "NamedProposals: empty proposal")
        self.entries = dict(entries)


class CompositeProposal:
    """What MetropolisHastings holds for a list of proposals or a NamedProposals that does not fold into one vector proposal: an
    ordered list of blocks, each with its own kind, symmetric flag and (for a function entry) parameter map over its own slice
    (DESIGN.md section 3.15).  `.blocks` [(first, count, flags)], `.table()`, `.mapped`, `.source` / `.data`: the arguments of
    mhx_rwmh_create_composite."""

    issymmetric = False

    def __init__(self, labels, parts, named):
        entries, self.blocks, names, first = [], [], [], 0
        for label, q in zip(labels, parts):
            pr = q.proposal
            if isinstance(pr, ConditionalProposal):
                n, what = pr.dim, pr.fn
            elif isinstance(pr, ComponentProposal):
                n, what = pr.dim, list(pr.comps)
            else:
                if pr.kind == L.PROP_DENSE:
                    raise L.ArgumentError(L.MHX_EINVAL, "entry %r: an MvNormal with a dense covariance is not a list of independent components: "
                                          "a composite proposal takes isotropic or diagonal covariances (give a dense proposal alone)" % (label,))
                n = pr.dim
                what = [Normal(float(pr.mean[i]), float(pr.vec[i]) if pr.kind == L.PROP_DIAG else pr.scale) for i in range(n)]
            flags = (L.BLOCK_STATIC if isinstance(q, StaticProposal) else 0) | (L.BLOCK_SYMMETRIC if q.issymmetric else 0)
            self.blocks.append((first, n, flags))
            entries.append((label, n, what))
            names += [str(label)] if n == 1 else ["%s[%d]" % (label, i + 1) for i in range(n)]
            first += n
        self.dim = first
        self.param_names = names if named else None
        self.traced = _trace.trace_composite(entries)
        self.mapped, self.source, self.data = list(self.traced.mapped), self.traced.source, self.traced.data
        for fam, p0, p1 in self.traced.table:                 # the constants, checked like any component's
            _lower_univariate(_UNIVARIATES[fam](p0) if fam == L.FAMILY_EXPONENTIAL else _UNIVARIATES[fam](p0, p1))
        self.proposal = self                                    # (MetropolisHastings(...).proposal.proposal: what the run lowers)

    def table(self):
        return list(self.traced.table)


def _as_proposal(dist, dim=None):
    """What a RandomWalkProposal / StaticProposal holds: an MvNormal (everything _as_mvnormal takes, exactly as it lowers it), or a
    ComponentProposal for one univariate of a device family / a vector mixing them with Normals."""
    if isinstance(dist, (ComponentProposal, ConditionalProposal)):
        return dist
    if callable(dist):
        return ConditionalProposal(dist, dim)
    if dim is not None and not isinstance(dist, (list, tuple, np.ndarray, MvNormal)) and int(dim) != 1:
        raise L.ArgumentError(L.MHX_EINVAL, "dim = %d given with a scalar proposal" % dim)
    one = None if isinstance(dist, Normal) else _lower_univariate(dist)
    if one is not None:
        return ComponentProposal([one])
    if isinstance(dist, (list, tuple)) and len(dist) and not all(isinstance(p, Normal) for p in dist):
        comps = [_lower_univariate(p) for p in dist]
        if any(c is None for c in comps):
            raise L.ArgumentError(L.MHX_EINVAL, "a vector proposal takes Normal, Uniform, Laplace, Cauchy, Exponential, Gamma, InverseGamma "
                                  "or TDist(1) components; got %r" % (dist,))
        return ComponentProposal(comps)
    return _as_mvnormal(dist)


# ------------------------------------------------------------------------------------------------
# log-densities that can live on the device


class _TargetSpec:
    kind = None
    dim = 0
    params = None

    def build(self, ctx):
        h = C.c_void_p()
        p = None if self.params is None else ctx.arr(self.params)      # rounded once to the context's dtype
        L.check(L.lib().mhx_target_builtin(ctx.h, self.kind, self.dim, L.rptr(p), 0 if p is None else p.size,
                                           C.byref(h)))
        return h


class IsoGaussian(_TargetSpec):
    """logpdf(MvNormal(zeros(d), I), x)"""
    kind = L.TARGET_ISO_GAUSS

    def __init__(self, d):
        self.dim = int(d)


MAX_BAND = 8        # MHX_EMCEE_MAX_BAND: the widest band the engine's band form is specialised for


def precision_factor(Sigma):
    """A = inv(chol(Sigma)) in float64 (log-density -1/2 |A x|^2 + log det A), with the STRUCTURAL zeros of a banded factor
    restored.  A Markov / autoregressive / banded-precision model (Sigma_ij = rho^|i-j|: A is bidiagonal) comes out of the
    inversion with round-off ~1e-15 where the exact factor is zero; the engine detects an EXACTLY banded factor and skips the
    zeros (same bits: fma(0, y, w) == w), which lets such a model run at its own cost instead of the dense d(d+1)/2.
    The rule is scale-aware and conservative: an OFF-diagonal entry is round-off iff |A_ij| <= 256 eps |A_jj| (relative
    to its COLUMN's scale: at stationarity x_j ~ 1/A_jj, so dropping the entry moves row i of A x -- a unit-variance number -- by
    less than 256 eps; a model whose standard deviations span many decades keeps every genuine entry);
    the diagonal is never touched; and the cleaned factor is used only if it really is banded (bandwidth <= 8, the engine's band
    form) -- otherwise the raw inverse is kept, the reference's MvNormal has no truncation at all."""
    A = np.tril(np.linalg.inv(np.linalg.cholesky(np.asarray(Sigma, dtype=np.float64))))
    d = A.shape[0]
    dg = np.abs(np.diag(A))
    noise = np.abs(A) <= 256.0 * np.finfo(np.float64).eps * dg[None, :]
    noise[np.arange(d), np.arange(d)] = False
    B = np.where(noise, 0.0, A)
    i, j = np.nonzero(B)
    return B if d > 1 and int((i - j).max()) <= min(MAX_BAND, d - 2) else A


class CorrGaussian(_TargetSpec):
    """logpdf(MvNormal(zeros(d), Sigma), x); stored as inv(chol(Sigma)) packed lower (precision_factor)."""
    kind = L.TARGET_CORR_GAUSS

    def __init__(self, Sigma):
        Sigma = np.asarray(Sigma, dtype=np.float64)
        self.dim = Sigma.shape[0]
        try:
            A = precision_factor(Sigma)
        except np.linalg.LinAlgError as e:
            raise L.PosDefException(L.MHX_ENOTPD, "CorrGaussian: Sigma is not positive definite") from e
        self.params = pack_lower(A)


class IIDNormal(_TargetSpec):
    """theta = (mu, sigma):  sigma >= 0 ? sum(logpdf.(Normal(mu, sigma), data)) : -Inf   (README.md:29-31)"""
    kind = L.TARGET_IID_NORMAL
    dim = 2

    def __init__(self, data):
        self.params = np.asarray(data, dtype=np.float64).ravel()


class Banana(_TargetSpec):
    kind = L.TARGET_BANANA

    def __init__(self, d, b=0.03):
        self.dim = int(d)
        self.params = np.array([b], dtype=np.float64)


class Funnel(_TargetSpec):
    kind = L.TARGET_FUNNEL

    def __init__(self, d):
        self.dim = int(d)


class HipLogDensity(_TargetSpec):
    """A user log-density as HIP source:  MHX_LOGDENSITY(x, d, data, ndata) { ...; return lp; }  written against
    `mhx_real` / `MHX_R(literal)` so that it compiles for either dtype."""
    kind = L.TARGET_USER

    def __init__(self, source, dim, data=None):
        self.source, self.dim = source, int(dim)
        self.params = None if data is None else np.asarray(data, dtype=np.float64).ravel()

    def build(self, ctx):
        h = C.c_void_p()
        p = None if self.params is None else ctx.arr(self.params)
        L.check(L.lib().mhx_target_from_hip_source(ctx.h, self.source.encode(), self.dim, L.rptr(p),
                                                   0 if p is None else p.size, C.byref(h)))
        return h


class HipMap:
    """A map of the saved draws as HIP source (Run.derive):  MHX_DERIVED(x, y, d, data, ndata) { y.set(0, x[1] * x[1]); }  -- x[0 .. d-1]
    one draw, x[d] its lp, y.set(j, value) output j < nout -- written against `mhx_real` / `MHX_R(literal)` so that it compiles for
    either dtype.  The hand-written form of what mhx.trace.trace_map records."""

    def __init__(self, source, nout, data=None):
        self.source, self.nout = source, int(nout)
        self.data = None if data is None else np.asarray(data, dtype=np.float64).ravel()


class HipPredictive(HipMap):
    """A predictive map of the saved draws as HIP source (Run.predict):  MHX_PREDICTIVE(x, rng, y, d, data, ndata) { y.set(0, rng.draw(0,
    MHX_FAMILY_NORMAL, x[0], x[1])); }  -- HipMap's x, y, d and data, and rng, the stream of this (chain, saved draw): rng.draw(k, family,
    p0, p1) / rng.gamma(k, family, alpha, theta, d, c, 1 / alpha) as documented at the macro (csrc/mhx_device_math.h).  The hand-written
    form of what mhx.trace.trace_predictive records."""


class HipPointwise:
    """The log-likelihood of one data row under one draw as HIP source (Run.pointwise):  MHX_POINTWISE(x, r, m, d, data, ndata) { return
    ...; }  -- x the draw as HipMap's, r[j] entry j < m of the current data row -- with its `rows` ([nrows] or [nrows][rowlen]).  The
    hand-written form of what mhx.trace.trace_pointwise records; it has no host evaluator (Chains.dic needs a traced function)."""

    def __init__(self, source, rows, data=None):
        self.source = source
        self.rows = _pointwise_rows("HipPointwise", rows)
        self.data = None if data is None else np.asarray(data, dtype=np.float64).ravel()


def _pointwise_rows(who, rows):
    arr = np.asarray(rows, dtype=np.float64)
    if arr.ndim not in (1, 2) or arr.size == 0:
        raise L.ArgumentError(L.MHX_EINVAL, "%s: rows must be a non-empty 1-D or 2-D array" % who)
    return np.ascontiguousarray(arr.reshape(arr.shape[0], -1))


def _pointwise_fn(who, fn, rows, dim, names, model_names):
    """(the function of Run.pointwise / Group.pointwise -- traced where it is a callable --, its rows [nrows][rowlen] float64)"""
    got = fn
    if isinstance(fn, (HipPointwise, _trace.TracedPointwise)):
        mat = fn.rows if rows is None else _pointwise_rows(who, rows)
        if mat.shape[1] != fn.rows.shape[1]:
            raise L.ArgumentError(L.MHX_EINVAL, "%s: rows of %d entries, the function was written for rows of %d" % (who, mat.shape[1], fn.rows.shape[1]))
    elif callable(fn):
        if rows is None:
            raise L.ArgumentError(L.MHX_EINVAL, "%s: a callable needs the data rows" % who)
        mat = _pointwise_rows(who, rows)
        try:
            fn = _trace.trace_pointwise(fn, dim, rows, names=names if names is not None else model_names)
        except _trace.TraceError as e:
            raise L.ArgumentError(L.MHX_EINVAL, "%s: the callable cannot be traced: %s" % (who, e)) from e
    else:
        raise L.ArgumentError(L.MHX_EINVAL, "%s: a callable, a TracedPointwise or a HipPointwise is needed, got %r" % (who, got))
    if isinstance(fn, _trace.TracedPointwise) and fn.dim != dim:
        raise L.ArgumentError(L.MHX_EINVAL, "%s: the function was traced for %d parameters, the run has %d" % (who, fn.dim, dim))
    return fn, mat


class PointwiseSums(dict):
    """what Run.pointwise / Group.pointwise return: dict(max, sumexp, s1, s2, bad, shift -- float64 [nrows] each -- and T), the raw
    per-row reductions of include/mhx.h (mhx_run_pointwise).  They are sums on purpose: merge_pointwise adds the members of a group."""


def merge_pointwise(a, b):
    """The PointwiseSums of the union of two disjoint sets of draws taken about the SAME shift (include/mhx.h: mhx_run_pointwise): s1, s2,
    bad and T add; max = max(a, b) and sumexp = sumexp_big + sumexp_small exp(max_small - max_big), on equal maxima (two -inf among them)
    the sums add; a NaN max (a NaN or +inf l among the draws) or a NaN sumexp makes both NaN."""
    if not np.array_equal(a["shift"], b["shift"]):
        raise L.ArgumentError(L.MHX_EINVAL, "merge_pointwise: the two results were taken about different shifts")
    am, bm, asum, bsum = (np.asarray(v, dtype=np.float64) for v in (a["max"], b["max"], a["sumexp"], b["sumexp"]))
    with np.errstate(all="ignore"):
        a_big = am > bm
        big_m, small_m = np.where(a_big, am, bm), np.where(a_big, bm, am)
        big_s, small_s = np.where(a_big, asum, bsum), np.where(a_big, bsum, asum)
        equal = am == bm
        scale = np.where(equal, 1.0, np.exp(np.where(equal, 0.0, small_m - big_m)))       # (never -inf - -inf: equal maxima add)
        se = big_s + small_s * scale
        mx = big_m.copy()
    poisoned = np.isnan(am) | np.isnan(bm) | np.isnan(se)
    mx[poisoned] = np.nan
    se[poisoned] = np.nan
    return PointwiseSums(max=mx, sumexp=se, s1=a["s1"] + b["s1"], s2=a["s2"] + b["s2"], bad=a["bad"] + b["bad"],
                         shift=np.array(a["shift"], dtype=np.float64), T=int(a["T"]) + int(b["T"]))


class PointwiseTable(dict):
    """what Chains.pointwise returns and pointwise_table makes: dict(lppd, mean, var, p_waic, elpd, bad -- float64 [nrows] each -- and T)
    that prints in the style of the HPD table (the first and last rows of a long one)"""

    COLUMNS = ("lppd", "mean", "var", "p_waic", "elpd", "bad")

    def __str__(self):
        n = len(self["lppd"])
        lines = ["Pointwise log-likelihood (%d rows, %d draws)" % (n, self["T"]), "  row     " + " ".join("%11s" % c for c in self.COLUMNS)]
        show = range(n) if n <= 12 else list(range(6)) + [None] + list(range(n - 5, n))
        for i in show:
            lines.append("  ..." if i is None else "  %-7d " % i + " ".join("%11.4f" % self[c][i] for c in self.COLUMNS))
        return "\n".join(lines)

    __repr__ = __str__


def pointwise_table(sums):
    """The per-row quantities of a PointwiseSums, in float64 on the host:
        lppd    max + log(sumexp) - log(T): the log of the MEAN of p(y_i | theta_s) over ALL T draws.  T divides, not T - bad: a draw whose
                l is -inf is a draw with p = 0 and stays in the divisor; a NaN or +inf l makes max NaN, and with it lppd, so no count of
                such draws is needed
        mean    shift + s1 / n, n = T - bad the draws that entered s1 and s2 (the finite l)
        var     (s2 - s1^2 / n) / (n - 1), the sample variance of those l; NaN where n < 2
        p_waic  var (the WAIC-2 penalty of the row);  elpd = lppd - p_waic;  bad as returned"""
    T = int(sums["T"])
    mx, se, s1, s2, bad, sh = (np.asarray(sums[k], dtype=np.float64) for k in ("max", "sumexp", "s1", "s2", "bad", "shift"))
    with np.errstate(all="ignore"):
        lppd = mx + np.log(se) - math.log(T)
        n = T - bad
        mean = np.where(n >= 1, sh + s1 / n, np.nan)
        var = np.where(n >= 2, (s2 - s1 * s1 / n) / (n - 1.0), np.nan)
        elpd = lppd - var
    return PointwiseTable(lppd=lppd, mean=mean, var=var, p_waic=var.copy(), elpd=elpd, bad=bad.copy(), T=T)


class WaicResult(dict):
    """what Chains.waic returns: dict(elpd_waic, p_waic, waic, se, n_high_variance, pointwise) that prints"""

    def __str__(self):
        s = "WAIC %.4f (se %.4f)   elpd_waic %.4f   p_waic %.4f   rows %d" % (self["waic"], self["se"], self["elpd_waic"], self["p_waic"],
                                                                              len(self["pointwise"]["lppd"]))
        if self["n_high_variance"]:
            s += "\n  %d rows with p_waic > 0.4: WAIC is unreliable there" % self["n_high_variance"]
        return s

    __repr__ = __str__


def waic_from_table(table):
    """elpd_waic = sum_i elpd_i, p_waic = sum_i p_waic_i, waic = -2 elpd_waic, se = 2 sqrt(nrows var_i(elpd_i)) (the sample variance over
    the rows; NaN for one row), n_high_variance = the rows with p_waic > 0.4"""
    elpd, p = table["elpd"], table["p_waic"]
    n = len(elpd)
    with np.errstate(all="ignore"):
        se = 2.0 * math.sqrt(n * float(np.var(elpd, ddof=1))) if n > 1 else math.nan
    return WaicResult(elpd_waic=float(np.sum(elpd)), p_waic=float(np.sum(p)), waic=-2.0 * float(np.sum(elpd)), se=se,
                      n_high_variance=int(np.sum(p > 0.4)), pointwise=table)


class DicResult(dict):
    """what Chains.dic returns: dict(dic, p_d, d_bar, d_hat) that prints"""

    def __str__(self):
        return "DIC %.4f   p_D %.4f   mean deviance %.4f   deviance at the posterior mean %.4f" % (self["dic"], self["p_d"], self["d_bar"], self["d_hat"])

    __repr__ = __str__


def dic_from_table(table, fn, theta_bar, rows):
    """D-bar = -2 sum_i mean_i; D(theta-bar) = -2 sum_i fn(theta-bar, row_i), on the host by the trace's evaluate; p_D = D-bar -
    D(theta-bar); DIC = D-bar + p_D"""
    d_bar = -2.0 * float(np.sum(table["mean"]))
    d_hat = -2.0 * float(sum(fn.evaluate(theta_bar, r) for r in rows))
    return DicResult(dic=2.0 * d_bar - d_hat, p_d=d_bar - d_hat, d_bar=d_bar, d_hat=d_hat)


class PsisResult(dict):
    """what Run.psis returns: dict(elpd_loo, khat, sigma, tau, lmin, body, n_below, bad -- float64 [nrows] each --, T, M, reff and, with
    tails=True, tails [nrows][M]) as include/mhx.h defines them (mhx_run_psis)"""


def psis_tail_length(T, reff=1.0):
    """M = min(floor(0.2 T), ceil(3 sqrt(T / reff))) in float64, as the engine computes it; M < 5 counts as 0 (no smoothing)"""
    m = min(math.floor(0.2 * float(T)), math.ceil(3.0 * math.sqrt(float(T) / float(reff))))
    return 0 if m < 5 else int(m)


class LooTable(dict):
    """what loo_table makes: dict(elpd_loo, p_loo, khat, lppd, bad -- float64 [nrows] each --, T, M) that prints as PointwiseTable does"""

    COLUMNS = ("elpd_loo", "p_loo", "khat", "lppd", "bad")

    def __str__(self):
        n = len(self["elpd_loo"])
        lines = ["PSIS-LOO (%d rows, %d draws, tails of %d)" % (n, self["T"], self["M"]), "  row     " + " ".join("%11s" % c for c in self.COLUMNS)]
        show = range(n) if n <= 12 else list(range(6)) + [None] + list(range(n - 5, n))
        for i in show:
            lines.append("  ..." if i is None else "  %-7d " % i + " ".join("%11.4f" % self[c][i] for c in self.COLUMNS))
        return "\n".join(lines)

    __repr__ = __str__


def loo_table(psis, sums):
    """Per row, in float64 on the host: elpd_loo and khat of a PsisResult, lppd of a PointwiseSums of the SAME draws and rows (as
    pointwise_table forms it), p_loo = lppd - elpd_loo; bad as the PsisResult counts it"""
    if int(psis["T"]) != int(sums["T"]) or len(psis["elpd_loo"]) != len(sums["max"]):
        raise L.ArgumentError(L.MHX_EINVAL, "loo_table: the two results are not of the same draws and rows")
    lppd = pointwise_table(sums)["lppd"]
    elpd = np.array(psis["elpd_loo"], dtype=np.float64)
    with np.errstate(all="ignore"):
        p = lppd - elpd
    return LooTable(elpd_loo=elpd, p_loo=p, khat=np.array(psis["khat"], dtype=np.float64), lppd=lppd,
                    bad=np.array(psis["bad"], dtype=np.float64), T=int(psis["T"]), M=int(psis["M"]))


KHAT_EDGES = (0.5, 0.7, 1.0)            # the classes of the printout: (-inf, 0.5], (0.5, 0.7], (0.7, 1], (1, inf)


def khat_threshold(T):
    """min(1 - 1 / log10(T), 0.7): the khat up to which T draws give a reliable estimate (Vehtari et al. 2024)"""
    return min(1.0 - 1.0 / math.log10(T), 0.7) if T > 1 else -math.inf


class LooResult(dict):
    """what Chains.loo returns: dict(elpd_loo, p_loo, looic, se, khat_counts, khat_threshold, pointwise) that prints"""

    def __str__(self):
        c = self["khat_counts"]
        return ("PSIS-LOO   elpd_loo %.4f (se %.4f)   p_loo %.4f   looic %.4f   rows %d\n"
                "  khat (-inf, 0.5]: %d   (0.5, 0.7]: %d   (0.7, 1]: %d   (1, inf): %d   sample-size threshold %.3f" % (
                    self["elpd_loo"], self["se"], self["p_loo"], self["looic"], len(self["pointwise"]["elpd_loo"]), c[0], c[1], c[2], c[3],
                    self["khat_threshold"]))

    __repr__ = __str__


def loo_from_table(table):
    """elpd_loo = sum_i elpd_loo_i, p_loo = sum_i p_loo_i, looic = -2 elpd_loo, se = 2 sqrt(nrows var_i(elpd_loo_i)) as waic_from_table
    forms it, khat_counts = the rows per class of KHAT_EDGES (a NaN khat is in none), khat_threshold = khat_threshold(T)"""
    elpd, k = table["elpd_loo"], table["khat"]
    n = len(elpd)
    with np.errstate(all="ignore"):
        se = 2.0 * math.sqrt(n * float(np.var(elpd, ddof=1))) if n > 1 else math.nan
        counts = [int(np.sum(k <= 0.5)), int(np.sum((k > 0.5) & (k <= 0.7))), int(np.sum((k > 0.7) & (k <= 1.0))), int(np.sum(k > 1.0))]
    return LooResult(elpd_loo=float(np.sum(elpd)), p_loo=float(np.sum(table["p_loo"])), looic=-2.0 * float(np.sum(elpd)), se=se,
                     khat_counts=counts, khat_threshold=khat_threshold(table["T"]), pointwise=table)


class CompareTable(list):
    """what compare returns: a list of dict(name, elpd, elpd_diff, se_diff), best first, that prints"""

    def __str__(self):
        lines = ["  %-16s %12s %12s %12s" % ("model", "elpd", "elpd_diff", "se_diff")]
        lines += ["  %-16s %12.4f %12.4f %12.4f" % (r["name"], r["elpd"], r["elpd_diff"], r["se_diff"]) for r in self]
        return "\n".join(lines)

    __repr__ = __str__


def compare(results):
    """Model comparison on the host, as loo_compare: `results` maps a name to a LooResult or a WaicResult (or a LooTable / PointwiseTable)
    over the SAME data rows.  Best (largest total elpd) first; elpd_diff = sum_i (elpd_i - elpd_i^best) and se_diff =
    sqrt(n var_i(elpd_i - elpd_i^best)) (the sample variance over the rows), both 0 for the best model."""
    rows = {}
    for name, r in results.items():
        t = r["pointwise"] if "pointwise" in r else r
        e = np.asarray(t["elpd_loo"] if "elpd_loo" in t else t["elpd"], dtype=np.float64)
        rows[str(name)] = e
    if not rows:
        raise L.ArgumentError(L.MHX_EINVAL, "compare: no models")
    n = {len(e) for e in rows.values()}
    if len(n) != 1:
        raise L.ArgumentError(L.MHX_EINVAL, "compare: the models are not over the same number of data rows")
    n = n.pop()
    order = sorted(rows, key=lambda k: -float(np.sum(rows[k])))
    best = rows[order[0]]
    out = CompareTable()
    for name in order:
        diff = rows[name] - best
        with np.errstate(all="ignore"):
            se = math.sqrt(n * float(np.var(diff, ddof=1))) if n > 1 else math.nan
        out.append(dict(name=name, elpd=float(np.sum(rows[name])), elpd_diff=float(np.sum(diff)), se_diff=0.0 if name == order[0] else se))
    return out


class DensityModel:
    """DensityModel(logdensity) -- src/AdvancedMH.jl:52-54.  `logdensity` is a catalogue log-density, HipLogDensity(source, dim),
    or a Python callable of the parameter vector together with `dim`: the callable is traced once (mhx/trace.py) and lowered
    to the HIP source form, with its reverse-mode gradient (MALA) unless gradient=False."""

    def __init__(self, logdensity, dim=None, gradient=True, names=None):
        self.traced = None
        if names is not None:                   # the closure reads its parameters by name (x.a, x["a"]): test/runtests.jl:184
            names = [str(n) for n in names]
            dim = len(names) if dim is None else dim
        if callable(logdensity) and not isinstance(logdensity, _TargetSpec):
            if dim is None:
                raise L.ArgumentError(L.MHX_EINVAL, "DensityModel(f): pass dim=<number of parameters> so that the callable "
                                      "can be traced (or a catalogue log-density / HipLogDensity(source, dim))")
            from . import trace as _trace
            try:
                self.traced = _trace.trace(logdensity, dim, gradient=gradient, names=names)
            except _trace.TraceError as e:
                raise L.ArgumentError(L.MHX_EINVAL, "DensityModel(f): the callable cannot be traced: %s" % e) from e
            logdensity = HipLogDensity(self.traced.source, dim, data=self.traced.data)      # (the rows of its sum_over loops)
        if not isinstance(logdensity, _TargetSpec):
            raise L.ArgumentError(L.MHX_EINVAL, "DensityModel: unsupported log-density %r" % (logdensity,))
        self.logdensity = logdensity
        self.param_names = names
        self._handles = {}

    @property
    def dim(self):
        return self.logdensity.dim

    def handle(self, ctx):
        if ctx not in self._handles:
            self._handles[ctx] = self.logdensity.build(ctx)
        return self._handles[ctx]


def _is_logdensity_problem(obj):
    """an object that implements the LogDensityProblems interface: dimension() and logdensity(theta)"""
    return callable(getattr(obj, "dimension", None)) and callable(getattr(obj, "logdensity", None))


class LogDensityModel(DensityModel):
    """AbstractMCMC.LogDensityModel(problem) -- the LogDensityProblems form of a model (src/AdvancedMH.jl:56,76-77; README.md:75-90),
    and the ONLY form the reference's RobustAdaptiveMetropolis takes (src/RobustAdaptiveMetropolis.jl:175-181,
    test/RobustAdaptiveMetropolis.jl:1-9,30-56).  `problem` has  dimension() -> d  and  logdensity(theta) -> lp  (the methods
    LogDensityProblems.dimension / .logdensity of the Julia object): the dimension comes from the problem, the log-density is traced
    through problem.logdensity exactly as a closure's is.  A catalogue log-density is its own problem.  `sample(problem, sampler, ...)`
    wraps by itself, as AbstractMCMC does."""

    def __init__(self, problem, gradient=True):
        if isinstance(problem, _TargetSpec):
            super().__init__(problem)
        elif _is_logdensity_problem(problem):
            super().__init__(lambda theta: problem.logdensity(theta), dim=int(problem.dimension()), gradient=gradient)
        else:
            raise L.ArgumentError(L.MHX_EINVAL, "LogDensityModel: %r does not implement dimension() / logdensity(theta)" % (problem,))
        self.problem = problem


def logdensity(model, x, ctx=None, dtype=None):
    """logdensity(model, params) for one point (d,) or a batch (d, n) -- src/AdvancedMH.jl:74."""
    if isinstance(x, Transition):
        return x.lp                                              # cached, src/AdvancedMH.jl:75
    ctx = ctx or L.Context.default(dtype=dtype)
    x = ctx.arr(x)
    single = x.ndim == 1
    xb = x.reshape(model.dim, -1)
    if xb.shape[0] != model.dim:
        raise L.ArgumentError(L.MHX_EINVAL, "logdensity: x has the wrong dimension")
    xb = np.ascontiguousarray(xb)
    lp = np.empty(xb.shape[1], dtype=ctx.real)
    L.check(L.lib().mhx_target_eval(ctx.h, model.handle(ctx), L.rptr(xb), xb.shape[1], L.rptr(lp)))
    return float(lp[0]) if single else lp


class Transition:
    """Transition(params, lp, accepted) -- src/AdvancedMH.jl:61-65."""

    def __init__(self, params, lp, accepted):
        self.params, self.lp, self.accepted = params, lp, accepted


# ------------------------------------------------------------------------------------------------
# samplers


class RandomWalkProposal:
    """RandomWalkProposal{issymmetric}(dist) -- src/proposal.jl:13-21.  `dist` may be a function of the state that returns the
    distribution(s) of the step, e.g. `lambda x: Normal(0, 0.5 + abs(x))` (src/proposal.jl:92-126); it then needs `dim=` and
    `sample(..., initial_params=...)`, and `issymmetric=True` is the user's word that the ratio may be left out (:195)."""

    def __init__(self, proposal, issymmetric=False, dim=None):
        self.proposal = _as_proposal(proposal, dim)
        self.issymmetric = bool(issymmetric)
        if isinstance(self.proposal, ConditionalProposal):
            return
        # a non-zero mean makes the walk drift; its Hastings ratio (src/proposal.jl:58-64,190-192) is then
        # evaluated on the device (generic kernel).  Declaring such a proposal symmetric would skip it.
        if isinstance(self.proposal, ComponentProposal):
            if issymmetric and not self.proposal.symmetric_about_zero():
                raise L.ArgumentError(L.MHX_EINVAL, "a random-walk proposal with a component that is not symmetric about zero is not symmetric")
        elif issymmetric and np.any(self.proposal.mean != 0):
            raise L.ArgumentError(L.MHX_EINVAL, "a random-walk proposal with a non-zero mean is not symmetric")


def SymmetricRandomWalkProposal(proposal, dim=None):
    return RandomWalkProposal(proposal, True, dim)


class StaticProposal:
    """StaticProposal(dist) -- src/proposal.jl:9-11: every candidate is a fresh draw from `dist`, whatever the
    current state (independence sampler); the acceptance ratio carries logpdf(dist, x) - logpdf(dist, y)
    (src/proposal.jl:66-83).  `dist`: Normal / list of Normals / MvNormal, or a univariate of a device family / a list mixing them
    with Normals (README.md:106: StaticProposal([Normal(0, 1), InverseGamma(2, 3)])), or a function of the state that returns
    such (src/proposal.jl:92-126, `StaticProposal(lambda x: Normal(x, 1), dim=1)`): the ratio is then
    q(x | y) - q(y | x) (:120-126), left out when `issymmetric` (StaticProposal{true}, :196)."""

    def __init__(self, proposal, dim=None, issymmetric=False):
        self.proposal = _as_proposal(proposal, dim)
        self.issymmetric = bool(issymmetric)
        if self.issymmetric and not isinstance(self.proposal, ConditionalProposal):
            raise L.ArgumentError(L.MHX_EINVAL, "StaticProposal{true}: a static proposal is declared symmetric only as a function of the "
                                  "state (a fixed distribution's ratio q(x) - q(y) is always formed)")


def SymmetricStaticProposal(proposal, dim=None):
    """SymmetricStaticProposal(f) = StaticProposal{true}(f) -- src/proposal.jl:11, test/runtests.jl:244."""
    return StaticProposal(proposal, dim, True)


class MetropolisHastings:
    """MetropolisHastings(proposal) -- src/mh-core.jl:44-46.  `proposal`: a RandomWalkProposal / StaticProposal, or -- the
    reference's NamedTuple of proposals, test/runtests.jl:136-160, :187-189 -- a dict {name: proposal} of scalar proposals
    of ONE kind (all random-walk or all static; Normal or any other device family); its keys name the parameters
    (src/AdvancedMH.jl:96-104)."""

    def __init__(self, proposal, adapt=None):
        """adapt: a ProposalAdaptation -- every chain tunes its own proposal during the first adapt.steps transitions
        (mhx_rwmh_create_adaptive); only for a zero-mean isotropic or diagonal MvNormal random walk."""
        self.param_names = None
        self.adapt = None
        if adapt is not None:
            if not isinstance(adapt, ProposalAdaptation):
                raise L.ArgumentError(L.MHX_EINVAL, "MetropolisHastings: adapt must be a ProposalAdaptation or None")
            self.__init__(proposal)
            mv = self.proposal.proposal
            if not isinstance(self.proposal, RandomWalkProposal) or not isinstance(mv, MvNormal) or \
                    mv.kind not in (L.PROP_ISO, L.PROP_DIAG) or np.any(mv.mean != 0):
                raise L.ArgumentError(L.MHX_EINVAL, "MetropolisHastings: adapt is for a random walk over a zero-mean isotropic or diagonal "
                                      "MvNormal (dense, drifting, static, family, function and composite proposals do not adapt)")
            self.adapt = adapt
            return
        if isinstance(proposal, (list, tuple, NamedProposals)):
            # the reference's Array{Proposal} / NamedTuple{Proposal} in full (src/proposal.jl:128-175): entries that are all scalar,
            # constant and of one kind fold exactly as the mapping form below does; anything else is a composite run
            named = isinstance(proposal, NamedProposals)
            labels = list(proposal.entries) if named else list(range(1, len(proposal) + 1))
            parts = list(proposal.entries.values()) if named else list(proposal)
            if not parts:
                raise L.ArgumentError(L.MHX_EINVAL, "MetropolisHastings: empty proposal")
            for label, q in zip(labels, parts):
                if not isinstance(q, (RandomWalkProposal, StaticProposal)):
                    raise L.ArgumentError(L.MHX_EINVAL, "entry %r of a list of proposals / NamedProposals is %r, not a RandomWalkProposal or a "
                                          "StaticProposal" % (label, q))
            folds = len({type(q) for q in parts}) == 1 and all(
                not isinstance(q.proposal, ConditionalProposal) and q.proposal.dim == 1 for q in parts)
            if folds:
                proposal = {str(k): q for k, q in zip(labels, parts)}
            else:
                comp = CompositeProposal(labels, parts, named)
                self.param_names = comp.param_names
                self.proposal = comp
                return
            if not named:
                self.__init__(proposal)
                self.param_names = None
                return
        if isinstance(proposal, dict):
            if not proposal:
                raise L.ArgumentError(L.MHX_EINVAL, "MetropolisHastings: empty proposal")
            kinds = {type(p) for p in proposal.values()}
            if kinds not in ({RandomWalkProposal}, {StaticProposal}):
                raise L.ArgumentError(L.MHX_EINVAL, "a NamedTuple of proposals is lowered when every entry is a RandomWalkProposal or "
                                      "every entry is a StaticProposal (mixed kinds stay on the CPU reference)")
            parts = list(proposal.values())
            if any(isinstance(q.proposal, ConditionalProposal) for q in parts):
                raise L.ArgumentError(L.MHX_EINVAL, "a NamedTuple of function proposals is not lowered: give one function of the whole "
                                      "state that returns the list of components")
            if any(q.proposal.dim != 1 for q in parts):
                raise L.ArgumentError(L.MHX_EINVAL, "a NamedTuple of proposals takes one scalar Normal per name")
            if any(isinstance(q.proposal, ComponentProposal) for q in parts):
                # a name with a non-Normal scalar proposal (test/runtests.jl:189): the component vector, Normals by their (mu, sigma)
                mv = ComponentProposal([q.proposal.comps[0] if isinstance(q.proposal, ComponentProposal) else
                                        Normal(float(q.proposal.mean[0]), float(q.proposal.vec[0]) if q.proposal.kind == L.PROP_DIAG else q.proposal.scale)
                                        for q in parts])
            else:
                mv = MvNormal([float(q.proposal.mean[0]) for q in parts],
                              np.array([float(q.proposal.vec[0]) ** 2 if q.proposal.kind == L.PROP_DIAG else q.proposal.scale ** 2 for q in parts]))
            self.param_names = [str(k) for k in proposal]
            if kinds == {StaticProposal}:
                proposal = StaticProposal(mv)
            else:
                proposal = RandomWalkProposal(mv, all(q.issymmetric for q in parts))
        if not isinstance(proposal, (RandomWalkProposal, StaticProposal)):
            raise L.ArgumentError(L.MHX_EINVAL, "the GPU path implements RandomWalkProposal and StaticProposal "
                                  "over (Mv)Normal distributions, vectors of univariate components and functions of the state "
                                  "that return such components")
        self.proposal = proposal


def StaticMH(d):
    """StaticMH(d) -- src/mh-core.jl:48."""
    return MetropolisHastings(StaticProposal(d))


def RWMH(d, adapt=None):
    """RWMH(d) / RWMH(d::Int) -- src/mh-core.jl:50-51.  adapt: a ProposalAdaptation (see MetropolisHastings)."""
    return MetropolisHastings(RandomWalkProposal(d), adapt=adapt)


class ProposalAdaptation:
    """ProposalAdaptation(steps, target_rate=0.234, c=1.0, kappa=0.6, shape=False, lam_min=None, lam_max=None) -- how the chains of an
    RWMH sampler tune their own proposal during the first `steps` transitions (mhx_proposal_adapt_cfg): after
    transition t the chain's log-scale moves by min(1, c * t^(-kappa)) * (min(1, accept ratio) - target_rate), clamped to
    [lam_min, lam_max] (None: the library's defaults, -20 and 20); shape=True: the per-coordinate standard deviations follow the
    chain's own running variance as well.  Afterwards the proposal is frozen and the chain is a plain random walk."""

    def __init__(self, steps, target_rate=0.234, c=1.0, kappa=0.6, shape=False, lam_min=None, lam_max=None):
        self.steps, self.target_rate, self.c, self.kappa = int(steps), float(target_rate), float(c), float(kappa)
        self.shape = bool(shape)
        self.lam_min = None if lam_min is None else float(lam_min)
        self.lam_max = None if lam_max is None else float(lam_max)
        if self.steps < 0:
            raise L.ArgumentError(L.MHX_EINVAL, "ProposalAdaptation: steps = %d must not be negative" % self.steps)
        if not (0.5 < self.kappa <= 1.0):
            raise L.ArgumentError(L.MHX_EINVAL, "ProposalAdaptation: kappa = %g outside (0.5, 1]" % self.kappa)
        if not (self.c >= 0.0 and np.isfinite(self.c)):
            raise L.ArgumentError(L.MHX_EINVAL, "ProposalAdaptation: c = %g must be finite and not negative" % self.c)
        if not (0.0 < self.target_rate < 1.0):
            raise L.ArgumentError(L.MHX_EINVAL, "ProposalAdaptation: target_rate = %g outside (0, 1)" % self.target_rate)
        if self.lam_min is not None and self.lam_max is not None and not (self.lam_min <= self.lam_max):
            raise L.ArgumentError(L.MHX_EINVAL, "ProposalAdaptation: lam_min = %g > lam_max = %g" % (self.lam_min, self.lam_max))

    def cfg(self):
        nan = float("nan")
        return L.ProposalAdaptCfg(self.steps, 1 if self.shape else 0, self.target_rate, self.c, self.kappa,
                                  nan if self.lam_min is None else self.lam_min, nan if self.lam_max is None else self.lam_max)


class AdaptationTable(list):
    """chain.adaptation of an adaptive run: one row {parameter, sd_median, sd_min, sd_max} per parameter -- the frozen proposal's
    standard deviations over the chains -- with `lam_median`, the median log-scale, and `accept_rate`, the pooled acceptance rate of
    the frozen phase (NaN: no frozen transition yet), as attributes"""
    lam_median = float("nan")
    accept_rate = float("nan")

    def __str__(self):
        out = ["parameter         sd median         min         max"]
        for w in self:
            out.append("%-12s %14.5g %11.5g %11.5g" % (w["parameter"], w["sd_median"], w["sd_min"], w["sd_max"]))
        out.append("median log-scale %.4f, acceptance rate of the frozen phase %.3f" % (self.lam_median, self.accept_rate))
        return "\n".join(out)

    __repr__ = __str__


def geometric_betas(R, beta_min):
    """The usual ladder of parallel tempering: R inverse temperatures 1 = beta_0 > ... > beta_{R-1} = beta_min in geometric
    progression, beta_r = beta_min^(r / (R - 1)) (doubles; beta_0 is exactly 1)."""
    R = int(R)
    if R < 2 or not (0.0 < float(beta_min) < 1.0):
        raise L.ArgumentError(L.MHX_EINVAL, "geometric_betas: R >= 2 rungs and 0 < beta_min < 1")
    b = np.array([float(beta_min) ** (r / (R - 1.0)) for r in range(R)], dtype=np.float64)
    b[0], b[-1] = 1.0, float(beta_min)
    return b


def power_betas(R, p=3.0):
    """The usual ladder of thermodynamic integration: beta_r = ((R - 1 - r) / (R - 1))^p, from beta_0 exactly 1 to beta_{R-1} exactly 0,
    dense near 0 where E_beta[u] changes fastest.  For an anchored ladder (Tempered(..., reference=...)); give `scales` with it."""
    R = int(R)
    if R < 2 or not (float(p) > 0.0 and math.isfinite(float(p))):
        raise L.ArgumentError(L.MHX_EINVAL, "power_betas: R >= 2 rungs and a finite p > 0")
    b = np.array([((R - 1.0 - r) / (R - 1.0)) ** float(p) for r in range(R)], dtype=np.float64)
    b[0], b[-1] = 1.0, 0.0
    return b


class LadderAdaptation:
    """LadderAdaptation(steps, target_rate=0.234, c=1.0, kappa=0.6, rho_min=None, rho_max=None) -- how the ladders of a Tempered
    sampler tune their temperatures during the first `steps` transitions (mhx_ladder_adapt_cfg): after swap
    round s every attempted pair moves rho, the log of its gap in log beta, by c * s^(-kappa) * (min(1, swap ratio) - target_rate),
    clamped to [rho_min, rho_max] (None: the library's defaults, -10 and log(16 / (R - 1))).  What the library would refuse on every
    ladder is refused here; the limit on rho_max depends on R and is the library's."""

    def __init__(self, steps, target_rate=0.234, c=1.0, kappa=0.6, rho_min=None, rho_max=None):
        self.steps, self.target_rate, self.c, self.kappa = int(steps), float(target_rate), float(c), float(kappa)
        self.rho_min = None if rho_min is None else float(rho_min)
        self.rho_max = None if rho_max is None else float(rho_max)
        if self.steps < 0:
            raise L.ArgumentError(L.MHX_EINVAL, "LadderAdaptation: steps = %d must not be negative" % self.steps)
        if not (0.5 < self.kappa <= 1.0):
            raise L.ArgumentError(L.MHX_EINVAL, "LadderAdaptation: kappa = %g outside (0.5, 1]" % self.kappa)
        if not (self.c >= 0.0 and np.isfinite(self.c)):
            raise L.ArgumentError(L.MHX_EINVAL, "LadderAdaptation: c = %g must be finite and not negative" % self.c)
        if not (0.0 < self.target_rate < 1.0):
            raise L.ArgumentError(L.MHX_EINVAL, "LadderAdaptation: target_rate = %g outside (0, 1)" % self.target_rate)
        if self.rho_min is not None and self.rho_max is not None and not (self.rho_min <= self.rho_max):
            raise L.ArgumentError(L.MHX_EINVAL, "LadderAdaptation: rho_min = %g > rho_max = %g" % (self.rho_min, self.rho_max))

    def cfg(self):
        nan = float("nan")
        return L.LadderAdaptCfg(self.steps, self.target_rate, self.c, self.kappa, nan if self.rho_min is None else self.rho_min,
                                nan if self.rho_max is None else self.rho_max)


class Tempered:
    """Tempered(sampler, betas, swap_every=1, scales=None, adapt=None, reference=None) -- parallel tempering (replica exchange) around a random-walk
    sampler, what MCMCTempering.jl wraps around AdvancedMH's samplers and emcee shipped as PTSampler.  `sampler`: an RWMH over an
    isotropic or diagonal zero-mean MvNormal.  `betas`: the ladder, betas[0] == 1, strictly decreasing, a power of two of rungs (2..64).
    Rung r samples target^betas[r] with the proposal scaled by scales[r] (default betas[r]^(-1/2)); after every swap_every-th transition
    neighbouring rungs may exchange their states.  `adapt`: a LadderAdaptation -- `betas` is then where every ladder starts and each
    tunes its own temperatures from its own swaps (no `scales`: they follow the ladder).  `reference`: an MvNormal(mean, diagonal
    variances) q -- the ladder is ANCHORED: rung r samples target^beta q^(1 - beta), the last beta may be
    exactly 0 (then `scales` must be given) and `chain.tempered.evidence()` is the log marginal likelihood.  At beta = 0 the rung samples
    q restricted to the target's support.  Fixed ladders only.
    `sample(model, Tempered(...), N, nladders)` returns the nladders cold chains."""

    def __init__(self, sampler, betas, swap_every=1, scales=None, adapt=None, reference=None):
        if not isinstance(sampler, MetropolisHastings) or not isinstance(sampler.proposal, RandomWalkProposal) or \
                not isinstance(sampler.proposal.proposal, MvNormal):
            raise L.ArgumentError(L.MHX_EINVAL, "Tempered wraps an RWMH sampler over an isotropic or diagonal MvNormal")
        if getattr(sampler, "adapt", None) is not None:
            raise L.ArgumentError(L.MHX_EINVAL, "Tempered: the wrapped sampler adapts its proposal (ProposalAdaptation), which a tempered run does not")
        self.sampler = sampler
        self.proposal = sampler.proposal                     # (what Run.init looks at)
        self.param_names = sampler.param_names
        self.betas = np.ascontiguousarray(betas, dtype=np.float64).ravel()
        self.R = int(self.betas.size)
        self.swap_every = int(swap_every)
        self.scales = None if scales is None else np.ascontiguousarray(scales, dtype=np.float64).ravel()
        if self.scales is not None and self.scales.size != self.R:
            raise L.ArgumentError(L.MHX_EINVAL, "Tempered: %d scales for %d betas" % (self.scales.size, self.R))
        if adapt is not None and not isinstance(adapt, LadderAdaptation):
            raise L.ArgumentError(L.MHX_EINVAL, "Tempered: adapt must be a LadderAdaptation or None")
        if adapt is not None and self.scales is not None:
            raise L.ArgumentError(L.MHX_EINVAL, "Tempered: scales with adapt -- the proposal scales of an adaptive ladder follow its temperatures")
        if adapt is not None and self.swap_every == 0:
            raise L.ArgumentError(L.MHX_EINVAL, "Tempered: swap_every = 0 with adapt -- an adaptive ladder tunes itself from its swap rounds")
        self.adapt = adapt
        self.reference = reference
        self.ref_mean = self.ref_sd = None
        if reference is not None:
            if adapt is not None:
                raise L.ArgumentError(L.MHX_EINVAL, "Tempered: reference with adapt -- an adaptive ladder moves in log beta, which cannot reach "
                                      "0: an anchored ladder is a fixed ladder")
            if not isinstance(reference, MvNormal) or reference.kind == L.PROP_DENSE:
                raise L.ArgumentError(L.MHX_EINVAL, "Tempered: reference must be an MvNormal with an isotropic or a diagonal covariance (a dense "
                                      "reference is not supported)")
            self.ref_mean = np.ascontiguousarray(reference.mean, dtype=np.float64).ravel()
            self.ref_sd = np.full(reference.dim, reference.scale, dtype=np.float64) if reference.kind == L.PROP_ISO else \
                np.ascontiguousarray(reference.vec, dtype=np.float64).ravel()
            if not (np.isfinite(self.ref_mean).all() and np.isfinite(self.ref_sd).all() and (self.ref_sd > 0).all()):
                raise L.ArgumentError(L.MHX_EINVAL, "Tempered: the reference needs a finite mean and finite positive variances")
        zero = np.flatnonzero(self.betas == 0.0)
        if zero.size and reference is not None:
            if zero[0] != self.R - 1:
                raise L.ArgumentError(L.MHX_EINVAL, "Tempered: betas[%d] = 0 is not the last rung -- only the last inverse temperature of an "
                                      "anchored ladder may be 0" % zero[0])
            if self.scales is None:
                raise L.ArgumentError(L.MHX_EINVAL, "Tempered: betas[%d] = 0 without scales -- the default proposal scale beta^(-1/2) has no "
                                      "value there: give scales" % zero[0])


class EvidenceResult(dict):
    """what Run.evidence returns: dict(rungs, log_z_ti, log_z_ti_coarse, log_z_ss, log_z_ss_backward, se_ti, se_ss, se_ss_backward, bad,
    nladders, n_saved) that prints.  rungs: one row {rung, beta, n, mean_u, var_u} per rung, u = log target - log reference."""

    def __str__(self):
        out = ["log Z   stepping stone %.5f (se %.5f)   backward %.5f (se %.5f)" % (self["log_z_ss"], self["se_ss"], self["log_z_ss_backward"],
                                                                                   self["se_ss_backward"]),
               "        thermodynamic integration %.5f (se %.5f)   every other rung %.5f" % (self["log_z_ti"], self["se_ti"],
                                                                                           self["log_z_ti_coarse"]),
               "        %d ladders, %d saved draws per chain, %d draws left out" % (self["nladders"], self["n_saved"], self["bad"]),
               "rung        beta         n        mean u         var u"]
        for w in self["rungs"]:
            out.append("%4d %11.5g %9d %13.5f %13.5f" % (w["rung"], w["beta"], w["n"], w["mean_u"], w["var_u"]))
        return "\n".join(out)

    __repr__ = __str__


def _lse_pool(mx, se):
    """log sum exp of chains given as (max, sum exp(. - max)) pairs"""
    m = float(np.max(mx))
    if not math.isfinite(m):
        return m if m < 0 else math.nan
    return m + math.log(float(np.sum(se * np.exp(mx - m))))


def evidence_from_table(table, betas, n_saved):
    """The log evidence from the per-chain table [nladders * R][8] of mhx_run_evidence (bad, shift, s1, s2, max_f, sumexp_f, max_b,
    sumexp_b), the ladder's betas [R] as the run holds them and the draws per chain, all in float64 on the host:
    log_z_ti  the trapezoid over beta of the rung means of u;  log_z_ti_coarse  the same rule on rungs 0, 2, 4, .. and the last (NaN for
    R = 2): their difference is the discretisation error's size;  log_z_ss = sum_r log mean exp(dbeta[r] u) over rung r + 1;
    log_z_ss_backward = -sum_r log mean exp(-dbeta[r] u) over rung r;  se_*: the standard deviation of the per-ladder estimates over
    sqrt(nladders) (NaN with one ladder)."""
    betas = np.asarray(betas, dtype=np.float64).ravel()
    R = betas.size
    t = np.asarray(table, dtype=np.float64).reshape(-1, R, 8)
    nl = t.shape[0]
    with np.errstate(all="ignore"):
        n = float(n_saved) - t[:, :, 0]                              # [nl][R] draws that count
        mean_c = t[:, :, 1] + t[:, :, 2] / n                         # per chain
        m2_c = t[:, :, 3] - t[:, :, 2] * t[:, :, 2] / n
        ntot = n.sum(axis=0)
        mean = (n * mean_c).sum(axis=0) / ntot
        var = (m2_c.sum(axis=0) + (n * (mean_c - mean) ** 2).sum(axis=0)) / (ntot - 1.0)

        def trapezoid(m, idx):
            idx = np.asarray(idx)
            return ((betas[idx[:-1]] - betas[idx[1:]]) * 0.5 * (m[..., idx[:-1]] + m[..., idx[1:]])).sum(axis=-1)
        full = np.arange(R)
        coarse = np.concatenate([np.arange(0, R - 1, 2), [R - 1]])
        lf = t[:, :, 4] + np.log(t[:, :, 5] / n)                     # per chain: log mean exp(dbeta[r - 1] u)
        lb = t[:, :, 6] + np.log(t[:, :, 7] / n)
        ss_l, ssb_l, ti_l = lf[:, 1:].sum(axis=1), -lb[:, :-1].sum(axis=1), trapezoid(mean_c, full)
        ss = sum(_lse_pool(t[:, r, 4], t[:, r, 5]) - math.log(ntot[r]) for r in range(1, R))
        ssb = -sum(_lse_pool(t[:, r, 6], t[:, r, 7]) - math.log(ntot[r]) for r in range(R - 1))

        def se(v):
            return float(np.std(v, ddof=1) / math.sqrt(nl)) if nl > 1 else math.nan
        return EvidenceResult(rungs=[dict(rung=r, beta=float(betas[r]), n=int(ntot[r]), mean_u=float(mean[r]), var_u=float(var[r])) for r in range(R)],
                              log_z_ti=float(trapezoid(mean, full)), log_z_ti_coarse=float(trapezoid(mean, coarse)) if R > 2 else math.nan,
                              log_z_ss=float(ss), log_z_ss_backward=float(ssb), se_ti=se(ti_l), se_ss=se(ss_l), se_ss_backward=se(ssb_l),
                              bad=int(t[:, :, 0].sum()), nladders=int(nl), n_saved=int(n_saved))


def bayes_factor(a, b):
    """log Bayes factor of two EvidenceResults, model a over model b: the difference of their log_z_ss and the combined standard error"""
    return dict(log_bf=a["log_z_ss"] - b["log_z_ss"], se=math.hypot(a["se_ss"], b["se_ss"]))


class LadderTable(list):
    """ladder() of a tempered run: one row {rung, beta_median, beta_min, beta_max, rate} per rung -- the temperature over the ladders
    and the swap rate of the pair (rung, rung + 1) (NaN for the last rung)"""

    def __str__(self):
        out = ["rung   beta median         min         max  swap rate"]
        for w in self:
            out.append("%4d %13.5g %11.5g %11.5g %10.3f" % (w["rung"], w["beta_median"], w["beta_min"], w["beta_max"], w["rate"]))
        return "\n".join(out)

    __repr__ = __str__


class SwapTable(list):
    """swap_rates() of a tempered run: one row {pair, beta_lo, beta_hi, attempts, swaps, rate} per pair of neighbouring rungs (an
    adaptive run: the betas are the medians over the ladders)"""

    def __str__(self):
        out = ["pair     beta_r    beta_r+1    attempts       swaps    rate"]
        for w in self:
            out.append("%2d-%-2d %9.4g %11.4g %11d %11d %7.3f" % (w["pair"][0], w["pair"][1], w["beta_lo"], w["beta_hi"], w["attempts"],
                                                               w["swaps"], w["rate"]))
        return "\n".join(out)

    __repr__ = __str__


class StretchProposal:
    """StretchProposal(prior, a = 2.0) -- src/emcee.jl:63-68."""

    def __init__(self, proposal, stretch_length=2.0):
        self.proposal, self.stretch_length = proposal, float(stretch_length)

    def rand_initial(self, rng):
        p = self.proposal
        if isinstance(p, (list, tuple)):
            return np.array([q.rand(rng) for q in p])
        return np.asarray(p.rand(rng))


class Ensemble:
    """Ensemble(n_walkers, proposal) -- src/emcee.jl:1-4."""

    def __init__(self, n_walkers, proposal):
        if not isinstance(proposal, StretchProposal):
            raise L.ArgumentError(L.MHX_EINVAL, "Ensemble: only StretchProposal is implemented (as in the reference)")
        self.n_walkers, self.proposal = int(n_walkers), proposal


class RobustAdaptiveMetropolis:
    """RobustAdaptiveMetropolis(; α=0.234, γ=0.6, S=nothing, eigenvalue_lower_bound=0, eigenvalue_upper_bound=Inf)
    -- src/RobustAdaptiveMetropolis.jl:75-87."""

    def __init__(self, α=0.234, γ=0.6, S=None, eigenvalue_lower_bound=0.0, eigenvalue_upper_bound=float("inf"),
                 alpha=None, gamma=None, deferred_factor=False):
        """deferred_factor=True: MHX_FLAG_RAM_DEFERRED (dim <= 256) -- up to 8 rank-one updates stay pending as O(dim) triples and
        are folded into S in one pass: the same chain in exact arithmetic, its own rounding (include/mhx.h)."""
        self.deferred_factor = bool(deferred_factor)
        self.α = float(alpha if alpha is not None else α)
        self.γ = float(gamma if gamma is not None else γ)
        self.S = None if S is None else np.asarray(S, dtype=np.float64)
        self.eigenvalue_lower_bound = float(eigenvalue_lower_bound)
        self.eigenvalue_upper_bound = float(eigenvalue_upper_bound)


class MALA:
    """MALA(sigma2), or the reference's own form `MALA(g -> MvNormal((sigma2 / 2) .* g, sigma2 * I))` (src/MALA.jl:1-11,
    test/runtests.jl:291,352) as a Python callable of the gradient: the callable is probed once the dimension is known and
    must be that Langevin proposal -- mean (sigma2 / 2) g, covariance sigma2 I; any other gradient -> Distribution closure
    stays on the CPU reference."""

    def __init__(self, sigma2):
        self.closure = sigma2 if callable(sigma2) else None
        self.sigma2 = None if callable(sigma2) else float(sigma2)

    def resolve(self, d):
        """sigma2 of the Langevin proposal the closure describes (probed at g = 0, g = 1 and a ramp)."""
        if self.closure is None:
            return self.sigma2
        bad = L.ArgumentError(L.MHX_EINVAL, "MALA on the GPU path takes sigma2 or the Langevin closure g -> MvNormal((sigma2/2) g, sigma2 I); "
                              "this closure is not of that form and cannot be lowered")
        try:
            p0, p1, p2 = (_as_mvnormal(self.closure(g)) for g in (np.zeros(d), np.ones(d), np.arange(1.0, d + 1.0)))
        except L.ArgumentError:
            raise bad from None
        for q in (p0, p1, p2):
            iso = q.kind == L.PROP_ISO or (q.kind == L.PROP_DIAG and np.all(q.vec == q.vec[0]))
            if q.dim != d or not iso:
                raise bad
        s2 = (p0.scale if p0.kind == L.PROP_ISO else float(p0.vec[0])) ** 2
        same = all(abs((q.scale if q.kind == L.PROP_ISO else float(q.vec[0])) ** 2 - s2) <= 1e-12 * s2 for q in (p1, p2))
        if not (same and np.all(p0.mean == 0) and np.allclose(p1.mean, 0.5 * s2, rtol=1e-12, atol=0)
                and np.allclose(p2.mean, 0.5 * s2 * np.arange(1.0, d + 1.0), rtol=1e-12, atol=0)):
            raise bad
        return float(s2)


# ------------------------------------------------------------------------------------------------
# chains container (the part of MCMCChains.Chains the reference tests touch)


DEFAULT_QUANTILE_PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)        # the columns of MCMCChains' "Quantiles" table (README.md:65-71)


def quantile_ranks(S, probs):
    """(j, j1, g) of Julia's `quantile` / numpy's default ("type 7"): h = (S - 1) p, j = floor(h), j1 = min(j + 1, S - 1),
    g = h - j; the quantile lies between the order statistics x_(j) and x_(j1).  p outside [0, 1] (or NaN) is refused."""
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    if int(S) < 1:
        raise L.ArgumentError(L.MHX_EINVAL, "quantiles: no draws")
    if probs.ndim != 1 or probs.size == 0 or not np.all((probs >= 0.0) & (probs <= 1.0)):
        raise L.ArgumentError(L.MHX_EINVAL, "quantiles: probs must lie in [0, 1]")
    h = (float(int(S)) - 1.0) * probs
    j = np.floor(h)
    g = h - j
    j = j.astype(np.int64)
    return j, np.minimum(j + 1, int(S) - 1), g


def quantiles_from_order_statistics(lo, hi, g, top=None):
    """Quantiles [..., nprobs] from the order statistics lo = x_(j), hi = x_(j1) and the weights g of quantile_ranks, in float64:
    lo where lo == hi (no arithmetic: infinities stay, no NaN), else lo + g (hi - lo).  `top` [...]: the largest draw x_(S-1);
    where it is NaN (NaNs order last, so the parameter holds one) every quantile of that row is NaN, as numpy's."""
    lo, hi, g = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64), np.asarray(g, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.where(lo == hi, lo, lo + g * (hi - lo))
    if top is not None:
        q = np.where(np.isnan(np.asarray(top, dtype=np.float64))[..., None], np.nan, q)
    return q


def _quantiles(order_statistics, S, probs, params):
    """quantiles through ONE order_statistics call: the ranks j and j + 1 of every prob and the top rank"""
    j, j1, g = quantile_ranks(S, probs)
    x = order_statistics(np.concatenate([j, j1, [int(S) - 1]]), params)
    n = len(j)
    return quantiles_from_order_statistics(x[:, :n], x[:, n:2 * n], g, top=x[:, 2 * n])


def hpd_ranks(S, alpha):
    """m = max(1, ceil(alpha S)), in float64 as the C side computes it (include/mhx.h: mhx_run_hpd): the HPD interval of S pooled
    draws is the narrowest [y[i], y[S - m + i]], i < m, of their ascending order y.  alpha outside (0, 1) (or NaN) is refused."""
    alpha = float(alpha)
    if int(S) < 1:
        raise L.ArgumentError(L.MHX_EINVAL, "hpd: no draws")
    if not (0.0 < alpha < 1.0):
        raise L.ArgumentError(L.MHX_EINVAL, "hpd: alpha must lie in (0, 1)")
    return max(1, int(math.ceil(alpha * float(int(S)))))


class HPDTable(dict):
    """what Chains.hpd returns: dict(parameters, alpha, lower [nparams], upper [nparams]) that prints in the style of the Quantiles table"""

    def __str__(self):
        lines = ["HPD (%g%%)" % (100.0 * (1.0 - self["alpha"])), "  parameters   " + " ".join("%9s" % c for c in ("lower", "upper"))]
        for i, n in enumerate(self["parameters"]):
            lines.append("  %-12s " % n + " ".join("%9.4f" % v for v in (self["lower"][i], self["upper"][i])))
        return "\n".join(lines)

    __repr__ = __str__


def covariance_from_moments(n, sum, cross):
    """The covariance matrix of n pooled draws from their moments about ANY common shift (Run.cross_moments): sum[i] = sum_k y_ik,
    cross[i][j] = sum_k y_ik y_jk  ->  (cross - sum sum^T / n) / (n - 1), in float64 on the host; what `np.cov` of the flattened
    chains gives.  Moments of shards taken about the same shift add before this call."""
    n = int(n)
    if n < 2:
        raise L.ArgumentError(L.MHX_EINVAL, "covariance_from_moments: a covariance needs n >= 2 draws, got %d" % n)
    s, x = np.asarray(sum, dtype=np.float64), np.asarray(cross, dtype=np.float64)
    if s.ndim != 1 or x.shape != (s.size, s.size):
        raise L.ArgumentError(L.MHX_EINVAL, "covariance_from_moments: sum must be [m] and cross [m][m]")
    with np.errstate(invalid="ignore", over="ignore"):
        return (x - np.outer(s, s) / float(n)) / float(n - 1)


def correlation_from_covariance(cov):
    """cov[i][j] / (sd_i sd_j) with the diagonal set to exactly 1 and the rest clamped to [-1, 1], as Julia's `cor` (cov2cor!) does;
    a row whose variance is not a positive finite number is NaN."""
    cov = np.asarray(cov, dtype=np.float64)
    var = np.diagonal(cov)
    ok = np.isfinite(var) & (var > 0.0)
    sd = np.sqrt(np.where(ok, var, np.nan))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        cor = np.clip(cov / np.outer(sd, sd), -1.0, 1.0)        # (one division by a symmetric product: symmetric bit for bit)
    cor[np.diag_indices_from(cor)] = np.where(ok, 1.0, np.nan)
    return cor


HISTOGRAM_MAX_BINS, HISTOGRAM2D_MAX_BINS = 2048, 128      # MHX_HIST_MAX_BINS / MHX_HIST2D_MAX_BINS of the library


def histogram_edges(lo, hi, bins):
    """The bins + 1 float64 edges numpy itself uses for `np.histogram(x, bins, range=(lo, hi))`:
    np.histogram_bin_edges([], bins, (lo, hi)), its widening of lo == hi to (lo - 0.5, hi + 0.5) included."""
    try:
        bins, lo, hi = int(bins), float(lo), float(hi)
    except (TypeError, ValueError):
        raise L.ArgumentError(L.MHX_EINVAL, "histogram_edges: bins must be an integer and lo, hi numbers")
    if bins < 1:
        raise L.ArgumentError(L.MHX_EINVAL, "histogram_edges: bins = %d must be at least 1" % bins)
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
        raise L.ArgumentError(L.MHX_EINVAL, "histogram_edges: the range (%r, %r) must be finite and non-decreasing" % (lo, hi))
    return np.histogram_bin_edges(np.empty(0, dtype=np.float64), bins, (lo, hi))


def _histogram_edges(owner, idx, bins, range, edges, what):
    """[m][bins + 1] float64 edges of a histogram call on a Run or Group: `edges` passed through (one set, or one per row), else
    numpy's edges of `range` (one (lo, hi), or one per row), else of every row's own minimum and maximum -- ONE order_statistics call
    for ranks 0 and S - 1.  A NaN or infinite end is refused with the row's index (numpy raises ValueError there)."""
    m = len(idx)
    if edges is not None:
        e = np.array(edges, dtype=np.float64, ndmin=1)
        if e.ndim == 1:
            e = np.tile(e, (m, 1))
        if e.ndim != 2 or e.shape[0] != m or e.shape[1] < 2:
            raise L.ArgumentError(L.MHX_EINVAL, "%s: edges must be [bins + 1] or [%d][bins + 1]" % (what, m))
        return np.ascontiguousarray(e)
    if range is None:
        S = owner._n_draws()
        if S < 1:
            owner.order_statistics([0], idx)                # raises the library's refusal (no device sample tensor)
        ends = owner.order_statistics([0, S - 1], idx)
    else:
        ends = np.array(range, dtype=np.float64)
        if ends.shape == (2,):
            ends = np.tile(ends, (m, 1))
        if ends.shape != (m, 2):
            raise L.ArgumentError(L.MHX_EINVAL, "%s: range must be (lo, hi) or one (lo, hi) per row, [%d][2]" % (what, m))
    for k in np.arange(m):
        if not np.all(np.isfinite(ends[k])):
            raise L.ArgumentError(L.MHX_EINVAL, "%s: the range of row %d, (%r, %r), is not finite%s" % (
                what, int(idx[k]), float(ends[k, 0]), float(ends[k, 1]), " (the row holds such draws: give a range)" if range is None else ""))
    if m == 0:
        return np.empty((0, int(bins) + 1))
    return np.ascontiguousarray(np.stack([histogram_edges(lo, hi, bins) for lo, hi in ends]))


def _all_pairs(m):
    """every i < j of m slots, [m (m - 1) / 2][2] int32"""
    i, j = np.triu_indices(int(m), 1)
    return np.ascontiguousarray(np.stack([i, j], axis=1), dtype=np.int32)


def _histogram_call(fn, handle, idx, e, pairs=None):
    """one mhx_*_histogram (pairs None) or mhx_*_histogram2d call: (counts, outside) as int64"""
    m, B = len(idx), e.shape[1] - 1
    i32p, u64p = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    if pairs is None:
        counts, outside = np.zeros((m, B), dtype=np.uint64), np.zeros((m, 3), dtype=np.uint64)
        rc = fn(handle, idx.ctypes.data_as(i32p), m, e.ctypes.data_as(C.POINTER(C.c_double)), B, counts.ctypes.data_as(u64p),
                outside.ctypes.data_as(u64p))
    else:
        counts, outside = np.zeros((len(pairs), B, B), dtype=np.uint64), np.zeros(len(pairs), dtype=np.uint64)
        rc = fn(handle, idx.ctypes.data_as(i32p), m, e.ctypes.data_as(C.POINTER(C.c_double)), B, pairs.ctypes.data_as(i32p), len(pairs),
                counts.ctypes.data_as(u64p), outside.ctypes.data_as(u64p))
    L.check(rc)
    return counts.view(np.int64), outside.view(np.int64)


def _histogram(owner, fn, bins, range, params, edges):
    idx = owner._rows(params)
    e = _histogram_edges(owner, idx, bins, range, edges, "histogram")
    counts, outside = _histogram_call(fn, owner.h, idx, e)
    return counts, e, outside


def _histogram2d(owner, fn, params, pairs, bins, range, edges):
    idx = owner._rows(params)
    pr = _all_pairs(len(idx)) if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    e = _histogram_edges(owner, idx, bins, range, edges, "histogram2d")
    counts, outside = _histogram_call(fn, owner.h, idx, e, pr)
    return counts, e, outside, pr


def silverman_bandwidth(std, q25, q75, S):
    """Silverman's rule as KernelDensity.jl's default applies it: 0.9 min(std, IQR / 1.34) S^(-1/5); where that minimum is 0 the std
    takes its place, and 1 where the std is 0 as well (or there is a single draw)."""
    width = min(float(std), (float(q75) - float(q25)) / 1.34) if int(S) > 1 else 0.0
    if width == 0.0:
        width = float(std) if int(S) > 1 and float(std) != 0.0 else 1.0
    return 0.9 * width * float(int(S)) ** -0.2


def density_from_counts(counts, edges, h):
    """(x, density): the Gaussian kernel density estimate of bandwidth h of draws that were binned to `counts` over `edges`, every
    draw standing at its bin's centre: x[k] = the centres, density[k] = sum_j counts[j] phi_h(x[k] - x[j]) / sum(counts), a direct
    sum in float64.  Every draw moved by at most half a cell delta / 2, so
    |density[k] - the exact estimate at x[k]| <= (delta / 2) max|phi_h'| = delta / (2 h^2 sqrt(2 pi e))."""
    counts, edges, h = np.asarray(counts, dtype=np.float64), np.asarray(edges, dtype=np.float64), float(h)
    x = 0.5 * (edges[:-1] + edges[1:])
    nz = np.flatnonzero(counts)
    z = (x[:, None] - x[None, nz]) / h
    dens = (np.exp(-0.5 * z * z) @ counts[nz]) / (counts.sum() * h * math.sqrt(2.0 * math.pi))
    return x, dens


def density_binning_bound(edges, h):
    """the bound of density_from_counts for uniform edges"""
    delta = (float(edges[-1]) - float(edges[0])) / (len(edges) - 1)
    return delta / (2.0 * float(h) ** 2 * math.sqrt(2.0 * math.pi * math.e))


class Corner:
    """what Chains.corner returns: the numbers of a corner plot.  names [m]; edges[name] [bins + 1]; marginal[name] int64 [bins];
    joint[(a, b)] int64 [bins][bins] for every a before b in names, cell [bin of a][bin of b]; outside[name] / outside[(a, b)]:
    the draws a histogram left out (none for a row of finite draws: the edges span each row's minimum and maximum)."""

    def __init__(self, names, edges, marginal, joint, outside):
        self.names, self.edges, self.marginal, self.joint, self.outside = list(names), edges, marginal, joint, outside

    def __repr__(self):
        bins = len(next(iter(self.edges.values()))) - 1 if self.edges else 0
        lines = ["Corner (%d parameters, %d bins): %d marginal [%d], %d joint [%d][%d]" % (
            len(self.names), bins, len(self.marginal), bins, len(self.joint), bins, bins)]
        for n in self.names:
            lines.append("  %-12s [%.4g, %.4g]  %d draws" % (n, self.edges[n][0], self.edges[n][-1], int(self.marginal[n].sum())))
        for (a, b), H in self.joint.items():
            lines.append("  %-12s %d draws" % ("%s x %s" % (a, b), int(H.sum())))
        return "\n".join(lines)

    __str__ = __repr__


ACF_TILE = {"f64": 16, "f32": 8}                            # MHX_ACF_R of the library: the lags of a tile, per width


def _autocovariance(owner, fn, lags, params, chains, normalise):
    """one mhx_*_autocovariance call of a Run (chains: (begin, count), None = all) or a Group (chains False): (acov, nvalid)"""
    idx = owner._rows(params)
    lg = np.ascontiguousarray(np.atleast_1d(lags), dtype=np.int64).reshape(-1)
    if lg.size and (lg.min() < -2 ** 31 or lg.max() >= 2 ** 31):
        raise L.ArgumentError(L.MHX_EINVAL, "autocovariance: a lag does not fit 32 bits")
    lg = lg.astype(np.int32)
    acov = np.full((len(idx), len(lg)), np.nan, dtype=np.float64)
    nvalid = np.zeros(len(idx), dtype=np.int64)
    i32p = C.POINTER(C.c_int32)
    args = [idx.ctypes.data_as(i32p), len(idx), lg.ctypes.data_as(i32p), len(lg)]
    if chains is not False:                                 # False: the group form, which takes no range
        args += [0, 0] if chains is None else [int(chains[0]), int(chains[1])]
    L.check(fn(owner.h, *args, 1 if normalise else 0, acov.ctypes.data_as(C.POINTER(C.c_double)),
               nvalid.ctypes.data_as(C.POINTER(C.c_int64))))
    return acov, nvalid


def autocorrelation(acov):
    """rho(k) = acov[..., k] / acov[..., 0] in float64, for sums over lags that start at lag 0 (either mode of
    Run.autocovariance: un-normalised, the ratio of the pooled sums; normalised, the mean over the valid chains of each chain's own
    autocorrelation, since acov[0] is then their number).  A row whose acov[0] is not positive (no chain with variance, or NaN) is
    NaN."""
    a = np.asarray(acov, dtype=np.float64)
    a0 = a[..., :1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.where(a0 > 0.0, a / np.where(a0 > 0.0, a0, 1.0), np.nan)


def integrated_time(rho, c=5.0):
    """(tau, M, truncated) of ONE autocorrelation function rho over lags 0..K: taus = 2 cumsum(rho) - 1, the window M the first
    index with M >= c taus[M] (Sokal's automatic windowing, emcee's `auto_window`), tau = taus[M].  No such index: M = K and
    truncated = True -- the series is too short for this c.  A rho that holds a NaN gives (NaN, K, True)."""
    r = np.asarray(rho, dtype=np.float64).reshape(-1)
    if r.size < 1:
        raise L.ArgumentError(L.MHX_EINVAL, "integrated_time: rho is empty")
    taus = 2.0 * np.cumsum(r) - 1.0
    with np.errstate(invalid="ignore"):
        ok = np.flatnonzero(np.arange(r.size) >= float(c) * taus)
    if ok.size == 0 or not np.isfinite(taus).all():
        return float(taus[-1]), r.size - 1, True
    M = int(ok[0])
    return float(taus[M]), M, False


class AutocorTable(dict):
    """what Chains.autocor returns: dict(parameters, lags, autocor [nparams][nlags]) that prints as MCMCChains' Autocorrelation table"""

    def __str__(self):
        lines = ["Autocorrelation", "  parameters   " + " ".join("%9s" % ("lag %d" % k) for k in self["lags"])]
        for i, n in enumerate(self["parameters"]):
            lines.append("  %-12s " % n + " ".join("%9.4f" % v for v in self["autocor"][i]))
        return "\n".join(lines)

    __repr__ = __str__


def _check_moments(rc):
    """check() for the cross moments: asking a run that kept no sample tensor for them is an ArgumentError here (the C ABI says
    MHX_ESTATE, as for the order statistics)"""
    if rc == L.MHX_ESTATE:
        raise L.ArgumentError(rc, L.lib().mhx_last_error().decode("utf-8", "replace"))
    L.check(rc)


def _first_sample_mean(sums, nchains):
    """the default shift of the cross moments: the mean over the chains of saved sample 0 of each row, 0 where that is not finite"""
    with np.errstate(invalid="ignore", over="ignore"):
        mean = np.asarray(sums, dtype=np.float64) / float(nchains)
    return np.where(np.isfinite(mean), mean, 0.0)


class CorrelationMatrix(np.ndarray):
    """what Chains.cor returns: the [d][d] float64 matrix (an ndarray in every respect) that prints with the parameter names"""

    def __new__(cls, cor, names):
        obj = np.asarray(cor, dtype=np.float64).view(cls)
        obj.names = list(names)
        return obj

    def __array_finalize__(self, obj):
        self.names = getattr(obj, "names", None)

    def __str__(self):
        names = self.names
        if names is None or self.ndim != 2 or self.shape != (len(names), len(names)):
            return np.ndarray.__str__(self)
        w = max([12] + [len(n) for n in names])
        lines = ["Correlation", "  %-*s " % (w, "parameters") + " ".join("%*s" % (max(9, len(n)), n) for n in names)]
        for i, n in enumerate(names):
            lines.append("  %-*s " % (w, n) + " ".join("%*.4f" % (max(9, len(c)), self[i, j]) for j, c in enumerate(names)))
        return "\n".join(lines)

    __repr__ = __str__


RHAT_KINDS = {"rank": "rhat", "bulk": "rhat_bulk", "tail": "rhat_tail", "basic": None}


def _rhat_column(kind):
    """the key of Run.rank_diagnostics that holds an R-hat kind (MCMCDiagnosticTools' names); None: the split R-hat of diagnostics"""
    if kind not in RHAT_KINDS:
        raise L.ArgumentError(L.MHX_EINVAL, "rhat kind must be one of %s" % ", ".join(repr(k) for k in RHAT_KINDS))
    return RHAT_KINDS[kind]


class Chains:
    """value[iteration, parameter, chain]; the last parameter is the internal `lp`
    (ext/AdvancedMHMCMCChainsExt.jl:36, :96-118)."""

    def __init__(self, value, names, start, thin, accepted=None, stats=None, state=None):
        self.value = value
        self.names = list(names)
        self.start, self.thin = int(start), int(thin)
        self.accepted = accepted
        self.stats = stats or {}
        self.state = state
        self.internals = ["lp"]

    def range(self):
        n = self.value.shape[0]
        return range(self.start, self.start + self.thin * n, self.thin)

    def __getitem__(self, name):
        if isinstance(name, str):
            return self.value[:, self.names.index(name), :]
        return self.value[name]

    def __len__(self):
        return self.value.shape[0]

    @property
    def nchains(self):
        return self.value.shape[2]

    def mean(self, name):
        return float(np.mean(self[name], dtype=np.float64))

    def params(self):
        return [n for n in self.names if n not in self.internals]

    def summarystats(self, max_lag=0, rhat_kind="basic"):
        """The table MCMCChains prints for the reference's chains (README.md:59-63): mean, std, ess_bulk, ess_tail
        and (split) rhat per parameter, computed on the device from the run's sample buffer (mhx_run_diagnostics,
        mhx_run_ess_bulk_tail); internals (lp) are left out as MCMCChains does.  rhat_kind: as Chains.rhat; any kind but "basic"
        takes the ESS columns and R-hat from one mhx_run_rank_diagnostics call."""
        if self.state is None:
            raise L.ArgumentError(L.MHX_EINVAL, "summarystats needs the live run (chain.state)")
        col = _rhat_column(rhat_kind)
        idx = [i for i, n in enumerate(self.names) if n not in self.internals]
        if col is None:
            dg = self.state.diagnostics(max_lag=0, split=True)
            et = self.state.ess_bulk_tail(params=idx, max_lag=max_lag, split=True)
            rhat = dg["rhat"][idx] if "rhat" in dg else np.full(len(idx), np.nan)
        else:
            et = self.state.rank_diagnostics(params=idx, max_lag=max_lag, split=True)
            rhat = et[col]
        full = self.state.diagnostics(max_lag=0, split=False)
        std = np.sqrt(np.maximum(full.get("var_plus", full["W"]), 0.0))
        return dict(parameters=[self.names[i] for i in idx], mean=full["mean"][idx], std=std[idx],
                    ess_bulk=et["ess_bulk"], ess_tail=et["ess_tail"], rhat=rhat)

    def rhat(self, kind="rank"):
        """Split R-hat of every parameter (internals left out as in summarystats), by MCMCDiagnosticTools' kinds: "rank" (its
        default: the larger of "bulk" and "tail"), "bulk" (of the normal scores of the ranks), "tail" (of the normal scores of the
        ranks of |x - median|) -- all three from Run.rank_diagnostics -- and "basic", the classic split R-hat of the draws
        themselves (mhx_run_diagnostics; what summarystats prints by default).  dict(parameters, kind, rhat [nparams])."""
        if self.state is None:
            raise L.ArgumentError(L.MHX_EINVAL, "rhat needs the live run (chain.state)")
        col = _rhat_column(kind)
        idx = [i for i, n in enumerate(self.names) if n not in self.internals]
        if col is None:
            dg = self.state.diagnostics(max_lag=0, split=True)
            rhat = dg["rhat"][idx] if "rhat" in dg else np.full(len(idx), np.nan)
        else:
            rhat = self.state.rank_diagnostics(params=idx, split=True, ess=False)[col]
        return dict(parameters=[self.names[i] for i in idx], kind=kind, rhat=rhat)

    def quantile(self, probs=DEFAULT_QUANTILE_PROBS):
        """The "Quantiles" table MCMCChains prints for the reference's chains (README.md:65-71): exact quantiles (Julia's and
        numpy's default definition) of every parameter over all draws of all chains, selected on the device from the run's
        sample buffer (mhx_run_order_statistics); internals (lp) are left out as in summarystats.
        dict(parameters, probs, quantiles [nparams][nprobs])."""
        if self.state is None:
            raise L.ArgumentError(L.MHX_EINVAL, "quantile needs the live run (chain.state)")
        idx = [i for i, n in enumerate(self.names) if n not in self.internals]
        probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        return dict(parameters=[self.names[i] for i in idx], probs=probs, quantiles=self.state.quantiles(probs, params=idx))

    def hpd(self, alpha=0.05):
        """MCMCChains' `hpd(chain; alpha)`: the highest-posterior-density interval of mass 1 - alpha of every parameter over all draws of
        all chains (the Chen-Shao interval), taken on the device from the run's sample buffer (mhx_run_hpd); internals (lp) are left
        out as in quantile.  An HPDTable: dict(parameters, alpha, lower [nparams], upper [nparams]) that prints as a table."""
        if self.state is None:
            raise L.ArgumentError(L.MHX_EINVAL, "hpd needs the live run (chain.state)")
        idx = [i for i, n in enumerate(self.names) if n not in self.internals]
        lower, upper = self.state.hpd(alpha, params=idx)
        return HPDTable(parameters=[self.names[i] for i in idx], alpha=float(alpha), lower=lower, upper=upper)

    def _moment_rows(self, include_lp, what):
        if self.state is None:
            raise L.ArgumentError(L.MHX_EINVAL, "%s needs the live run (chain.state)" % what)
        return [i for i, n in enumerate(self.names) if include_lp or n not in self.internals]

    def cov(self, include_lp=False):
        """[d][d] float64 covariance matrix of the parameters over all draws of all chains (np.cov of the flattened chains), from
        cross moments taken on the device (mhx_run_cross_moments); internals (lp) are left out unless include_lp."""
        return self.state.cov(params=self._moment_rows(include_lp, "cov"))

    def cor(self, include_lp=False):
        """the correlation matrix of the same rows (MCMCChains' `cor(chain)`); prints with the parameter names"""
        idx = self._moment_rows(include_lp, "cor")
        return CorrelationMatrix(self.state.cor(params=idx), [self.names[i] for i in idx])

    def _live_row(self, name, what):
        if self.state is None:
            raise L.ArgumentError(L.MHX_EINVAL, "%s needs the live run (chain.state)" % what)
        return self.names.index(name)

    def histogram(self, name, bins=64, range=None):
        """(counts int64 [bins], edges [bins + 1]) of one parameter over all draws of all chains, counted on the device from the run's
        sample buffer (mhx_run_histogram): both members equal `np.histogram(chain[name].astype(np.float64).ravel(), bins, range)`
        -- the draws widened, as numpy builds float32 edges for a float32 array.  range None: the row's minimum and maximum."""
        row = self._live_row(name, "histogram")
        counts, e, _ = self.state.histogram(bins, range, params=[row])
        return counts[0], e[0]

    def histogram2d(self, x, y, bins=32, range=None):
        """(H int64 [bins][bins], xedges, yedges) of two parameters over all draws of all chains, counted on the device
        (mhx_run_histogram2d): what `np.histogram2d` gives for the widened draws, its H cast to integers.  range: None (each row's
        minimum and maximum) or [(xlo, xhi), (ylo, yhi)]."""
        rows = [self._live_row(x, "histogram2d"), self._live_row(y, "histogram2d")]
        H, e, _, _ = self.state.histogram2d(params=rows, pairs=[(0, 1)], bins=bins, range=range)
        return H[0], e[0], e[1]

    def corner(self, names=None, bins=32):
        """MCMCChains' `corner`, as numbers: a Corner with the marginal histogram of every parameter in `names` (default: all,
        internals (lp) left out unless named) and the joint histogram of every pair, over `bins` uniform bins between each row's
        minimum and maximum -- one order-statistics call, one 1-D and one 2-D histogram call on the device."""
        if self.state is None:
            raise L.ArgumentError(L.MHX_EINVAL, "corner needs the live run (chain.state)")
        names = self.params() if names is None else list(names)
        idx = np.array([self.names.index(n) for n in names], dtype=np.int32)
        e = _histogram_edges(self.state, idx, bins, None, None, "corner")
        if e.shape[1] - 1 > HISTOGRAM2D_MAX_BINS:
            raise L.ArgumentError(L.MHX_EINVAL, "corner: bins = %d is not in [1, %d]" % (e.shape[1] - 1, HISTOGRAM2D_MAX_BINS))
        counts, _, out1 = self.state.histogram(params=idx, edges=e)
        joint, outside = {}, {n: out1[i] for i, n in enumerate(names)}
        if len(names) > 1:
            H, _, out2, pairs = self.state.histogram2d(params=idx, edges=e)
            for q, (i, j) in enumerate(pairs):
                joint[(names[i], names[j])] = H[q]
                outside[(names[i], names[j])] = int(out2[q])
        return Corner(names, {n: e[i] for i, n in enumerate(names)}, {n: counts[i] for i, n in enumerate(names)}, joint, outside)

    def density(self, name, npoints=2048, bandwidth=None):
        """MCMCChains' `density`: (x [npoints], density [npoints]), the Gaussian kernel density estimate of one parameter over all
        draws of all chains.  bandwidth None: Silverman's rule as KernelDensity.jl's default applies it (silverman_bandwidth), the
        std from the pooled variance (Run.cov of the row), the quartiles by the definition of Run.quantiles.  x are the centres of
        the npoints (<= 2048) bins of histogram_edges(min - 4 h, max + 4 h, npoints); the only sweep of the draws is a histogram on
        the device (mhx_run_histogram), and the kernel sum over its integer counts runs on the host in float64
        (density_from_counts).
        Deviation from KernelDensity.jl: that package spreads every draw linearly over its two neighbouring grid points (and
        convolves by FFT); here a draw counts in the cell it lies in, so that the counts stay integers -- exact, reproducible and
        additive over shards.  The price is bounded: a draw moves by at most half a cell delta / 2, so
        |density[k] - the exact estimate at x[k]| <= delta / (2 h^2 sqrt(2 pi e)) (density_binning_bound)."""
        row = self._live_row(name, "density")
        run = self.state
        S = run._n_draws()
        if S < 1:
            run.order_statistics([0], [row])               # raises the library's refusal
        j, j1, g = quantile_ranks(S, [0.25, 0.75])
        os_ = run.order_statistics(np.concatenate([j, j1, [0, S - 1]]), [row])[0]
        q25, q75 = quantiles_from_order_statistics(os_[:2], os_[2:4], g)
        lo, hi = float(os_[4]), float(os_[5])
        if not (math.isfinite(lo) and math.isfinite(hi)):
            raise L.ArgumentError(L.MHX_EINVAL, "density: the draws of %s span (%r, %r): not finite" % (name, lo, hi))
        if bandwidth is None:
            std = math.sqrt(max(float(run.cov([row])[0, 0]), 0.0)) if S > 1 else 0.0
            h = silverman_bandwidth(std, q25, q75, S)
        else:
            h = float(bandwidth)
        if not (math.isfinite(h) and h > 0.0):
            raise L.ArgumentError(L.MHX_EINVAL, "density: the bandwidth %r is not a positive finite number" % h)
        e = histogram_edges(lo - 4.0 * h, hi + 4.0 * h, npoints)
        counts, _, _ = run.histogram(params=[row], edges=e)
        return density_from_counts(counts[0], e, h)

    def autocor(self, lags=(1, 5, 10, 50), mean_of_chains=False, chains=None):
        """MCMCChains' `autocor(chain; lags)`: an AutocorTable dict(parameters, lags, autocor [nparams][nlags]) of every parameter
        (internals (lp) left out as in quantile), summed on the device from the run's sample buffer (mhx_run_autocovariance).
        Every chain is centred about its own mean.  Default: the ratio of the sums over the chains, sum_c A_c(k) / sum_c A_c(0);
        mean_of_chains: the mean over the chains of each chain's own autocorrelation A_c(k) / A_c(0) (chains that never moved left
        out).  chains = (begin, count) restricts both to a range; with (c, 1) the row is StatsBase.autocor of chain c either way.
        Lag 0 is always asked for (it is the denominator) and shown only if listed.  A lag >= len(chain) is an ArgumentError."""
        if self.state is None:
            raise L.ArgumentError(L.MHX_EINVAL, "autocor needs the live run (chain.state)")
        lg = sorted(set(int(k) for k in np.atleast_1d(lags)))
        for k in lg:
            if k < 0 or k >= len(self):
                raise L.ArgumentError(L.MHX_EINVAL, "autocor: lag %d is not in [0, %d), the draws of a chain" % (k, len(self)))
        idx = [i for i, n in enumerate(self.names) if n not in self.internals]
        ask = lg if lg and lg[0] == 0 else [0] + lg
        acov, _ = self.state.autocovariance(ask, params=idx, chains=chains, normalise=bool(mean_of_chains))
        rho = autocorrelation(acov)[:, len(ask) - len(lg):]
        return AutocorTable(parameters=[self.names[i] for i in idx], lags=lg, autocor=rho)

    def autocorr_time(self, c=5.0, tol=50, max_lag=None, ensemble=None):
        """The integrated autocorrelation time of every parameter (internals left out), as emcee's `get_autocorr_time` defines it
        for an ensemble: the mean over the chains (walkers) of each chain's own autocorrelation function -- the normalised sums of
        mhx_run_autocovariance over lags 0..max_lag -- summed under Sokal's automatic window (mhx.integrated_time).
        dict(parameters, tau [nparams], window, truncated, converged = N >= tol tau).  On an Ensemble run of several ensembles,
        ensemble=e takes the walkers of ensemble e, chains [e W, (e + 1) W); the walkers of different ensembles never mix otherwise
        than by this choice (None: all chains).
        max_lag None: N - 1, every lag, as emcee does -- N (N + 1) / 2 multiply-adds per chain and row, about N / 2 sweeps' worth of
        arithmetic over the tensor (the window rarely needs more than a few tau of them): max_lag caps the lags computed, and a
        window that is not reached within them comes back truncated."""
        if self.state is None:
            raise L.ArgumentError(L.MHX_EINVAL, "autocorr_time needs the live run (chain.state)")
        N = len(self)
        K = N - 1 if max_lag is None else int(max_lag)
        if K < 0 or K >= max(N, 1):
            raise L.ArgumentError(L.MHX_EINVAL, "autocorr_time: max_lag = %d is not in [0, %d)" % (K, N))
        chains = None
        if ensemble is not None:
            E = int(getattr(self.state, "n_ensembles", 0))
            if E < 1 or not 0 <= int(ensemble) < E:
                raise L.ArgumentError(L.MHX_EINVAL, "autocorr_time: ensemble %r of a run of %d ensembles" % (ensemble, E))
            W = self.state.n // E
            chains = (int(ensemble) * W, W)
        idx = [i for i, n in enumerate(self.names) if n not in self.internals]
        acov, nvalid = self.state.autocovariance(np.arange(K + 1), params=idx, chains=chains, normalise=True)
        rho = autocorrelation(acov)
        res = [integrated_time(r, c) for r in rho]
        tau = np.array([r[0] for r in res], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            converged = float(N) >= float(tol) * tau
        return dict(parameters=[self.names[i] for i in idx], tau=tau, window=np.array([r[1] for r in res], dtype=np.int64),
                    truncated=np.array([r[2] for r in res], dtype=bool), converged=converged, nvalid=nvalid)

    def derive(self, fn, names=None, lp=False):
        """The chain of derived quantities -- sigma ** 2, exp(beta), mu[1] - mu[0], an indicator where(theta > 0, 1.0, 0.0) -- of
        every draw, mapped on the device from the run's sample buffer (Run.derive): `chain.derive(lambda t: t.sigma ** 2,
        names=["sigma2"]).describe()`.  fn gets the parameters as a vector that answers to their names (with lp=True: fn(theta, lp))
        and returns one number or a list of them; `names` names the outputs.  The result is a Chains over a derived run
        (chain.state), with the same start and thin and this chain's accept flags: describe, hpd, cor, corner, density, autocor and
        rhat work on it as on any chain.  Needs the live run."""
        if self.state is None:
            raise L.ArgumentError(L.MHX_EINVAL, "derive needs the live run (chain.state)")
        run = self.state.derive(fn, names=self.params(), lp=lp)
        if names is None:
            names = ["derived"] if run.dim == 1 else ["derived[%d]" % (j + 1) for j in range(run.dim)]
        names = [str(n) for n in ([names] if isinstance(names, str) else names)]
        if len(names) != run.dim:
            raise L.ArgumentError(L.MHX_EINVAL, "derive: %d names for %d outputs" % (len(names), run.dim))
        value, _ = run.samples()
        return Chains(value, names + ["lp"], self.start, self.thin, accepted=self.accepted, stats=dict(self.stats), state=run)

    def predict(self, fn, names=None, seed=None):
        """The chain of posterior predictive draws: `chain.predict(lambda t: mhx.Normal(t.mu, t.sigma), names=["y_rep"]).describe()`.
        As derive, for a function that draws: it returns distributions (one draw from each) or numbers computed from
        mhx.trace.draw(dist) values and the parameters; every (chain, saved draw) has a stream of its own, keyed by `seed` (default:
        the run's) -- Run.predict.  The same call gives the same draws.  Needs the live run."""
        if self.state is None:
            raise L.ArgumentError(L.MHX_EINVAL, "predict needs the live run (chain.state)")
        run = self.state.predict(fn, names=self.params(), seed=seed)
        if names is None:
            names = ["predicted"] if run.dim == 1 else ["predicted[%d]" % (j + 1) for j in range(run.dim)]
        names = [str(n) for n in ([names] if isinstance(names, str) else names)]
        if len(names) != run.dim:
            raise L.ArgumentError(L.MHX_EINVAL, "predict: %d names for %d outputs" % (len(names), run.dim))
        value, _ = run.samples()
        return Chains(value, names + ["lp"], self.start, self.thin, accepted=self.accepted, stats=dict(self.stats), state=run)

    def _pointwise_sums(self, who, fn, rows):
        if self.state is None:
            raise L.ArgumentError(L.MHX_EINVAL, "%s needs the live run (chain.state)" % who)
        return self.state.pointwise(fn, rows, names=self.params())

    def pointwise(self, fn, rows=None):
        """The pointwise log-likelihood table of the chain: `chain.pointwise(lambda t, y: ..., data)` -- per data row lppd, mean, var,
        p_waic, elpd and bad (pointwise_table has the formulas), from one pass over the run's sample buffer on the device
        (Run.pointwise); the draws x rows matrix is never stored.  fn(theta, row) returns log p(row | theta): theta answers to the
        parameter names, row is a number (1-D rows) or a vector (2-D).  Needs the live run."""
        return pointwise_table(self._pointwise_sums("pointwise", fn, rows))

    def waic(self, fn, rows=None):
        """WAIC of the model whose per-row log-likelihood is fn (Turing's pointwise_loglikelihoods followed by WAIC; Watanabe's WAIC-2,
        the variance form): dict(elpd_waic, p_waic, waic = -2 elpd_waic, se, n_high_variance, pointwise) -- waic_from_table.  Needs
        the live run."""
        return waic_from_table(self.pointwise(fn, rows))

    def dic(self, fn, rows=None):
        """DIC (MCMCChains' dic): D-bar = -2 sum_i mean_i from the same device pass as waic, D(theta-bar) on the host at the chain's
        posterior means by the trace's evaluate, p_D = D-bar - D(theta-bar), DIC = D-bar + p_D.  fn must be a callable or a
        TracedPointwise: a HipPointwise has no host evaluator.  Needs the live run."""
        if isinstance(fn, HipPointwise):
            raise L.ArgumentError(L.MHX_EINVAL, "dic: a HipPointwise has no host evaluator for D(theta-bar): pass a callable or a TracedPointwise")
        sums = self._pointwise_sums("dic", fn, rows)
        traced = sums.fn
        theta_bar = np.array([self.mean(n) for n in self.params()], dtype=np.float64)
        if traced.lp:
            raise L.ArgumentError(L.MHX_EINVAL, "dic: a function that reads lp has no value at the posterior mean")
        mat = traced.rows if rows is None else _pointwise_rows("dic", rows)
        return dic_from_table(pointwise_table(sums), traced, theta_bar, mat)

    def loo(self, fn, rows=None, reff=1.0):
        """PSIS-LOO of the model whose per-row log-likelihood is fn (what ArviZ / R loo compute from Turing's
        pointwise_loglikelihoods): `chain.loo(lambda t, y: ..., data)` -- dict(elpd_loo, p_loo, looic = -2 elpd_loo, se, khat_counts,
        khat_threshold, pointwise) that prints, loo_from_table of loo_table of Run.psis and Run.pointwise.  reff: the relative
        efficiency of the draws the tail length is computed with (1: as if independent).  Needs the live run."""
        if self.state is None:
            raise L.ArgumentError(L.MHX_EINVAL, "loo needs the live run (chain.state)")
        sums = self.state.pointwise(fn, rows, names=self.params())
        return loo_from_table(loo_table(self.state.psis(sums.fn, rows, reff=reff), sums))

    def _header(self):
        """the first line of the printout: shape, element type and iteration range, as MCMCChains words it"""
        return "Chains MCMC chain (%dx%dx%d Array{%s, 3}), iterations %d:%d:%d" % (
            self.value.shape[0], self.value.shape[1], self.value.shape[2],
            "Float64" if self.value.dtype == np.float64 else "Float32", self.start, self.thin, self.range()[-1])

    def describe(self, probs=DEFAULT_QUANTILE_PROBS, max_lag=0, rhat_kind="basic"):
        """The two tables MCMCChains prints for the reference's chains (README.md:57-71) as text: "Summary Statistics" -- the columns
        of summarystats() with naive_se = std / sqrt(S) and mcse = std / sqrt(ess_bulk), S the draws of all chains -- and
        "Quantiles" below it.  rhat_kind: which R-hat the rhat column holds (Chains.rhat)."""
        st, qt = self.summarystats(max_lag=max_lag, rhat_kind=rhat_kind), self.quantile(probs)
        S = float(self.value.shape[0] * self.value.shape[2])
        with np.errstate(divide="ignore", invalid="ignore"):
            naive_se, mcse = st["std"] / np.sqrt(S), st["std"] / np.sqrt(st["ess_bulk"])
        head = self._header()
        lines = [head, "", "Summary Statistics",
                 "  parameters        mean       std  naive_se      mcse   ess_bulk   ess_tail      rhat"]
        for i, n in enumerate(st["parameters"]):
            lines.append("  %-12s %9.4f %9.4f %9.4f %9.4f %10.1f %10.1f %9.4f" % (
                n, st["mean"][i], st["std"][i], naive_se[i], mcse[i], st["ess_bulk"][i], st["ess_tail"][i], st["rhat"][i]))
        lines += ["", "Quantiles", "  parameters   " + " ".join("%9s" % ("%.1f%%" % (100.0 * p)) for p in qt["probs"])]
        for i, n in enumerate(qt["parameters"]):
            lines.append("  %-12s " % n + " ".join("%9.4f" % q for q in qt["quantiles"][i]))
        return "\n".join(lines)

    def __repr__(self, rhat_kind="basic"):
        head = self._header()
        _rhat_column(rhat_kind)
        try:
            st = self.summarystats(rhat_kind=rhat_kind)
        except Exception:
            return head
        lines = [head, "  parameters        mean       std   ess_bulk   ess_tail      rhat"]
        for i, n in enumerate(st["parameters"][:20]):
            lines.append("  %-12s %9.4f %9.4f %10.1f %10.1f %9.4f" % (n, st["mean"][i], st["std"][i], st["ess_bulk"][i],
                                                                   st["ess_tail"][i], st["rhat"][i]))
        if len(st["parameters"]) > 20:
            lines.append("  ... %d more" % (len(st["parameters"]) - 20))
        return "\n".join(lines)


# ------------------------------------------------------------------------------------------------
# a live run (what AbstractMCMC's `state` is for the reference)


class Run:
    def __init__(self, model, sampler, nchains=1, seed=0, first_chain=0, ctx=None, flags=0, reduce_lanes=0, dtype=None,
                 normal_gen=None):
        """normal_gen: None / "box-muller" (default) or "ziggurat" (MHX_FLAG_ZIGGURAT: RWMH on the cooperative or the register
        kernel of an fp64 context, user log-densities included -- a different, cheaper stream of standard normals; reported in
        stats()["normal_gen"])."""
        if normal_gen not in (None, "box-muller", "ziggurat"):
            raise L.ArgumentError(L.MHX_EINVAL, "normal_gen must be None, 'box-muller' or 'ziggurat'")
        if normal_gen == "ziggurat":
            flags |= L.FLAG_ZIGGURAT
        self.ctx = ctx or L.Context.default(dtype=dtype)
        self.real = self.ctx.real
        f32 = self.ctx.arr                                  # (the name of round 1: now "an array of the context's reals")
        self.model, self.sampler = model, sampler
        self.h = C.c_void_p()
        lib = L.lib()
        d = model.dim
        self._keep = []
        self.tempered = isinstance(sampler, Tempered)
        self.adaptive = False
        if self.tempered:
            # a ladder of R rungs per "chain" asked for: nchains device chains in all, whole ladders (mhx_rwmh_create_tempered)
            mv = sampler.proposal.proposal
            if mv.dim != d:
                raise L.ArgumentError(L.MHX_EINVAL, "proposal dimension %d != model dimension %d" % (mv.dim, d))
            vec = None if mv.vec is None else f32(mv.vec)
            mean = f32(mv.mean) if np.any(mv.mean != 0) else None
            self._keep += [vec, mean, sampler.betas, sampler.scales]
            cfg = L.RwmhCfg(d, nchains, seed, first_chain, mv.kind, mv.scale, L.fptr(vec), flags, L.fptr(mean), reduce_lanes)
            tcfg = L.TemperedCfg(sampler.R, sampler.swap_every, sampler.betas.ctypes.data,
                                 None if sampler.scales is None else sampler.scales.ctypes.data)
            if sampler.reference is not None:
                self._keep += [sampler.ref_mean, sampler.ref_sd]
                ref = L.TemperedReference(sampler.ref_mean.ctypes.data, sampler.ref_sd.ctypes.data)
                L.check(lib.mhx_rwmh_create_tempered_anchored(self.ctx.h, model.handle(self.ctx), C.byref(cfg), C.byref(tcfg), C.byref(ref),
                                                              C.byref(self.h)))
            elif sampler.adapt is None:
                L.check(lib.mhx_rwmh_create_tempered(self.ctx.h, model.handle(self.ctx), C.byref(cfg), C.byref(tcfg), C.byref(self.h)))
            else:
                acfg = sampler.adapt.cfg()
                L.check(lib.mhx_rwmh_create_tempered_adaptive(self.ctx.h, model.handle(self.ctx), C.byref(cfg), C.byref(tcfg), C.byref(acfg),
                                                              C.byref(self.h)))
            self.n = nchains
            self.kind = "rwmh"
        elif isinstance(sampler, MetropolisHastings):
            mv = sampler.proposal.proposal
            if mv.dim != d:
                raise L.ArgumentError(L.MHX_EINVAL, "proposal dimension %d != model dimension %d" % (mv.dim, d))
            if isinstance(sampler.proposal, StaticProposal):
                flags |= L.MHX_FLAG_STATIC_PROPOSAL
            if isinstance(mv, CompositeProposal):
                # blocks with their own kind, symmetric flag and parameter map: the tables and one traced source, its own entry point
                tab = (L.ProposalComponent * mv.dim)(*[L.ProposalComponent(f, 0, p0, p1) for f, p0, p1 in mv.table()])
                blk = (L.ProposalBlock * len(mv.blocks))(*[L.ProposalBlock(f, n, fl, 0) for f, n, fl in mv.blocks])
                mapped = (C.c_int32 * mv.dim)(*mv.mapped) if any(mv.mapped) else None
                data = None if mv.data is None else f32(mv.data)
                self._keep += [data]
                cfg = L.RwmhCfg(d, nchains, seed, first_chain, L.PROP_ISO, 1.0, None, flags, None, reduce_lanes)
                L.check(lib.mhx_rwmh_create_composite(self.ctx.h, model.handle(self.ctx), C.byref(cfg), tab, mv.dim, blk, len(mv.blocks), mapped,
                                                      mv.source.encode() if mv.source else None, L.fptr(data),
                                                      0 if data is None else data.size, C.byref(self.h)))
            elif isinstance(mv, ConditionalProposal):
                # a function of the state: the component table and the traced parameter map, its own entry point
                if sampler.proposal.issymmetric:
                    flags |= L.FLAG_SYMMETRIC_PROPOSAL
                tab = (L.ProposalComponent * mv.dim)(*[L.ProposalComponent(f, 0, p0, p1) for f, p0, p1 in mv.table()])
                data = None if mv.data is None else f32(mv.data)
                self._keep += [data]
                cfg = L.RwmhCfg(d, nchains, seed, first_chain, L.PROP_ISO, 1.0, None, flags, None, reduce_lanes)
                L.check(lib.mhx_rwmh_create_conditional(self.ctx.h, model.handle(self.ctx), C.byref(cfg), tab, mv.dim,
                                                        mv.source.encode(), L.fptr(data), 0 if data is None else data.size, C.byref(self.h)))
            elif isinstance(mv, ComponentProposal):
                # univariate family components: their own entry point, the (Mv)Normal fields of the configuration unused
                if sampler.proposal.issymmetric:
                    flags |= L.FLAG_SYMMETRIC_PROPOSAL
                tab = (L.ProposalComponent * mv.dim)(*[L.ProposalComponent(f, 0, p0, p1) for f, p0, p1 in mv.table()])
                cfg = L.RwmhCfg(d, nchains, seed, first_chain, L.PROP_ISO, 1.0, None, flags, None, reduce_lanes)
                L.check(lib.mhx_rwmh_create_components(self.ctx.h, model.handle(self.ctx), C.byref(cfg), tab, mv.dim, C.byref(self.h)))
            else:
                vec = None if mv.vec is None else f32(mv.vec)
                mean = f32(mv.mean) if np.any(mv.mean != 0) else None
                self._keep += [vec, mean]
                cfg = L.RwmhCfg(d, nchains, seed, first_chain, mv.kind, mv.scale, L.fptr(vec), flags, L.fptr(mean), reduce_lanes)
                if getattr(sampler, "adapt", None) is not None:
                    acfg = sampler.adapt.cfg()
                    L.check(lib.mhx_rwmh_create_adaptive(self.ctx.h, model.handle(self.ctx), C.byref(cfg), C.byref(acfg), C.byref(self.h)))
                    self.adaptive = True
                else:
                    L.check(lib.mhx_rwmh_create(self.ctx.h, model.handle(self.ctx), C.byref(cfg), C.byref(self.h)))
            self.n = nchains
            self.kind = "rwmh"
        elif isinstance(sampler, Ensemble):
            # the distribution StretchProposal wraps is the prior of the initial walkers (src/emcee.jl:29-34): a (Mv)Normal
            # or a vector of Normals is drawn on the device, anything else by the host in init()
            self._prior = None
            try:
                self._prior = _as_mvnormal(sampler.proposal.proposal)
            except L.ArgumentError:
                pass
            ik, isc, ivec, imean = -1, 1.0, None, None
            if self._prior is not None and self._prior.dim == d:
                mvp = self._prior
                ik, isc = mvp.kind, mvp.scale
                ivec = None if mvp.vec is None else f32(mvp.vec)
                imean = f32(mvp.mean) if np.any(mvp.mean != 0) else None
                self._keep += [ivec, imean]
            else:
                self._prior = None
            # `sample(model, Ensemble(W, ..), MCMCThreads(), N, nchains)` runs nchains ENSEMBLES (README.md:135-148): here all of
            # them in one run, ids first_chain .. first_chain + nchains - 1, walkers side by side in the chain axis
            self.n_ensembles = max(1, int(nchains))
            cfg = L.EmceeCfg(d, sampler.n_walkers, seed, first_chain, sampler.proposal.stretch_length, flags, reduce_lanes,
                             ik, isc, L.rptr(ivec), L.rptr(imean), self.n_ensembles)
            L.check(lib.mhx_emcee_create(self.ctx.h, model.handle(self.ctx), C.byref(cfg), C.byref(self.h)))
            self.n = sampler.n_walkers * self.n_ensembles
            self.kind = "emcee"
        elif isinstance(sampler, MALA):
            cfg = L.MalaCfg(d, nchains, seed, first_chain, sampler.resolve(d), flags, reduce_lanes)
            L.check(lib.mhx_mala_create(self.ctx.h, model.handle(self.ctx), C.byref(cfg), C.byref(self.h)))
            self.n = nchains
            self.kind = "mala"
        elif isinstance(sampler, RobustAdaptiveMetropolis):
            if sampler.S is not None and sampler.S.shape != (d, d) and sampler.S.shape != (nchains, d, d):
                # src/RobustAdaptiveMetropolis.jl:202-204
                raise L.ArgumentError(L.MHX_EINVAL, "The provided `S` has the wrong dimensionality.")
            cfg = L.RamCfg(d, nchains, seed, first_chain, sampler.α, sampler.γ, sampler.eigenvalue_lower_bound,
                           sampler.eigenvalue_upper_bound, flags | (L.FLAG_RAM_DEFERRED if sampler.deferred_factor else 0))
            L.check(lib.mhx_ram_create(self.ctx.h, model.handle(self.ctx), C.byref(cfg), C.byref(self.h)))
            self.n = nchains
            self.kind = "ram"
            if sampler.S is not None:
                if sampler.S.ndim == 3:                      # one factor per chain
                    S = np.stack([pack_lower(np.tril(sampler.S[c])) for c in range(nchains)])
                    L.check(lib.mhx_ram_set_factor(self.h, L.rptr(f32(S))))
                else:                                        # the reference's form: one S for the sampler (RAM.jl:198-206)
                    L.check(lib.mhx_ram_set_factor_all(self.h, L.rptr(f32(pack_lower(np.tril(sampler.S))))))
        else:
            raise L.ArgumentError(L.MHX_EINVAL, "unsupported sampler %r" % (sampler,))
        self.dim = d
        self.seed = seed

    # -- initial AbstractMCMC.step
    def init(self, initial_params=None):
        ip = None
        mv = self.sampler.proposal.proposal if self.kind == "rwmh" else None
        if initial_params is None and (isinstance(mv, ConditionalProposal) or (isinstance(mv, CompositeProposal) and any(mv.mapped))):
            raise L.ArgumentError(L.MHX_EINVAL, "a function proposal has no distribution to draw the first state from: "
                                  "give initial_params (as for MALA)")
        if initial_params is not None:
            ip = np.asarray(initial_params, dtype=self.real)
            if self.kind == "emcee" and ip.ndim == 2 and ip.shape == (self.n, self.dim) and self.n != self.dim:
                ip = ip.T                                       # vector-of-walkers form
            if ip.ndim == 1:
                if ip.size != self.dim:
                    raise L.ArgumentError(L.MHX_EINVAL, "initial_params has the wrong dimension")
                ip = np.repeat(ip.reshape(self.dim, 1), self.n, axis=1)
            if ip.shape != (self.dim, self.n):
                raise L.ArgumentError(L.MHX_EINVAL, "initial_params must be (dim,) or (dim, nchains)")
            ip = self.ctx.arr(ip)
        elif self.kind == "emcee" and self._prior is None:
            # src/emcee.jl:29-34: W draws from the wrapped prior.  A (Mv)Normal prior is drawn on the device
            # (mhx_run_init(run, NULL)); any other Distribution: a one-off host draw (numpy Generator seeded from the run
            # seed), the device takes over from the first sweep.
            rng = np.random.default_rng([self.seed, 0xE3CEE])
            ip = self.ctx.arr(np.stack([self.sampler.proposal.rand_initial(rng) for _ in range(self.n)], axis=1))
        L.check(L.lib().mhx_run_init(self.h, L.fptr(ip)))
        self._transitions = 0

    def sample(self, n_samples, discard_initial=0, thinning=1, num_warmup=0, save=True):
        """save: True/1 sample tensor, False/0 nothing, "moments"/2 running moments only (mhx.h)."""
        s = L.Schedule(n_samples, discard_initial, thinning, num_warmup)
        mode = 2 if (isinstance(save, str) and save == "moments") or (save is not True and save == 2) else (1 if save else 0)
        L.check(L.lib().mhx_run_sample(self.h, C.byref(s), mode))
        self._last_n = n_samples if mode == 1 else 0
        self._transitions = getattr(self, "_transitions", 0) + discard_initial + (n_samples - 1) * thinning

    def sample_to_host(self, n_samples, discard_initial=0, thinning=1, num_warmup=0, want_accepted=True, out=None,
                       out_accepted=None, slab_samples=0, pinned=None):
        """mhx_run_sample_to_host: the whole schedule with the samples streamed to the host while the chains keep running
        (two device slabs; what `sample` returns is a host tensor, ext/AdvancedMHMCMCChainsExt.jl:12-39).  Returns
        (samples [N][dim+1][n], accepted [N][n] or None).  `pinned`: allocate the results page-locked (mhx_host_alloc); None = only
        where a DMA writes them -- a save-all run of >= 1024 chains comes back accept-compacted (include/mhx.h: mhx_compact_hdr),
        host threads write the tensor, and page-locking it would cost more than the whole return (0.55 s for C2's 13 GB);
        `out` / `out_accepted`: caller-provided arrays (any host memory: registered for the call when a DMA targets them)."""
        s = L.Schedule(n_samples, discard_initial, thinning, num_warmup)
        shape = (n_samples, self.dim + 1, self.n)
        if pinned is None:
            oc = self.ctx.get_option("HOST_COMPACT")
            pinned = not (int(oc) != 0 if oc else (thinning == 1 and self.n >= 1024))

        def result(shp, dt):
            # page-locked when asked for and available; a host that cannot lock that much (ulimit -l, fragmented memory) gets
            # pageable memory -- the C side registers what it can for the call and otherwise copies pageable
            if pinned:
                try:
                    return L.host_array(shp, dt)
                except L.MhxError:
                    pass
            return np.empty(shp, dtype=dt)
        if out is None:
            out = result(shape, self.real)
        elif out.shape != shape or out.dtype != self.real or not out.flags.c_contiguous:
            raise L.ArgumentError(L.MHX_EINVAL, "sample_to_host: out must be a C-contiguous %s array of shape %s" % (np.dtype(self.real), shape))
        acc = out_accepted
        if acc is None and want_accepted:
            acc = result((n_samples, self.n), np.uint8)
        elif acc is not None and (acc.shape != (n_samples, self.n) or acc.dtype != np.uint8 or not acc.flags.c_contiguous):
            raise L.ArgumentError(L.MHX_EINVAL, "sample_to_host: out_accepted must be a C-contiguous uint8 array of shape (N, nchains)")
        L.check(L.lib().mhx_run_sample_to_host(self.h, C.byref(s), L.fptr(out), L.u8ptr(acc), slab_samples))
        self._last_n = n_samples
        return out, acc

    def host_stats(self):
        """mhx_run_host_stats: what the last sample_to_host moved -- tensor / wire bytes, link and expand time, whether the
        accept-compacted path ran and with how many host threads"""
        st = L.HostStats()
        L.check(L.lib().mhx_run_host_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in L.HostStats._fields_}

    def samples(self, want_accepted=True):
        n_saved = C.c_int64()
        L.check(L.lib().mhx_run_device_samples(self.h, None, None, C.byref(n_saved)))
        N = int(n_saved.value)
        out = np.empty((N, self.dim + 1, self.n), dtype=self.real)
        acc = np.empty((N, self.n), dtype=np.uint8) if want_accepted else None
        L.check(L.lib().mhx_run_get_samples(self.h, L.fptr(out), L.u8ptr(acc)))
        return out, acc

    def state(self):
        x = np.empty((self.dim, self.n), dtype=self.real)
        lp = np.empty(self.n, dtype=self.real)
        cnt = np.empty(self.n, dtype=np.uint32)
        L.check(L.lib().mhx_run_get_state(self.h, L.fptr(x), L.fptr(lp), L.u32ptr(cnt)))
        return x, lp, cnt

    def set_params(self, x):
        """AbstractMCMC.setparams!! (src/AdvancedMH.jl:150-157): replaces params, lp is re-evaluated."""
        x = self.ctx.arr(x)
        if x.shape != (self.dim, self.n):
            raise L.ArgumentError(L.MHX_EINVAL, "set_params: x must be (dim, nchains)")
        L.check(L.lib().mhx_run_set_state(self.h, L.fptr(x)))

    def factor(self):
        nS = self.dim * (self.dim + 1) // 2
        S = np.empty((self.n, nS), dtype=self.real)
        st = np.empty(self.n, dtype=np.uint8)
        L.check(L.lib().mhx_ram_get_factor(self.h, L.fptr(S), L.u8ptr(st)))
        return S, st

    def diag_range(self):
        lo = np.empty((self.dim, self.n), dtype=self.real)
        hi = np.empty((self.dim, self.n), dtype=self.real)
        L.check(L.lib().mhx_ram_get_diag_range(self.h, L.fptr(lo), L.fptr(hi)))
        return lo, hi

    def adapt_state(self):
        """The rest of RobustAdaptiveMetropolisState (src/RobustAdaptiveMetropolis.jl:99-114): logα of every chain's latest
        transition (min(lp' - lp, 0): average exp(logα) for the acceptance probability), the step size η of the latest
        warm-up transition, the iteration counter and isaccept."""
        la = np.empty(self.n, dtype=self.real)
        acc = np.empty(self.n, dtype=np.uint8)
        eta, it = C.c_double(), C.c_uint64()
        L.check(L.lib().mhx_ram_get_adapt_state(self.h, L.rptr(la), C.byref(eta), L.u8ptr(acc), C.byref(it)))
        return dict(logα=la, η=eta.value, iteration=int(it.value), isaccept=acc.astype(bool))

    def watch_factors(self, chains):
        """RobustAdaptiveMetropolis: keep `state.S` of these chains after EVERY recorded step of the following sampling calls -- what a
        reference callback that stores state.S records (test/RobustAdaptiveMetropolis.jl:11-28).  [] switches it off."""
        ch = np.ascontiguousarray(chains, dtype=np.int32)
        L.check(L.lib().mhx_ram_watch_factors(self.h, ch.ctypes.data_as(C.POINTER(C.c_int32)), ch.size))

    def watched_factors(self, full=True):
        """[n recorded][n watched] lower-triangular factors of the last sampling call (full=False: packed row-major)"""
        nrec, nw = C.c_int64(), C.c_int32()
        L.check(L.lib().mhx_ram_get_watched_factors(self.h, None, 0, C.byref(nrec), C.byref(nw)))
        tri = self.dim * (self.dim + 1) // 2
        S = np.empty((nrec.value, nw.value, tri), dtype=self.real)
        L.check(L.lib().mhx_ram_get_watched_factors(self.h, L.rptr(S), nrec.value, None, None))
        if not full:
            return S
        out = np.zeros((nrec.value, nw.value, self.dim, self.dim), dtype=self.real)
        il = np.tril_indices(self.dim)
        out[:, :, il[0], il[1]] = S
        return out

    def step_stats(self, n_samples=None):
        """RobustAdaptiveMetropolis: the sampler state after EVERY recorded step of the last sampling call -- what the
        reference's callback reads off `state` (test/RobustAdaptiveMetropolis.jl:11-28): dict(logα [N][nchains], η [N]);
        mean(exp(logα)) is the acceptance rate the adaptation steers to α (RAM.jl:141-147).  isaccept = the accepted tensor."""
        nrec = C.c_int64()
        L.check(L.lib().mhx_ram_get_step_stats(self.h, None, None, 0, C.byref(nrec)))      # the count the engine recorded
        if n_samples is not None and int(n_samples) != nrec.value:
            raise L.ArgumentError(L.MHX_EINVAL, "step_stats: n_samples = %d, the last sampling call recorded %d" % (n_samples, nrec.value))
        n_samples = int(nrec.value)
        la = np.empty((n_samples, self.n), dtype=self.real)
        eta = np.empty(n_samples, dtype=np.float64)
        L.check(L.lib().mhx_ram_get_step_stats(self.h, L.rptr(la), eta.ctypes.data_as(C.POINTER(C.c_double)), n_samples, None))
        return {"logα": la, "η": eta, "logalpha": la, "eta": eta}

    def stats(self):
        st = L.Stats()
        L.check(L.lib().mhx_run_stats(self.h, C.byref(st)))
        return dict(transitions=st.transitions, accepted=st.accepted, kernel_ms=st.kernel_ms, wall_ms=st.wall_ms,
                    kernel_variant=st.kernel_variant, launches=st.launches, reduce_lanes=st.reduce_lanes,
                    dtype="f64" if st.dtype == L.MHX_F64 else "f32", normal_gen=st.normal_gen, factor_band=st.factor_band,
                    tainted=st.tainted, register_form=st.register_form)

    def form_name(self):
        """The name of the run's kernel form (include/mhx.h, mhx_run_form_name): "coop", "coop_pairs", "coop_jit", ..."""
        return L.lib().mhx_run_form_name(self.h).decode()

    def diagnostics(self, max_lag=0, ess_chains=256, split=False):
        """Sums for R-hat / between-chain ESS (all chains) and, if max_lag > 0, the Geyer ESS from the multi-chain
        autocorrelations.  split=True: every chain counts as two half-chains (split R-hat).  A row that never moved, or that
        holds a non-finite draw, has ess_geyer = NaN (never the n_chains x n_samples of a perfect sampler).  See include/mhx.h
        (mhx_run_diagnostics)."""
        d1 = self.dim + 1
        arrs = [np.zeros(d1, dtype=np.float64) for _ in range(4)]
        cfg = L.DiagCfg(max_lag, ess_chains, 1 if split else 0)
        ptrs = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrs]
        if max_lag <= 0:
            ptrs[3] = None
        L.check(L.lib().mhx_run_diagnostics(self.h, C.byref(cfg), *ptrs))
        n_saved = C.c_int64()
        L.check(L.lib().mhx_run_device_samples(self.h, None, None, C.byref(n_saved)))
        parts = 2 if split else 1
        out = dict(sum_m=arrs[0], sum_m2=arrs[1], sum_v=arrs[2], n_chains=self.n * parts, n_samples=int(n_saved.value) // parts)
        if max_lag > 0:
            out["ess_geyer"] = np.abs(arrs[3])
            out["ess_geyer_truncated"] = arrs[3] < 0
        out.update(combine_diagnostics(out["sum_m"], out["sum_m2"], out["sum_v"], out["n_chains"], out["n_samples"]))
        return out

    def save_state(self):
        """The complete state of the run as bytes (checkpoint; upstream's `state` of step / `initial_state`)."""
        nb = C.c_size_t()
        L.check(L.lib().mhx_run_state_size(self.h, C.byref(nb)))
        buf = np.empty(nb.value, dtype=np.uint8)
        L.check(L.lib().mhx_run_save_state(self.h, buf.ctypes.data_as(C.c_void_p), nb.value))
        return buf.tobytes()

    def load_state(self, blob):
        """Continue a saved run: same sampler, model, dim and chain count; seed, global ids and the RNG step counter come
        from the blob, so the continuation is the uninterrupted run bit for bit."""
        buf = np.frombuffer(blob, dtype=np.uint8)
        L.check(L.lib().mhx_run_load_state(self.h, buf.ctypes.data_as(C.c_void_p), buf.size))

    def ess_bulk_tail(self, params=None, max_lag=0, ess_chains=256, split=True):
        """Rank-normalised bulk ESS and tail ESS (Vehtari et al. 2021; MCMCChains' ess_bulk / ess_tail) of the given
        parameter rows (default: all, lp included) of the last sample buffer, sorted and scored on the device.
        max_lag = 0: half the draws of a (half-)chain.  Negative values: upper bounds; a constant row or one that holds a NaN
        gives NaN, +-inf draws are ranked like any other (see include/mhx.h)."""
        n_saved = C.c_int64()
        L.check(L.lib().mhx_run_device_samples(self.h, None, None, C.byref(n_saved)))
        N = int(n_saved.value) // (2 if split else 1)
        if max_lag <= 0:
            max_lag = max(2, N // 2)
        idx = np.arange(self.dim + 1, dtype=np.int32) if params is None else np.ascontiguousarray(params, dtype=np.int32)
        bulk, tail = np.zeros(len(idx)), np.zeros(len(idx))
        cfg = L.DiagCfg(max_lag, ess_chains, 1 if split else 0)
        dp = C.POINTER(C.c_double)
        L.check(L.lib().mhx_run_ess_bulk_tail(self.h, C.byref(cfg), idx.ctypes.data_as(C.POINTER(C.c_int32)), len(idx),
                                              bulk.ctypes.data_as(dp), tail.ctypes.data_as(dp)))
        return dict(params=idx, ess_bulk=np.abs(bulk), ess_tail=np.abs(tail), bulk_truncated=bulk < 0, tail_truncated=tail < 0)

    def rank_diagnostics(self, params=None, max_lag=0, ess_chains=256, split=True, ess=True, rhat=True):
        """ess_bulk_tail and the rank-normalised split R-hat of the same rows from ONE sort per row (mhx_run_rank_diagnostics):
        rhat_bulk of the normal scores of the draws, rhat_tail of those of the folded draws |x - median|, rhat = the larger of the
        two (Vehtari et al. 2021; MCMCDiagnosticTools' kinds :bulk, :tail, :rank), NaN only if both are.  A row that holds a NaN
        gives NaN everywhere, a median that is not finite rhat_tail = NaN (see include/mhx.h).  ess=False / rhat=False: that half is
        neither computed nor returned."""
        n_saved = C.c_int64()
        L.check(L.lib().mhx_run_device_samples(self.h, None, None, C.byref(n_saved)))
        N = int(n_saved.value) // (2 if split else 1)
        if max_lag <= 0:
            max_lag = max(2, N // 2)
        idx = self._rows(params)
        bulk, tail, rb, rt = [np.zeros(len(idx)) for _ in range(4)]
        cfg = L.DiagCfg(max_lag, ess_chains, 1 if split else 0)
        dp = C.POINTER(C.c_double)
        ptrs = [a.ctypes.data_as(dp) if on else None for a, on in ((bulk, ess), (tail, ess), (rb, rhat), (rt, rhat))]
        L.check(L.lib().mhx_run_rank_diagnostics(self.h, C.byref(cfg), idx.ctypes.data_as(C.POINTER(C.c_int32)), len(idx), *ptrs))
        out = dict(params=idx)
        if ess:
            out.update(ess_bulk=np.abs(bulk), ess_tail=np.abs(tail), bulk_truncated=bulk < 0, tail_truncated=tail < 0)
        if rhat:
            out.update(rhat_bulk=rb, rhat_tail=rt, rhat=np.fmax(rb, rt))
        return out

    def rank_scores(self, param, folded=False):
        """[n_saved][nchains] in the run's width: the normal scores of the tie-averaged ranks of one parameter row over all draws of
        all chains (folded: of |x - median|), as rank_diagnostics reads them (mhx_run_rank_scores) -- what the rank plots are made
        of.  NaN throughout for a row that holds a NaN (folded: also for a median that is not finite)."""
        n_saved = C.c_int64()
        L.check(L.lib().mhx_run_device_samples(self.h, None, None, C.byref(n_saved)))
        out = np.empty((max(int(n_saved.value), 0), self.n), dtype=self.real)
        L.check(L.lib().mhx_run_rank_scores(self.h, int(param), 1 if folded else 0, L.rptr(out)))
        return out

    def order_statistics(self, ranks, params=None):
        """Exact order statistics of the last sample buffer, selected on the device without a sort (mhx_run_order_statistics):
        [nparams][nranks] float64, the draws at the 0-based positions `ranks` (any order, repeats allowed) of the ascending order
        of the n_saved x nchains draws of each parameter row (default: all, lp included).  NaNs order last."""
        idx = np.arange(self.dim + 1, dtype=np.int32) if params is None else np.ascontiguousarray(params, dtype=np.int32).reshape(-1)
        rk = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
        out = np.empty((len(idx), len(rk)), dtype=np.float64)
        L.check(L.lib().mhx_run_order_statistics(self.h, idx.ctypes.data_as(C.POINTER(C.c_int32)), len(idx),
                                                 rk.ctypes.data_as(C.POINTER(C.c_int64)), len(rk),
                                                 out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def quantiles(self, probs=DEFAULT_QUANTILE_PROBS, params=None):
        """[nparams][nprobs] float64: the quantiles (Julia's `quantile` / numpy's default definition) of the given parameter rows
        over all draws of all chains of the last sample buffer -- two order statistics per prob, one order_statistics call."""
        quantile_ranks(1, probs)                            # refuse bad probs before anything else
        n_saved = C.c_int64()
        L.check(L.lib().mhx_run_device_samples(self.h, None, None, C.byref(n_saved)))
        if n_saved.value < 1:
            return self.order_statistics([0], params)       # raises the library's refusal (no device sample tensor)
        return _quantiles(self.order_statistics, int(n_saved.value) * self.n, probs, params)

    def hpd(self, alpha=0.05, params=None):
        """(lower, upper), float64 [nparams] each: the highest-posterior-density interval of mass 1 - alpha of the given parameter rows
        (default: all, lp included, as quantiles) over all draws of all chains of the last sample buffer -- the narrowest
        [y[i], y[S - m + i]], i < m = hpd_ranks(S, alpha), of the ascending order y (the first of equally narrow ones), found on the
        device without a full sort (mhx_run_hpd).  A row that holds a NaN gives (NaN, NaN)."""
        idx = self._rows(params)
        lower, upper = np.empty(len(idx), dtype=np.float64), np.empty(len(idx), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        L.check(L.lib().mhx_run_hpd(self.h, idx.ctypes.data_as(C.POINTER(C.c_int32)), len(idx), float(alpha),
                                    lower.ctypes.data_as(dp), upper.ctypes.data_as(dp)))
        return lower, upper

    def _n_draws(self):
        """n_saved x nchains of the last sample buffer (0: the run holds none)"""
        n_saved = C.c_int64()
        L.check(L.lib().mhx_run_device_samples(self.h, None, None, C.byref(n_saved)))
        return max(int(n_saved.value), 0) * self.n

    def histogram(self, bins=64, range=None, params=None, edges=None):
        """(counts int64 [m][bins], edges float64 [m][bins + 1], outside int64 [m][3]) of the given parameter rows (default: all, lp
        included; a row may repeat) over all draws of all chains of the last sample buffer, counted on the device in one sweep of
        the tensor in place (mhx_run_histogram).  Bin j holds e[j] <= x < e[j+1], the last bin is closed; outside = the draws below
        e[0], above e[bins], and NaN: exactly `np.histogram` of the draws cast to float64 over the same edges, and
        counts.sum(1) + outside.sum(1) == n_saved x nchains.
        range: one (lo, hi) or one per row, turned into numpy's own edges (histogram_edges); None: every row's minimum and maximum,
        from one order_statistics call (a NaN or infinite end is an ArgumentError that names the row).  edges: explicit edges
        ([bins + 1] for all rows or [m][bins + 1]; finite, non-decreasing, need not be uniform) instead of bins / range."""
        return _histogram(self, L.lib().mhx_run_histogram, bins, range, params, edges)

    def histogram2d(self, params=None, pairs=None, bins=32, range=None, edges=None):
        """(counts int64 [npairs][bins][bins], edges [m][bins + 1], outside int64 [npairs], pairs int32 [npairs][2]): the pair
        histograms of the given rows (mhx_run_histogram2d).  pairs: slots (i, j) into params, default every i < j; cell
        [bin of slot i][bin of slot j] by the rule of histogram on each axis (what `np.histogram2d` gives for the widened draws); a
        draw without a bin on either axis counts in the pair's outside.  bins (one for both axes, <= 128), range and edges as in
        histogram, per row.  One sweep reads both rows of every pair: m (m - 1) rows for all pairs of m."""
        return _histogram2d(self, L.lib().mhx_run_histogram2d, params, pairs, bins, range, edges)

    def autocovariance(self, lags, params=None, chains=None, normalise=False):
        """(acov float64 [m][nlags], nvalid int64 [m]) of the given parameter rows (default: all, lp included) at the given lags
        (strictly increasing, 0 <= lag < n_saved) over the chains `chains` = (begin, count) (count 0: to the last; None: all) of the
        last sample buffer, summed on the device from the tensor in place (mhx_run_autocovariance).  With m_c the chain's own mean
        and A_c(k) = sum_{t < N - k} (x_t - m_c)(x_{t+k} - m_c): acov[i][j] = sum_c A_c(k_j), un-normalised, so that shards add; with
        normalise, sum_c A_c(k_j) / A_c(0) over the nvalid[i] chains that moved at all -- the sum over chains of each chain's own
        autocorrelation function (StatsBase.autocor; emcee's walker-averaged f).  mhx.autocorrelation turns either into rho(k).  A
        row with a non-finite draw among the chains read is NaN at every lag, its nvalid 0."""
        return _autocovariance(self, L.lib().mhx_run_autocovariance, lags, params, chains, normalise)

    def _rows(self, params):
        return np.arange(self.dim + 1, dtype=np.int32) if params is None else np.ascontiguousarray(params, dtype=np.int32).reshape(-1)

    def first_sample_sums(self, idx):
        """per-row sums over the chains of saved sample 0 (mhx_ctx_cross_moments on that one sample), or None without a tensor"""
        ptr, n_saved = C.c_void_p(), C.c_int64()
        L.check(L.lib().mhx_run_device_samples(self.h, C.byref(ptr), None, C.byref(n_saved)))
        if n_saved.value < 1 or not ptr.value:
            return None
        dp = C.POINTER(C.c_double)
        s, x = np.empty(len(idx)), np.empty((len(idx), len(idx)))
        L.check(L.lib().mhx_ctx_cross_moments(self.ctx.h, ptr, 1, self.dim + 1, self.n, idx.ctypes.data_as(C.POINTER(C.c_int32)), len(idx),
                                              None, s.ctypes.data_as(dp), x.ctypes.data_as(dp)))
        return s

    def cross_moments(self, params=None, shift=None):
        """(n, shift, sum [m], cross [m][m]) of the given parameter rows (default: all, lp included) of the last sample buffer, taken
        on the device's fp64 matrix cores from the tensor in place (mhx_run_cross_moments): with y = x - shift,
        sum[i] = sum_k y_ik and cross[i][j] = sum_k y_ik y_jk over all n = n_saved x nchains draws, float64 in both widths.
        shift None: the mean over the chains of saved sample 0 of each row (0 where that is not finite) -- near enough to the mean
        to take the cancellation out of covariance_from_moments without a second pass over the tensor."""
        idx = self._rows(params)
        m = len(idx)
        if shift is None:
            s0 = self.first_sample_sums(idx) if m and np.all((idx >= 0) & (idx <= self.dim)) else None
            sh = None if s0 is None else _first_sample_mean(s0, self.n)      # None: the call below raises the library's refusal
        else:
            sh = np.ascontiguousarray(shift, dtype=np.float64).reshape(-1)
            if sh.size != m:
                raise L.ArgumentError(L.MHX_EINVAL, "cross_moments: %d shifts for %d rows" % (sh.size, m))
        dp = C.POINTER(C.c_double)
        s, x, n = np.empty(m), np.empty((m, m)), C.c_int64()
        _check_moments(L.lib().mhx_run_cross_moments(self.h, idx.ctypes.data_as(C.POINTER(C.c_int32)), m, None if sh is None else sh.ctypes.data_as(dp),
                                                     s.ctypes.data_as(dp), x.ctypes.data_as(dp), C.byref(n)))
        return int(n.value), (np.zeros(m) if sh is None else sh), s, x

    def cov(self, params=None):
        """[m][m] float64 covariance matrix of the rows over all draws of all chains (np.cov of the flattened chains)"""
        n, _, s, x = self.cross_moments(params)
        return covariance_from_moments(n, s, x)

    def cor(self, params=None):
        """the correlation matrix of the same rows"""
        return correlation_from_covariance(self.cov(params))

    def derive(self, fn, nout=None, names=None, lp=False):
        """Map every saved draw through `fn` on the device (mhx_run_derive) and return the result as a DerivedRun: a run of dim = nout
        that holds the tensor [n_saved][nout + 1][nchains] -- the outputs, then this run's lp row -- and answers every statistic
        method (quantiles, hpd, cov, histogram, diagnostics, ...) without a host copy.  It is a snapshot: sampling this run again does
        not change it.  fn: a Python callable of the parameter vector (with lp=True: of the vector and the draw's lp) that returns
        one number or a list of them -- traced once by mhx.trace.trace_map, `names` (default: the model's parameter names) making
        the vector answer to theta.<name> --, a TracedMap, or a HipMap(source, nout, data).  nout: checked against the map's."""
        fn, data = self._map("derive", fn, nout, names, lp, False)
        h = C.c_void_p()
        L.check(L.lib().mhx_run_derive(self.h, fn.source.encode(), fn.nout, L.rptr(data), 0 if data is None else data.size, C.byref(h)))
        return DerivedRun(h, self, fn.nout)

    def _map(self, who, fn, nout, names, lp, predictive):
        """the map of derive / predict, traced where it is a callable, and its data block as the library takes it"""
        if names is None and getattr(self, "model", None) is not None:
            names = getattr(self.model, "param_names", None)
        got = fn
        if isinstance(fn, (HipMap, _trace.TracedMap)):      # a recorded or hand-written map: of this entry's kind?
            if isinstance(fn, (HipPredictive, _trace.TracedPredictive)) != predictive:
                fn = None
        elif callable(fn):
            try:
                fn = (_trace.trace_predictive if predictive else _trace.trace_map)(fn, self.dim, names=names, lp=lp)
            except _trace.TraceError as e:
                raise L.ArgumentError(L.MHX_EINVAL, "%s: the callable cannot be traced: %s" % (who, e)) from e
        else:
            fn = None
        if fn is None:
            raise L.ArgumentError(L.MHX_EINVAL, "%s: a callable, a %s or a %s is needed, got %r" % (
                who, "TracedPredictive" if predictive else "TracedMap", "HipPredictive" if predictive else "HipMap", got))
        if isinstance(fn, _trace.TracedMap) and fn.dim != self.dim:
            raise L.ArgumentError(L.MHX_EINVAL, "%s: the map was traced for %d parameters, the run has %d" % (who, fn.dim, self.dim))
        if nout is not None and int(nout) != fn.nout:
            raise L.ArgumentError(L.MHX_EINVAL, "%s: nout = %d, the map has %d outputs" % (who, int(nout), fn.nout))
        return fn, None if fn.data is None else self.ctx.arr(fn.data)

    def predict(self, fn, nout=None, names=None, lp=False, seed=None):
        """Posterior predictive draws on the device (mhx_run_predict): derive for a map that draws random
        numbers, with a DerivedRun as the result.  fn: a Python callable that returns distributions (`lambda t: mhx.Normal(t.mu,
        t.sigma)`: one draw from each), numbers computed from `mhx.trace.draw(dist)` values and the parameters, or a mix -- traced
        once by mhx.trace.trace_predictive --, a TracedPredictive, or a HipPredictive(source, nout, data).  seed: the key of the
        streams, default this run's own (the salt of the spec keeps them apart from the sampler's); every (chain, saved draw, draw
        index) has its own numbers and the same call gives the same bits."""
        fn, data = self._map("predict", fn, nout, names, lp, True)
        seed = self.seed if seed is None else int(seed)
        h = C.c_void_p()
        L.check(L.lib().mhx_run_predict(self.h, fn.source.encode(), fn.nout, L.rptr(data), 0 if data is None else data.size,
                                        seed & 0xffffffffffffffff, C.byref(h)))
        return DerivedRun(h, self, fn.nout)

    def pointwise(self, fn, rows=None, shift=None, names=None):
        """The pointwise log-likelihood l[i, s] = log p(rows[i] | saved draw s) reduced over all draws of all chains on the device
        (mhx_run_pointwise): a PointwiseSums -- dict(max, sumexp, s1, s2, bad, shift [nrows] float64 each, T)
        as include/mhx.h defines them; the T x nrows matrix is never stored.  fn: a Python callable fn(theta, row) that returns one
        number -- traced once by mhx.trace.trace_pointwise, theta answering to the model's parameter names (or `names`), row a number
        for 1-D rows and a vector for 2-D --, a TracedPointwise, or a HipPointwise(source, rows, data); `rows` may be left out where
        fn carries its own.  shift: [nrows] to sum s1 and s2 about (None: the engine's, l of draw 0 of chain 0, returned).
        pointwise_table(sums) turns the result into lppd, mean, var, p_waic and elpd per row."""
        fn, mat = _pointwise_fn("pointwise", fn, rows, self.dim, names, getattr(getattr(self, "model", None), "param_names", None))
        data = None if fn.data is None else self.ctx.arr(fn.data)
        rr = self.ctx.arr(mat)
        nrows, rowlen = rr.shape
        if shift is None:
            sh = np.zeros(nrows, dtype=np.float64)
        else:
            sh = np.array(shift, dtype=np.float64).reshape(-1)
            if sh.size != nrows:
                raise L.ArgumentError(L.MHX_EINVAL, "pointwise: %d shifts for %d rows" % (sh.size, nrows))
        out, T = np.zeros((5, nrows), dtype=np.float64), C.c_int64()
        dp = C.POINTER(C.c_double)
        L.check(L.lib().mhx_run_pointwise(self.h, fn.source.encode(), L.rptr(rr), nrows, rowlen, L.rptr(data), 0 if data is None else data.size,
                                          0 if shift is None else 1, sh.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(T)))
        res = PointwiseSums(max=out[0], sumexp=out[1], s1=out[2], s2=out[3], bad=out[4], shift=sh, T=int(T.value))
        res.fn = fn
        return res

    def psis(self, fn, rows=None, reff=1.0, names=None, tails=False):
        """PSIS-LOO per data row on the device (mhx_run_psis): a PsisResult -- dict(elpd_loo, khat, sigma, tau,
        lmin, body, n_below, bad [nrows] float64 each, T, M, reff; tails [nrows][M] with tails=True) as include/mhx.h defines them.  fn and
        rows as Run.pointwise takes them.  loo_table(psis, sums) adds p_loo from a PointwiseSums."""
        fn, mat = _pointwise_fn("psis", fn, rows, self.dim, names, getattr(getattr(self, "model", None), "param_names", None))
        data = None if fn.data is None else self.ctx.arr(fn.data)
        rr = self.ctx.arr(mat)
        nrows, rowlen = rr.shape
        reff = float(reff)
        out, T, M = np.zeros((8, nrows), dtype=np.float64), C.c_int64(), C.c_int64()
        tl = None
        if tails:                               # [nrows][M]: M from the saved draws, as the engine computes it
            n_saved = C.c_int64()
            L.check(L.lib().mhx_run_device_samples(self.h, None, None, C.byref(n_saved)))
            ok = reff > 0 and math.isfinite(reff)
            tl = np.zeros((nrows, psis_tail_length(int(n_saved.value) * self.n, reff) if ok else 0), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        L.check(L.lib().mhx_run_psis(self.h, fn.source.encode(), L.rptr(rr), nrows, rowlen, L.rptr(data), 0 if data is None else data.size,
                                     reff, out.ctypes.data_as(dp), None if tl is None else tl.ctypes.data_as(dp), C.byref(T), C.byref(M)))
        res = PsisResult(elpd_loo=out[0], khat=out[1], sigma=out[2], tau=out[3], lmin=out[4], body=out[5], n_below=out[6], bad=out[7],
                         T=int(T.value), M=int(M.value), reff=reff)
        if tails:
            assert tl.shape[1] == res["M"]
            res["tails"] = tl
        res.fn = fn
        return res

    # -- a tempered run (mhx.Tempered): the ladder's own statistics
    def swap_stats(self):
        """(attempts [R - 1], swaps [R - 1]) of the pairs (r, r + 1), summed over the ladders, since init (mhx_run_swap_stats)"""
        R = self.sampler.R if getattr(self, "tempered", False) else 2
        att, sw = (C.c_uint64 * (R - 1))(), (C.c_uint64 * (R - 1))()
        L.check(L.lib().mhx_run_swap_stats(self.h, att, sw))
        return np.array(att[:], dtype=np.uint64), np.array(sw[:], dtype=np.uint64)

    def betas(self):
        """the current inverse temperature of every slot, [nladders][R] float64 (mhx_run_ladder_betas): an adaptive run's ladders as
        of the end of the last sample call, a fixed ladder's table in every row"""
        R = self.sampler.R if getattr(self, "tempered", False) else 1
        out = np.empty(self.n, dtype=np.float64)
        L.check(L.lib().mhx_run_ladder_betas(self.h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out.reshape(-1, R)

    def ladder(self):
        """a printable table: per rung the median, minimum and maximum beta over the ladders and the swap rate of pair (rung, rung + 1)"""
        b = self.betas()
        att, sw = self.swap_stats()
        rate = [float(sw[r]) / float(att[r]) if att[r] else float("nan") for r in range(len(att))] + [float("nan")]
        return LadderTable(dict(rung=r, beta_median=float(np.median(b[:, r])), beta_min=float(b[:, r].min()), beta_max=float(b[:, r].max()),
                                rate=rate[r]) for r in range(b.shape[1]))

    def swap_rates(self):
        att, sw = self.swap_stats()
        b = self.sampler.betas if self.sampler.adapt is None else np.median(self.betas(), axis=0)
        return SwapTable(dict(pair=(r, r + 1), beta_lo=float(b[r]), beta_hi=float(b[r + 1]), attempts=int(att[r]), swaps=int(sw[r]),
                              rate=(float(sw[r]) / float(att[r]) if att[r] else float("nan"))) for r in range(len(att)))

    def evidence_table(self):
        """(table [nchains][8] float64, n_saved) of mhx_run_evidence: per chain bad, shift, s1, s2, max_f, sumexp_f, max_b, sumexp_b of
        u = lp - lq over its saved draws"""
        out = np.empty((self.n, 8), dtype=np.float64)
        n_saved = C.c_int64()
        L.check(L.lib().mhx_run_evidence(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n_saved)))
        return out, int(n_saved.value)

    def evidence(self):
        """the log marginal likelihood of an anchored tempered run whose ladder ends at beta = 0 (Tempered(..., reference=...)): an
        EvidenceResult -- thermodynamic integration and both stepping-stone estimates with their standard errors between ladders"""
        table, n_saved = self.evidence_table()
        return evidence_from_table(table, self.betas()[0], n_saved)

    def rung(self, r):
        """rung r of every ladder as a snapshot run (mhx_run_rung): [n_saved][dim + 1][nladders] on the device, read by every post-run
        statistic like any run"""
        h = C.c_void_p()
        L.check(L.lib().mhx_run_rung(self.h, int(r), C.byref(h)))
        out = DerivedRun(h, self, self.dim)
        out.n = self.n // self.sampler.R
        return out

    # -- an adaptive run (RWMH(..., adapt=ProposalAdaptation(...))): every chain's own proposal
    def proposal_state(self):
        """dict(lam [nchains], sd [dim][nchains], mean [dim][nchains] (NaN without shape), acc_at_freeze [nchains] uint32) as of the end
        of the last sample call, float64 widened exactly from the run's width (mhx_run_proposal_state)"""
        n, d = self.n, self.dim
        lam, sd, mean = np.empty(n, dtype=np.float64), np.empty((d, n), dtype=np.float64), np.empty((d, n), dtype=np.float64)
        acc = np.empty(n, dtype=np.uint32)
        dp = C.POINTER(C.c_double)
        L.check(L.lib().mhx_run_proposal_state(self.h, lam.ctypes.data_as(dp), sd.ctypes.data_as(dp), mean.ctypes.data_as(dp),
                                               acc.ctypes.data_as(C.POINTER(C.c_uint32))))
        return dict(lam=lam, sd=sd, mean=mean, acc_at_freeze=acc)

    def adaptation(self, names=None):
        """the AdaptationTable of an adaptive run: median / min / max of sd over the chains per parameter, the median lam and the pooled
        acceptance rate of the transitions after the proposal froze"""
        ps = self.proposal_state()
        names = names or ["param_%d" % (k + 1) for k in range(self.dim)]
        t = AdaptationTable(dict(parameter=str(names[k]), sd_median=float(np.median(ps["sd"][k])), sd_min=float(ps["sd"][k].min()),
                                 sd_max=float(ps["sd"][k].max())) for k in range(self.dim))
        t.lam_median = float(np.median(ps["lam"]))
        frozen = getattr(self, "_transitions", 0) - self.sampler.adapt.steps
        if frozen > 0:
            cnt = self.state()[2].astype(np.int64) - ps["acc_at_freeze"].astype(np.int64)
            t.accept_rate = float(cnt.sum()) / (float(frozen) * self.n)
        return t

    def accept_rates(self):
        """Metropolis-Hastings acceptance rate of every temperature since init: accepted proposals of the rung's slots over their
        transitions, [R]"""
        R = self.sampler.R
        cnt = self.state()[2].astype(np.float64).reshape(-1, R)
        total = getattr(self, "_transitions", 0)
        return cnt.mean(axis=0) / float(total) if total else np.full(R, np.nan)

    def close(self):
        if self.h:
            L.lib().mhx_run_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DerivedRun(Run):
    """What Run.derive returns: the handle of a derived run (include/mhx.h, mhx_run_derive) -- a device sample tensor and nothing else.
    Every statistic method of Run works on it; what steps or reads sampler state (init, sample, state, set_params, save_state,
    factor, ...) raises the library's refusal (MHX_ESTATE, "... is a derived run").  `source` keeps the run it came from alive (they
    share a context)."""

    def __init__(self, handle, source, nout):
        self.h = handle
        self.source = source
        self.ctx, self.real = source.ctx, source.real
        self.model = self.sampler = None
        self.n, self.dim = source.n, int(nout)
        self.seed = source.seed
        self.kind = "derived"
        self._keep = []

    def samples(self, want_accepted=False):
        """(tensor [n_saved][nout + 1][nchains], None): a derived run holds no accept flags -- they are its source's"""
        if want_accepted:
            return Run.samples(self, True)                  # the library's refusal
        return Run.samples(self, False)


def combine_diagnostics(sum_m, sum_m2, sum_v, n_chains, n_samples):
    """R-hat and between-chain ESS from the (all-reduced) per-parameter sums; see include/mhx.h."""
    Cn, N = float(n_chains), float(n_samples)
    mean = sum_m / Cn
    W = sum_v / Cn
    out = dict(mean=mean, W=W)
    if n_chains > 1:
        Vm = np.maximum((sum_m2 - sum_m * sum_m / Cn) / (Cn - 1.0), 0.0)
        varp = (N - 1.0) / N * W + Vm
        with np.errstate(divide="ignore", invalid="ignore"):
            out["rhat"] = np.sqrt(varp / W)
            out["ess_between"] = Cn * varp / Vm
        out["var_plus"] = varp
    return out


class _ParallelTag:
    """MCMCSerial() / MCMCThreads() / MCMCDistributed() of AbstractMCMC (re-exported, src/AdvancedMH.jl:30) and the
    MCMCHIP() of the Julia glue: accepted as the third positional argument of `sample` for drop-in call sites
    (README.md:141-147, test/runtests.jl:99-108).  On this engine every form runs all chains together on the GPU."""


class MCMCSerial(_ParallelTag):
    pass


class MCMCThreads(_ParallelTag):
    pass


class MCMCDistributed(_ParallelTag):
    pass


class MCMCHIP(_ParallelTag):
    pass


def sample(model, sampler, N, nchains=1, *more, initial_params=None, discard_initial=None, thinning=1, num_warmup=0,
           param_names=None, chain_type=Chains, seed=0, first_chain=0, callback=None, ctx=None, flags=0,
           reduce_lanes=0, progress=False, dtype=None, normal_gen=None, allow_tainted=False):
    """sample(model, sampler, N[, nchains]; kwargs...) -- AbstractMCMC.sample as re-exported by the
    reference (src/AdvancedMH.jl:30).  All chains advance together on the GPU (what
    `sample(model, spl, MCMCThreads(), N, nchains)` does with one task per chain, README.md:141-147).

    dtype: "f64" (default: the reference's Float64) or "f32"; see mhx.set_default_dtype.
    discard_initial defaults to num_warmup [upstream]; `callback(run, i)` is called after each saved
    sample (the reference signature callback(rng, model, sampler, sample, state, i) carries objects
    that live on the device here -- the Run gives access to them).

    allow_tainted: a run of a context that carries a timing probe / fault-injection option of the TOOLS build (mhx_stats.tainted)
    may hold invalid chains; `sample` refuses to wrap it into a container unless this is set (tests of the hooks themselves)."""
    if isinstance(N, _ParallelTag):                 # sample(model, spl, MCMCThreads(), N, nchains)
        if not more:
            raise L.ArgumentError(L.MHX_EINVAL, "sample(model, sampler, parallel, N, nchains): nchains is missing")
        N, nchains = nchains, more[0]
    elif more:
        raise L.ArgumentError(L.MHX_EINVAL, "sample: too many positional arguments")
    if discard_initial is None:
        discard_initial = num_warmup
    if not isinstance(model, DensityModel) and (_is_logdensity_problem(model) or isinstance(model, _TargetSpec)):
        model = LogDensityModel(model)              # sample(problem, sampler, N): AbstractMCMC wraps what implements the interface
    if isinstance(sampler, Tempered):              # sample(model, Tempered(...), N, nladders): R device chains per ladder
        nchains = int(nchains) * sampler.R
        if sampler.adapt is not None and discard_initial < sampler.adapt.steps:
            raise L.ArgumentError(L.MHX_EINVAL, "sample: discard_initial = %d < adapt.steps = %d -- draws taken while the ladder moves are "
                                  "not draws of the target: discard at least the adapting transitions (discard_initial >= adapt.steps)"
                                  % (discard_initial, sampler.adapt.steps))
    adapt = getattr(sampler, "adapt", None) if isinstance(sampler, MetropolisHastings) else None
    if adapt is not None and discard_initial < adapt.steps:
        raise L.ArgumentError(L.MHX_EINVAL, "sample: discard_initial = %d < adapt.steps = %d -- draws taken while the proposal moves are "
                              "not draws of the target: discard at least the adapting transitions (discard_initial >= adapt.steps)"
                              % (discard_initial, adapt.steps))
    run = Run(model, sampler, nchains=nchains, seed=seed, first_chain=first_chain, ctx=ctx, flags=flags,
              reduce_lanes=reduce_lanes, dtype=dtype, normal_gen=normal_gen)
    run.init(initial_params)
    cold = None
    if run.adaptive:
        # the draws stay on the device (the accept-compacted return path is left out for this form) and come back in one copy
        if callback is not None:
            raise L.ArgumentError(L.MHX_EINVAL, "sample: an adaptive run takes no callback")
        run.sample(N, discard_initial, thinning, num_warmup)
        value, acc = run.samples()
    elif run.tempered:
        # the draws stay on the device (the accept-compacted return path does not know swaps): the cold rung is gathered there and
        # only it comes back
        if callback is not None:
            raise L.ArgumentError(L.MHX_EINVAL, "sample: a tempered run takes no callback")
        run.sample(N, discard_initial, thinning, num_warmup)
        cold = run.rung(0)
        value = cold.samples()[0]
        acc = np.ascontiguousarray(run.samples()[1][:, 0::sampler.R])
    elif callback is None:
        # one call: the samples stream to the host while the chains advance (mhx_run_sample_to_host)
        value, acc = run.sample_to_host(N, discard_initial, thinning, num_warmup)
    else:
        # one saved sample per call, so that the callback can look at every state
        chunks, accs = [], []
        dfw = min(num_warmup, discard_initial)
        kfw = num_warmup - dfw
        run.sample(1, discard_initial, 1, dfw)
        v, a = run.samples()
        chunks.append(v), accs.append(a)
        callback(run, 1)
        for i in range(2, N + 1):
            warm = thinning if i <= kfw else 0
            # `thinning` transitions, the last one saved: discard = thinning - 1 ... expressed as
            # N=1, discard_initial=thinning (sample 1 = state after `thinning` transitions)
            run.sample(1, thinning, 1, warm)
            v, a = run.samples()
            chunks.append(v), accs.append(a)
            callback(run, i)
        value, acc = np.concatenate(chunks, axis=0), np.concatenate(accs, axis=0)
    if run.stats()["tainted"] and not allow_tainted:
        raise L.MhxError(L.MHX_ESTATE, "sample: the run's context is tainted (a probe / fault-injection option of the tools build was "
                         "set on it): its chains may be invalid; pass allow_tainted=True to look at them anyway")
    d = model.dim
    if param_names is None:                                         # a NamedTuple of proposals / named parameters carry their names
        param_names = getattr(sampler, "param_names", None) or getattr(model, "param_names", None)
    if param_names is None:
        names = ["param_%d" % (i + 1) for i in range(d)]           # src/AdvancedMH.jl:91
    else:
        names = [str(p) for p in param_names]
        if len(names) != d:
            raise L.ArgumentError(L.MHX_EINVAL, "param_names has the wrong length")
    names = names + ["lp"]
    if chain_type is Chains:
        chain = Chains(value, names, discard_initial + 1, thinning, accepted=acc, stats=run.stats(), state=cold if cold is not None else run)
        if cold is not None:
            chain.tempered = run                                    # the full run: swap_rates(), rung(r), accept_rates()
        if run.adaptive:
            chain.adaptation = run.adaptation(names[:-1])           # what every chain's proposal froze at
        return chain
    if chain_type is np.ndarray:
        return value
    if chain_type is StructArray:
        return StructArray(value, names)
    if chain_type in (Transition, dict):
        # Vector{Transition} (the reference's default container, src/mh-core.jl:76-117) / Vector{NamedTuple}
        # (ext/AdvancedMHStructArraysExt.jl, src/AdvancedMH.jl:96-125: the parameters by name, then lp): one list per chain,
        # the bare list for a single chain
        out = bundle_samples(value, acc, names, chain_type)
        return out[0] if value.shape[2] == 1 else out
    raise L.ArgumentError(L.MHX_EINVAL, "chain_type must be Chains, numpy.ndarray, StructArray, Transition or dict")


class StructArray:
    """chain_type=StructArray (ext/AdvancedMHStructArraysExt.jl; test/runtests.jl:63-73 reads `chain.μ`): one array per
    parameter and `lp`, [iteration] for a single chain, [iteration, chain] otherwise -- views of the sample tensor."""

    def __init__(self, value, names):
        self._names = list(names)
        for k, n in enumerate(self._names):
            col = value[:, k, :]
            self.__dict__[n] = col[:, 0] if value.shape[2] == 1 else col

    def __getitem__(self, name):
        return self.__dict__[name]

    def keys(self):
        return tuple(self._names)

    def __len__(self):
        return len(self.__dict__[self._names[0]])


def bundle_samples(value, accepted, names, chain_type):
    """Host reshaping of the sample tensor value[iteration, parameter (+ lp), chain] into per-chain lists of Transition
    (params, lp, accepted) or of dicts {name: value, ..., "lp": lp} -- what the reference's bundle_samples methods build
    (src/AdvancedMH.jl:96-125)."""
    N, d1, C = value.shape
    out = []
    for c in range(C):
        if chain_type is Transition:
            out.append([Transition(value[i, :d1 - 1, c].copy(), value[i, d1 - 1, c], bool(accepted[i, c]) if accepted is not None else None)
                        for i in range(N)])
        else:
            out.append([dict(zip(names, value[i, :, c].tolist())) for i in range(N)])
    return out
