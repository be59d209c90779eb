"""mhx -- Python host mirror of the AdvancedMH.jl API over libmhx.so (MI355X / gfx950 HIP kernels)."""
from ._lib import (ArgumentError, Context, MhxError, PosDefException, FLAG_GENERIC, FLAG_NO_JIT, FLAG_EMCEE_SEQUENTIAL, FLAG_ZIGGURAT, FLAG_DENSE_FACTOR, FLAG_RAM_DEFERRED, FLAG_SYMMETRIC_PROPOSAL, LIB_PATH,
                   EXPORTS, MHX_EINVAL, MHX_ESTATE, Schedule, check, host_array, lib, get_default_dtype, set_default_dtype, use_library, TOOLS_LIB_PATH)
from .dist import Group
from .api import (I, Banana, Cauchy, Chains, ComponentProposal, CompositeProposal, ConditionalProposal, CorrGaussian, DensityModel, Ensemble, Exponential, Funnel, Gamma, HipLogDensity, IIDNormal,
                  InverseGamma, IsoGaussian, Laplace, LogDensityModel, MALA, MCMCDistributed, MCMCHIP, MCMCSerial, MCMCThreads, MetropolisHastings, MvNormal, NamedProposals, Normal, RandomWalkProposal,
                  RobustAdaptiveMetropolis, Run, RWMH, StaticMH, StaticProposal, StructArray, combine_diagnostics, StretchProposal,
                  correlation_from_covariance, covariance_from_moments, hpd_ranks, Corner, density_binning_bound, density_from_counts, histogram_edges,
                  silverman_bandwidth, ACF_TILE, AutocorTable, autocorrelation, integrated_time, HipMap, HipPredictive, DerivedRun,
                  HipPointwise, PointwiseSums, PointwiseTable, merge_pointwise, pointwise_table, waic_from_table, dic_from_table,
                  PsisResult, LooTable, LooResult, CompareTable, loo_table, loo_from_table, compare, psis_tail_length, khat_threshold,
                  SymmetricRandomWalkProposal, SymmetricStaticProposal, TDist, Transition, Uniform, bundle_samples,
                  Tempered, LadderAdaptation, ProposalAdaptation, AdaptationTable, SwapTable, LadderTable, geometric_betas, power_betas, EvidenceResult, evidence_from_table,
                  bayes_factor, logdensity, pack_lower, sample, unpack_lower, zeros)
from . import trace


def set_option(name, value):
    """An explicit engine option (mhx_ctx_set_option; include/mhx.h lists them) on the default contexts; None unsets."""
    Context.set_default_option(name, value)


def clear_options():
    Context.clear_default_options()


__all__ = [n for n in dir() if not n.startswith("_")]
