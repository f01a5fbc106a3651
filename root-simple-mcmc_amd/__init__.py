"""root-simple-mcmc_amd: MI355X-native many-chain adaptive Metropolis engine.

Drop-in for one path of ClarkMcGrew/root-simple-mcmc: the
sMCMC::TSimpleMCMC<L, TProposeAdaptiveStep>::Step() loop.  The directory name has
a hyphen, so import it through the loader at the repo root:

    from smcmc_amd_loader import load_package
    smcmc = load_package()          # module object, registered as "root_simple_mcmc_amd"
"""
from ._capi import (LIKE_ASYM, LIKE_CONSTRAINED, LIKE_EVENT_SAMPLE, LIKE_EVENT_SHAPE, LIKE_EVENT_TEMPLATE, LIKE_HORRIFIC, LIKE_ISO_GAUSS, LIKE_QUADFORM, LIKE_ROSENBROCK, LIKE_USER, MODE_FROZEN, MODE_PER_CHAIN, MODE_POOLED, SmcmcError,  # noqa: F401
                    LIB_PATH, SIGNATURES, HMC_RECORD_FIELDS, VAAT_RECORD_FIELDS, load)
from .engine import Autocorrelation, AutocorrelationGrid, AutocorrelationPlan, Convergence, Engine, HmcEngine, MacroAutocorrelation, Marginals, PosteriorMoments, PosteriorPredictive, PredictiveCheck, TraceMoments, TraceQuantiles, VaatEngine, autocorrelation_plan, cholesky_chain, event_predictive, order_keys, order_statistics_combined, order_values, poisson_draw, predictive_check, quantile_ranks, trace_digit_counts, event_sample_evaluate, event_sample_params, event_shape_evaluate, event_shape_kernel, event_shape_params, event_template_evaluate, selftest_detmath, selftest_hmc_error_matrix, selftest_mfma, selftest_mfma_strip  # noqa: F401
from . import build as _build_mod  # noqa: F401
from . import distributed  # noqa: F401


def build(**kw):
    """Compile the HIP library in-tree (hipcc, gfx950)."""
    return _build_mod.build(**kw)


FROZEN_DEFINITION_LIB_PATH = _build_mod.FROZEN_LIB_PATH


def build_frozen_definition():
    """The test library of the frozen-definition golden set (build.py build_frozen_definition); call after build()."""
    return _build_mod.build_frozen_definition()
