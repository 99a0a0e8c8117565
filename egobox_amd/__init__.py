"""egobox_amd -- MI355X-native (gfx950) kriging hot path behind egobox-gp's builder / fit / predict API.

Importing the package loads `egobox_amd/lib/libegx_gp_hip.so` (C ABI: include/egx_gp.h); the import fails
if the library has not been built, and model construction fails with NoDeviceError without a GPU: there is
no CPU or PyTorch fallback for the compute path.
"""
from . import _lib
from ._lib import (ClusteringError, EgxError, InvalidValueError, LikelihoodComputationError, LinalgError, NoDeviceError,
                   NotFittedError, PeerError, SampleError)

_lib.load()  # fail loudly at import when the HIP library is missing

from .gp import (AbsoluteExponentialCorr, ConstantMean, GaussianProcess, GpHandle, GpParams, Kriging,  # noqa: E402
                 LinearMean, Matern32Corr, Matern52Corr, QuadraticMean, SquaredExponentialCorr, ThetaTuning,
                 chain_stats, corr_matrix, cross_corr, finalize_multi, fit_lbfgs_multi, fit_multi, likelihood_grad_multi,
                 likelihood_multi, mfma_probe, normalize, pool_stats, potrf,
                 predict_valvar_gradients_multi, predict_valvar_multi, regression_basis, set_tuning, trim)
from .gpx import CorrelationSpec, GpMix, Gpx, Recombination, RegressionSpec  # noqa: E402
from .multistart import prepare_multistart, theta_sweep_candidates  # noqa: E402
from .sgp import (Inducings, ParamTuning, SgpHandle, SgpParams, SparseGaussianProcess, SparseGpMix, SparseGpx,  # noqa: E402
                  SparseMethod)
from . import cv, infill, moe, workload  # noqa: E402
from .cv import GpMetrics, IaeAlphaPlotData, cross_validate, fold_indices  # noqa: E402
from .moe import GaussianMixture, GpMixture, GpMixtureParams  # noqa: E402
from .infill import EI, LOG_EI, WB2, WB2S, InfillObjective, QEiStrategy  # noqa: E402
from . import mixint  # noqa: E402
from .mixint import (MixintContext, MixintGpMixture, MixintGpMixtureParams, XType, as_continuous_limits,  # noqa: E402
                     cast_to_discrete_values, fold_with_enum_index, to_continuous_space, to_discrete_space, unfold_with_enum_mask)
from . import doe, egor  # noqa: E402
from .doe import FullFactorial, Lhs, Random, Sampling, lhs, sampling  # noqa: E402
from .egor import Egor, GpConfig, OptimResult  # noqa: E402
from .sweep import Sweep, best_candidate, rendezvous_sweep, shard_indices, sweep_likelihood  # noqa: E402

__all__ = [n for n in dir() if not n.startswith("_")]
