"""ctypes binding of libegx_gp_hip.so (include/egx_gp.h).

This is the same C ABI a Rust `extern "C"` shim would bind.  The library is
built in-tree by `__graft_entry__.build()` / `make -C egobox_amd/csrc`; if it is missing the
import fails loudly -- there is no Python or CPU fallback for the compute path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libegx_gp_hip.so")
#: the same library built with -DEGX_TEST_HOOKS (the "pipe_stall" knob, grid / trace overrides of the chain launch): loaded
#: instead of the product library only when EGX_TEST_LIBRARY=1 is set -- by tests that force a hand-off to fail, in a
#: process of their own.  Never the default, never used by bench.py.
TEST_LIB_PATH = os.path.join(_HERE, "lib", "_dev", "libegx_gp_hip_testhooks.so")
#: EGX_TEST_LIBRARY=trace: the profiling build with per-tile stamps in the left-looking group updates (tools/dev_build.sh trace;
#: tools/long_update_attribution.py) -- built by hand, never by build(), never the default
TRACE_LIB_PATH = os.path.join(_HERE, "lib", "_dev", "libegx_gp_hip_trace.so")

# sampling methods (egx_sample_method)
SAMPLE_CHOLESKY, SAMPLE_PSD = 0, 1

# return codes / status values (egx_rc, egx_status)
SUCCESS, ERR_INVALID_VALUE, ERR_NO_DEVICE, ERR_HIP, ERR_NOT_FITTED, ERR_LINALG, ERR_LIKELIHOOD, ERR_UNSUPPORTED, ERR_PEER, \
    ERR_NO_FINITE_START = range(10)
STATUS_OK, STATUS_NOT_POSITIVE_DEFINITE, STATUS_ILL_CONDITIONED_FT, STATUS_ILL_CONDITIONED_F, STATUS_NAN_THETA, STATUS_RANK_FAILED = range(6)

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_int64_p = C.POINTER(C.c_int64)


class GpConfig(C.Structure):
    _fields_ = [("corr", C.c_int32), ("mean", C.c_int32), ("nugget", C.c_double), ("device", C.c_int32),
                ("n_workspaces", C.c_int32), ("w_star", c_double_p), ("kpls_dim", C.c_int64)]


class InnerView(C.Structure):
    _fields_ = [(k, c_double_p) for k in (
        "theta", "likelihood", "sigma2", "beta", "gamma", "r_chol", "ft", "ft_qr_r", "x_mean", "x_std",
        "y_mean", "y_std", "xt_norm", "yt_norm")]


class SgpConfig(C.Structure):
    _fields_ = [("corr", C.c_int32), ("method", C.c_int32), ("nugget", C.c_double), ("device", C.c_int32)]


class PlsPlan(C.Structure):
    """egx_pls_plan"""
    _fields_ = [(k, C.c_int64) for k in ("n", "d", "chunk_rows", "n_chunks", "tiles", "out_tiles", "block_side", "blocks")]


class InfillConfig(C.Structure):
    _fields_ = [("criterion", C.c_int32), ("feasibility", C.c_int32), ("fmin", C.c_double), ("sigma_weight", C.c_double),
                ("scale_ic", C.c_double), ("scale", C.c_double)]


class GmmConfig(C.Structure):
    _fields_ = [("n_clusters", C.c_int32), ("n_runs", C.c_int32), ("max_iter", C.c_int32), ("device", C.c_int32),
                ("tol", C.c_double), ("reg_covar", C.c_double)]


class InfillParts(C.Structure):
    _fields_ = [(k, c_double_p) for k in ("mean", "var", "grad_mean", "grad_var")]


class InfillSurrogate(C.Structure):
    _fields_ = [("experts", C.POINTER(C.c_void_p)), ("n_experts", C.c_int32), ("weights", c_double_p), ("means", c_double_p),
                ("precisions_chol", c_double_p), ("heaviside_factor", C.c_double), ("smooth", C.c_int32)]


#: egx_model_kind
MODEL_GP, MODEL_SGP = 0, 1


class ModelRef(C.Structure):
    """egx_model_ref"""
    _fields_ = [("kind", C.c_int32), ("handle", C.c_void_p)]


class InfillSurrogateAny(C.Structure):
    """egx_infill_surrogate_any"""
    _fields_ = [("experts", C.POINTER(ModelRef)), ("n_experts", C.c_int32), ("weights", c_double_p), ("means", c_double_p),
                ("precisions_chol", c_double_p), ("heaviside_factor", C.c_double), ("smooth", C.c_int32)]


class InfillStats(C.Structure):
    _fields_ = [("rounds", C.c_int64), ("best_start", C.c_int64), ("evals", c_int64_p)]


class InfillCstrStats(C.Structure):
    _fields_ = [("rounds", C.c_int64), ("best_start", C.c_int64), ("feasible", C.c_int32), ("violation", C.c_double),
                ("evals", c_int64_p)]


class InfillSlsqpStats(C.Structure):
    """egx_infill_slsqp_stats"""
    _fields_ = [("rounds", C.c_int64), ("best_start", C.c_int64), ("feasible", C.c_int32), ("violation", C.c_double),
                ("evals", c_int64_p), ("stop", c_int32_p)]


class InfillBatchConfig(C.Structure):
    """egx_infill_batch_config"""
    _fields_ = [("strategy", C.c_int32), ("optimizer", C.c_int32), ("max_eval", C.c_int64), ("scaling_points", c_double_p),
                ("n_scaling", C.c_int64)]


class XTypeC(C.Structure):
    """egx_xtype"""
    _fields_ = [("kind", C.c_int32), ("n", C.c_int32), ("lo", C.c_double), ("hi", C.c_double), ("values", c_double_p)]


_XT_P = C.POINTER(XTypeC)


class Timings(C.Structure):
    _fields_ = [("corr_build_ms", C.c_double), ("potrf_ms", C.c_double), ("potrf_syrk_ms", C.c_double),
                ("solve_ms", C.c_double), ("host_ms", C.c_double), ("total_ms", C.c_double),
                ("potrf_flops", C.c_int64), ("corr_bytes", C.c_int64), ("syrk_launches", C.c_int64),
                ("syrk_flops", C.c_int64)]


#: every symbol include/egx_gp.h declares: (name, restype, argtypes)
SIGNATURES = [
    ("egx_abi_version", C.c_int32, []),
    ("egx_last_error", C.c_char_p, []),
    ("egx_device_count", C.c_int32, []),
    ("egx_gp_config_default", None, [C.POINTER(GpConfig)]),
    ("egx_trim", C.c_int64, []),
    ("egx_set_tuning", C.c_int32, [C.c_char_p, C.c_int32, c_int32_p]),
    ("egx_pool_stats", None, [c_int64_p, c_int64_p, c_int64_p]),
    ("egx_chain_stats", None, [c_int64_p, c_int64_p]),
    ("egx_normalize", C.c_int32, [c_double_p, C.c_int64, C.c_int64, c_double_p, c_double_p, c_double_p]),
    ("egx_regression_ncols", C.c_int64, [C.c_int32, C.c_int64]),
    ("egx_regression_basis", C.c_int32, [C.c_int32, c_double_p, C.c_int64, C.c_int64, c_double_p]),
    ("egx_mixint_unfolded_dim", C.c_int32, [_XT_P, C.c_int32, c_int64_p]),
    ("egx_mixint_continuous_limits", C.c_int32, [_XT_P, C.c_int32, c_double_p]),
    ("egx_mixint_unfold", C.c_int32, [_XT_P, C.c_int32, c_double_p, C.c_int64, c_double_p]),
    ("egx_mixint_fold", C.c_int32, [_XT_P, C.c_int32, c_double_p, C.c_int64, c_double_p]),
    ("egx_mixint_cast", C.c_int32, [_XT_P, C.c_int32, c_double_p, C.c_int64, c_double_p]),
    ("egx_mixint_to_discrete", C.c_int32, [_XT_P, C.c_int32, c_double_p, C.c_int64, c_double_p]),
    ("egx_gp_set_xtypes", C.c_int32, [C.c_void_p, _XT_P, C.c_int32]),
    ("egx_gp_get_xtypes", C.c_int32, [C.c_void_p, _XT_P, C.c_int32, c_int32_p, c_double_p, c_int64_p]),
    ("egx_gmx_predict_probas_mixint", C.c_int32, [C.c_int32, c_double_p, c_double_p, c_double_p, C.c_int64, C.c_int64, C.c_double,
                                                  c_double_p, C.c_int64, c_double_p, _XT_P, C.c_int32]),
    ("egx_gmx_predict_probas_derivatives_mixint", C.c_int32, [C.c_int32, c_double_p, c_double_p, c_double_p, C.c_int64, C.c_int64,
                                                              C.c_double, c_double_p, C.c_int64, c_double_p, _XT_P, C.c_int32]),
    ("egx_gp_create", C.c_int32, [C.POINTER(GpConfig), c_double_p, c_double_p, C.c_int64, C.c_int64,
                                  C.POINTER(C.c_void_p)]),
    ("egx_gp_destroy", None, [C.c_void_p]),
    ("egx_gp_dims", C.c_int32, [C.c_void_p, c_int64_p, c_int64_p, c_int64_p, c_int64_p]),
    ("egx_gp_get_training_data", C.c_int32, [C.c_void_p, c_double_p, c_double_p]),
    ("egx_gp_likelihood", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_int32_p]),
    ("egx_gp_likelihood_batch", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, C.c_int64, c_double_p, c_int32_p]),
    ("egx_gp_set_lockstep", C.c_int32, [C.c_void_p, C.c_int32]),
    ("egx_gp_get_lockstep", C.c_int32, [C.c_void_p]),
    ("egx_gp_get_schedule", C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]),
    ("egx_gp_shrink", C.c_int32, [C.c_void_p, C.c_int32]),
    ("egx_gp_likelihood_grad", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_double_p, c_int32_p]),
    ("egx_gp_likelihood_grad_batch", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, C.c_int64, c_double_p, c_double_p,
                                                 c_int32_p]),
    ("egx_gp_finalize", C.c_int32, [C.c_void_p, c_double_p, C.c_int64]),
    ("egx_gp_create_group", C.c_int32, [C.c_void_p, c_double_p, c_double_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]),
    ("egx_gp_finalize_multi", C.c_int32, [C.POINTER(C.c_void_p), C.c_int32, c_double_p, C.c_int64]),
    ("egx_gp_likelihood_multi", C.c_int32, [C.POINTER(C.c_void_p), C.c_int32, c_double_p, C.c_int64, c_double_p, C.POINTER(C.c_int32)]),
    ("egx_gp_fit_multi", C.c_int32, [C.POINTER(C.c_void_p), C.c_int32, c_double_p, C.c_int64, c_double_p, c_double_p, C.c_int64, C.c_int64,
                                     c_int64_p]),
    ("egx_gp_likelihood_grad_multi", C.c_int32, [C.POINTER(C.c_void_p), C.c_int32, c_double_p, C.c_int64, c_double_p, c_double_p,
                                                 C.POINTER(C.c_int32)]),
    ("egx_gp_fit_lbfgs_multi", C.c_int32, [C.POINTER(C.c_void_p), C.c_int32, c_double_p, C.c_int64, c_double_p, c_double_p, C.c_int64,
                                           C.c_int64, c_int64_p]),
    ("egx_gp_fit", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_double_p, C.c_int64, C.c_int64,
                               c_int64_p]),
    ("egx_gp_fit_partial", C.c_int32, [C.c_void_p, c_double_p, c_int64_p, C.c_int64, c_double_p, C.c_int64, c_double_p,
                                       c_double_p, C.c_int64, C.c_int64, c_int64_p]),
    ("egx_gp_fit_lbfgs", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_double_p, C.c_int64, C.c_int64,
                                     c_int64_p]),
    ("egx_gp_predict", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p]),
    ("egx_gp_predict_var", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p]),
    ("egx_gp_predict_valvar", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_double_p]),
    ("egx_gp_predict_valvar_multi", C.c_int32, [C.POINTER(C.c_void_p), C.c_int32, c_double_p, C.c_int64, c_double_p, c_double_p]),
    ("egx_gp_predict_gradients", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p]),
    ("egx_gp_predict_var_gradients", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p]),
    ("egx_gp_predict_valvar_gradients", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_double_p]),
    ("egx_gp_predict_valvar_gradients_multi", C.c_int32, [C.POINTER(C.c_void_p), C.c_int32, c_double_p, C.c_int64, c_double_p,
                                                          c_double_p]),
    ("egx_gp_predict_covariance", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p]),
    ("egx_gp_sample", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, C.c_int64, C.c_int32, C.c_uint64, c_double_p, c_double_p,
                                  c_double_p]),
    ("egx_random_normals", C.c_int32, [C.c_int32, C.c_uint64, C.c_int64, C.c_int64, c_double_p]),
    ("egx_gp_get_inner", C.c_int32, [C.c_void_p, C.POINTER(InnerView)]),
    ("egx_gp_set_inner", C.c_int32, [C.c_void_p, C.POINTER(InnerView)]),
    ("egx_corr_matrix", C.c_int32, [C.c_int32, c_double_p, C.c_int64, C.c_int64, c_double_p, C.c_double, c_double_p]),
    ("egx_cross_corr", C.c_int32, [C.c_int32, c_double_p, C.c_int64, c_double_p, C.c_int64, C.c_int64, c_double_p,
                                   c_double_p]),
    ("egx_potrf", C.c_int32, [c_double_p, C.c_int64, c_int32_p]),
    ("egx_sweep_unique_id", C.c_int32, [C.c_void_p]),
    ("egx_sweep_create", C.c_int32, [C.POINTER(GpConfig), c_double_p, c_double_p, C.c_int64, C.c_int64, C.c_void_p,
                                     C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    ("egx_sweep_destroy", None, [C.c_void_p]),
    ("egx_sweep_handle", C.c_void_p, [C.c_void_p]),
    ("egx_sweep_info", C.c_int32, [C.c_void_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_int64_p]),
    ("egx_sweep_likelihood", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, C.c_int64, c_double_p, c_int32_p]),
    ("egx_sweep_set_assignment", C.c_int32, [C.c_void_p, C.c_int32]),
    ("egx_sweep_last_balance", C.c_int32, [C.c_void_p, c_int64_p, c_double_p]),
    ("egx_sweep_allgather", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p]),
    ("egx_sweep_fit", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_double_p, C.c_int64, C.c_int64, c_int64_p]),
    ("egx_moe_predict_valvar", C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), c_int32_p, C.c_int64, C.c_int64, c_double_p,
                                           c_double_p, C.c_int64, C.c_int64, C.c_int32, c_double_p, c_double_p]),
    ("egx_gmx_precisions_chol", C.c_int32, [c_double_p, C.c_int64, C.c_int64, c_double_p]),
    ("egx_gmx_predict_probas", C.c_int32, [C.c_int32, c_double_p, c_double_p, c_double_p, C.c_int64, C.c_int64, C.c_double,
                                           c_double_p, C.c_int64, c_double_p]),
    ("egx_gmx_predict_probas_derivatives", C.c_int32, [C.c_int32, c_double_p, c_double_p, c_double_p, C.c_int64, C.c_int64,
                                                       C.c_double, c_double_p, C.c_int64, c_double_p]),
    ("egx_gmm_config_default", None, [C.POINTER(GmmConfig)]),
    ("egx_gmm_fit", C.c_int32, [C.POINTER(GmmConfig), c_double_p, C.c_int64, C.c_int32, c_double_p, c_double_p, c_double_p,
                                c_double_p, c_double_p, c_int32_p, c_int32_p, c_int32_p, c_double_p, c_double_p, c_double_p]),
    ("egx_gmm_fit_wide", C.c_int32, [C.POINTER(GmmConfig), c_double_p, C.c_int64, C.c_int32, c_double_p, c_double_p, c_double_p,
                                     c_double_p, c_double_p, c_int32_p, c_int32_p, c_int32_p, c_double_p, c_double_p,
                                     c_double_p]),
    ("egx_moe_predict_valvar_gradients", C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), c_int32_p, C.c_int64, C.c_int64,
                                                     c_double_p, c_double_p, c_double_p, C.c_int64, C.c_int64, C.c_int32,
                                                     c_double_p, c_double_p]),
    ("egx_gp_last_timings", C.c_int32, [C.c_void_p, C.POINTER(Timings)]),
    ("egx_mfma_probe", C.c_int32, [c_double_p]),
    ("egx_sgp_config_default", None, [C.POINTER(SgpConfig)]),
    ("egx_sgp_create", C.c_int32, [C.POINTER(SgpConfig), c_double_p, c_double_p, C.c_int64, C.c_int64, c_double_p,
                                   C.c_int64, C.POINTER(C.c_void_p)]),
    ("egx_sgp_destroy", None, [C.c_void_p]),
    ("egx_sgp_dims", C.c_int32, [C.c_void_p, c_int64_p, c_int64_p, c_int64_p]),
    ("egx_sgp_likelihood", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, C.c_double, C.c_double, c_double_p, c_int32_p]),
    ("egx_sgp_finalize", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, C.c_double, C.c_double]),
    ("egx_sgp_fit", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_double_p, C.c_int32, C.c_double,
                                C.c_int64, c_int64_p]),
    ("egx_sgp_likelihood_grad", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, C.c_double, C.c_double, c_double_p, c_double_p,
                                            c_int32_p]),
    ("egx_sgp_fit_lbfgs", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_double_p, C.c_int32, C.c_double,
                                      C.c_int64, c_int64_p]),
    ("egx_sgp_likelihood_grad_z", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, C.c_double, C.c_double, c_double_p, c_double_p,
                                              c_double_p, c_int32_p]),
    ("egx_sgp_set_inducings", C.c_int32, [C.c_void_p, c_double_p]),
    ("egx_sgp_get_inducings", C.c_int32, [C.c_void_p, c_double_p]),
    ("egx_sgp_set_w_star", C.c_int32, [C.c_void_p, c_double_p, C.c_int64]),
    ("egx_sgp_get_w_star", C.c_int32, [C.c_void_p, c_double_p, c_int64_p]),
    ("egx_pls_rotations", C.c_int32, [C.c_int32, c_double_p, c_double_p, C.c_int64, C.c_int64, C.c_int64, c_double_p, c_int32_p]),
    ("egx_sgp_compute_w_star", C.c_int32, [C.c_void_p, C.c_int64]),
    ("egx_sgp_pls_launch_ms", C.c_int32, [C.c_void_p, c_double_p]),
    ("egx_pls_get_plan", C.c_int32, [C.c_int64, C.c_int64, C.POINTER(PlsPlan)]),
    ("egx_sgp_fit_lbfgs_z", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_double_p, C.c_int32, C.c_double,
                                        C.c_int64, c_double_p, c_double_p, C.c_int64, c_int64_p]),
    ("egx_sgp_predict", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p]),
    ("egx_sgp_predict_var", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p]),
    ("egx_sgp_predict_valvar", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_double_p]),
    ("egx_sgp_predict_gradients", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p]),
    ("egx_sgp_predict_var_gradients", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p]),
    ("egx_sgp_predict_valvar_gradients", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_double_p]),
    ("egx_sgp_sample", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, C.c_int64, C.c_int32, C.c_uint64, c_double_p, c_double_p,
                        c_double_p]),
    ("egx_sgp_get_state", C.c_int32, [C.c_void_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    ("egx_infill_config_default", None, [C.POINTER(InfillConfig)]),
    ("egx_infill_create", C.c_int32, [C.POINTER(InfillConfig), C.c_void_p, C.POINTER(C.c_void_p), c_double_p, C.c_int32,
                                      C.POINTER(C.c_void_p)]),
    ("egx_infill_destroy", None, [C.c_void_p]),
    ("egx_infill_set_params", C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32]),
    ("egx_infill_get_params", C.c_int32, [C.c_void_p, C.POINTER(InfillConfig)]),
    ("egx_infill_eval", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_double_p, C.POINTER(InfillParts)]),
    ("egx_infill_scaling", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_double_p, c_double_p]),
    ("egx_infill_optimize", C.c_int32, [C.c_void_p, c_double_p, c_double_p, c_double_p, C.c_int64, C.c_int64, c_double_p,
                                        c_double_p, C.POINTER(InfillStats)]),
    ("egx_infill_set_cstr_strategy", C.c_int32, [C.c_void_p, C.c_int32, c_double_p]),
    ("egx_infill_get_cstr_strategy", C.c_int32, [C.c_void_p, c_int32_p, c_double_p]),
    ("egx_infill_eval_cstr", C.c_int32, [C.c_void_p, c_double_p, C.c_int64, c_double_p, c_double_p, c_double_p, c_double_p]),
    ("egx_infill_optimize_cstr", C.c_int32, [C.c_void_p, c_double_p, c_double_p, c_double_p, C.c_int64, C.c_int64, c_double_p,
                                             c_double_p, c_double_p, C.POINTER(InfillCstrStats)]),
    ("egx_infill_optimize_slsqp", C.c_int32, [C.c_void_p, c_double_p, c_double_p, c_double_p, C.c_int64, C.c_int64, c_double_p,
                                              c_double_p, c_double_p, C.POINTER(InfillSlsqpStats)]),
    ("egx_infill_create_mix", C.c_int32, [C.POINTER(InfillConfig), C.POINTER(InfillSurrogate), c_double_p, C.c_int32,
                                          C.POINTER(C.c_void_p)]),
    ("egx_infill_eval_experts", C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_int64, c_double_p, c_double_p, c_double_p,
                                            c_double_p, c_double_p, c_double_p]),
    ("egx_infill_create_any", C.c_int32, [C.POINTER(InfillConfig), C.POINTER(InfillSurrogateAny), c_double_p, C.c_int32,
                                          C.POINTER(C.c_void_p)]),
    ("egx_moe_predict_valvar_sgp", C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), c_int32_p, C.c_int64, C.c_int64, c_double_p,
                                               c_double_p, C.c_int64, C.c_int64, C.c_int32, c_double_p, c_double_p]),
    ("egx_moe_predict_valvar_gradients_sgp", C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), c_int32_p, C.c_int64, C.c_int64,
                                                         c_double_p, c_double_p, c_double_p, C.c_int64, C.c_int64, C.c_int32,
                                                         c_double_p, c_double_p]),
    ("egx_infill_push_pending", C.c_int32, [C.c_void_p, c_double_p, c_double_p]),
    ("egx_infill_clear_pending", C.c_int32, [C.c_void_p]),
    ("egx_infill_get_pending", C.c_int32, [C.c_void_p, c_int32_p, c_double_p, c_double_p, c_double_p]),
    ("egx_infill_virtual_point", C.c_int32, [C.c_void_p, c_double_p, C.c_int32, c_double_p]),
    ("egx_infill_batch_config_default", None, [C.POINTER(InfillBatchConfig)]),
    ("egx_infill_optimize_batch", C.c_int32, [C.c_void_p, C.POINTER(InfillBatchConfig), c_double_p, c_double_p, c_double_p,
                                              C.c_int64, C.c_int32, c_double_p, c_double_p, c_double_p, c_int32_p]),
    ("egx_infill_set_active", C.c_int32, [C.c_void_p, c_int32_p, C.c_int32, c_double_p]),
    ("egx_infill_clear_active", C.c_int32, [C.c_void_p]),
    ("egx_infill_get_active", C.c_int32, [C.c_void_p, c_int32_p, c_int32_p, c_double_p]),
    ("egx_infill_get_runs", C.c_int32, [C.c_void_p, c_int32_p, c_int32_p]),
]


class EgxError(RuntimeError):
    """Base error; `.rc` is the egx_rc.  Subclasses mirror GpError (crates/gp/src/errors.rs:8-40)."""

    def __init__(self, rc, msg):
        super().__init__(msg)
        self.rc = rc


class InvalidValueError(EgxError, ValueError):
    pass


class NoDeviceError(EgxError):
    pass


class NotFittedError(EgxError):
    pass


class LinalgError(EgxError):
    pass


class LikelihoodComputationError(EgxError):
    pass


class PeerError(EgxError):
    """A collective call in which another rank failed or did not answer (EGX_ERR_PEER)."""


class SampleError(EgxError, ValueError):
    """MoeError::SampleError (crates/moe/src/errors.rs:30): a mixture of several clusters cannot be sampled."""


class ClusteringError(EgxError, ValueError):
    """MoeError::ClusteringError (crates/moe/src/errors.rs): no usable clustering -- every restart of the mixture's
    training failed, or a cluster is left with fewer than three points."""


_ERR = {ERR_INVALID_VALUE: InvalidValueError, ERR_NO_DEVICE: NoDeviceError, ERR_NOT_FITTED: NotFittedError,
        ERR_LINALG: LinalgError, ERR_LIKELIHOOD: LikelihoodComputationError, ERR_PEER: PeerError}

_lib = None


def load():
    """Load (once) and type the shared library.  Raises ImportError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    which = os.environ.get("EGX_TEST_LIBRARY")
    if which == "1":
        path = TEST_LIB_PATH
    elif which == "trace":
        path = TRACE_LIB_PATH
    elif which:  # any other scratch build of tools/dev_build.sh <name> <defines>: A/B measurements (tools/ab_lib.py)
        path = os.path.join(_HERE, "lib", "_dev", f"libegx_gp_hip_{which}.so")
    else:
        path = LIB_PATH
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C egobox_amd/csrc`).  egobox_amd has no fallback compute path.")
    lib = C.CDLL(path)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != SUCCESS:
        msg = load().egx_last_error().decode("utf-8", "replace")
        raise _ERR.get(rc, EgxError)(rc, msg)


def dptr(a):
    return a.ctypes.data_as(c_double_p)


def as_f64(a, ndim=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if ndim is not None and a.ndim != ndim:
        raise InvalidValueError(ERR_INVALID_VALUE, f"expected a {ndim}-d array, got shape {a.shape}")
    return a
