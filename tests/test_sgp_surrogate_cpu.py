"""Sparse GP as a full surrogate, the parts that need no GPU: the closed-form x-gradients themselves (pinned against central
differences of the CPU oracle: this is the reference the GPU tests hold the library to), argument validation of the new entry
points before any device call, and the C host of tests/c_host/sgp_surrogate_driver.c compiling and linking."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["SquaredExponential", "AbsoluteExponential", "Matern32", "Matern52"]


def problem(n, nz, d, seed=0, noise=0.05):
    """The generator of tests/test_sgp_gpu.py::_problem."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, d)) * 2 - 1
    y = np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, -1]) + noise * rng.standard_normal(n)
    z = x[rng.permutation(n)[:nz]].copy()
    return x, y, z


def analytic_gradients(ref, xq):
    """(d mean / dx, d var / dx, var_raw) of a SparseGpOracle at xq (m, d), raw x, zero trend:
        d mean / dx_k = sigma2 sum_j vec_j dr(x, z_j)/dx_k
        d var  / dx_k = -2 sigma2 sum_j (W kx)_j dr(x, z_j)/dx_k  where var_raw = sigma2 - kx^T W kx >= 1e-15, else 0."""
    from oracle import gp_oracle as O
    from oracle import sgp_oracle as S
    xq = np.atleast_2d(xq)
    kx = S.compute_k(ref.corr, xq, ref.z, ref.w_star, ref.theta, ref.sigma2)            # (m, nz)
    c = kx @ ref.w_inv                                                                    # W symmetric: rows (W kx)^T
    var_raw = ref.sigma2 - (c * kx).sum(axis=1)
    gy, gv = np.empty(xq.shape), np.empty(xq.shape)
    for a in range(xq.shape[0]):
        jac = O.corr_jacobian(ref.corr, xq[a], ref.z, ref.theta, ref.w_star)             # (nz, d)
        gy[a] = ref.sigma2 * ref.w_vec[:, 0] @ jac
        gv[a] = -2.0 * ref.sigma2 * (c[a] @ jac) if var_raw[a] >= 1e-15 else 0.0
    return gy, gv, var_raw


def central_differences(fn, xq, h=1e-5):
    g = np.empty(xq.shape)
    for k in range(xq.shape[1]):
        dq = np.zeros(xq.shape[1])
        dq[k] = h
        g[:, k] = (fn(xq + dq) - fn(xq - dq)) / (2 * h)
    return g


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", range(4))
def test_closed_form_equals_central_differences_of_the_oracle(corr, method):
    """The eight problems of test_sgp_gpu.py::test_likelihood_and_predictions_vs_oracle.  Measured where this was written
    (step 1e-5): mean <= 1.5e-8 (squared exponential), <= 2e-9 (others); variance <= 1.8e-6 (squared exponential, the
    differences being the noisy side), <= 5.7e-9 (others); the bounds below leave a factor of about ten for another libm / BLAS."""
    from oracle import sgp_oracle as S
    x, y, z = problem(700, 40, 3, seed=corr)
    theta, sigma2, noise = np.array([1.3, 0.8, 1.1]), 0.9, 0.02
    ref = S.SparseGpOracle(x, y, z, theta, sigma2, noise, corr=KINDS[corr], method=[S.FITC, S.VFE][method])
    xq = np.random.default_rng(9).random((333, 3)) * 2 - 1
    gy, gv, var_raw = analytic_gradients(ref, xq)
    fy, fv = central_differences(ref.predict, xq), central_differences(ref.predict_var, xq)
    print(f"corr {corr} method {method}: mean {np.abs(gy - fy).max():.3g} var {np.abs(gv - fv).max():.3g} "
          f"clamped {(var_raw < 1e-15).sum()}")
    np.testing.assert_allclose(gy, fy, rtol=0, atol=2e-7)
    np.testing.assert_allclose(gv, fv, rtol=0, atol=2e-5 if corr == 0 else 1e-7)
    clamped = var_raw < 1e-15
    assert np.all(gv[clamped] == 0.0) and np.all(fv[clamped] == 0.0)
    if corr == 0 and method == 1:
        assert clamped.sum() > 50  # the case that exercises the clamp (102 of 333 where this was written)


NEW_ENTRY_POINTS = ["egx_sgp_predict_valvar", "egx_sgp_predict_gradients", "egx_sgp_predict_var_gradients",
                    "egx_sgp_predict_valvar_gradients", "egx_sgp_sample"]


def test_new_entry_points_validate_arguments_before_any_device_call():
    """NULL handle, and NULL arrays with m > 0 (on a handle that is never dereferenced: the check comes first), give
    EGX_ERR_INVALID_VALUE and a message, with or without a GPU."""
    import egobox_amd as egx
    lib = egx._lib.load()
    dp = egx._lib.dptr
    xq, out, out2 = np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 3))
    dummy = C.cast(C.create_string_buffer(4096), C.c_void_p)  # a non-NULL "handle"; no call below may look inside it
    inv = egx._lib.ERR_INVALID_VALUE

    def last():
        return lib.egx_last_error()

    calls = {
        "egx_sgp_predict_valvar": lambda h, x, a, b: lib.egx_sgp_predict_valvar(h, x, 2, a, b),
        "egx_sgp_predict_gradients": lambda h, x, a, b: lib.egx_sgp_predict_gradients(h, x, 2, a),
        "egx_sgp_predict_var_gradients": lambda h, x, a, b: lib.egx_sgp_predict_var_gradients(h, x, 2, a),
        "egx_sgp_predict_valvar_gradients": lambda h, x, a, b: lib.egx_sgp_predict_valvar_gradients(h, x, 2, a, b),
        "egx_sgp_sample": lambda h, x, a, b: lib.egx_sgp_sample(h, x, 2, 3, 0, 1, None, a, None),
    }
    assert sorted(calls) == sorted(NEW_ENTRY_POINTS)
    for name, call in calls.items():
        lib.egx_normalize(dp(np.zeros((1, 2))), 1, 2, None, None, None)  # leaves another message behind
        before = last()
        assert call(None, dp(xq), dp(out), dp(out2)) == inv, name       # NULL handle
        assert last() and b"NULL" in last() and last() != before, name
        assert call(dummy, None, dp(out), dp(out2)) == inv, name        # NULL queries
        assert call(dummy, dp(xq), None, dp(out2)) == inv, name         # NULL first result
    assert lib.egx_sgp_predict_valvar(dummy, dp(xq), 2, dp(out), None) == inv
    assert lib.egx_sgp_predict_valvar_gradients(dummy, dp(xq), 2, dp(out), None) == inv


def test_sgp_surrogate_c_host_compiles_and_links(tmp_path):
    """tests/c_host/sgp_surrogate_driver.c uses the header alone; without a GPU it reports that and exits with 77."""
    src = os.path.join(ROOT, "tests", "c_host", "sgp_surrogate_driver.c")
    exe = tmp_path / "sgp_surrogate_driver"
    libdir = os.path.join(ROOT, "egobox_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}", src, f"-L{libdir}",
                    "-legx_gp_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    import torch
    if not torch.cuda.is_available():
        out = subprocess.run([str(exe)], capture_output=True, text=True)
        assert out.returncode == 77, out  # no HIP device: nothing computes without a GPU
