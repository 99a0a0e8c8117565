"""The sparse GP's closed-form likelihood gradient without a GPU: the numpy restatement (tests/sgp_grad_oracle.py, dense
n x n algebra) against central differences of the CPU oracle's likelihood (oracle/sgp_oracle.py fitc / vfe), the host-only
L-BFGS machine (csrc/lbfgs.h) on a quadratic with an active bound, and the two new symbols of the built library."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sgp_grad_oracle as GO  # noqa: E402
from oracle import sgp_oracle as S  # noqa: E402

N, NZ, D = 130, 17, 3
THETA, SIGMA2, NOISE, NUGGET = np.array([1.3, 0.8, 1.1]), 0.9, 0.02, 1e-8


def _problem(n, nz, d, seed=0, noise=0.05):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d)) * 2 - 1
    y = np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, -1]) + noise * rng.standard_normal(n)
    z = x[rng.permutation(n)[:nz]].copy()
    return x, y, z


@pytest.fixture(scope="module")
def problem():
    return _problem(N, NZ, D, seed=N)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", range(4))
def test_restatement_matches_central_differences_of_the_oracle(problem, corr, method):
    """Relative step 1e-6 per component (1e-7 for the noise); bar 1e-6 of max(1, |difference quotient|): the closed form has
    rounding error ~1e-13 here, the quotient's own noise is eps |L| / step ~ 1e-8 (measured 1e-7 at the worst), and the
    factor left is for other seeds."""
    x, y, z = problem
    fn = S.fitc if method == 0 else S.vfe

    def lkh(p):
        return fn(GO.KINDS[corr], p[:D], p[D], p[D + 1], np.eye(D), x, y.reshape(-1, 1), z, NUGGET)[0]

    p0 = np.concatenate([THETA, [SIGMA2, NOISE]])
    fd = np.zeros(D + 2)
    for i in range(D + 2):
        h = p0[i] * (1e-7 if i == D + 1 else 1e-6)
        pp, pm = p0.copy(), p0.copy()
        pp[i] += h
        pm[i] -= h
        fd[i] = (lkh(pp) - lkh(pm)) / (2.0 * h)
    got = GO.likelihood_grad(corr, method, x, y, z, THETA, SIGMA2, NOISE, NUGGET)
    dev = np.abs(got - fd) / np.maximum(1.0, np.abs(fd))
    print(f"corr {corr} method {method}: worst deviation {dev.max():.3e}")
    assert got.shape == (D + 2,)
    assert dev.max() <= 1e-6, (got, fd)


@pytest.mark.parametrize("corr", range(4))
def test_vfe_noise_component_is_exactly_zero_below_the_nugget(problem, corr):
    x, y, z = problem
    g = GO.likelihood_grad(corr, 1, x, y, z, THETA, SIGMA2, 1e-9, NUGGET)  # noise < nugget: nu = nugget
    assert g[D + 1] == 0.0 and np.all(np.isfinite(g)) and np.any(g[:D + 1] != 0.0)
    assert GO.likelihood_grad(corr, 1, x, y, z, THETA, SIGMA2, NUGGET, NUGGET)[D + 1] == 0.0  # noise == nugget


def test_theta_broadcast(problem):
    x, y, z = problem
    a = GO.likelihood_grad(0, 0, x, y, z, [0.9], SIGMA2, NOISE, NUGGET)
    b = GO.likelihood_grad(0, 0, x, y, z, [0.9] * D, SIGMA2, NOISE, NUGGET)
    np.testing.assert_array_equal(a, b)


def test_lbfgs_machine_on_a_quadratic_with_an_active_bound(tmp_path):
    """csrc/lbfgs.h compiled for the host: ask / tell on a convex quadratic in a box, the known minimiser (one bound active)
    to 1e-6 from an interior start and from a corner, a failed first evaluation."""
    exe = tmp_path / "lbfgs_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "egobox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_host", "lbfgs_test.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "lbfgs ok" in out.stdout, out.stdout[-2000:]


def test_new_symbols_and_their_argument_counts():
    """The built library exports both calls, and _lib.py declares them with the documented argument lists
    (egx_sgp_likelihood_grad: 8 arguments, egx_sgp_fit_lbfgs: 9, the layout of egx_sgp_fit)."""
    from egobox_amd import _lib as L

    path = os.path.join(ROOT, "egobox_amd", "lib", "libegx_gp_hip.so")
    assert os.path.exists(path), "build() has not run"
    lib = ctypes.CDLL(path)
    assert hasattr(lib, "egx_sgp_likelihood_grad") and hasattr(lib, "egx_sgp_fit_lbfgs")
    sigs = {name: (res, args) for name, res, args in L.SIGNATURES}
    res, args = sigs["egx_sgp_likelihood_grad"]
    assert res is ctypes.c_int32 and len(args) == 8
    assert args[3] is ctypes.c_double and args[4] is ctypes.c_double and args[2] is ctypes.c_int64
    res, args = sigs["egx_sgp_fit_lbfgs"]
    assert res is ctypes.c_int32 and len(args) == 9
    assert list(args) == list(sigs["egx_sgp_fit"][1])
