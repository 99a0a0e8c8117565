"""The sparse GP's likelihood gradient in the inducing points without a GPU: the numpy restatement (tests/sgp_zgrad_oracle.py)
against central differences of the CPU oracle's likelihood (oracle/sgp_oracle.py fitc / vfe), its behaviour where an inducing
point sits on a training point or far away, the second entry of the host-only L-BFGS machine (csrc/lbfgs.h), and the four new
symbols of the built library against the header."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sgp_grad_oracle as GO  # noqa: E402
import sgp_zgrad_oracle as ZO  # noqa: E402
from oracle import sgp_oracle as S  # noqa: E402

N, NZ, D = 130, 17, 3
THETA, SIGMA2, NOISE, NUGGET = np.array([1.3, 0.8, 1.1]), 0.9, 0.02, 1e-8
NEW = ["egx_sgp_likelihood_grad_z", "egx_sgp_set_inducings", "egx_sgp_get_inducings", "egx_sgp_fit_lbfgs_z"]


@pytest.fixture(scope="module")
def problem():
    rng = np.random.default_rng(N)
    x = rng.random((N, D)) * 2 - 1
    y = np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, -1]) + 0.05 * rng.standard_normal(N)
    z = rng.random((NZ, D)) * 2 - 1  # NOT rows of x
    return x, y, z


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", range(4))
def test_restatement_matches_central_differences_of_the_oracle(problem, corr, method):
    """Absolute step 1e-6 per entry of z; bar 5e-6 of max(1, |difference quotient|): 7 x the 6.7e-7 measured over six seeds
    (the quotient's own noise, eps |L| / step ~ 1e-7, dominates: the closed form is good to ~1e-12 here)."""
    x, y, z = problem
    fn = S.fitc if method == 0 else S.vfe

    def lkh(zz):
        return fn(GO.KINDS[corr], THETA, SIGMA2, NOISE, np.eye(D), x, y.reshape(-1, 1), zz, NUGGET)[0]

    fd = np.zeros((NZ, D))
    for j in range(NZ):
        for k in range(D):
            zp, zm = z.copy(), z.copy()
            zp[j, k] += 1e-6
            zm[j, k] -= 1e-6
            fd[j, k] = (lkh(zp) - lkh(zm)) / 2e-6
    got = ZO.likelihood_grad_z(corr, method, x, y, z, THETA, SIGMA2, NOISE, NUGGET)
    dev = np.abs(got - fd) / np.maximum(1.0, np.abs(fd))
    print(f"corr {corr} method {method}: worst deviation {dev.max():.3e}, max |fd| {np.abs(fd).max():.3e}")
    assert got.shape == (NZ, D) and np.abs(fd).max() > 1e-2
    assert dev.max() <= 5e-6, (got, fd)


@pytest.mark.parametrize("method", [0, 1])
def test_inducing_points_on_training_rows_under_the_absolute_exponential(problem, method):
    """A Randomized draw: every z_j is some x_t, where the absolute exponential has a kink.  sgn(0) = 0: the pair contributes
    exactly 0 in each coordinate, every entry is finite, and a bit-identical copy of x_t in place of z_j changes nothing.  No
    comparison with a difference quotient (it straddles the kink)."""
    x, y, _ = problem
    idx = np.random.default_rng(1).permutation(N)[:NZ]
    z = x[idx].copy()
    g = ZO.likelihood_grad_z(1, method, x, y, z, THETA, SIGMA2, NOISE, NUGGET)
    assert g.shape == (NZ, D) and np.all(np.isfinite(g)) and np.all(g != 0.0)
    for k in range(D):
        ph = ZO.phi(1, x, z, THETA, k)
        assert np.all(ph[idx, np.arange(NZ)] == 0.0)
        assert np.all(np.abs(ph[np.abs(x[:, None, k] - z[None, :, k]) > 0]) == THETA[k])
        assert np.all(np.diag(ZO.phi(1, z, z, THETA, k)) == 0.0)
    z2 = z.copy()
    z2[3] = np.frombuffer(x[idx[3]].tobytes(), dtype=np.float64)  # the same bits, another buffer
    np.testing.assert_array_equal(ZO.likelihood_grad_z(1, method, x, y, z2, THETA, SIGMA2, NOISE, NUGGET), g)


@pytest.mark.parametrize("corr", range(4))
def test_a_far_inducing_point_gets_exact_zeros_from_the_first_sum(problem, corr):
    """z_j so far away that r(x, z_j) < 1e-300 for every x (here it underflows to 0): its row of the first sum is exactly 0, the
    whole gradient stays finite, and the other rows are those of a gradient (non-zero)."""
    x, y, z = problem
    z = z.copy()
    z[5] = 1e4
    assert GO.corr(corr, x, z[5:6], THETA).max() < 1e-300
    g_nz, g_zz = ZO.likelihood_grad_z(corr, 0, x, y, z, THETA, SIGMA2, NOISE, NUGGET, parts=True)
    assert np.all(g_nz[5] == 0.0) and np.all(g_zz[5] == 0.0)
    assert np.all(np.isfinite(g_nz)) and np.all(np.isfinite(g_zz))
    assert np.all(np.delete(g_nz + g_zz, 5, axis=0) != 0.0)


def test_lbfgs_machine_started_from_mixed_variables(tmp_path):
    """csrc/lbfgs.h's second entry compiled for the host (tests/c_host/lbfgs_linear_test.cpp): a quadratic in two log10 and three
    linear variables with one bound active, minimiser to 1e-6; the old constructor's walk on lbfgs_test.cpp's problem unchanged."""
    exe = tmp_path / "lbfgs_linear_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "egobox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_host", "lbfgs_linear_test.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "lbfgs linear ok" in out.stdout, out.stdout[-2000:]


def _header_prototype(text, name):
    """[ctypes type of every argument] of `int32_t name(...);` in the header."""
    m = re.search(r"int32_t\s+" + name + r"\s*\((.*?)\)\s*;", text, re.S)
    assert m, name
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    out = []
    for a in args:
        if "*" in a:
            base = {"double": ctypes.c_double, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}.get(
                a.replace("const", "").split("*")[0].strip())
            out.append(ctypes.POINTER(base) if base else ctypes.c_void_p)
        else:
            out.append({"double": ctypes.c_double, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[a.split()[0]])
    return out


def test_new_symbols_are_exported_and_declared_as_the_header_has_them():
    from egobox_amd import _lib as L

    path = os.path.join(ROOT, "egobox_amd", "lib", "libegx_gp_hip.so")
    assert os.path.exists(path), "build() has not run"
    lib = ctypes.CDLL(path)
    header = open(os.path.join(ROOT, "include", "egx_gp.h")).read()
    hpp = open(os.path.join(ROOT, "include", "egx_gp.hpp")).read()
    sigs = {name: (res, args) for name, res, args in L.SIGNATURES}
    for name in NEW:
        assert hasattr(lib, name), name
        res, args = sigs[name]
        assert res is ctypes.c_int32
        assert list(args) == _header_prototype(header, name), name
        assert name + "(" in hpp, name
    assert len(sigs["egx_sgp_likelihood_grad_z"][1]) == len(sigs["egx_sgp_likelihood_grad"][1]) + 1
    assert len(sigs["egx_sgp_fit_lbfgs_z"][1]) == len(sigs["egx_sgp_fit_lbfgs"][1]) + 3
