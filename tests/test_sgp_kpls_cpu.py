"""KPLS for the sparse GP without a GPU: the case rows (tests/sgp_kpls_cases.py) meet the project's conditioning bar, the dense
restatement with weights (tests/sgp_kpls_oracle.py) equals the two w = I oracles and the central differences of
oracle/sgp_oracle.py's likelihood, the shared coefficient table (csrc/kpls_coef.h) is checked as a stand-alone program, plain and
under the address / undefined-behaviour sanitizers, and the built library has the two new entry points with their refusals."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sgp_grad_oracle as GO  # noqa: E402
import sgp_kpls_cases as KC  # noqa: E402
import sgp_kpls_oracle as KO  # noqa: E402
import sgp_zgrad_oracle as ZO  # noqa: E402

CSRC = os.path.join(ROOT, "egobox_amd", "csrc")


@pytest.mark.parametrize("corr", range(4))
@pytest.mark.parametrize("cid", list(KC.CASES))
def test_case_rows_meet_the_conditioning_bar(cid, corr):
    """median R_nz >= 0.2 (the weights matter) and cond(R_zz + nugget / sigma2) <= 1e8, the bar of tests/test_gpu_sgp_grad.py."""
    x, _, z, w = KC.data(cid)
    th = KC.theta(cid, corr)
    med = float(np.median(KO.corr(corr, x, z, w, th)))
    cond = KO.zz_condition(corr, z, w, th, KC.SIGMA2, KC.NUGGET)
    print(f"case {cid} corr {corr}: theta {th[0]}, median R_nz {med:.3f}, cond {cond:.3e}")
    assert th.shape == (KC.CASES[cid][3],) and med >= 0.2 and cond <= 1e8


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", range(4))
def test_restatement_with_identity_weights_equals_the_two_oracles(corr, method):
    n, nz, d = 130, 17, 3
    rng = np.random.default_rng(n)
    x = rng.random((n, d)) * 2 - 1
    y = np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, -1]) + 0.05 * rng.standard_normal(n)
    z = rng.random((nz, d)) * 2 - 1
    th = np.array([1.3, 0.8, 1.1])
    got = KO.likelihood_grad(corr, method, x, y, z, np.eye(d), th, 0.9, 0.02, 1e-8)
    want = GO.likelihood_grad(corr, method, x, y, z, th, 0.9, 0.02, 1e-8)
    np.testing.assert_allclose(got, want, rtol=1e-9)
    got_z = KO.likelihood_grad_z(corr, method, x, y, z, np.eye(d), th, 0.9, 0.02, 1e-8)
    want_z = ZO.likelihood_grad_z(corr, method, x, y, z, th, 0.9, 0.02, 1e-8)
    np.testing.assert_allclose(got_z, want_z, rtol=1e-9)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", range(4))
@pytest.mark.parametrize("cid", list(KC.CASES))
def test_directional_derivative_matches_central_differences_of_the_oracle(cid, corr, method):
    """The step and the bar of test_directional_derivative_matches_the_gpus_own_likelihood: p (1 +- 1e-4 v) along a random unit
    direction v in (theta, sigma2, noise), grad . (p o v) at rtol 1e-5."""
    x, y, z, w = KC.data(cid)
    th = KC.theta(cid, corr)
    h = th.size
    p = np.concatenate([th, [KC.SIGMA2, KC.NOISE]])
    v = np.random.default_rng(7).standard_normal(p.size)
    v /= np.linalg.norm(v)
    g = KO.likelihood_grad(corr, method, x, y, z, w, th, KC.SIGMA2, KC.NOISE, KC.NUGGET)
    pp, pm = p * (1.0 + 1e-4 * v), p * (1.0 - 1e-4 * v)
    lp = KO.likelihood(corr, method, x, y, z, w, pp[:h], pp[h], pp[h + 1], KC.NUGGET)
    lm = KO.likelihood(corr, method, x, y, z, w, pm[:h], pm[h], pm[h + 1], KC.NUGGET)
    fd, an = (lp - lm) / 2e-4, float(g.dot(p * v))
    print(f"case {cid} corr {corr} method {method}: central difference {fd:.10g}, grad . (p o v) {an:.10g}")
    assert g.shape == (h + 2,) and an == pytest.approx(fd, rel=1e-5)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", [0, 2, 3])
def test_inducing_point_gradient_matches_central_differences_of_the_oracle(corr, method):
    """Row a, along a random unit direction V in z with the absolute step 1e-6 (the inducing points are rows of x, a kink of the
    absolute exponential, which is left out here).  rtol 1e-5: the quotient's own noise eps |L| / 1e-6 ~ 1e-8 is below it."""
    x, y, z, w = KC.data("a")
    th = KC.theta("a", corr)
    v = np.random.default_rng(11).standard_normal(z.shape)
    v /= np.linalg.norm(v)
    gz = KO.likelihood_grad_z(corr, method, x, y, z, w, th, KC.SIGMA2, KC.NOISE, KC.NUGGET)
    lp = KO.likelihood(corr, method, x, y, z + 1e-6 * v, w, th, KC.SIGMA2, KC.NOISE, KC.NUGGET)
    lm = KO.likelihood(corr, method, x, y, z - 1e-6 * v, w, th, KC.SIGMA2, KC.NOISE, KC.NUGGET)
    fd, an = (lp - lm) / 2e-6, float((gz * v).sum())
    print(f"corr {corr} method {method}: central difference {fd:.10g}, grad_z . V {an:.10g}")
    assert gz.shape == z.shape and an == pytest.approx(fd, rel=1e-5)


# ---- csrc/kpls_coef.h as a stand-alone program
D_, H_ = 4, 2
W_ = np.array([[0.6, -0.3], [0.0, 0.0], [-0.2, 0.9], [0.5, 0.0]])  # a zero row: c_1 = 0
TH_ = np.array([0.7, 1.9])
GD_ = np.array([0.3, -1.1, 0.8, 2.5])
GH_ = np.array([-0.4, 1.7])
DIV_ = float(np.log(10.0))


def _numpy_table_and_chain_rule(corr):
    aw = np.abs(W_)
    if corr == 0:
        coef = np.sqrt(((TH_ * W_) ** 2).sum(axis=1))
        with np.errstate(divide="ignore", invalid="ignore"):
            dc = np.where(coef[:, None] > 0.0, TH_ * W_ * W_ / coef[:, None], 0.0)
        return 1, coef, (GD_ / DIV_).dot(dc)
    if corr == 1:
        return 1, aw.dot(TH_), (GD_ / DIV_).dot(aw)
    return H_, (TH_ * aw).ravel(), GH_ / DIV_


def _run_kpls_coef(exe):
    args = [str(exe), str(D_), str(H_)] + [repr(float(v)) for v in np.concatenate([W_.ravel(), TH_, GD_, GH_, [DIV_]])]
    out = subprocess.run(args, capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-800:], out.stderr[-800:])
    assert "runtime error" not in out.stderr, out.stderr[-800:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 4
    for corr, line in enumerate(lines):
        tok = line.split()
        assert tok[0] == "corr" and int(tok[1]) == corr and tok[2] == "hcols"
        hcols = int(tok[3])
        ic, ig, ino = tok.index("coef"), tok.index("grad"), tok.index("nograd")
        coef = np.array(tok[ic + 1:ig], dtype=np.float64)
        grad = np.array(tok[ig + 1:ino], dtype=np.float64)
        nograd = np.array(tok[ino + 1:], dtype=np.float64)
        want_hcols, want_coef, want_grad = _numpy_table_and_chain_rule(corr)
        print(f"corr {corr}: numpy hcols {want_hcols} coef {want_coef.tolist()} grad {want_grad.tolist()}")
        assert hcols == want_hcols
        np.testing.assert_allclose(coef, want_coef, rtol=1e-14, atol=0.0)
        np.testing.assert_allclose(grad, want_grad, rtol=1e-14, atol=0.0)
        np.testing.assert_array_equal(nograd, GD_ / DIV_)  # w = I: the table is theta, the sums are passed on
        if corr < 2:
            assert coef[1] == 0.0  # the zero row of w contributes nothing, and no NaN
        assert np.all(np.isfinite(grad))


def test_kpls_coef_header_as_a_program(tmp_path):
    exe = tmp_path / "kpls_coef_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "c_host", "kpls_coef_test.cpp"),
                    "-o", str(exe)], check=True)
    _run_kpls_coef(exe)


def test_kpls_coef_header_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "kpls_coef_test_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-I", CSRC, os.path.join(ROOT, "tests", "c_host", "kpls_coef_test.cpp"), "-o", str(exe)], check=True)
    _run_kpls_coef(exe)


def test_dense_and_sparse_sources_share_the_header():
    for name in ("gp_host.hip", "gp_fit.hip", "sgp_host.hip", "sgp_grad.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "kpls_coef.h"' in text and "kpls::" in text, name
    assert "kpls_coef.h" in open(os.path.join(CSRC, "Makefile")).read()


# ---- the built library, no GPU needed
def test_new_entry_points_and_their_refusals_without_a_handle():
    from egobox_amd import _lib as L

    path = os.path.join(ROOT, "egobox_amd", "lib", "libegx_gp_hip.so")
    assert os.path.exists(path), "build() has not run"
    raw = ctypes.CDLL(path)
    header = open(os.path.join(ROOT, "include", "egx_gp.h")).read()
    hpp = open(os.path.join(ROOT, "include", "egx_gp.hpp")).read()
    sigs = {name: (res, args) for name, res, args in L.SIGNATURES}
    for name in ("egx_sgp_set_w_star", "egx_sgp_get_w_star"):
        assert hasattr(raw, name), name
        assert name in sigs and sigs[name][0] is ctypes.c_int32
        assert name + "(" in header and name + "(" in hpp
    lib = L.load()
    w = np.ones((3, 2))
    hh = ctypes.c_int64()
    with pytest.raises(L.InvalidValueError, match="NULL handle"):
        L.check(lib.egx_sgp_set_w_star(None, L.dptr(w), 2))
    with pytest.raises(L.InvalidValueError, match="canot be 0"):
        L.check(lib.egx_sgp_set_w_star(None, L.dptr(w), 0))
    with pytest.raises(L.InvalidValueError, match="NULL"):
        L.check(lib.egx_sgp_get_w_star(None, None, ctypes.byref(hh)))


def test_builders_refuse_what_they_must():
    import egobox_amd as egx
    from egobox_amd import sgp as SG

    with pytest.raises(egx.InvalidValueError, match="canot be 0"):
        SG.SparseGaussianProcess.params(SG.Inducings.Randomized(10)).kpls_dim(0)
    with pytest.raises(egx.InvalidValueError, match="Dimension reduction"):
        SG.SparseGaussianProcess.params(SG.Inducings.Randomized(10)).theta_init([0.1, 0.1]).kpls_dim(3)
    p = SG.SparseGaussianProcess.params(SG.Inducings.Randomized(10)).kpls_dim(2)
    assert p._kpls_dim == 2 and p.kpls_dim(None)._kpls_dim is None
    with pytest.raises(NotImplementedError, match="KPLS"):
        SG.SparseGpMix(nz=10, kpls_dim=2)
    with pytest.raises(NotImplementedError, match="KPLS"):
        SG.SparseGpx.builder(nz=10, kpls_dim=2)
