"""Pins the CPU oracle (oracle/gp_oracle.py) to the reference's own known answers.

Sources of every expected value: tests/golden/make_golden.py (reference file:line there).
"""
import json
import math
import os

import numpy as np
import pytest

from oracle import gp_oracle as O


def _load(golden_dir, name):
    return json.load(open(os.path.join(golden_dir, name)))


# ---------------------------------------------------------------- utils.rs KATs
def test_pairwise_differences(golden_dir):
    k = _load(golden_dir, "kat.json")["pairwise_differences"]
    got = O.pairwise_differences(np.array(k["x"]), np.array(k["y"]))
    np.testing.assert_allclose(got, np.array(k["expected"]), atol=k["tol"], rtol=0)


def test_normalize(golden_dir):
    k = _load(golden_dir, "kat.json")["normalize"]
    xn, mean, std = O.normalize(np.array(k["x"]))
    assert mean.tolist() == k["mean"]
    assert std.tolist() == [math.sqrt(v) for v in k["std_sq"]]


def test_normalize_zero_std():
    xn, mean, std = O.normalize(np.array([[1.0, 5.0], [2.0, 5.0], [4.0, 5.0]]))
    assert std[1] == 1.0 and np.all(xn[:, 1] == 0.0)


def test_diff_matrix(golden_dir):
    k = _load(golden_dir, "kat.json")["diff_matrix"]
    d, idx = O.diff_matrix(np.array(k["xt"]))
    np.testing.assert_allclose(d, np.array(k["d"]), atol=1e-15, rtol=0)
    assert idx.tolist() == k["idx"]


# --------------------------------------------------- correlation_models.rs KATs
def test_sqexp_1d(golden_dir):
    k = _load(golden_dir, "kat.json")["sqexp_1d"]
    d, _ = O.diff_matrix(np.array(k["xt"]))
    r = O.corr_value(O.SQEXP, d, np.sqrt(k["theta_sq"]), np.array(k["w"]))
    np.testing.assert_allclose(r[:, 0], k["expected"], atol=k["tol"], rtol=0)
    # these literals carry full precision: the oracle reproduces them much tighter
    np.testing.assert_allclose(r[:, 0], k["expected"], rtol=1e-13)


@pytest.mark.parametrize("name,kind", [("sqexp_2d", O.SQEXP), ("matern32_2d", O.MATERN32),
                                       ("matern52_2d", O.MATERN52)])
def test_corr_2d(golden_dir, name, kind):
    k = _load(golden_dir, "kat.json")[name]
    d, _ = O.diff_matrix(np.array(k["xt"]))
    theta = np.sqrt(k["theta_sq"]) if "theta_sq" in k else np.array(k["theta"])
    r = O.corr_value(kind, d, theta, np.eye(2))
    np.testing.assert_allclose(r[:, 0], k["expected"], atol=k["tol"], rtol=0)
    np.testing.assert_allclose(r[:, 0], k["expected"], rtol=2e-8)  # 9 printed digits


# ------------------------------------------------------------ mean_models.rs KATs
def test_quadratic(golden_dir):
    kat = _load(golden_dir, "kat.json")
    for name in ("quadratic", "quadratic2"):
        k = kat[name]
        np.testing.assert_array_equal(O.regression_value(O.QUADRATIC, np.array(k["x"])),
                                      np.array(k["expected"]))


# ---------------------------------------------------------------- notebook golden B
def test_golden_b_full_precision(golden_dir):
    g = _load(golden_dir, "golden_b.json")
    gp = O.fit_fixed(np.array(g["training_x"]), np.array(g["training_y"]), g["theta"],
                     mean=O.LINEAR, corr=O.MATERN52, nugget=g["nugget"], dense=False)
    assert gp.likelihood == pytest.approx(g["likelihood"], rel=1e-13)
    assert gp.inner.sigma2 == pytest.approx(g["sigma2"], rel=1e-12)
    np.testing.assert_allclose(gp.inner.r_chol, np.array(g["r_chol"]), atol=1e-15, rtol=1e-13)
    np.testing.assert_allclose(gp.inner.ft, np.array(g["ft"]), atol=1e-14)
    np.testing.assert_allclose(gp.inner.ft_qr_r, np.array(g["ft_qr_r"]), atol=1e-14)
    np.testing.assert_allclose(gp.inner.beta, np.array(g["beta"]), atol=1e-14)
    np.testing.assert_allclose(gp.inner.gamma, np.array(g["gamma"]), atol=1e-13)
    np.testing.assert_allclose(gp.xt_norm, np.array(g["xt_norm"]["data"]), atol=1e-15)
    np.testing.assert_allclose(gp.x_mean, g["xt_norm"]["mean"], atol=1e-15)
    np.testing.assert_allclose(gp.x_std, g["xt_norm"]["std"], rtol=1e-15)
    np.testing.assert_allclose(gp.yt_norm, np.array(g["yt_norm"]["data"]), atol=1e-14)
    np.testing.assert_allclose(gp.y_mean, g["yt_norm"]["mean"], rtol=1e-14)
    np.testing.assert_allclose(gp.y_std, g["yt_norm"]["std"], rtol=1e-14)
    # dense assembly (the large-n path of the oracle) is the same arithmetic
    gp2 = O.fit_fixed(np.array(g["training_x"]), np.array(g["training_y"]), g["theta"],
                      mean=O.LINEAR, corr=O.MATERN52, nugget=g["nugget"], dense=True)
    assert gp2.likelihood == gp.likelihood
    # interpolation property (python/egobox/tests/test_gpmix.py:40-41 style)
    yp = gp.predict(np.array(g["training_x"]))
    np.testing.assert_allclose(yp, np.array(g["training_y"]).ravel(), rtol=1e-9, atol=1e-9)
    vp = gp.predict_var(np.array(g["training_x"]))
    assert np.all(vp >= 0) and np.all(vp < 1e-7 * g["sigma2"])


# ---------------------------------------------------------------- notebook golden A + python pins
def test_golden_a_and_python_pins(golden_dir):
    g = _load(golden_dir, "golden_a.json")
    k = _load(golden_dir, "kat.json")["python_kriging"]
    gp = O.fit_fixed(np.array(g["xt"]), np.array(g["yt"]), [g["theta_printed_8_digits"]],
                     mean=O.CONSTANT, corr=O.SQEXP)
    # theta is printed to 8 digits; at the optimum dL/dtheta = 0 so L is second-order insensitive
    assert gp.likelihood == pytest.approx(g["likelihood"], abs=1e-12)
    assert gp.inner.sigma2 == pytest.approx(g["variance"], rel=1e-8)
    assert gp.predict(np.array([[1.0]]))[0] == pytest.approx(k["predict_1.0"], abs=10 ** -k["places"])
    assert gp.predict_var(np.array([[1.0]]))[0] == pytest.approx(k["var_1.0"], abs=10 ** -k["places"])
    assert gp.predict(np.array([[1.1]]))[0] == pytest.approx(k["predict_1.1"], abs=k["delta"])
    assert gp.predict_var(np.array([[1.1]]))[0] == pytest.approx(k["var_1.1"], abs=k["delta"])
    assert gp.predict_gradients(np.array([[1.1]]))[0, 0] == pytest.approx(k["predict_gradients_1.1"], abs=k["delta"])
    assert gp.predict_var_gradients(np.array([[1.1]]))[0, 0] == pytest.approx(k["predict_var_gradients_1.1"], abs=k["delta"])
    yv, vv = gp.predict_valvar(np.array([[1.1], [2.5]]))
    np.testing.assert_array_equal(yv, gp.predict(np.array([[1.1], [2.5]])))
    np.testing.assert_array_equal(vv, gp.predict_var(np.array([[1.1], [2.5]])))


# ---------------------------------------------------------------- internal consistency
@pytest.mark.parametrize("kind", [O.SQEXP, O.ABSEXP, O.MATERN32, O.MATERN52])
def test_dense_equals_table(kind):
    rng = np.random.default_rng(3)
    x = rng.random((40, 3))
    xn, _, _ = O.normalize(x)
    theta = np.array([0.3, 1.1, 0.7])
    d, idx = O.diff_matrix(xn)
    r1 = O.assemble_r(O.corr_value(kind, d, theta, np.eye(3)), idx, 40, O.DEFAULT_NUGGET)
    r2 = O.corr_matrix_dense(kind, xn, theta, np.eye(3), O.DEFAULT_NUGGET, chunk=7)
    np.testing.assert_allclose(r2, r1, rtol=1e-15, atol=0)


def test_status_channel():
    x = np.array([[0.0], [1.0], [1.0], [2.0]])  # duplicate row -> singular R at any theta
    y = np.array([0.0, 1.0, 1.0, 0.5])
    lk, st = O.likelihood_at(x, y, [1.0])
    assert st in (0, 1)  # nugget may or may not rescue it; either way no exception
    lk, st = O.likelihood_at(x, y, [float("nan")])
    assert st == 4 and lk == math.inf


@pytest.mark.parametrize("corr", [O.SQEXP, O.MATERN52, O.MATERN32, O.ABSEXP])
def test_gradient_matches_finite_differences(corr):
    rng = np.random.default_rng(0)
    x = rng.random((60, 3))
    y = np.sin(3 * x[:, 0]) + x[:, 1] ** 2 - x[:, 2]
    theta = np.array([0.8, 1.3, 0.5])
    _, g = O.likelihood_grad(x, y, theta, corr=corr)
    for k in range(3):
        h = 1e-6
        tp, tm = theta.copy(), theta.copy()
        tp[k] += h
        tm[k] -= h
        fd = (O.likelihood_at(x, y, tp, corr=corr)[0] - O.likelihood_at(x, y, tm, corr=corr)[0]) / (2 * h)
        assert g[k] == pytest.approx(fd, rel=2e-5, abs=1e-6)


# ---------------------------------------------------------------- the C "reference-shaped" restatement (oracle/ref_shaped.c)
@pytest.fixture(scope="module")
def RS():
    import subprocess
    from oracle import ref_shaped
    if not ref_shaped.available():
        subprocess.run(["make", "-C", os.path.dirname(ref_shaped.__file__)], check=True)
    return ref_shaped


def test_ref_shaped_reproduces_golden_a(golden_dir, RS):
    """The single-thread, LAPACK-free restatement hits the reference's own notebook values too."""
    g = _load(golden_dir, "golden_a.json")
    r = RS.likelihood(np.array(g["xt"]), np.array(g["yt"]), [g["theta_printed_8_digits"]], corr="squared_exponential")
    assert r["status"] == 0
    assert r["likelihood"] == pytest.approx(g["likelihood"], abs=1e-12)
    assert r["sigma2"] == pytest.approx(g["variance"], rel=1e-8)


@pytest.mark.parametrize("kind,name", [(O.SQEXP, "squared_exponential"), (O.ABSEXP, "absolute_exponential"),
                                       (O.MATERN32, "matern32"), (O.MATERN52, "matern52")])
def test_ref_shaped_agrees_with_numpy_oracle(RS, kind, name):
    """Two independent restatements (numpy + LAPACK vs plain C, unblocked) of the same reference lines."""
    rng = np.random.default_rng(17)
    x = rng.random((150, 3))
    y = np.sin(3 * x[:, 0]) + x[:, 1] ** 2 - 0.5 * x[:, 2]
    theta = np.array([1.5, 2.0, 1.0])
    ref = O.fit_fixed(x, y, theta, mean=O.CONSTANT, corr=kind)
    r = RS.likelihood(x, y, theta, corr=name, want_factor=True)
    assert r["status"] == 0
    assert r["likelihood"] == pytest.approx(ref.likelihood, rel=1e-9)
    assert r["sigma2"] == pytest.approx(ref.inner.sigma2, rel=1e-9)
    assert r["beta"] == pytest.approx(float(ref.inner.beta.ravel()[0]), rel=1e-9, abs=1e-12)
    np.testing.assert_allclose(r["r_chol"], ref.inner.r_chol, rtol=0, atol=1e-10)
    np.testing.assert_allclose(r["gamma"], ref.inner.gamma.ravel(), rtol=1e-6, atol=1e-6 * np.abs(ref.inner.gamma).max())


def test_ref_shaped_not_positive_definite(RS):
    x = np.array([[0.0], [1.0], [1.0], [2.0]])  # duplicate row, negative nugget -> exact singularity and below
    r = RS.likelihood(x, np.array([0.0, 1.0, 1.0, 0.5]), [1.0], nugget=-1e-3)
    assert r["status"] == 1
    assert O.likelihood_at(x, np.array([0.0, 1.0, 1.0, 0.5]), [1.0], nugget=-1e-3)[1] == 1


# ---------------------------------------------------------------- x-gradients of the predictions
def test_quadratic_jacobian_kat(golden_dir):
    k = _load(golden_dir, "kat.json")["quadratic_jac"]  # mean_models.rs:196-214
    np.testing.assert_array_equal(O.regression_jacobian(O.QUADRATIC, k["x"]), np.array(k["expected"]))


def test_bug_var_derivatives_kat(golden_dir):
    """The reference's own fixed data set (algorithm.rs:1723-1797): d var / d x against central differences."""
    b = _load(golden_dir, "kat.json")["bug_var_derivatives"]
    gp = O.fit_fixed(np.array(b["xt"]), np.array(b["yt"]), np.sqrt(2.0 * np.array(b["theta_sq_half"])))
    xa, xb = b["x"]
    e = b["e"]
    v = gp.predict_var(np.array([[xa + e, xb], [xa - e, xb], [xa, xb + e], [xa, xb - e]]))
    g = gp.predict_var_gradients(np.array([[xa, xb]]))
    assert g[0, 0] == pytest.approx((v[0] - v[1]) / (2 * e), abs=b["epsilon"])
    assert g[0, 1] == pytest.approx((v[2] - v[3]) / (2 * e), abs=b["epsilon"])


@pytest.mark.parametrize("mean", [O.CONSTANT, O.LINEAR, O.QUADRATIC])
@pytest.mark.parametrize("corr", [O.SQEXP, O.ABSEXP, O.MATERN32, O.MATERN52])
def test_prediction_gradients_match_finite_differences(mean, corr):
    """What the reference's test_gp_derivatives / test_gp_variance_derivatives macros assert (algorithm.rs:1458-1660)."""
    rng = np.random.default_rng(0)
    x = rng.random((30, 3)) * 4 - 2
    y = np.sin(x[:, 0]) + x[:, 1] ** 2 + np.abs(x[:, 2])
    gp = O.fit_fixed(x, y, np.array([0.7, 1.1, 0.9]), mean=mean, corr=corr)
    q = rng.random((4, 3)) * 3 - 1.5
    e = 1e-6
    gm, gv = gp.predict_valvar_gradients(q)
    for k in range(3):
        dq = np.zeros(3)
        dq[k] = e
        fm = (gp.predict(q + dq) - gp.predict(q - dq)) / (2 * e)
        fv = (gp.predict_var(q + dq) - gp.predict_var(q - dq)) / (2 * e)
        np.testing.assert_allclose(gm[:, k], fm, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(gv[:, k], fv, rtol=1e-6, atol=1e-7)


def test_jacobian_with_kpls_weights_matches_finite_differences():
    rng = np.random.default_rng(5)
    xt = rng.standard_normal((12, 4))
    w = rng.standard_normal((4, 2))
    theta = np.array([0.6, 1.3])
    x = rng.standard_normal(4)
    for kind in (O.SQEXP, O.ABSEXP, O.MATERN32, O.MATERN52):
        jac = O.corr_jacobian(kind, x, xt, theta, w)
        for k in range(4):
            dx = np.zeros(4)
            dx[k] = 1e-6
            fd = (O.corr_value(kind, (x + dx)[None, :] - xt, theta, w) - O.corr_value(kind, (x - dx)[None, :] - xt, theta, w)) / 2e-6
            np.testing.assert_allclose(jac[:, k], fd[:, 0], rtol=1e-6, atol=1e-9)


# ---------------------------------------------------------------- the extended-precision arbiter (oracle/arbiter_ld.c)
@pytest.fixture(scope="module")
def ARB():
    import subprocess
    from oracle import arbiter
    if not arbiter.available():
        subprocess.run(["make", "-C", os.path.dirname(arbiter.__file__)], check=True)
    return arbiter


def test_arbiter_reproduces_golden_a(golden_dir, ARB):
    """The long double evaluation hits the reference's own notebook likelihood (Constant + sq-exp, 5 points)."""
    g = _load(golden_dir, "golden_a.json")
    r = ARB.likelihood(np.array(g["xt"]), np.array(g["yt"]), [g["theta_printed_8_digits"]], corr=O.SQEXP)
    assert r["status"] == 0
    assert r["likelihood"] == pytest.approx(g["likelihood"], abs=1e-12)
    assert r["sigma2"] == pytest.approx(g["variance"], rel=1e-8)


@pytest.mark.parametrize("kind", [O.SQEXP, O.ABSEXP, O.MATERN32, O.MATERN52])
def test_arbiter_agrees_with_numpy_oracle_where_the_problem_is_well_posed(ARB, kind):
    rng = np.random.default_rng(17)
    x = rng.random((300, 3))
    y = np.sin(3 * x[:, 0]) + x[:, 1] ** 2 - 0.5 * x[:, 2]
    theta = np.array([1.5, 2.0, 1.0])
    ref = O.fit_fixed(x, y, theta, mean=O.CONSTANT, corr=kind)
    r = ARB.likelihood(x, y, theta, corr=kind)
    assert r["status"] == 0
    assert r["likelihood"] == pytest.approx(ref.likelihood, rel=1e-11)
    assert r["sigma2"] == pytest.approx(ref.inner.sigma2, rel=1e-10)
    assert r["min_pivot"] == pytest.approx(np.diag(ref.inner.r_chol).min(), rel=1e-9)


def test_arbiter_fixture_is_what_the_arbiter_computes(golden_dir, ARB):
    """tests/golden/arbiter.json was generated by this code: the control case reproduces (the arithmetic is x87 long
    double in a fixed order per row -- OpenMP only splits rows -- but the x87 transcendental instructions behind expl /
    log10l are not correctly rounded and differ in their last bits between CPU models, so on another host the value is
    a few double ulps away: 1e-14 relative, 400x closer than LAPACK), and on it LAPACK and the arbiter agree; the
    recorded LAPACK errors of the ill-posed cases are what this container's numpy gives, to within the BLAS build."""
    fx = _load(golden_dir, "arbiter.json")
    c = fx["control_n2048_d8_matern52"]
    x = O.lhs_classic(c["n"], c["d"], c["seed"])
    y = O.griewank(x)
    r = ARB.likelihood(x, y, np.array(c["theta"]), corr=c["corr"])
    assert r["status"] == 0 and abs(r["likelihood"] - c["truth_likelihood"]) <= 1e-14 * abs(c["truth_likelihood"])
    assert c["lapack_rel_error"] < 1e-10
    # the ill-posed cases: LAPACK is 1e-9 .. 1e-5 away from the extended-precision value, and not consistently
    assert 1e-7 < fx["config2_n4096_d8_sqexp"]["lapack_rel_error"] < 1e-4
    a, b = fx["config2_n4096_d8_sqexp"], fx["perm_n4096_d8_sqexp"]
    assert abs(a["truth_likelihood"] - b["truth_likelihood"]) / abs(a["truth_likelihood"]) < 1e-8
    assert abs(a["lapack_likelihood"] - b["lapack_likelihood"]) / abs(a["truth_likelihood"]) > 1e-7
