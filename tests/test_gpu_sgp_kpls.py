"""KPLS for the sparse GP on the GPU (egx_sgp_set_w_star and everything a handle with weights then does): likelihood, predictions
and Woodbury data against oracle/sgp_oracle.py with w_star, both likelihood gradients against the dense restatement
(tests/sgp_kpls_oracle.py) and against central differences of the GPU's own likelihood, same bits with and without weights,
x-gradients, sampling, the three fits of the Rust-shaped builder, save / load, an infill objective, the refusals and a C host.
The rows (n, nz, d, h), their weights and thetas: tests/sgp_kpls_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sgp_kpls_cases as KC  # noqa: E402
import sgp_kpls_oracle as KO  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = KO.KINDS
SIGMA2, NOISE = KC.SIGMA2, KC.NOISE


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def S():
    from oracle import sgp_oracle
    return sgp_oracle


_want = {}


def _restated(cid, corr, method):
    """(gradient (h + 2), grad_z (nz, d)) of the dense restatement, computed once per case."""
    key = (cid, corr, method)
    if key not in _want:
        x, y, z, w = KC.data(cid)
        th = KC.theta(cid, corr)
        _want[key] = (KO.likelihood_grad(corr, method, x, y, z, w, th, SIGMA2, NOISE, KC.NUGGET),
                      KO.likelihood_grad_z(corr, method, x, y, z, w, th, SIGMA2, NOISE, KC.NUGGET))
    return _want[key]


# ---- 1
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", range(4))
@pytest.mark.parametrize("cid", ["a", "b"])
def test_likelihood_and_predictions_vs_oracle(egx, S, cid, corr, method):
    """The tolerances of tests/test_sgp_gpu.py::test_likelihood_and_predictions_vs_oracle."""
    x, y, z, w = KC.data(cid)
    th = KC.theta(cid, corr)
    ref = S.SparseGpOracle(x, y, z, th, SIGMA2, NOISE, corr=KINDS[corr], method=[S.FITC, S.VFE][method], w_star=w)
    with egx.SgpHandle(x, y, z, corr=corr, method=method, w_star=w) as h:
        assert h.h == w.shape[1]
        np.testing.assert_array_equal(h.w_star(), w)
        lk, st = h.likelihood(th, SIGMA2, NOISE)
        assert st == 0 and lk == pytest.approx(ref.likelihood, rel=1e-8)
        h.finalize(th, SIGMA2, NOISE)
        xq = np.random.default_rng(9).random((133, x.shape[1])) * 2 - 1
        np.testing.assert_allclose(h.predict(xq), ref.predict(xq), rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(h.predict_var(xq), ref.predict_var(xq), rtol=1e-6, atol=1e-9)
        s = h.state(with_inv=True)
        assert s["likelihood"] == lk and s["sigma2"] == SIGMA2 and s["noise"] == NOISE
        np.testing.assert_array_equal(s["theta"], th)
        np.testing.assert_allclose(s["w_vec"], ref.w_vec[:, 0], rtol=1e-6, atol=1e-6 * np.abs(ref.w_vec).max())
        np.testing.assert_allclose(s["w_inv"], ref.w_inv, rtol=1e-6, atol=1e-6 * np.abs(ref.w_inv).max())


# ---- 2
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", range(4))
@pytest.mark.parametrize("cid", list(KC.CASES))
def test_both_gradients_match_the_restatement(egx, cid, corr, method):
    x, y, z, w = KC.data(cid)
    th = KC.theta(cid, corr)
    h_, nz, d = w.shape[1], z.shape[0], x.shape[1]
    want, want_z = _restated(cid, corr, method)
    with egx.SgpHandle(x, y, z, corr=corr, method=method, w_star=w) as h:
        lk0, st0 = h.likelihood(th, SIGMA2, NOISE)
        lk1, g1, st1 = h.likelihood_grad(th, SIGMA2, NOISE)
        lk2, g2, gz, st2 = h.likelihood_grad_z(th, SIGMA2, NOISE)
        _, g3, gz3, st3 = h.likelihood_grad_z(th[:1], SIGMA2, NOISE)  # theta_len == 1: the ladder value for every component
    dev = np.abs(g1 - want).max() / np.abs(want).max()
    dev_z = np.abs(gz - want_z).max() / np.abs(want_z).max()
    print(f"case {cid} corr {corr} method {method}: max |got - want| / max |want| = {dev:.3e} (params), {dev_z:.3e} (z)")
    assert st0 == 0 and st1 == 0 and st2 == 0 and st3 == 0
    assert lk1 == lk0 and lk2 == lk0  # bit for bit
    assert g1.shape == (h_ + 2,) and gz.shape == (nz, d)
    np.testing.assert_array_equal(g1, g2)
    np.testing.assert_array_equal(g3, g2)
    np.testing.assert_array_equal(gz3, gz)
    np.testing.assert_allclose(g1, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())
    np.testing.assert_allclose(gz, want_z, rtol=1e-6, atol=1e-6 * np.abs(want_z).max())


# ---- 3
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", [3, 0])
def test_directional_derivatives_match_the_gpus_own_likelihood(egx, corr, method):
    """Row b.  In (theta, sigma2, noise): p (1 +- 1e-4 v) as tests/test_gpu_sgp_grad.py; in z: z +- 1e-6 V.  rtol 1e-5."""
    x, y, z, w = KC.data("b")
    th = KC.theta("b", corr)
    h_ = th.size
    p = np.concatenate([th, [SIGMA2, NOISE]])
    v = np.random.default_rng(7).standard_normal(p.size)
    v /= np.linalg.norm(v)
    vz = np.random.default_rng(11).standard_normal(z.shape)
    vz /= np.linalg.norm(vz)
    with egx.SgpHandle(x, y, z, corr=corr, method=method, w_star=w) as h:
        _, g, gz, st = h.likelihood_grad_z(th, SIGMA2, NOISE)
        pp, pm = p * (1.0 + 1e-4 * v), p * (1.0 - 1e-4 * v)
        lp, sp = h.likelihood(pp[:h_], pp[h_], pp[h_ + 1])
        lm, sm = h.likelihood(pm[:h_], pm[h_], pm[h_ + 1])
        h.set_inducings(z + 1e-6 * vz)
        assert h.w_star() is not None  # the weights stay with the handle
        zp, szp = h.likelihood(th, SIGMA2, NOISE)
        h.set_inducings(z - 1e-6 * vz)
        zm, szm = h.likelihood(th, SIGMA2, NOISE)
    assert st == 0 and sp == 0 and sm == 0 and szp == 0 and szm == 0
    fd, an = (lp - lm) / 2e-4, float(g.dot(p * v))
    fdz, anz = (zp - zm) / 2e-6, float((gz * vz).sum())
    print(f"corr {corr} method {method}: params {fd:.10g} vs {an:.10g}; z {fdz:.10g} vs {anz:.10g}")
    assert an == pytest.approx(fd, rel=1e-5)
    assert anz == pytest.approx(fdz, rel=1e-5)


# ---- 4
def _everything(h, th, xq):
    lk, st = h.likelihood(th, SIGMA2, NOISE)
    _, g, gz, st2 = h.likelihood_grad_z(th, SIGMA2, NOISE)
    h.finalize(th, SIGMA2, NOISE)
    assert st == 0 and st2 == 0
    return [np.array([lk]), g, gz, h.predict(xq), h.predict_var(xq)] + list(h.predict_valvar_gradients(xq)) + \
        list(h.predict_valvar_gradients(xq[:1]))


@pytest.mark.parametrize("corr", range(4))
def test_same_bits_and_identity_weights(egx, corr):
    """Two calls give the same bits; w = eye(d) gives the untouched handle's bits under the squared and the absolute exponential
    (the table collapses to theta) and agrees with it under the Matern kinds (hcols = d: d factors per input, all but one of them
    1) at the tolerances of tests 1 and 2; set_w_star(None) restores the untouched bits for all four."""
    x, y, z, w = KC.data("a")
    d = x.shape[1]
    th = np.full(d, 0.3)
    xq = np.random.default_rng(5).random((70, d)) * 2 - 1
    with egx.SgpHandle(x, y, z, corr=corr) as h0:
        base = _everything(h0, th, xq)
    with egx.SgpHandle(x, y, z, corr=corr, w_star=w) as h:
        thw = KC.theta("a", corr)
        r1 = h.likelihood_grad_z(thw, SIGMA2, NOISE)
        r2 = h.likelihood_grad_z(thw, SIGMA2, NOISE)
        assert r1[0] == r2[0] and r1[3] == 0
        np.testing.assert_array_equal(r1[1], r2[1])
        np.testing.assert_array_equal(r1[2], r2[2])
        assert np.all(np.isfinite(r1[2])) and np.all(r1[1] != 0.0)
        h.set_w_star(np.eye(d))
        assert h.h == d
        ident = _everything(h, th, xq)
        h.set_w_star(None)
        assert h.w_star() is None and h.h == d
        with pytest.raises(egx.NotFittedError):
            h.predict(xq)
        cleared = _everything(h, th, xq)
    for a, b in zip(base, cleared):
        np.testing.assert_array_equal(a, b)
    for i, (a, b) in enumerate(zip(base, ident)):
        if corr < 2:
            np.testing.assert_array_equal(a, b, err_msg=str(i))
        elif i == 0:
            assert b[0] == pytest.approx(a[0], rel=1e-8)
        else:
            np.testing.assert_allclose(b, a, rtol=1e-6, atol=1e-6 * np.abs(a).max(), err_msg=str(i))


# ---- 5
@pytest.mark.parametrize("corr", [2, 0])
def test_x_gradients_against_central_differences_of_the_oracle(egx, S, corr):
    """The way and the tolerances of tests/test_sgp_gpu.py::test_numerical_gradients_like_the_reference, row a; seven queries
    (the few-query end) and one (the one-point path) give the same rows."""
    x, y, z, w = KC.data("a")
    th = KC.theta("a", corr)
    d = x.shape[1]
    ref = S.SparseGpOracle(x, y, z, th, SIGMA2, NOISE, corr=KINDS[corr], w_star=w)
    xq = np.random.default_rng(3).random((7, d)) - 0.5
    xb = np.random.default_rng(4).random((40, d)) - 0.5  # the batched route
    step = 1e-5
    with egx.SgpHandle(x, y, z, corr=corr, w_star=w) as h:
        h.finalize(th, SIGMA2, NOISE)
        for q in (xq, xb):
            gy, gv = h.predict_valvar_gradients(q)
            np.testing.assert_array_equal(gy, h.predict_gradients(q))
            np.testing.assert_array_equal(gv, h.predict_var_gradients(q))
            for g, fn_ref, atol in ((gy, ref.predict, 5e-6), (gv, ref.predict_var, 5e-5)):
                assert g.shape == q.shape
                for k in range(d):
                    dq = np.zeros(d)
                    dq[k] = step
                    fd = (fn_ref(q + dq) - fn_ref(q - dq)) / (2 * step)
                    np.testing.assert_allclose(g[:, k], fd, rtol=2e-5, atol=atol)
        g1y, g1v = h.predict_valvar_gradients(xq[2:3])  # m = 1
        gy, gv = h.predict_valvar_gradients(xq)
        np.testing.assert_allclose(g1y[0], gy[2], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(g1v[0], gv[2], rtol=1e-12, atol=1e-14)


# ---- 6
@pytest.mark.parametrize("corr", [1, 2])
def test_sample_with_given_normals(egx, S, corr):
    """traj = predict + chol(sigma2 r(xq, xq)) z with the oracle's r, the PRIOR covariance under the weights; the tolerance of
    tests/test_gpu_sample.py::test_covariance_kpls (1e-9 sigma2, absolute) on the covariance F F^T and, scaled by the normals, on
    the trajectories."""
    x, y, z, w = KC.data("a")
    th = KC.theta("a", corr)
    m = 48
    xq = np.random.default_rng(21).random((m, x.shape[1])) * 2 - 1
    zz = np.random.default_rng(22).standard_normal((m, 5))
    k = S.compute_k(KINDS[corr], xq, xq, w, th, SIGMA2)
    lo = np.linalg.cholesky(k)
    with egx.SgpHandle(x, y, z, corr=corr, w_star=w) as h:
        h.finalize(th, SIGMA2, NOISE)
        mean = h.predict(xq)
        f, tau = h.sample(xq, m, "cholesky", z=np.eye(m), return_tau=True)
        f = f - mean[:, None]
        t = h.sample(xq, 5, "cholesky", z=zz)
    print(f"corr {corr}: |F F^T - K| {np.abs(f @ f.T - k).max():.3g}, cond {np.linalg.cond(k):.3g}")
    assert tau == 0.0
    np.testing.assert_allclose(f @ f.T, k, rtol=0, atol=1e-9 * SIGMA2)
    np.testing.assert_allclose(t, mean[:, None] + lo @ zz, rtol=0, atol=1e-9 * SIGMA2 * np.abs(zz).sum(axis=0).max())


# ---- 7
def _fit_problem():
    rng = np.random.default_rng(600)
    n, d = 600, 10
    x = rng.random((n, d)) * 2 - 1
    u1, u2 = rng.standard_normal(d), rng.standard_normal(d)
    u1, u2 = u1 / np.linalg.norm(u1), u2 / np.linalg.norm(u2)
    y = np.sin(3 * x.dot(u1)) + 0.5 * np.cos(2 * x.dot(u2)) + 0.05 * rng.standard_normal(n)
    return x, y


def _builder(egx, optimizer):
    from egobox_amd import sgp as SG
    return SG.SparseGaussianProcess.params(SG.Inducings.Randomized(40)).kpls_dim(2).theta_init([1.0]).seed(3).n_start(3) \
        .max_eval(60).optimizer(optimizer)


@pytest.mark.parametrize("optimizer", ["cobyla", "lbfgs"])
def test_fits_with_kpls(egx, optimizer, tmp_path):
    from egobox_amd import kpls
    from egobox_amd import sgp as SG

    x, y = _fit_problem()
    sgp = _builder(egx, optimizer).fit(x, y)
    xq = np.random.default_rng(8).random((50, 10)) * 2 - 1
    try:
        assert sgp.theta().shape == (2,) and sgp.dims() == (2, 1) and "theta=[" in str(sgp)
        np.testing.assert_array_equal(sgp.w_star(), kpls.pls_rotations(x, y, 2))
        lk = sgp.likelihood()
        pred, var = sgp.predict(xq), sgp.predict_var(xq)
        assert np.all(np.isfinite(pred)) and np.all(var > 0.0)
        # save -> load: the real weights go through set_w_star before the state
        path = tmp_path / "sgp_kpls.json"
        assert SG.SparseGpx(sgp).save(str(path))
        back = SG.SparseGpx.load(str(path))
        np.testing.assert_array_equal(back._sgp.w_star(), sgp.w_star())
        assert back._sgp.theta().shape == (2,)
        np.testing.assert_allclose(back.predict(xq), pred, rtol=1e-9)
        np.testing.assert_allclose(back.predict_var(xq), var, rtol=1e-9)
        back._sgp.close()
        if optimizer == "lbfgs":
            moved = _builder(egx, "lbfgs").optimize_inducings(10).fit(x, y)
            print(f"lbfgs {lk:.6f}, with optimize_inducings {moved.likelihood():.6f}")
            assert moved.likelihood() >= lk and moved.theta().shape == (2,) and moved.inducings().shape == (40, 10)
            moved.close()
        # the first start: (theta_init, var(y), the default noise); this un-fits the handle, so it comes last
        lk0, st0 = sgp._h.likelihood([1.0, 1.0], float(np.std(y, ddof=1) ** 2), SG.DEFAULT_NOISE_INIT)
        print(f"{optimizer}: first start {lk0:.6f}, fitted {lk:.6f} in {sgp.n_evals} evaluations, theta {sgp.params_._kpls_dim}")
        assert st0 == 0 and lk >= lk0
    finally:
        sgp.close()


# ---- 8
def test_infill_objective_on_a_sparse_kpls_model_with_a_dense_constraint(egx):
    """The way and the tolerances of tests/test_gpu_infill_sparse.py: the parts are the handles' own predictions, value and
    gradient are tests/infill_oracle.py's recombination of them."""
    from test_gpu_infill import PRED_RTOL, _check_criterion, _data, _grad_tol

    x, y, z, w = KC.data("a")
    d = x.shape[1]
    th = KC.theta("a", 3)
    xd, yd = _data(150, d, seed=3)
    xq = np.random.default_rng(13).random((37, d)) * 2 - 1
    with egx.SgpHandle(x, y, z, corr=3, method=1, w_star=w) as ho, egx.GpHandle(2.0 * xd - 1.0, yd - np.quantile(yd, 0.6), corr=2) as hd:
        ho.finalize(th, SIGMA2, NOISE)
        hd.finalize(np.full(d, 1.4))
        own = ho.predict_valvar(xq) + ho.predict_valvar_gradients(xq)
        for crit in (egx.EI, egx.WB2):
            with egx.InfillObjective(ho, [hd], [0.3], criterion=crit, fmin=float(np.quantile(y, 0.1))) as obj:
                p = obj.parts(xq)
                np.testing.assert_allclose(p["mean"][0], own[0], rtol=PRED_RTOL, atol=1e-9)
                np.testing.assert_allclose(p["var"][0], own[1], rtol=PRED_RTOL, atol=1e-9 * SIGMA2)
                np.testing.assert_allclose(p["grad_mean"][0], own[2], **_grad_tol(own[2]))
                np.testing.assert_allclose(p["grad_var"][0], own[3], **_grad_tol(own[3]))
                wv, wg = _check_criterion(obj, p, [0.3])
                print(f"crit {crit}: value err {wv:.2e} grad err {wg:.2e}")
                assert np.all(np.isfinite(p["value"])) and np.any(p["grad"] != 0.0)


# ---- 9
def test_refusals(egx):
    x, y, z, w = KC.data("a")
    d, h_ = w.shape
    th = KC.theta("a", 3)
    with egx.SgpHandle(x, y, z, corr=3) as h:
        h.finalize(np.full(d, 0.3), SIGMA2, NOISE)
        with pytest.raises(egx.InvalidValueError, match="Dimension reduction 13 should be smaller"):
            h.set_w_star(np.ones((d, d + 1)))
        bad = w.copy()
        bad[3, 1] = np.inf
        with pytest.raises(egx.InvalidValueError, match="non-finite"):
            h.set_w_star(bad)
        assert h.w_star() is None and h.h == d
        assert np.all(np.isfinite(h.predict(x[:2])))  # a refused call leaves the handle as it was: still fitted
        h.set_w_star(w)
        with pytest.raises(egx.NotFittedError):  # un-fitted: finalize again
            h.predict(x[:2])
        for bad_len in (d, h_ + 1):
            with pytest.raises(egx.InvalidValueError, match=r"w_star\.ncols\(\)"):
                h.likelihood(np.full(bad_len, 0.3), SIGMA2, NOISE)
            with pytest.raises(egx.InvalidValueError, match=r"w_star\.ncols\(\)"):
                h.finalize(np.full(bad_len, 0.3), SIGMA2, NOISE)
        h.set_w_star(np.zeros((d, h_)))  # accepted: the reference passes it on a constant PLS residual
        lk, st = h.likelihood(th, SIGMA2, NOISE)
        assert st != 0 or np.isfinite(lk)  # the status is a value, not an error
    # d (hcols + 5) > 20480 under a Matern correlation: refused before any evaluation
    rng = np.random.default_rng(0)
    xb = rng.random((40, 600))
    with egx.SgpHandle(xb, rng.random(40), xb[:5], corr=2, w_star=rng.standard_normal((600, 30)) / 25.0) as h:
        with pytest.raises(egx.EgxError, match="hcols = 30") as err:
            h.predict_gradients(xb[:2])
        assert err.value.rc == egx._lib.ERR_UNSUPPORTED


def test_c_host_drives_a_sparse_kpls_model(egx, tmp_path):
    """tests/c_host/sgp_kpls_driver.c from plain C; its printed values are those of the Python calls on the same data."""
    exe = tmp_path / "sgp_kpls_driver"
    libdir = os.path.join(ROOT, "egobox_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "c_host", "sgp_kpls_driver.c"), f"-L{libdir}", "-legx_gp_hip", "-lm",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "OK"
    got = {ln.split()[0]: np.array(ln.split()[1:], dtype=np.float64) for ln in lines[1:]}
    n, d, h_, nz, m = 40, 4, 2, 8, 3
    i, k = np.arange(n)[:, None], np.arange(d)[None, :]
    x = ((7 * i + 13 * k) % 32) / 16.0 - 1.0
    y = ((5 * np.arange(n)) % 17) / 8.0 - 1.0 + 0.25 * x[:, 0]
    w = ((3 * np.arange(d)[:, None] + 5 * np.arange(h_)[None, :]) % 7 - 3) / 8.0
    xq = ((11 * np.arange(m)[:, None] + 5 * k) % 16) / 8.0 - 0.9375
    th = np.array([0.75, 1.25])
    with egx.SgpHandle(x, y, x[:nz].copy(), corr=3, w_star=w) as h:
        lk, g, st = h.likelihood_grad(th, 0.5, 0.03125)
        h.finalize(th, 0.5, 0.03125)
        mean, var = h.predict_valvar(xq)
        gy, gv = h.predict_valvar_gradients(xq)
    assert st == 0 and got["lkh"][0] == lk
    for key, want in (("grad", g), ("mean", mean), ("var", var), ("gy", gy.ravel()), ("gv", gv.ravel())):
        np.testing.assert_array_equal(got[key], want, err_msg=key)
