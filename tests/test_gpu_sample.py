"""Posterior covariance and trajectory sampling on the GPU (egx_gp_predict_covariance, egx_gp_sample, egx_random_normals)
against an oracle built from oracle.gp_oracle (_compute_rt_u, corr_value, pairwise_differences) and numpy's cholesky / eigh:
GaussianProcess::_compute_covariance / sample_chol / sample_eig, crates/gp/src/algorithm.rs:310-326, 383-395, 1153-1193."""
import json
import os

import numpy as np
import pytest

KINDS = ["SquaredExponential", "AbsoluteExponential", "Matern32", "Matern52"]
MEANS = ["Constant", "Linear", "Quadratic"]
MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


def _data(n, d, seed=0):
    from egobox_amd import workload
    return workload.make_training_set(n, d, seed=seed)


def oracle_cov(O, ref, xq):
    """sigma2 (K(x, x) - rt^T rt + u^T u), algorithm.rs:310-326, from the oracle's own pieces"""
    xq = np.atleast_2d(xq)
    m = xq.shape[0]
    xn = (xq - ref.x_mean) / ref.x_std
    rt, u = ref._compute_rt_u(xn, ref._compute_correlation(xn))
    k = O.corr_value(ref.corr, O.pairwise_differences(xn, xn), ref.theta, ref.w_star).reshape(m, m)
    return ref.inner.sigma2 * (k - rt.T @ rt + u.T @ u)


def oracle_from_handle(O, h, mean, corr, x, y, w_star=None):
    """the oracle evaluated on the handle's OWN fitted state (nothing refitted): GaussianProcessOracle around h.inner()"""
    ip = h.inner(with_chol=True)
    inner = O.GpInnerParams(sigma2=ip["sigma2"], beta=ip["beta"], gamma=ip["gamma"],
                            r_chol=ip["r_chol"], ft=ip["ft"], ft_qr_r=ip["ft_qr_r"])
    d = x.shape[1]
    return O.GaussianProcessOracle(theta=np.atleast_1d(ip["theta"]), likelihood=ip["likelihood"], inner=inner,
                                   w_star=np.eye(d) if w_star is None else w_star, xt_norm=ip["xt_norm"],
                                   x_mean=ip["x_mean"], x_std=ip["x_std"], yt_norm=ip["yt_norm"],
                                   y_mean=np.atleast_1d(ip["y_mean"]), y_std=np.atleast_1d(ip["y_std"]), mean=mean,
                                   corr=corr)


def numpy_normals(seed, m, n_traj):
    """philox.h restated in numpy (tests/test_sample_cpu.py checks the raw stream against numpy.random.Philox, which steps
    its counter before a block: the block of counter c is random_raw(4) from counter c - 1)"""
    g = (m + 3) // 4
    z = np.empty((4 * g, n_traj))
    for j in range(n_traj):
        for b in range(g):
            v = ((b | j << 64) - 1) & ((1 << 256) - 1)
            start = np.array([(v >> (64 * i)) & MASK64 for i in range(4)], dtype=np.uint64)
            w = np.random.Philox(key=np.array([seed, 0], dtype=np.uint64), counter=start).random_raw(4)
            u = ((w >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
            r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
            z[4 * b:4 * b + 4, j] = [r0 * np.cos(2 * np.pi * u[1]), r0 * np.sin(2 * np.pi * u[1]),
                                     r1 * np.cos(2 * np.pi * u[3]), r1 * np.sin(2 * np.pi * u[3])]
    return z[:m]


def _check_cov(c, want, var, sigma2):
    assert c.shape == want.shape
    np.testing.assert_array_equal(c, c.T)  # exactly symmetric
    assert np.abs(c - want).max() <= 1e-9 * sigma2, np.abs(c - want).max() / sigma2
    dg = np.diag(c)
    pos = dg >= 0
    np.testing.assert_allclose(dg[pos], var[pos], rtol=0, atol=1e-11 * sigma2)


# ------------------------------------------------------------------ 1. covariance vs the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("corr", range(4))
@pytest.mark.parametrize("mean", range(3))
def test_covariance_vs_oracle(egx, O, corr, mean):
    n, d = [(30, 3), (700, 3), (2100, 4)][(corr + mean) % 3]
    x, y = _data(n, d, seed=5 + corr)
    theta = np.full(d, 2.0)
    rng = np.random.default_rng(10 * corr + mean)
    with egx.GpHandle(x, y, mean=mean, corr=corr) as h:
        h.finalize(theta)
        ref = oracle_from_handle(O, h, MEANS[mean], KINDS[corr], x, y)
        sigma2 = ref.inner.sigma2
        for m in (1, 7, 129, 1000):
            xq = rng.random((m, d)) * 1.2 - 0.1
            if m >= 7:
                xq[:3] = x[:3]  # on training points: the variance is ~0 there
            _check_cov(h.predict_covariance(xq), oracle_cov(O, ref, xq), h.predict_var(xq), sigma2)


@pytest.mark.gpu
def test_covariance_kpls(egx, O):
    x, y = _data(400, 5, seed=9)
    rng = np.random.default_rng(1)
    w = rng.standard_normal((5, 2))
    theta = np.array([0.7, 0.3])
    for corr in (0, 3):
        with egx.GpHandle(x, y, corr=corr, w_star=w) as h:
            h.finalize(theta)
            ref = oracle_from_handle(O, h, "Constant", KINDS[corr], x, y, w_star=w)
            xq = rng.random((129, 5))
            _check_cov(h.predict_covariance(xq), oracle_cov(O, ref, xq), h.predict_var(xq), ref.inner.sigma2)


@pytest.mark.gpu
def test_covariance_model_loaded_from_reference_dump(egx, O):
    """golden B: a model the reference serialised, installed without refactoring (egx_gp_set_inner)"""
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden_b.json")))
    nd = lambda a: {"v": 1, "dim": list(np.shape(a)), "data": np.asarray(a, dtype=float).ravel().tolist()}
    expert = {
        "type_fullgp": g["type_fullgp"], "theta": nd(g["theta"]), "likelihood": g["likelihood"],
        "inner_params": {"sigma2": g["sigma2"], "beta": nd(g["beta"]), "gamma": nd(g["gamma"]),
                         "r_chol": nd(g["r_chol"]), "ft": nd(g["ft"]), "ft_qr_r": nd(g["ft_qr_r"])},
        "w_star": nd(g["w_star"]),
        "xt_norm": {k: nd(v) for k, v in g["xt_norm"].items()}, "yt_norm": {k: nd(v) for k, v in g["yt_norm"].items()},
        "training_data": [nd(g["training_x"]), nd(g["training_y"])],
        "params": {"theta_tuning": {"Full": {}}, "mean": "LinearMean", "corr": "Matern52", "kpls_dim": None,
                   "n_start": 10, "max_eval": 1000, "nugget": g["nugget"]},
    }
    gpx = egx.Gpx.from_dict({"recombination": "Hard", "experts": [expert], "gp_type": "FullGp"})
    inner = O.GpInnerParams(sigma2=g["sigma2"], beta=np.array(g["beta"]), gamma=np.array(g["gamma"]),
                            r_chol=np.array(g["r_chol"]), ft=np.array(g["ft"]), ft_qr_r=np.array(g["ft_qr_r"]))
    ref = O.GaussianProcessOracle(theta=np.array(g["theta"]), likelihood=g["likelihood"], inner=inner,
                                  w_star=np.eye(1), xt_norm=np.array(g["xt_norm"]["data"]),
                                  x_mean=np.array(g["xt_norm"]["mean"]), x_std=np.array(g["xt_norm"]["std"]),
                                  yt_norm=np.array(g["yt_norm"]["data"]), y_mean=np.array(g["yt_norm"]["mean"]),
                                  y_std=np.array(g["yt_norm"]["std"]), mean=O.LINEAR, corr=O.MATERN52, nugget=g["nugget"])
    xq = np.linspace(-10, 10, 129).reshape(-1, 1)
    gp = gpx._experts[0]
    _check_cov(gp.predict_covariance(xq), oracle_cov(O, ref, xq), gp.predict_var(xq), g["sigma2"])
    t, tau = gp.handle.sample(xq, 4, seed=1, return_tau=True)
    assert t.shape == (129, 4) and np.isfinite(t).all() and tau >= 1e-9


@pytest.mark.gpu
def test_covariance_large_n(egx):
    """n = 8192: the diagonal is predict_var, and a 2 x 2 covariance is the matching block of a 1000-point one"""
    n, d = 8192, 8
    x, y = _data(n, d, seed=3)
    rng = np.random.default_rng(8)
    xq = rng.random((1000, d))
    with egx.GpHandle(x, y, corr=0) as h:
        h.finalize(np.full(d, 1.0))
        c = h.predict_covariance(xq)
        np.testing.assert_array_equal(c, c.T)
        s2 = h.inner()["sigma2"]
        v = h.predict_var(xq)
        dg = np.diag(c)
        np.testing.assert_allclose(dg[dg >= 0], v[dg >= 0], rtol=0, atol=1e-11 * s2)
        c2 = h.predict_covariance(xq[[17, 803]])
        np.testing.assert_allclose(c2, c[np.ix_([17, 803], [17, 803])], rtol=0, atol=1e-11 * s2)


# ------------------------------------------------------------------ 2. the exact factor
@pytest.mark.gpu
@pytest.mark.parametrize("mean", [0, 2])
def test_exact_cholesky_factor(egx, O, mean):
    x, y = _data(200, 3, seed=12)
    xq = np.random.default_rng(4).random((40, 3)) * 1.6 - 0.3  # spread out, partly beyond the data: well conditioned
    with egx.GpHandle(x, y, mean=mean, corr=3) as h:
        h.finalize(np.full(3, 2.0))
        ref = oracle_from_handle(O, h, MEANS[mean], "Matern52", x, y)
        want = np.linalg.cholesky(oracle_cov(O, ref, xq))
        t, tau = h.sample(xq, 40, method="cholesky", z=np.eye(40), return_tau=True)
        assert tau == 0.0
        f = t - h.predict(xq)[:, None]
        assert np.abs(f - want).max() <= 1e-8 * np.abs(want).max()
        np.testing.assert_array_equal(np.triu(f, 1), 0.0)


# ------------------------------------------------------------------ 3. PSD sampling on the reference's own case
def _x2sinx(x):
    return (x * x * np.sin(x)).reshape(-1)


@pytest.mark.gpu
def test_psd_sample_reference_case(egx, O):
    """algorithm.rs:1681-1697: 6 training points of x^2 sin x, 500 points on [-10, 10], n_traj = 10"""
    xt = np.array([[-8.5], [-4.0], [-3.0], [-1.0], [4.0], [7.5]])
    gp = egx.Kriging.params().fit(xt, _x2sinx(xt))
    x = np.linspace(-10.0, 10.0, 500).reshape(-1, 1)
    traj = gp.sample(x, 10)
    assert traj.shape == (500, 10) and not np.isnan(traj).any()
    assert gp.sample_eig(x, 10).shape == (500, 10)
    h = gp.handle
    sig = h.predict_covariance(x)
    t, tau = h.sample(x, 500, z=np.eye(500), return_tau=True)
    assert tau >= 1e-9
    f = t - h.predict(x)[:, None]
    nrm = np.linalg.norm(sig, 2)
    assert np.linalg.norm(f @ f.T - sig, 2) <= tau + 1e-12 * nrm
    ip = h.inner()
    ref = oracle_from_handle(O, h, "Constant", "SquaredExponential", xt, _x2sinx(xt))
    lam, v = np.linalg.eigh(oracle_cov(O, ref, x))
    plus = (v * np.where(lam < 1e-9, 0.0, lam)) @ v.T
    assert np.linalg.norm(f @ f.T - plus, 2) <= tau + max(1e-9, abs(lam.min())) + 1e-12 * nrm
    assert ip["sigma2"] > 0
    # the plain factor of this rank-deficient covariance does not exist: the reference panics, here EGX_ERR_LINALG + pivot
    with pytest.raises(egx.LinalgError, match="pivot"):
        gp.sample_chol(x, 10)


# ------------------------------------------------------------------ 4. device normals
@pytest.mark.gpu
def test_device_normals_and_seeds(egx):
    lib = egx._lib.load()
    for seed, m, nt in ((0, 37, 5), (12345, 8, 3), (MASK64, 5, 2)):
        z = np.empty((m, nt))
        egx._lib.check(lib.egx_random_normals(-1, seed, m, nt, egx._lib.dptr(z)))
        np.testing.assert_allclose(z, numpy_normals(seed, m, nt), rtol=0, atol=1e-13)
    x, y = _data(300, 2, seed=2)
    xq = np.random.default_rng(5).random((150, 2))
    with egx.GpHandle(x, y, corr=1) as h:
        h.finalize(np.full(2, 1.5))
        a = h.sample(xq, 10, seed=77)
        np.testing.assert_array_equal(h.sample(xq, 10, seed=77), a)
        assert not np.array_equal(h.sample(xq, 10, seed=78), a)
        np.testing.assert_array_equal(h.sample(xq, 20, seed=77)[:, :10], a)
        # the library's stream IS egx_random_normals: the same trajectories through z
        z = np.empty((150, 10))
        egx._lib.check(lib.egx_random_normals(-1, 77, 150, 10, egx._lib.dptr(z)))
        np.testing.assert_array_equal(h.sample(xq, 10, seed=5, z=z), a)


# ------------------------------------------------------------------ 5. distribution
@pytest.mark.gpu
def test_sample_distribution(egx, O):
    x, y = _data(120, 2, seed=21)
    xq = np.random.default_rng(6).random((16, 2)) * 1.4 - 0.2
    N = 20000
    with egx.GpHandle(x, y, mean=1, corr=2) as h:
        h.finalize(np.full(2, 3.0))
        ref = oracle_from_handle(O, h, "Linear", "Matern32", x, y)
        t, tau = h.sample(xq, N, seed=2024, return_tau=True)
        sig = oracle_cov(O, ref, xq) + tau * np.eye(16)
        mu = ref.predict(xq)
        se_mean = np.sqrt(np.diag(sig) / N)
        assert np.all(np.abs(t.mean(axis=1) - mu) <= 6 * se_mean)
        emp = np.cov(t, bias=False)
        dg = np.diag(sig)
        se_cov = np.sqrt((np.outer(dg, dg) + sig * sig) / N)
        assert np.all(np.abs(emp - sig) <= 6 * se_cov)


# ------------------------------------------------------------------ 6. handles and errors
@pytest.mark.gpu
def test_handles_and_errors(egx, O):
    x, y = _data(256, 3, seed=30)
    xq = np.random.default_rng(7).random((50, 3))
    theta = np.full(3, 2.0)
    with egx.GpHandle(x, y, corr=0, n_workspaces=3) as h:
        with pytest.raises(egx.NotFittedError):
            h.sample(xq, 3, seed=1)
        with pytest.raises(egx.NotFittedError):
            h.predict_covariance(xq)
        h.finalize(theta)
        a = h.sample(xq, 6, seed=9)
        c = h.predict_covariance(xq)
        h.shrink(1)  # after shrink: same state, same bits
        np.testing.assert_array_equal(h.sample(xq, 6, seed=9), a)
        np.testing.assert_array_equal(h.predict_covariance(xq), c)
        with pytest.raises(egx.InvalidValueError):
            h.sample(xq, 3, method=7, seed=1)
        assert h.sample(np.zeros((0, 3)), 4, seed=1).shape == (0, 4)
        assert h.sample(xq, 0, seed=1).shape == (50, 0)
        assert h.predict_covariance(np.zeros((0, 3))).shape == (0, 0)
    # members of a group: each samples its own model
    xs = np.stack([_data(256, 3, seed=s)[0] for s in (40, 41)])
    ys = np.stack([_data(256, 3, seed=s)[1] for s in (40, 41)])
    members = egx.GpHandle.create_group(xs, ys, corr=0)
    try:
        egx.finalize_multi(members, np.stack([theta, theta]))
        for j, mh in enumerate(members):
            ref = oracle_from_handle(O, mh, "Constant", "SquaredExponential", xs[j], ys[j])
            cj = mh.predict_covariance(xq)
            assert np.abs(cj - oracle_cov(O, ref, xq)).max() <= 1e-9 * ref.inner.sigma2
            with egx.GpHandle(xs[j], ys[j], corr=0) as alone:
                alone.finalize(theta)
                np.testing.assert_allclose(mh.sample(xq, 4, seed=3), alone.sample(xq, 4, seed=3), rtol=1e-9, atol=1e-9)
    finally:
        for mh in members:
            mh.close()
    # Gpx: one cluster samples its expert; a two-expert mixture of GPU models raises the reference's error
    xt = np.linspace(0.0, 4.0, 8).reshape(-1, 1)
    yt = np.sin(xt).reshape(-1)
    gpx = egx.Gpx.builder(theta_init=[1.0], n_start=-1).fit(xt, yt)
    assert gpx.sample(np.linspace(0, 4, 30).reshape(-1, 1), 5).shape == (30, 5)
    g2 = egx.Gpx(gpx._experts * 2)
    with pytest.raises(egx.SampleError):
        g2.sample(xt, 2)
    gmx = egx.moe.GaussianMixture(np.full(2, 0.5), np.array([[0.0], [4.0]]), np.ones((2, 1, 1)))
    with pytest.raises(egx.SampleError):
        egx.moe.GpMixture(gpx._experts * 2, gmx).sample(xt, 2)


# ------------------------------------------------------------------ 7. a handle finalised twice
@pytest.mark.gpu
def test_refinalised_handle_samples_new_state(egx):
    """The trend state the sampling kernels read (beta, Rq, the column index) is cached on the device per fitted state: a
    second finalize must replace it.  Linear mean (p = 3), so Rq is a matrix and depends on theta."""
    x, y = _data(200, 2, seed=17)
    xq = np.random.default_rng(11).random((9, 2))
    th1, th2 = np.array([0.5, 3.0]), np.array([4.0, 0.8])
    with egx.GpHandle(x, y, mean=1, corr=0) as h, egx.GpHandle(x, y, mean=1, corr=0) as fresh:
        h.finalize(th1)
        c1 = h.predict_covariance(xq)
        s1 = h.sample(xq, 5, seed=31)
        h.finalize(th2)
        c2 = h.predict_covariance(xq)
        s2 = h.sample(xq, 5, seed=31)
        fresh.finalize(th2)
        np.testing.assert_array_equal(c2, fresh.predict_covariance(xq))
        np.testing.assert_array_equal(s2, fresh.sample(xq, 5, seed=31))
        assert not np.array_equal(c2, c1)
        assert not np.array_equal(s2, s1)
