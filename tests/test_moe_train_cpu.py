"""CPU side of the mixture-of-experts training (egobox_amd.moe: GaussianMixture.fit, GpMixtureParams): the numpy EM oracle of
tests/gmm_oracle.py against an independent implementation, the host logic restated from crates/moe/src/algorithm.rs against
hand-written cases, and the validation that happens before a device is touched.  No device compute."""
import numpy as np
import pytest

import gmm_oracle as GO


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_oracle_agrees_with_scikit_learn():
    """Five EM iterations from the same post-iteration-0 state: weights 2e-16, means and covariances 2e-15 (a few ulp of
    values of order one to ten), the lower bound to the last bits of a mean over n rows."""
    mixture = pytest.importorskip("sklearn.mixture")
    x = GO.blobs(301, 3, 3, seed=5, separation=4.0)
    w0, m0, c0 = GO.m_step(x, GO.nearest_mean_resp(x, GO.starts(x, 1, 3, seed=1)[0]), 1e-6)
    w, m, c, lbs = GO.em_iterations(x, w0, m0, c0, 5, 1e-6)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (ConvergenceWarning: tol = 0 never converges, on purpose)
        sk = mixture.GaussianMixture(n_components=3, covariance_type="full", tol=0.0, max_iter=5, reg_covar=1e-6, weights_init=w0,
                                     means_init=m0, precisions_init=np.linalg.inv(c0)).fit(x)
    # precisions_init goes through an inverse and a Cholesky factor before the first E-step: what it costs is the
    # conditioning of c0 times eps, far below the bounds here
    assert np.abs(sk.weights_ - w).max() <= 1e-13
    assert np.abs(sk.means_ - m).max() <= 1e-12 * np.abs(m).max()
    assert np.abs(sk.covariances_ - c).max() <= 1e-12 * np.abs(c).max()
    assert abs(sk.lower_bound_ - lbs[-1]) <= 1e-13 * abs(lbs[-1])


def test_oracle_two_pass_covariance_survives_an_offset():
    """Moments about the mean: shifting the data by 1e6 moves the means and leaves covariances and lower bounds alone."""
    x = GO.blobs(301, 3, 3, seed=5)
    s = GO.starts(x, 1, 3, seed=1)[0]
    a = GO.fit_run(x, s, max_iter=5, tol=0.0)
    b = GO.fit_run(x + 1e6, s + 1e6, max_iter=5, tol=0.0)
    assert np.abs(b["means"] - 1e6 - a["means"]).max() < 1e-8
    assert np.abs(b["covariances"] - a["covariances"]).max() < 1e-8 * np.abs(a["covariances"]).max()
    assert abs(b["lower_bound"] - a["lower_bound"]) < 1e-8 * abs(a["lower_bound"])


def test_oracle_failed_restart_is_a_status():
    x = GO.blobs(64, 2, 2, seed=2)
    run = GO.fit_run(x, np.stack([x[0], x[0]]), max_iter=5, tol=0.0, reg_covar=0.0)
    assert run["status"] == GO.FAILED and run["n_iter"] == 0 and np.isnan(run["lower_bound"])
    runs, best = GO.fit(x, np.stack([np.stack([x[0], x[0]]), np.stack([x[0], x[1]])]), max_iter=5, tol=0.0, reg_covar=0.0)
    assert best == 1 and runs[1]["status"] == GO.MAX_ITER and runs[1]["n_iter"] == 5


def test_extract_part(egx):
    data = np.arange(24.0).reshape(12, 2)
    test, train = egx.moe.extract_part(data, 5)
    np.testing.assert_array_equal(test, data[[0, 5, 10]])
    np.testing.assert_array_equal(train, data[[1, 2, 3, 4, 6, 7, 8, 9, 11]])
    test, train = egx.moe.extract_part(data[:5], 5)
    np.testing.assert_array_equal(test, data[:1])
    np.testing.assert_array_equal(train, data[1:5])


def test_sort_by_cluster(egx):
    data = np.arange(12.0).reshape(6, 2)
    parts = egx.moe.sort_by_cluster(3, data, np.array([2, 0, 2, 0, 0, 2]))
    np.testing.assert_array_equal(parts[0], data[[1, 3, 4]])
    assert parts[1].shape == (0, 2)
    np.testing.assert_array_equal(parts[2], data[[0, 2, 5]])


def test_check_number_of_points_and_three_point_rule(egx):
    M = egx.moe
    nx = 3
    big, small = np.zeros((5, nx + 1)), np.zeros((2, nx + 1))
    M.check_number_of_points([small], nx, egx.QuadraticMean())  # one cluster: no rule
    M.check_number_of_points([big, small], nx, egx.ConstantMean())  # needs 1
    M.check_number_of_points([big, small], nx, egx.LinearMean())  # needs nx + 1 = 4 ELEMENTS (Array2::len): 8 >= 4
    with pytest.raises(egx.ClusteringError, match="Need 10 points, got 8"):
        M.check_number_of_points([big, small], nx, egx.QuadraticMean())  # (nx + 1)(nx + 2) / 2 = 10 > 2 * 4
    M.check_number_of_points([big, np.zeros((3, nx + 1))], nx, egx.QuadraticMean())  # 12 elements
    with pytest.raises(egx.ClusteringError, match="at least 3, got 2"):
        M.check_three_points([big, small])
    M.check_three_points([small])  # one cluster: no rule
    M.check_three_points([big, np.zeros((3, nx + 1))])
    assert issubclass(egx.ClusteringError, egx.EgxError)


class _StubExpert:
    def __init__(self, fn):
        self.fn = fn

    def predict(self, x):
        return self.fn(np.atleast_2d(x))


def _two_cluster_gmx(egx):
    return egx.GaussianMixture([0.5, 0.5], [[0.25], [0.75]], [[[0.01]], [[0.01]]])


def test_optimize_heaviside_factor_with_stub_experts(egx):
    M = egx.moe
    gmx = _two_cluster_gmx(egx)
    experts = [_StubExpert(lambda x: np.zeros(x.shape[0])), _StubExpert(lambda x: np.ones(x.shape[0]))]
    xt = np.linspace(0.05, 0.95, 19).reshape(-1, 1)
    np.testing.assert_array_equal(M.HEAVISIDE_GRID, np.linspace(0.1, 2.1, 20))
    for target in (0.1, M.HEAVISIDE_GRID[7], 2.1):
        g = egx.GaussianMixture(gmx.weights, gmx.means, gmx.covariances, target)
        yt = g.predict_probas(xt)[:, 1]  # exactly what the smooth recombination gives under `target`
        assert M.optimize_heaviside_factor(experts, gmx, xt, yt) == target
        errors = M.heaviside_errors(experts, gmx, xt, yt)
        want = [np.sqrt(np.sum((egx.GaussianMixture(gmx.weights, gmx.means, gmx.covariances, f).predict_probas(xt)[:, 1] - yt) ** 2))
                / np.sqrt(np.sum(xt * xt)) for f in M.HEAVISIDE_GRID]
        np.testing.assert_allclose(errors, want, rtol=1e-12, atol=1e-15)
    assert gmx.heaviside_factor == 1.0  # the caller's mixture is not touched
    # every error below 1e-6 -> 1: both experts say the same, so the factor does not matter
    same = [_StubExpert(lambda x: x[:, 0] + 1e-8), _StubExpert(lambda x: x[:, 0] + 1e-8)]
    assert M.optimize_heaviside_factor(same, gmx, xt, xt[:, 0]) == 1.0
    # hard recombination / one cluster -> 1
    assert M.optimize_heaviside_factor(experts, gmx, xt, xt[:, 0], recombination="hard") == 1.0
    one = egx.GaussianMixture([1.0], [[0.5]], [[[1.0]]])
    assert M.optimize_heaviside_factor(experts[:1], one, xt, xt[:, 0]) == 1.0


def test_builder_validation(egx):
    P = egx.GpMixture.params
    assert isinstance(P(), egx.GpMixtureParams)
    with pytest.raises(NotImplementedError):
        P().regression_spec(egx.RegressionSpec.CONSTANT | egx.RegressionSpec.LINEAR)
    with pytest.raises(NotImplementedError):
        P().correlation_spec(egx.CorrelationSpec.ALL)
    with pytest.raises(NotImplementedError):
        P().n_clusters("auto")
    with pytest.raises(egx.InvalidValueError):
        P().n_clusters(0)
    with pytest.raises(egx.InvalidValueError):
        P().recombination("soft")
    x = np.linspace(0, 1, 4).reshape(-1, 1)
    with pytest.raises(egx.InvalidValueError, match="exceeds"):
        P().n_clusters(5).fit(x, x[:, 0])  # k > n, before any device is touched
    with pytest.raises(egx.InvalidValueError):
        P().n_clusters(2).theta_tunings([egx.ThetaTuning.default()] * 3).fit(x, x[:, 0])
    p = P().n_clusters(3).recombination("smooth", 0.5).regression_spec(egx.RegressionSpec.LINEAR) \
        .correlation_spec(egx.CorrelationSpec.MATERN52).n_start(3).max_eval(40).kpls_dim(None).seed(7).device(0)
    assert (p._n_clusters, p._recombination, p._heaviside_factor, p._n_start, p._seed) == (3, "smooth", 0.5, 3, 7)
    assert p._mean == egx.LinearMean() and p._corr == egx.Matern52Corr()
    d = P()
    assert (d._recombination, d._heaviside_factor, d._n_start, d._n_runs) == ("smooth", 1.0, 10, 20)  # parameters.rs:142-159, 249
    assert P().recombination("smooth")._heaviside_factor is None


def test_gmm_default_config(egx):
    cfg = egx._lib.GmmConfig()
    egx._lib.load().egx_gmm_config_default(cfg)
    assert (cfg.n_clusters, cfg.n_runs, cfg.max_iter, cfg.device, cfg.tol, cfg.reg_covar) == (1, 20, 100, -1, 1e-3, 1e-6)


def test_gmm_fit_validates_before_the_device(egx):
    x = GO.blobs(40, 3, 2, seed=0)
    bad = x.copy()
    bad[7, 1] = np.nan
    with pytest.raises(egx.InvalidValueError, match="finite"):
        egx.GaussianMixture.fit(bad, 2)
    with pytest.raises(egx.InvalidValueError):
        egx.GaussianMixture.fit(x, 0)
    with pytest.raises(egx.InvalidValueError):
        egx.GaussianMixture.fit(x[:3], 4)
    with pytest.raises(egx.InvalidValueError):
        egx.GaussianMixture.fit(x, 2, n_runs=0)
    with pytest.raises(egx.InvalidValueError):
        egx.GaussianMixture.fit(x, 2, n_runs=2, init_means=np.zeros((2, 2, 4)))
    with pytest.raises(egx.InvalidValueError, match="dim <= 36"):
        egx.GaussianMixture.fit(np.random.default_rng(0).random((50, 37)), 2)
    with pytest.raises(egx.InvalidValueError, match="n_clusters <= 16"):
        egx.GaussianMixture.fit(np.random.default_rng(0).random((50, 3)), 17)


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_gmm_fit_has_no_cpu_fallback(egx):
    x = GO.blobs(40, 3, 2, seed=0)
    with pytest.raises(egx.NoDeviceError):
        egx.GaussianMixture.fit(x, 2)
    with pytest.raises(egx.NoDeviceError):
        egx.GpMixture.params().n_clusters(2).recombination("hard").fit(x[:, :2], x[:, 2])


def test_too_few_points_in_a_cluster(egx):
    """A ready mixture that leaves a cluster with two points: the three-point rule (algorithm.rs:168-173)."""
    x = np.array([0.0, 0.01, 0.5, 0.52, 0.54, 0.56, 0.58]).reshape(-1, 1)
    gmx = egx.GaussianMixture([0.5, 0.5], [[0.0], [0.55]], [[[0.01]], [[0.01]]])
    with pytest.raises(egx.ClusteringError, match="at least 3, got 2"):
        egx.GpMixture.params().n_clusters(2).recombination("hard").gmx(gmx).fit(x, x[:, 0] ** 2)
