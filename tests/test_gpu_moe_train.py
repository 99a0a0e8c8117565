"""GpMixture.params(..).fit(x, y) end to end on the GPU (crates/moe/src/algorithm.rs:72-205): the Gaussian mixture trained by
egx_gmm_fit on [x, y], the clusters' experts through fit_experts, on the reference's own test function f_test_1d
(algorithm.rs:1175-1188)."""
import copy

import numpy as np
import pytest

import gmm_oracle as GO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


def f_test_1d(x):
    x = np.asarray(x, dtype=np.float64).ravel()
    return np.where(x < 0.4, x * x, np.where(x < 0.8, 3.0 * x + 1.0, np.sin(10.0 * x)))


XT = np.linspace(0.0, 1.0, 60).reshape(-1, 1)
YT = f_test_1d(XT)
XQ = np.array([0.1, 0.2, 0.3, 0.36, 0.45, 0.6, 0.75, 0.85, 0.9, 0.97]).reshape(-1, 1)


def _builder(egx, k):
    return egx.GpMixture.params().n_clusters(k).regression_spec(egx.RegressionSpec.CONSTANT) \
        .correlation_spec(egx.CorrelationSpec.SQUARED_EXPONENTIAL).seed(0)


@pytest.fixture(scope="module")
def hard3(egx):
    return _builder(egx, 3).recombination("hard").fit(XT, YT)


def test_f_test_1d_three_clusters_hard(egx, hard3):
    """The clusters are the function's three pieces (12, 24 and 24 points: the two equal ones go through fit_group), the
    mixture's lower bound is the oracle's best over the same starts, and the predictions hold the reference's own epsilon
    (algorithm.rs:1228-1237)."""
    moe = hard3
    sizes = sorted(e.training_data[0].shape[0] for e in moe.experts)
    assert sizes == [12, 24, 24]
    data = np.column_stack([XT, YT])
    runs, best = GO.fit(data, GO.starts(data, 20, 3, seed=0))
    assert abs(moe.gmx.lower_bound_ - runs[best]["lower_bound"]) <= 1e-6
    assert moe.gmx.lower_bounds_.shape == (20,) and moe.gmx.n_clusters == 3 and moe.gmx.means.shape == (3, 1)
    err = np.abs(moe.predict(XQ) - f_test_1d(XQ))
    print("prediction errors", err)
    assert err.max() <= 1e-4
    assert moe.recombination == "hard" and moe.gmx.heaviside_factor == 1.0
    np.testing.assert_array_equal(moe.training_data[0], XT)


def test_one_cluster_is_the_plain_gp(egx):
    moe = _builder(egx, 1).recombination("hard").n_start(10).fit(XT[:24], YT[:24])
    gp = egx.GaussianProcess.params(egx.ConstantMean(), egx.SquaredExponentialCorr()).n_start(10).fit(XT[:24], YT[:24])
    xq = np.linspace(0.0, 0.4, 17).reshape(-1, 1)
    np.testing.assert_array_equal(moe.predict(xq), gp.predict(xq))
    np.testing.assert_array_equal(moe.predict_var(xq), gp.predict_var(xq))
    assert moe.gmx.n_clusters == 1 and len(moe.experts) == 1


def test_smooth_with_a_given_factor(egx, hard3):
    moe = _builder(egx, 3).recombination("smooth", 0.5).fit(XT, YT)
    assert moe.recombination == "smooth" and moe.gmx.heaviside_factor == 0.5
    np.testing.assert_array_equal(moe.gmx.means, hard3.gmx.means)  # the same clustering: the factor only scales it
    assert np.all(np.isfinite(moe.predict(XQ)))


def test_smooth_chooses_its_factor(egx):
    """Smooth(None): the factor is chosen on rows 0, 5, 10, .. with a mixture trained on the others, then everything is
    trained again on all 60 rows with it."""
    M = egx.moe
    moe = _builder(egx, 3).recombination("smooth").fit(XT, YT)
    factor = moe.gmx.heaviside_factor
    assert np.any(M.HEAVISIDE_GRID == factor)
    stage = moe.heaviside_stage_
    xtest, ytest = XT[::5], YT[::5]
    errors = []
    for f in M.HEAVISIDE_GRID:
        g = copy.copy(stage.gmx).set_heaviside_factor(f)
        pred = M.GpMixture(stage.experts, g, "smooth").predict(xtest)
        errors.append(np.sqrt(np.sum((pred - ytest) ** 2)) / np.sqrt(np.sum(xtest * xtest)))
    errors = np.array(errors)
    assert max(errors) >= 1e-6  # (else the rule says 1, which is not on the grid)
    assert errors[M.HEAVISIDE_GRID == factor][0] == errors.min()
    # the stage's mixture saw 48 rows, the final one all 60
    data = np.column_stack([XT, YT])
    all_rows = egx.GaussianMixture.fit(data, 3, seed=0)
    part = egx.GaussianMixture.fit(M.extract_part(data, 5)[1], 3, seed=0)
    assert moe.gmx.lower_bound_ == all_rows.lower_bound_ and stage.gmx.lower_bound_ == part.lower_bound_
    np.testing.assert_array_equal(moe.gmx.means, all_rows.means[:, :1])
    assert moe.gmx.lower_bound_ != stage.gmx.lower_bound_
    assert moe.recombination == "smooth"
