"""A clustered surrogate on 40 input columns, end to end on the GPU: the joined rows [x, y] are 41 wide, beyond what
GaussianMixture.fit takes, so moe.train_mixture sends the mixture's training to GaussianMixture.fit_wide
(egx_gmm_fit_wide).  GpMixture (plain and with KPLS), SparseGpMix and Egor."""
import numpy as np
import pytest

import gmm_oracle as GO

pytestmark = pytest.mark.gpu

NX = 40


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


def _data(n, seed):
    """Two blobs of n / 2 rows around -3 and +3 in every coordinate (unit noise, rows alternating), a smooth function of x
    plus an offset per blob."""
    rng = np.random.default_rng(seed)
    blob = np.arange(n) % 2
    x = (6.0 * blob[:, None] - 3.0) + rng.standard_normal((n, NX))
    y = np.sin(0.3 * x[:, :4].sum(axis=1)) + 0.05 * x[:, 4:].sum(axis=1) + 20.0 * blob
    return x, y, blob


X, Y, BLOB = _data(240, 3)
XQ = _data(16, 1)[0]


@pytest.fixture(scope="module")
def oracle_gmx(egx):
    """The oracle's mixture of [x, y] from the builder's own starts (seed 0), marginal in x.  A restart whose two starts
    are rows of one blob can end in a cluster of fewer rows than columns, whose near-singular covariance buys a great
    likelihood: EM's own behaviour, the reference's included, and not this test's subject.  The data seed is one where the
    blob pair wins all the same, by 2 in the lower bound over the best such restart (14 of 20 find the blobs and agree among
    themselves to rounding) -- checked here on the oracle, the library is not consulted."""
    data = np.column_stack([X, Y])
    runs, best = GO.fit(data, GO.starts(data, 20, 2, seed=0))
    r = runs[best]
    blobs = [q["lower_bound"] for q in runs if abs(q["weights"][0] - 0.5) <= 1e-9]
    others = [q["lower_bound"] for q in runs if abs(q["weights"][0] - 0.5) > 1e-9]
    assert len(blobs) == 14 and max(blobs) - min(blobs) <= 1e-9 and min(blobs) - max(others) >= 2.0
    return egx.GaussianMixture(r["weights"], r["means"][:, :NX], r["covariances"][:, :NX, :NX])


def _builder(egx, kpls_dim):
    theta = [0.05] * (NX if kpls_dim is None else kpls_dim)
    return egx.GpMixture.params().n_clusters(2).recombination("hard").regression_spec(egx.RegressionSpec.CONSTANT) \
        .correlation_spec(egx.CorrelationSpec.SQUARED_EXPONENTIAL).theta_tunings([egx.ThetaTuning.Fixed(theta)]) \
        .kpls_dim(kpls_dim).seed(0)


@pytest.mark.parametrize("kpls_dim", [None, 3])
def test_mixture_fit_at_40_columns(egx, oracle_gmx, kpls_dim):
    """The fit succeeds (the narrow training refuses 41 columns), the rows' clusters are the blobs, and the predictions are
    those of the same builder given the oracle's mixture, at the project's 1e-6 prediction bar."""
    moe = _builder(egx, kpls_dim).fit(X, Y)
    assert moe.gmx.n_clusters == 2 and moe.gmx.means.shape == (2, NX) and moe.gmx.lower_bounds_.shape == (20,)
    label = moe.gmx.predict(X)
    assert len(set(label[BLOB == 0])) == 1 and len(set(label[BLOB == 1])) == 1 and label[0] != label[1]
    assert sorted(e.training_data[0].shape[0] for e in moe.experts) == [120, 120]
    ref = _builder(egx, kpls_dim).gmx(oracle_gmx).fit(X, Y)
    a, b = moe.predict(XQ), ref.predict(XQ)
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    print("kpls", kpls_dim, "max prediction difference", err.max())
    assert np.all(err <= 1e-6)
    va, vb = moe.predict_var(XQ), ref.predict_var(XQ)
    assert np.all(np.abs(va - vb) <= 1e-6 * np.maximum(1.0, np.abs(vb)))


def test_sparse_mixture_at_40_columns(egx):
    mix = egx.SparseGpMix(n_clusters=2, recombination="hard", nz=20, seed=0, n_start=2, max_eval=20).fit(X, Y)
    pred = np.asarray(mix.predict(XQ)).ravel()
    assert pred.shape == (16,) and np.all(np.isfinite(pred))
    # the blobs' levels of y are 30 apart and y spreads by about 1.3 inside a blob: a query answered by the other blob's
    # expert, or by none, misses by far more than 5
    assert np.all(np.abs(pred - _data(16, 1)[1]) <= 5.0)


def test_egor_suggests_at_40_columns(egx):
    xlim = np.tile(np.array([[-6.0, 6.0]]), (NX, 1))
    x_doe, y_doe, _ = _data(120, 2)
    x_doe = np.clip(x_doe, -6.0, 6.0)
    ego = egx.Egor(xlim, gp_config=egx.GpConfig(n_clusters=2, recombination="hard", kpls_dim=3), seed=1)
    first = ego.suggest(x_doe, y_doe.reshape(-1, 1))
    assert first.shape == (1, NX) and np.all(first >= -6.0) and np.all(first <= 6.0)
    assert np.array_equal(first, ego.suggest(x_doe, y_doe.reshape(-1, 1)))
