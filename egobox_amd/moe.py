"""Mixture of experts around the GPU GP experts: training (clustering + expert fits) and predict-side recombination.

Training mirrors egobox-moe's `GpMixture::params().n_clusters(k).fit(..)`:
  GpMixtureParams / .fit (train, train_on_clusters) crates/moe/src/parameters.rs, crates/moe/src/algorithm.rs:72-205
  optimize_heaviside_factor, check_number_of_points crates/moe/src/algorithm.rs:353-405
  extract_part, sort_by_cluster                     crates/moe/src/algorithm.rs:1111-1121, clustering.rs:33-56
  GaussianMixture.fit                               GaussianMixtureModel::params(k).n_runs(20).fit, algorithm.rs:120-123
The Gaussian mixture is trained inside libegx_gp_hip.so (egx_gmm_fit: full-covariance EM, the restarts in lock-step on the
GPU); the experts go through `GpMixture.fit_experts`, clusters of equal size in lock-step.  With several allowed
(regression, correlation) pairs (`expert_specs`) every cluster's expert is chosen by find_best_expert's 5-fold
cross-validation (algorithm.rs:209-347), its folds fitted and asked in lock-step (egobox_amd/cv.py); a trained mixture
answers the cross-validation scores of GpMetrics (crates/moe/src/metrics.rs).  Not here: NbClusters::Auto, sparse-GP
experts, a k-means initialisation.

Prediction mirrors what egobox-moe does with the trained mixture:
  GaussianMixture.predict_probas / predict        crates/moe/src/gaussian_mixture.rs:114-121, 231-283, 305-316
  GpMixture.predict_smooth / predict_var_smooth   crates/moe/src/algorithm.rs:411-423, 670-685, 789-809
  GpMixture.predict_hard  / predict_var_hard      crates/moe/src/algorithm.rs:879-935
  GpMixture.predict_(var_)gradients smooth / hard crates/moe/src/algorithm.rs:691-783, 942-1010;
  GaussianMixture.predict_probas_derivatives      crates/moe/src/gaussian_mixture.rs:127-170

Differences that matter on a GPU: the reference's hard recombination calls the expert ONCE PER ROW with a
1 x nx batch (each a full n^2 triangular solve for the variance); here queries are routed once and every
expert gets one batched call on its subset.  With several GPUs expert e lives on rank e mod G
(BASELINE config 5) and one all-reduce of the weighted vectors replaces the fold over experts.
With GPU experts the recombinations of values, variances AND their x-gradients, the responsibilities and their
derivatives run inside libegx_gp_hip.so (egx_moe_predict_valvar, egx_moe_predict_valvar_gradients,
egx_gmx_predict_probas(_derivatives)); the numpy forms below serve duck-typed experts and the CPU tests.
"""
from __future__ import annotations

import copy
import math

import numpy as np

from ._lib import ERR_INVALID_VALUE, ERR_LINALG, ClusteringError, InvalidValueError
from .cv import GpMetrics, cross_validate, cross_validate_surrogates, expert_pairs
from .cv import pair_name as _pair_name
from .cv import select_expert as _select_expert


class GaussianMixture:
    """Responsibilities of a fitted Gaussian mixture (weights (k,), means (k,nx), covariances (k,nx,nx))."""

    def __init__(self, weights, means, covariances, heaviside_factor=1.0):
        self.weights = np.asarray(weights, dtype=np.float64)
        self.means = np.atleast_2d(np.asarray(means, dtype=np.float64))
        self.covariances = np.asarray(covariances, dtype=np.float64)
        k, nx = self.means.shape
        if self.weights.shape != (k,) or self.covariances.shape != (k, nx, nx):
            raise ValueError("weights (k,), means (k,nx), covariances (k,nx,nx) expected")
        # precisions_chol[k] = (chol(cov_k)^-1)^T, gaussian_mixture.rs:182-205
        self.precisions_chol = np.empty((k, nx, nx))
        for i in range(k):
            c = np.linalg.cholesky(self.covariances[i])
            self.precisions_chol[i] = np.linalg.solve(c, np.eye(nx)).T
        self.set_heaviside_factor(heaviside_factor)

    @classmethod
    def fit(cls, data, n_clusters, n_runs=20, seed=42, max_iter=100, tol=1e-3, reg_covar=1e-6, init_means=None, device=-1):
        """Train a full-covariance mixture on `data` (n, dim) by EM with `n_runs` restarts in lock-step on the GPU
        (egx_gmm_fit; GaussianMixtureModel::params(n_clusters).n_runs(20).fit, crates/moe/src/algorithm.rs:120-123) and
        keep the restart with the greatest lower bound.  `init_means` (n_runs, n_clusters, dim) are the restarts' initial
        means; by default restart r starts from n_clusters distinct rows of `data` drawn by numpy.random.default_rng(seed)
        (not the reference's Xoshiro256Plus stream).  The result carries lower_bound_, n_iter_, and per restart
        lower_bounds_, n_iters_, statuses_ (0 converged, 1 stopped at max_iter, 2 failed) and best_run_.  dim <= 36; wider
        rows: fit_wide."""
        return cls._fit("egx_gmm_fit", data, n_clusters, n_runs, seed, max_iter, tol, reg_covar, init_means, device)

    @classmethod
    def fit_wide(cls, data, n_clusters, n_runs=20, seed=42, max_iter=100, tol=1e-3, reg_covar=1e-6, init_means=None, device=-1):
        """`fit` for rows up to 128 wide (egx_gmm_fit_wide: the same EM with its two O(dim^2) products per row on the FP64
        matrix unit).  Same arguments, attributes and defaults; narrow rows are taken too and agree with `fit` to rounding,
        not to the bit."""
        return cls._fit("egx_gmm_fit_wide", data, n_clusters, n_runs, seed, max_iter, tol, reg_covar, init_means, device)

    @classmethod
    def _fit(cls, entry, data, n_clusters, n_runs, seed, max_iter, tol, reg_covar, init_means, device):
        from . import _lib as L
        data = np.asarray(data, dtype=np.float64)
        if data.ndim != 2:
            raise InvalidValueError(ERR_INVALID_VALUE, f"data must be (n, dim), got shape {data.shape}")
        data = np.ascontiguousarray(data)
        n, dim = data.shape
        k, n_runs = int(n_clusters), int(n_runs)
        if k < 1 or k > n or n_runs < 1:
            raise InvalidValueError(ERR_INVALID_VALUE, f"n >= n_clusters >= 1 and n_runs >= 1 expected (n {n}, n_clusters {k}, "
                                                       f"n_runs {n_runs})")
        if init_means is None:
            rng = np.random.default_rng(seed)
            init_means = np.stack([data[rng.choice(n, size=k, replace=False)] for _ in range(n_runs)])
        init_means = np.ascontiguousarray(init_means, dtype=np.float64)
        if init_means.shape != (n_runs, k, dim):
            raise InvalidValueError(ERR_INVALID_VALUE, f"init_means must be (n_runs, n_clusters, dim) = {(n_runs, k, dim)}, "
                                                       f"got {init_means.shape}")
        lib = L.load()
        cfg = L.GmmConfig()
        lib.egx_gmm_config_default(cfg)
        cfg.n_clusters, cfg.n_runs, cfg.max_iter, cfg.device = k, n_runs, int(max_iter), int(device)
        cfg.tol, cfg.reg_covar = float(tol), float(reg_covar)
        weights, means, covs = np.empty(k), np.empty((k, dim)), np.empty((k, dim, dim))
        lbs = np.empty(n_runs)
        n_iters, statuses = np.zeros(n_runs, dtype=np.int32), np.zeros(n_runs, dtype=np.int32)
        best = L.C.c_int32(-1)
        all_w, all_m, all_c = np.empty((n_runs, k)), np.empty((n_runs, k, dim)), np.empty((n_runs, k, dim, dim))
        rc = getattr(lib, entry)(cfg, L.dptr(data), n, dim, L.dptr(init_means), L.dptr(weights), L.dptr(means), L.dptr(covs),
                                 L.dptr(lbs), n_iters.ctypes.data_as(L.c_int32_p), statuses.ctypes.data_as(L.c_int32_p),
                                 L.C.byref(best), L.dptr(all_w), L.dptr(all_m), L.dptr(all_c))
        if rc == ERR_LINALG:
            raise ClusteringError(rc, lib.egx_last_error().decode("utf-8", "replace"))
        L.check(rc)
        gm = cls(weights, means, covs)
        gm.best_run_ = int(best.value)
        gm.lower_bounds_, gm.n_iters_, gm.statuses_ = lbs, n_iters, statuses
        gm.lower_bound_, gm.n_iter_ = float(lbs[gm.best_run_]), int(n_iters[gm.best_run_])
        gm.all_weights_, gm.all_means_, gm.all_covariances_ = all_w, all_m, all_c
        return gm

    def marginal(self, nx, heaviside_factor=1.0):
        """The mixture of the first nx coordinates (crates/moe/src/algorithm.rs:126-134: a mixture trained on [x, y] serves
        the x-space); the training record (lower_bound_, ...) is carried over."""
        gmx = GaussianMixture(self.weights, self.means[:, :nx], self.covariances[:, :nx, :nx], heaviside_factor)
        for name in ("best_run_", "lower_bounds_", "n_iters_", "statuses_", "lower_bound_", "n_iter_"):
            if hasattr(self, name):
                setattr(gmx, name, getattr(self, name))
        return gmx

    def set_heaviside_factor(self, f):
        """gaussian_mixture.rs:105-110: refresh the log-determinants."""
        self.heaviside_factor = float(f)
        precs = self.precisions_chol * self.heaviside_factor ** -0.5
        self.log_det = np.log(np.einsum("kii->ki", precs)).sum(axis=1)
        return self

    @property
    def n_clusters(self):
        return self.means.shape[0]

    def _log_gaussian_prob(self, x):
        nx = self.means.shape[1]
        precs = self.precisions_chol * self.heaviside_factor ** -0.5
        q = np.empty((x.shape[0], self.n_clusters))
        for k in range(self.n_clusters):  # one (m,nx)x(nx,nx) product per cluster
            diff = (x - self.means[k]) @ precs[k]
            q[:, k] = np.einsum("ij,ij->i", diff, diff)
        return -0.5 * (q + nx * math.log(2.0 * math.pi)) + self.log_det

    def _log_resp(self, x):
        wlp = self._log_gaussian_prob(x) + np.log(self.weights)
        e = np.where(wlp <= -307.0, 0.0, np.exp(wlp))
        s = e.sum(axis=1)
        norm = np.where(np.abs(s) < np.finfo(float).eps, 0.0, np.log(np.where(s > 0, s, 1.0)))
        return wlp - norm[:, None]

    def predict_probas(self, x):
        x = np.atleast_2d(np.asarray(x, dtype=np.float64))
        if self.n_clusters == 1:
            return np.ones((x.shape[0], 1))
        return np.exp(self._log_resp(x))

    def predict_probas_device(self, x, device=-1, xtypes=None):
        """The same responsibilities from the library (egx_gmx_predict_probas: one lane per point on the GPU); what the
        library-side recombination of `GpMixture` consumes.  xtypes (`egobox_amd.mixint.XType`s): the points are cast on the
        device first (egx_gmx_predict_probas_mixint)."""
        from . import _lib as L
        lib = L.load()
        x = np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=np.float64)))
        k, nx = self.means.shape
        out = np.empty((x.shape[0], k))
        if xtypes:
            from .mixint import _c_xtypes
            arr, nxt, _keep = _c_xtypes(xtypes)
            L.check(lib.egx_gmx_predict_probas_mixint(int(device), L.dptr(np.ascontiguousarray(self.weights)),
                                                      L.dptr(np.ascontiguousarray(self.means)),
                                                      L.dptr(np.ascontiguousarray(self.precisions_chol)), k, nx,
                                                      self.heaviside_factor, L.dptr(x), x.shape[0], L.dptr(out), arr, nxt))
            return out
        L.check(lib.egx_gmx_predict_probas(int(device), L.dptr(np.ascontiguousarray(self.weights)),
                                           L.dptr(np.ascontiguousarray(self.means)),
                                           L.dptr(np.ascontiguousarray(self.precisions_chol)), k, nx,
                                           self.heaviside_factor, L.dptr(x), x.shape[0], L.dptr(out)))
        return out

    def predict_probas_derivatives_device(self, x, device=-1, xtypes=None):
        """d p_c / d x, (m, k, nx), from the library (egx_gmx_predict_probas_derivatives, one lane per point on the GPU);
        xtypes: at the cast points (egx_gmx_predict_probas_derivatives_mixint)."""
        from . import _lib as L
        lib = L.load()
        x = np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=np.float64)))
        k, nx = self.means.shape
        if 3 * nx + k > 320:  # (the kernel keeps one point per lane with 3 nx + k doubles of LDS scratch: beyond that, the host form)
            if xtypes:
                from .mixint import cast_to_discrete_values
                x = cast_to_discrete_values(xtypes, x)
            return self.predict_probas_derivatives(x)
        out = np.empty((x.shape[0], k, nx))
        if xtypes:
            from .mixint import _c_xtypes
            arr, nxt, _keep = _c_xtypes(xtypes)
            L.check(lib.egx_gmx_predict_probas_derivatives_mixint(int(device), L.dptr(np.ascontiguousarray(self.weights)),
                                                                  L.dptr(np.ascontiguousarray(self.means)),
                                                                  L.dptr(np.ascontiguousarray(self.precisions_chol)), k, nx,
                                                                  self.heaviside_factor, L.dptr(x), x.shape[0], L.dptr(out), arr, nxt))
            return out
        L.check(lib.egx_gmx_predict_probas_derivatives(int(device), L.dptr(np.ascontiguousarray(self.weights)),
                                                       L.dptr(np.ascontiguousarray(self.means)),
                                                       L.dptr(np.ascontiguousarray(self.precisions_chol)), k, nx,
                                                       self.heaviside_factor, L.dptr(x), x.shape[0], L.dptr(out)))
        return out

    def predict(self, x):
        x = np.atleast_2d(np.asarray(x, dtype=np.float64))
        return np.argmax(np.exp(self._log_resp(x)), axis=1)

    def pdfs(self, x):
        return np.exp(self._log_gaussian_prob(np.asarray(x, dtype=np.float64).reshape(1, -1))[0])

    def predict_probas_derivatives(self, x):
        """gaussian_mixture.rs:127-170, all points at once -> (m, k, nx): d p_i(x) / d x with p_i = u_i / v,
        u_i = w_i pdf_i(x), v = sum_i u_i."""
        x = np.atleast_2d(np.asarray(x, dtype=np.float64))
        u = self.weights * np.exp(self._log_gaussian_prob(x))                      # (m, k)
        v = u.sum(axis=1)                                                          # (m,)
        precs = np.einsum("kij,klj->kil", self.precisions_chol, self.precisions_chol) / self.heaviside_factor
        deriv = np.einsum("mkj,kjl->mkl", x[:, None, :] - self.means[None, :, :], precs)
        uprime = -deriv * u[:, :, None]                                            # (m, k, nx)
        vprime = uprime.sum(axis=1)                                                # (m, nx)
        return (uprime * v[:, None, None] - u[:, :, None] * vprime[:, None, :]) / (v * v)[:, None, None]


GMM_NARROW_MAX_DIM = 36  # the widest row GaussianMixture.fit takes (egx_gmm_fit); beyond: fit_wide, up to 128


def train_mixture(data, n_clusters, **kw):
    """The mixture of a mixture of experts on the joined rows `data` (n, dim): GaussianMixture.fit up to 36 columns -- what
    it has always been, to the bit -- and GaussianMixture.fit_wide beyond.  Keywords as GaussianMixture.fit."""
    dim = np.shape(data)[1] if np.ndim(data) == 2 else 0
    fit = GaussianMixture.fit if dim <= GMM_NARROW_MAX_DIM else GaussianMixture.fit_wide
    return fit(data, n_clusters, **kw)


def extract_part(data, quantile):
    """crates/moe/src/algorithm.rs:1111-1121: one row out of `quantile` (rows 0, quantile, 2 quantile, ..) and the rest."""
    data = np.asarray(data)
    idx = np.arange(data.shape[0])
    return data[idx % quantile == 0], data[idx % quantile != 0]


def sort_by_cluster(n_clusters, data, clustering):
    """crates/moe/src/clustering.rs:33-56: the rows of `data` per cluster, in their order."""
    data, clustering = np.asarray(data), np.asarray(clustering)
    return [data[clustering == c] for c in range(n_clusters)]


def check_number_of_points(clusters, dim, mean):
    """crates/moe/src/algorithm.rs:381-405, as written there: `cluster.len()` counts the ELEMENTS of the (rows, nx + 1)
    array.  `mean` is the regression model (ConstantMean / LinearMean / QuadraticMean)."""
    if len(clusters) > 1:
        need = {2: (dim + 1) * (dim + 2) // 2, 1: dim + 1}.get(mean.code, 1)
        for c in clusters:
            if np.asarray(c).size < need:
                raise ClusteringError(ERR_INVALID_VALUE,
                                      f"Not enough points in training set. Need {need} points, got {np.asarray(c).size}")


def check_three_points(clusters):
    """crates/moe/src/algorithm.rs:168-173."""
    if len(clusters) > 1:
        for c in clusters:
            if np.asarray(c).shape[0] < 3:
                raise ClusteringError(ERR_INVALID_VALUE,
                                      f"Not enough points in cluster, requires at least 3, got {np.asarray(c).shape[0]}")


HEAVISIDE_GRID = np.linspace(0.1, 2.1, 20)


def heaviside_errors(experts, gmx, xtest, ytest, **kw):
    """The error of every grid factor, crates/moe/src/algorithm.rs:363-369: ||pred - y||_2 / ||x_test||_2 with the smooth
    recombination of the trained experts under a copy of `gmx` that carries the factor."""
    xtest = np.atleast_2d(np.asarray(xtest, dtype=np.float64))
    ytest = np.asarray(ytest, dtype=np.float64).ravel()
    errors = np.empty(HEAVISIDE_GRID.size)
    for i, f in enumerate(HEAVISIDE_GRID):
        gmx2 = copy.copy(gmx).set_heaviside_factor(f)
        pred = GpMixture(experts, gmx2, "smooth", **kw).predict(xtest)
        errors[i] = math.sqrt(np.sum((pred - ytest) ** 2)) / math.sqrt(np.sum(xtest * xtest))
    return errors


def optimize_heaviside_factor(experts, gmx, xtest, ytest, recombination="smooth", **kw):
    """crates/moe/src/algorithm.rs:353-378: the grid factor of the smallest error (the first among equals), 1 when every
    error is below 1e-6, when the recombination is hard or with one cluster."""
    if recombination == "hard" or gmx.n_clusters == 1:
        return 1.0
    errors = heaviside_errors(experts, gmx, xtest, ytest, **kw)
    if errors.max() < 1e-6:
        return 1.0
    return float(HEAVISIDE_GRID[int(np.argmin(errors))])


class GpMixtureParams:
    """Builder of a trained mixture of experts, crates/moe/src/parameters.rs (defaults :142-159, 246-253): setters return
    self, `.fit(x, y)` trains the Gaussian mixture on [x, y] on the GPU and one GP expert per cluster."""

    def __init__(self):
        from . import gp as G
        self._n_clusters = 1
        self._recombination, self._heaviside_factor = "smooth", 1.0  # parameters.rs:249
        self._mean, self._corr = G.ConstantMean(), G.SquaredExponentialCorr()
        self._theta_tunings = [G.ThetaTuning.default()]
        self._kpls_dim = None
        self._n_start = 10
        self._max_eval = G.GP_COBYLA_MAX_EVAL
        self._gmx = None
        self._seed = 42
        self._device = -1
        self._n_runs = 20  # algorithm.rs:121
        self._expert_pairs = None  # several allowed (mean, correlation) pairs: expert_specs
        self._selection_tuning = None  # ThetaTuning of the selection's fold fits (None: the pairs' defaults): selection_tuning

    def n_clusters(self, n_clusters):
        if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)):
            raise NotImplementedError("n_clusters must be a number: NbClusters::Auto (find_best_number_of_clusters) is not "
                                      "implemented")
        if n_clusters < 1:
            raise InvalidValueError(ERR_INVALID_VALUE, f"n_clusters must be at least 1, got {n_clusters}")
        self._n_clusters = int(n_clusters)
        return self

    def recombination(self, mode, heaviside_factor=None):
        """"hard", or "smooth" with its heaviside factor; smooth without one (the reference's Smooth(None)) chooses the
        factor on one row out of five held back from the training (algorithm.rs:106-113, 179-193)."""
        mode = str(getattr(mode, "name", mode)).lower()
        if mode not in ("hard", "smooth"):
            raise InvalidValueError(ERR_INVALID_VALUE, "recombination must be 'hard' or 'smooth'")
        if heaviside_factor is not None and not float(heaviside_factor) > 0.0:
            raise InvalidValueError(ERR_INVALID_VALUE, "heaviside_factor must be positive")
        self._recombination = mode
        self._heaviside_factor = None if heaviside_factor is None else float(heaviside_factor)
        return self

    def regression_spec(self, spec):
        """One RegressionSpec flag (or a mean object); several at once ask for the cross-validated expert selection of
        find_best_expert (algorithm.rs:209-347): that is `expert_specs`."""
        from . import gpx
        self._mean = gpx._single(spec, gpx._REGR, "regression_spec") if isinstance(spec, (int, gpx.RegressionSpec)) else spec
        return self

    def correlation_spec(self, spec):
        from . import gpx
        self._corr = gpx._single(spec, gpx._CORR, "correlation_spec") if isinstance(spec, (int, gpx.CorrelationSpec)) else spec
        return self

    def expert_specs(self, regression=1, correlation=1):
        """The allowed experts as two flag sets (RegressionSpec, CorrelationSpec; the defaults are CONSTANT and
        SQUARED_EXPONENTIAL): with more than one (regression, correlation) pair every cluster's expert is the pair of the
        smallest 5-fold cross-validation error (`select_expert`: find_best_expert, algorithm.rs:209-347), then trained on
        the whole cluster as ever.  One pair is the reference's shortcut: no fold is fitted."""
        pairs = expert_pairs(regression, correlation)
        if len(pairs) == 1:
            self._mean, self._corr, self._expert_pairs = pairs[0][0](), pairs[0][1](), None
        else:
            self._expert_pairs = pairs
        return self

    def select_expert(self, cluster_x, cluster_y, theta_tuning=None):
        """(winning name, [(name, error), ..]) among the allowed pairs on one cluster (egobox_amd/cv.py select_expert).  The fold
        fits use the pair's default GpParams plus kpls_dim, not this builder's tunings (expertise_macros.rs:22);
        `theta_tuning` overrides that (extension)."""
        pairs = self._expert_pairs or [(type(self._mean), type(self._corr))]
        if theta_tuning is None:
            theta_tuning = self._selection_tuning
        return _select_expert(pairs, cluster_x, cluster_y, kpls_dim=self._kpls_dim, theta_tuning=theta_tuning, device=self._device)

    def selection_tuning(self, theta_tuning):
        """Extension: the ThetaTuning `fit` hands to `select_expert` for the selection's fold fits (None: the pairs' defaults,
        as the reference, expertise_macros.rs:22).  `fit` reaches `select_expert` only through `_train_on_clusters`, so without
        this a trained mixture could not use the `theta_tuning` extension of `select_expert`."""
        self._selection_tuning = theta_tuning
        return self

    def theta_tunings(self, theta_tunings):
        """One tuning for every expert, or one per cluster (algorithm.rs:297-302)."""
        self._theta_tunings = list(theta_tunings)
        if not self._theta_tunings:
            raise InvalidValueError(ERR_INVALID_VALUE, "at least one theta tuning expected")
        return self

    def n_start(self, n_start):
        self._n_start = int(n_start)
        return self

    def max_eval(self, max_eval):
        self._max_eval = int(max_eval)
        return self

    def kpls_dim(self, kpls_dim):
        self._kpls_dim = kpls_dim
        return self

    def gmx(self, gmx):
        """A ready mixture of the x-space instead of a trained one (the reference's .gmx(), algorithm.rs:116-117)."""
        self._gmx = gmx
        return self

    def seed(self, seed):
        self._seed = seed
        return self

    def device(self, device):
        self._device = int(device)
        return self

    def n_runs(self, n_runs):
        """Extension: the restarts of the mixture's EM (the reference fixes 20, algorithm.rs:121)."""
        self._n_runs = int(n_runs)
        return self

    def _expert_params(self, nc, pair=None):
        from . import gp as G
        tt = self._theta_tunings
        if len(tt) != 1 and len(tt) != self._n_clusters:
            raise InvalidValueError(ERR_INVALID_VALUE, f"theta_tunings: 1 or n_clusters ({self._n_clusters}) expected, "
                                                       f"got {len(tt)}")
        mean, corr = (self._mean, self._corr) if pair is None else (pair[0](), pair[1]())
        return G.GpParams(mean, corr).theta_tuning(tt[0] if len(tt) == 1 else tt[nc]).n_start(self._n_start) \
            .max_eval(self._max_eval).kpls_dim(self._kpls_dim).device(self._device)

    def fit(self, x, y):
        """GpMixtureValidParams::train, crates/moe/src/algorithm.rs:72-140."""
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        if x.ndim != 2 or y.shape[0] != x.shape[0]:
            raise InvalidValueError(ERR_INVALID_VALUE, f"x (n, nx) and y (n,) expected, got {x.shape} and {y.shape}")
        n, nx = x.shape
        k = self._n_clusters
        if k > n:
            raise InvalidValueError(ERR_INVALID_VALUE, f"n_clusters ({k}) exceeds the number of training points ({n})")
        self._expert_params(0)
        data = np.column_stack([x, y])
        smooth_none = self._recombination == "smooth" and self._heaviside_factor is None and k > 1
        if self._gmx is not None:
            gmx = self._gmx
        else:
            training = extract_part(data, 5)[1] if smooth_none else data
            gmm = train_mixture(training, k, n_runs=self._n_runs, seed=self._seed, device=self._device)
            gmx = gmm.marginal(nx, self._heaviside_factor if self._heaviside_factor is not None else 1.0)
        return self._train_on_clusters(x, y, data, gmx, smooth_none)

    def _train_on_clusters(self, x, y, data, gmx, smooth_none):
        """train_on_clusters, crates/moe/src/algorithm.rs:144-205."""
        nx = x.shape[1]
        clusters = sort_by_cluster(gmx.n_clusters, data, gmx.predict(x))
        # (several allowed regressions: the most demanding one counts, algorithm.rs:387-393)
        check_number_of_points(clusters, nx, self._mean if not self._expert_pairs
                               else max((m() for m, _ in self._expert_pairs), key=lambda m: m.code))
        check_three_points(clusters)
        cxs, cys = [c[:, :nx] for c in clusters], [c[:, nx] for c in clusters]
        expert_errors = None
        if self._expert_pairs:
            # find_best_expert per cluster (algorithm.rs:167-177 -> :209-347): the choice by cross-validation, then the winner
            # trained on the whole cluster under this builder's tunings
            by_name = {_pair_name(m, c): (m, c) for m, c in self._expert_pairs}
            expert_errors, experts = [], []
            for i in range(len(clusters)):
                name, table = self.select_expert(cxs[i], cys[i])
                expert_errors.append(table)
                experts.append(self._expert_params(i, by_name[name]).fit(cxs[i], cys[i]))
            moe = GpMixture(experts, gmx, self._recombination)
        elif len(self._theta_tunings) == 1 and self._kpls_dim is None:
            moe = GpMixture.fit_experts(self._expert_params(0), cxs, cys, gmx, self._recombination)
        else:  # a tuning per cluster, or the PLS rotations of each cluster's own data: one fit per expert
            moe = GpMixture([self._expert_params(i).fit(cxs[i], cys[i]) for i in range(len(clusters))], gmx,
                            self._recombination)
        if smooth_none:
            test = extract_part(data, 5)[0]
            factor = optimize_heaviside_factor(moe.experts, gmx, test[:, :nx], test[:, nx], self._recombination)
            final = copy.copy(self).recombination("smooth", factor).fit(x, y)  # on ALL data, algorithm.rs:188-193
            final.heaviside_stage_ = moe  # the mixture the factor was chosen on (its gmx saw four rows out of five)
            return final
        moe.training_data = (x, y)
        moe.params_ = self
        moe.expert_errors_ = expert_errors  # per cluster the selection's [(name, error), ..]; None without a selection
        return moe


class GpMixture(GpMetrics):
    """Experts + mixture.  `GpMixture.params()` builds and trains one; the constructor takes trained experts (`experts[i]` is
    None for experts that live on another rank).  A mixture trained by `GpMixtureParams.fit` (it keeps `params_` and
    `training_data`) answers the cross-validation scores of GpMetrics (crates/moe/src/metrics.rs:19-144)."""

    def _cv_targets(self):
        if getattr(self, "params_", None) is None:
            raise InvalidValueError(ERR_INVALID_VALUE, "cross-validation scores need a mixture trained by GpMixtureParams.fit")
        return self.training_data[1]

    def _cv_folds(self, kfold, want_var):
        y = self._cv_targets()
        x, p = self.training_data[0], self.params_
        if p._n_clusters == 1 and not p._expert_pairs and p._gmx is None:
            # one cluster: the folds are those of its one expert, fitted and asked in lock-step
            return cross_validate(p._expert_params(0), x, y, kfold, want_var)
        # several clusters: the clusters' sizes differ from fold to fold, every fold is a training of its own
        return cross_validate_surrogates(p.fit, x, y, kfold, want_var)

    @staticmethod
    def params():
        return GpMixtureParams()

    def __init__(self, experts, gmx, recombination="hard", rank=0, world=1, device=None, sweep=None):
        """`sweep`: the rank's `egobox_amd.Sweep` (its RCCL communicator carries the recombination's one all-gather
        inside the library, egx_moe_predict_valvar); without it a multi-rank mixture reduces through torch.distributed."""
        self.experts, self.gmx = list(experts), gmx
        self.sweep = sweep
        self.recombination = recombination.lower()
        if self.recombination not in ("hard", "smooth"):
            raise ValueError("recombination must be 'hard' or 'smooth'")
        if len(self.experts) != gmx.n_clusters:
            raise ValueError("one expert per cluster expected")
        self.rank, self.world, self.device = rank, world, device
        self.n_in_flight = 2

    @classmethod
    def fit_experts(cls, params, cluster_xs, cluster_ys, gmx, recombination="hard", **kw):
        """The expert loop of egobox-moe (crates/moe/src/algorithm.rs:167-177: one GP per cluster, fitted one after the other)
        with the experts of EQUAL training-set size fitted in lock-step: `params` is a `GpParams` with ThetaTuning.Fixed,
        cluster_xs[i] / cluster_ys[i] the training set of cluster i (`GpMixtureParams.fit` clusters and calls this).
        Clusters of one size go through `GpParams.fit_group` (one launch sequence for all of them), the others through
        `fit`; every expert is bit for bit what `fit` alone gives."""
        k = len(cluster_xs)
        experts = [None] * k
        by_shape = {}
        for i in range(k):
            by_shape.setdefault(np.asarray(cluster_xs[i]).shape, []).append(i)
        for shape, idx in by_shape.items():
            if len(idx) > 1:
                gps = params.fit_group(np.stack([np.asarray(cluster_xs[i], dtype=np.float64) for i in idx]),
                                       np.stack([np.asarray(cluster_ys[i], dtype=np.float64).reshape(shape[0]) for i in idx]))
                for i, g in zip(idx, gps):
                    experts[i] = g
            else:
                experts[idx[0]] = params.fit(cluster_xs[idx[0]], cluster_ys[idx[0]])
        return cls(experts, gmx, recombination, **kw)

    def _mine(self, i):
        return i % self.world == self.rank and self.experts[i] is not None

    #: the `XType`s of a mixed-integer mixture (set by `egobox_amd.mixint.MixintGpMixture`, whose experts carry them as well):
    #: the responsibilities are then taken at the cast point, on the device
    xtypes = None

    def _probas(self, dev, x):
        return dev(x, xtypes=self.xtypes) if self.xtypes else dev(x)

    def _allreduce(self, *arrays):
        if self.world == 1:
            return arrays
        import torch
        import torch.distributed as dist
        t = torch.from_numpy(np.stack(arrays))
        if self.device is not None:
            t = t.to(self.device)
        dist.all_reduce(t)  # ncclAllReduce(sum) over xGMI; gloo in the CPU tests
        out = t.cpu().numpy()
        return tuple(out[i] for i in range(len(arrays)))

    def _library_handles(self):
        """(ids, handles, sparse) of this rank's experts when ALL of them are GPU handles of ONE kind -- dense (egx_gp*) or
        sparse (egx_sgp*: SparseGaussianProcess / SgpHandle) -- and the collective, if any, is the library's: then the
        recombination runs inside libegx_gp_hip.so (egx_moe_predict_valvar, or its _sgp twin).  A mixture of both kinds
        takes the numpy fold below."""
        from .sgp import SgpHandle
        if self.world > 1 and self.sweep is None:
            return None
        ids, hs, kinds = [], [], set()
        for i, e in enumerate(self.experts):
            if not self._mine(i):
                continue
            owner = e if isinstance(e, SgpHandle) else getattr(e, "_h", None)
            h = getattr(owner, "_h", None)
            if h is None or not h:
                return None
            kinds.add(isinstance(owner, SgpHandle))
            ids.append(i)
            hs.append(h)
        if len(kinds) > 1:
            return None
        return ids, hs, bool(kinds and kinds.pop())

    def _predict_valvar_library(self, x, lib_handles, want_val, want_var):
        import ctypes as C
        from . import _lib as L
        lib = L.load()
        ids, hs, sparse = lib_handles
        m, d = x.shape
        k = len(self.experts)
        dev = getattr(self.gmx, "predict_probas_device", None)  # the library's kernel; a duck-typed mixture keeps its own
        probas = np.ascontiguousarray(self._probas(dev, x) if dev is not None else self.gmx.predict_probas(x), dtype=np.float64)
        harr = (C.c_void_p * max(1, len(hs)))(*[h.value if hasattr(h, "value") else h for h in hs])
        iarr = np.asarray(ids, dtype=np.int32)
        val = np.empty(m) if want_val else None
        var = np.empty(m) if want_var else None
        entry = lib.egx_moe_predict_valvar_sgp if sparse else lib.egx_moe_predict_valvar
        L.check(entry(self.sweep._h if self.sweep is not None else None, harr,
                      iarr.ctypes.data_as(L.c_int32_p), len(hs), k, L.dptr(probas), L.dptr(x), m, d,
                      1 if self.recombination == "smooth" else 0,
                      L.dptr(val) if want_val else None, L.dptr(var) if want_var else None))
        return (val if want_val else np.zeros(m)), (var if want_var else np.zeros(m))

    def predict_valvar(self, x, want_val=True, want_var=True):
        x = np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=np.float64)))
        m = x.shape[0]
        lib_handles = self._library_handles()
        if lib_handles is not None and m > 0:
            return self._predict_valvar_library(x, lib_handles, want_val, want_var)
        val, var = np.zeros(m), np.zeros(m)
        smooth = self.recombination == "smooth"
        if smooth:
            p = self.gmx.predict_probas(x)
        else:
            c = self.gmx.predict(x)

        def run(i):
            e = self.experts[i]
            idx = None if smooth else np.flatnonzero(c == i)
            if idx is not None and idx.size == 0:
                return i, idx, None, None
            xi = x if smooth else x[idx]
            if want_val and want_var:
                y, v = e.predict_valvar(xi)
            elif want_val:
                y, v = e.predict(xi), None
            else:
                y, v = None, e.predict_var(xi)
            return i, idx, y, v

        mine = [i for i in range(len(self.experts)) if self._mine(i)]
        # every expert owns a handle with its own HIP streams: a few in flight hide each other's launch gaps
        if len(mine) > 1 and self.n_in_flight > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(min(self.n_in_flight, len(mine))) as pool:
                results = list(pool.map(run, mine))
        else:
            results = [run(i) for i in mine]
        for i, idx, y, v in results:
            if smooth:
                if y is not None:
                    val += y * p[:, i]
                if v is not None:
                    var += v * p[:, i] * p[:, i]
            elif idx.size:
                if y is not None:
                    val[idx] = y
                if v is not None:
                    var[idx] = v
        val, var = self._allreduce(val, var)
        return val, var

    def predict(self, x):
        return self.predict_valvar(x, True, False)[0]

    def sample(self, x, n_traj):
        """GpMixture::sample (crates/moe/src/algorithm.rs:550-558): (m, n_traj) trajectories of the single expert
        (GaussianProcess.sample); a mixture of several clusters raises the reference's SampleError."""
        if self.gmx.n_clusters != 1:
            from ._lib import ERR_INVALID_VALUE, SampleError
            raise SampleError(ERR_INVALID_VALUE, f"Can not sample when several clusters {self.gmx.n_clusters}")
        if self.experts[0] is None:
            raise ValueError("the single expert lives on another rank")
        return self.experts[0].sample(x, n_traj)

    def predict_var(self, x):
        return self.predict_valvar(x, False, True)[1]

    def _predict_valvar_gradients_library(self, x, lib_handles, want_val, want_var):
        import ctypes as C
        from . import _lib as L
        lib = L.load()
        ids, hs, sparse = lib_handles
        m, d = x.shape
        k = len(self.experts)
        smooth = self.recombination == "smooth"
        dev = getattr(self.gmx, "predict_probas_device", None)
        probas = np.ascontiguousarray(self._probas(dev, x) if dev is not None else self.gmx.predict_probas(x), dtype=np.float64)
        dprobas = None
        if smooth and k > 1:
            ddev = getattr(self.gmx, "predict_probas_derivatives_device", None)
            dprobas = np.ascontiguousarray(self._probas(ddev, x) if ddev is not None else self.gmx.predict_probas_derivatives(x),
                                           dtype=np.float64)
        harr = (C.c_void_p * max(1, len(hs)))(*[h.value if hasattr(h, "value") else h for h in hs])
        iarr = np.asarray(ids, dtype=np.int32)
        gy = np.empty((m, d)) if want_val else None
        gv = np.empty((m, d)) if want_var else None
        entry = lib.egx_moe_predict_valvar_gradients_sgp if sparse else lib.egx_moe_predict_valvar_gradients
        L.check(entry(self.sweep._h if self.sweep is not None else None, harr,
                      iarr.ctypes.data_as(L.c_int32_p), len(hs), k, L.dptr(probas),
                      L.dptr(dprobas) if dprobas is not None else None, L.dptr(x), m, d,
                      1 if smooth else 0, L.dptr(gy) if want_val else None,
                      L.dptr(gv) if want_var else None))
        return (gy if want_val else np.zeros((m, d))), (gv if want_var else np.zeros((m, d)))

    def predict_valvar_gradients(self, x, want_val=True, want_var=True):
        """crates/moe/src/algorithm.rs:691-783 (smooth), :942-1010 (hard) -> ((m, nx), (m, nx)).
        smooth:  d mean = sum_i p_i grad y_i + p'_i y_i ;  d var = sum_i p_i^2 grad v_i + 2 p_i p'_i v_i.
        Every expert gets ONE batched call per quantity (the reference calls it once per row).  With GPU experts the
        recombination runs inside the library (egx_moe_predict_valvar_gradients, round 4); the numpy fold below serves
        duck-typed experts (the CPU tests)."""
        x = np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=np.float64)))
        m, nx = x.shape
        lib_handles = self._library_handles()
        if lib_handles is not None and m > 0:
            return self._predict_valvar_gradients_library(x, lib_handles, want_val, want_var)
        gy, gv = np.zeros((m, nx)), np.zeros((m, nx))
        smooth = self.recombination == "smooth"
        if smooth:
            p = self.gmx.predict_probas(x)
            pp = self.gmx.predict_probas_derivatives(x) if self.gmx.n_clusters > 1 else np.zeros((m, 1, nx))
        else:
            c = self.gmx.predict(x)
        for i, e in enumerate(self.experts):
            if not self._mine(i):
                continue
            idx = None if smooth else np.flatnonzero(c == i)
            if idx is not None and idx.size == 0:
                continue
            xi = x if smooth else x[idx]
            if want_val:
                g = e.predict_gradients(xi)
                if smooth:
                    gy += g * p[:, i:i + 1] + pp[:, i, :] * e.predict(xi)[:, None]
                else:
                    gy[idx] = g
            if want_var:
                g = e.predict_var_gradients(xi)
                if smooth:
                    gv += g * (p[:, i:i + 1] ** 2) + 2.0 * p[:, i:i + 1] * pp[:, i, :] * e.predict_var(xi)[:, None]
                else:
                    gv[idx] = g
        gy, gv = self._allreduce(gy, gv)
        return gy, gv

    def predict_gradients(self, x):
        return self.predict_valvar_gradients(x, True, False)[0]

    def predict_var_gradients(self, x):
        return self.predict_valvar_gradients(x, False, True)[1]
