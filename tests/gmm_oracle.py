"""Test oracle of the Gaussian-mixture training (egx_gmm_fit): a plain two-pass numpy EM, float64 throughout.

The formulation is scikit-learn's `GaussianMixture(covariance_type="full")` (tests/test_moe_train_cpu.py pins `em_iterations`
against it): nk = sum resp + 10 eps, weights = nk / sum nk, means = resp^T x / nk, cov_c = (resp_c diff)^T diff / nk_c + reg I
with diff = x - mean_c (the NEW mean: two passes), log p through precisions_chol, lower bound = mean log-prob-norm, stop when
|lb - lb_prev| < tol.  What the library adds around it is restated here as the issue of the feature sets it: iteration 0
assigns every row to its nearest initial mean (squared Euclidean distance, ties to the lowest index) and runs the M-step on
the one-hot responsibilities; a restart whose covariance is not positive definite, or whose numbers are not finite, has
failed (status 2) and is excluded; the best restart is the greatest final lower bound, the lowest index among equals.
"""
import numpy as np

EPS10 = 10.0 * np.finfo(np.float64).eps
CONVERGED, MAX_ITER, FAILED = 0, 1, 2


def nearest_mean_resp(x, means):
    d2 = ((x[:, None, :] - means[None, :, :]) ** 2).sum(axis=2)
    resp = np.zeros((x.shape[0], means.shape[0]))
    resp[np.arange(x.shape[0]), np.argmin(d2, axis=1)] = 1.0  # argmin: the first among equals
    return resp


def m_step(x, resp, reg_covar):
    nk = resp.sum(axis=0) + EPS10
    means = resp.T @ x / nk[:, None]
    k, d = means.shape
    covs = np.empty((k, d, d))
    for c in range(k):
        diff = x - means[c]
        covs[c] = (resp[:, c, None] * diff).T @ diff / nk[c]
        covs[c].flat[:: d + 1] += reg_covar
    return nk / nk.sum(), means, covs


def precisions_chol(covs):
    k, d, _ = covs.shape
    out = np.empty_like(covs)
    for c in range(k):
        low = np.linalg.cholesky(covs[c])  # LinAlgError when not positive definite
        out[c] = np.linalg.solve(low, np.eye(d)).T
    return out


def e_step(x, weights, means, pchol):
    n, d = x.shape
    k = means.shape[0]
    wlp = np.empty((n, k))
    for c in range(k):
        z = (x - means[c]) @ pchol[c]
        wlp[:, c] = -0.5 * (d * np.log(2.0 * np.pi) + (z * z).sum(axis=1)) + np.log(np.diag(pchol[c])).sum() + np.log(weights[c])
    m = wlp.max(axis=1)
    lpn = m + np.log(np.exp(wlp - m[:, None]).sum(axis=1))
    return lpn, np.exp(wlp - lpn[:, None])


def em_iterations(x, weights, means, covs, n_iter, reg_covar):
    """n_iter plain EM iterations from a given state; returns the state and every iteration's lower bound."""
    lbs = []
    for _ in range(n_iter):
        lpn, resp = e_step(x, weights, means, precisions_chol(covs))
        weights, means, covs = m_step(x, resp, reg_covar)
        lbs.append(lpn.mean())
    return weights, means, covs, lbs


def fit_run(x, init_means, max_iter=100, tol=1e-3, reg_covar=1e-6):
    """One restart.  Returns dict(weights, means, covariances, lower_bound, n_iter, status, trace)."""
    x = np.asarray(x, dtype=np.float64)
    out = dict(weights=None, means=None, covariances=None, lower_bound=np.nan, n_iter=0, status=MAX_ITER, trace=[])
    weights, means, covs = m_step(x, nearest_mean_resp(x, np.asarray(init_means, dtype=np.float64)), reg_covar)
    prev = -np.inf
    for it in range(0, max_iter + 1):
        try:
            pchol = precisions_chol(covs)
            if not (np.isfinite(pchol).all() and np.isfinite(means).all()):
                raise np.linalg.LinAlgError("not finite")
        except np.linalg.LinAlgError:
            out.update(status=FAILED, lower_bound=np.nan)
            return out
        out.update(weights=weights, means=means, covariances=covs)
        if it == max_iter:
            return out
        lpn, resp = e_step(x, weights, means, pchol)
        weights, means, covs = m_step(x, resp, reg_covar)
        lb = lpn.mean()
        out["n_iter"] = it + 1
        if not np.isfinite(lb):
            out.update(status=FAILED, lower_bound=np.nan)
            return out
        out["lower_bound"] = lb
        out["trace"].append(lb)
        if abs(lb - prev) < tol:
            try:
                precisions_chol(covs)
            except np.linalg.LinAlgError:
                out.update(status=FAILED, lower_bound=np.nan)
                return out
            out.update(weights=weights, means=means, covariances=covs, status=CONVERGED)
            return out
        prev = lb
    return out


def fit(x, init_means, max_iter=100, tol=1e-3, reg_covar=1e-6):
    """Every restart of init_means (R, k, D) and the index of the best one (None when all failed)."""
    runs = [fit_run(x, m, max_iter, tol, reg_covar) for m in init_means]
    best = None
    for r, run in enumerate(runs):
        if run["status"] != FAILED and (best is None or run["lower_bound"] > runs[best]["lower_bound"]):
            best = r
    return runs, best


def blobs(n, d, k, seed, separation=8.0, spread=1.0, offset=0.0):
    """k well-separated Gaussian blobs (centres `separation` * N(0, 1), anisotropic spreads), rows in random order."""
    rng = np.random.default_rng(seed)
    centres = separation * rng.standard_normal((k, d))
    scales = spread * (0.5 + rng.random((k, d)))
    label = np.arange(n) % k
    rng.shuffle(label)
    return centres[label] + scales[label] * rng.standard_normal((n, d)) + offset


def starts(x, n_runs, k, seed):
    rng = np.random.default_rng(seed)
    return np.stack([x[rng.choice(x.shape[0], size=k, replace=False)] for _ in range(n_runs)])
