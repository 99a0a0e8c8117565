"""Helper of the pending-point tests (not a test): what a fitted GP becomes when q virtual observations are appended and it is
refitted at its theta with its normalisation frozen -- once by actually refitting with oracle.gp_oracle (`refit_frozen`), once by
the closed form of egobox_amd/csrc/pending_math.h in numpy (`closed_form`).  `g` is a GaussianProcessOracle."""
import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as O


def _norm(g, xv, yv):
    xv = np.atleast_2d(np.asarray(xv, dtype=np.float64))
    yv = np.asarray(yv, dtype=np.float64).reshape(-1, 1)
    return (xv - g.x_mean) / g.x_std, (yv - g.y_mean) / g.y_std


def refit_frozen(g, xv, yv):
    """The oracle on the n + q points: g's x_mean / x_std / y_mean / y_std / theta / w_star, a new factorisation."""
    xn, yn = _norm(g, xv, yv)
    xa, ya = np.vstack([g.xt_norm, xn]), np.vstack([g.yt_norm, yn])
    r_mx = O.corr_matrix_dense(g.corr, xa, g.theta, g.w_star, g.nugget)
    fx = O.regression_value(g.mean, xa)
    lkh, inner = O.reduced_likelihood_from_r(fx, r_mx, ya, g.y_std[0])
    return O.GaussianProcessOracle(theta=g.theta, likelihood=lkh, inner=inner, w_star=g.w_star, xt_norm=xa, x_mean=g.x_mean,
                                   x_std=g.x_std, yt_norm=ya, y_mean=g.y_mean, y_std=g.y_std, mean=g.mean, corr=g.corr,
                                   nugget=g.nugget)


def _rt_u(g, xn):
    return g._compute_rt_u(xn, g._compute_correlation(xn))


def unit_cov(g, xa, xb):
    """k(xa, xb) = r(xa, xb) - rt(xa)^T rt(xb) + u(xa)^T u(xb) on normalised points (algorithm.rs:330-369), (ma, mb)"""
    rta, ua = _rt_u(g, xa)
    rtb, ub = _rt_u(g, xb)
    dx = O.pairwise_differences(xa, xb)
    r = O.corr_value(g.corr, dx, g.theta, g.w_star).reshape(xa.shape[0], xb.shape[0])
    return r - rta.T.dot(rtb) + ua.T.dot(ub)


def _system(g, xv, yv):
    xn, yn = _norm(g, xv, yv)
    s = unit_cov(g, xn, xn)
    s[np.diag_indices_from(s)] += g.nugget
    mu_n = (g.predict(np.atleast_2d(xv)).reshape(-1, 1) - g.y_mean) / g.y_std
    return xn, s, (yn - mu_n)[:, 0]


def closed_form(g, xv, yv, xq):
    """(mean', var', sigma2', unit var') at the raw queries xq of g conditioned on (xv, yv), without a refit"""
    xn, s, delta = _system(g, xv, yv)
    chol = sla.cholesky(s, lower=True)
    alpha = sla.cho_solve((chol, True), delta)
    xqn = (np.atleast_2d(xq) - g.x_mean) / g.x_std
    c = unit_cov(g, xqn, xn)
    z = sla.solve_triangular(chol, c.T, lower=True)
    rt, u = _rt_u(g, xqn)
    unit = 1.0 - (rt * rt).sum(axis=0) + (u * u).sum(axis=0) - (z * z).sum(axis=0)
    n, q = g.xt_norm.shape[0], xn.shape[0]
    ys2 = float(g.y_std[0]) ** 2
    sigma2 = (n * g.inner.sigma2 / ys2 + delta.dot(alpha)) / (n + q) * ys2
    mean = g.predict(np.atleast_2d(xq)) + float(g.y_std[0]) * c.dot(alpha)
    return mean, sigma2 * np.maximum(unit, 0.0), sigma2, unit


def cond_report(g, xv, xq):
    """(min diag S, the smallest conditioned unit variance over xq): what decides whether s^2 - c^T S^-1 c keeps its digits"""
    xn, s, _ = _system(g, xv, np.zeros(np.atleast_2d(xv).shape[0]))
    unit = closed_form(g, xv, np.zeros(xn.shape[0]), xq)[3]
    return float(np.min(np.diag(s))), float(np.min(unit))
