"""Helper of the theta-gradient tests (not a test): the closed form of dL/dtheta for ANY weights w_star, trend and kernel, in
numpy/scipy on top of oracle.gp_oracle.fit_fixed.  oracle.gp_oracle.likelihood_grad is the case w = I of it
(tests/test_theta_grad_oracle_cpu.py holds the two together at 1e-12, and this one against differences of the likelihood).

    dL/dtheta_l = (1 / ln 10) [ gamma^T (R o D_l) gamma / sigma2_n - tr(R^-1 (R o D_l)) ],     D_l = d log r / d theta_l

with R = C C^T from the oracle's own factor (nugget on the diagonal; the diagonal of R o D_l is zero: r_ii does not depend on
theta), sigma2_n = sigma2 / y_std^2, and, from oracle.gp_oracle.corr_value with a_j = |x_ij - x_kj| on the normalised inputs
and t = theta_l |w_jl| a_j,

    sq-exp      log r = -1/2 sum_j (sum_l theta_l^2 w_jl^2) a_j^2        D_l = -theta_l sum_j w_jl^2 a_j^2
    abs-exp     log r = -sum_j (sum_l theta_l |w_jl|) a_j                D_l = -sum_j |w_jl| a_j
    Matern-3/2  log r = sum_jl log(1 + s3 t) - s3 t                      D_l = sum_j |w_jl| a_j (s3 / (1 + s3 t) - s3)
    Matern-5/2  log r = sum_jl log(1 + s5 t + 5/3 t^2) - s5 t            D_l = sum_j |w_jl| a_j ((s5 + 10/3 t) / (1 + s5 t + 5/3 t^2) - s5)

None of them divides by theta or by a weight: theta_l = 0 and zero entries of w_star need no special case."""
import math

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as GO

S3, S5 = math.sqrt(3.0), math.sqrt(5.0)


def dlog_dtheta(corr, a, theta, w, l):
    """D_l of the pairs whose component distances are a (..., d), theta (h), w (d, h): an array of a's leading shape."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    nz = np.flatnonzero(w[:, l])  # (a zero weight's term is exactly 0)
    wa = np.abs(w[nz, l])
    wa_a = a[..., nz] * wa
    if corr == GO.SQEXP:
        return -theta[l] * (wa_a * wa_a).sum(axis=-1)
    if corr == GO.ABSEXP:
        return -wa_a.sum(axis=-1)
    t = theta[l] * wa_a
    if corr == GO.MATERN32:
        return (wa_a * (S3 / (1.0 + S3 * t) - S3)).sum(axis=-1)
    if corr == GO.MATERN52:
        return (wa_a * ((S5 + (10.0 / 3.0) * t) / (1.0 + S5 * t + (5.0 / 3.0) * t * t) - S5)).sum(axis=-1)
    raise ValueError(corr)


def likelihood_grad(x, y, theta, mean=GO.CONSTANT, corr=GO.SQEXP, w_star=None, nugget=GO.DEFAULT_NUGGET):
    """(likelihood, dL/dtheta (h), the smallest pivot of the factor of R) at theta (length 1 or h)."""
    gp = GO.fit_fixed(x, y, theta, mean, corr, nugget, w_star=w_star, dense=False)
    xn, w = gp.xt_norm, gp.w_star
    n = xn.shape[0]
    theta = GO.expand_theta(theta, w.shape[1])
    c = gp.inner.r_chol
    r_mx = c.dot(c.T)
    cinv, info = sla.lapack.dtrtri(c, lower=1, overwrite_c=0)
    if info != 0:
        raise np.linalg.LinAlgError(f"dtrtri info {info}")
    rinv = cinv.T.dot(cinv)
    gamma = gp.inner.gamma[:, 0]
    sigma2n = gp.inner.sigma2 / (gp.y_std[0] ** 2)
    a = np.abs(xn[:, None, :] - xn[None, :, :])
    grad = np.zeros(theta.size)
    for l in range(theta.size):
        dr = r_mx * dlog_dtheta(corr, a, theta, w, l)
        dr[np.arange(n), np.arange(n)] = 0.0
        grad[l] = (gamma.dot(dr).dot(gamma) / sigma2n - np.sum(rinv * dr)) / math.log(10.0)
    return gp.likelihood, grad, float(np.diag(c).min())
