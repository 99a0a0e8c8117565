"""Gradient of the sparse GP's likelihood (FITC / VFE) with respect to the inducing points, in numpy by the DENSE n x n algebra
of tests/sgp_grad_oracle.py (its notation: T' = P~ B', S = B P~ B'), DESIGN.md 4.6.1:

    dL/dz[j, k] = sigma2 sum_t T'[t, j] R(x_t, z_j) phi_k(x_tk - z_jk) + sigma2 sum_b S[j, b] R(z_j, z_b) phi_k(z_jk - z_bk)

with phi_k(dlt) = d ln r(a, b) / d a_k at dlt = a_k - b_k, t = theta_k |dlt|:
    squared exponential   -theta_k^2 dlt
    absolute exponential  -theta_k sgn(dlt)                                                      sgn(0) = 0
    Matern-3/2            sgn(dlt) theta_k (sqrt3 / (1 + sqrt3 t) - sqrt3)
    Matern-5/2            sgn(dlt) theta_k ((sqrt5 + 10/3 t) / (1 + sqrt5 t + 5/3 t^2) - sqrt5)
The first sum carries a plus sign because dR(x, z)/dz = -R phi(x - z) meets the -sigma2 of dL/dtheta; the second has the
factor 1 because S is symmetric: row j and column j give twice 1/2."""
import math

import numpy as np
import scipy.linalg as sla

from sgp_grad_oracle import FITC, KINDS, corr


def phi(kind, a, b, theta, k):
    """d ln r(a_i, b_j) / d a_ik (na x nb); np.sign(0) = 0."""
    kind = KINDS[kind] if isinstance(kind, (int, np.integer)) else kind
    dlt = a[:, None, k] - b[None, :, k]
    sg, t = np.sign(dlt), theta[k] * np.abs(dlt)
    if kind == "SquaredExponential":
        return -theta[k] ** 2 * dlt
    if kind == "AbsoluteExponential":
        return -theta[k] * sg
    if kind == "Matern32":
        s = math.sqrt(3.0)
        return sg * theta[k] * (s / (1.0 + s * t) - s)
    s = math.sqrt(5.0)
    return sg * theta[k] * ((s + 10.0 / 3.0 * t) / (1.0 + s * t + 5.0 / 3.0 * t * t) - s)


def pair_weights(kind, method, x, y, z, theta, sigma2, noise, nugget):
    """(T' (n x nz), S (nz x nz), R_nz, R_zz): the dense route of sgp_grad_oracle.likelihood_grad."""
    n, nz = x.shape[0], z.shape[0]
    r_zz = corr(kind, z, z, theta)
    r_nz = corr(kind, x, z, theta)
    kmm = sigma2 * r_zz + nugget * np.eye(nz)
    bm = np.linalg.solve(kmm, sigma2 * r_nz.T)
    q = sigma2 * r_nz.dot(bm)
    q = 0.5 * (q + q.T)
    fitc = method in (FITC, 0)
    if fitc:
        sig = q + np.diag(sigma2 - np.diag(q) + noise)
    else:
        nu = max(noise, nugget)
        sig = q + nu * np.eye(n)
    cf = sla.cho_factor(sig, lower=True, check_finite=False)
    sinv = sla.cho_solve(cf, np.eye(n), check_finite=False)
    alpha = sinv.dot(y)
    p_full = sinv - np.outer(alpha, alpha)
    pt = p_full - np.diag(np.diag(p_full)) if fitc else p_full - np.eye(n) / nu
    tt = pt.dot(bm.T)
    ss = bm.dot(tt)
    return tt, ss, r_nz, r_zz


def likelihood_grad_z(kind, method, x, y, z, theta, sigma2, noise, nugget, parts=False):
    """(nz, d): dL/dz.  parts=True: the two sums separately."""
    x = np.asarray(x, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    d = x.shape[1]
    theta = np.broadcast_to(np.asarray(theta, dtype=np.float64).reshape(-1), (d,)).copy()
    tt, ss, r_nz, r_zz = pair_weights(kind, method, x, y, z, theta, sigma2, noise, nugget)
    g_nz, g_zz = np.zeros(z.shape), np.zeros(z.shape)
    for k in range(d):
        g_nz[:, k] = sigma2 * (tt * r_nz * phi(kind, x, z, theta, k)).sum(axis=0)
        g_zz[:, k] = sigma2 * (ss * r_zz * phi(kind, z, z, theta, k)).sum(axis=1)
    return (g_nz, g_zz) if parts else g_nz + g_zz
