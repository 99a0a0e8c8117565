"""Closed-form gradient of the sparse GP's likelihood (FITC / VFE) in numpy, by DENSE n x n algebra -- a route that
shares nothing with the library's Woodbury form.

With K_mm = sigma2 R_zz + nugget I, K_nm = sigma2 R_nz, B = K_mm^-1 K_mn (nz x n), Q = K_nm B and
    FITC  Sigma = Q + diag(nu),  nu_t = sigma2 - Q_tt + noise          L = -1/2 [ln|Sigma| + y' Sigma^-1 y]
    VFE   Sigma = Q + nu I,      nu = max(noise, nugget), beta = 1/nu  L = -1/2 [ln|Sigma| + y' Sigma^-1 y + beta (n sigma2 - tr Q)]
let alpha = Sigma^-1 y, P = Sigma^-1 - alpha alpha', and P~ = P with its diagonal removed (FITC: the diagonal of Q cancels
in Sigma) or P - beta I (VFE: the trace term).  Then dL = -1/2 [tr(P~ dQ) + ...] and dQ = dK_nm B + B' dK_mn - B' dK_mm B give
    T' = P~ B' (n x nz),   S = B P~ B' (nz x nz),   p_t = P_tt
    dL/dtheta_k = -sigma2 sum T' o d_k R_nz + 1/2 sigma2 sum S o d_k R_zz
    dL/dsigma2  = -1/2 [2 sum T' o R_nz - sum S o R_zz + c_sigma],  c_sigma = sum p (FITC), n beta (VFE)
    dL/dnoise   = -1/2 c_nu,  c_nu = sum p (FITC);  VFE: sum p - beta^2 (n sigma2 - tr Q) if noise > nugget, else exactly 0
The likelihood is oracle/sgp_oracle.py's (natural logarithm, no constant)."""
import math

import numpy as np
import scipy.linalg as sla

KINDS = ["SquaredExponential", "AbsoluteExponential", "Matern32", "Matern52"]
FITC, VFE = "Fitc", "Vfe"


def corr(kind, a, b, theta):
    """R (na x nb) of the kernel `kind` (a name or its index) with w = I, unit diagonal, no nugget."""
    kind = KINDS[kind] if isinstance(kind, (int, np.integer)) else kind
    ad = np.abs(a[:, None, :] - b[None, :, :])
    t = ad * theta
    if kind == "SquaredExponential":
        return np.exp(-0.5 * (t * t).sum(axis=2))
    if kind == "AbsoluteExponential":
        return np.exp(-t.sum(axis=2))
    if kind == "Matern32":
        s = math.sqrt(3.0)
        return np.prod(1.0 + s * t, axis=2) * np.exp(-s * t.sum(axis=2))
    if kind == "Matern52":
        s = math.sqrt(5.0)
        return np.prod(1.0 + s * t + 5.0 / 3.0 * t * t, axis=2) * np.exp(-s * t.sum(axis=2))
    raise ValueError(kind)


def dlog_corr(kind, a, b, theta, k):
    """d ln R / d theta_k (na x nb)."""
    kind = KINDS[kind] if isinstance(kind, (int, np.integer)) else kind
    ad = np.abs(a[:, None, k] - b[None, :, k])
    t = theta[k] * ad
    if kind == "SquaredExponential":
        return -theta[k] * ad * ad
    if kind == "AbsoluteExponential":
        return -ad
    if kind == "Matern32":
        return -3.0 * ad * t / (1.0 + math.sqrt(3.0) * t)
    s = math.sqrt(5.0)
    return -(5.0 / 3.0) * ad * t * (1.0 + s * t) / (1.0 + s * t + 5.0 / 3.0 * t * t)


def zz_condition(kind, z, theta, sigma2, nugget):
    """cond(R_zz + nugget / sigma2 I): what the closed form's error scales with."""
    return float(np.linalg.cond(corr(kind, z, z, np.asarray(theta, dtype=np.float64)) + nugget / sigma2 * np.eye(z.shape[0])))


def likelihood_grad(kind, method, x, y, z, theta, sigma2, noise, nugget):
    """(d + 2,): dL/dtheta_0..d-1, dL/dsigma2, dL/dnoise."""
    x = np.asarray(x, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, d = x.shape
    nz = z.shape[0]
    theta = np.broadcast_to(np.asarray(theta, dtype=np.float64).reshape(-1), (d,)).copy()
    r_zz = corr(kind, z, z, theta)
    r_nz = corr(kind, x, z, theta)
    kmm = sigma2 * r_zz + nugget * np.eye(nz)
    bm = np.linalg.solve(kmm, sigma2 * r_nz.T)  # nz x n
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
    p_diag = np.diag(p_full).copy()
    if fitc:
        pt = p_full - np.diag(p_diag)
    else:
        pt = p_full - np.eye(n) / nu
    tt = pt.dot(bm.T)  # n x nz
    ss = bm.dot(tt)    # nz x nz
    grad = np.zeros(d + 2)
    for k in range(d):
        grad[k] = (-sigma2 * (tt * r_nz * dlog_corr(kind, x, z, theta, k)).sum()
                   + 0.5 * sigma2 * (ss * r_zz * dlog_corr(kind, z, z, theta, k)).sum())
    c_sigma = p_diag.sum() if fitc else n / nu
    grad[d] = -0.5 * (2.0 * (tt * r_nz).sum() - (ss * r_zz).sum() + c_sigma)
    if fitc:
        grad[d + 1] = -0.5 * p_diag.sum()
    elif noise > nugget:
        grad[d + 1] = -0.5 * (p_diag.sum() - (n * sigma2 - np.trace(q)) / (nu * nu))
    else:
        grad[d + 1] = 0.0
    return grad
