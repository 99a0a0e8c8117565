"""Gradients of the sparse GP's likelihood (FITC / VFE) WITH KPLS weights w_star (d x h), in numpy by dense n x n algebra,
for n <= 300.  The counterpart of tests/sgp_grad_oracle.py / sgp_zgrad_oracle.py (which are w = I) with the correlations taken
from oracle/sgp_oracle.py's compute_k and their logarithmic derivatives worked out by hand from the reference's formulas
(crates/gp/src/correlation_models.rs, c_jl = theta_l |w_jl|, a = |x_j - z_j|):

    squared exponential   ln r = -1/2 sum_j (sum_l (theta_l w_jl)^2) a_j^2
    absolute exponential  ln r = -sum_j (sum_l c_jl) a_j
    Matern-3/2            ln r = sum_jl ln(1 + s t_jl) - s t_jl,                t_jl = c_jl a_j, s = sqrt 3
    Matern-5/2            ln r = sum_jl ln(1 + s t_jl + 5/3 t_jl^2) - s t_jl,   s = sqrt 5

    Sigma = Q + diag(nu) (FITC: nu_t = sigma2 - Q_tt + noise) or Q + nu I (VFE: nu = max(noise, nugget)),  Q = K_nm K_mm^-1 K_mn
    L     = -1/2 [ln|Sigma| + y' Sigma^-1 y (+ (n sigma2 - tr Q) / nu, VFE)]
    dL    = -1/2 tr(Sigma^-1 dSigma) + 1/2 alpha' dSigma alpha (- 1/2 d[(n sigma2 - tr Q) / nu]),   alpha = Sigma^-1 y

Every dSigma is a dQ plus a diagonal, and dQ = dK_nm B + B' dK_mn - B' dK_mm B with B = K_mm^-1 K_mn, so with
P = Sigma^-1 - alpha alpha' and P~ = P without its diagonal (FITC: the diagonal of Q cancels in Sigma) or P - I / nu (VFE: the
trace term) the traces contract to two weight matrices, T' = P~ B' (n x nz) and S = B P~ B' (nz x nz), against the elementwise
derivatives of K_nm and K_mm -- the same sums, in the same scaling (natural logarithm, no constant), as the w = I oracles."""
import math

import numpy as np
import scipy.linalg as sla

from oracle import sgp_oracle as S

KINDS = ["SquaredExponential", "AbsoluteExponential", "Matern32", "Matern52"]
FITC, VFE = "Fitc", "Vfe"


def _kind(kind):
    return KINDS[kind] if isinstance(kind, (int, np.integer)) else kind


def corr(kind, a, b, w, theta):
    """R (na x nb) from the reference's compute_k at sigma2 = 1."""
    return S.compute_k(_kind(kind), a, b, w, theta, 1.0)


def dlog_dtheta(kind, a, b, w, theta):
    """d ln R / d theta_l, (na, nb, h)."""
    kind = _kind(kind)
    ad = np.abs(a[:, None, :] - b[None, :, :])  # (na, nb, d)
    aw = np.abs(w)
    if kind == "SquaredExponential":
        return -np.einsum("abj,jl->abl", ad * ad, w * w) * theta
    if kind == "AbsoluteExponential":
        return -np.einsum("abj,jl->abl", ad, aw)
    t = ad[:, :, :, None] * (theta * aw)  # (na, nb, d, h)
    if kind == "Matern32":
        s = math.sqrt(3.0)
        f1 = s / (1.0 + s * t) - s
    else:
        s = math.sqrt(5.0)
        f1 = (s + 10.0 / 3.0 * t) / (1.0 + s * t + 5.0 / 3.0 * t * t) - s
    return np.einsum("abjl,abj,jl->abl", f1, ad, aw)


def phi(kind, a, b, w, theta):
    """d ln r(a_i, b_j) / d a_ik, (na, nb, d); np.sign(0) = 0."""
    kind = _kind(kind)
    dlt = a[:, None, :] - b[None, :, :]
    aw = np.abs(w)
    if kind == "SquaredExponential":
        return -dlt * ((theta * w) ** 2).sum(axis=1)
    if kind == "AbsoluteExponential":
        return -np.sign(dlt) * aw.dot(theta)
    c = theta * aw  # (d, h)
    t = np.abs(dlt)[:, :, :, None] * c
    if kind == "Matern32":
        s = math.sqrt(3.0)
        f1 = s / (1.0 + s * t) - s
    else:
        s = math.sqrt(5.0)
        f1 = (s + 10.0 / 3.0 * t) / (1.0 + s * t + 5.0 / 3.0 * t * t) - s
    return np.sign(dlt) * (f1 * c).sum(axis=3)


def zz_condition(kind, z, w, theta, sigma2, nugget):
    return float(np.linalg.cond(corr(kind, z, z, w, theta) + nugget / sigma2 * np.eye(z.shape[0])))


def _args(x, y, z, w, theta):
    x = np.asarray(x, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    w = np.asarray(w, dtype=np.float64)
    theta = np.broadcast_to(np.asarray(theta, dtype=np.float64).reshape(-1), (w.shape[1],)).copy()
    return x, y, z, w, theta


def _dense(kind, method, x, y, z, w, theta, sigma2, noise, nugget):
    """(T', S, R_nz, R_zz, diag P, tr Q, nu)."""
    n, nz = x.shape[0], z.shape[0]
    r_zz, r_nz = corr(kind, z, z, w, theta), corr(kind, x, z, w, theta)
    kmm = sigma2 * r_zz + nugget * np.eye(nz)
    bm = np.linalg.solve(kmm, sigma2 * r_nz.T)  # nz x n
    q = sigma2 * r_nz.dot(bm)
    q = 0.5 * (q + q.T)
    fitc = method in (FITC, 0)
    nu = None if fitc else max(noise, nugget)
    sig = q + (np.diag(sigma2 - np.diag(q) + noise) if fitc else nu * np.eye(n))
    cf = sla.cho_factor(sig, lower=True, check_finite=False)
    sinv = sla.cho_solve(cf, np.eye(n), check_finite=False)
    alpha = sinv.dot(y)
    p_full = sinv - np.outer(alpha, alpha)
    p_diag = np.diag(p_full).copy()
    pt = p_full - np.diag(p_diag) if fitc else p_full - np.eye(n) / nu
    tt = pt.dot(bm.T)
    return tt, bm.dot(tt), r_nz, r_zz, p_diag, float(np.trace(q)), nu


def likelihood_grad(kind, method, x, y, z, w, theta, sigma2, noise, nugget):
    """(h + 2,): dL/dtheta_0..h-1, dL/dsigma2, dL/dnoise."""
    x, y, z, w, theta = _args(x, y, z, w, theta)
    n, h = x.shape[0], w.shape[1]
    tt, ss, r_nz, r_zz, p_diag, trq, nu = _dense(kind, method, x, y, z, w, theta, sigma2, noise, nugget)
    fitc = method in (FITC, 0)
    grad = np.zeros(h + 2)
    grad[:h] = (-sigma2 * np.einsum("ab,abl->l", tt * r_nz, dlog_dtheta(kind, x, z, w, theta))
                + 0.5 * sigma2 * np.einsum("ab,abl->l", ss * r_zz, dlog_dtheta(kind, z, z, w, theta)))
    c_sigma = p_diag.sum() if fitc else n / nu
    grad[h] = -0.5 * (2.0 * (tt * r_nz).sum() - (ss * r_zz).sum() + c_sigma)
    if fitc:
        grad[h + 1] = -0.5 * p_diag.sum()
    elif noise > nugget:
        grad[h + 1] = -0.5 * (p_diag.sum() - (n * sigma2 - trq) / (nu * nu))
    return grad


def likelihood_grad_z(kind, method, x, y, z, w, theta, sigma2, noise, nugget):
    """(nz, d): dL/dz_jk = sigma2 sum_t T'[t, j] R(x_t, z_j) phi_k(x_t - z_j) + sigma2 sum_b S[j, b] R(z_j, z_b) phi_k(z_j - z_b)
    (the plus of the first sum: dR(x, z)/dz = -R phi(x - z) meets the -sigma2 of dL/dtheta; S is symmetric: twice 1/2)."""
    x, y, z, w, theta = _args(x, y, z, w, theta)
    tt, ss, r_nz, r_zz = _dense(kind, method, x, y, z, w, theta, sigma2, noise, nugget)[:4]
    return (sigma2 * np.einsum("tj,tjk->jk", tt * r_nz, phi(kind, x, z, w, theta))
            + sigma2 * np.einsum("jb,jbk->jk", ss * r_zz, phi(kind, z, z, w, theta)))


def likelihood(kind, method, x, y, z, w, theta, sigma2, noise, nugget):
    """oracle/sgp_oracle.py's likelihood."""
    x, y, z, w, theta = _args(x, y, z, w, theta)
    fn = S.fitc if method in (FITC, 0) else S.vfe
    return fn(_kind(kind), theta, sigma2, noise, w, x, y.reshape(-1, 1), z, nugget)[0]
