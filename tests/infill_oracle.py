"""numpy / math restatement of the reference's infill arithmetic (crates/ego/src, paths below relative to it), line by line
INCLUDING its own erfcx and pof_grad, and -- as separate, named functions -- the deviations of egobox_amd/csrc/infill_math.h.
Test infrastructure: imported by tests/test_infill_cpu.py, tests/test_gpu_infill.py and tools/infill_bench.py.

A point's predictions are `parts = (mu, var, dmu, dvar)`: mu, var of shape (1 + k,), dmu, dvar of shape (1 + k, d); model 0 is
the objective model, 1..k the constraint models."""
import math

import numpy as np

EPS = float(np.finfo(float).eps)
F64_MAX = float(np.finfo(float).max)
EI, LOG_EI, WB2, WB2S = 0, 1, 2, 3
SQRT_2PI = 2.5066282746310007          # utils/misc.rs:7
INV_SQRT_2 = 0.7071067811865475        # utils/logei_helper.rs:4
LOG_2PI_OVER_2 = 0.9189385332046727
LOG_PI_OVER_2_ALL_OVER_2 = 0.2257913526447274
INV_SQRT_EPSILON = 1.0 / 1e-6


def norm_cdf(x):  # misc.rs:31-33
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def norm_pdf(x):  # misc.rs:36-38
    return math.exp(-0.5 * x * x) / SQRT_2PI


# ---- utils/logei_helper.rs, line by line -------------------------------------------------------------------------------
def ref_erfcx(u):  # :9-11  (math.exp raises OverflowError where libm returns inf)
    return math.exp(u * u) * math.erfc(u)


def ref_log1mexp(x):  # :13-20
    if x > -math.log(2.0):
        return math.log(-math.expm1(x))
    return math.log1p(-math.exp(x))


def ref_log_ei_helper(u):  # :22-37
    if u > -1.0:
        return math.log(norm_pdf(u) + u * norm_cdf(u))
    log_phi_u = -0.5 * u * u - LOG_2PI_OVER_2
    if u > -INV_SQRT_EPSILON:
        w = math.log(ref_erfcx(-INV_SQRT_2 * u) * abs(u)) + LOG_PI_OVER_2_ALL_OVER_2
        log_term = ref_log1mexp(w)
    else:
        log_term = -2.0 * math.log(abs(u))
    return log_phi_u + log_term


def ref_d_log_ei_helper(u):  # :39-75
    if u > -1.0:
        return norm_cdf(u) / math.exp(ref_log_ei_helper(u))
    if u > -INV_SQRT_EPSILON:
        z = -INV_SQRT_2 * u
        val = ref_erfcx(z)
        erfcx_prime = 2.0 * z * val - 2.0 / math.sqrt(math.pi)
        w = math.log(val * abs(u)) + LOG_PI_OVER_2_ALL_OVER_2
        w_prime = (erfcx_prime * -INV_SQRT_2 / val) + 1.0 / u
        d_log_term = (-math.exp(w) / (1.0 - math.exp(w))) * w_prime
    else:
        d_log_term = -2.0 / u
    return -u + d_log_term


# ---- deviation 1: the asymptotic form from u <= -20 down ---------------------------------------------------------------
TAIL_SWITCH = -20.0


def _tail_series(u):
    q = 1.0 / (u * u)
    term, s, ds = 1.0, 0.0, 0.0
    for j in range(1, 13):
        term *= -(2 * j + 1) * q
        s += term
        ds += term * (-2 * j)
    return s, ds / u


def dev_log_ei_helper(u):
    if u > TAIL_SWITCH:
        return ref_log_ei_helper(u)
    s, _ = _tail_series(u)
    return -0.5 * u * u - LOG_2PI_OVER_2 + (-2.0 * math.log(abs(u)) + math.log1p(s))


def dev_d_log_ei_helper(u):
    if u > TAIL_SWITCH:
        return ref_d_log_ei_helper(u)
    s, ds = _tail_series(u)
    return -u + (-2.0 / u + ds / (1.0 + s))


# ---- criteria/ei.rs ----------------------------------------------------------------------------------------------------
def ei_value(mu, var, fmin, k=1.0):  # :22-47
    if var < EPS:
        return 0.0
    sigma = k * math.sqrt(var)
    a = (fmin - mu) / sigma
    return sigma * (a * norm_cdf(a) + norm_pdf(a))


def ei_grad(mu, var, dmu, dvar, fmin, k=1.0):  # :51-88, the four terms as written
    dmu, dvar = np.asarray(dmu, float), np.asarray(dvar, float)
    if var < EPS:
        return np.zeros_like(dmu)
    diff_y = fmin - mu
    sigma = math.sqrt(var)
    arg = diff_y / (k * sigma)
    sig_prime = k * dvar / (2.0 * sigma)
    arg_prime = dmu / (-k * sigma) - diff_y * (sig_prime / (k * sigma * k * sigma))
    factor = k * sigma * (-arg / SQRT_2PI) * math.exp(-(arg * arg) / 2.0)
    return dmu * (-norm_cdf(arg)) + diff_y * norm_pdf(arg) * arg_prime + sig_prime * norm_pdf(arg) + factor * arg_prime


def logei_value(mu, var, fmin, helper=ref_log_ei_helper):  # :106-129
    if var < EPS:
        return -F64_MAX
    sigma = math.sqrt(var)
    return helper((fmin - mu) / sigma) + math.log(sigma)


def logei_grad(mu, var, dmu, dvar, fmin, dhelper=ref_d_log_ei_helper):  # :133-170
    dmu, dvar = np.asarray(dmu, float), np.asarray(dvar, float)
    if var < EPS:
        return np.full_like(dmu, -F64_MAX)
    diff_y = fmin - mu
    sigma = math.sqrt(var)
    sig_prime = dvar / (2.0 * sigma)
    arg_prime = dmu / (-sigma) - diff_y * (sig_prime / (sigma * sigma))
    return dhelper(diff_y / sigma) * arg_prime + sig_prime / sigma


def crit_value(kind, mu, var, fmin, k, scale_ic, dev=False):
    if kind == EI:
        return ei_value(mu, var, fmin, k)
    if kind == LOG_EI:
        return logei_value(mu, var, fmin, dev_log_ei_helper if dev else ref_log_ei_helper)
    sc = 1.0 if kind == WB2 else scale_ic  # criteria/wb2.rs:21-33
    return sc * ei_value(mu, var, fmin, k) - mu


def crit_grad(kind, mu, var, dmu, dvar, fmin, k, scale_ic, dev=False):
    if kind == EI:
        return ei_grad(mu, var, dmu, dvar, fmin, k)
    if kind == LOG_EI:
        return logei_grad(mu, var, dmu, dvar, fmin, dev_d_log_ei_helper if dev else ref_d_log_ei_helper)
    sc = 1.0 if kind == WB2 else scale_ic  # wb2.rs:37-49
    return sc * ei_grad(mu, var, dmu, dvar, fmin, k) - np.asarray(dmu, float)


# ---- utils/cstr_pof.rs -------------------------------------------------------------------------------------------------
def pof(mu, var, tol):  # :9-24
    if var < EPS:
        return 0.0
    return norm_cdf((tol - mu) / math.sqrt(var))


def ref_pof_grad(mu, var, dmu, dvar, tol):  # :28-49, as written (the derivative for tol = 0 only)
    dmu, dvar = np.asarray(dmu, float), np.asarray(dvar, float)
    if var < EPS:
        return np.zeros_like(dmu)
    sigma = math.sqrt(var)
    arg = (tol - mu) / sigma
    sig_prime = dvar / (2.0 * sigma)
    arg_prime = dmu / (-sigma) + sig_prime * mu / (sigma * sigma)
    return norm_pdf(arg) * arg_prime


def dev_pof_grad(mu, var, dmu, dvar, tol):  # deviation 2
    dmu, dvar = np.asarray(dmu, float), np.asarray(dvar, float)
    if var < EPS:
        return np.zeros_like(dmu)
    sigma = math.sqrt(var)
    arg = (tol - mu) / sigma
    sig_prime = dvar / (2.0 * sigma)
    return norm_pdf(arg) * (dmu / (-sigma) - (tol - mu) * sig_prime / (sigma * sigma))


def pofs(mu, var, tols):  # :51-60
    acc = 1.0
    for j, t in enumerate(tols):
        acc *= pof(mu[1 + j], var[1 + j], t)
    return acc


def logpofs(mu, var, tols):  # :62-71
    acc = 0.0
    for j, t in enumerate(tols):
        acc += math.log(max(pof(mu[1 + j], var[1 + j], t), EPS))
    return acc


def pofs_grad(parts, tols, pof_grad=ref_pof_grad):  # :73-101
    mu, var, dmu, dvar = parts
    vals = [pof(mu[1 + j], var[1 + j], t) for j, t in enumerate(tols)]
    acc = np.zeros(np.asarray(dmu).shape[1])
    for i, t in enumerate(tols):
        others = 1.0
        for j, v in enumerate(vals):
            if j != i:
                others *= v
        acc = acc + pof_grad(mu[1 + i], var[1 + i], dmu[1 + i], dvar[1 + i], t) * others
    return acc


def logpofs_grad(parts, tols, pof_grad=ref_pof_grad):  # :103-125
    mu, var, dmu, dvar = parts
    acc = np.zeros(np.asarray(dmu).shape[1])
    for j, t in enumerate(tols):
        acc = acc + pof_grad(mu[1 + j], var[1 + j], dmu[1 + j], dvar[1 + j], t) / max(pof(mu[1 + j], var[1 + j], t), EPS)
    return acc


# ---- solver/solver_computations.rs:356-475 -----------------------------------------------------------------------------
def objective(kind, mu, var, tols, fmin, sigma_weight, scale_ic, scale, feasibility, dev=False):
    """eval_infill_obj_with_cstrs (:398-422); without constraint models pofs = 1 / logpofs = 0."""
    if feasibility:
        obj = -crit_value(kind, mu[0], var[0], fmin, sigma_weight, scale_ic, dev) / scale
    else:
        obj = 0.0 if kind == LOG_EI else -1.0
    if len(tols) == 0:
        return obj
    return obj - logpofs(mu, var, tols) if kind == LOG_EI else obj * pofs(mu, var, tols)


def ref_objective_grad(kind, parts, tols, fmin, sigma_weight, scale_ic, scale, feasibility):
    """eval_grad_infill_obj_with_cstrs (:426-475) as written: sigma_weight is NOT passed on (:387-391), pof_grad is the
    reference's, and without constraint models `feasibility` is ignored (:438-439)."""
    mu, var, dmu, dvar = parts
    g0 = -crit_grad(kind, mu[0], var[0], dmu[0], dvar[0], fmin, 1.0, scale_ic) / scale
    if len(tols) == 0:
        return g0
    if kind == LOG_EI:
        infill_grad = g0 if feasibility else np.zeros_like(g0)
        return infill_grad - logpofs_grad(parts, tols, ref_pof_grad)
    if feasibility:
        infill = -crit_value(kind, mu[0], var[0], fmin, sigma_weight, scale_ic) / scale
        infill_grad = g0
    else:
        infill, infill_grad = -1.0, np.zeros_like(g0)
    return infill_grad * pofs(mu, var, tols) + pofs_grad(parts, tols, ref_pof_grad) * infill


def dev_objective_grad(kind, parts, tols, fmin, sigma_weight, scale_ic, scale, feasibility):
    """The gradient infill_math.h computes: the same k in value and gradient (deviation 3), the corrected pof_grad (deviation 2),
    the tail of the LogEI helper (deviation 1), and the gradient of the constant that replaces an infeasible objective is 0
    with and without constraint models."""
    mu, var, dmu, dvar = parts
    if feasibility:
        g0 = -crit_grad(kind, mu[0], var[0], dmu[0], dvar[0], fmin, sigma_weight, scale_ic, dev=True) / scale
    else:
        g0 = np.zeros(np.asarray(dmu).shape[1])
    if len(tols) == 0:
        return g0
    if kind == LOG_EI:
        return g0 - logpofs_grad(parts, tols, dev_pof_grad)
    infill = -crit_value(kind, mu[0], var[0], fmin, sigma_weight, scale_ic) / scale if feasibility else -1.0
    return g0 * pofs(mu, var, tols) + pofs_grad(parts, tols, dev_pof_grad) * infill


# ---- compute_scaling (:132-193) fed with per-point predictions ---------------------------------------------------------
def compute_scaling(kind, mu, var, tols, fmin, sigma_weight):
    """mu, var: (1 + k, npts) predictions at the scaling points.  Returns (scale_ic, scale, scale_cstr)."""
    mu, var = np.asarray(mu, float), np.asarray(var, float)
    npts = mu.shape[1]
    scale_ic = 1.0
    if kind == WB2S:  # criteria/wb2.rs:67-88
        ei = np.array([ei_value(mu[0, i], var[0, i], fmin, sigma_weight) for i in range(npts)])
        i_max = int(np.argmax(ei))
        if abs(ei[i_max]) > 100.0 * EPS:
            scale_ic = 100.0 * abs(mu[0, i_max]) / ei[i_max]
    vals = np.empty(npts)  # :297-351
    for i in range(npts):
        v = -crit_value(kind, mu[0, i], var[0, i], fmin, sigma_weight, scale_ic, dev=True) / 1.0
        if math.isnan(v) or math.isinf(v):
            v = 1.0
        if len(tols):
            if kind == LOG_EI:
                v -= logpofs(mu[:, i], var[:, i], tols)
            else:
                v *= pofs(mu[:, i], var[:, i], tols)
        vals[i] = v
    scale = float(np.max(np.abs(vals))) if npts else 1.0
    if scale < 100.0 * EPS:
        scale = 1.0
    scale_cstr = []  # utils/misc.rs:10-28
    for j in range(len(tols)):
        p = np.abs(mu[1 + j][~np.isinf(mu[1 + j])])
        scale_cstr.append(float(p.max()) if p.size else 1.0)
    return scale_ic, scale, np.array(scale_cstr)
