// EGO infill criteria as arithmetic on the predictions of ONE point: the value and x-gradient of the objective the infill
// optimiser minimises, from (mean, variance) and their gradients of the objective model and of the constraint models.
// Plain C++17 behind a host / device macro (as philox.h): g++ compiles it for the CPU suite (tests/c_host/infill_math_test.cpp),
// k_infill_combine (kernels_infill.hip) uses the same text.  Paths are relative to the reference checkout (crates/ego/src).
//
//   norm_cdf, norm_pdf          utils/misc.rs:31-38
//   EI value / gradient         criteria/ei.rs:22-88     var < DBL_EPSILON -> 0 / 0;  s = k sqrt(var), a = (fmin - mu) / s,
//                                                        EI = s (a Phi(a) + phi(a)).  The reference's four gradient terms collapse
//                                                        to  k s' phi(a) - Phi(a) mu'  with s' = var' / (2 sqrt(var))  (its arg2 and
//                                                        arg4 cancel exactly because diff_y = k sigma a); that form is coded here
//   LogEI value / gradient      ei.rs:106-170, utils/logei_helper.rs   var < DBL_EPSILON -> -DBL_MAX (value and every component);
//                                                        log_ei_helper(u) + ln s, u = (fmin - mu) / s; sigma_weight ignored (as there)
//   WB2 / WB2S                  criteria/wb2.rs:21-49    scale_ic EI - mu  (WB2: scale_ic = 1)
//   probability of feasibility  utils/cstr_pof.rs        pof = Phi((tol - mu_c) / s_c), 0 when var_c < DBL_EPSILON; pofs (product),
//                                                        logpofs (sum of ln max(pof, DBL_EPSILON)), their gradients
//   the minimised objective     solver/solver_computations.rs:356-475   obj = -crit / scale; with constraint models obj * pofs
//                                                        (EI, WB2, WB2S) or obj - logpofs (LogEI); feasibility == 0 replaces obj by
//                                                        -1 (0 for LogEI) and its gradient by 0 (:410-416, 441-466)
//
//   constraint values           solver/solver_computations.rs:196-257   what the optimiser is handed as c(x) <= 0 when
//                                                        cstr_infill = false: mean_cstr = mu_c / scale_cstr, or the upper trust
//                                                        bound (mu_c + 3 sigma_c) / scale_cstr (CSTR_DOUBT = 3)
//
// Four places where the reference is NOT followed (each pinned by tests/test_infill_cpu.py):
//   1. log_ei_helper far in the tail.  The reference's erfcx(z) = exp(z^2) erfc(z) (logei_helper.rs:9-11) leaves double range near
//      u = -37.6 and its own asymptotic branch starts at u <= -1e6 only.  Here, for u <= kTailSwitch = -20 the asymptotic form is
//      used directly:  log_term = -2 ln|u| + log1p(-3/u^2 + 15/u^4 - 105/u^6 + ...)  (12 terms), never exp(z^2).
//   2. pof_grad with a non-zero tolerance.  cstr_pof.rs:42-43 differentiates (tol - mu) / s as -mu'/s + s' mu / s^2, the derivative
//      for tol = 0 only.  Here: -mu'/s - (tol - mu) s' / s^2.
//   3. sigma_weight in the gradient.  eval_grad_infill_obj (solver_computations.rs:387-391) passes None where the value got
//      Some(sigma_weight).  Here value and gradient use the same k.
//   4. sigma' of the upper trust bound.  upper_trust_bound_cstr (solver_computations.rs:224-257) takes var_grad[[0, 0]], the FIRST
//      coordinate's derivative of the variance, for every coordinate of its gradient (:242).  Here coordinate c uses d var / d x_c
//      (tests/c_host/infill_cstr_math_test.cpp; at d = 1 both agree).
//   (A consequence of the feasibility rule: without constraint models the reference's gradient ignores `feasibility` (:438-439)
//    while its value is the constant -1 / 0; here the gradient of that constant is 0 as well.)
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EGX_IM_HD __host__ __device__ inline
#else
#define EGX_IM_HD inline
#endif

namespace egx {
namespace infill {

enum Kind { kEI = 0, kLogEI = 1, kWB2 = 2, kWB2S = 3 };  // egx_infill_criterion

constexpr double kEps = 2.220446049250313e-16;     // f64::EPSILON
constexpr double kMax = 1.7976931348623157e308;    // f64::MAX (f64::MIN = -kMax)
constexpr double kInvSqrt2 = 0.7071067811865475;   // logei_helper.rs:4
constexpr double kSqrt2Pi = 2.5066282746310007;    // misc.rs:7
constexpr double kLog2PiOver2 = 0.9189385332046727;       // logei_helper.rs:5
constexpr double kLogPiOver2Over2 = 0.2257913526447274;   // logei_helper.rs:6
constexpr double kTailSwitch = -20.0;  // deviation 1: at and below, the asymptotic series (z = 14.1 there: far above the overflow)

struct Params {
    int kind;  // Kind
    double fmin, sigma_weight, scale_ic, scale;
    int feasibility;
};

EGX_IM_HD double norm_cdf(double x) { return 0.5 * erfc(-x / 1.4142135623730951); }
EGX_IM_HD double norm_pdf(double x) { return exp(-0.5 * x * x) / kSqrt2Pi; }

// exp(z^2) erfc(z): only used for 1/sqrt(2) <= z < 14.2 (-20 < u <= -1), where neither factor leaves double range
EGX_IM_HD double erfcx_mid(double z) { return exp(z * z) * erfc(z); }

EGX_IM_HD double log1mexp(double x) {  // logei_helper.rs:13-20
    return (x > -0.6931471805599453) ? log(-expm1(x)) : log1p(-exp(x));
}

// S(u) = sum_{j=1..12} (-1)^j (2j+1)!! / u^(2j)  and  dS/du: phi(u) + u Phi(u) = phi(u) / u^2 (1 + S(u)) for u -> -inf
EGX_IM_HD void tail_series(double u, double *s_out, double *ds_out) {
    const double q = 1.0 / (u * u);
    double term = 1.0, s = 0.0, ds = 0.0;
    for (int j = 1; j <= 12; j++) {
        term *= -(double)(2 * j + 1) * q;  // (-1)^j (2j+1)!! / u^(2j)
        s += term;
        ds += term * (double)(-2 * j);
    }
    *s_out = s;
    *ds_out = ds / u;
}

// log(phi(u) + u Phi(u)) on the whole line (logei_helper.rs:22-37 above kTailSwitch)
EGX_IM_HD double log_ei_helper(double u) {
    if (u > -1.0) return log(norm_pdf(u) + u * norm_cdf(u));
    const double log_phi_u = -0.5 * u * u - kLog2PiOver2;
    if (u > kTailSwitch) {
        const double w = log(erfcx_mid(-kInvSqrt2 * u) * fabs(u)) + kLogPiOver2Over2;
        return log_phi_u + log1mexp(w);
    }
    double s, ds;
    tail_series(u, &s, &ds);
    return log_phi_u + (-2.0 * log(fabs(u)) + log1p(s));
}

// its derivative Phi(u) / (phi(u) + u Phi(u)) (logei_helper.rs:39-75 above kTailSwitch)
EGX_IM_HD double d_log_ei_helper(double u) {
    if (u > -1.0) return norm_cdf(u) / exp(log_ei_helper(u));
    if (u > kTailSwitch) {
        const double z = -kInvSqrt2 * u;
        const double ex = erfcx_mid(z);
        const double ex_prime = 2.0 * z * ex - 2.0 / 1.7724538509055159;  // sqrt(pi)
        const double w = log(ex * fabs(u)) + kLogPiOver2Over2;
        const double w_prime = (ex_prime * -kInvSqrt2 / ex) + 1.0 / u;
        const double ew = exp(w);
        return -u + (-ew / (1.0 - ew)) * w_prime;
    }
    double s, ds;
    tail_series(u, &s, &ds);
    return -u + (-2.0 / u + ds / (1.0 + s));
}

EGX_IM_HD double ei_value(double mu, double var, double fmin, double k) {
    if (var < kEps) return 0.0;
    const double s = k * sqrt(var);
    const double a = (fmin - mu) / s;
    return s * (a * norm_cdf(a) + norm_pdf(a));
}
// one component: dmu, dvar are d mu / d x_c, d var / d x_c
EGX_IM_HD double ei_grad(double mu, double var, double dmu, double dvar, double fmin, double k) {
    if (var < kEps) return 0.0;
    const double sigma = sqrt(var);
    const double a = (fmin - mu) / (k * sigma);
    return k * (dvar / (2.0 * sigma)) * norm_pdf(a) - norm_cdf(a) * dmu;
}
EGX_IM_HD double logei_value(double mu, double var, double fmin) {
    if (var < kEps) return -kMax;
    const double sigma = sqrt(var);
    return log_ei_helper((fmin - mu) / sigma) + log(sigma);
}
EGX_IM_HD double logei_grad(double mu, double var, double dmu, double dvar, double fmin) {
    if (var < kEps) return -kMax;
    const double sigma = sqrt(var);
    const double diff = fmin - mu;
    const double sp = dvar / (2.0 * sigma);
    const double up = dmu / (-sigma) - diff * (sp / (sigma * sigma));
    return d_log_ei_helper(diff / sigma) * up + sp / sigma;
}

// the criterion (to be MAXIMISED) of `kind` and one component of its gradient
EGX_IM_HD double crit_value(const Params &p, double mu, double var) {
    switch (p.kind) {
        case kEI: return ei_value(mu, var, p.fmin, p.sigma_weight);
        case kLogEI: return logei_value(mu, var, p.fmin);
        case kWB2: return ei_value(mu, var, p.fmin, p.sigma_weight) - mu;
        default: return p.scale_ic * ei_value(mu, var, p.fmin, p.sigma_weight) - mu;
    }
}
EGX_IM_HD double crit_grad(const Params &p, double mu, double var, double dmu, double dvar) {
    switch (p.kind) {
        case kEI: return ei_grad(mu, var, dmu, dvar, p.fmin, p.sigma_weight);
        case kLogEI: return logei_grad(mu, var, dmu, dvar, p.fmin);
        case kWB2: return ei_grad(mu, var, dmu, dvar, p.fmin, p.sigma_weight) - dmu;
        default: return p.scale_ic * ei_grad(mu, var, dmu, dvar, p.fmin, p.sigma_weight) - dmu;
    }
}

EGX_IM_HD double pof(double mu, double var, double tol) {
    if (var < kEps) return 0.0;
    return norm_cdf((tol - mu) / sqrt(var));
}
EGX_IM_HD double pof_grad(double mu, double var, double dmu, double dvar, double tol) {  // deviation 2
    if (var < kEps) return 0.0;
    const double sigma = sqrt(var);
    const double arg = (tol - mu) / sigma;
    const double sp = dvar / (2.0 * sigma);
    return norm_pdf(arg) * (dmu / (-sigma) - (tol - mu) * sp / (sigma * sigma));
}

// Model j of a point sits at index j * stride (j = 0 the objective model, 1..k the constraint models) in mu / var, component c
// of its gradients at j * gstride + c in dmu / dvar; tol has k entries.
EGX_IM_HD double pofs(int k, const double *mu, const double *var, int64_t stride, const double *tol) {
    double acc = 1.0;
    for (int j = 1; j <= k; j++) acc *= pof(mu[j * stride], var[j * stride], tol[j - 1]);
    return acc;
}
EGX_IM_HD double logpofs(int k, const double *mu, const double *var, int64_t stride, const double *tol) {
    double acc = 0.0;
    for (int j = 1; j <= k; j++) acc += log(fmax(pof(mu[j * stride], var[j * stride], tol[j - 1]), kEps));
    return acc;
}

// the objective the infill optimiser MINIMISES (solver_computations.rs:356-422)
EGX_IM_HD double objective(const Params &p, int k, const double *mu, const double *var, int64_t stride, const double *tol) {
    const bool is_log = p.kind == kLogEI;
    double obj;
    if (p.feasibility)
        obj = -crit_value(p, mu[0], var[0]) / p.scale;
    else
        obj = is_log ? 0.0 : -1.0;
    if (k == 0) return obj;
    return is_log ? obj - logpofs(k, mu, var, stride, tol) : obj * pofs(k, mu, var, stride, tol);
}

// its gradient, d components written to grad[c * gout] (solver_computations.rs:378-393, 426-475 with deviations 2 and 3)
EGX_IM_HD void objective_grad(const Params &p, int k, int d, const double *mu, const double *var, int64_t stride,
                              const double *dmu, const double *dvar, int64_t gstride, const double *tol, double *grad,
                              int64_t gout) {
    const bool is_log = p.kind == kLogEI;
    if (k == 0) {
        for (int c = 0; c < d; c++)
            grad[c * gout] = p.feasibility ? -crit_grad(p, mu[0], var[0], dmu[c], dvar[c]) / p.scale : 0.0;
        return;
    }
    if (is_log) {
        for (int c = 0; c < d; c++) {
            double g = p.feasibility ? -crit_grad(p, mu[0], var[0], dmu[c], dvar[c]) / p.scale : 0.0;
            for (int j = 1; j <= k; j++) {  // logpofs_grad: sum of pof_grad / max(pof, eps)
                const double den = fmax(pof(mu[j * stride], var[j * stride], tol[j - 1]), kEps);
                g -= pof_grad(mu[j * stride], var[j * stride], dmu[j * gstride + c], dvar[j * gstride + c], tol[j - 1]) / den;
            }
            grad[c * gout] = g;
        }
        return;
    }
    const double infill = p.feasibility ? -crit_value(p, mu[0], var[0]) / p.scale : -1.0;
    const double pf = pofs(k, mu, var, stride, tol);
    for (int c = 0; c < d; c++) {
        const double ig = p.feasibility ? -crit_grad(p, mu[0], var[0], dmu[c], dvar[c]) / p.scale : 0.0;
        double pg = 0.0;  // pofs_grad: product rule
        for (int i = 1; i <= k; i++) {
            double others = 1.0;
            for (int j = 1; j <= k; j++)
                if (j != i) others *= pof(mu[j * stride], var[j * stride], tol[j - 1]);
            pg += pof_grad(mu[i * stride], var[i * stride], dmu[i * gstride + c], dvar[i * gstride + c], tol[i - 1]) * others;
        }
        grad[c * gout] = ig * pf + pg * infill;
    }
}

// How the constraint surrogates enter the optimisation (egx_cstr_strategy): kCstrInfill folds them into the objective (pofs /
// logpofs above); kCstrMean / kCstrUtb hand cstr_value to the optimiser as c(x) <= 0 and leave the objective without the factor.
enum CstrStrategy { kCstrInfill = 0, kCstrMean = 1, kCstrUtb = 2 };
constexpr double kCstrDoubt = 3.0;  // CSTR_DOUBT

EGX_IM_HD double cstr_value(int strategy, double mu, double var, double scale) {
    if (strategy == kCstrUtb) return (mu + kCstrDoubt * sqrt(var)) / scale;
    return mu / scale;
}
// one component: dmu, dvar are d mu_c / d x_c, d var_c / d x_c (deviation 4)
EGX_IM_HD double cstr_grad(int strategy, double var, double dmu, double dvar, double scale) {
    if (strategy != kCstrUtb) return dmu / scale;
    const double sigma = sqrt(var);
    const double sp = sigma < kEps ? 0.0 : dvar / (2.0 * sigma);
    return (dmu + kCstrDoubt * sp) / scale;
}

}  // namespace infill
}  // namespace egx
