// Conditioning a fitted universal-kriging model on q VIRTUAL observations in closed form (infill_pending.hip: the pending points of a
// q-point infill batch; crates/ego/src/solver/solver_impl.rs:622-791 refits instead).  With k(x, x') = r(x, x') - rt(x)^T rt(x')
// + u(x)^T u(x') the model's unit posterior covariance (algorithm.rs:330-369), X_v / y_v the virtual observations in the model's
// own normalisation,
//     S = k(X_v, X_v) + nugget I = L L^T,   delta = y~_v - mu~(X_v),   alpha = S^-1 delta,   c(x) = k(x, X_v),
// a refit at fixed theta with the normalisation frozen gives exactly
//     mean'(x)  = mean(x) + y_std c^T alpha
//     unit var' = s^2(x) - c^T S^-1 c = s^2(x) - |L^-1 c|^2
//     sigma2~'  = (n sigma2~ + delta^T S^-1 delta) / (n + q)             (the rho^T rho / n estimator of :1042)
//     var'(x)   = sigma2~' y_std^2 max(0, unit var')
// and the x-gradients follow through c(x).  The functions below are the FP64 arithmetic of that: the host borders L, alpha
// and sigma2' when a point is pushed; the finish kernel (kernels_pending.hip) and tests/c_host/pending_math_test.cpp call the
// per-point part.  Everything is __host__ __device__, fixed order, no allocation; LD is the row stride of L.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EGX_PM_HD __host__ __device__
#else
#define EGX_PM_HD
#endif

namespace egx {
namespace pending {

constexpr int kMaxPending = 16;  // EGX_INFILL_MAX_PENDING
constexpr int kLd = kMaxPending;

// Border the lower Cholesky factor L (q x q in a kLd-strided array) of S by one row: row q <- [L^-1 s_col ; sqrt(s_qq - |.|^2)],
// s_col[v] = S[q][v] (v < q), s_qq = S[q][q].  Returns false (L untouched beyond row q's scratch, which nobody reads) when the
// pivot is not positive and finite.
EGX_PM_HD inline bool chol_border(double *L, int q, const double *s_col, double s_qq) {
    double *row = L + q * kLd;
    double sq = 0.0;
    for (int i = 0; i < q; i++) {
        double acc = s_col[i];
        for (int j = 0; j < i; j++) acc -= L[i * kLd + j] * row[j];
        row[i] = acc / L[i * kLd + i];
        sq += row[i] * row[i];
    }
    const double piv = s_qq - sq;
    if (!(piv > 0.0) || !std::isfinite(piv)) return false;
    row[q] = std::sqrt(piv);
    for (int j = q + 1; j < kLd; j++) row[j] = 0.0;
    return true;
}

// z = L^-1 b (forward substitution), q <= kMaxPending; z may alias b
EGX_PM_HD inline void solve_lower(const double *L, int q, const double *b, double *z) {
    for (int i = 0; i < q; i++) {
        double acc = b[i];
        for (int j = 0; j < i; j++) acc -= L[i * kLd + j] * z[j];
        z[i] = acc / L[i * kLd + i];
    }
}

// x = L^-T z (back substitution); x may alias z
EGX_PM_HD inline void solve_lower_t(const double *L, int q, const double *z, double *x) {
    for (int i = q - 1; i >= 0; i--) {
        double acc = z[i];
        for (int j = i + 1; j < q; j++) acc -= L[j * kLd + i] * x[j];
        x[i] = acc / L[i * kLd + i];
    }
}

// alpha = S^-1 delta; returns delta^T S^-1 delta = |L^-1 delta|^2
EGX_PM_HD inline double solve_alpha(const double *L, int q, const double *delta, double *alpha) {
    double z[kMaxPending], quad = 0.0;
    solve_lower(L, q, delta, z);
    for (int i = 0; i < q; i++) quad += z[i] * z[i];
    solve_lower_t(L, q, z, alpha);
    return quad;
}

// the rho^T rho / n estimator after q virtual observations, in the units of sigma2 (raw: both carry y_std^2; quad is in
// normalised y units)
EGX_PM_HD inline double sigma2_conditioned(double sigma2, double y_std, int n, int q, double quad) {
    return ((double)n * sigma2 + y_std * y_std * quad) / (double)(n + q);
}

// What one point contributes, from its cross-covariances c (q): dm = c^T alpha, quad = c^T S^-1 c, and (want_b) b = S^-1 c,
// the weights of d c / d x in the variance gradient
EGX_PM_HD inline void point_terms(const double *L, const double *alpha, int q, const double *c, double *dm, double *quad, double *b) {
    double z[kMaxPending], m = 0.0, s = 0.0;
    solve_lower(L, q, c, z);
    for (int i = 0; i < q; i++) {
        m += c[i] * alpha[i];
        s += z[i] * z[i];
    }
    *dm = m;
    *quad = s;
    if (b) solve_lower_t(L, q, z, b);
}

// mean'(x) in raw units
EGX_PM_HD inline double cond_mean(double mean, double y_std, double dm) { return mean + y_std * dm; }

// var'(x) in raw units from the base model's CLAMPED raw variance (sigma2 s^2, 0 where s^2 < 0 -- and then 0 here as well)
EGX_PM_HD inline double cond_var(double var, double sigma2, double sigma2c, double quad) {
    const double unit = (sigma2 > 0.0 ? var / sigma2 : 0.0) - quad;
    return unit > 0.0 ? sigma2c * unit : 0.0;
}

// d mean' / d x_k (raw): gc = sum_v alpha_v d c_v / d x~_k in normalised coordinates
EGX_PM_HD inline double cond_gmean(double gmean, double y_std, double x_std, double gc) { return gmean + y_std * gc / x_std; }

// d var' / d x_k (raw): gb = sum_v b_v d c_v / d x~_k
EGX_PM_HD inline double cond_gvar(double gvar, double sigma2, double sigma2c, double x_std, double gb) {
    return (sigma2 > 0.0 ? gvar * (sigma2c / sigma2) : 0.0) - 2.0 * sigma2c * gb / x_std;
}

}  // namespace pending
}  // namespace egx
