// Recombination of a mixture of experts at ONE point (crates/moe/src/algorithm.rs): from the responsibilities p_e, their
// x-derivatives p'_e and every expert's (mean, variance, grad mean, grad variance) to the four quantities of the mixture.
// Plain C++17 behind a host / device macro (as infill_math.h): g++ compiles it for the CPU suite
// (tests/c_host/infill_mix_math_test.cpp), k_infill_mix (kernels_infill.hip) runs the same text, and the host fold of
// egx_moe_predict_valvar(_gradients) (moe_fold.h) takes its mean and gradient terms from here.
//
//   smooth  (:411-423, 670-685, 691-783), the experts in index order:
//       mean = sum p_e mu_e                     var = sum p_e^2 v_e
//       grad mean = sum (p_e grad mu_e + p'_e mu_e)    grad var = sum (p_e^2 grad v_e + 2 p_e p'_e v_e)
//   hard    (:879-935, 942-1010): the four quantities of the expert of the FIRST maximum of p_e
//
// Every product and sum is one IEEE operation in the order written (no contraction: kernels_infill.hip switches it off and
// the host build has none), so the device and the host form agree bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EGX_MX_HD __host__ __device__ inline
#else
#define EGX_MX_HD inline
#endif

namespace egx {
namespace infill {

// the first maximum of p[0], p[sp], ..: numpy / ndarray argmax (a NaN never wins against p[0])
EGX_MX_HD int mix_first_max(int k, const double *p, int64_t sp) {
    int best = 0;
    for (int e = 1; e < k; e++)
        if (p[e * sp] > p[best * sp]) best = e;
    return best;
}

EGX_MX_HD double mix_mean_term(double p, double mu) { return p * mu; }
// (the host fold's variance term is moe::fold_var_term, (p p) v: another association, other bits -- moe_fold.h)
EGX_MX_HD double mix_var_term(double p, double v) { return (v * p) * p; }
EGX_MX_HD double mix_grad_mean_term(double p, double dp, double mu, double gmu) { return gmu * p + dp * mu; }
EGX_MX_HD double mix_grad_var_term(double p, double dp, double v, double gv) { return gv * (p * p) + ((2.0 * p) * dp) * v; }

// mean and variance of the mixture: p (k, stride sp), the experts' mu / v (k, stride se)
EGX_MX_HD void mix_value(bool smooth, int k, const double *p, int64_t sp, const double *mu, const double *v, int64_t se,
                         double *mean, double *var) {
    if (!smooth) {
        const int e = mix_first_max(k, p, sp);
        *mean = mu[e * se];
        *var = v[e * se];
        return;
    }
    double am = 0.0, av = 0.0;
    for (int e = 0; e < k; e++) {
        am += mix_mean_term(p[e * sp], mu[e * se]);
        av += mix_var_term(p[e * sp], v[e * se]);
    }
    *mean = am;
    *var = av;
}

// their x-gradients (d each): dp[e * sdp + l] = d p_e / d x_l (unused in hard mode, may be NULL there), the experts'
// gradients gmu / gv at [e * sg + l]
EGX_MX_HD void mix_grad(bool smooth, int k, int d, const double *p, int64_t sp, const double *dp, int64_t sdp, const double *mu,
                        const double *v, int64_t se, const double *gmu, const double *gv, int64_t sg, double *gmean,
                        double *gvar) {
    if (!smooth) {
        const int e = mix_first_max(k, p, sp);
        for (int l = 0; l < d; l++) {
            gmean[l] = gmu[e * sg + l];
            gvar[l] = gv[e * sg + l];
        }
        return;
    }
    for (int l = 0; l < d; l++) {
        double am = 0.0, av = 0.0;
        for (int e = 0; e < k; e++) {
            am += mix_grad_mean_term(p[e * sp], dp[e * sdp + l], mu[e * se], gmu[e * sg + l]);
            av += mix_grad_var_term(p[e * sp], dp[e * sdp + l], v[e * se], gv[e * sg + l]);
        }
        gmean[l] = am;
        gvar[l] = av;
    }
}

// The mean half of mix_value / mix_grad alone, for a surrogate whose variance nobody reads (a constraint handed to the optimiser
// as its scaled mean): the same terms in the same order, so the bits are those of the full forms.
EGX_MX_HD double mix_mean(bool smooth, int k, const double *p, int64_t sp, const double *mu, int64_t se) {
    if (!smooth) return mu[mix_first_max(k, p, sp) * se];
    double am = 0.0;
    for (int e = 0; e < k; e++) am += mix_mean_term(p[e * sp], mu[e * se]);
    return am;
}
EGX_MX_HD void mix_grad_mean(bool smooth, int k, int d, const double *p, int64_t sp, const double *dp, int64_t sdp, const double *mu,
                             int64_t se, const double *gmu, int64_t sg, double *gmean) {
    if (!smooth) {
        const int e = mix_first_max(k, p, sp);
        for (int l = 0; l < d; l++) gmean[l] = gmu[e * sg + l];
        return;
    }
    for (int l = 0; l < d; l++) {
        double am = 0.0;
        for (int e = 0; e < k; e++) am += mix_grad_mean_term(p[e * sp], dp[e * sdp + l], mu[e * se], gmu[e * sg + l]);
        gmean[l] = am;
    }
}

}  // namespace infill
}  // namespace egx
