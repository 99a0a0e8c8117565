// The responsibilities of a Gaussian mixture at ONE point (GaussianMixture::predict_probas / predict_probas_derivatives,
// crates/moe/src/gaussian_mixture.rs:114-170, 231-283): the one text behind k_gmx_probas / k_gmx_probas_deriv (kernels_gmm.hip)
// and k_infill_mix (kernels_infill.hip), and the host preparation of the operands they read (gmx_pack).  A lane owns the point; x, z, vp and
// u are the lane's own scratch rows, means / precs / par are read at wave-uniform addresses.
// The bodies switch FMA contraction OFF and spell out every fused multiply-add, so that every translation unit runs the same
// operations whatever its contraction mode: the explicit ones are those the compiler's default mode chose when the two
// k_gmx_* kernels held this text themselves (v' += u' and u' v - u v'), which therefore keep their bits.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace egx {

// scaled factors and the per-cluster constant (:105-110, 253-283): precs = P * hf^-0.5, log det = sum log diag(precs),
// par[c] = log w_c + log det_c - 0.5 d ln 2 pi
inline void gmx_scaled_factors(const double *weights, const double *precisions_chol, int64_t k, int64_t d, double heaviside_factor,
                               double *precs, double *par) {
    const double factor = std::pow(heaviside_factor, -0.5);
    const double cst = (double)d * std::log(2.0 * M_PI);
    for (int64_t c = 0; c < k; c++) {
        double ld = 0.0;
        for (int64_t i = 0; i < d * d; i++) precs[(size_t)c * d * d + i] = precisions_chol[(size_t)c * d * d + i] * factor;
        for (int64_t i = 0; i < d; i++) ld += std::log(precs[(size_t)c * d * d + i * d + i]);
        par[c] = (-0.5 * cst + ld) + std::log(weights[c]);
    }
}

// the operands of the three kernels as ONE block: [means (k d) | scaled factors (k d d) | par (k)]
inline std::vector<double> gmx_pack(const double *weights, const double *means, const double *precisions_chol, int64_t k, int64_t d,
                                    double heaviside_factor) {
    std::vector<double> blk((size_t)(k * d + k * d * d + k));
    std::copy(means, means + k * d, blk.begin());
    gmx_scaled_factors(weights, precisions_chol, k, d, heaviside_factor, blk.data() + k * d, blk.data() + k * d + k * d * d);
    return blk;
}

#if defined(__HIPCC__)
// q_c = || (x - mu_c) P_c ||^2; weighted log probability, the sum of the exponentials above f64::MIN_10_EXP, its logarithm
// unless the sum is below epsilon (:236-251), exp of the difference (:119).  out: k values (the lane's own).
__device__ inline void gmx_probas_point(const double *x, int d, int k, const double *__restrict__ means,
                                        const double *__restrict__ precs, const double *__restrict__ par, double *out) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int c = 0; c < k; c++) {
        const double *mu = means + (size_t)c * d, *P = precs + (size_t)c * d * d;
        double q = 0.0;
        for (int j = 0; j < d; j++) {
            double acc = 0.0;
            for (int i = 0; i < d; i++) acc = __builtin_fma(x[i] - mu[i], P[(size_t)i * d + j], acc);
            q = __builtin_fma(acc, acc, q);
        }
        const double wlp = par[c] - 0.5 * q;
        out[c] = wlp;
        s += (wlp <= -307.0) ? 0.0 : exp(wlp);
    }
    const double norm = (fabs(s) < 2.220446049250313e-16) ? 0.0 : log(s);
    for (int c = 0; c < k; c++) out[c] = exp(out[c] - norm);
}

//   u_c = w_c pdf_c(x),  v = sum_c u_c,  deriv_c = (x - mu_c) precisions_c / hf,  u'_c = -deriv_c u_c,  v' = sum_c u'_c
//   d p_c / d x = (u'_c v - u_c v') / v^2
// With the scaled factor P' = precisions_chol_c hf^-1/2 (what pdfs() itself uses, :253-283): z = (x - mu_c) P' gives both the
// quadratic form |z|^2 of the pdf and deriv_c = z P'^T (precisions = P P^T, :208-217).  Pass A writes u'_c to the output and
// accumulates v, v'; pass B finishes the output in place.  z, vp: d each, u: k (the lane's scratch); o: k x d.
__device__ inline void gmx_probas_deriv_point(const double *x, double *z, double *vp, double *u, int d, int k,
                                              const double *__restrict__ means, const double *__restrict__ precs,
                                              const double *__restrict__ par, double *o) {
#pragma clang fp contract(off)
    for (int l = 0; l < d; l++) vp[l] = 0.0;
    double v = 0.0;
    for (int c = 0; c < k; c++) {
        const double *mu = means + (size_t)c * d, *P = precs + (size_t)c * d * d;
        double q = 0.0;
        for (int j = 0; j < d; j++) {
            double acc = 0.0;
            for (int i = 0; i < d; i++) acc = __builtin_fma(x[i] - mu[i], P[(size_t)i * d + j], acc);
            z[j] = acc;
            q = __builtin_fma(acc, acc, q);
        }
        const double uc = exp(par[c] - 0.5 * q);  // w_c pdf_c(x)  (:136-139: no MIN_10_EXP guard on this path)
        u[c] = uc;
        v += uc;
        for (int l = 0; l < d; l++) {
            double acc = 0.0;
            for (int j = 0; j < d; j++) acc = __builtin_fma(z[j], P[(size_t)l * d + j], acc);
            o[(int64_t)c * d + l] = -acc * uc;
            vp[l] = __builtin_fma(-acc, uc, vp[l]);  // v' += u', the product not rounded
        }
    }
    const double v2 = v * v;
    for (int c = 0; c < k; c++)
        for (int l = 0; l < d; l++) o[(int64_t)c * d + l] = __builtin_fma(o[(int64_t)c * d + l], v, -(u[c] * vp[l])) / v2;
}
#endif

}  // namespace egx
