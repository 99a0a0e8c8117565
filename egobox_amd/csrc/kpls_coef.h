// The coefficient table of a KPLS-reduced correlation and the chain rule back to theta: host code only, shared by the dense model
// (make_coef, gp_host.hip; grad_chain_rule, gp_fit.hip) and the sparse one (sgp_host.hip, sgp_grad.hip), and checked on its own
// by tests/c_host/kpls_coef_test.cpp.  With the weights w (d x h, row-major) and theta (h) the kernels read one table
// coef (d x hcols), see kernels_corr.hip / corr_pair.h PairAcc::add:
//   squared exponential   hcols = 1   c_j  = sqrt(sum_l (theta_l w_jl)^2)      correlation_models.rs:97-98
//   absolute exponential  hcols = 1   c_j  = sum_l theta_l |w_jl|               :191
//   Matern-3/2, -5/2      hcols = h   c_jl = theta_l |w_jl|                     :333, :505
// Without weights (w == nullptr: w = I, h == d) the table is theta itself, hcols = 1.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/egx_gp.h"

namespace egx {
namespace kpls {

// coef <- the table of (corr, d, h, w, th); returns hcols
inline int coef_table(int corr, int d, int h, const double *w, const double *th, std::vector<double> &coef) {
    if (!w) {
        coef.assign(th, th + h);  // h == d
        return 1;
    }
    if (corr == EGX_CORR_SQUARED_EXPONENTIAL) {
        coef.assign(d, 0.0);
        for (int j = 0; j < d; j++) {
            double s = 0.0;
            for (int l = 0; l < h; l++) s += (th[l] * w[j * h + l]) * (th[l] * w[j * h + l]);
            coef[j] = std::sqrt(s);
        }
        return 1;
    }
    if (corr == EGX_CORR_ABSOLUTE_EXPONENTIAL) {
        coef.assign(d, 0.0);
        for (int j = 0; j < d; j++) {
            double s = 0.0;
            for (int l = 0; l < h; l++) s += std::fabs(w[j * h + l]) * th[l];
            coef[j] = s;
        }
        return 1;
    }
    coef.assign((size_t)d * h, 0.0);
    for (int j = 0; j < d; j++)
        for (int l = 0; l < h; l++) coef[j * h + l] = th[l] * std::fabs(w[j * h + l]);
    return h;
}

// grad (h) = dL/dtheta from the kernel's sums gsum, each divided by div first (the dense kernel sums are per ln theta ... / ln 10;
// the sparse ones pass 1).  Without weights, or with hcols > 1 (Matern: the kernel's outputs are per theta already), gsum has h
// entries and is passed on.  With a collapsed coefficient c_j (gsum: d entries, dL/dc_j) the chain rule dc_j / dtheta_l is
//   squared exponential   theta_l w_jl^2 / c_j     (a row with c_j == 0 contributes nothing)
//   absolute exponential  |w_jl|
// ratio_first: theta_l w_jl^2 / c_j is formed before it meets the sum -- exactly 1 where w is the identity, so that the sparse
// model under w = I returns the bits of a handle without weights; the dense model keeps the order its results were pinned with.
inline void chain_rule(int corr, int d, int h, const double *w, int hcols, const double *coef, const double *th, const double *gsum,
                       double div, double *grad, bool ratio_first = false) {
    if (!w || hcols > 1) {
        for (int k = 0; k < h; k++) grad[k] = gsum[k] / div;
        return;
    }
    for (int l = 0; l < h; l++) {
        double sacc = 0.0;
        for (int j = 0; j < d; j++) {
            const double wjl = w[(size_t)j * h + l], pk = gsum[j] / div;
            if (corr == EGX_CORR_SQUARED_EXPONENTIAL) {
                if (coef[j] > 0.0) sacc += ratio_first ? pk * (th[l] * wjl * wjl / coef[j]) : pk * th[l] * wjl * wjl / coef[j];
            } else {
                sacc += pk * std::fabs(wjl);
            }
        }
        grad[l] = sacc;
    }
}

}  // namespace kpls
}  // namespace egx
