// Device-side pieces of the correlation kernels shared by kernels_corr.hip (correlation matrices, dense theta-gradient) and
// sgp_grad.hip (the sparse model's rectangular theta-gradient): the exponential of a non-positive argument, the per-pair
// accumulator, the LDS staging of a 64-point slab and d log r / d c of one dimension.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/egx_gp.h"

namespace egx {

constexpr double kSqrt3 = 1.7320508075688772;
constexpr double kSqrt5 = 2.23606797749979;
constexpr double k5over3 = 5.0 / 3.0;

// exp(x) for x <= 0 (every correlation is exp of a non-positive sum): round-to-nearest range reduction x = k ln2 + r,
// |r| <= ln2 / 2, degree-13 Taylor polynomial in Horner form (truncation 4e-18, all FMA), one v_ldexp_f64: ~20 VALU
// instructions and no branches or selects, against ~30 of the library exp with its special-case handling.  K1 is bound
// by FP64 VALU issue (profiles/r03_*_pmc_corr_*), so instructions per pair are what counts.  Error <= 2 ulp; underflow
// goes through ldexp (gradual, then 0); NaN propagates.
__device__ __forceinline__ double exp_nonpos(double x) {
    // exp(x) == 0 below -745.2: the clamp keeps -inf (a huge theta: the sum overflows) from turning into NaN in the
    // reduction (fma(-inf, -c, -inf)), keeps the cast of kf defined, and lets v_ldexp flush the result to 0 as the reference's
    // exp does.  A select, not fmax: a NaN argument must stay NaN (v_max_f64 would return the other operand).
    x = (x < -800.0) ? -800.0 : x;
    const double kf = __builtin_rint(x * 1.4426950408889634074);
    double r = __builtin_fma(kf, -6.93147180369123816490e-01, x);
    r = __builtin_fma(kf, -1.90821492927058770002e-10, r);
    double p = 1.6059043836821614599e-10;                  // 1 / 13!
    p = __builtin_fma(p, r, 2.0876756987868098979e-09);    // 1 / 12!
    p = __builtin_fma(p, r, 2.5052108385441718775e-08);    // 1 / 11!
    p = __builtin_fma(p, r, 2.7557319223985890653e-07);    // 1 / 10!
    p = __builtin_fma(p, r, 2.7557319223985892511e-06);    // 1 / 9!
    p = __builtin_fma(p, r, 2.4801587301587301566e-05);    // 1 / 8!
    p = __builtin_fma(p, r, 1.9841269841269841253e-04);    // 1 / 7!
    p = __builtin_fma(p, r, 1.3888888888888889419e-03);    // 1 / 6!
    p = __builtin_fma(p, r, 8.3333333333333332177e-03);    // 1 / 5!
    p = __builtin_fma(p, r, 4.1666666666666664354e-02);    // 1 / 4!
    p = __builtin_fma(p, r, 1.6666666666666665741e-01);    // 1 / 3!
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return __builtin_ldexp(p, (int)kf);
}

// Accumulator for one (i, j) pair, updated one input dimension at a time.
template <int CORR>
struct PairAcc {
    double s;  // sum inside the exponential
    double a;  // polynomial product (Matern)
    __device__ __forceinline__ PairAcc() : s(0.0), a(1.0) {}
    __device__ __forceinline__ void add(double diff, const double *__restrict__ coef, int hcols) {
        const double ad = fabs(diff);
        if (CORR == EGX_CORR_SQUARED_EXPONENTIAL) {
            const double t = coef[0] * diff;
            s = __builtin_fma(t, t, s);
        } else if (CORR == EGX_CORR_ABSOLUTE_EXPONENTIAL) {
            s = __builtin_fma(coef[0], ad, s);
        } else if (CORR == EGX_CORR_MATERN32) {
            for (int l = 0; l < hcols; l++) {
                const double t = coef[l] * ad;
                s += t;
                a *= __builtin_fma(kSqrt3, t, 1.0);
            }
        } else {
            for (int l = 0; l < hcols; l++) {
                const double t = coef[l] * ad;
                s += t;
                a *= 1.0 + kSqrt5 * t + k5over3 * (t * t);
            }
        }
    }
    // the same with the coefficient already applied to both coordinates (hcols == 1: diff = c x_i - c x_j, so that
    // c |x_i - x_j| costs no instruction per pair; the rounding of the two products perturbs the exponent by
    // <= 2 eps sum_k |t_k| max |c x|, below 1e-13 wherever r is not negligible): 2 VALU instructions per pair and dimension
    // for the squared exponential instead of 3, 5 instead of 8 for Matern-5/2
    __device__ __forceinline__ void add_scaled(double diff) {
        if (CORR == EGX_CORR_SQUARED_EXPONENTIAL) {
            s = __builtin_fma(diff, diff, s);
        } else if (CORR == EGX_CORR_ABSOLUTE_EXPONENTIAL) {
            s += fabs(diff);
        } else if (CORR == EGX_CORR_MATERN32) {
            const double t = fabs(diff);
            s += t;
            a *= __builtin_fma(kSqrt3, t, 1.0);
        } else {
            const double t = fabs(diff);
            s += t;
            a *= __builtin_fma(__builtin_fma(k5over3, t, kSqrt5), t, 1.0);
        }
    }
    __device__ __forceinline__ double value() const {
        if (CORR == EGX_CORR_SQUARED_EXPONENTIAL) return exp_nonpos(-0.5 * s);
        if (CORR == EGX_CORR_ABSOLUTE_EXPONENTIAL) return exp_nonpos(-s);
        if (CORR == EGX_CORR_MATERN32) return a * exp_nonpos(-kSqrt3 * s);
        return a * exp_nonpos(-kSqrt5 * s);
    }
};

// Stage a 64-point slab (all d dimensions, k-major) into LDS: dst[k*64 + i]; scale != nullptr: times scale[k]
// (PairAcc::add_scaled, hcols == 1).
__device__ __forceinline__ void stage_slab(double *dst, const double *__restrict__ xT, int64_t ldx, int i0,
                                           int d, int tid, const double *__restrict__ scale = nullptr, int nthreads = 256) {
    for (int e = tid; e < d * 64; e += nthreads) {
        const int k = e >> 6, i = e & 63;
        const double v = xT[(int64_t)k * ldx + i0 + i];
        dst[e] = scale ? scale[k] * v : v;
    }
}

// d log r / d c for one dimension (a = |x_i - x_j|, t = c a): the forms of kernels_corr.hip K7
__device__ __forceinline__ double rcp_ge1(double m) {  // 1 / m for m >= 1 (finite), <= 1 ulp-ish
    double y = __builtin_amdgcn_rcp(m);
    double e = __builtin_fma(-m, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-m, y, 1.0);
    return __builtin_fma(y, e, y);
}
template <int CORR>
__device__ __forceinline__ double dlog_dc(double c, double a) {
    if (CORR == EGX_CORR_SQUARED_EXPONENTIAL) return -c * a * a;
    if (CORR == EGX_CORR_ABSOLUTE_EXPONENTIAL) return -a;
    const double t = c * a;
    if (CORR == EGX_CORR_MATERN32) return -3.0 * a * t * rcp_ge1(__builtin_fma(kSqrt3, t, 1.0));
    const double u = __builtin_fma(kSqrt5, t, 1.0);
    return -k5over3 * (a * t) * u * rcp_ge1(__builtin_fma(k5over3 * t, t, u));
}

// d r / d x_k = r * xgrad_factor(x_ak - x_jk) (the closed forms above k_xgrad, kernels_corr.hip); shared with kernels_pending.hip
template <int CORR>
__device__ __forceinline__ double xgrad_factor(double diff, const double *__restrict__ c, int hcols) {
    if (CORR == EGX_CORR_SQUARED_EXPONENTIAL) return -(c[0] * c[0]) * diff;
    if (CORR == EGX_CORR_ABSOLUTE_EXPONENTIAL) return -copysign(c[0], diff);
    const double ad = fabs(diff);
    double sacc = 0.0;
    for (int l = 0; l < hcols; l++) {
        const double t = c[l] * ad;
        if (CORR == EGX_CORR_MATERN32)
            sacc += c[l] * (kSqrt3 / __builtin_fma(kSqrt3, t, 1.0) - kSqrt3);
        else
            sacc += c[l] * ((kSqrt5 + 2.0 * k5over3 * t) / (1.0 + kSqrt5 * t + k5over3 * (t * t)) - kSqrt5);
    }
    return copysign(1.0, diff) * sacc;
}

}  // namespace egx
