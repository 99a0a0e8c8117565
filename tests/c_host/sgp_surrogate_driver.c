/* A plain C99 host of the sparse GP's surrogate entry points: egx_sgp_predict_valvar, the three analytic x-gradient calls and
 * egx_sgp_sample, on the five-point problem of golden_a_driver.c (all five points inducing).  What a Rust `extern "C"` shim
 * behind SgpSurrogate would call.  Exit code 0 = all good, 77 = no HIP device. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "egx_gp.h"

#define CHECK(call)                                                              \
    do {                                                                         \
        int32_t rc_ = (call);                                                    \
        if (rc_ != EGX_SUCCESS) {                                                \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, egx_last_error());     \
            return 10 + rc_;                                                     \
        }                                                                        \
    } while (0)

static int close_to(double a, double b, double tol, const char *what) {
    if (fabs(a - b) <= tol) return 1;
    fprintf(stderr, "%s: got %.15g, want %.15g (tol %g)\n", what, a, b, tol);
    return 0;
}

int main(void) {
    const double xt[5] = {0.0, 1.0, 2.0, 3.0, 4.0}, yt[5] = {0.0, 1.0, 1.5, 0.9, 1.0};
    const double theta = 1.83209405, sigma2 = 0.3, noise = 1e-4;
    if (egx_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 77;
    }
    egx_sgp *sgp = NULL;
    CHECK(egx_sgp_create(NULL, xt, yt, 5, 1, xt, 5, &sgp));
    const double xq[3] = {0.4, 1.1, 2.7};
    double y[3], v[3], y2[3], v2[3], gy[3], gv[3], gy2[3], gv2[3];
    int ok = egx_sgp_predict_valvar(sgp, xq, 3, y, v) == EGX_ERR_NOT_FITTED;
    CHECK(egx_sgp_finalize(sgp, &theta, 1, sigma2, noise));
    CHECK(egx_sgp_predict(sgp, xq, 3, y));
    CHECK(egx_sgp_predict_var(sgp, xq, 3, v));
    CHECK(egx_sgp_predict_valvar(sgp, xq, 3, y2, v2));
    CHECK(egx_sgp_predict_gradients(sgp, xq, 3, gy));
    CHECK(egx_sgp_predict_var_gradients(sgp, xq, 3, gv));
    CHECK(egx_sgp_predict_valvar_gradients(sgp, xq, 3, gy2, gv2));
    CHECK(egx_sgp_predict_valvar(sgp, xq, 0, NULL, NULL)); /* m = 0: nothing to do */
    const double h = 1e-5;
    for (int i = 0; i < 3; i++) {
        ok &= y[i] == y2[i] && v[i] == v2[i] && gy[i] == gy2[i] && gv[i] == gv2[i];
        /* the closed form against central differences of the library's own predictions */
        const double xs[2] = {xq[i] + h, xq[i] - h};
        double ys[2], vs[2];
        CHECK(egx_sgp_predict_valvar(sgp, xs, 2, ys, vs));
        ok &= close_to(gy[i], (ys[0] - ys[1]) / (2 * h), 1e-6, "d mean / dx");
        ok &= close_to(gv[i], (vs[0] - vs[1]) / (2 * h), 1e-6, "d var / dx");
    }
    /* trajectories: z = I gives the factor F of the PRIOR covariance sigma2 r(xq, xq) */
    const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double f[9], tau = -1.0;
    CHECK(egx_sgp_sample(sgp, xq, 3, 3, EGX_SAMPLE_CHOLESKY, 0, eye, f, &tau));
    ok &= tau == 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) f[i * 3 + j] -= y[i];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j <= i; j++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += f[i * 3 + k] * f[j * 3 + k];
            const double dx = theta * (xq[i] - xq[j]);
            ok &= close_to(s, sigma2 * exp(-0.5 * dx * dx), 1e-12, "F F^T = sigma2 r(x, x)");
        }
    double t1[6], t2[12];
    CHECK(egx_sgp_sample(sgp, xq, 3, 2, EGX_SAMPLE_PSD, 42, NULL, t1, &tau));
    CHECK(egx_sgp_sample(sgp, xq, 3, 4, EGX_SAMPLE_PSD, 42, NULL, t2, NULL));
    ok &= tau >= 1e-9;
    for (int i = 0; i < 3; i++) ok &= t1[i * 2] == t2[i * 4] && t1[i * 2 + 1] == t2[i * 4 + 1] && isfinite(t1[i * 2]);
    ok &= egx_sgp_predict_gradients(sgp, NULL, 3, gy) == EGX_ERR_INVALID_VALUE;
    egx_sgp_destroy(sgp);
    printf("%s: predict(1.1) %.6f dy/dx %.6f dvar/dx %.6g\n", ok ? "OK" : "FAILED", y[1], gy[1], gv[1]);
    return ok ? 0 : 1;
}
