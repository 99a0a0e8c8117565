/* A compiled (plain C99) host of the infill entry points: an objective model and a constraint model (egx_gp_create +
 * egx_gp_finalize), the scaling pass, one evaluation with gradients and parts, the lock-step multistart, destroy.
 * Checks only what needs no second implementation: the evaluation of a point alone equals its evaluation in the batch bit
 * for bit, the values with and without gradients agree bit for bit, the gradient matches a central difference of the value,
 * and the optimiser's result is inside the box, not above the best start, and re-evaluates to itself.
 * What a Rust `extern "C"` shim behind InfillCriterion::{value, grad, scaling} and optimize_infill_criterion would call
 * (INTEGRATION.md).  Exit code 0 = all good. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "egx_gp.h"

#define CHECK(call)                                                              \
    do {                                                                         \
        int32_t rc_ = (call);                                                    \
        if (rc_ != EGX_SUCCESS) {                                                \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, egx_last_error());     \
            return 10 + rc_;                                                     \
        }                                                                        \
    } while (0)

enum { N = 300, D = 2, M = 37, NS = 5, NPTS = 200 };

static unsigned long long rng_state = 88172645463325252ULL;
static double urand(void) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

int main(void) {
    if (egx_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 2;
    }
    static double x[N * D], y[N], c[N], xq[M * D], pts[NPTS * D];
    static double val[M], val2[M], grad[M * D], mean[2 * M], var[2 * M];
    const double theta[D] = {1.5, 1.1};
    double fmin = 1e300;
    for (int i = 0; i < N; i++) {
        x[i * D] = urand();
        x[i * D + 1] = urand();
        y[i] = sin(5.0 * x[i * D]) + x[i * D + 1] * x[i * D + 1];
        c[i] = x[i * D] + x[i * D + 1] - 1.2; /* feasible where c <= 0 */
        if (y[i] < fmin) fmin = y[i];
    }
    egx_gp_config cfg;
    egx_gp_config_default(&cfg);
    egx_gp *obj = NULL, *cstr = NULL;
    CHECK(egx_gp_create(&cfg, x, y, N, D, &obj));
    CHECK(egx_gp_create(&cfg, x, c, N, D, &cstr));
    CHECK(egx_gp_finalize(obj, theta, D));
    CHECK(egx_gp_finalize(cstr, theta, D));

    egx_infill_config ic;
    egx_infill_config_default(&ic);
    ic.criterion = EGX_INFILL_WB2S;
    ic.fmin = fmin;
    egx_infill *h = NULL;
    egx_gp *cstrs[1];
    const double tols[1] = {0.0};
    cstrs[0] = cstr;
    CHECK(egx_infill_create(&ic, obj, cstrs, tols, 1, &h));

    for (int i = 0; i < NPTS * D; i++) pts[i] = urand();
    double scale_ic = 0.0, scale = 0.0, scale_cstr[1] = {0.0};
    CHECK(egx_infill_scaling(h, pts, NPTS, &scale_ic, &scale, scale_cstr));
    if (!(scale > 0.0) || !(scale_cstr[0] > 0.0) || !isfinite(scale_ic)) {
        fprintf(stderr, "scaling: %g %g %g\n", scale_ic, scale, scale_cstr[0]);
        return 3;
    }
    egx_infill_config now;
    CHECK(egx_infill_get_params(h, &now));
    if (now.scale != scale || now.scale_ic != scale_ic) return 4;

    for (int i = 0; i < M * D; i++) xq[i] = urand();
    egx_infill_parts parts;
    parts.mean = mean; parts.var = var; parts.grad_mean = NULL; parts.grad_var = NULL;
    CHECK(egx_infill_eval(h, xq, M, val, grad, &parts));
    CHECK(egx_infill_eval(h, xq, M, val2, NULL, NULL));
    if (memcmp(val, val2, sizeof val) != 0) {
        fprintf(stderr, "values with and without gradients differ\n");
        return 5;
    }
    for (int a = 0; a < M; a += 9) { /* a point alone = the point in the batch */
        double v1, g1[D];
        CHECK(egx_infill_eval(h, xq + a * D, 1, &v1, g1, NULL));
        if (memcmp(&v1, &val[a], sizeof v1) != 0 || memcmp(g1, &grad[a * D], sizeof g1) != 0) {
            fprintf(stderr, "point %d alone differs from the batch\n", a);
            return 6;
        }
    }
    { /* central difference at one point */
        const double e = 1e-5;
        double xp[2 * D], vp[2];
        for (int k = 0; k < D; k++) {
            memcpy(xp, xq, sizeof(double) * D);
            memcpy(xp + D, xq, sizeof(double) * D);
            xp[k] += e;
            xp[D + k] -= e;
            CHECK(egx_infill_eval(h, xp, 2, vp, NULL, NULL));
            const double fd = (vp[0] - vp[1]) / (2.0 * e);
            if (fabs(fd - grad[k]) > 1e-5 * (1.0 + fabs(fd))) {
                fprintf(stderr, "gradient %d: %.12g against the difference quotient %.12g\n", k, grad[k], fd);
                return 7;
            }
        }
    }
    CHECK(egx_infill_eval(h, xq, 0, NULL, NULL, NULL));

    const double lo[D] = {0.0, 0.0}, hi[D] = {1.0, 1.0};
    double starts[NS * D], f_best, x_best[D], f_again, best_start_val = 1e300;
    int64_t evals[NS];
    for (int i = 0; i < NS * D; i++) starts[i] = urand();
    egx_infill_stats st;
    st.evals = evals;
    CHECK(egx_infill_optimize(h, lo, hi, starts, NS, 0, &f_best, x_best, &st));
    CHECK(egx_infill_eval(h, starts, NS, val, NULL, NULL));
    for (int s = 0; s < NS; s++)
        if (val[s] < best_start_val) best_start_val = val[s];
    CHECK(egx_infill_eval(h, x_best, 1, &f_again, NULL, NULL));
    if (memcmp(&f_again, &f_best, sizeof f_best) != 0 || f_best > best_start_val) {
        fprintf(stderr, "optimize: f_best %.17g, re-evaluated %.17g, best start %.17g\n", f_best, f_again, best_start_val);
        return 8;
    }
    for (int k = 0; k < D; k++)
        if (x_best[k] < lo[k] || x_best[k] > hi[k]) return 9;
    for (int s = 0; s < NS; s++)
        if (evals[s] < 1 || evals[s] > 10 * NS * D) return 9;
    if (st.best_start < 0 || st.best_start >= NS || st.rounds < 1) return 9;

    egx_infill_destroy(h);
    egx_gp_destroy(cstr);
    egx_gp_destroy(obj);
    printf("OK scale_ic %.6g scale %.6g f_best %.9g at (%.6f, %.6f) rounds %lld\n", scale_ic, scale, f_best, x_best[0], x_best[1],
           (long long)st.rounds);
    return 0;
}
