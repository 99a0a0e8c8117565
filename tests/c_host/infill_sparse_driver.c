/* A compiled (plain C99) host of the infill criterion on SPARSE models: a sparse objective (egx_sgp_create + egx_sgp_finalize)
 * with one sparse and one dense constraint through egx_infill_create_any, then egx_infill_scaling / egx_infill_eval /
 * egx_infill_optimize and, under EGX_CSTR_MEAN, egx_infill_eval_cstr.
 * Checks only what needs no second implementation: the sparse parts against the model's own egx_sgp_predict_valvar, values with
 * and without gradients bit for bit, a point alone against the point in the batch bit for bit, the constraint means of the
 * mean-only sequence against the full sequence bit for bit, the optimiser's result inside the box and re-evaluating to
 * itself, and the refusals that come before the device is touched.  Exit code 0 = all good. */
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

enum { N = 400, NZ = 30, NC = 150, D = 2, M = 131, NS = 4 };

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
    static double x[N * D], y[N], yc[N], z[NZ * D], xd[NC * D], yd[NC], xq[M * D];
    static double val[M], val2[M], grad[M * D], mean[3 * M], var[3 * M], pm[M], pv[M], cstr[M * 2], cval[M];
    for (int i = 0; i < N; i++) {
        x[i * D] = urand(); x[i * D + 1] = urand();
        y[i] = sin(5.0 * x[i * D]) + x[i * D + 1] * x[i * D + 1] + 0.01 * (urand() - 0.5);
        yc[i] = x[i * D] + x[i * D + 1] - 1.2 + 0.01 * (urand() - 0.5);
    }
    memcpy(z, x, sizeof z); /* the first NZ training points as inducing points */
    for (int i = 0; i < NC; i++) {
        xd[i * D] = urand(); xd[i * D + 1] = urand();
        yd[i] = xd[i * D] * xd[i * D + 1] - 0.4;
    }
    for (int i = 0; i < M * D; i++) xq[i] = urand();
    double fmin = 1e300;
    for (int i = 0; i < N; i++) if (y[i] < fmin) fmin = y[i];
    const double theta[D] = {1.5, 1.1};

    egx_sgp_config sc;
    egx_sgp_config_default(&sc);
    sc.corr = EGX_CORR_MATERN52;
    egx_sgp *obj = NULL, *cs = NULL;
    CHECK(egx_sgp_create(&sc, x, y, N, D, z, NZ, &obj));
    sc.method = EGX_SGP_VFE;
    CHECK(egx_sgp_create(&sc, x, yc, N, D, z, NZ, &cs));
    CHECK(egx_sgp_finalize(obj, theta, D, 0.8, 1e-3));
    CHECK(egx_sgp_finalize(cs, theta, D, 0.5, 1e-3));
    egx_gp_config gc;
    egx_gp_config_default(&gc);
    egx_gp *cd = NULL;
    CHECK(egx_gp_create(&gc, xd, yd, NC, D, &cd));
    CHECK(egx_gp_finalize(cd, theta, D));

    egx_model_ref r0[1], r1[1], r2[1];
    r0[0].kind = EGX_MODEL_SGP; r0[0].handle = obj;
    r1[0].kind = EGX_MODEL_SGP; r1[0].handle = cs;
    r2[0].kind = EGX_MODEL_GP; r2[0].handle = cd;
    egx_infill_surrogate_any s[3];
    memset(s, 0, sizeof s);
    s[0].experts = r0; s[1].experts = r1; s[2].experts = r2;
    for (int j = 0; j < 3; j++) { s[j].n_experts = 1; s[j].heaviside_factor = 1.0; s[j].smooth = 1; }
    const double tols[2] = {0.0, 0.0};
    egx_infill_config ic;
    egx_infill_config_default(&ic);
    ic.criterion = EGX_INFILL_WB2;
    ic.fmin = fmin;

    { /* refusals before the device is touched */
        egx_infill *h = NULL;
        r1[0].kind = 7;
        if (egx_infill_create_any(&ic, s, tols, 2, &h) != EGX_ERR_INVALID_VALUE || h != NULL) return 9;
        if (!strstr(egx_last_error(), "surrogate 1 expert 0")) return 9;
        r1[0].kind = EGX_MODEL_SGP;
        s[2].n_experts = 0;
        if (egx_infill_create_any(&ic, s, tols, 2, &h) != EGX_ERR_INVALID_VALUE || h != NULL) return 9;
        s[2].n_experts = 1;
    }

    egx_infill *h = NULL;
    CHECK(egx_infill_create_any(&ic, s, tols, 2, &h));
    double scale_ic, scale, scale_cstr[2];
    CHECK(egx_infill_scaling(h, xq, M, &scale_ic, &scale, scale_cstr));
    if (!(scale > 0.0) || !(scale_cstr[0] > 0.0) || !(scale_cstr[1] > 0.0)) return 3;
    egx_infill_parts parts;
    parts.mean = mean; parts.var = var; parts.grad_mean = NULL; parts.grad_var = NULL;
    CHECK(egx_infill_eval(h, xq, M, val, grad, &parts));
    CHECK(egx_infill_eval(h, xq, M, val2, NULL, NULL));
    if (memcmp(val, val2, sizeof val) != 0) {
        fprintf(stderr, "values with and without gradients differ\n");
        return 5;
    }
    /* the sparse parts are the model's own predictions (another summation order of the mean: 1e-9), variance = clamp + noise */
    CHECK(egx_sgp_predict_valvar(obj, xq, M, pm, pv));
    for (int a = 0; a < M; a++)
        if (fabs(mean[a] - pm[a]) > 1e-9 * (1.0 + fabs(pm[a])) || fabs(var[a] - pv[a]) > 1e-9 * (1.0 + pv[a]) || !(var[a] >= 1e-3)) {
            fprintf(stderr, "point %d: parts %.17g %.17g, the model %.17g %.17g\n", a, mean[a], var[a], pm[a], pv[a]);
            return 4;
        }
    for (int a = 0; a < M; a += 13) { /* a point alone = the point in the batch (the last one sits in the second tile) */
        double v1, g1[D];
        CHECK(egx_infill_eval(h, xq + a * D, 1, &v1, g1, NULL));
        if (memcmp(&v1, &val[a], sizeof v1) != 0 || memcmp(g1, &grad[a * D], sizeof g1) != 0) {
            fprintf(stderr, "point %d alone differs from the batch\n", a);
            return 6;
        }
    }
    { /* central difference of the objective at one point */
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
    const double lo[D] = {0.0, 0.0}, hi[D] = {1.0, 1.0};
    double starts[NS * D], f_best, x_best[D], f_again;
    int64_t evals[NS];
    for (int i = 0; i < NS * D; i++) starts[i] = urand();
    egx_infill_stats st;
    st.evals = evals;
    CHECK(egx_infill_optimize(h, lo, hi, starts, NS, 40, &f_best, x_best, &st));
    CHECK(egx_infill_eval(h, x_best, 1, &f_again, NULL, NULL));
    if (memcmp(&f_again, &f_best, sizeof f_best) != 0) {
        fprintf(stderr, "optimize: f_best %.17g, re-evaluated %.17g\n", f_best, f_again);
        return 8;
    }
    for (int k = 0; k < D; k++)
        if (x_best[k] < lo[k] || x_best[k] > hi[k]) return 9;
    if (st.best_start < 0 || st.best_start >= NS || st.rounds < 1) return 9;

    /* the constraints handed to the optimiser: the mean-only sequence keeps the bits of the full one */
    const double ones[2] = {1.0, 1.0};
    CHECK(egx_infill_set_cstr_strategy(h, EGX_CSTR_MEAN, ones));
    CHECK(egx_infill_eval_cstr(h, xq, M, cval, cstr, NULL, NULL));
    for (int a = 0; a < M; a++)
        if (memcmp(&cstr[a * 2], &mean[M + a], sizeof(double)) != 0 || memcmp(&cstr[a * 2 + 1], &mean[2 * M + a], sizeof(double)) != 0) {
            fprintf(stderr, "point %d: mean-only constraint values differ from the full sequence\n", a);
            return 4;
        }
    egx_infill_destroy(h);
    egx_gp_destroy(cd);
    egx_sgp_destroy(cs);
    egx_sgp_destroy(obj);
    printf("OK\n");
    return 0;
}
