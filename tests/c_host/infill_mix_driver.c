/* A compiled (plain C99) host of the mixture entry points of the infill criterion: an objective surrogate of two experts with
 * an explicit two-cluster Gaussian mixture and a single-expert constraint (egx_gp_create + egx_gp_finalize), through
 * egx_infill_create_mix / egx_infill_eval / egx_infill_eval_experts / egx_infill_optimize, smooth and hard.
 * Checks only what needs no second implementation: the responsibilities of a point sum to one, the smooth mean and variance
 * are the weighted sums of the returned expert parts, the hard parts are those of the expert with the larger responsibility
 * bit for bit, a point alone equals the point in the batch bit for bit, values with and without gradients agree bit for bit,
 * and the optimiser's result is inside the box and re-evaluates to itself.  Exit code 0 = all good. */
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

enum { N0 = 160, N1 = 140, NC = 150, D = 2, M = 37, NS = 4, K = 2 };

static unsigned long long rng_state = 88172645463325252ULL;
static double urand(void) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

static void fill(double *x, double *y, int n, double x0_lo, double x0_hi, int which) {
    for (int i = 0; i < n; i++) {
        x[i * D] = x0_lo + (x0_hi - x0_lo) * urand();
        x[i * D + 1] = urand();
        y[i] = which ? x[i * D] + x[i * D + 1] - 1.2 : sin(5.0 * x[i * D]) + x[i * D + 1] * x[i * D + 1];
    }
}

int main(void) {
    if (egx_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 2;
    }
    static double x0[N0 * D], y0[N0], x1[N1 * D], y1[N1], xc[NC * D], yc[NC], xq[M * D];
    static double val[M], val2[M], grad[M * D], mean[2 * M], var[2 * M];
    static double emean[K * M], evar[K * M], probas[M * K], dprobas[M * K * D];
    const double theta[D] = {1.5, 1.1};
    fill(x0, y0, N0, 0.0, 0.6, 0); /* the two experts overlap on 0.4 <= x0 <= 0.6 */
    fill(x1, y1, N1, 0.4, 1.0, 0);
    fill(xc, yc, NC, 0.0, 1.0, 1);
    double fmin = 1e300;
    for (int i = 0; i < N0; i++) if (y0[i] < fmin) fmin = y0[i];
    egx_gp_config cfg;
    egx_gp_config_default(&cfg);
    egx_gp *e0 = NULL, *e1 = NULL, *cstr = NULL;
    CHECK(egx_gp_create(&cfg, x0, y0, N0, D, &e0));
    CHECK(egx_gp_create(&cfg, x1, y1, N1, D, &e1));
    CHECK(egx_gp_create(&cfg, xc, yc, NC, D, &cstr));
    CHECK(egx_gp_finalize(e0, theta, D));
    CHECK(egx_gp_finalize(e1, theta, D));
    CHECK(egx_gp_finalize(cstr, theta, D));

    /* clusters at x0 = 0.3 and 0.7, standard deviation 0.2 / 0.5: precisions_chol = diag(1 / sd), upper triangular */
    const double weights[K] = {0.5, 0.5}, means[K * D] = {0.3, 0.5, 0.7, 0.5};
    const double chol[K * D * D] = {5.0, 0.0, 0.0, 2.0, 5.0, 0.0, 0.0, 2.0};
    egx_gp *experts[K], *lone[1];
    experts[0] = e0; experts[1] = e1; lone[0] = cstr;
    egx_infill_surrogate s[2];
    memset(s, 0, sizeof s);
    s[0].experts = experts; s[0].n_experts = K; s[0].weights = weights; s[0].means = means; s[0].precisions_chol = chol;
    s[0].heaviside_factor = 1.0; s[0].smooth = 1;
    s[1].experts = lone; s[1].n_experts = 1; s[1].heaviside_factor = 1.0; s[1].smooth = 1; /* no mixture: one expert */
    const double tols[1] = {0.0};
    egx_infill_config ic;
    egx_infill_config_default(&ic);
    ic.criterion = EGX_INFILL_WB2;
    ic.fmin = fmin;
    for (int i = 0; i < M * D; i++) xq[i] = urand();

    for (int smooth = 1; smooth >= 0; smooth--) {
        egx_infill *h = NULL;
        s[0].smooth = smooth;
        CHECK(egx_infill_create_mix(&ic, s, tols, 1, &h));
        egx_infill_parts parts;
        parts.mean = mean; parts.var = var; parts.grad_mean = NULL; parts.grad_var = NULL;
        CHECK(egx_infill_eval(h, xq, M, val, grad, &parts));
        CHECK(egx_infill_eval(h, xq, M, val2, NULL, NULL));
        if (memcmp(val, val2, sizeof val) != 0) {
            fprintf(stderr, "values with and without gradients differ\n");
            return 5;
        }
        CHECK(egx_infill_eval_experts(h, 0, xq, M, emean, evar, NULL, NULL, probas, dprobas));
        for (int a = 0; a < M; a++) {
            const double p0 = probas[a * K], p1 = probas[a * K + 1];
            if (fabs(p0 + p1 - 1.0) > 1e-12) {
                fprintf(stderr, "responsibilities of point %d sum to %.17g\n", a, p0 + p1);
                return 3;
            }
            for (int k = 0; k < D; k++) /* ... and their derivatives to zero */
                if (fabs(dprobas[(a * K) * D + k] + dprobas[(a * K + 1) * D + k]) > 1e-9) return 3;
            if (smooth) {
                const double wm = p0 * emean[a] + p1 * emean[M + a], wv = p0 * p0 * evar[a] + p1 * p1 * evar[M + a];
                if (fabs(wm - mean[a]) > 1e-13 * (fabs(p0 * emean[a]) + fabs(p1 * emean[M + a])) ||
                    fabs(wv - var[a]) > 1e-13 * (p0 * p0 * evar[a] + p1 * p1 * evar[M + a])) {
                    fprintf(stderr, "point %d: smooth parts %.17g %.17g, from the experts %.17g %.17g\n", a, mean[a], var[a], wm, wv);
                    return 4;
                }
            } else {
                const int w = p1 > p0 ? 1 : 0;
                if (memcmp(&mean[a], &emean[w * M + a], sizeof(double)) != 0 || memcmp(&var[a], &evar[w * M + a], sizeof(double)) != 0) {
                    fprintf(stderr, "point %d: hard parts are not expert %d's\n", a, w);
                    return 4;
                }
            }
        }
        { /* the single-expert constraint: its expert IS the surrogate, the responsibilities are ones */
            static double cm[M], cp[M];
            CHECK(egx_infill_eval_experts(h, 1, xq, M, cm, NULL, NULL, NULL, cp, NULL));
            if (memcmp(cm, mean + M, sizeof cm) != 0) return 4;
            for (int a = 0; a < M; a++) if (cp[a] != 1.0) return 4;
        }
        for (int a = 0; a < M; a += 9) { /* a point alone = the point in the batch */
            double v1, g1[D];
            CHECK(egx_infill_eval(h, xq + a * D, 1, &v1, g1, NULL));
            if (memcmp(&v1, &val[a], sizeof v1) != 0 || memcmp(g1, &grad[a * D], sizeof g1) != 0) {
                fprintf(stderr, "point %d alone differs from the batch\n", a);
                return 6;
            }
        }
        if (smooth) { /* central difference at one point (the hard recombination jumps where the winner changes) */
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
        egx_infill_destroy(h);
    }
    { /* refusals before the device is touched */
        egx_infill *h = NULL;
        s[0].heaviside_factor = 0.0;
        if (egx_infill_create_mix(&ic, s, tols, 1, &h) != EGX_ERR_INVALID_VALUE || h != NULL) return 9;
        s[0].heaviside_factor = 1.0;
        s[0].n_experts = 0;
        if (egx_infill_create_mix(&ic, s, tols, 1, &h) != EGX_ERR_INVALID_VALUE || h != NULL) return 9;
    }
    egx_gp_destroy(cstr);
    egx_gp_destroy(e1);
    egx_gp_destroy(e0);
    printf("OK\n");
    return 0;
}
