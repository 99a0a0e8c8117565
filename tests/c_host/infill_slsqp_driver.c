/* A compiled (plain C99) host of egx_infill_optimize_slsqp: an objective model and a constraint model (egx_gp_create +
 * egx_gp_finalize, default configuration), the handle under EGX_CSTR_MEAN, the lock-step SLSQP multistart, destroy.
 *   infill_slsqp_driver <file>
 * The file holds raw doubles: n, d, n_start, fmin, cstr_tol, scale_cstr, then theta_obj (d), theta_cstr (d), lo (d), hi (d),
 * x (n x d), y (n), c (n), starts (n_start x d) -- written by tests/test_gpu_infill_slsqp.py, which runs the same problem
 * through the Python mirror and compares what is printed here, in %a, to the last bit.  Checks on its own what needs no
 * second implementation: the result lies in the box and re-evaluates to itself, the statistics describe it.
 * What a Rust `extern "C"` shim at the InfillOptimizer::Slsqp seam would call.  Exit code 0 = all
 * good. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "egx_gp.h"

#define CHECK(call)                                                          \
    do {                                                                     \
        int32_t rc_ = (call);                                                \
        if (rc_ != EGX_SUCCESS) {                                            \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, egx_last_error()); \
            return 10 + rc_;                                                 \
        }                                                                    \
    } while (0)

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (egx_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 2;
    }
    FILE *fp = fopen(argv[1], "rb");
    double head[6];
    if (!fp || fread(head, sizeof(double), 6, fp) != 6) return 3;
    const int64_t n = (int64_t)head[0], d = (int64_t)head[1], ns = (int64_t)head[2];
    if (n < 1 || n > 4096 || d < 1 || d > 64 || ns < 1 || ns > 4096) return 3;
    const size_t total = (size_t)(4 * d + n * d + 2 * n + ns * d);
    double *buf = (double *)malloc(sizeof(double) * total);
    if (!buf || fread(buf, sizeof(double), total, fp) != total) return 3;
    fclose(fp);
    const double *theta_o = buf, *theta_c = buf + d, *lo = buf + 2 * d, *hi = buf + 3 * d, *x = buf + 4 * d;
    const double *y = x + n * d, *c = y + n, *starts = c + n;

    egx_gp_config cfg;
    egx_gp_config_default(&cfg);
    egx_gp *obj = NULL, *cstr = NULL;
    CHECK(egx_gp_create(&cfg, x, y, n, d, &obj));
    CHECK(egx_gp_create(&cfg, x, c, n, d, &cstr));
    CHECK(egx_gp_finalize(obj, theta_o, d));
    CHECK(egx_gp_finalize(cstr, theta_c, d));
    egx_infill_config ic;
    egx_infill_config_default(&ic);
    ic.criterion = EGX_INFILL_WB2;
    ic.fmin = head[3];
    egx_infill *h = NULL;
    egx_gp *cstrs[1];
    const double tols[1] = {head[4]}, scales[1] = {head[5]};
    cstrs[0] = cstr;
    CHECK(egx_infill_create(&ic, obj, cstrs, tols, 1, &h));
    CHECK(egx_infill_set_cstr_strategy(h, EGX_CSTR_MEAN, scales));

    double f_best = 0.0, c_best[1] = {0.0}, f_again = 0.0, c_again = 0.0;
    double *x_best = (double *)malloc(sizeof(double) * (size_t)d);
    int64_t *evals = (int64_t *)malloc(sizeof(int64_t) * (size_t)ns);
    int32_t *stop = (int32_t *)malloc(sizeof(int32_t) * (size_t)ns);
    if (!x_best || !evals || !stop) return 3;
    egx_infill_slsqp_stats st;
    memset(&st, 0, sizeof st);
    st.evals = evals;
    st.stop = stop;
    if (egx_infill_optimize_slsqp(h, lo, hi, starts, 0, 0, &f_best, x_best, c_best, &st) != EGX_ERR_INVALID_VALUE) return 4;
    if (egx_infill_optimize_slsqp(h, lo, hi, starts, ns, 0, &f_best, x_best, NULL, &st) != EGX_ERR_INVALID_VALUE) return 4;
    CHECK(egx_infill_optimize_slsqp(h, lo, hi, starts, ns, 0, &f_best, x_best, c_best, &st));
    CHECK(egx_infill_eval_cstr(h, x_best, 1, &f_again, &c_again, NULL, NULL));
    if (memcmp(&f_again, &f_best, sizeof f_best) != 0 || memcmp(&c_again, c_best, sizeof c_again) != 0) {
        fprintf(stderr, "optimize_slsqp: (%.17g, %.17g) re-evaluates to (%.17g, %.17g)\n", f_best, c_best[0], f_again, c_again);
        return 5;
    }
    int64_t longest = 0;
    for (int64_t k = 0; k < d; k++)
        if (x_best[k] < lo[k] || x_best[k] > hi[k]) return 6;
    for (int64_t s = 0; s < ns; s++) {
        if (evals[s] < 1 || evals[s] > 10 * ns * d || stop[s] < 1 || stop[s] > 5) return 6;
        if (evals[s] > longest) longest = evals[s];
    }
    const double viol = c_best[0] - tols[0] / scales[0];
    if (st.best_start < 0 || st.best_start >= ns || st.rounds != longest) return 6;
    if (st.feasible != (viol <= 0.0 ? 1 : 0) || st.violation != viol) return 6;
    /* the folded strategy takes the same call: no constraints are seen, c_best is not needed */
    CHECK(egx_infill_set_cstr_strategy(h, EGX_CSTR_INFILL, NULL));
    double f_in = 0.0;
    double *x_in = (double *)malloc(sizeof(double) * (size_t)d);
    if (!x_in) return 3;
    CHECK(egx_infill_optimize_slsqp(h, lo, hi, starts, ns, 0, &f_in, x_in, NULL, NULL));
    CHECK(egx_infill_eval(h, x_in, 1, &f_again, NULL, NULL));
    if (memcmp(&f_again, &f_in, sizeof f_in) != 0) return 7;

    printf("OK f %a c %a best_start %lld rounds %lld feasible %d x", f_best, c_best[0], (long long)st.best_start,
           (long long)st.rounds, (int)st.feasible);
    for (int64_t k = 0; k < d; k++) printf(" %a", x_best[k]);
    printf(" evals");
    for (int64_t s = 0; s < ns; s++) printf(" %lld", (long long)evals[s]);
    printf(" stop");
    for (int64_t s = 0; s < ns; s++) printf(" %d", (int)stop[s]);
    printf(" folded %a", f_in);
    for (int64_t k = 0; k < d; k++) printf(" %a", x_in[k]);
    printf("\n");
    egx_infill_destroy(h);
    egx_gp_destroy(obj);
    egx_gp_destroy(cstr);
    free(buf), free(x_best), free(evals), free(stop), free(x_in);
    return 0;
}
