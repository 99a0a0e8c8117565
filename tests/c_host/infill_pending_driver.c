/* A compiled (plain C99) host of the pending points of an infill handle: an objective model and a constraint model on a small
 * synthetic set (egx_gp_create + egx_gp_finalize, default configuration), then
 *   - egx_infill_optimize_batch (q = 3, SLSQP, Kriging believer) against the loop a caller writes with
 *     egx_infill_optimize_slsqp -> egx_infill_virtual_point -> egx_infill_push_pending on a second handle: the same bits;
 *   - egx_infill_get_pending returns what was pushed; the conditioned sigma2 shrinks by n / (n + q) under the believer;
 *   - egx_infill_clear_pending gives back the values of a handle that never held a point, bit for bit;
 *   - a 17th point and a NaN coordinate are EGX_ERR_INVALID_VALUE.
 * What a Rust `extern "C"` shim at the q_points loop of solver_impl.rs:622-791 would call.
 * Prints PASS and exits 0 when all holds. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "egx_gp.h"

#define N 90
#define D 2
#define Q 3
#define NS 5

#define CHECK(call)                                                          \
    do {                                                                     \
        int32_t rc_ = (call);                                                \
        if (rc_ != EGX_SUCCESS) {                                            \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, egx_last_error()); \
            return 10 + rc_;                                                 \
        }                                                                    \
    } while (0)

static double frac(double v) { return v - floor(v); }

int main(void) {
    if (egx_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 2;
    }
    static double x[N * D], y[N], c[N];
    for (int i = 0; i < N; i++) {  /* a low-discrepancy set in the unit square */
        x[i * D] = frac(0.5 + 0.7548776662466927 * (i + 1));
        x[i * D + 1] = frac(0.5 + 0.5698402909980532 * (i + 1));
        y[i] = sin(5.0 * x[i * D]) + (x[i * D + 1] - 0.4) * (x[i * D + 1] - 0.4);
        c[i] = x[i * D] + x[i * D + 1] - 1.2;
    }
    const double theta[D] = {1.5, 1.5}, lo[D] = {0.0, 0.0}, hi[D] = {1.0, 1.0}, tols[1] = {0.0};
    egx_gp_config cfg;
    egx_gp_config_default(&cfg);
    egx_gp *obj = NULL, *cstr = NULL, *cstrs[1];
    CHECK(egx_gp_create(&cfg, x, y, N, D, &obj));
    CHECK(egx_gp_create(&cfg, x, c, N, D, &cstr));
    CHECK(egx_gp_finalize(obj, theta, D));
    CHECK(egx_gp_finalize(cstr, theta, D));
    cstrs[0] = cstr;
    egx_infill_config ic;
    egx_infill_config_default(&ic);
    ic.fmin = -0.9;
    egx_infill *a = NULL, *b = NULL;
    CHECK(egx_infill_create(&ic, obj, cstrs, tols, 1, &a));
    CHECK(egx_infill_create(&ic, obj, cstrs, tols, 1, &b));

    double starts[Q * NS * D], probe[4 * D], v0[4], v1[4];
    for (int i = 0; i < Q * NS * D; i++) starts[i] = frac(0.31 + 0.6180339887498949 * (i + 1));
    for (int i = 0; i < 4 * D; i++) probe[i] = frac(0.17 + 0.4142135623730951 * (i + 1));
    CHECK(egx_infill_eval(a, probe, 4, v0, NULL, NULL));

    egx_infill_batch_config bc;
    egx_infill_batch_config_default(&bc);
    if (bc.strategy != EGX_QEI_KB || bc.optimizer != EGX_BATCH_SLSQP) return 3;
    double xo[Q * D], yv[Q * 2], fo[Q], s2_0[2], s2_q[2];
    int32_t nf = -1, q = -1;
    CHECK(egx_infill_get_pending(a, &q, NULL, NULL, s2_0));
    if (q != 0) return 3;
    CHECK(egx_infill_optimize_batch(a, &bc, lo, hi, starts, NS, Q, xo, yv, fo, &nf));
    if (nf != Q) return 4;
    for (int i = 0; i < Q; i++) {  /* the loop a caller writes */
        double f = 0.0, xb[D], cb[1], yy[2];
        CHECK(egx_infill_optimize_slsqp(b, lo, hi, starts + i * NS * D, NS, 0, &f, xb, cb, NULL));
        CHECK(egx_infill_virtual_point(b, xb, EGX_QEI_KB, yy));
        CHECK(egx_infill_push_pending(b, xb, yy));
        if (memcmp(xb, xo + i * D, sizeof xb) || memcmp(yy, yv + i * 2, sizeof yy) || memcmp(&f, fo + i, sizeof f)) {
            fprintf(stderr, "step %d: the batch call and the manual loop differ\n", i);
            return 5;
        }
    }
    double px[EGX_INFILL_MAX_PENDING * D], py[EGX_INFILL_MAX_PENDING * 2];
    CHECK(egx_infill_get_pending(a, &q, px, py, s2_q));
    if (q != Q || memcmp(px, xo, sizeof xo) || memcmp(py, yv, sizeof yv)) return 6;
    for (int j = 0; j < 2; j++)  /* the believer adds no residual: rho^T rho / (n + q) */
        if (fabs(s2_q[j] - s2_0[j] * N / (N + Q)) > 1e-9 * s2_0[j]) return 6;
    CHECK(egx_infill_eval(a, probe, 4, v1, NULL, NULL));
    if (!memcmp(v0, v1, sizeof v0)) return 7;  /* conditioned: the criterion moved */

    double bad[D] = {0.5, NAN}, zero[2] = {0.0, 0.0};
    if (egx_infill_push_pending(a, bad, zero) != EGX_ERR_INVALID_VALUE) return 8;
    for (int i = Q; i < EGX_INFILL_MAX_PENDING; i++) {
        double p[D], yy[2];
        p[0] = frac(0.05 + 0.6180339887498949 * (i + 1)), p[1] = frac(0.95 + 0.7548776662466927 * (i + 1));
        CHECK(egx_infill_virtual_point(a, p, EGX_QEI_KB_UB, yy));
        CHECK(egx_infill_push_pending(a, p, yy));
    }
    bad[1] = 0.123;
    if (egx_infill_push_pending(a, bad, zero) != EGX_ERR_INVALID_VALUE) return 8;
    CHECK(egx_infill_get_pending(a, &q, NULL, NULL, NULL));
    if (q != EGX_INFILL_MAX_PENDING) return 8;

    CHECK(egx_infill_clear_pending(a));
    CHECK(egx_infill_eval(a, probe, 4, v1, NULL, NULL));
    if (memcmp(v0, v1, sizeof v0)) return 9;  /* bit for bit the handle that never held a point */
    CHECK(egx_infill_virtual_point(a, NULL, EGX_QEI_CL_MIN, zero));
    int imin = 0;
    for (int i = 1; i < N; i++)
        if (y[i] < y[imin]) imin = i;
    if (zero[0] != y[imin] || zero[1] != c[imin]) return 9;

    printf("PASS q %d f", (int)nf);
    for (int i = 0; i < Q; i++) printf(" %a", fo[i]);
    printf("\n");
    egx_infill_destroy(a);
    egx_infill_destroy(b);
    egx_gp_destroy(obj);
    egx_gp_destroy(cstr);
    return 0;
}
