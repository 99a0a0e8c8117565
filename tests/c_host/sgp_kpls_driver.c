/* A plain C99 host of the sparse GP with KPLS weights: egx_sgp_create -> egx_sgp_set_w_star -> egx_sgp_finalize ->
 * egx_sgp_likelihood_grad (h + 2 long; it un-fits the handle, so a second finalize follows) -> egx_sgp_predict_valvar_gradients,
 * on data made of small dyadic fractions that tests/test_gpu_sgp_kpls.py rebuilds exactly.  It prints the values; the test
 * compares them with the Python calls.  Exit code 0 = every call went as the header says, 77 = no HIP device. */
#include <stdio.h>
#include <stdlib.h>

#include "egx_gp.h"

#define N 40
#define D 4
#define H 2
#define NZ 8
#define M 3

#define CHECK(call)                                                          \
    do {                                                                     \
        int32_t rc_ = (call);                                                \
        if (rc_ != EGX_SUCCESS) {                                            \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, egx_last_error()); \
            return 10 + rc_;                                                 \
        }                                                                    \
    } while (0)

int main(void) {
    double x[N * D], y[N], w[D * H], xq[M * D];
    for (int i = 0; i < N; i++) {
        for (int k = 0; k < D; k++) x[i * D + k] = ((7 * i + 13 * k) % 32) / 16.0 - 1.0;
        y[i] = ((5 * i) % 17) / 8.0 - 1.0 + 0.25 * x[i * D];
    }
    for (int k = 0; k < D; k++)
        for (int l = 0; l < H; l++) w[k * H + l] = ((3 * k + 5 * l) % 7 - 3) / 8.0;
    for (int a = 0; a < M; a++)
        for (int k = 0; k < D; k++) xq[a * D + k] = ((11 * a + 5 * k) % 16) / 8.0 - 0.9375;
    const double theta[H] = {0.75, 1.25}, sigma2 = 0.5, noise = 0.03125;
    if (egx_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 77;
    }
    egx_sgp_config cfg;
    egx_sgp_config_default(&cfg);
    cfg.corr = EGX_CORR_MATERN52;
    egx_sgp *sgp = NULL;
    CHECK(egx_sgp_create(&cfg, x, y, N, D, x, NZ, &sgp)); /* the first NZ rows are the inducing points */
    int64_t h = 0;
    CHECK(egx_sgp_get_w_star(sgp, NULL, &h));
    int ok = h == D;
    ok &= egx_sgp_set_w_star(sgp, w, D + 1) == EGX_ERR_INVALID_VALUE;
    ok &= egx_sgp_set_w_star(sgp, w, 0) == EGX_ERR_INVALID_VALUE;
    CHECK(egx_sgp_set_w_star(sgp, w, H));
    double wb[D * H];
    CHECK(egx_sgp_get_w_star(sgp, wb, &h));
    ok &= h == H;
    for (int e = 0; e < D * H; e++) ok &= wb[e] == w[e];
    ok &= egx_sgp_finalize(sgp, theta, D, sigma2, noise) == EGX_ERR_INVALID_VALUE; /* theta_len is 1 or h now */
    CHECK(egx_sgp_finalize(sgp, theta, H, sigma2, noise));
    double lkh = 0.0, grad[H + 2], gy[M * D], gv[M * D], ym[M], vm[M];
    int32_t status = -1;
    CHECK(egx_sgp_likelihood_grad(sgp, theta, H, sigma2, noise, &lkh, grad, &status));
    ok &= status == 0;
    ok &= egx_sgp_predict_valvar(sgp, xq, M, ym, vm) == EGX_ERR_NOT_FITTED;
    CHECK(egx_sgp_finalize(sgp, theta, H, sigma2, noise));
    CHECK(egx_sgp_predict_valvar(sgp, xq, M, ym, vm));
    CHECK(egx_sgp_predict_valvar_gradients(sgp, xq, M, gy, gv));
    egx_sgp_destroy(sgp);
    printf("%s\n", ok ? "OK" : "FAILED");
    printf("lkh %.17g\n", lkh);
    printf("grad");
    for (int e = 0; e < H + 2; e++) printf(" %.17g", grad[e]);
    printf("\nmean");
    for (int e = 0; e < M; e++) printf(" %.17g", ym[e]);
    printf("\nvar");
    for (int e = 0; e < M; e++) printf(" %.17g", vm[e]);
    printf("\ngy");
    for (int e = 0; e < M * D; e++) printf(" %.17g", gy[e]);
    printf("\ngv");
    for (int e = 0; e < M * D; e++) printf(" %.17g", gv[e]);
    printf("\n");
    return ok ? 0 : 1;
}
