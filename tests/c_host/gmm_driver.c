/* A C99 host trains a Gaussian mixture through the C ABI (egx_gmm_fit): 64 rows in 3 dimensions, two clusters of 32 rows
 * around (0, 0, 0) and (10, -10, 5), two restarts with given starts.  Checks the return code, the statuses, the weights and
 * the means; prints OK.  Compiled and run by tests/test_gpu_gmm.py. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "egx_gp.h"

#define N 64
#define D 3
#define K 2
#define R 2

static double unit(uint64_t *s) { /* a 64-bit LCG's upper bits, in (-0.5, 0.5) */
    *s = *s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(*s >> 11) / 9007199254740992.0 - 0.5;
}

int main(void) {
    static const double centre[K][D] = {{0.0, 0.0, 0.0}, {10.0, -10.0, 5.0}};
    double data[N * D], init[R * K * D], w[K], mu[K * D], cov[K * D * D], lb[R];
    double sum[K][D] = {{0}};
    int32_t iters[R], status[R], best = -1;
    uint64_t s = 12345;
    egx_gmm_config cfg;
    int i, j, c, rc;
    for (i = 0; i < N; i++)
        for (j = 0; j < D; j++) {
            data[i * D + j] = centre[i % K][j] + unit(&s);
            sum[i % K][j] += data[i * D + j];
        }
    /* restart 0 starts from rows 0 and 1 (one of each cluster), restart 1 from rows 3 and 2 (the clusters in the other order) */
    for (j = 0; j < D; j++) {
        init[(0 * K + 0) * D + j] = data[0 * D + j];
        init[(0 * K + 1) * D + j] = data[1 * D + j];
        init[(1 * K + 0) * D + j] = data[3 * D + j];
        init[(1 * K + 1) * D + j] = data[2 * D + j];
    }
    egx_gmm_config_default(&cfg);
    if (cfg.n_runs != 20 || cfg.max_iter != 100 || cfg.device != -1) return 1;
    cfg.n_clusters = K;
    cfg.n_runs = R;
    rc = egx_gmm_fit(&cfg, data, N, D, init, w, mu, cov, lb, iters, status, &best, NULL, NULL, NULL);
    if (rc != EGX_SUCCESS) {
        printf("egx_gmm_fit: %d %s\n", rc, egx_last_error());
        return 2;
    }
    if (best < 0 || best >= R || status[0] != 0 || status[1] != 0 || iters[best] < 1 || !(lb[best] >= lb[1 - best])) {
        printf("best %d status %d %d iters %d %d lb %g %g\n", best, status[0], status[1], iters[0], iters[1], lb[0], lb[1]);
        return 3;
    }
    for (c = 0; c < K; c++) {
        if (fabs(w[c] - 0.5) > 1e-9) return 4;
        for (j = 0; j < D; j++) { /* (restart 1 names the clusters the other way round) */
            if (fabs(mu[c * D + j] - sum[best == 0 ? c : 1 - c][j] / (N / K)) > 1e-9) return 5;
            if (!(cov[(c * D + j) * D + j] > 0.0)) return 6;
        }
    }
    cfg.n_clusters = 17; /* beyond the limit: an error, not a wrong answer */
    if (egx_gmm_fit(&cfg, data, N, D, init, w, mu, cov, lb, iters, status, &best, NULL, NULL, NULL) != EGX_ERR_INVALID_VALUE) return 7;
    printf("OK lower bound %.12g after %d iterations\n", lb[best], (int)iters[best]);
    return 0;
}
