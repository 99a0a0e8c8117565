/* A C99 host trains a Gaussian mixture on wide rows through the C ABI (egx_gmm_fit_wide): 300 rows in 40 dimensions, two
 * clusters of 150 rows around 0 and around (10, -10, 10, -10, ..), two restarts with given starts.  Checks the return code,
 * the statuses, the weights and the means; prints OK.  Compiled and run by tests/test_gpu_gmm_wide.py. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "egx_gp.h"

#define N 300
#define D 40
#define K 2
#define R 2

static double unit(uint64_t *s) { /* a 64-bit LCG's upper bits, in (-0.5, 0.5) */
    *s = *s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(*s >> 11) / 9007199254740992.0 - 0.5;
}

static double data[N * D], init[R * K * D], w[K], mu[K * D], cov[K * D * D], sum[K][D];

int main(void) {
    double lb[R];
    int32_t iters[R], status[R], best = -1;
    uint64_t s = 12345;
    egx_gmm_config cfg;
    int i, j, c, rc;
    for (i = 0; i < N; i++)
        for (j = 0; j < D; j++) {
            data[i * D + j] = (i % K) * (j % 2 ? -10.0 : 10.0) + unit(&s);
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
    cfg.n_clusters = K;
    cfg.n_runs = R;
    /* the narrow entry point refuses this width and says where to go */
    if (egx_gmm_fit(&cfg, data, N, D, init, w, mu, cov, lb, iters, status, &best, NULL, NULL, NULL) != EGX_ERR_INVALID_VALUE) return 1;
    rc = egx_gmm_fit_wide(&cfg, data, N, D, init, w, mu, cov, lb, iters, status, &best, NULL, NULL, NULL);
    if (rc != EGX_SUCCESS) {
        printf("egx_gmm_fit_wide: %d %s\n", rc, egx_last_error());
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
    if (egx_gmm_fit_wide(&cfg, data, N, 129, init, w, mu, cov, lb, iters, status, &best, NULL, NULL, NULL) != EGX_ERR_INVALID_VALUE)
        return 7; /* beyond the limit: an error before anything is read, not a wrong answer */
    printf("OK lower bound %.12g after %d iterations\n", lb[best], (int)iters[best]);
    return 0;
}
