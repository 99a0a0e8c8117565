// Host build of egobox_amd/csrc/pending_math.h (g++, no GPU) for tests/test_pending_cpu.py.  One case per input line:
//   P q n sigma2 y_std  S[q*q]  delta[q]  c[q]  mean var  x_std gmean gvar  dc[q]
// S is bordered row by row with chol_border; then alpha, sigma2', and one point's finish arithmetic from its cross-covariances c
// and the derivatives dc of those along one coordinate.  Output line:
//   L[q*q] alpha[q] sigma2c mean' var' gmean' gvar'          or   FAIL <row>   when a pivot is not positive
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "pending_math.h"

using namespace egx::pending;

int main() {
    std::string tag;
    while (std::cin >> tag) {
        if (tag != "P") return 2;
        int q, n;
        double sigma2, y_std;
        std::cin >> q >> n >> sigma2 >> y_std;
        if (q < 1 || q > kMaxPending) return 3;
        std::vector<double> S((size_t)q * q), delta(q), c(q), dc(q);
        for (double &v : S) std::cin >> v;
        for (double &v : delta) std::cin >> v;
        for (double &v : c) std::cin >> v;
        double mean, var, x_std, gmean, gvar;
        std::cin >> mean >> var >> x_std >> gmean >> gvar;
        for (double &v : dc) std::cin >> v;
        std::vector<double> L((size_t)kLd * kLd, 0.0);
        int failed = -1;
        for (int r = 0; r < q && failed < 0; r++)
            if (!chol_border(L.data(), r, S.data() + (size_t)r * q, S[(size_t)r * q + r])) failed = r;
        if (failed >= 0) {
            std::printf("FAIL %d\n", failed);
            continue;
        }
        double alpha[kMaxPending], b[kMaxPending], dm, quad;
        const double dq = solve_alpha(L.data(), q, delta.data(), alpha);
        const double s2c = sigma2_conditioned(sigma2, y_std, n, q, dq);
        point_terms(L.data(), alpha, q, c.data(), &dm, &quad, b);
        double gc = 0.0, gb = 0.0;
        for (int v = 0; v < q; v++) gc += alpha[v] * dc[v], gb += b[v] * dc[v];
        for (int i = 0; i < q; i++)
            for (int j = 0; j < q; j++) std::printf("%.17g ", L[(size_t)i * kLd + j]);
        for (int i = 0; i < q; i++) std::printf("%.17g ", alpha[i]);
        std::printf("%.17g %.17g %.17g %.17g %.17g\n", s2c, cond_mean(mean, y_std, dm), cond_var(var, sigma2, s2c, quad),
                    cond_gmean(gmean, y_std, x_std, gc), cond_gvar(gvar, sigma2, s2c, x_std, gb));
    }
    return 0;
}
