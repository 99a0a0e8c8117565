// KPLS through the C++ builder (include/egx_gp.hpp): GpParams::kpls_dim(2) computes the PLS rotations on the device and fits on
// two components.  Prints "OK", then theta's length, kpls_dim(), the rotations pls_rotations returns and the predictions at three
// points; tests/test_gpu_pls.py compares them with the Python device path on the same data.
#include <cstdio>
#include <vector>

#include "egx_gp.hpp"

int main() {
    const int64_t n = 60, d = 5, m = 3;
    std::vector<double> x((size_t)(n * d)), y((size_t)n), xq((size_t)(m * d));
    for (int64_t i = 0; i < n; i++) {
        for (int64_t k = 0; k < d; k++) x[(size_t)(i * d + k)] = (double)((7 * i + 13 * k + 3 * i * k) % 32) / 16.0 - 1.0;
        y[(size_t)i] = 0.5 * x[(size_t)(i * d)] - 0.25 * x[(size_t)(i * d + 2)] * x[(size_t)(i * d + 1)] + (double)((5 * i) % 17) / 64.0;
    }
    for (int64_t i = 0; i < m; i++)
        for (int64_t k = 0; k < d; k++) xq[(size_t)(i * d + k)] = (double)((11 * i + 5 * k) % 16) / 8.0 - 0.9375;
    try {
        using namespace egobox;
        const std::vector<double> w = pls_rotations(x.data(), y.data(), n, d, 2);
        GaussianProcess gp = GaussianProcess::params(Mean::Constant, Corr::SquaredExponential)
                                 .kpls_dim(2)
                                 .theta_tuning(ThetaTuning::Fixed({0.75}))
                                 .fit(x.data(), n, d, y.data());
        const std::vector<double> yp = gp.predict(xq.data(), m);
        // the caller's own weights: the same model
        GaussianProcess gw = GaussianProcess::params(Mean::Constant, Corr::SquaredExponential)
                                 .w_star(w, 2)
                                 .theta_tuning(ThetaTuning::Fixed({0.75}))
                                 .fit(x.data(), n, d, y.data());
        const std::vector<double> yw = gw.predict(xq.data(), m);
        for (int64_t i = 0; i < m; i++)
            if (yw[(size_t)i] != yp[(size_t)i]) {
                std::printf("FAIL w_star(w, 2) differs from kpls_dim(2) at query %lld\n", (long long)i);
                return 1;
            }
        bool refused = false;
        try {
            GaussianProcess::params(Mean::Constant, Corr::SquaredExponential).kpls_dim(0).theta_tuning(ThetaTuning::Fixed({0.75}))
                .fit(x.data(), n, d, y.data());
        } catch (const InvalidValueError &) {
            refused = true;
        }
        if (!refused) {
            std::printf("FAIL kpls_dim(0) was not refused\n");
            return 1;
        }
        std::printf("OK\n");
        std::printf("theta_len %zu\n", gp.theta().size());
        std::printf("kpls_dim %lld\n", (long long)gp.kpls_dim());
        std::printf("w");
        for (double v : w) std::printf(" %.17g", v);
        std::printf("\npredict");
        for (double v : yp) std::printf(" %.17g", v);
        std::printf("\n");
    } catch (const std::exception &e) {
        std::printf("FAIL %s\n", e.what());
        return 1;
    }
    return 0;
}
