// A C++ host of the lock-step theta-gradient and L-BFGS fit of a group (include/egx_gp.hpp: egobox::likelihood_grad_group,
// egobox::fit_lbfgs_group over egx_gp_likelihood_grad_multi / egx_gp_fit_lbfgs_multi): k = 4 models of one shape (n = 90, d = 2,
// Matern-5/2) from GpParams::fit_group, every row and every fitted model compared BIT FOR BIT with the lone calls of the C ABI
// (egx_gp_likelihood_grad on the member itself; egx_gp_fit_lbfgs on a one-workspace handle of the member's training set).
// Exit status 0: equal bits.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "egx_gp.hpp"

static int failures = 0;
#define EXPECT(cond, ...)             \
    do {                              \
        if (!(cond)) {                \
            failures++;               \
            std::printf("FAIL: ");    \
            std::printf(__VA_ARGS__); \
            std::printf("\n");        \
        }                             \
    } while (0)

static bool same_bits(const double *a, const double *b, size_t n) { return std::memcmp(a, b, sizeof(double) * n) == 0; }

int main() {
    using namespace egobox;
    const int32_t k = 4;
    const int64_t n = 90, d = 2, m = 19, n_starts = 3;
    // k training sets: a fixed linear congruential stream, a smooth response with a member-dependent phase
    std::vector<double> x((size_t)(k * n * d)), y((size_t)(k * n)), xq((size_t)(m * d));
    uint64_t s = 12345;
    auto u01 = [&]() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) / 9007199254740992.0;
    };
    for (int32_t j = 0; j < k; j++)
        for (int64_t i = 0; i < n; i++) {
            double *row = &x[(size_t)((j * n + i) * d)];
            row[0] = u01(), row[1] = u01();
            y[(size_t)(j * n + i)] = std::sin(5.0 * row[0] + 0.3 * j) + std::cos(3.0 * row[1]) * row[0];
        }
    for (double &v : xq) v = u01();
    try {
        std::vector<GaussianProcess> gps = GaussianProcess::params(Mean::Constant, Corr::Matern52)
                                               .theta_tuning(ThetaTuning::Fixed({2.0}))
                                               .fit_group(x.data(), y.data(), n, d, k);
        std::vector<GaussianProcess *> models;
        for (GaussianProcess &g : gps) models.push_back(&g);

        // ---- likelihood + gradient: the lone calls first (both un-fit), then the group
        std::vector<double> thetas((size_t)(k * d));
        for (int32_t j = 0; j < k; j++)
            for (int64_t l = 0; l < d; l++) thetas[(size_t)(j * d + l)] = 2.0 * (1.0 + 0.1 * j) + 0.05 * (double)l;
        std::vector<double> lk1((size_t)k), g1((size_t)(k * d));
        std::vector<int32_t> st1((size_t)k);
        for (int32_t j = 0; j < k; j++)
            check(egx_gp_likelihood_grad(gps[(size_t)j].handle(), &thetas[(size_t)(j * d)], d, &lk1[(size_t)j], &g1[(size_t)(j * d)],
                                         &st1[(size_t)j]));
        const GaussianProcess::LikelihoodGrad r = likelihood_grad_group(models, thetas.data(), d);
        EXPECT(r.likelihood.size() == (size_t)k && r.gradient.size() == (size_t)(k * d) && r.status.size() == (size_t)k, "output sizes");
        for (int32_t j = 0; j < k; j++) {
            EXPECT(r.status[(size_t)j] == st1[(size_t)j] && st1[(size_t)j] == EGX_STATUS_OK, "status of member %d", j);
            EXPECT(same_bits(&r.likelihood[(size_t)j], &lk1[(size_t)j], 1), "likelihood of member %d: %.17g vs %.17g", j,
                   r.likelihood[(size_t)j], lk1[(size_t)j]);
            EXPECT(same_bits(&r.gradient[(size_t)(j * d)], &g1[(size_t)(j * d)], (size_t)d), "gradient of member %d", j);
            EXPECT(std::isfinite(r.gradient[(size_t)(j * d)]) && r.gradient[(size_t)(j * d)] != 0.0, "gradient of member %d is set", j);
        }
        bool threw = false;  // the call un-fitted the models
        try {
            (void)gps[0].predict(xq.data(), m);
        } catch (const std::exception &) {
            threw = true;
        }
        EXPECT(threw, "a member still predicts after likelihood_grad_group");

        // ---- the fit: the same three starts for every member, against egx_gp_fit_lbfgs on one-workspace handles
        const double starts[] = {0.3, 0.3, 2.0, 0.5, 0.05, 4.0}, lo = 1e-3, hi = 50.0;
        std::vector<double> theta0s;
        for (int32_t j = 0; j < k; j++) theta0s.insert(theta0s.end(), starts, starts + n_starts * d);
        const std::vector<int64_t> ne = fit_lbfgs_group(models, theta0s.data(), n_starts, &lo, &hi, 1, 30);
        for (int32_t j = 0; j < k; j++) {
            egx_gp_config cfg;
            egx_gp_config_default(&cfg);
            cfg.corr = EGX_CORR_MATERN52;
            cfg.n_workspaces = 1;
            egx_gp *one = nullptr;
            check(egx_gp_create(&cfg, &x[(size_t)(j * n * d)], &y[(size_t)(j * n)], n, d, &one));
            int64_t ne1 = 0;
            check(egx_gp_fit_lbfgs(one, starts, n_starts, &lo, &hi, 1, 30, &ne1));
            std::vector<double> th1((size_t)d), y1((size_t)m), v1((size_t)m);
            double lkh1 = 0.0, s21 = 0.0;
            egx_gp_inner_view view{};
            view.theta = th1.data(), view.likelihood = &lkh1, view.sigma2 = &s21;
            check(egx_gp_get_inner(one, &view));
            check(egx_gp_predict_valvar(one, xq.data(), m, y1.data(), v1.data()));
            egx_gp_destroy(one);
            const GaussianProcess &g = gps[(size_t)j];
            EXPECT(ne[(size_t)j] == ne1 && g.n_evals() == ne1, "evaluations of member %d: %lld vs %lld", j, (long long)ne[(size_t)j],
                   (long long)ne1);
            EXPECT(same_bits(g.theta().data(), th1.data(), (size_t)d), "theta* of member %d", j);
            const double lkg = g.likelihood(), s2g = g.variance();
            EXPECT(same_bits(&lkg, &lkh1, 1) && same_bits(&s2g, &s21, 1), "likelihood / variance of member %d", j);
            const auto yv = g.predict_valvar(xq.data(), m);
            EXPECT(same_bits(yv.first.data(), y1.data(), (size_t)m) && same_bits(yv.second.data(), v1.data(), (size_t)m),
                   "predictions of member %d", j);
        }
    } catch (const std::exception &e) {
        std::printf("FAIL: exception: %s\n", e.what());
        return 2;
    }
    if (failures == 0) std::printf("OK grad_multi_host: %d members, rows and fits equal the lone calls bit for bit\n", (int)k);
    return failures == 0 ? 0 : 1;
}
