// The q_points loop of the reference's solver (crates/ego/src/solver/solver_impl.rs:622-791) in C++ through include/egx_gp.hpp:
// InfillObjective::optimize_batch against the loop optimize_slsqp -> virtual_point -> push_pending on a second object, the
// believer's sigma2 recursion through n_pending / egx_infill_get_pending, clear_pending.  Prints OK and exits 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "egx_gp.hpp"

using namespace egobox;

static double frac(double v) { return v - std::floor(v); }

#define REQUIRE(cond)                                                    \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
            return 1;                                                    \
        }                                                                \
    } while (0)

int main() {
    if (egx_device_count() < 1) {
        std::fprintf(stderr, "no HIP device\n");
        return 2;
    }
    const int n = 80, d = 2, q = 3, ns = 4;
    std::vector<double> x((size_t)n * d), y(n), c(n);
    for (int i = 0; i < n; i++) {
        x[(size_t)i * d] = frac(0.5 + 0.7548776662466927 * (i + 1));
        x[(size_t)i * d + 1] = frac(0.5 + 0.5698402909980532 * (i + 1));
        y[i] = std::cos(4.0 * x[(size_t)i * d]) + x[(size_t)i * d + 1] * x[(size_t)i * d + 1];
        c[i] = x[(size_t)i * d] - x[(size_t)i * d + 1] - 0.3;
    }
    auto obj = Kriging::params().theta_tuning(ThetaTuning::Fixed({1.5, 1.5})).fit(x.data(), n, d, y.data());
    auto cst = GaussianProcess::params(Mean::Linear, Corr::Matern52).theta_tuning(ThetaTuning::Fixed({1.2, 1.2})).fit(x.data(), n, d, c.data());
    InfillObjective a(obj, {&cst}, {0.0}, EGX_INFILL_LOG_EI, -0.5), b(obj, {&cst}, {0.0}, EGX_INFILL_LOG_EI, -0.5);
    const double lo[2] = {0.0, 0.0}, hi[2] = {1.0, 1.0};
    std::vector<double> starts((size_t)q * ns * d);
    for (size_t i = 0; i < starts.size(); i++) starts[i] = frac(0.29 + 0.6180339887498949 * (double)(i + 1));

    auto batch = a.optimize_batch(lo, hi, starts.data(), ns, q, QEiStrategy::KrigingBeliever);
    REQUIRE(batch.n_found == q && a.n_pending() == q);
    REQUIRE(batch.x.size() == (size_t)q * d && batch.y_virtual.size() == (size_t)q * 2 && batch.f.size() == (size_t)q);
    for (int i = 0; i < q; i++) {
        auto o = b.optimize_slsqp(lo, hi, starts.data() + (size_t)i * ns * d, ns);
        auto yv = b.virtual_point(o.x.data(), QEiStrategy::KrigingBeliever);
        b.push_pending(o.x.data(), yv.data());
        REQUIRE(std::memcmp(o.x.data(), batch.x.data() + (size_t)i * d, sizeof(double) * d) == 0);
        REQUIRE(std::memcmp(yv.data(), batch.y_virtual.data() + (size_t)i * 2, sizeof(double) * 2) == 0);
        REQUIRE(std::memcmp(&o.f, &batch.f[(size_t)i], sizeof(double)) == 0);
    }
    const double probe[2] = {0.37, 0.61};
    const double v_pending = a.value(probe, 1)[0];
    a.clear_pending();
    b.clear_pending();
    REQUIRE(a.n_pending() == 0);
    InfillObjective never(obj, {&cst}, {0.0}, EGX_INFILL_LOG_EI, -0.5);
    const double v_clear = a.value(probe, 1)[0], v_never = never.value(probe, 1)[0];
    REQUIRE(std::memcmp(&v_clear, &v_never, sizeof(double)) == 0);
    REQUIRE(v_pending != v_never);
    // the constant liar: the row of the smallest objective value
    int imin = 0;
    for (int i = 1; i < n; i++)
        if (y[i] < y[imin]) imin = i;
    auto liar = a.virtual_point(probe, QEiStrategy::ConstantLiarMinimum);
    REQUIRE(liar[0] == y[imin] && liar[1] == c[imin]);
    try {  // a non-finite coordinate is GpError::InvalidValueError
        const double bad[2] = {0.5, NAN}, zero[2] = {0.0, 0.0};
        a.push_pending(bad, zero);
        return 3;
    } catch (const InvalidValueError &) {
    }
    std::printf("OK batch of %d: f %.6g %.6g %.6g\n", q, batch.f[0], batch.f[1], batch.f[2]);
    return 0;
}
