// A compiled host of the constraint-strategy entry points, through the C ABI and through the C++ mirror: an objective model and
// a constraint model, egx_infill_set_cstr_strategy / _get_cstr_strategy, egx_infill_eval_cstr, egx_infill_optimize_cstr, then
// the same four on egobox::InfillObjective.  Checks only what needs no second implementation: the value equals
// egx_infill_eval's in this mode bit for bit, a point alone equals the point in the batch, the constraint gradient matches a
// central difference, the optimiser's result is inside the box and re-evaluates to itself, and the mirror returns the C
// ABI's bits.  What a Rust `extern "C"` shim at the solver_infill_optim.rs:148-204 seam would call.
// Exit code 0 = all good.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "egx_gp.hpp"

#define CHECK(call)                                                          \
    do {                                                                     \
        int32_t rc_ = (call);                                                \
        if (rc_ != EGX_SUCCESS) {                                            \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, egx_last_error()); \
            return 10 + rc_;                                                 \
        }                                                                    \
    } while (0)

enum { N = 120, D = 2, M = 21, NS = 3 };

static unsigned long long rng_state = 88172645463325252ULL;
static double urand() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

int main() {
    if (egx_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 2;
    }
    static double x[N * D], y[N], c[N], xq[M * D];
    double fmin = 1e300;
    for (int i = 0; i < N; i++) {
        x[i * D] = urand();
        x[i * D + 1] = urand();
        y[i] = std::sin(5.0 * x[i * D]) + x[i * D + 1] * x[i * D + 1];
        c[i] = x[i * D] + x[i * D + 1] - 1.2;  // feasible where c <= 0
        if (y[i] < fmin) fmin = y[i];
    }
    for (int i = 0; i < M * D; i++) xq[i] = urand();
    using namespace egobox;
    auto obj = Kriging::params().theta_tuning(ThetaTuning::Fixed({1.5, 1.1})).fit(x, N, D, y);
    auto cst = Kriging::params().theta_tuning(ThetaTuning::Fixed({1.5, 1.1})).fit(x, N, D, c);

    // ---- the C ABI
    egx_infill_config ic;
    egx_infill_config_default(&ic);
    ic.criterion = EGX_INFILL_WB2;
    ic.fmin = fmin;
    egx_infill *h = nullptr;
    egx_gp *cstrs[1] = {cst.handle()};
    const double tols[1] = {0.0}, scale_in[1] = {2.0};
    CHECK(egx_infill_create(&ic, obj.handle(), cstrs, tols, 1, &h));
    double val[M], cv[M], grad[M * D], gc[M * D], val2[M];
    if (egx_infill_eval_cstr(h, xq, M, val, cv, nullptr, nullptr) != EGX_ERR_INVALID_VALUE) return 3;  // still EGX_CSTR_INFILL
    const double bad[1] = {0.0};
    if (egx_infill_set_cstr_strategy(h, EGX_CSTR_UTB, bad) != EGX_ERR_INVALID_VALUE) return 3;
    CHECK(egx_infill_set_cstr_strategy(h, EGX_CSTR_UTB, scale_in));
    int32_t strat = -1;
    double scale_out[1] = {0.0};
    CHECK(egx_infill_get_cstr_strategy(h, &strat, scale_out));
    if (strat != EGX_CSTR_UTB || scale_out[0] != 2.0) return 4;
    CHECK(egx_infill_eval_cstr(h, xq, M, val, cv, grad, gc));
    CHECK(egx_infill_eval(h, xq, M, val2, nullptr, nullptr));
    if (std::memcmp(val, val2, sizeof val) != 0) {
        fprintf(stderr, "eval_cstr's value differs from egx_infill_eval's\n");
        return 5;
    }
    for (int a = 0; a < M; a += 5) {  // a point alone = the point in the batch
        double v1, c1, g1[D], gc1[D];
        CHECK(egx_infill_eval_cstr(h, xq + a * D, 1, &v1, &c1, g1, gc1));
        if (std::memcmp(&v1, &val[a], sizeof v1) || std::memcmp(&c1, &cv[a], sizeof c1) || std::memcmp(g1, &grad[a * D], sizeof g1) ||
            std::memcmp(gc1, &gc[a * D], sizeof gc1)) {
            fprintf(stderr, "point %d alone differs from the batch\n", a);
            return 6;
        }
    }
    for (int k = 0; k < D; k++) {  // central difference of the constraint at point 0
        const double e = 1e-5;
        double xp[2 * D], vp[2], cp[2];
        std::memcpy(xp, xq, sizeof(double) * D);
        std::memcpy(xp + D, xq, sizeof(double) * D);
        xp[k] += e;
        xp[D + k] -= e;
        CHECK(egx_infill_eval_cstr(h, xp, 2, vp, cp, nullptr, nullptr));
        const double fd = (cp[0] - cp[1]) / (2.0 * e);
        if (std::fabs(fd - gc[k]) > 1e-5 * (1.0 + std::fabs(fd))) {
            fprintf(stderr, "constraint gradient %d: %.12g against the difference quotient %.12g\n", k, gc[k], fd);
            return 7;
        }
    }
    CHECK(egx_infill_eval_cstr(h, xq, 0, nullptr, nullptr, nullptr, nullptr));
    CHECK(egx_infill_set_cstr_strategy(h, EGX_CSTR_MEAN, nullptr));  // the scales stay
    const double lo[D] = {0.0, 0.0}, hi[D] = {1.0, 1.0};
    double starts[NS * D], f_best, x_best[D], c_best[1], f_again, c_again;
    int64_t evals[NS];
    for (int i = 0; i < NS * D; i++) starts[i] = urand();
    egx_infill_cstr_stats st;
    st.evals = evals;
    CHECK(egx_infill_optimize_cstr(h, lo, hi, starts, NS, 0, &f_best, x_best, c_best, &st));
    CHECK(egx_infill_eval_cstr(h, x_best, 1, &f_again, &c_again, nullptr, nullptr));
    if (std::memcmp(&f_again, &f_best, sizeof f_best) || std::memcmp(&c_again, c_best, sizeof c_again)) {
        fprintf(stderr, "optimize_cstr: (%.17g, %.17g) re-evaluates to (%.17g, %.17g)\n", f_best, c_best[0], f_again, c_again);
        return 8;
    }
    for (int k = 0; k < D; k++)
        if (x_best[k] < lo[k] || x_best[k] > hi[k]) return 9;
    for (int s = 0; s < NS; s++)
        if (evals[s] < 1 || evals[s] > 10 * NS * D) return 9;
    if (st.best_start < 0 || st.best_start >= NS || st.rounds < 1) return 9;
    if (st.feasible != (c_best[0] <= 0.0 ? 1 : 0) || st.violation != c_best[0]) return 9;
    egx_infill_destroy(h);

    // ---- the C++ mirror returns the same bits
    try {
        InfillObjective o(obj, {&cst}, {0.0}, EGX_INFILL_WB2, fmin);
        o.set_cstr_strategy(EGX_CSTR_UTB, {2.0});
        const auto got = o.cstr_strategy();
        if (got.first != EGX_CSTR_UTB || got.second.size() != 1 || got.second[0] != 2.0) return 20;
        const auto r = o.constraints(xq, M, true);
        if (std::memcmp(r.value.data(), val, sizeof val) || std::memcmp(r.cstr.data(), cv, sizeof cv) ||
            std::memcmp(r.grad.data(), grad, sizeof grad) || std::memcmp(r.grad_cstr.data(), gc, sizeof gc)) {
            fprintf(stderr, "the C++ mirror's constraints() differs from the C ABI\n");
            return 21;
        }
        o.set_cstr_strategy(EGX_CSTR_MEAN);
        const auto opt = o.optimize_constrained(lo, hi, starts, NS);
        if (std::memcmp(&opt.f, &f_best, sizeof f_best) || std::memcmp(opt.x.data(), x_best, sizeof x_best) ||
            std::memcmp(opt.c.data(), c_best, sizeof c_best) || opt.best_start != st.best_start || opt.rounds != st.rounds ||
            opt.feasible != (st.feasible != 0) || !opt.finite) {
            fprintf(stderr, "the C++ mirror's optimize_constrained() differs from the C ABI\n");
            return 22;
        }
    } catch (const GpError &e) {
        fprintf(stderr, "C++ mirror: %s\n", e.what());
        return 23;
    }
    printf("OK f_best %.9g c_best %.6g at (%.6f, %.6f) feasible %d rounds %lld\n", f_best, c_best[0], x_best[0], x_best[1],
           (int)st.feasible, (long long)st.rounds);
    return 0;
}
