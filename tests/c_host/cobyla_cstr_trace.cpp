// Host-only harness for egx::Cobyla (csrc/cobyla.h, no HIP): runs one analytic test problem with nonlinear constraints and
// prints every point the optimiser asks for with f and the constraint values there, then two summary lines.
// tests/test_cobyla_cstr_cpu.py compares the sequences with Powell's own Fortran COBYLA as shipped in scipy (< 1.16), which is
// given the same constraints in the class's order: the nonlinear ones, then the bounds (lo_0, hi_0, lo_1, ...) in the
// rescaled units the class states them in.
//   cobyla_cstr_trace <case 0..3 = A..D> <rhobeg> <rhoend> <maxeval> <mode>
//       mode 0 = Powell (no clamping, no rho doubling, ftol off)
//       mode 1 = as egx_infill_optimize_cstr configures it (clamped evaluation, rho doubling, ftol_rel = ftol_abs = 1e-4)
//   cobyla_cstr_trace 9 <rhobeg> <rhoend> <maxeval> <mode> <n> <m> x0.. lo.. hi.. [cfeas..]
//       an EXTERNAL problem: after every printed point the program reads "f c_0 .. c_{m-1}" from standard input (the
//       caller evaluates; used to run the class over the oracle's restatement of GP surrogates)
// Constraints are in the class's convention, c(x) <= 0 feasible.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>

#include "../../egobox_amd/csrc/cobyla.h"
using namespace egx;

typedef std::vector<double> vec;

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const int cs = atoi(argv[1]), maxeval = atoi(argv[4]), mode = atoi(argv[5]);
    const double rhobeg = atof(argv[2]), rhoend = atof(argv[3]);
    std::function<double(const vec &)> f;
    std::function<void(const vec &, double *)> c;
    vec x0, lo, hi, cfeas;
    int m = 0;
    bool external = false;
    if (cs == 0) {  // A: the unit disc cuts off the unconstrained optimum
        f = [](const vec &x) { return (x[0] - 1.2) * (x[0] - 1.2) + (x[1] - 0.9) * (x[1] - 0.9); };
        c = [](const vec &x, double *o) { o[0] = -(1.0 - x[0] * x[0] - x[1] * x[1]); };
        m = 1, x0 = {0.1, 0.2}, lo = {-2, -2}, hi = {2, 2};
    } else if (cs == 1) {  // B: one active, one inactive constraint
        f = [](const vec &x) { return x[0] + x[1] + 0.1 * std::sin(3 * x[0]); };
        c = [](const vec &x, double *o) {
            o[0] = -(x[0] * x[1] - 0.25);
            o[1] = -(1.5 - x[0] - 0.5 * x[1] * x[1]);
        };
        m = 2, x0 = {1, 1}, lo = {0, 0}, hi = {2, 2};
    } else if (cs == 2) {  // C: four variables, three constraints
        f = [](const vec &x) {
            double s = 0;
            for (int i = 0; i < 4; i++) s += (i + 1) * (x[i] - 0.3 * i + 0.5) * (x[i] - 0.3 * i + 0.5);
            return s;
        };
        c = [](const vec &x, double *o) {
            double ss = 0, s = 0;
            for (int i = 0; i < 4; i++) ss += x[i] * x[i], s += x[i];
            o[0] = -(0.5 - ss);
            o[1] = -(s + 0.2);
            o[2] = -(std::cos(x[1]) - 0.8 - x[3]);
        };
        m = 3, x0 = {0.1, 0.1, 0.1, 0.1}, lo = {-2, -2, -2, -2}, hi = {2, 2, 2, 2};
    } else if (cs == 3) {  // D: the upper bound of x0 is active beside the nonlinear constraint
        f = [](const vec &x) { return -x[0] * x[1] * x[2]; };
        c = [](const vec &x, double *o) { o[0] = -(1.0 - x[0] * x[0] - 2 * x[1] * x[1] - 3 * x[2] * x[2]); };
        m = 1, x0 = {0.3, 0.3, 0.3}, lo = {0, 0, 0}, hi = {0.45, 1, 1};
    } else if (cs == 9) {
        if (argc < 8) return 2;
        const int n = atoi(argv[6]);
        m = atoi(argv[7]);
        if (n < 1 || m < 0 || argc < 8 + 3 * n) return 2;
        for (int i = 0; i < n; i++) {
            x0.push_back(atof(argv[8 + i]));
            lo.push_back(atof(argv[8 + n + i]));
            hi.push_back(atof(argv[8 + 2 * n + i]));
        }
        for (int j = 0; j < m && 8 + 3 * n + j < argc; j++) cfeas.push_back(atof(argv[8 + 3 * n + j]));
        external = true;
    } else {
        return 2;
    }
    Cobyla opt(x0, lo, hi, m, rhobeg, mode ? 1e-4 : 0.0, mode ? 1e-4 : 0.0, maxeval, rhoend / rhobeg, mode != 0, mode != 0, cfeas);
    vec x, cv((size_t)m + 1, 0.0);
    while (opt.ask(x)) {
        double v = 0.0;
        for (double t : x) printf("%.17g ", t);
        if (external) {
            printf("\n");
            fflush(stdout);
            if (scanf("%lf", &v) != 1) return 3;
            for (int j = 0; j < m; j++)
                if (scanf("%lf", &cv[j]) != 1) return 3;
        } else {
            v = f(x);
            c(x, cv.data());
            printf("%.17g", v);
            for (int j = 0; j < m; j++) printf(" %.17g", cv[j]);
            printf("\n");
        }
        opt.tell(v, cv.data());
    }
    printf("# final status %d evals %ld f %.17g x", (int)opt.status(), (long)opt.evals(), opt.final_f());
    for (double t : opt.final_x()) printf(" %.17g", t);
    printf(" c");
    for (double t : opt.final_c()) printf(" %.17g", t);
    printf("\n# best feasible %d violation %.17g f %.17g x", opt.best_feasible() ? 1 : 0, opt.best_violation(), opt.best_f());
    for (double t : opt.best_x()) printf(" %.17g", t);
    printf(" c");
    for (double t : opt.best_c()) printf(" %.17g", t);
    printf("\n");
    return 0;
}
