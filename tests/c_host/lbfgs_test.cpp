// csrc/lbfgs.h (the projected L-BFGS ask / tell machine of egx_gp_fit_lbfgs and egx_sgp_fit_lbfgs) compiled for the host and
// driven on a convex quadratic in a box whose minimiser has ONE active bound:
//   f(x) = 1/2 (x - c)^T Q (x - c) - f*,   Q symmetric positive definite,   box [-1, 1]^3,   c_1 = 1.8 outside it
// The constrained minimiser is x_1 = 1 with the free components from the reduced 2 x 2 system (Cramer's rule below), the
// multiplier of the bound has the right sign, and f* is subtracted so that the machine stops on its projected-gradient test.
// g++ -std=c++17 -Wall -Werror -I egobox_amd/csrc tests/c_host/lbfgs_test.cpp
#include <cmath>
#include <cstdio>
#include <vector>

#include "lbfgs.h"

namespace {
const double Q[3][3] = {{200.0, 40.0, 10.0}, {40.0, 120.0, 20.0}, {10.0, 20.0, 80.0}};
const double c[3] = {0.3, 1.8, -0.4};

double quad(const std::vector<double> &x, std::vector<double> &g) {
    double f = 0.0;
    for (int i = 0; i < 3; i++) {
        g[i] = 0.0;
        for (int j = 0; j < 3; j++) g[i] += Q[i][j] * (x[j] - c[j]);
        f += 0.5 * (x[i] - c[i]) * g[i];
    }
    return f;
}
}  // namespace

int main() {
    // the known minimiser: x_1 = 1, Q_FF (x_F - c_F) = -Q_F1 (1 - c_1) for F = {0, 2}
    const double r0 = -Q[0][1] * (1.0 - c[1]), r2 = -Q[2][1] * (1.0 - c[1]);
    const double det = Q[0][0] * Q[2][2] - Q[0][2] * Q[2][0];
    std::vector<double> xs = {c[0] + (r0 * Q[2][2] - Q[0][2] * r2) / det, 1.0, c[2] + (Q[0][0] * r2 - Q[2][0] * r0) / det}, gs(3);
    const double fstar = quad(xs, gs);
    int bad = 0;
    if (!(std::fabs(xs[0]) < 1.0 && std::fabs(xs[2]) < 1.0 && gs[1] < 0.0 && std::fabs(gs[0]) < 1e-12 && std::fabs(gs[2]) < 1e-12)) {
        std::printf("the stated minimiser does not satisfy the KKT conditions\n");
        bad++;
    }
    const std::vector<double> lo(3, -1.0), hi(3, 1.0);
    const double starts[2][3] = {{-0.5, -0.5, 0.5}, {1.0, 1.0, -1.0}};  // interior; a corner with x_1 already on its bound
    for (int s = 0; s < 2; s++) {
        double theta0[3];
        for (int i = 0; i < 3; i++) theta0[i] = std::pow(10.0, starts[s][i]);
        egx::LbfgsStart m(theta0, 3, lo, hi, 200);
        std::vector<double> x, g(3);
        int evals = 0;
        while (m.ask(x)) {
            for (int i = 0; i < 3; i++)
                if (x[i] < -1.0 || x[i] > 1.0) {
                    std::printf("start %d: trial point outside the box\n", s);
                    bad++;
                }
            const double f = quad(x, g) - fstar;
            evals++;
            m.tell(f, g);
            if (evals > 5000) break;
        }
        double err = 0.0;
        for (int i = 0; i < 3; i++) err = std::fmax(err, std::fabs(m.x[i] - xs[i]));
        std::printf("start %d: %d evaluations, %lld iterations, max |x - x*| = %.3e, f - f* = %.3e\n", s, evals, (long long)m.it, err,
                    m.f);
        if (!(err <= 1e-6) || evals > 5000 || m.x[1] != 1.0) bad++;
    }
    // a start whose first evaluation fails ends at once and stays infinite
    {
        const double theta0[3] = {1.0, 1.0, 1.0};
        egx::LbfgsStart m(theta0, 3, lo, hi, 50);
        std::vector<double> x, g(3, 0.0);
        if (!m.ask(x)) bad++;
        m.tell(std::numeric_limits<double>::infinity(), g);
        if (m.ask(x) || std::isfinite(m.f)) bad++;
    }
    if (bad) return 1;
    std::printf("lbfgs ok\n");
    return 0;
}
