// csrc/lbfgs.h's second entry, LbfgsStart(LbfgsStart::Linear(), x0, ...): the machine started from the point itself, not from
// log10 of it -- what egx_sgp_fit_lbfgs_z uses for [log10 params, inducing coordinates scaled to [0, 1]].
//   1. a convex quadratic in MIXED variables: v = (log10 p_0, log10 p_1 in [-2, 2]; u_0, u_1, u_2 in [0, 1]),
//      f(v) = 1/2 (v - c)^T Q (v - c) - f*, c_{u_1} = 1.4 outside the box: the minimiser has u_1 = 1 active, the other four from
//      the reduced 4 x 4 system (Gaussian elimination below), to 1e-6;
//   2. the old constructor on lbfgs_test.cpp's problem: the evaluation and iteration counts it had before the second entry
//      existed (10 / 9 and 9 / 8), and, started from the old machine's own first point, the new entry asks for the same points
//      bit for bit: one machine behind both.
// g++ -std=c++17 -Wall -Werror -I egobox_amd/csrc tests/c_host/lbfgs_linear_test.cpp
#include <cmath>
#include <cstdio>
#include <vector>

#include "lbfgs.h"

namespace {
constexpr int H = 5;
const double Q5[H][H] = {{90.0, 12.0, 8.0, -6.0, 4.0},
                         {12.0, 70.0, -5.0, 9.0, 3.0},
                         {8.0, -5.0, 150.0, 20.0, -10.0},
                         {-6.0, 9.0, 20.0, 110.0, 15.0},
                         {4.0, 3.0, -10.0, 15.0, 130.0}};
const double c5[H] = {0.7, -1.1, 0.35, 1.4, 0.8};

double quad5(const std::vector<double> &v, std::vector<double> &g) {
    double f = 0.0;
    for (int i = 0; i < H; i++) {
        g[i] = 0.0;
        for (int j = 0; j < H; j++) g[i] += Q5[i][j] * (v[j] - c5[j]);
        f += 0.5 * (v[i] - c5[i]) * g[i];
    }
    return f;
}

const double Q3[3][3] = {{200.0, 40.0, 10.0}, {40.0, 120.0, 20.0}, {10.0, 20.0, 80.0}};  // lbfgs_test.cpp's problem
const double c3[3] = {0.3, 1.8, -0.4};
double quad3(const std::vector<double> &x, std::vector<double> &g) {
    double f = 0.0;
    for (int i = 0; i < 3; i++) {
        g[i] = 0.0;
        for (int j = 0; j < 3; j++) g[i] += Q3[i][j] * (x[j] - c3[j]);
        f += 0.5 * (x[i] - c3[i]) * g[i];
    }
    return f;
}
}  // namespace

int main() {
    int bad = 0;
    // ---- 1. mixed variables, u_1 (index 3) on its upper bound
    const int F[4] = {0, 1, 2, 4};
    double A[4][5];
    for (int r = 0; r < 4; r++) {
        for (int q = 0; q < 4; q++) A[r][q] = Q5[F[r]][F[q]];
        A[r][4] = -Q5[F[r]][3] * (1.0 - c5[3]);
    }
    for (int p = 0; p < 4; p++)  // Q_FF is diagonally dominant: no pivoting
        for (int r = p + 1; r < 4; r++) {
            const double m = A[r][p] / A[p][p];
            for (int q = p; q < 5; q++) A[r][q] -= m * A[p][q];
        }
    double w[4];
    for (int r = 3; r >= 0; r--) {
        double s = A[r][4];
        for (int q = r + 1; q < 4; q++) s -= A[r][q] * w[q];
        w[r] = s / A[r][r];
    }
    std::vector<double> vs(H), gs(H);
    for (int r = 0; r < 4; r++) vs[F[r]] = c5[F[r]] + w[r];
    vs[3] = 1.0;
    const double fstar = quad5(vs, gs);
    const std::vector<double> lo = {-2.0, -2.0, 0.0, 0.0, 0.0}, hi = {2.0, 2.0, 1.0, 1.0, 1.0};
    for (int i = 0; i < H; i++)
        if (i != 3 && !(vs[i] > lo[i] && vs[i] < hi[i] && std::fabs(gs[i]) < 1e-11)) bad++;
    if (!(gs[3] < 0.0)) bad++;
    if (bad) std::printf("the stated minimiser does not satisfy the KKT conditions\n");
    const double p0[2][2] = {{3.0, 0.2}, {100.0, 0.01}};  // parameters, handed over as log10
    const double u0[2][3] = {{0.5, 0.5, 0.5}, {0.0, 1.0, 1.0}};
    for (int s = 0; s < 2; s++) {
        const double x0[H] = {std::log10(p0[s][0]), std::log10(p0[s][1]), u0[s][0], u0[s][1], u0[s][2]};
        egx::LbfgsStart m(egx::LbfgsStart::Linear(), x0, H, lo, hi, 200);
        for (int i = 0; i < H; i++)
            if (m.x[i] != x0[i]) bad++;  // inside the box: the start is the point itself
        std::vector<double> x, g(H);
        int evals = 0;
        while (m.ask(x)) {
            for (int i = 0; i < H; i++)
                if (x[i] < lo[i] || x[i] > hi[i]) {
                    std::printf("mixed start %d: trial point outside the box\n", s);
                    bad++;
                }
            const double f = quad5(x, g) - fstar;
            evals++;
            m.tell(f, g);
            if (evals > 5000) break;
        }
        double err = 0.0;
        for (int i = 0; i < H; i++) err = std::fmax(err, std::fabs(m.x[i] - vs[i]));
        std::printf("mixed start %d: %d evaluations, %lld iterations, max |v - v*| = %.3e, f - f* = %.3e\n", s, evals,
                    (long long)m.it, err, m.f);
        if (!(err <= 1e-6) || evals > 5000 || m.x[3] != 1.0) bad++;
    }
    {  // a start outside the box is clipped onto it
        const double x0[H] = {5.0, -5.0, -0.5, 1.5, 0.25};
        egx::LbfgsStart m(egx::LbfgsStart::Linear(), x0, H, lo, hi, 5);
        if (m.x[0] != 2.0 || m.x[1] != -2.0 || m.x[2] != 0.0 || m.x[3] != 1.0 || m.x[4] != 0.25) bad++;
    }
    // ---- 2. the old constructor's walk on lbfgs_test.cpp's problem
    {
        std::vector<double> xs(3), gtmp(3);
        const double r0 = -Q3[0][1] * (1.0 - c3[1]), r2 = -Q3[2][1] * (1.0 - c3[1]);
        const double det = Q3[0][0] * Q3[2][2] - Q3[0][2] * Q3[2][0];
        xs = {c3[0] + (r0 * Q3[2][2] - Q3[0][2] * r2) / det, 1.0, c3[2] + (Q3[0][0] * r2 - Q3[2][0] * r0) / det};
        const double fs3 = quad3(xs, gtmp);
        const std::vector<double> lo3(3, -1.0), hi3(3, 1.0);
        const double starts[2][3] = {{-0.5, -0.5, 0.5}, {1.0, 1.0, -1.0}};
        const int want_evals[2] = {10, 9}, want_it[2] = {9, 8};
        for (int s = 0; s < 2; s++) {
            double theta0[3];
            for (int i = 0; i < 3; i++) theta0[i] = std::pow(10.0, starts[s][i]);
            egx::LbfgsStart a(theta0, 3, lo3, hi3, 200);
            egx::LbfgsStart b(egx::LbfgsStart::Linear(), a.x.data(), 3, lo3, hi3, 200);
            std::vector<double> xa, xb, g(3);
            int evals = 0;
            while (a.ask(xa)) {
                if (!b.ask(xb) || xa != xb) {
                    std::printf("old start %d: the two entries part at evaluation %d\n", s, evals);
                    bad++;
                    break;
                }
                const double f = quad3(xa, g) - fs3;
                evals++;
                a.tell(f, g);
                b.tell(f, g);
                if (evals > 5000) break;
            }
            if (b.ask(xb)) bad++;
            std::printf("old start %d: %d evaluations, %lld iterations\n", s, evals, (long long)a.it);
            if (evals != want_evals[s] || a.it != want_it[s] || a.x != b.x || a.f != b.f) bad++;
        }
    }
    if (bad) return 1;
    std::printf("lbfgs linear ok\n");
    return 0;
}
