// Host build of egobox_amd/csrc/infill_math.h and infill_mix_math.h for tests/test_infill_cstr_cpu.py: the constraint values
// handed to the optimiser (cstr_value / cstr_grad) and the mean halves of the mixture fold.  Self-checking: prints one line per
// failed check, exit code = number of failures.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "infill_math.h"
#include "infill_mix_math.h"

using namespace egx::infill;

static int fails = 0;
static void expect(bool ok, const char *what, double got, double want) {
    if (ok) return;
    fails++;
    std::printf("FAIL %s: got %.17g, want %.17g\n", what, got, want);
}

// a smooth "surrogate" of d inputs: mean and variance as functions of x
static double mu_of(const double *x, int d) {
    double s = 0.3;
    for (int c = 0; c < d; c++) s += std::sin(1.3 * x[c] + 0.2 * c) * (c + 1);
    return s;
}
static double var_of(const double *x, int d) {
    double s = 0.05;
    for (int c = 0; c < d; c++) s += 0.4 * (x[c] - 0.1 * c) * (x[c] - 0.1 * c) * (c + 1);
    return s;
}

int main() {
    const double h = 1e-6;
    for (int d = 1; d <= 3; d++) {
        const double x0[3] = {0.37, -0.81, 1.4}, scale = 2.5;
        double dmu[3], dvar[3];
        for (int c = 0; c < d; c++) {
            double xp[3], xm[3];
            std::memcpy(xp, x0, sizeof xp), std::memcpy(xm, x0, sizeof xm);
            xp[c] += h, xm[c] -= h;
            dmu[c] = (mu_of(xp, d) - mu_of(xm, d)) / (2 * h);  // (exact derivatives to ~1e-10: smooth closed forms)
            dvar[c] = (var_of(xp, d) - var_of(xm, d)) / (2 * h);
        }
        const double mu = mu_of(x0, d), var = var_of(x0, d);
        expect(cstr_value(kCstrMean, mu, var, scale) == mu / scale, "mean value", cstr_value(kCstrMean, mu, var, scale), mu / scale);
        expect(cstr_value(kCstrUtb, mu, var, scale) == (mu + 3.0 * std::sqrt(var)) / scale, "utb value",
               cstr_value(kCstrUtb, mu, var, scale), (mu + 3.0 * std::sqrt(var)) / scale);
        for (int s = kCstrMean; s <= kCstrUtb; s++)
            for (int c = 0; c < d; c++) {  // against central differences of cstr_value along coordinate c
                double xp[3], xm[3];
                std::memcpy(xp, x0, sizeof xp), std::memcpy(xm, x0, sizeof xm);
                xp[c] += h, xm[c] -= h;
                const double fd = (cstr_value(s, mu_of(xp, d), var_of(xp, d), scale) - cstr_value(s, mu_of(xm, d), var_of(xm, d), scale)) /
                                  (2 * h);
                const double g = cstr_grad(s, var, dmu[c], dvar[c], scale);
                expect(std::fabs(g - fd) <= 1e-7 * (1.0 + std::fabs(fd)), "gradient against central differences", g, fd);
            }
        // deviation 4: the reference's formula takes var_grad[[0, 0]] for every coordinate (solver_computations.rs:242)
        const double sigma = std::sqrt(var);
        for (int c = 0; c < d; c++) {
            const double ref = (dmu[c] + 3.0 * (dvar[0] / (2.0 * sigma))) / scale;
            const double g = cstr_grad(kCstrUtb, var, dmu[c], dvar[c], scale);
            if (c == 0) expect(g == ref, "d = 1 / first coordinate agrees with the reference's formula", g, ref);
            else expect(std::fabs(g - ref) > 1e-3, "other coordinates use their own d var / d x_c", g, ref);
        }
    }
    // sigma < DBL_EPSILON: sigma' = 0 (a training point); just above: the quotient
    expect(cstr_grad(kCstrUtb, 0.0, 0.7, 5.0, 2.0) == 0.35, "sigma' = 0 at var = 0", cstr_grad(kCstrUtb, 0.0, 0.7, 5.0, 2.0), 0.35);
    expect(cstr_grad(kCstrUtb, 1e-33, 0.7, 5.0, 2.0) == 0.35, "sigma' = 0 below eps", cstr_grad(kCstrUtb, 1e-33, 0.7, 5.0, 2.0), 0.35);
    {
        const double var = 1e-30, sigma = std::sqrt(var), want = (0.7 + 3.0 * (5.0 / (2.0 * sigma))) / 2.0;
        expect(cstr_grad(kCstrUtb, var, 0.7, 5.0, 2.0) == want, "sigma' above eps", cstr_grad(kCstrUtb, var, 0.7, 5.0, 2.0), want);
    }
    expect(cstr_value(kCstrUtb, 1.0, 0.0, 4.0) == 0.25, "utb value at var = 0", cstr_value(kCstrUtb, 1.0, 0.0, 4.0), 0.25);
    expect(cstr_grad(kCstrMean, 123.0, 0.7, 5.0, 2.0) == 0.35, "mean gradient ignores the variance",
           cstr_grad(kCstrMean, 123.0, 0.7, 5.0, 2.0), 0.35);
    // the mean halves of the mixture fold are bit for bit the full fold's means
    for (int smooth = 0; smooth <= 1; smooth++) {
        const int k = 3, d = 2;
        const double p[k] = {0.2, 0.5, 0.3}, dp[k * d] = {0.1, -0.2, 0.05, 0.3, -0.15, -0.1};
        const double mu[k] = {1.7, -0.3, 0.9}, v[k] = {0.2, 0.4, 0.1};
        const double gmu[k * d] = {0.3, 0.1, -0.7, 0.2, 0.5, -0.4}, gv[k * d] = {0.01, 0.02, 0.03, -0.01, 0.0, 0.05};
        double mean, var, gm[d], gvv[d], gm2[d];
        mix_value(smooth != 0, k, p, 1, mu, v, 1, &mean, &var);
        mix_grad(smooth != 0, k, d, p, 1, dp, d, mu, v, 1, gmu, gv, d, gm, gvv);
        const double mean2 = mix_mean(smooth != 0, k, p, 1, mu, 1);
        mix_grad_mean(smooth != 0, k, d, p, 1, dp, d, mu, 1, gmu, d, gm2);
        expect(mean2 == mean, "mix_mean equals mix_value's mean", mean2, mean);
        for (int l = 0; l < d; l++) expect(gm2[l] == gm[l], "mix_grad_mean equals mix_grad's gmean", gm2[l], gm[l]);
    }
    if (!fails) std::printf("ok\n");
    return fails;
}
