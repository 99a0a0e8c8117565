// Projected L-BFGS on a box as an ask / tell machine, one per start point: the caller evaluates the objective and its gradient
// at the point ask() hands out and reports them with tell().  The variable is x = log10(parameter); a step moves at most one
// decade, the line search is Armijo on the projected step, the memory is 8 pairs.  Host only (no device code: compiles under
// g++, tests/c_host/lbfgs_test.cpp).  The machines of a fit's starts are built by fit_starts.h (lbfgs_machines: they point into
// its Log10Box) and driven by multistart::run: egx_gp_fit_lbfgs (gp_fit.hip) every start in lock-step, egx_sgp_fit_lbfgs
// (sgp_host.hip) the starts one after the other; egx_sgp_fit_lbfgs_z adds one start in mixed variables (LbfgsStart::Linear).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace egx {
struct LbfgsStart {
    int h = 0;
    int64_t max_iter = 50;
    const std::vector<double> *blo = nullptr, *bhi = nullptr;
    std::vector<double> x, g, pg, dir, xn;
    std::vector<std::vector<double>> S, Y;
    std::vector<double> rho;
    double f = std::numeric_limits<double>::infinity(), t = 1.0;
    int64_t it = 0;
    int ls = 0;
    enum { INIT, LINE, DONE } st = INIT;
    static constexpr int mem = 8;

    void clip(std::vector<double> &v) const {
        for (int i = 0; i < h; i++) v[i] = std::fmin((*bhi)[i], std::fmax((*blo)[i], v[i]));
    }
    LbfgsStart(const double *theta0, int h_, const std::vector<double> &lo, const std::vector<double> &hi, int64_t max_it)
        : h(h_), max_iter(max_it), blo(&lo), bhi(&hi), x(h_), g(h_), pg(h_), dir(h_), xn(h_) {
        for (int i = 0; i < h; i++) x[i] = std::log10(theta0[i]);
        clip(x);
    }
    // The same machine started from variables that are not log10 of anything (egx_sgp_fit_lbfgs_z: log10 parameters followed by
    // inducing coordinates scaled to [0, 1]): x0 is the point itself, clipped to the box.  "One decade per step" then reads "one
    // unit of the caller's variables per step".
    struct Linear {};
    LbfgsStart(Linear, const double *x0, int h_, const std::vector<double> &lo, const std::vector<double> &hi, int64_t max_it)
        : h(h_), max_iter(max_it), blo(&lo), bhi(&hi), x(x0, x0 + h_), g(h_), pg(h_), dir(h_), xn(h_) {
        clip(x);
    }
    // the point to evaluate next (log10 theta), or false when this start is finished
    bool ask(std::vector<double> &out) const {
        if (st == DONE) return false;
        out = (st == INIT) ? x : xn;
        return true;
    }
    // start iteration `it` at (x, f, g): convergence test, two-loop recursion on the projected gradient, first trial step
    void begin_iteration() {
        if (it >= max_iter) {
            st = DONE;
            return;
        }
        double pgmax = 0.0;
        for (int i = 0; i < h; i++) {
            const bool at_lo = x[i] <= (*blo)[i] && g[i] > 0.0, at_hi = x[i] >= (*bhi)[i] && g[i] < 0.0;
            pg[i] = (at_lo || at_hi) ? 0.0 : g[i];
            pgmax = std::fmax(pgmax, std::fabs(pg[i]));
        }
        if (pgmax <= 1e-5 * (1.0 + std::fabs(f))) {
            st = DONE;
            return;
        }
        std::vector<double> q(pg), alpha(S.size());
        for (int j = (int)S.size() - 1; j >= 0; j--) {
            double a = 0.0;
            for (int i = 0; i < h; i++) a += S[j][i] * q[i];
            a *= rho[j];
            alpha[j] = a;
            for (int i = 0; i < h; i++) q[i] -= a * Y[j][i];
        }
        if (!S.empty()) {
            double sy = 0.0, yy = 0.0;
            for (int i = 0; i < h; i++) {
                sy += S.back()[i] * Y.back()[i];
                yy += Y.back()[i] * Y.back()[i];
            }
            for (int i = 0; i < h; i++) q[i] *= sy / yy;
        }
        for (size_t j = 0; j < S.size(); j++) {
            double b = 0.0;
            for (int i = 0; i < h; i++) b += Y[j][i] * q[i];
            b *= rho[j];
            for (int i = 0; i < h; i++) q[i] += (alpha[j] - b) * S[j][i];
        }
        double dg = 0.0, dmax = 0.0;
        for (int i = 0; i < h; i++) {
            dir[i] = (pg[i] == 0.0) ? 0.0 : -q[i];
            dg += dir[i] * pg[i];
            dmax = std::fmax(dmax, std::fabs(dir[i]));
        }
        if (!(dg < 0.0)) {  // not a descent direction: steepest descent
            dmax = 0.0;
            for (int i = 0; i < h; i++) {
                dir[i] = -pg[i];
                dmax = std::fmax(dmax, std::fabs(dir[i]));
            }
        }
        t = S.empty() ? std::fmin(1.0, 0.5 / dmax) : std::fmin(1.0, 1.0 / dmax);  // <= 1 decade per step
        ls = 0;
        trial();
        st = LINE;
    }
    void trial() {
        for (int i = 0; i < h; i++) xn[i] = x[i] + t * dir[i];
        clip(xn);
    }
    // objective and gradient (in x) at the point ask() handed out; fv = +inf for a failed evaluation
    void tell(double fv, const std::vector<double> &gv) {
        if (st == INIT) {
            f = fv;
            g = gv;
            if (!std::isfinite(f)) {
                st = DONE;
                return;
            }
            begin_iteration();
            return;
        }
        if (st != LINE) return;
        double dec = 0.0;
        for (int i = 0; i < h; i++) dec += pg[i] * (xn[i] - x[i]);
        if (std::isfinite(fv) && fv <= f + 1e-4 * dec) {  // Armijo on the projected step
            std::vector<double> sv(h), yv(h);
            double sy = 0.0;
            for (int i = 0; i < h; i++) {
                sv[i] = xn[i] - x[i];
                yv[i] = gv[i] - g[i];
                sy += sv[i] * yv[i];
            }
            const double fprev = f;
            x = xn;
            g = gv;
            f = fv;
            if (sy > 1e-12) {
                S.push_back(sv);
                Y.push_back(yv);
                rho.push_back(1.0 / sy);
                if ((int)S.size() > mem) {
                    S.erase(S.begin());
                    Y.erase(Y.begin());
                    rho.erase(rho.begin());
                }
            }
            it++;
            if (std::fabs(fprev - f) <= 1e-7 * (std::fabs(f) + 1e-300)) {
                st = DONE;
                return;
            }
            begin_iteration();
            return;
        }
        if (++ls >= 12) {  // the line search gave up: this start ends where it is
            st = DONE;
            return;
        }
        t *= 0.5;
        trial();
    }
};
}  // namespace egx
