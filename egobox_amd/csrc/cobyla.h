// COBYLA for bound-constrained minimisation, as a resumable (ask / tell) state machine.
//
// The reference tunes theta with the `cobyla` crate 0.8.0 (crates/gp/src/optimization.rs:122-169: `minimize(objfn, x0,
// bounds, cons = [], maxeval, RhoBeg::All(0.5), StopTols { ftol_rel: 1e-4, .. })`), a port of the COBYLA in NLopt, which is
// M. J. D. Powell's "direct search optimization method that models the objective and constraint functions by linear
// interpolation" (1994) plus S. G. Johnson's wrapper: variables rescaled by the initial step, bounds turned into 2n
// linear inequality constraints AND the objective evaluated at the point clamped into the box, initial simplex steps
// flipped to stay inside the box, rho doubled after a step whose actual reduction is within 10 % of the predicted
// one, and the ftol test made where rho is about to be reduced (best value now against the best value at the previous
// reduction).  The crate is not vendored in the reference checkout, so this file restates the PUBLISHED algorithm:
//   * the simplex / merit-function / trust-radius logic of Powell's COBYLB (vertex replacement by the sigma / eta
//     acceptability test, penalty parameter mu raised to 2 * barmu, rho halved when no progress) follows the paper;
//   * the trust-region subproblem -- minimise the greatest violation of the linearised constraints inside the ball, then
//     the linear model of f without increasing it (Powell's TRSTLP) -- is solved in CLOSED FORM: the only constraints
//     here are bounds, whose linear models are exact, so the two stages reduce to a shrink-the-excess step and to
//     d(tau) = clip(-tau g, L, U) with tau fixed by |d| = rho (the point Powell's active-set path ends at for a box).
// Every start of the multistart is one machine; the driver advances all of them in lock-step and evaluates their
// requests as ONE egx_gp_likelihood_batch (gp_fit.hip).
// Two classes: CobylaBox (bounds only, the closed form above) and, further down, Cobyla (m nonlinear constraints beside the
// bounds, Powell's TRSTLP in full) for the infill optimiser whose constraint surrogates are constraints (infill_optimize.hip).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace egx {

class CobylaBox {
public:
    enum Status { RUNNING = 0, MAXEVAL = 1, FTOL = 2, RHOEND = 3, ROUNDOFF = 4 };

    // x0, lo, hi in the caller's units; rhobeg = initial step (all coordinates), ftol_rel / ftol_abs as nlopt_stop_ftol
    // (ftol_abs = 0: the relative test alone, bit for bit what every caller before the infill optimiser got)
    CobylaBox(const std::vector<double> &x0, const std::vector<double> &lo, const std::vector<double> &hi, double rhobeg,
              double ftol_rel, int64_t maxeval, double rhoend_scaled = 0.0, bool rho_doubling = true, bool clamp_eval = true,
              double ftol_abs = 0.0)
        : n_((int)x0.size()), scale_(rhobeg), ftol_rel_(ftol_rel), ftol_abs_(ftol_abs), maxfun_(maxeval), rhoend_(rhoend_scaled),
          rho_doubling_(rho_doubling), clamp_eval_(clamp_eval) {
        const int n = n_;
        lo_.resize(n);
        hi_.resize(n);
        x_.resize(n);
        for (int i = 0; i < n; i++) {  // rescaled variables: the initial step is 1 in every coordinate
            lo_[i] = lo[i] / scale_;
            hi_[i] = hi[i] / scale_;
            x_[i] = std::fmin(hi_[i], std::fmax(lo_[i], x0[i] / scale_));
        }
        sim_.assign((size_t)n * (n + 1), 0.0);
        simi_.assign((size_t)n * n, 0.0);
        datf_.assign(n + 1, 0.0);
        datr_.assign(n + 1, 0.0);
        vsig_.assign(n, 0.0);
        veta_.assign(n, 0.0);
        sigbar_.assign(n, 0.0);
        dx_.assign(n, 0.0);
        g_.assign(n, 0.0);
        rho_ = 1.0;
        parmu_ = 0.0;
        for (int i = 0; i < n; i++) sim(i, n) = x_[i];
        jdrop_ = n;
        ibrnch_ = 0;
        label_ = L_EVAL;
    }

    // Next point to evaluate (caller's units, inside the box).  Returns false when the run has finished.
    bool ask(std::vector<double> &x_out) {
        if (label_ != L_EVAL) run();
        if (status_ != RUNNING) return false;
        if (nfvals_ >= maxfun_ && nfvals_ > 0) {
            finish(MAXEVAL);
            return false;
        }
        x_out.resize(n_);
        for (int i = 0; i < n_; i++) x_out[i] = (clamp_eval_ ? std::fmin(hi_[i], std::fmax(lo_[i], x_[i])) : x_[i]) * scale_;
        return true;
    }

    // Objective value at the point handed out by the last ask().  Non-finite values (a failed likelihood is +inf in
    // the reference's objective, algorithm.rs:893-896) enter as a large finite barrier so that the simplex algebra
    // stays finite.
    void tell(double f) {
        if (!(f == f) || f > kBarrier) f = kBarrier;
        nfvals_++;
        f_ = f;
        resmax_ = violation(x_);
        label_ = L_AFTER_EVAL;
        run();
    }

    Status status() const { return status_; }
    int64_t evals() const { return nfvals_; }
    double best_f() const { return fbest_; }
    std::vector<double> best_x() const {
        std::vector<double> r(n_);
        for (int i = 0; i < n_; i++) r[i] = std::fmin(hi_[i], std::fmax(lo_[i], xbest_[i])) * scale_;
        return r;
    }

private:
    static constexpr double kBarrier = 1e30;
    enum Label { L_EVAL, L_AFTER_EVAL, L140, L370, L440, L550, L_DONE };
    int n_;
    double scale_, ftol_rel_, ftol_abs_;
    int64_t maxfun_;
    double rhoend_;
    bool rho_doubling_;  // false = Powell's original radius schedule (used to validate against his Fortran code)
    bool clamp_eval_;    // false = hand out the raw trial point even outside the box (Powell's original; validation only)
    std::vector<double> lo_, hi_, x_, sim_, simi_, datf_, datr_, vsig_, veta_, sigbar_, dx_, g_, xbest_;
    double rho_ = 1.0, parmu_ = 0.0, f_ = 0.0, resmax_ = 0.0, prerec_ = 0.0, prerem_ = 0.0, parsig_ = 0.0;
    double minf_ = std::numeric_limits<double>::infinity(), fbest_ = std::numeric_limits<double>::infinity();
    int jdrop_ = 0, ibrnch_ = 0, iflag_ = 0, ifull_ = 0;
    int64_t nfvals_ = 0;
    Label label_ = L_EVAL;
    Status status_ = RUNNING;

    double &sim(int i, int j) { return sim_[(size_t)i * (n_ + 1) + j]; }
    double &simi(int i, int j) { return simi_[(size_t)i * n_ + j]; }

    // greatest violation of the 2n bound constraints c = x - lo >= 0, hi - x >= 0 (rescaled units)
    double violation(const std::vector<double> &x) const {
        double r = 0.0;
        for (int i = 0; i < n_; i++) r = std::fmax(r, std::fmax(lo_[i] - x[i], x[i] - hi_[i]));
        return r;
    }

    // simi_ <- inverse of the n x n displacement matrix (Gauss-Jordan, partial pivoting); false when singular
    bool invert_simplex() {
        const int n = n_;
        std::vector<double> a((size_t)n * 2 * n, 0.0);
        for (int i = 0; i < n; i++) {
            for (int j = 0; j < n; j++) a[(size_t)i * 2 * n + j] = sim(i, j);
            a[(size_t)i * 2 * n + n + i] = 1.0;
        }
        for (int c = 0; c < n; c++) {
            int piv = c;
            for (int r = c + 1; r < n; r++)
                if (std::fabs(a[(size_t)r * 2 * n + c]) > std::fabs(a[(size_t)piv * 2 * n + c])) piv = r;
            if (a[(size_t)piv * 2 * n + c] == 0.0) return false;
            if (piv != c)
                for (int j = 0; j < 2 * n; j++) std::swap(a[(size_t)piv * 2 * n + j], a[(size_t)c * 2 * n + j]);
            const double inv = 1.0 / a[(size_t)c * 2 * n + c];
            for (int j = 0; j < 2 * n; j++) a[(size_t)c * 2 * n + j] *= inv;
            for (int r = 0; r < n; r++)
                if (r != c) {
                    const double f = a[(size_t)r * 2 * n + c];
                    if (f != 0.0)
                        for (int j = 0; j < 2 * n; j++) a[(size_t)r * 2 * n + j] -= f * a[(size_t)c * 2 * n + j];
                }
        }
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) simi(i, j) = a[(size_t)i * 2 * n + n + j];
        return true;
    }

    void finish(Status s) {
        status_ = s;
        label_ = L_DONE;
        // the optimal vertex sits in the pole position of the simplex
        xbest_.resize(n_);
        for (int i = 0; i < n_; i++) xbest_[i] = sim(i, n_);
        fbest_ = datf_[n_];
        if (s == RHOEND && ifull_ == 1) {  // Powell returns the last trial point itself in this case
            xbest_ = x_;
            fbest_ = f_;
        }
    }

    // Powell's TRSTLP for box constraints in closed form: dx_ <- step from the pole x0, ifull_ <- 1 when |dx| = rho
    void trust_step(const std::vector<double> &x0) {
        const int n = n_;
        const double rho = rho_;
        std::vector<double> vlo(n), vhi(n);
        double res0 = 0.0;
        for (int i = 0; i < n; i++) {
            vlo[i] = lo_[i] - x0[i];
            vhi[i] = x0[i] - hi_[i];
            res0 = std::fmax(res0, std::fmax(vlo[i], vhi[i]));
        }
        double tstar = 0.0;
        if (res0 > 0.0) {  // stage 1: the least greatest violation t reachable inside the ball
            auto need = [&](double t) {
                double s = 0.0;
                for (int i = 0; i < n; i++) {
                    const double a = std::fmax(0.0, vlo[i] - t), b = std::fmax(0.0, vhi[i] - t);
                    s += a * a + b * b;
                }
                return s;
            };
            if (need(0.0) > rho * rho) {
                double a = 0.0, b = res0;
                for (int it = 0; it < 200; it++) {
                    const double mid = 0.5 * (a + b);
                    if (need(mid) > rho * rho) a = mid; else b = mid;
                }
                tstar = b;
            }
        }
        std::vector<double> L(n), U(n);
        for (int i = 0; i < n; i++) {
            L[i] = vlo[i] - tstar;   // d_i >= L_i keeps the lower-bound violation at or below t*
            U[i] = -vhi[i] + tstar;  // d_i <= U_i
        }
        auto clipd = [&](double tau, std::vector<double> &d) {
            double s = 0.0;
            for (int i = 0; i < n; i++) {
                double v = -tau * g_[i];
                if (g_[i] == 0.0) v = 0.0;
                v = std::fmin(U[i], std::fmax(L[i], v));
                d[i] = v;
                s += v * v;
            }
            return s;
        };
        ifull_ = 0;
        if (tstar > 0.0) {  // the ball was used up reducing the violation: no second stage
            clipd(0.0, dx_);
            ifull_ = 1;
            return;
        }
        // stage 2: d(tau) = clip(-tau g, L, U), tau as large as the ball allows
        double gmax = 0.0;
        for (int i = 0; i < n; i++) gmax = std::fmax(gmax, std::fabs(g_[i]));
        if (gmax == 0.0 || !(gmax < std::numeric_limits<double>::infinity())) {
            clipd(0.0, dx_);
            return;
        }
        double tau_inf = 0.0;  // beyond this tau every moving coordinate sits on its bound
        for (int i = 0; i < n; i++)
            if (g_[i] != 0.0) tau_inf = std::fmax(tau_inf, (g_[i] < 0.0 ? U[i] : -L[i]) / std::fabs(g_[i]));
        tau_inf = std::fmax(tau_inf, 0.0);
        if (clipd(tau_inf, dx_) <= rho * rho) return;  // the whole box corner lies inside the ball
        double a = 0.0, b = tau_inf;
        for (int it = 0; it < 200; it++) {
            const double mid = 0.5 * (a + b);
            if (clipd(mid, dx_) > rho * rho) b = mid; else a = mid;
        }
        clipd(a, dx_);
        ifull_ = 1;
    }

    void run() {
        const int n = n_, np = n_;
        const double alpha = 0.25, beta = 2.1, gamma = 0.5, delta = 1.1;
        for (;;) {
            switch (label_) {
            case L_EVAL:
            case L_DONE:
                return;
            case L_AFTER_EVAL: {
                if (ibrnch_ == 1) {
                    label_ = L440;
                    break;
                }
                // a vertex of the initial simplex (or of a geometry step)
                datf_[jdrop_] = f_;
                datr_[jdrop_] = resmax_;
                if (nfvals_ <= np + 1) {
                    if (jdrop_ < n) {
                        if (datf_[np] <= f_) {
                            x_[jdrop_] = sim(jdrop_, np);
                        } else {  // the new point becomes the pole
                            // (the old pole and the vertices made so far all move by -step along this coordinate)
                            const double step = sim(jdrop_, jdrop_);
                            sim(jdrop_, np) = x_[jdrop_];
                            std::swap(datf_[jdrop_], datf_[np]);
                            std::swap(datr_[jdrop_], datr_[np]);
                            for (int k = 0; k <= jdrop_; k++) sim(jdrop_, k) = -step;
                        }
                    }
                    if (nfvals_ <= n) {
                        jdrop_ = (int)nfvals_ - 1;
                        // step of the initial simplex, flipped / shortened so that the vertex stays inside the box
                        double step = rho_;
                        const double xj = x_[jdrop_];
                        if (xj + step > hi_[jdrop_]) {
                            if (xj - step >= lo_[jdrop_]) step = -step;
                            else if (hi_[jdrop_] - xj > xj - lo_[jdrop_]) step = 0.5 * (hi_[jdrop_] - xj);
                            else step = -0.5 * (xj - lo_[jdrop_]);
                        }
                        if (step == 0.0) step = rho_;  // degenerate box (lo == hi): the violation term takes over
                        x_[jdrop_] += step;
                        sim(jdrop_, jdrop_) = step;
                        label_ = L_EVAL;
                        return;
                    }
                    if (!invert_simplex()) {  // initial simplex complete: SIMI = inverse of the displacement matrix
                        finish(ROUNDOFF);
                        return;
                    }
                }
                ibrnch_ = 1;
                label_ = L140;
                break;
            }
            case L140: {
                // the optimal vertex (merit f + mu * violation) goes to the pole position
                double phimin = datf_[np] + parmu_ * datr_[np];
                int nbest = np;
                for (int j = 0; j < n; j++) {
                    const double temp = datf_[j] + parmu_ * datr_[j];
                    if (temp < phimin) {
                        nbest = j;
                        phimin = temp;
                    } else if (temp == phimin && parmu_ == 0.0 && datr_[j] < datr_[nbest]) {
                        nbest = j;
                    }
                }
                if (nbest < n) {
                    std::swap(datf_[np], datf_[nbest]);
                    std::swap(datr_[np], datr_[nbest]);
                    for (int i = 0; i < n; i++) {
                        const double temp = sim(i, nbest);
                        sim(i, nbest) = 0.0;
                        sim(i, np) += temp;
                        double tempa = 0.0;
                        for (int k = 0; k < n; k++) {
                            sim(i, k) -= temp;
                            tempa -= simi(k, i);
                        }
                        simi(nbest, i) = tempa;
                    }
                }
                // SIMI must still be the inverse of SIM
                double error = 0.0;
                for (int i = 0; i < n; i++)
                    for (int j = 0; j < n; j++) {
                        double temp = (i == j) ? -1.0 : 0.0;
                        for (int k = 0; k < n; k++) temp += simi(i, k) * sim(k, j);
                        error = std::fmax(error, std::fabs(temp));
                    }
                if (!(error <= 0.1)) {
                    finish(ROUNDOFF);
                    return;
                }
                // gradient of the linear interpolant of f
                for (int i = 0; i < n; i++) {
                    double temp = 0.0;
                    for (int j = 0; j < n; j++) temp += (datf_[j] - datf_[np]) * simi(j, i);
                    g_[i] = temp;
                }
                // acceptability of the simplex
                iflag_ = 1;
                parsig_ = alpha * rho_;
                const double pareta = beta * rho_;
                for (int j = 0; j < n; j++) {
                    double wsig = 0.0, weta = 0.0;
                    for (int i = 0; i < n; i++) {
                        wsig += simi(j, i) * simi(j, i);
                        weta += sim(i, j) * sim(i, j);
                    }
                    vsig_[j] = 1.0 / std::sqrt(wsig);
                    veta_[j] = std::sqrt(weta);
                    if (vsig_[j] < parsig_ || veta_[j] > pareta) iflag_ = 0;
                }
                if (ibrnch_ == 1 || iflag_ == 1) {
                    label_ = L370;
                    break;
                }
                // geometry step: replace the worst vertex
                int jd = -1;
                double temp = pareta;
                for (int j = 0; j < n; j++)
                    if (veta_[j] > temp) {
                        jd = j;
                        temp = veta_[j];
                    }
                if (jd < 0)
                    for (int j = 0; j < n; j++)
                        if (vsig_[j] < temp) {
                            jd = j;
                            temp = vsig_[j];
                        }
                jdrop_ = jd;
                temp = gamma * rho_ * vsig_[jd];
                for (int i = 0; i < n; i++) dx_[i] = temp * simi(jd, i);
                // sign of the step: the one with the smaller predicted merit (constraints are linear: exact)
                double cvmaxp = 0.0, cvmaxm = 0.0, sum = 0.0;
                for (int i = 0; i < n; i++) {
                    const double clo = sim(i, np) - lo_[i], chi = hi_[i] - sim(i, np);
                    cvmaxp = std::fmax(cvmaxp, std::fmax(-dx_[i] - clo, dx_[i] - chi));
                    cvmaxm = std::fmax(cvmaxm, std::fmax(dx_[i] - clo, -dx_[i] - chi));
                    sum -= g_[i] * dx_[i];
                }
                const double dxsign = (parmu_ * (cvmaxp - cvmaxm) > sum + sum) ? -1.0 : 1.0;
                temp = 0.0;
                for (int i = 0; i < n; i++) {
                    dx_[i] *= dxsign;
                    sim(i, jd) = dx_[i];
                    temp += simi(jd, i) * dx_[i];
                }
                for (int i = 0; i < n; i++) simi(jd, i) /= temp;
                for (int j = 0; j < n; j++) {
                    if (j != jd) {
                        double t2 = 0.0;
                        for (int i = 0; i < n; i++) t2 += simi(j, i) * dx_[i];
                        for (int i = 0; i < n; i++) simi(j, i) -= t2 * simi(jd, i);
                    }
                    x_[j] = sim(j, np) + dx_[j];
                }
                label_ = L_EVAL;
                return;
            }
            case L370: {
                std::vector<double> x0(n);
                for (int i = 0; i < n; i++) x0[i] = sim(i, np);
                trust_step(x0);
                if (ifull_ == 0) {
                    double temp = 0.0;
                    for (int i = 0; i < n; i++) temp += dx_[i] * dx_[i];
                    if (temp < rho_ * 0.25 * rho_) {
                        ibrnch_ = 1;
                        label_ = L550;
                        break;
                    }
                }
                // predicted change of f and of the greatest violation
                std::vector<double> xn(n);
                double sum = 0.0;
                for (int i = 0; i < n; i++) {
                    xn[i] = x0[i] + dx_[i];
                    sum += g_[i] * dx_[i];
                }
                const double resnew = violation(xn);
                double barmu = 0.0;
                prerec_ = datr_[np] - resnew;
                if (prerec_ > 0.0) barmu = sum / prerec_;
                if (parmu_ < barmu * 1.5) {
                    parmu_ = barmu * 2.0;
                    const double phi = datf_[np] + parmu_ * datr_[np];
                    bool again = false;
                    for (int j = 0; j < n && !again; j++) {
                        const double temp = datf_[j] + parmu_ * datr_[j];
                        if (temp < phi) again = true;
                        else if (temp == phi && parmu_ == 0.0 && datr_[j] < datr_[np]) again = true;
                    }
                    if (again) {
                        label_ = L140;
                        break;
                    }
                }
                prerem_ = parmu_ * prerec_ - sum;
                x_ = xn;
                ibrnch_ = 1;
                label_ = L_EVAL;
                return;
            }
            case L440: {
                const double vmold = datf_[np] + parmu_ * datr_[np];
                const double vmnew = f_ + parmu_ * resmax_;
                double trured = vmold - vmnew;
                if (parmu_ == 0.0 && f_ == datf_[np]) {
                    prerem_ = prerec_;
                    trured = datr_[np] - resmax_;
                }
                // which vertex does the new point replace?
                double ratio = (trured <= 0.0) ? 1.0 : 0.0;
                int jd = -1;
                for (int j = 0; j < n; j++) {
                    double temp = 0.0;
                    for (int i = 0; i < n; i++) temp += simi(j, i) * dx_[i];
                    temp = std::fabs(temp);
                    if (temp > ratio) {
                        jd = j;
                        ratio = temp;
                    }
                    sigbar_[j] = temp * vsig_[j];
                }
                double edgmax = delta * rho_;
                int l = -1;
                for (int j = 0; j < n; j++)
                    if (sigbar_[j] >= parsig_ || sigbar_[j] >= vsig_[j]) {
                        double temp = veta_[j];
                        if (trured > 0.0) {
                            temp = 0.0;
                            for (int i = 0; i < n; i++) temp += (dx_[i] - sim(i, j)) * (dx_[i] - sim(i, j));
                            temp = std::sqrt(temp);
                        }
                        if (temp > edgmax) {
                            l = j;
                            edgmax = temp;
                        }
                    }
                if (l >= 0) jd = l;
                if (jd < 0) {
                    label_ = L550;
                    break;
                }
                jdrop_ = jd;
                double temp = 0.0;
                for (int i = 0; i < n; i++) {
                    sim(i, jd) = dx_[i];
                    temp += simi(jd, i) * dx_[i];
                }
                for (int i = 0; i < n; i++) simi(jd, i) /= temp;
                for (int j = 0; j < n; j++)
                    if (j != jd) {
                        double t2 = 0.0;
                        for (int i = 0; i < n; i++) t2 += simi(j, i) * dx_[i];
                        for (int i = 0; i < n; i++) simi(j, i) -= t2 * simi(jd, i);
                    }
                datf_[jd] = f_;
                datr_[jd] = resmax_;
                if (trured > 0.0 && trured >= prerem_ * 0.1) {
                    // (S. G. Johnson's modification) a step that did what the model promised earns a larger radius
                    if (rho_doubling_ && trured >= prerem_ * 0.9 && trured <= prerem_ * 1.1 && iflag_) rho_ *= 2.0;
                    label_ = L140;
                    break;
                }
                label_ = L550;
                break;
            }
            case L550: {
                if (iflag_ == 0) {
                    ibrnch_ = 0;
                    label_ = L140;
                    break;
                }
                // the function-value stopping test lives where rho is about to be reduced
                {
                    const double fb = (ifull_ == 1) ? f_ : datf_[np];
                    if (fb < minf_ && (ftol_rel_ > 0.0 || ftol_abs_ > 0.0)) {
                        const double d = std::fabs(fb - minf_);
                        if (std::isfinite(minf_) && (d < ftol_abs_ || d < ftol_rel_ * (std::fabs(fb) + std::fabs(minf_)) * 0.5 || fb == minf_)) {
                            finish(FTOL);
                            return;
                        }
                    }
                    minf_ = fb;
                }
                if (rho_ > rhoend_) {
                    rho_ *= 0.5;
                    if (rho_ <= rhoend_ * 1.5) rho_ = rhoend_;
                    if (parmu_ > 0.0) {
                        // mu is reset from the spread of f over the simplex against the spread of the constraints
                        double denom = 0.0;
                        for (int c = 0; c < 2 * n; c++) {
                            const int i = c >> 1;
                            auto cval = [&](int j) {
                                const double xi = sim(i, np) + (j < n ? sim(i, j) : 0.0);
                                return (c & 1) ? hi_[i] - xi : xi - lo_[i];
                            };
                            double cmin = cval(np), cmax = cmin;
                            for (int j = 0; j < n; j++) {
                                cmin = std::fmin(cmin, cval(j));
                                cmax = std::fmax(cmax, cval(j));
                            }
                            if (cmin < cmax * 0.5) {
                                const double temp = std::fmax(cmax, 0.0) - cmin;
                                denom = (denom <= 0.0) ? temp : std::fmin(denom, temp);
                            }
                        }
                        double fmin = datf_[np], fmax = datf_[np];
                        for (int j = 0; j < n; j++) {
                            fmin = std::fmin(fmin, datf_[j]);
                            fmax = std::fmax(fmax, datf_[j]);
                        }
                        if (denom == 0.0) parmu_ = 0.0;
                        else if (fmax - fmin < parmu_ * denom) parmu_ = (fmax - fmin) / denom;
                    }
                    label_ = L140;
                    break;
                }
                finish(RHOEND);
                return;
            }
            }
        }
    }
};

// COBYLA with GENERAL nonlinear inequality constraints, the optimiser behind egx_infill_optimize_cstr (infill_optimize.hip): the
// reference hands every constraint surrogate to `cobyla` as a nonlinear constraint (crates/ego/src/solver/
// solver_infill_optim.rs:148-204).  Powell's algorithm as CobylaBox restates it -- the same COBYLB simplex / merit / radius
// logic, now over m + 2n constraints -- with his TRSTLP in full: stage one minimises the greatest violation of the
// linearised constraints inside the ball, stage two the linear model of f without increasing that violation, both along the
// active-set path (Z holds an orthogonal basis whose first nact columns span the active gradients, rotated by Givens steps
// as constraints enter and leave; vmultc the multipliers, or the residuals of the inactive constraints).
// The NLopt wrapper semantics are CobylaBox's: variables rescaled by rhobeg, the bounds as 2n linear constraints appended
// AFTER the m nonlinear ones in the order (lo_0, hi_0, lo_1, ...) and in rescaled units, f and c evaluated at the point
// clamped into the box, rho doubling, the ftol test at a rho reduction, the 1e30 barrier (a non-finite constraint value
// counts as violated by 1e30).  The caller's convention is c_j(x) <= 0 feasible; Powell's is the opposite sign.
// best_x / best_f / best_c: the best EVALUATED point, bit for bit as handed out.  A point is feasible when c_j <= cfeas_j
// for every j (and it lies in the box: always, when clamp_eval); feasible beats infeasible, among feasible points the
// smaller f wins, among infeasible ones the smaller max_j (c_j - cfeas_j), the first point on ties.
// final_x / final_f / final_c: the vertex Powell's code returns (the pole of the last simplex, or the last trial point).
class Cobyla {
public:
    enum Status { RUNNING = 0, MAXEVAL = 1, FTOL = 2, RHOEND = 3, ROUNDOFF = 4 };

    Cobyla(const std::vector<double> &x0, const std::vector<double> &lo, const std::vector<double> &hi, int m, double rhobeg,
           double ftol_rel, double ftol_abs, int64_t maxeval, double rhoend_scaled = 0.0, bool rho_doubling = true,
           bool clamp_eval = true, const std::vector<double> &cfeas = {})
        : n_((int)x0.size()), m_(m), mt_(m + 2 * (int)x0.size()), scale_(rhobeg), ftol_rel_(ftol_rel), ftol_abs_(ftol_abs),
          maxfun_(maxeval), rhoend_(rhoend_scaled), rho_doubling_(rho_doubling), clamp_eval_(clamp_eval), cfeas_(cfeas) {
        const int n = n_;
        cfeas_.resize(m, 0.0);
        lo_.resize(n);
        hi_.resize(n);
        x_.resize(n);
        for (int i = 0; i < n; i++) {
            lo_[i] = lo[i] / scale_;
            hi_[i] = hi[i] / scale_;
            x_[i] = std::fmin(hi_[i], std::fmax(lo_[i], x0[i] / scale_));
        }
        sim_.assign((size_t)n * (n + 1), 0.0);
        simi_.assign((size_t)n * n, 0.0);
        datmat_.assign((size_t)(mt_ + 2) * (n + 1), 0.0);
        con_.assign(mt_ + 2, 0.0);
        cb_.assign(mt_ + 2, 0.0);
        a_.assign((size_t)n * (mt_ + 1), 0.0);
        vsig_.assign(n, 0.0);
        veta_.assign(n, 0.0);
        sigbar_.assign(n, 0.0);
        dx_.assign(n, 0.0);
        z_.assign((size_t)n * n, 0.0);
        zdota_.assign(n + 1, 0.0);
        vmultc_.assign(mt_ + 1, 0.0);
        vmultd_.assign(mt_ + 1, 0.0);
        sdirn_.assign(n, 0.0);
        dxnew_.assign(n, 0.0);
        iact_.assign(mt_ + 1, 0);
        xout_.assign(n, 0.0);
        bestx_.assign(n, 0.0);
        bestc_.assign(m, 0.0);
        finalc_.assign(m, 0.0);
        for (int i = 0; i < n; i++) sim(i, n) = x_[i];
        jdrop_ = n;
        label_ = L_EVAL;
    }

    // Next point to evaluate (caller's units; inside the box when clamp_eval).  Returns false when the run has finished.
    bool ask(std::vector<double> &x_out) {
        if (label_ != L_EVAL) run();
        if (status_ != RUNNING) return false;
        if (nfvals_ >= maxfun_ && nfvals_ > 0) {
            finish(MAXEVAL);
            return false;
        }
        for (int i = 0; i < n_; i++) xout_[i] = (clamp_eval_ ? std::fmin(hi_[i], std::fmax(lo_[i], x_[i])) : x_[i]) * scale_;
        x_out = xout_;
        return true;
    }

    // f and the m constraint values (c_j <= 0 feasible) at the point handed out by the last ask()
    void tell(double f, const double *c) {
        const double f_raw = f;
        const bool f_ok = f == f && f < kBarrier;  // at or beyond the barrier a value counts as +inf
        any_finite_ |= f_ok;
        if (!f_ok) f = kBarrier;
        nfvals_++;
        double resmax = 0.0, viol = -std::numeric_limits<double>::infinity();
        bool c_ok = true;
        for (int k = 0; k < m_; k++) {
            double ck = c[k];
            if (!(ck == ck) || ck > kBarrier) ck = kBarrier, c_ok = false;
            if (ck < -kBarrier) ck = -kBarrier;
            con_[k] = -ck;
            resmax = std::fmax(resmax, ck);
            viol = std::fmax(viol, ck - cfeas_[k]);
        }
        for (int i = 0; i < n_; i++) {  // the bounds, on the UNclamped point
            con_[m_ + 2 * i] = x_[i] - lo_[i];
            con_[m_ + 2 * i + 1] = hi_[i] - x_[i];
            resmax = std::fmax(resmax, std::fmax(-con_[m_ + 2 * i], -con_[m_ + 2 * i + 1]));
            if (!clamp_eval_) viol = std::fmax(viol, std::fmax(-con_[m_ + 2 * i], -con_[m_ + 2 * i + 1]));
        }
        con_[mt_] = f;
        con_[mt_ + 1] = resmax;
        f_ = f;
        resmax_ = resmax;
        // the best evaluated point
        if (m_ == 0 && clamp_eval_) viol = 0.0;
        const bool feas = c_ok && !(viol > 0.0);
        bool better;
        if (!have_best_) better = true;
        else if (feas != bestfeas_) better = feas;
        else if (feas) better = f_ok && f < bestkey_;
        else better = viol < bestviol_;
        if (better) {
            have_best_ = true;
            bestfeas_ = feas;
            bestf_ = f_raw;
            bestkey_ = f_ok ? f : std::numeric_limits<double>::infinity();
            bestviol_ = viol;
            bestx_ = xout_;
            for (int k = 0; k < m_; k++) bestc_[k] = c[k];
        }
        label_ = L_AFTER_EVAL;
        run();
    }

    Status status() const { return status_; }
    int64_t evals() const { return nfvals_; }
    double best_f() const { return bestf_; }       // as told, bit for bit
    double best_key() const { return bestkey_; }   // what the ordering compares: best_f, +inf at or beyond the barrier
    bool any_finite_f() const { return any_finite_; }
    const std::vector<double> &best_x() const { return bestx_; }
    const std::vector<double> &best_c() const { return bestc_; }
    bool best_feasible() const { return have_best_ && bestfeas_; }
    double best_violation() const { return bestviol_; }  // max_j (c_j - cfeas_j) of the best point
    double final_f() const { return finalf_; }
    std::vector<double> final_x() const {
        std::vector<double> r(n_);
        for (int i = 0; i < n_; i++) r[i] = (clamp_eval_ ? std::fmin(hi_[i], std::fmax(lo_[i], finalx_[i])) : finalx_[i]) * scale_;
        return r;
    }
    const std::vector<double> &final_c() const { return finalc_; }  // the nonlinear constraints there (c_j <= 0 feasible)

private:
    static constexpr double kBarrier = 1e30;
    enum Label { L_EVAL, L_AFTER_EVAL, L140, L370, L440, L550, L_DONE };
    int n_, m_, mt_;  // variables, nonlinear constraints, all constraints (m + 2n)
    double scale_, ftol_rel_, ftol_abs_;
    int64_t maxfun_;
    double rhoend_;
    bool rho_doubling_, clamp_eval_;
    std::vector<double> cfeas_, lo_, hi_, x_, sim_, simi_, datmat_, con_, cb_, a_, vsig_, veta_, sigbar_, dx_;
    std::vector<double> z_, zdota_, vmultc_, vmultd_, sdirn_, dxnew_, xout_, bestx_, bestc_, finalx_, finalc_;
    std::vector<int> iact_;
    double rho_ = 1.0, parmu_ = 0.0, f_ = 0.0, resmax_ = 0.0, prerec_ = 0.0, prerem_ = 0.0, parsig_ = 0.0;
    double minf_ = std::numeric_limits<double>::infinity();
    double bestf_ = std::numeric_limits<double>::infinity(), bestviol_ = std::numeric_limits<double>::infinity();
    double bestkey_ = std::numeric_limits<double>::infinity();
    bool any_finite_ = false;
    double finalf_ = std::numeric_limits<double>::infinity();
    bool have_best_ = false, bestfeas_ = false;
    int jdrop_ = 0, ibrnch_ = 0, iflag_ = 0, ifull_ = 0;
    int64_t nfvals_ = 0;
    Label label_ = L_EVAL;
    Status status_ = RUNNING;

    double &sim(int i, int j) { return sim_[(size_t)i * (n_ + 1) + j]; }
    double &simi(int i, int j) { return simi_[(size_t)i * n_ + j]; }
    double &datmat(int k, int j) { return datmat_[(size_t)k * (n_ + 1) + j]; }  // k: constraints, then f (mt_), resmax (mt_ + 1)
    double &a(int i, int k) { return a_[(size_t)k * n_ + i]; }                  // column k: gradient of constraint k; mt_: -grad f
    double &z(int i, int k) { return z_[(size_t)k * n_ + i]; }

    bool invert_simplex() {
        const int n = n_;
        std::vector<double> w((size_t)n * 2 * n, 0.0);
        for (int i = 0; i < n; i++) {
            for (int j = 0; j < n; j++) w[(size_t)i * 2 * n + j] = sim(i, j);
            w[(size_t)i * 2 * n + n + i] = 1.0;
        }
        for (int c = 0; c < n; c++) {
            int piv = c;
            for (int r = c + 1; r < n; r++)
                if (std::fabs(w[(size_t)r * 2 * n + c]) > std::fabs(w[(size_t)piv * 2 * n + c])) piv = r;
            if (w[(size_t)piv * 2 * n + c] == 0.0) return false;
            if (piv != c)
                for (int j = 0; j < 2 * n; j++) std::swap(w[(size_t)piv * 2 * n + j], w[(size_t)c * 2 * n + j]);
            const double inv = 1.0 / w[(size_t)c * 2 * n + c];
            for (int j = 0; j < 2 * n; j++) w[(size_t)c * 2 * n + j] *= inv;
            for (int r = 0; r < n; r++)
                if (r != c) {
                    const double f = w[(size_t)r * 2 * n + c];
                    if (f != 0.0)
                        for (int j = 0; j < 2 * n; j++) w[(size_t)r * 2 * n + j] -= f * w[(size_t)c * 2 * n + j];
                }
        }
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) simi(i, j) = w[(size_t)i * 2 * n + n + j];
        return true;
    }

    void finish(Status s) {
        status_ = s;
        label_ = L_DONE;
        finalx_.resize(n_);
        if (s == RHOEND && ifull_ == 1) {  // Powell returns the last trial point itself in this case
            finalx_ = x_;
            finalf_ = f_;
            for (int k = 0; k < m_; k++) finalc_[k] = -con_[k];
            return;
        }
        for (int i = 0; i < n_; i++) finalx_[i] = sim(i, n_);
        finalf_ = datmat(mt_, n_);
        for (int k = 0; k < m_; k++) finalc_[k] = -datmat(k, n_);
    }

    // a sum whose rounding error may exceed it counts as zero (Powell's ACCA / ACCB test)
    static bool negligible(double sum_abs, double sum) {
        const double acca = sum_abs + 0.1 * std::fabs(sum), accb = sum_abs + 0.2 * std::fabs(sum);
        return sum_abs >= acca || acca >= accb;
    }

    // the constraint at position k of the active list moves to position nact - 1, the ones behind it one place forward
    void rotate_to_end(int k, int nact) {
        const int n = n_;
        const int isave = iact_[k];
        const double vsave = vmultc_[k];
        for (; k < nact - 1; k++) {
            const int kp = k + 1, kw = iact_[kp];
            double sp = 0.0;
            for (int i = 0; i < n; i++) sp += z(i, k) * a(i, kw);
            double temp = std::sqrt(sp * sp + zdota_[kp] * zdota_[kp]);
            const double alpha = zdota_[kp] / temp, beta = sp / temp;
            zdota_[kp] = alpha * zdota_[k];
            zdota_[k] = temp;
            for (int i = 0; i < n; i++) {
                temp = alpha * z(i, kp) + beta * z(i, k);
                z(i, kp) = alpha * z(i, k) - beta * z(i, kp);
                z(i, k) = temp;
            }
            iact_[k] = kw;
            vmultc_[k] = vmultc_[kp];
        }
        iact_[k] = isave;
        vmultc_[k] = vsave;
    }

    // Powell's TRSTLP: dx_ <- the step from the pole, ifull_ <- 1 when |dx| = rho.  Constraint k of the linear models reads
    // a(:, k) . dx >= cb_[k] (k < mt_); column mt_ of a is -grad f.
    void trstlp() {
        const int n = n_, m = mt_;
        const double rho = rho_;
        int mcon = m, nact = 0, icon = 0, nactx = 0, icount = 0;
        double resmax = 0.0, resold = 0.0, optold = 0.0, step = 0.0, stpful = 0.0;
        ifull_ = 1;
        for (int i = 0; i < n; i++) {
            for (int j = 0; j < n; j++) z(i, j) = 0.0;
            z(i, i) = 1.0;
            dx_[i] = 0.0;
            sdirn_[i] = 0.0;
        }
        for (int k = 0; k < m; k++)
            if (cb_[k] > resmax) {
                resmax = cb_[k];
                icon = k;
            }
        for (int k = 0; k < m; k++) {
            iact_[k] = k;
            vmultc_[k] = resmax - cb_[k];
        }
        bool stage_start = true;  // the counters of the "three iterations without progress" rule start afresh
        int64_t iter = 0;
        if (resmax == 0.0) goto L480;
        for (;; iter++) {
            if (iter > 1000 + 200 * (int64_t)(m + n)) goto L490;  // (never met on the test problems: a guard against cycling)
            if (stage_start) {
                optold = 0.0;
                icount = 0;
                stage_start = false;
            }
            {
                double optnew;
                if (mcon == m) {
                    optnew = resmax;
                } else {
                    optnew = 0.0;
                    for (int i = 0; i < n; i++) optnew -= dx_[i] * a(i, mcon - 1);
                }
                if (icount == 0 || optnew < optold) {
                    optold = optnew;
                    nactx = nact;
                    icount = 3;
                } else if (nact > nactx) {
                    nactx = nact;
                    icount = 3;
                } else {
                    icount--;
                    if (icount == 0) goto L490;
                }
            }
            if (icon >= nact) {  // the constraint at position icon joins the active set
                const int kk = iact_[icon];
                for (int i = 0; i < n; i++) dxnew_[i] = a(i, kk);
                double tot = 0.0;
                for (int k = n - 1; k >= nact; k--) {
                    double sp = 0.0, spabs = 0.0;
                    for (int i = 0; i < n; i++) {
                        const double temp = z(i, k) * dxnew_[i];
                        sp += temp;
                        spabs += std::fabs(temp);
                    }
                    if (negligible(spabs, sp)) sp = 0.0;
                    if (tot == 0.0) {
                        tot = sp;
                    } else {
                        const int kp = k + 1;
                        double temp = std::sqrt(sp * sp + tot * tot);
                        const double alpha = sp / temp, beta = tot / temp;
                        tot = temp;
                        for (int i = 0; i < n; i++) {
                            temp = alpha * z(i, k) + beta * z(i, kp);
                            z(i, kp) = alpha * z(i, kp) - beta * z(i, k);
                            z(i, k) = temp;
                        }
                    }
                }
                if (tot != 0.0) {  // it fits without a deletion
                    zdota_[nact] = tot;
                    vmultc_[icon] = vmultc_[nact];
                    vmultc_[nact] = 0.0;
                    nact++;
                } else {  // one active constraint has to make room: the ratio test on the multipliers
                    double ratio = -1.0;
                    int iout = -1;
                    for (int k = nact - 1; k >= 0; k--) {
                        double zdotv = 0.0, zdvabs = 0.0;
                        for (int i = 0; i < n; i++) {
                            const double temp = z(i, k) * dxnew_[i];
                            zdotv += temp;
                            zdvabs += std::fabs(temp);
                        }
                        if (!negligible(zdvabs, zdotv)) {
                            const double temp = zdotv / zdota_[k];
                            if (temp > 0.0 && iact_[k] < m) {
                                const double tempa = vmultc_[k] / temp;
                                if (ratio < 0.0 || tempa < ratio) {
                                    ratio = tempa;
                                    iout = k;
                                }
                            }
                            if (k >= 1) {
                                const int kw = iact_[k];
                                for (int i = 0; i < n; i++) dxnew_[i] -= temp * a(i, kw);
                            }
                            vmultd_[k] = temp;
                        } else {
                            vmultd_[k] = 0.0;
                        }
                    }
                    if (ratio < 0.0) goto L490;
                    for (int k = 0; k < nact; k++) vmultc_[k] = std::fmax(0.0, vmultc_[k] - ratio * vmultd_[k]);
                    if (iout < nact - 1) rotate_to_end(iout, nact);
                    double temp = 0.0;
                    for (int i = 0; i < n; i++) temp += z(i, nact - 1) * a(i, kk);
                    if (temp == 0.0) goto L490;
                    zdota_[nact - 1] = temp;
                    vmultc_[icon] = 0.0;
                    vmultc_[nact - 1] = ratio;
                }
                // the new constraint takes the last active position; in stage two the objective stays behind it
                iact_[icon] = iact_[nact - 1];
                iact_[nact - 1] = kk;
                if (mcon > m && kk != mcon - 1) {
                    const int k = nact - 2, l = nact - 1;
                    double sp = 0.0;
                    for (int i = 0; i < n; i++) sp += z(i, k) * a(i, kk);
                    double temp = std::sqrt(sp * sp + zdota_[l] * zdota_[l]);
                    const double alpha = zdota_[l] / temp, beta = sp / temp;
                    zdota_[l] = alpha * zdota_[k];
                    zdota_[k] = temp;
                    for (int i = 0; i < n; i++) {
                        temp = alpha * z(i, l) + beta * z(i, k);
                        z(i, l) = alpha * z(i, k) - beta * z(i, l);
                        z(i, k) = temp;
                    }
                    iact_[l] = iact_[k];
                    iact_[k] = kk;
                    std::swap(vmultc_[k], vmultc_[l]);
                }
                if (mcon > m) {
                    const double temp = 1.0 / zdota_[nact - 1];
                    for (int i = 0; i < n; i++) sdirn_[i] = temp * z(i, nact - 1);
                } else {  // stage one: the direction along which every active residual falls at the same rate
                    const int k2 = iact_[nact - 1];
                    double temp = 0.0;
                    for (int i = 0; i < n; i++) temp += sdirn_[i] * a(i, k2);
                    temp -= 1.0;
                    temp /= zdota_[nact - 1];
                    for (int i = 0; i < n; i++) sdirn_[i] -= temp * z(i, nact - 1);
                }
            } else {  // the constraint at position icon leaves the active set
                if (icon < nact - 1) rotate_to_end(icon, nact);
                nact--;
                if (mcon > m) {
                    const double temp = 1.0 / zdota_[nact - 1];
                    for (int i = 0; i < n; i++) sdirn_[i] = temp * z(i, nact - 1);
                } else {
                    double temp = 0.0;
                    for (int i = 0; i < n; i++) temp += sdirn_[i] * z(i, nact);
                    for (int i = 0; i < n; i++) sdirn_[i] -= temp * z(i, nact);
                }
            }
            // the step to the boundary of the ball, or the one that takes resmax to zero
            {
                double dd = rho * rho, sd = 0.0, ss = 0.0;
                for (int i = 0; i < n; i++) {
                    if (std::fabs(dx_[i]) >= rho * 1e-6) dd -= dx_[i] * dx_[i];
                    sd += dx_[i] * sdirn_[i];
                    ss += sdirn_[i] * sdirn_[i];
                }
                if (dd <= 0.0) goto L490;
                double temp = std::sqrt(ss * dd);
                if (std::fabs(sd) >= temp * 1e-6) temp = std::sqrt(ss * dd + sd * sd);
                stpful = dd / (temp + sd);
                step = stpful;
                if (mcon == m) {
                    const double acca = step + 0.1 * resmax, accb = step + 0.2 * resmax;
                    if (step >= acca || acca >= accb) goto L480;
                    step = std::fmin(step, resmax);
                }
            }
            for (int i = 0; i < n; i++) dxnew_[i] = dx_[i] + step * sdirn_[i];
            if (mcon == m) {
                resold = resmax;
                resmax = 0.0;
                for (int k = 0; k < nact; k++) {
                    const int kk = iact_[k];
                    double temp = cb_[kk];
                    for (int i = 0; i < n; i++) temp -= a(i, kk) * dxnew_[i];
                    resmax = std::fmax(resmax, temp);
                }
            }
            // vmultd: the multipliers that would hold at dxnew
            for (int k = nact - 1; k >= 0; k--) {
                double zdotw = 0.0, zdwabs = 0.0;
                for (int i = 0; i < n; i++) {
                    const double temp = z(i, k) * dxnew_[i];
                    zdotw += temp;
                    zdwabs += std::fabs(temp);
                }
                if (negligible(zdwabs, zdotw)) zdotw = 0.0;
                vmultd_[k] = zdotw / zdota_[k];
                if (k >= 1) {
                    const int kk = iact_[k];
                    for (int i = 0; i < n; i++) dxnew_[i] -= vmultd_[k] * a(i, kk);
                }
            }
            if (mcon > m) vmultd_[nact - 1] = std::fmax(0.0, vmultd_[nact - 1]);
            // ... and the residuals of the inactive constraints there
            for (int i = 0; i < n; i++) dxnew_[i] = dx_[i] + step * sdirn_[i];
            for (int k = nact; k < mcon; k++) {
                const int kk = iact_[k];
                double sum = resmax - cb_[kk], sumabs = resmax + std::fabs(cb_[kk]);
                for (int i = 0; i < n; i++) {
                    const double temp = a(i, kk) * dxnew_[i];
                    sum += temp;
                    sumabs += std::fabs(temp);
                }
                if (negligible(sumabs, sum)) sum = 0.0;
                vmultd_[k] = sum;
            }
            // the fraction of the step that keeps every multiplier and residual non-negative
            {
                double ratio = 1.0;
                icon = -1;
                for (int k = 0; k < mcon; k++)
                    if (vmultd_[k] < 0.0) {
                        const double temp = vmultc_[k] / (vmultc_[k] - vmultd_[k]);
                        if (temp < ratio) {
                            ratio = temp;
                            icon = k;
                        }
                    }
                const double temp = 1.0 - ratio;
                for (int i = 0; i < n; i++) dx_[i] = temp * dx_[i] + ratio * dxnew_[i];
                for (int k = 0; k < mcon; k++) vmultc_[k] = std::fmax(0.0, temp * vmultc_[k] + ratio * vmultd_[k]);
                if (mcon == m) resmax = resold + ratio * (resmax - resold);
            }
            if (icon >= 0) continue;
            if (step == stpful) return;
        L480:  // stage two: the objective joins as the last "constraint"
            mcon = m + 1;
            icon = mcon - 1;
            iact_[mcon - 1] = mcon - 1;
            vmultc_[mcon - 1] = 0.0;
            stage_start = true;
            continue;
        L490:
            if (mcon == m) goto L480;
            ifull_ = 0;
            return;
        }
    }

    void run() {
        const int n = n_, np = n_, m = mt_, mp = mt_, mpp = mt_ + 1;
        const double alpha = 0.25, beta = 2.1, gamma = 0.5, delta = 1.1;
        for (;;) {
            switch (label_) {
            case L_EVAL:
            case L_DONE:
                return;
            case L_AFTER_EVAL: {
                if (ibrnch_ == 1) {
                    label_ = L440;
                    break;
                }
                for (int k = 0; k <= mpp; k++) datmat(k, jdrop_) = con_[k];
                if (nfvals_ <= np + 1) {
                    if (jdrop_ < n) {
                        if (datmat(mp, np) <= f_) {
                            x_[jdrop_] = sim(jdrop_, np);
                        } else {  // the new point becomes the pole
                            const double step = sim(jdrop_, jdrop_);
                            sim(jdrop_, np) = x_[jdrop_];
                            for (int k = 0; k <= mpp; k++) {
                                datmat(k, jdrop_) = datmat(k, np);
                                datmat(k, np) = con_[k];
                            }
                            for (int k = 0; k <= jdrop_; k++) sim(jdrop_, k) = -step;
                        }
                    }
                    if (nfvals_ <= n) {
                        jdrop_ = (int)nfvals_ - 1;
                        double step = rho_;  // flipped / shortened so that the vertex stays inside the box (NLopt)
                        const double xj = x_[jdrop_];
                        if (clamp_eval_ && xj + step > hi_[jdrop_]) {
                            if (xj - step >= lo_[jdrop_]) step = -step;
                            else if (hi_[jdrop_] - xj > xj - lo_[jdrop_]) step = 0.5 * (hi_[jdrop_] - xj);
                            else step = -0.5 * (xj - lo_[jdrop_]);
                        }
                        if (step == 0.0) step = rho_;
                        x_[jdrop_] += step;
                        sim(jdrop_, jdrop_) = step;
                        label_ = L_EVAL;
                        return;
                    }
                    if (!invert_simplex()) {
                        finish(ROUNDOFF);
                        return;
                    }
                }
                ibrnch_ = 1;
                label_ = L140;
                break;
            }
            case L140: {
                double phimin = datmat(mp, np) + parmu_ * datmat(mpp, np);
                int nbest = np;
                for (int j = 0; j < n; j++) {
                    const double temp = datmat(mp, j) + parmu_ * datmat(mpp, j);
                    if (temp < phimin) {
                        nbest = j;
                        phimin = temp;
                    } else if (temp == phimin && parmu_ == 0.0 && datmat(mpp, j) < datmat(mpp, nbest)) {
                        nbest = j;
                    }
                }
                if (nbest < n) {
                    for (int k = 0; k <= mpp; k++) std::swap(datmat(k, np), datmat(k, nbest));
                    for (int i = 0; i < n; i++) {
                        const double temp = sim(i, nbest);
                        sim(i, nbest) = 0.0;
                        sim(i, np) += temp;
                        double tempa = 0.0;
                        for (int k = 0; k < n; k++) {
                            sim(i, k) -= temp;
                            tempa -= simi(k, i);
                        }
                        simi(nbest, i) = tempa;
                    }
                }
                double error = 0.0;
                for (int i = 0; i < n; i++)
                    for (int j = 0; j < n; j++) {
                        double temp = (i == j) ? -1.0 : 0.0;
                        for (int k = 0; k < n; k++) temp += simi(i, k) * sim(k, j);
                        error = std::fmax(error, std::fabs(temp));
                    }
                if (!(error <= 0.1)) {
                    finish(ROUNDOFF);
                    return;
                }
                // linear models of the constraints and of f (the latter negated: TRSTLP treats it as one more constraint)
                for (int k = 0; k <= mp; k++) {
                    cb_[k] = -datmat(k, np);
                    for (int i = 0; i < n; i++) {
                        double temp = 0.0;
                        for (int j = 0; j < n; j++) temp += (datmat(k, j) + cb_[k]) * simi(j, i);
                        a(i, k) = (k == mp) ? -temp : temp;
                    }
                }
                iflag_ = 1;
                parsig_ = alpha * rho_;
                const double pareta = beta * rho_;
                for (int j = 0; j < n; j++) {
                    double wsig = 0.0, weta = 0.0;
                    for (int i = 0; i < n; i++) {
                        wsig += simi(j, i) * simi(j, i);
                        weta += sim(i, j) * sim(i, j);
                    }
                    vsig_[j] = 1.0 / std::sqrt(wsig);
                    veta_[j] = std::sqrt(weta);
                    if (vsig_[j] < parsig_ || veta_[j] > pareta) iflag_ = 0;
                }
                if (ibrnch_ == 1 || iflag_ == 1) {
                    label_ = L370;
                    break;
                }
                int jd = -1;
                double temp = pareta;
                for (int j = 0; j < n; j++)
                    if (veta_[j] > temp) {
                        jd = j;
                        temp = veta_[j];
                    }
                if (jd < 0)
                    for (int j = 0; j < n; j++)
                        if (vsig_[j] < temp) {
                            jd = j;
                            temp = vsig_[j];
                        }
                jdrop_ = jd;
                temp = gamma * rho_ * vsig_[jd];
                for (int i = 0; i < n; i++) dx_[i] = temp * simi(jd, i);
                double cvmaxp = 0.0, cvmaxm = 0.0, sum = 0.0;
                for (int k = 0; k <= mp; k++) {
                    sum = 0.0;
                    for (int i = 0; i < n; i++) sum += a(i, k) * dx_[i];
                    if (k < mp) {
                        const double t2 = datmat(k, np);
                        cvmaxp = std::fmax(cvmaxp, -sum - t2);
                        cvmaxm = std::fmax(cvmaxm, sum - t2);
                    }
                }
                const double dxsign = (parmu_ * (cvmaxp - cvmaxm) > sum + sum) ? -1.0 : 1.0;
                temp = 0.0;
                for (int i = 0; i < n; i++) {
                    dx_[i] *= dxsign;
                    sim(i, jd) = dx_[i];
                    temp += simi(jd, i) * dx_[i];
                }
                for (int i = 0; i < n; i++) simi(jd, i) /= temp;
                for (int j = 0; j < n; j++) {
                    if (j != jd) {
                        double t2 = 0.0;
                        for (int i = 0; i < n; i++) t2 += simi(j, i) * dx_[i];
                        for (int i = 0; i < n; i++) simi(j, i) -= t2 * simi(jd, i);
                    }
                    x_[j] = sim(j, np) + dx_[j];
                }
                label_ = L_EVAL;
                return;
            }
            case L370: {
                trstlp();
                if (ifull_ == 0) {
                    double temp = 0.0;
                    for (int i = 0; i < n; i++) temp += dx_[i] * dx_[i];
                    if (temp < rho_ * 0.25 * rho_) {
                        ibrnch_ = 1;
                        label_ = L550;
                        break;
                    }
                }
                // predicted change of f and of the greatest violation
                double resnew = 0.0, sum = 0.0;
                cb_[mp] = 0.0;
                for (int k = 0; k <= mp; k++) {
                    sum = cb_[k];
                    for (int i = 0; i < n; i++) sum -= a(i, k) * dx_[i];
                    if (k < mp) resnew = std::fmax(resnew, sum);
                }
                double barmu = 0.0;
                prerec_ = datmat(mpp, np) - resnew;
                if (prerec_ > 0.0) barmu = sum / prerec_;
                if (parmu_ < barmu * 1.5) {
                    parmu_ = barmu * 2.0;
                    const double phi = datmat(mp, np) + parmu_ * datmat(mpp, np);
                    bool again = false;
                    for (int j = 0; j < n && !again; j++) {
                        const double temp = datmat(mp, j) + parmu_ * datmat(mpp, j);
                        if (temp < phi) again = true;
                        else if (temp == phi && parmu_ == 0.0 && datmat(mpp, j) < datmat(mpp, np)) again = true;
                    }
                    if (again) {
                        label_ = L140;
                        break;
                    }
                }
                prerem_ = parmu_ * prerec_ - sum;
                for (int i = 0; i < n; i++) x_[i] = sim(i, np) + dx_[i];
                ibrnch_ = 1;
                label_ = L_EVAL;
                return;
            }
            case L440: {
                const double vmold = datmat(mp, np) + parmu_ * datmat(mpp, np);
                const double vmnew = f_ + parmu_ * resmax_;
                double trured = vmold - vmnew;
                if (parmu_ == 0.0 && f_ == datmat(mp, np)) {
                    prerem_ = prerec_;
                    trured = datmat(mpp, np) - resmax_;
                }
                double ratio = (trured <= 0.0) ? 1.0 : 0.0;
                int jd = -1;
                for (int j = 0; j < n; j++) {
                    double temp = 0.0;
                    for (int i = 0; i < n; i++) temp += simi(j, i) * dx_[i];
                    temp = std::fabs(temp);
                    if (temp > ratio) {
                        jd = j;
                        ratio = temp;
                    }
                    sigbar_[j] = temp * vsig_[j];
                }
                double edgmax = delta * rho_;
                int l = -1;
                for (int j = 0; j < n; j++)
                    if (sigbar_[j] >= parsig_ || sigbar_[j] >= vsig_[j]) {
                        double temp = veta_[j];
                        if (trured > 0.0) {
                            temp = 0.0;
                            for (int i = 0; i < n; i++) temp += (dx_[i] - sim(i, j)) * (dx_[i] - sim(i, j));
                            temp = std::sqrt(temp);
                        }
                        if (temp > edgmax) {
                            l = j;
                            edgmax = temp;
                        }
                    }
                if (l >= 0) jd = l;
                if (jd < 0) {
                    label_ = L550;
                    break;
                }
                jdrop_ = jd;
                double temp = 0.0;
                for (int i = 0; i < n; i++) {
                    sim(i, jd) = dx_[i];
                    temp += simi(jd, i) * dx_[i];
                }
                for (int i = 0; i < n; i++) simi(jd, i) /= temp;
                for (int j = 0; j < n; j++)
                    if (j != jd) {
                        double t2 = 0.0;
                        for (int i = 0; i < n; i++) t2 += simi(j, i) * dx_[i];
                        for (int i = 0; i < n; i++) simi(j, i) -= t2 * simi(jd, i);
                    }
                for (int k = 0; k <= mpp; k++) datmat(k, jd) = con_[k];
                if (trured > 0.0 && trured >= prerem_ * 0.1) {
                    if (rho_doubling_ && trured >= prerem_ * 0.9 && trured <= prerem_ * 1.1 && iflag_) rho_ *= 2.0;
                    label_ = L140;
                    break;
                }
                label_ = L550;
                break;
            }
            case L550: {
                if (iflag_ == 0) {
                    ibrnch_ = 0;
                    label_ = L140;
                    break;
                }
                {
                    const double fb = (ifull_ == 1) ? f_ : datmat(mp, np);
                    if (fb < minf_ && (ftol_rel_ > 0.0 || ftol_abs_ > 0.0)) {
                        const double d = std::fabs(fb - minf_);
                        if (std::isfinite(minf_) && (d < ftol_abs_ || d < ftol_rel_ * (std::fabs(fb) + std::fabs(minf_)) * 0.5 || fb == minf_)) {
                            finish(FTOL);
                            return;
                        }
                    }
                    minf_ = fb;
                }
                if (rho_ > rhoend_) {
                    rho_ *= 0.5;
                    if (rho_ <= rhoend_ * 1.5) rho_ = rhoend_;
                    if (parmu_ > 0.0) {
                        double denom = 0.0, cmin = 0.0, cmax = 0.0;
                        for (int k = 0; k <= mp; k++) {
                            cmin = cmax = datmat(k, np);
                            for (int j = 0; j < n; j++) {
                                cmin = std::fmin(cmin, datmat(k, j));
                                cmax = std::fmax(cmax, datmat(k, j));
                            }
                            if (k < m && cmin < cmax * 0.5) {
                                const double temp = std::fmax(cmax, 0.0) - cmin;
                                denom = (denom <= 0.0) ? temp : std::fmin(denom, temp);
                            }
                        }
                        if (denom == 0.0) parmu_ = 0.0;
                        else if (cmax - cmin < parmu_ * denom) parmu_ = (cmax - cmin) / denom;
                    }
                    label_ = L140;
                    break;
                }
                finish(RHOEND);
                return;
            }
            }
        }
    }
};


}  // namespace egx
