// SLSQP for  minimise f(x)  subject to  c_j(x) <= cfeas_j (j < k)  and  lo <= x <= hi,  as a resumable (ask / tell)
// state machine: the optimiser behind egx_infill_optimize_slsqp (infill_optimize.hip).
//
// The reference's default inner optimiser is the `slsqp` crate (crates/ego/src/optimizers/optimizer.rs:169-204), a port of
// the SLSQP in NLopt, which is D. Kraft's "A software package for sequential quadratic programming" (DFVLR-FB 88-28, 1988).
// The crate is not vendored in the reference checkout, so this file restates the PUBLISHED algorithm, as cobyla.h does for
// Powell's:
//   * B, the approximation of the Lagrangian's Hessian, is kept as L D L^T (L packed by columns, the diagonal holding D),
//     starts from I and takes the BFGS update with Powell's damping (s^T y raised to 0.2 s^T B s) as two rank-one
//     modifications of the factor (Fletcher & Powell's composite-t method);
//   * the search direction solves  min 1/2 s^T B s + g^T s  s.t.  c + A s <= 0,  lo - x <= s <= hi - x  -- the bounds are
//     bounds of the STEP, so every iterate stays in the box;
//   * when that linearisation is inconsistent, the problem is augmented by a slack variable delta in [0, 1] that relaxes the
//     violated constraints, penalised by rho / 2 delta^2 (rho = 100, times 10 while still inconsistent);
//   * the merit function is  f + sum_j mu_j max(c_j, 0)  with  mu_j = max(|r_j|, (mu_j + |r_j|) / 2)  from the
//     subproblem's multipliers r, searched by Kraft's inexact rule: accept when the merit falls by a tenth of what its
//     directional derivative h3 promises, else alpha = max(h3 / (2 (h3 - dphi)), 0.1), at most 10 shortenings;
//   * a non-negative directional derivative resets B to I (at most four times, then the relaxed test with 10 acc).
// The quadratic subproblem follows Kraft's route LSQ -> LSI -> LDP -> NNLS (Lawson & Hanson 1974): with E = D^1/2 L^T the
// objective is 1/2 |E s - f|^2, the substitution z = E s - f leaves a least-distance problem, and that is a non-negative
// least squares problem whose residual gives z and whose solution gives the multipliers.  It is EXACT (an active-set
// method); its least squares solves are Householder QR on the passive columns.
//
// What differs from Kraft's driver:
//   * every point is asked WITH its gradient, so a line-search trial point that is accepted is not evaluated a second time
//     (his code returns mode -1 for a second call at the same x); evals() counts distinct points;
//   * an objective value that is NaN, or at or beyond 1e30, counts as +inf (as does a point with a non-finite constraint
//     value or gradient): at a trial point it shortens the step, at the start point it ends the run;
//   * the stop test takes ftol_abs for acc and adds the relative test |f - f_prev| <= ftol_rel |f| beside the absolute one;
//   * there is no iteration limit beside the evaluation budget.
// best_x / best_f / best_c: the best EVALUATED point, bit for bit as handed out and as told, in Cobyla's ordering: feasible
// (c_j <= cfeas_j for all j) beats infeasible, among feasible points the smaller f, among infeasible ones the smaller
// max_j (c_j - cfeas_j), the first point on ties.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace egx {

namespace slsqp_detail {

// position of the diagonal entry of column i in the packed factor (columns one after the other, n - i entries each)
inline size_t ldl_diag(int n, int i) { return (size_t)i * n - (size_t)i * (i - 1) / 2; }

// L D L^T + sigma z z^T by the composite-t method (Fletcher & Powell 1974; Kraft's LDL).  z is destroyed, w is scratch (n).
// A negative sigma must leave the matrix positive definite.
inline void ldl_update(int n, double *a, double *z, double sigma, double *w) {
    if (sigma == 0.0) return;
    size_t ij = 0;
    double t = 1.0 / sigma;
    if (sigma < 0.0) {  // prepare the negative update: the partial sums t_i, formed forwards and stored backwards
        for (int i = 0; i < n; i++) w[i] = z[i];
        for (int i = 0; i < n; i++) {
            const double v = w[i];
            t += v * v / a[ij];
            for (int j = i + 1; j < n; j++) {
                ij++;
                w[j] -= v * a[ij];
            }
            ij++;
        }
        if (t >= 0.0) t = std::numeric_limits<double>::epsilon() / sigma;
        for (int i = 0; i < n; i++) {
            const int j = n - 1 - i;
            ij -= (size_t)i + 1;
            const double u = w[j];
            w[j] = t;
            t -= u * u / a[ij];
        }
    }
    for (int i = 0; i < n; i++) {
        const double v = z[i], delta = v / a[ij];
        const double tp = sigma < 0.0 ? w[i] : t + delta * v;
        const double alpha = tp / t;
        a[ij] *= alpha;
        if (i == n - 1) return;
        const double beta = delta / tp;
        if (alpha > 4.0) {
            const double gamma = t / tp;
            for (int j = i + 1; j < n; j++) {
                ij++;
                const double u = a[ij];
                a[ij] = gamma * u + beta * z[j];
                z[j] -= v * u;
            }
        } else {
            for (int j = i + 1; j < n; j++) {
                ij++;
                z[j] -= v * a[ij];
                a[ij] += beta * z[j];
            }
        }
        ij++;
        t = tp;
    }
}

// min |E u - f| over u >= 0, E with `rows` rows and `cols` columns stored by columns (Lawson & Hanson's NNLS).  r: the
// residual E u - f.  Returns false when the iteration limit is reached.
inline bool nnls(int rows, int cols, const double *E, const double *f, double *u, double *r) {
    std::vector<int> P;  // the passive (positive) columns, in the order they entered
    std::vector<char> inP((size_t)cols, 0), barred((size_t)cols, 0);
    std::vector<double> z, Q, rhs, cn((size_t)cols);
    for (int j = 0; j < cols; j++) {
        u[j] = 0.0;
        double s = 0.0;
        for (int i = 0; i < rows; i++) s += E[(size_t)j * rows + i] * E[(size_t)j * rows + i];
        cn[j] = std::sqrt(s);
    }
    // least squares over the passive columns by Householder QR; false when the LAST column depends on the others
    auto solve_passive = [&]() {
        const int p = (int)P.size();
        Q.assign((size_t)rows * p, 0.0);
        rhs.assign(f, f + rows);
        for (int c = 0; c < p; c++)
            for (int i = 0; i < rows; i++) Q[(size_t)c * rows + i] = E[(size_t)P[c] * rows + i];
        for (int c = 0; c < p; c++) {
            double *col = &Q[(size_t)c * rows];
            double s = 0.0;
            for (int i = c; i < rows; i++) s += col[i] * col[i];
            const double nrm = std::sqrt(s);
            if (c == p - 1 && !(nrm > 1e-13 * cn[P[c]])) return false;
            if (nrm == 0.0) return false;
            const double alpha = col[c] > 0.0 ? -nrm : nrm;
            const double v0 = col[c] - alpha, vv = s - col[c] * col[c] + v0 * v0;  // v = (v0, col[c+1..]), |v|^2
            auto reflect = [&](double *y) {
                double dot = v0 * y[c];
                for (int i = c + 1; i < rows; i++) dot += col[i] * y[i];
                const double k = 2.0 * dot / vv;
                y[c] -= k * v0;
                for (int i = c + 1; i < rows; i++) y[i] -= k * col[i];
            };
            if (vv > 0.0) {
                for (int c2 = c + 1; c2 < p; c2++) reflect(&Q[(size_t)c2 * rows]);
                reflect(rhs.data());
            }
            col[c] = alpha;  // R's diagonal; the entries below keep v's tail, no longer read
        }
        z.assign((size_t)p, 0.0);
        for (int c = p - 1; c >= 0; c--) {
            double s = rhs[c];
            for (int c2 = c + 1; c2 < p; c2++) s -= Q[(size_t)c2 * rows + c] * z[c2];
            z[c] = s / Q[(size_t)c * rows + c];
        }
        return true;
    };
    auto residual = [&]() {
        for (int i = 0; i < rows; i++) r[i] = -f[i];
        for (int j : P)
            for (int i = 0; i < rows; i++) r[i] += E[(size_t)j * rows + i] * u[j];
    };
    residual();
    const int itmax = 3 * cols + 10;
    for (int it = 0;; it++) {
        if ((int)P.size() >= std::min(rows, cols)) return true;
        // the dual vector w = E^T (f - E u); the candidate is its largest positive entry among the columns at zero
        std::fill(barred.begin(), barred.end(), 0);
        int t = -1;
        for (;;) {
            t = -1;
            double wmax = 0.0;
            for (int j = 0; j < cols; j++) {
                if (inP[j] || barred[j]) continue;
                double s = 0.0;
                for (int i = 0; i < rows; i++) s -= E[(size_t)j * rows + i] * r[i];
                if (s > wmax) wmax = s, t = j;
            }
            if (t < 0) return true;  // Kuhn-Tucker: no column at zero can reduce the residual
            P.push_back(t);
            if (solve_passive() && z.back() > 0.0) break;
            P.pop_back();  // dependent on the passive columns, or its sign contradicts w by rounding: not a candidate now
            barred[t] = 1;
        }
        inP[t] = 1;
        if (it >= itmax) return false;
        for (int inner = 0;; inner++) {
            if (inner > itmax) return false;
            bool all_pos = true;
            double alpha = 2.0;
            int jdrop = -1;
            for (size_t c = 0; c < P.size(); c++)
                if (!(z[c] > 0.0)) {
                    all_pos = false;
                    const double a = u[P[c]] / (u[P[c]] - z[c]);
                    if (a < alpha) alpha = a, jdrop = (int)c;
                }
            if (all_pos) {
                for (size_t c = 0; c < P.size(); c++) u[P[c]] = z[c];
                break;
            }
            for (size_t c = 0; c < P.size(); c++) u[P[c]] += alpha * (z[c] - u[P[c]]);
            u[P[jdrop]] = 0.0;
            std::vector<int> keep;
            for (int j : P) {
                if (u[j] > 0.0) {
                    keep.push_back(j);
                } else {
                    u[j] = 0.0;
                    inP[j] = 0;
                }
            }
            P.swap(keep);
            if (P.empty()) break;
            while (!P.empty() && !solve_passive()) {  // (cannot happen for columns that were independent; kept finite)
                u[P.back()] = 0.0, inP[P.back()] = 0;
                P.pop_back();
            }
            if (P.empty()) break;
        }
        residual();
    }
}

// The strictly convex subproblem
//     min 1/2 s^T (L D L^T) s + g^T s    s.t.    A s + b >= 0  (m rows, A row-major m x n),   lo <= s <= hi
// by LSI -> LDP -> NNLS.  mult: the m + 2n multipliers (>= 0) of the general constraints, the lower and the upper bounds:
// B s + g = A^T mult_A + mult_lo - mult_hi.  Returns 0 (solved), 4 (the constraints are inconsistent), 3 (iteration limit).
inline int solve_qp(int n, const double *ldl, const double *g, int m, const double *A, const double *b, const double *lo,
                    const double *hi, double *s, double *mult) {
    const int M = m + 2 * n, rows = n + 1;
    std::vector<double> sd((size_t)n), f((size_t)n), E((size_t)rows * M), q((size_t)n), rhs((size_t)rows, 0.0), u((size_t)M),
        r((size_t)rows);
    auto L = [&](int j, int i) { return ldl[ldl_diag(n, i) + (size_t)(j - i)]; };  // j > i
    for (int i = 0; i < n; i++) sd[i] = std::sqrt(ldl[ldl_diag(n, i)]);
    for (int i = 0; i < n; i++) {  // f = -D^-1/2 L^-1 g
        double v = g[i];
        for (int j = 0; j < i; j++) v -= L(i, j) * f[j];
        f[i] = v;
    }
    for (int i = 0; i < n; i++) f[i] = -f[i] / sd[i];
    // a constraint q^T s >= h becomes (E^-T q)^T z >= h - (E^-T q)^T f  with  E^T = L D^1/2  lower triangular
    auto put = [&](int col, double h) {
        double *e = &E[(size_t)col * rows];
        double dot = 0.0;
        for (int i = 0; i < n; i++) {
            double v = q[i];
            for (int j = 0; j < i; j++) v -= L(i, j) * sd[j] * e[j];
            e[i] = v / sd[i];
            dot += e[i] * f[i];
        }
        e[n] = h - dot;
    };
    for (int j = 0; j < m; j++) {
        for (int i = 0; i < n; i++) q[i] = A[(size_t)j * n + i];
        put(j, -b[j]);
    }
    for (int i = 0; i < n; i++) {
        std::fill(q.begin(), q.end(), 0.0);
        q[i] = 1.0;
        put(m + i, lo[i]);
        q[i] = -1.0;
        put(m + n + i, -hi[i]);
    }
    rhs[n] = 1.0;
    if (!nnls(rows, M, E.data(), rhs.data(), u.data(), r.data())) return 3;
    // LDP: z = -r[0..n) / r[n], and at the minimum |r|^2 = -r[n] = 1 / (1 + |z|^2): the residual vanishes exactly when no z
    // satisfies the constraints.  |r|^2 is taken for both: next to zero -r[n] is rounding noise of the last row, while every
    // component of r keeps its absolute accuracy (~1e-16 for columns that NNLS has scaled to a combination of size 1).
    double fac = 0.0;
    for (int i = 0; i <= n; i++) fac += r[i] * r[i];
    if (!(fac > 1e-22)) return 4;
    for (int i = 0; i < n; i++) q[i] = r[i] / fac + f[i];  // z + f = E s
    for (int i = n - 1; i >= 0; i--) {                      // E = D^1/2 L^T, upper triangular
        double v = q[i] / sd[i];
        for (int j = i + 1; j < n; j++) v -= L(j, i) * s[j];
        s[i] = v;
    }
    for (int i = 0; i < n; i++) s[i] = std::fmin(hi[i], std::fmax(lo[i], s[i]));  // rounding only
    for (int j = 0; j < M; j++) mult[j] = u[j] / fac;
    return 0;
}

}  // namespace slsqp_detail

class Slsqp {
public:
    enum Status {
        RUNNING = 0,
        MAXEVAL = 1,       // the evaluation budget
        FTOL = 2,          // Kraft's convergence test
        LINESEARCH = 3,    // the line search can no longer move: no descent direction after the resets, or only +inf values
        NO_FINITE = 4,     // the start point has no finite value
        INCONSISTENT = 5,  // the augmented subproblem stayed inconsistent, or the subproblem solver hit its iteration limit
    };

    // x0, lo, hi in the caller's units; k constraints c_j(x) <= cfeas_j (cfeas: k thresholds, 0 when left out)
    Slsqp(const std::vector<double> &x0, const std::vector<double> &lo, const std::vector<double> &hi, int k, double ftol_rel,
          double ftol_abs, int64_t maxeval, const std::vector<double> &cfeas = {})
        : n_((int)x0.size()), m_(k), ftol_rel_(ftol_rel), acc_(ftol_abs), maxfun_(maxeval), cfeas_(cfeas), lo_(lo), hi_(hi) {
        const int n = n_, m = m_;
        cfeas_.resize((size_t)m, 0.0);
        x_.resize((size_t)n);
        for (int i = 0; i < n; i++) x_[i] = std::fmin(hi_[i], std::fmax(lo_[i], x0[i]));
        xc_ = x_, x0_ = x_;
        ldl_.assign((size_t)(n + 1) * (n + 2) / 2, 0.0);
        g_.assign((size_t)n + 1, 0.0);
        a_.assign((size_t)m * n, 0.0);
        c_.assign((size_t)m, 0.0);
        gn_ = g_, an_ = a_, cn_ = c_;
        s_.assign((size_t)n + 1, 0.0);
        r_.assign((size_t)m + 2 * (n + 1), 0.0);
        mu_.assign((size_t)m, 0.0);
        v_.assign((size_t)n, 0.0);
        u_.assign((size_t)n, 0.0);
        w_.assign((size_t)n, 0.0);
        bestx_.assign((size_t)n, 0.0);
        bestc_.assign((size_t)m, 0.0);
        reset_hessian();
    }

    // Next point to evaluate (inside the box); want_grad: the gradients are needed there (always).  False when finished.
    bool ask(std::vector<double> &x_out, bool &want_grad) {
        if (status_ != RUNNING) return false;
        if (nfvals_ >= maxfun_ && nfvals_ > 0) {
            status_ = MAXEVAL;
            return false;
        }
        want_grad = true;
        x_out = x_;
        return true;
    }

    // f, the k constraint values, grad f (n) and the Jacobian (k x n, row-major) at the point handed out by the last ask()
    void tell(double f, const double *c, const double *grad_f, const double *grad_c) {
        const int n = n_, m = m_;
        const bool f_ok = f == f && f < kBarrier;  // at or beyond the barrier a value counts as +inf
        any_finite_ |= f_ok;
        nfvals_++;
        bool c_ok = true, rest_ok = true;
        double viol = m > 0 ? -std::numeric_limits<double>::infinity() : 0.0;
        for (int j = 0; j < m; j++) {
            double cj = c[j];
            if (!(cj == cj) || cj > kBarrier) cj = kBarrier, c_ok = false;
            if (cj < -kBarrier) cj = -kBarrier, rest_ok = false;
            cn_[j] = cj - cfeas_[j];
            viol = std::fmax(viol, cn_[j]);
        }
        const bool feas = c_ok && !(viol > 0.0);
        bool better;
        if (!have_best_) better = true;
        else if (feas != bestfeas_) better = feas;
        else if (feas) better = f_ok && f < bestkey_;
        else better = viol < bestviol_;
        if (better) {
            have_best_ = true;
            bestfeas_ = feas;
            bestf_ = f;
            bestkey_ = f_ok ? f : std::numeric_limits<double>::infinity();
            bestviol_ = viol;
            bestx_ = x_;
            for (int j = 0; j < m; j++) bestc_[j] = c[j];
        }
        for (int i = 0; i < n; i++) rest_ok &= std::isfinite(gn_[i] = grad_f[i]);
        for (int i = 0; i < m * n; i++) rest_ok &= std::isfinite(an_[i] = grad_c[i]);
        const bool ok = f_ok && c_ok && rest_ok;
        if (!started_) {
            started_ = true;
            if (!ok) {
                status_ = NO_FINITE;
                return;
            }
            accept(f);
            major();
            return;
        }
        // Kraft's inexact line search on the merit function
        double t = ok ? f : std::numeric_limits<double>::infinity();
        if (ok)
            for (int j = 0; j < m; j++) t += mu_[j] * std::fmax(cn_[j], 0.0);
        const double h1 = t - t0_;
        if (!(h1 <= h3_ / 10.0) && line_ <= 10) {
            alpha_ = std::fmax(h3_ / (2.0 * (h3_ - h1)), 0.1);
            trial();
            return;
        }
        if (!ok) {  // ten shortenings and still no finite value
            x_ = xc_;
            status_ = LINESEARCH;
            return;
        }
        const double f_prev = f_;
        accept(f);
        double h3 = 0.0, snorm = 0.0;
        for (int j = 0; j < m; j++) h3 += std::fmax(c_[j], 0.0);
        for (int i = 0; i < n; i++) snorm += s_[i] * s_[i];
        const double df = std::fabs(f_ - f_prev);
        if ((df <= acc_ || df <= ftol_rel_ * std::fabs(f_) || std::sqrt(snorm) < acc_) && h3 < acc_) {
            status_ = FTOL;
            return;
        }
        bfgs();
        major();
    }

    Status status() const { return status_; }
    int64_t evals() const { return nfvals_; }      // distinct points asked and told
    int64_t iterations() const { return iter_; }   // major iterations begun
    int64_t accepted() const { return naccept_; }  // points that became the iterate (the start point is the first)
    int64_t augmented() const { return naug_; }    // major iterations whose linearisation was inconsistent
    const std::vector<double> &current_x() const { return xc_; }
    double current_f() const { return f_; }
    double best_f() const { return bestf_; }      // as told, bit for bit
    double best_key() const { return bestkey_; }  // what the ordering compares: best_f, +inf at or beyond the barrier
    bool any_finite_f() const { return any_finite_; }
    const std::vector<double> &best_x() const { return bestx_; }
    const std::vector<double> &best_c() const { return bestc_; }
    bool best_feasible() const { return have_best_ && bestfeas_; }
    double best_violation() const { return bestviol_; }  // max_j (c_j - cfeas_j) of the best point (0 without constraints)

private:
    static constexpr double kBarrier = 1e30;
    int n_, m_;
    double ftol_rel_, acc_;
    int64_t maxfun_;
    std::vector<double> cfeas_, lo_, hi_;
    std::vector<double> x_, xc_, x0_;       // the point asked, the iterate, the iterate the line search started from
    std::vector<double> ldl_;               // the packed factor, with room for the slack variable's column
    std::vector<double> g_, a_, c_;         // at the iterate: grad f (n + 1: the slack's entry), Jacobian, c - cfeas
    std::vector<double> gn_, an_, cn_;      // at the point told last
    std::vector<double> s_, r_, mu_, v_, u_, w_;
    std::vector<double> bestx_, bestc_;
    double f_ = 0.0, t0_ = 0.0, h3_ = 0.0, alpha_ = 1.0;
    double bestf_ = std::numeric_limits<double>::infinity(), bestviol_ = std::numeric_limits<double>::infinity();
    double bestkey_ = std::numeric_limits<double>::infinity();
    bool any_finite_ = false, have_best_ = false, bestfeas_ = false, started_ = false;
    int line_ = 0, ireset_ = 0;
    int64_t nfvals_ = 0, iter_ = 0, naccept_ = 0, naug_ = 0;
    Status status_ = RUNNING;

    void reset_hessian() {
        ireset_++;
        std::fill(ldl_.begin(), ldl_.end(), 0.0);
        for (int i = 0; i < n_; i++) ldl_[slsqp_detail::ldl_diag(n_, i)] = 1.0;
    }

    // the point told last becomes the iterate
    void accept(double f) {
        f_ = f;
        xc_ = x_;
        std::copy(gn_.begin(), gn_.begin() + n_, g_.begin());
        a_ = an_;
        c_ = cn_;
        naccept_++;
    }

    // the next line-search point: the step shortened by alpha_, the point kept in the box against rounding
    void trial() {
        line_++;
        h3_ *= alpha_;
        for (int i = 0; i < n_; i++) {
            s_[i] *= alpha_;
            x_[i] = std::fmin(hi_[i], std::fmax(lo_[i], x0_[i] + s_[i]));
        }
    }

    // One major iteration from the iterate: the subproblem, the multipliers, the first convergence test, the merit
    // function's directional derivative (resetting B while it is not negative), and the first trial point.
    void major() {
        const int n = n_, m = m_;
        std::vector<double> lo((size_t)n + 1), hi((size_t)n + 1), b((size_t)m), A;
        for (;;) {
            iter_++;
            for (int i = 0; i < n; i++) lo[i] = lo_[i] - xc_[i], hi[i] = hi_[i] - xc_[i];
            // Kraft states the constraints as c >= 0: his c is -c_ here, his Jacobian -a_
            for (int j = 0; j < m; j++) b[j] = -c_[j];
            A.assign((size_t)m * n, 0.0);
            for (size_t i = 0; i < A.size(); i++) A[i] = -a_[i];
            double h4 = 1.0;
            int mode = slsqp_detail::solve_qp(n, ldl_.data(), g_.data(), m, A.data(), b.data(), lo.data(), hi.data(), s_.data(),
                                              r_.data());
            if (mode == 4) {  // the augmented problem: a slack delta in [0, 1] relaxes the violated constraints
                naug_++;
                const int n1 = n + 1;
                std::vector<double> ldl1((size_t)n1 * (n1 + 1) / 2, 0.0), A1((size_t)m * n1);
                for (int i = 0; i < n; i++) {  // B's factor with one more row (zeros) and the column of the slack
                    const size_t src = slsqp_detail::ldl_diag(n, i), dst = slsqp_detail::ldl_diag(n1, i);
                    for (int j = 0; j < n - i; j++) ldl1[dst + j] = ldl_[src + j];
                }
                for (int j = 0; j < m; j++) {
                    for (int i = 0; i < n; i++) A1[(size_t)j * n1 + i] = A[(size_t)j * n + i];
                    A1[(size_t)j * n1 + n] = std::fmax(c_[j], 0.0);
                }
                g_[n] = 0.0, lo[n] = 0.0, hi[n] = 1.0;
                double rho = 100.0;
                std::vector<double> r1((size_t)m + 2 * n1);
                for (int incons = 0;; incons++) {
                    ldl1[slsqp_detail::ldl_diag(n1, n)] = rho;
                    mode = slsqp_detail::solve_qp(n1, ldl1.data(), g_.data(), m, A1.data(), b.data(), lo.data(), hi.data(),
                                                  s_.data(), r1.data());
                    if (mode != 4 || incons >= 5) break;
                    rho *= 10.0;
                }
                std::copy(r1.begin(), r1.begin() + m, r_.begin());
                h4 = 1.0 - s_[n];
            }
            if (mode != 0) {
                status_ = INCONSISTENT;
                return;
            }
            // the Lagrangian's gradient with these multipliers, kept for the BFGS update; Kraft's tests
            double gs = 0.0;
            for (int i = 0; i < n; i++) {
                double v = g_[i];
                for (int j = 0; j < m; j++) v += a_[(size_t)j * n + i] * r_[j];
                v_[i] = v;
                gs += g_[i] * s_[i];
            }
            double h1 = std::fabs(gs), h2 = 0.0;
            for (int j = 0; j < m; j++) {
                h2 += std::fmax(c_[j], 0.0);
                const double ar = std::fabs(r_[j]);
                mu_[j] = std::fmax(ar, (mu_[j] + ar) / 2.0);
                h1 += ar * std::fabs(c_[j]);
            }
            if (h1 < acc_ && h2 < acc_) {
                status_ = FTOL;
                return;
            }
            h1 = 0.0;
            for (int j = 0; j < m; j++) h1 += mu_[j] * std::fmax(c_[j], 0.0);
            t0_ = f_ + h1;
            h3_ = gs - h1 * h4;
            if (h3_ >= 0.0) {  // no descent for the merit function: start again from B = I, at most four times
                if (ireset_ + 1 > 5) {
                    // Kraft's relaxed test, 10 acc; |f - f0| is 0 here, and his h3 is this directional derivative
                    status_ = h3_ < 10.0 * acc_ ? FTOL : LINESEARCH;
                    return;
                }
                reset_hessian();
                continue;
            }
            x0_ = xc_;
            line_ = 0;
            alpha_ = 1.0;
            trial();
            return;
        }
    }

    // B <- B + y y^T / s^T y - B s s^T B / s^T B s  with Powell's damping, y the change of the Lagrangian's gradient
    void bfgs() {
        const int n = n_, m = m_;
        for (int i = 0; i < n; i++) {
            double v = g_[i];
            for (int j = 0; j < m; j++) v += a_[(size_t)j * n + i] * r_[j];
            u_[i] = v - v_[i];
        }
        auto L = [&](int j, int i) { return ldl_[slsqp_detail::ldl_diag(n, i) + (size_t)(j - i)]; };
        for (int i = 0; i < n; i++) {  // v = L D L^T s
            double h = s_[i];
            for (int j = i + 1; j < n; j++) h += L(j, i) * s_[j];
            v_[i] = h * ldl_[slsqp_detail::ldl_diag(n, i)];
        }
        for (int i = n - 1; i >= 0; i--) {
            double h = 0.0;
            for (int j = 0; j < i; j++) h += L(i, j) * v_[j];
            v_[i] += h;
        }
        double h1 = 0.0, h2 = 0.0;
        for (int i = 0; i < n; i++) h1 += s_[i] * u_[i], h2 += s_[i] * v_[i];
        const double h3 = 0.2 * h2;
        if (h1 < h3) {
            const double h4 = (h2 - h3) / (h2 - h1);
            h1 = h3;
            for (int i = 0; i < n; i++) u_[i] = h4 * u_[i] + (1.0 - h4) * v_[i];
        }
        if (!(h1 > 0.0) || !(h2 > 0.0)) return;  // a zero step (the box holds every coordinate): nothing to learn
        slsqp_detail::ldl_update(n, ldl_.data(), u_.data(), 1.0 / h1, w_.data());
        slsqp_detail::ldl_update(n, ldl_.data(), v_.data(), -1.0 / h2, w_.data());
    }
};

}  // namespace egx
