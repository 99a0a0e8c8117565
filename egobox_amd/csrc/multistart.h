// The lock-step multistart of the infill optimisers (infill_optimize.hip) and of the hyperparameter fits (gp_fit.hip,
// sgp_host.hip through fit_starts.h), without HIP: every start is one resumable (ask / tell) machine -- CobylaBox, Cobyla
// (cobyla.h), Slsqp (slsqp.h) or LbfgsStart (lbfgs.h) -- and a ROUND hands the points all unfinished machines ask for to ONE
// evaluation, then tells every machine its answer (the reference runs its starts one after the other,
// crates/ego/src/solver/solver_infill_optim.rs:206-236, or as rayon tasks, crates/gp/src/algorithm.rs:928-945).  A machine sees
// only its own points and values, so a start walks bit for bit the points it walks alone, whatever its companions do.
// Beside the round loop, for the infill optimisers (the fits': fit_starts.h): the argument check of the three entry points
// with its messages, the evaluation budget's default, and the two rules that pick the winning start.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include <utility>
#include <vector>

namespace egx {
namespace multistart {

// finite bounds with lo <= hi, finite start coordinates (x_start: n_start x d); false with the message in msg
inline bool check_box_and_starts(const double *lo, const double *hi, const double *x_start, int64_t n_start, int d, std::string &msg) {
    for (int i = 0; i < d; i++)
        if (!(lo[i] <= hi[i]) || std::isinf(lo[i]) || std::isinf(hi[i])) {
            msg = "infill optimize: bounds must be finite with lo <= hi (coordinate " + std::to_string(i) + ")";
            return false;
        }
    for (int64_t s = 0; s < n_start; s++)
        for (int i = 0; i < d; i++)
            if (!std::isfinite(x_start[s * d + i])) {
                msg = "infill optimize: start point " + std::to_string(s) + " has a non-finite coordinate";
                return false;
            }
    return true;
}

// at most min(10 n_start d, 2000) evaluations per start unless the caller says otherwise (solver_infill_optim.rs:217-221)
inline int64_t budget(int64_t max_eval, int64_t n_start, int d) {
    return max_eval > 0 ? max_eval : std::min<int64_t>(10 * n_start * d, 2000);
}

// the points of one round: point q (pts + q d) was asked by machine who[q]; machine-index order
struct Round {
    std::vector<double> pts;
    std::vector<size_t> who;
    size_t size() const { return who.size(); }
};

// Slsqp::ask has a want_grad out-parameter (always true: every point is asked with its gradient), the COBYLA machines have none
template <class Machine>
auto ask(Machine &m, std::vector<double> &x, int) -> decltype(m.ask(x, std::declval<bool &>())) {
    bool want_grad = true;
    return m.ask(x, want_grad);
}
template <class Machine>
bool ask(Machine &m, std::vector<double> &x, long) {
    return m.ask(x);
}

// All machines in LOCK-STEP until none asks any more.  eval(round) -> rc evaluates the round's points in ONE call into scratch of
// its own; tell(round, q, machine) hands point q's answer to the machine that asked.  Returns the number of rounds; a failed
// evaluation ends the loop with its code in rc and nothing told.
template <class Machine, class Eval, class Tell>
int64_t run(std::vector<Machine> &mach, Eval &&eval, Tell &&tell, int &rc) {
    Round r;
    const Round &round = r;  // what eval and tell see
    std::vector<double> x;
    int64_t rounds = 0;
    for (rc = 0;;) {
        r.pts.clear();
        r.who.clear();
        for (size_t s = 0; s < mach.size(); s++)
            if (ask(mach[s], x, 0)) {
                r.who.push_back(s);
                r.pts.insert(r.pts.end(), x.begin(), x.end());
            }
        if (r.who.empty()) return rounds;
        rc = eval(round);
        if (rc) return rounds;
        rounds++;
        for (size_t q = 0; q < r.size(); q++) tell(round, q, mach[r.who[q]]);
    }
}

// The ordering of the machines that keep their best EVALUATED point (Cobyla, Slsqp): a strictly better than b when it is feasible
// and b is not, else by the smaller objective (both feasible) or the smaller violation max_j (c_j - cstr_tol_j / scale_cstr_j)
// (both infeasible).  The reference returns every run's final vertex and takes the smallest objective, feasible or not
// (solver_infill_optim.rs:229-232).
template <class Machine>
bool better(const Machine &a, const Machine &b) {
    if (a.best_feasible() != b.best_feasible()) return a.best_feasible();
    return a.best_feasible() ? a.best_key() < b.best_key() : a.best_violation() < b.best_violation();
}

template <class Machine>
bool any_finite(const std::vector<Machine> &mach) {
    bool any = false;
    for (const Machine &m : mach) any |= m.any_finite_f();
    return any;
}

// the winning start in that ordering, the first on ties; compare = false: start 0 whatever the others hold
template <class Machine>
int64_t winner(const std::vector<Machine> &mach, bool compare = true) {
    size_t best = 0;
    for (size_t s = 1; s < mach.size() && compare; s++)
        if (better(mach[s], mach[best])) best = s;
    return (int64_t)best;
}

// The best EVALUATED point of every start for a machine that does not keep it (CobylaBox): the smallest value told, the first on
// ties; NaN and values at or beyond COBYLA's 1e30 barrier count as +inf (optimizer.rs:153-157 style) and are never the best.
// Until a start meets a finite value its point is the start point clamped into the box.
struct BestEvaluated {
    int d;
    std::vector<double> f, x;  // n_start | n_start x d
    BestEvaluated(const double *lo, const double *hi, const double *x_start, int64_t n_start, int d_)
        : d(d_), f((size_t)n_start, std::numeric_limits<double>::infinity()), x((size_t)n_start * d_, 0.0) {
        for (int64_t s = 0; s < n_start; s++)
            for (int i = 0; i < d; i++) x[s * d + i] = std::fmin(hi[i], std::fmax(lo[i], x_start[s * d + i]));
    }
    void told(size_t s, double v, const double *pt) {
        if (v == v && v < 1e30 && v < f[s]) {
            f[s] = v;
            std::copy(pt, pt + d, x.begin() + s * d);
        }
    }
    int64_t winner() const {  // the first wins ties (solver_infill_optim.rs:229-236)
        size_t best = 0;
        for (size_t s = 1; s < f.size(); s++)
            if (f[s] < f[best]) best = s;
        return (int64_t)best;
    }
};

}  // namespace multistart
}  // namespace egx
