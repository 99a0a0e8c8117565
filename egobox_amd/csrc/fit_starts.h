// The rules every multistart hyperparameter fit shares, without HIP (compiles under g++, tests/c_host/fit_starts_test.cpp): the
// box in x = log10(parameter) with its checks and messages, COBYLA's evaluation budget, the machines of a list of starts, how a
// failed evaluation and a start's result read, the reduction over the starts and the winner's parameters.  The round loop is
// multistart::run (multistart.h): the dense fits (gp_fit.hip) run their starts in LOCK-STEP, one evaluation call per round; the
// sparse fits (sgp_host.hip) one start after the other (run_sequential) -- a sparse handle has ONE workspace, and the gradient
// reads what the likelihood of the same point left in it.
#pragma once
#include <string>

#include "cobyla.h"
#include "lbfgs.h"
#include "multistart.h"

namespace egx {

// outcome of one start of a multistart optimisation: objective (-likelihood), its minimiser in log10 parameters, evaluations
struct StartResult {
    double f;
    std::vector<double> x;
    int64_t evals;
};

namespace fit {

enum Model { Dense, Sparse };  // whose messages a failed check carries: callers show them to users

// the box in x = log10(parameter) (optimization.rs:32-35).  The L-BFGS machines point INTO it: it outlives them.
struct Log10Box {
    std::vector<double> lo, hi;
};

// lo / hi hold one value for all h parameters or h values (algorithm.rs:901-912), 0 < lo <= hi; false with the message in msg
inline bool log10_box(const double *lo, const double *hi, int64_t bounds_len, int h, Model what, Log10Box &box, std::string &msg) {
    if (bounds_len != 1 && bounds_len != h) {
        msg = "Bounds for theta should be either 1-dim or dim of xtrain (" + std::to_string(h) + "), got " + std::to_string(bounds_len);
        return false;
    }
    box.lo.resize((size_t)h);
    box.hi.resize((size_t)h);
    for (int i = 0; i < h; i++) {
        const double l = lo[bounds_len == 1 ? 0 : i], u = hi[bounds_len == 1 ? 0 : i];
        if (!(l > 0.0) || !(u >= l)) {
            msg = what == Dense ? "theta bounds must satisfy 0 < lo <= hi" : "sparse GP parameter bounds must satisfy 0 < lo <= hi";
            return false;
        }
        box.lo[(size_t)i] = std::log10(l);
        box.hi[(size_t)i] = std::log10(u);
    }
    return true;
}

// the start points are parameters, not their logarithms: all `count` values > 0
inline bool positive_starts(const double *x0s, int64_t count, Model what, std::string &msg) {
    for (int64_t e = 0; e < count; e++)
        if (!(x0s[e] > 0.0)) {
            msg = what == Dense ? "theta start points must be > 0" : "sparse GP start points must be > 0";
            return false;
        }
    return true;
}

// evaluations per COBYLA start: clamp(10 h, GP_COBYLA_MIN_EVAL = 25, max_eval); a max_eval below 25 is ignored
// (algorithm.rs:933-936, sparse_algorithm.rs:601-603)
inline int64_t cobyla_budget(int64_t h, int64_t max_eval) {
    int64_t per_start = 10 * h;
    if (per_start < 25) per_start = 25;
    if (max_eval >= 25 && per_start > max_eval) per_start = max_eval;
    return per_start;
}

// the starts of rank `rank` of `world`: s = rank, rank + world, ... (all of them for rank 0 of 1; none when n_starts <= rank)
inline std::vector<int64_t> shard(int64_t n_starts, int rank = 0, int world = 1) {
    std::vector<int64_t> mine;
    for (int64_t s = rank; s < n_starts; s += world) mine.push_back(s);
    return mine;
}
inline std::vector<int> all_active(int h) {
    std::vector<int> active((size_t)h);
    for (int i = 0; i < h; i++) active[(size_t)i] = i;
    return active;
}

// One COBYLA machine per row of `rows` (row s of x0s: h parameters), rhobeg 0.5 / ftol_rel 1e-4 as the reference configures it
// for the dense and the sparse model (optimization.rs:16-24, 122-169)
inline std::vector<CobylaBox> cobyla_machines(const double *x0s, int h, const std::vector<int64_t> &rows, const Log10Box &box,
                                              int64_t budget) {
    std::vector<CobylaBox> mach;
    std::vector<double> x0((size_t)h);
    for (int64_t s : rows) {
        for (int i = 0; i < h; i++) x0[(size_t)i] = std::log10(x0s[s * h + i]);
        mach.emplace_back(x0, box.lo, box.hi, 0.5, 1e-4, budget);
    }
    return mach;
}
// One projected L-BFGS machine per row of `rows`.  The machines keep pointers to the box: a temporary box does not compile.
inline std::vector<LbfgsStart> lbfgs_machines(const double *x0s, int h, const std::vector<int64_t> &rows, const Log10Box &box,
                                              int64_t max_iter) {
    std::vector<LbfgsStart> mach;
    for (int64_t s : rows) mach.emplace_back(x0s + s * h, h, box.lo, box.hi, max_iter);
    return mach;
}
std::vector<LbfgsStart> lbfgs_machines(const double *, int, const std::vector<int64_t> &, Log10Box &&, int64_t) = delete;

// theta (full width, preset by the caller) <- 10^x in the active components
inline void set_active(const double *x, const std::vector<int> &active, double *theta) {
    for (size_t i = 0; i < active.size(); i++) theta[active[i]] = std::pow(10.0, x[i]);
}
// the points of a round as rows of full-width theta: `base` (hfull) with 10^x in the active components
inline void round_thetas(const multistart::Round &r, const double *base, int hfull, const std::vector<int> &active,
                         std::vector<double> &thetas) {
    thetas.clear();
    for (size_t q = 0; q < r.size(); q++) {
        thetas.insert(thetas.end(), base, base + hfull);
        set_active(r.pts.data() + q * active.size(), active, thetas.data() + q * (size_t)hfull);
    }
}

// what a COBYLA machine is told for a likelihood: -L, +inf for an evaluation that failed or gave NaN (algorithm.rs:893-896)
inline double cobyla_objective(bool status_ok, double lkh) {
    return status_ok && !std::isnan(lkh) ? -lkh : std::numeric_limits<double>::infinity();
}
// a finished COBYLA start; NaN and COBYLA's own 1e30 barrier read +inf (optimization.rs:153-157)
inline StartResult cobyla_result(const CobylaBox &m) {
    double fb = m.best_f();
    if (std::isnan(fb) || fb >= 1e30) fb = std::numeric_limits<double>::infinity();
    return StartResult{fb, m.best_x(), m.evals()};
}

// The reduction over the starts (algorithm.rs:942-945): the start with the smallest finite f, the FIRST on ties; nullptr when
// no start ended finite.  NaN -- a start of another rank in a sharded fit's local vector -- is never the best.  *evals: the sum
// over all starts.
inline const StartResult *best_start(const std::vector<StartResult> &results, int64_t *evals = nullptr) {
    const StartResult *best = nullptr;
    double best_f = std::numeric_limits<double>::infinity();
    if (evals) *evals = 0;
    for (const StartResult &r : results) {
        if (evals) *evals += r.evals;
        if (r.f < best_f) best_f = r.f, best = &r;
    }
    return best;
}
// theta of the fitted model: `base` (hfull) with 10^x of the best start in the active components -- or, when every start
// failed (best == nullptr), with start 0's values theta0 (active.size() of them)
inline std::vector<double> winner_theta(const double *base, int hfull, const std::vector<int> &active, const StartResult *best,
                                        const double *theta0) {
    std::vector<double> th(base, base + hfull);
    if (best) set_active(best->x.data(), active, th.data());
    else
        for (size_t i = 0; i < active.size(); i++) th[(size_t)active[i]] = theta0[i];
    return th;
}

// The machines ONE AFTER THE OTHER, each a multistart::run of its own (rounds of one point): for an evaluation that cannot be
// interleaved.  A failed evaluation ends everything with its code in rc.
template <class Machine, class Eval, class Tell>
void run_sequential(std::vector<Machine> &mach, Eval &&eval, Tell &&tell, int &rc) {
    std::vector<Machine> one;
    rc = 0;
    for (size_t s = 0; s < mach.size() && !rc; s++) {
        one.assign(1, mach[s]);
        multistart::run(one, eval, tell, rc);
        mach[s] = std::move(one[0]);
    }
}

// A round over machines laid out START-MAJOR, model-minor (machine st k + m: start st of model m; egx_gp_fit_multi): per start
// index that has points, in increasing order, fn(st, q0, count) for its points q0 .. q0 + count - 1 -- they are contiguous, the
// models in increasing order.  Ends at the first non-zero return.
template <class Fn>
int for_each_start(const multistart::Round &r, int k, Fn &&fn) {
    for (size_t q0 = 0, q1 = 0; q0 < r.size(); q0 = q1) {
        const size_t st = r.who[q0] / (size_t)k;
        while (q1 < r.size() && r.who[q1] / (size_t)k == st) q1++;
        if (const int rc = fn((int64_t)st, q0, q1 - q0)) return rc;
    }
    return 0;
}

}  // namespace fit
}  // namespace egx
