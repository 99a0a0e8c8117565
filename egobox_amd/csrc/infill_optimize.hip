// The lock-step multistarts of the infill criterion (crates/ego/src/solver/solver_infill_optim.rs:148-236) and the q-point batch
// call on top of them.  Every start is one ask / tell machine (cobyla.h, slsqp.h); multistart.h advances all of them in
// lock-step, and a round's points -- line-search trial points included -- are ONE evaluation of infill_eval.hip.  Each entry
// point: take the handle's lock, validate (the width of lo / hi / x_start is the activity's while one is set,
// egx_infill_set_active), take the models' locks, build the machines, run the rounds around eval_active, pick the winner, fill
// the stats.
//
// The three differ in these points ON PURPOSE (callers and tests observe them):
//  1. egx_infill_optimize keeps its OWN best evaluated point per start (multistart::BestEvaluated) and does not take
//     CobylaBox::best_x(): that is the pole of the final simplex, re-assembled by additions each time the pole moves, so it
//     need not be bit for bit a point that was evaluated -- and "f_best is egx_infill_eval at x_best" is part of this call's
//     contract.  NaN and values at or beyond 1e30 do not count, a start's point begins as the start point clamped into the box,
//     the first start wins ties, and the failure reads "no start ended at a finite value".
//  2. When no start met a finite value, egx_infill_optimize_cstr still picks its winner with multistart::better over all starts;
//     egx_infill_optimize_slsqp stays at start 0, whose only point is the start clamped into the box.  stats->best_start, x_best
//     and c_best follow.
//  3. Under EGX_CSTR_INFILL the constraint models are inside the objective: egx_infill_optimize_slsqp runs with k = 0 and
//     evaluates without a CstrOut, so its c_best check comes after the handle's lock (the strategy is read under it), with the
//     generic message.  egx_infill_optimize_cstr refuses EGX_CSTR_INFILL and checks c_best before the lock.
//  4. The scratch for constraint values and gradients is sized + 1, so that data() is non-null at k = 0.
//  5. stop[] exists in the SLSQP stats only; evals[] is filled only when non-null.
//  6. The COBYLA machines run with rhobeg 0.5, ftol_rel = ftol_abs = 1e-4, no rhoend, rho doubling, clamped evaluation
//     (optimizers/optimizer.rs:123-167, solver_infill_optim.rs:217-227: no constraint tolerances); SLSQP with ftol_rel =
//     ftol_abs = 1e-4.  A point is FEASIBLE when c_j <= cstr_tol_j / scale_cstr_j: Egor's acceptance tolerance in the units
//     of c, the constraint c_j - cstr_tol_j / scale_cstr_j <= 0 that optimizer.rs:188-199 hands to slsqp::minimize.
#include "infill_handle.h"
#include "multistart.h"
#include "slsqp.h"

using namespace egx;

namespace {

// the arguments the three entry points share; needs_c_best: a handle with constraints must be given c_best (checked here, before
// anything else).  Called under the handle's lock: the width of lo / hi / x_start is the activity's while one is set
int check_args(const egx_infill *h, const double *lo, const double *hi, const double *x_start, int64_t n_start, const double *f_best,
               const double *x_best, const double *c_best, bool needs_c_best) {
    if (!h || !lo || !hi || !x_start || !f_best || !x_best || n_start < 1 || (needs_c_best && h->surr.size() > 1 && !c_best))
        return fail(EGX_ERR_INVALID_VALUE, "infill optimize: NULL argument or no start point");
    std::string msg;
    if (!multistart::check_box_and_starts(lo, hi, x_start, n_start, h->width(), msg)) return fail(EGX_ERR_INVALID_VALUE, msg);
    return EGX_SUCCESS;
}

std::vector<double> start_point(const double *x_start, int64_t s, int d) {
    return std::vector<double>(x_start + s * d, x_start + (s + 1) * d);
}

// difference 6: the feasibility thresholds of the k constraints the machines see
std::vector<double> feasibility_thresholds(const egx_infill *h, int k) {
    std::vector<double> cfeas((size_t)k);
    for (int j = 0; j < k; j++) cfeas[j] = h->tol[j] / h->scale_cstr[j];
    return cfeas;
}

// The winner's best EVALUATED point and the stats the Cobyla and Slsqp multistarts share (differences 2 and 5 are the callers')
template <class Machine, class Stats>
int report(const std::vector<Machine> &mach, int64_t best, bool any_finite, int k, int64_t rounds, double *f_best, double *x_best,
           double *c_best, Stats *stats) {
    const Machine &win = mach[(size_t)best];
    *f_best = win.best_f();
    std::copy(win.best_x().begin(), win.best_x().end(), x_best);
    if (k > 0) std::copy(win.best_c().begin(), win.best_c().end(), c_best);
    if (stats) {
        stats->rounds = rounds;
        stats->best_start = best;
        stats->feasible = win.best_feasible() ? 1 : 0;
        stats->violation = k > 0 ? win.best_violation() : 0.0;
        if (stats->evals)
            for (size_t s = 0; s < mach.size(); s++) stats->evals[s] = mach[s].evals();
    }
    if (!any_finite) {
        *f_best = std::numeric_limits<double>::infinity();
        return fail(EGX_ERR_NO_FINITE_START, "infill optimize: no start met a finite objective value");
    }
    return EGX_SUCCESS;
}

}  // namespace

extern "C" {

int32_t egx_infill_optimize(egx_infill *h, const double *lo, const double *hi, const double *x_start, int64_t n_start,
                            int64_t max_eval, double *f_best, double *x_best, egx_infill_stats *stats) {
    if (!h) return fail(EGX_ERR_INVALID_VALUE, "infill optimize: NULL argument or no start point");
    std::lock_guard<std::mutex> lock(h->mu);
    EGX_RC(check_args(h, lo, hi, x_start, n_start, f_best, x_best, nullptr, false));
    const int d = h->width();  // the machines' dimension: n_active while an activity is set
    ModelLocks locks(h);
    max_eval = multistart::budget(max_eval, n_start, d);
    const std::vector<double> blo(lo, lo + d), bhi(hi, hi + d);
    std::vector<CobylaBox> mach;  // one per start (difference 6)
    mach.reserve((size_t)n_start);
    for (int64_t s = 0; s < n_start; s++) mach.emplace_back(start_point(x_start, s, d), blo, bhi, 0.5, 1e-4, max_eval, 0.0, true, true, 1e-4);
    multistart::BestEvaluated seen(lo, hi, x_start, n_start, d);  // difference 1
    std::vector<double> vals;
    int rc = EGX_SUCCESS;
    const int64_t rounds = multistart::run(
        mach,
        [&](const multistart::Round &r) {  // a round's trial points are ONE values-only evaluation
            vals.assign(r.size(), 0.0);
            return eval_active(h, r.pts.data(), (int64_t)r.size(), vals.data(), nullptr, nullptr);
        },
        [&](const multistart::Round &r, size_t q, CobylaBox &m) {
            seen.told(r.who[q], vals[q], r.pts.data() + q * d);
            m.tell(vals[q]);
        },
        rc);
    EGX_RC(rc);
    const int64_t best = seen.winner();
    *f_best = seen.f[(size_t)best];
    std::copy(seen.x.begin() + best * d, seen.x.begin() + (best + 1) * d, x_best);
    if (stats) {
        stats->rounds = rounds;
        stats->best_start = best;
        if (stats->evals)
            for (int64_t s = 0; s < n_start; s++) stats->evals[s] = mach[(size_t)s].evals();
    }
    if (!std::isfinite(*f_best)) return fail(EGX_ERR_NO_FINITE_START, "infill optimize: no start ended at a finite value");
    return EGX_SUCCESS;
}

int32_t egx_infill_optimize_cstr(egx_infill *h, const double *lo, const double *hi, const double *x_start, int64_t n_start,
                                 int64_t max_eval, double *f_best, double *x_best, double *c_best, egx_infill_cstr_stats *stats) {
    if (!h) return fail(EGX_ERR_INVALID_VALUE, "infill optimize: NULL argument or no start point");
    std::lock_guard<std::mutex> lock(h->mu);
    EGX_RC(check_args(h, lo, hi, x_start, n_start, f_best, x_best, c_best, true));
    const int d = h->width(), k = (int)h->surr.size() - 1;
    if (h->strategy == infill::kCstrInfill)  // difference 3
        return fail(EGX_ERR_INVALID_VALUE,
                    "infill optimize: the handle folds its constraints into the objective (EGX_CSTR_INFILL); use egx_infill_optimize");
    ModelLocks locks(h);
    max_eval = multistart::budget(max_eval, n_start, d);
    const std::vector<double> blo(lo, lo + d), bhi(hi, hi + d), cfeas = feasibility_thresholds(h, k);
    std::vector<Cobyla> mach;  // one general-constraint COBYLA per start, configured as egx_infill_optimize's (difference 6)
    mach.reserve((size_t)n_start);
    for (int64_t s = 0; s < n_start; s++)
        mach.emplace_back(start_point(x_start, s, d), blo, bhi, k, 0.5, 1e-4, 1e-4, max_eval, 0.0, true, true, cfeas);
    std::vector<double> vals, cvals;
    int rc = EGX_SUCCESS;
    const int64_t rounds = multistart::run(
        mach,
        [&](const multistart::Round &r) {  // a round's trial points are ONE values-only egx_infill_eval_cstr
            vals.assign(r.size(), 0.0);
            cvals.assign(r.size() * (size_t)k + 1, 0.0);  // difference 4
            CstrOut co;
            co.cstr = k > 0 ? cvals.data() : nullptr;
            return eval_active(h, r.pts.data(), (int64_t)r.size(), vals.data(), nullptr, nullptr, &co);
        },
        [&](const multistart::Round &, size_t q, Cobyla &m) { m.tell(vals[q], cvals.data() + q * (size_t)k); }, rc);
    EGX_RC(rc);
    // difference 2: the ordering over all starts, whatever they met
    return report(mach, multistart::winner(mach), multistart::any_finite(mach), k, rounds, f_best, x_best, c_best, stats);
}

int32_t egx_infill_optimize_slsqp(egx_infill *h, const double *lo, const double *hi, const double *x_start, int64_t n_start,
                                  int64_t max_eval, double *f_best, double *x_best, double *c_best, egx_infill_slsqp_stats *stats) {
    if (!h) return fail(EGX_ERR_INVALID_VALUE, "infill optimize: NULL argument or no start point");
    std::lock_guard<std::mutex> lock(h->mu);
    EGX_RC(check_args(h, lo, hi, x_start, n_start, f_best, x_best, nullptr, false));
    const int d = h->width();
    const bool folded = h->strategy == infill::kCstrInfill;  // difference 3: the machines see no constraint
    const int k = folded ? 0 : (int)h->surr.size() - 1;
    if (k > 0 && !c_best) return fail(EGX_ERR_INVALID_VALUE, "infill optimize: NULL argument or no start point");
    ModelLocks locks(h);
    max_eval = multistart::budget(max_eval, n_start, d);
    const std::vector<double> blo(lo, lo + d), bhi(hi, hi + d), cfeas = feasibility_thresholds(h, k);
    std::vector<Slsqp> mach;  // one per start; it is told c_j as evaluated and solves c_j <= cfeas_j (difference 6)
    mach.reserve((size_t)n_start);
    for (int64_t s = 0; s < n_start; s++) mach.emplace_back(start_point(x_start, s, d), blo, bhi, k, 1e-4, 1e-4, max_eval, cfeas);
    std::vector<double> vals, grads, cvals, cgrads;
    int rc = EGX_SUCCESS;
    const int64_t rounds = multistart::run(
        mach,
        [&](const multistart::Round &r) {  // a round's points are ONE evaluation with gradients
            const size_t m = r.size();
            vals.assign(m, 0.0);
            grads.assign(m * d, 0.0);
            cvals.assign(m * (size_t)k + 1, 0.0);  // difference 4
            cgrads.assign(m * (size_t)k * d + 1, 0.0);
            if (folded) return eval_active(h, r.pts.data(), (int64_t)m, vals.data(), grads.data(), nullptr);
            CstrOut co;
            co.cstr = k > 0 ? cvals.data() : nullptr, co.gcstr = k > 0 ? cgrads.data() : nullptr;
            return eval_active(h, r.pts.data(), (int64_t)m, vals.data(), grads.data(), nullptr, &co);
        },
        [&](const multistart::Round &, size_t q, Slsqp &m) {
            m.tell(vals[q], cvals.data() + q * (size_t)k, grads.data() + q * d, cgrads.data() + q * (size_t)k * d);
        },
        rc);
    EGX_RC(rc);
    const bool any_finite = multistart::any_finite(mach);
    if (stats && stats->stop)  // difference 5
        for (int64_t s = 0; s < n_start; s++) stats->stop[s] = (int32_t)mach[(size_t)s].status();
    // difference 2: nothing finite anywhere leaves start 0
    return report(mach, multistart::winner(mach, any_finite), any_finite, k, rounds, f_best, x_best, c_best, stats);
}

void egx_infill_batch_config_default(egx_infill_batch_config *cfg) {
    if (!cfg) return;
    cfg->strategy = EGX_QEI_KB;
    cfg->optimizer = EGX_BATCH_SLSQP;
    cfg->max_eval = 0;
    cfg->scaling_points = nullptr;
    cfg->n_scaling = 0;
}

int32_t egx_infill_optimize_batch(egx_infill *h, const egx_infill_batch_config *cfg_in, const double *lo, const double *hi,
                                  const double *x_start, int64_t n_start, int32_t q, double *x_out, double *y_virtual, double *f_out,
                                  int32_t *n_found) {
    if (n_found) *n_found = 0;
    if (!h || !lo || !hi || !x_start || !x_out || !y_virtual || !f_out || !n_found || n_start < 1)
        return fail(EGX_ERR_INVALID_VALUE, "infill batch: NULL argument or no start point");
    egx_infill_batch_config cfg;
    if (cfg_in) cfg = *cfg_in; else egx_infill_batch_config_default(&cfg);
    if (q < 1 || q > EGX_INFILL_MAX_PENDING || cfg.strategy < EGX_QEI_KB || cfg.strategy > EGX_QEI_CL_MIN ||
        (cfg.optimizer != EGX_BATCH_COBYLA && cfg.optimizer != EGX_BATCH_SLSQP) || (cfg.scaling_points && cfg.n_scaling < 1))
        return fail(EGX_ERR_INVALID_VALUE, "infill batch: q must be 1 .. 16, the strategy an egx_qei_strategy, the optimizer COBYLA or SLSQP");
    {  // a batch step pushes its full-width point: not under active coordinates
        std::lock_guard<std::mutex> lock(h->mu);
        if (!h->active.empty())
            return fail(EGX_ERR_UNSUPPORTED, "infill batch: active coordinates are set (egx_infill_set_active); call egx_infill_clear_active first");
    }
    const int d = h->d, nm = (int)h->surr.size();
    std::vector<double> cb((size_t)nm);
    // every step through the public entry points (each takes the handle's lock itself): the loop a caller would write
    for (int i = 0; i < q; i++) {
        const double *xs = x_start + (size_t)i * n_start * d;
        double *xo = x_out + (size_t)i * d, *yv = y_virtual + (size_t)i * nm;
        if (cfg.scaling_points) EGX_RC(egx_infill_scaling(h, cfg.scaling_points, cfg.n_scaling, nullptr, nullptr, nullptr));
        int32_t strategy = EGX_CSTR_INFILL;
        EGX_RC(egx_infill_get_cstr_strategy(h, &strategy, nullptr));
        if (cfg.optimizer == EGX_BATCH_SLSQP)
            EGX_RC(egx_infill_optimize_slsqp(h, lo, hi, xs, n_start, cfg.max_eval, f_out + i, xo, cb.data(), nullptr));
        else if (strategy == EGX_CSTR_INFILL)
            EGX_RC(egx_infill_optimize(h, lo, hi, xs, n_start, cfg.max_eval, f_out + i, xo, nullptr));
        else
            EGX_RC(egx_infill_optimize_cstr(h, lo, hi, xs, n_start, cfg.max_eval, f_out + i, xo, cb.data(), nullptr));
        EGX_RC(egx_infill_virtual_point(h, xo, cfg.strategy, yv));
        EGX_RC(egx_infill_push_pending(h, xo, yv));
        *n_found = i + 1;
    }
    return EGX_SUCCESS;
}

}  // extern "C"
