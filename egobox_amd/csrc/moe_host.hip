// The predict side of a mixture of experts behind the C ABI (include/egx_gp.h): egx_moe_predict_valvar and
// egx_moe_predict_valvar_gradients, two clients of ONE sharded fold (moe_fold.h: routing, two experts in flight, the order of
// additions, the payload) and of ONE status-word exchange (sweep_internal.h).  What stays here: each entry point's argument
// checks and the choice of the expert calls that fill a worker's scratch.
//
// GpMixture::predict_smooth / predict_var_smooth (crates/moe/src/algorithm.rs:411-423, 670-685): val = sum_e p_e y_e,
// var = sum_e p_e^2 v_e over ALL points; predict_hard / predict_var_hard (:879-935): every point is answered by the expert
// of its cluster, argmax_e p_e.  predict_gradients_smooth / predict_var_gradients_smooth (:691-783):
//     d val / dx = sum_e p_e grad y_e + p'_e y_e ,   d var / dx = sum_e p_e^2 grad v_e + 2 p_e p'_e v_e
// and predict_gradients_hard / predict_var_gradients_hard (:942-1010): the gradient of the expert of argmax_e p_e.  The
// reference calls the expert once per ROW (a full n^2 triangular solve per point for the variance); here the points are
// routed once and every expert gets ONE batched call per quantity on its points.  Multi-rank: every rank owns some of the
// experts (the reference's serial expert loop, :167-177, sharded), forms the partial sums of its own, and ONE all-gather of
// the partial vectors + a sum in rank order (the same bits on every rank) replaces the reference's fold over experts.
#include "moe_fold.h"
#include "sweep_internal.h"

using namespace egx;

namespace {

struct ExpertRows {
    std::vector<double> y, v, gy, gv;  // values (me each) and x-gradients (me x d each) of one expert call
};

// the prediction entry points of the two kinds of expert, under one set of names
inline int ex_predict(egx_gp *g, const double *x, int64_t m, double *y) { return egx_gp_predict(g, x, m, y); }
inline int ex_predict_var(egx_gp *g, const double *x, int64_t m, double *v) { return egx_gp_predict_var(g, x, m, v); }
inline int ex_predict_valvar(egx_gp *g, const double *x, int64_t m, double *y, double *v) { return egx_gp_predict_valvar(g, x, m, y, v); }
inline int ex_gradients(egx_gp *g, const double *x, int64_t m, double *gy) { return egx_gp_predict_gradients(g, x, m, gy); }
inline int ex_var_gradients(egx_gp *g, const double *x, int64_t m, double *gv) { return egx_gp_predict_var_gradients(g, x, m, gv); }
inline int ex_valvar_gradients(egx_gp *g, const double *x, int64_t m, double *gy, double *gv) {
    return egx_gp_predict_valvar_gradients(g, x, m, gy, gv);
}
inline int ex_predict(egx_sgp *g, const double *x, int64_t m, double *y) { return egx_sgp_predict(g, x, m, y); }
inline int ex_predict_var(egx_sgp *g, const double *x, int64_t m, double *v) { return egx_sgp_predict_var(g, x, m, v); }
inline int ex_predict_valvar(egx_sgp *g, const double *x, int64_t m, double *y, double *v) { return egx_sgp_predict_valvar(g, x, m, y, v); }
inline int ex_gradients(egx_sgp *g, const double *x, int64_t m, double *gy) { return egx_sgp_predict_gradients(g, x, m, gy); }
inline int ex_var_gradients(egx_sgp *g, const double *x, int64_t m, double *gv) { return egx_sgp_predict_var_gradients(g, x, m, gv); }
inline int ex_valvar_gradients(egx_sgp *g, const double *x, int64_t m, double *gy, double *gv) {
    return egx_sgp_predict_valvar_gradients(g, x, m, gy, gv);
}

// one expert's values through the entry point that serves the outputs wanted
template <class Expert>
int expert_values(Expert *gp, const double *xin, int64_t me, bool want_y, bool want_v, ExpertRows &s) {
    if (want_y) s.y.resize(me);
    if (want_v) s.v.resize(me);
    if (want_y && want_v) return ex_predict_valvar(gp, xin, me, s.y.data(), s.v.data());
    return want_y ? ex_predict(gp, xin, me, s.y.data()) : ex_predict_var(gp, xin, me, s.v.data());
}

// the local fold's payload through the collective (failures are carried into it: a rank that left early would hang the
// others) and the sum over ranks into the caller's outputs
int exchange_and_sum(egx_sweep *sw, const char *who, moe::LocalFold &lf, size_t mw, double *out_a, double *out_b) {
    std::vector<double> all;
    {
        std::unique_lock<std::mutex> lock;
        if (sw) {
            lock = std::unique_lock<std::mutex>(sw->mu);
            (void)set_device(sw->gp);
        }
        EGX_RC(sweep_exchange_status(sw, who, lf.rc, lf.msg, lf.part, all));
    }
    moe::fold_sum_ranks(all.data(), sw ? sw->world : 1, mw, out_a, out_b);
    return EGX_SUCCESS;
}

// egx_moe_predict_valvar / _valvar_sgp: `who` names the entry point in messages
template <class Expert>
int32_t moe_valvar(const char *who, egx_sweep *sw, Expert *const *experts, const int32_t *expert_ids, int64_t n_local,
                   int64_t n_experts, const double *probas, const double *xq, int64_t m, int64_t d, int32_t smooth, double *val,
                   double *var) {
    if (n_local < 0 || n_experts < 1 || m < 0 || d < 1 || (m > 0 && (!probas || !xq)) || (n_local > 0 && (!experts || !expert_ids)) ||
        (!val && !var)) {
        set_error(std::string(who) + ": bad arguments");
        return EGX_ERR_INVALID_VALUE;
    }
    if (!sw && n_local != n_experts) {
        set_error(std::string(who) + ": without a sweep handle (single process) every expert must be local");
        return EGX_ERR_INVALID_VALUE;
    }
    if (m == 0) return EGX_SUCCESS;
    const moe::Fold<Expert> f{experts, expert_ids, n_local, n_experts, probas, xq, m, d, 1, smooth != 0};
    auto eval = [&](Expert *gp, const double *xin, int64_t me, ExpertRows &s, std::string &msg) {
        const int rc = expert_values(gp, xin, me, val != nullptr, var != nullptr, s);
        if (rc) msg = last_error_string();
        return rc;
    };
    auto acc = [&](int32_t g, const ExpertRows &s, const int64_t *rows, int64_t me, double *tv, double *tw) {
        moe::accumulate_values(probas, n_experts, m, g, val ? s.y.data() : nullptr, var ? s.v.data() : nullptr, rows, me, tv, tw);
    };
    moe::LocalFold lf = moe::fold_local<ExpertRows>(who, f, eval, acc);
    return exchange_and_sum(sw, who, lf, (size_t)m, val, var);
}

template <class Expert>
int32_t moe_valvar_gradients(const char *who, egx_sweep *sw, Expert *const *experts, const int32_t *expert_ids, int64_t n_local,
                             int64_t n_experts, const double *probas, const double *dprobas, const double *xq, int64_t m, int64_t d,
                             int32_t smooth, double *grad_val, double *grad_var) {
    if (n_local < 0 || n_experts < 1 || m < 0 || d < 1 || (m > 0 && (!probas || !xq)) || (n_local > 0 && (!experts || !expert_ids)) ||
        (!grad_val && !grad_var) || (smooth && n_experts > 1 && m > 0 && !dprobas)) {
        set_error(std::string(who) + ": bad arguments (the smooth recombination of more than one expert needs dprobas)");
        return EGX_ERR_INVALID_VALUE;
    }
    if (!sw && n_local != n_experts) {
        set_error(std::string(who) + ": without a sweep handle (single process) every expert must be local");
        return EGX_ERR_INVALID_VALUE;
    }
    if (m == 0) return EGX_SUCCESS;
    const bool need_pp = smooth && n_experts > 1;  // the p' terms need the experts' values too
    const moe::Fold<Expert> f{experts, expert_ids, n_local, n_experts, probas, xq, m, d, d, smooth != 0};
    auto eval = [&](Expert *gp, const double *xin, int64_t me, ExpertRows &s, std::string &msg) {
        int rc;
        if (grad_val) s.gy.resize((size_t)me * d);
        if (grad_var) s.gv.resize((size_t)me * d);
        if (grad_val && grad_var) rc = ex_valvar_gradients(gp, xin, me, s.gy.data(), s.gv.data());
        else if (grad_val) rc = ex_gradients(gp, xin, me, s.gy.data());
        else rc = ex_var_gradients(gp, xin, me, s.gv.data());
        if (!rc && need_pp) rc = expert_values(gp, xin, me, grad_val != nullptr, grad_var != nullptr, s);
        if (rc) msg = last_error_string();
        return rc;
    };
    auto acc = [&](int32_t g, const ExpertRows &s, const int64_t *rows, int64_t me, double *tv, double *tw) {
        moe::accumulate_gradients(probas, need_pp ? dprobas : nullptr, n_experts, m, d, g, grad_val ? s.gy.data() : nullptr,
                                  grad_var ? s.gv.data() : nullptr, s.y.data(), s.v.data(), rows, me, tv, tw);
    };
    moe::LocalFold lf = moe::fold_local<ExpertRows>(who, f, eval, acc);
    return exchange_and_sum(sw, who, lf, (size_t)m * d, grad_val, grad_var);
}

}  // namespace

extern "C" {

int32_t egx_moe_predict_valvar(egx_sweep *sw, egx_gp *const *experts, const int32_t *expert_ids, int64_t n_local,
                               int64_t n_experts, const double *probas, const double *xq, int64_t m, int64_t d,
                               int32_t smooth, double *val, double *var) {
    return moe_valvar("egx_moe_predict_valvar", sw, experts, expert_ids, n_local, n_experts, probas, xq, m, d, smooth, val, var);
}

int32_t egx_moe_predict_valvar_sgp(egx_sweep *sw, egx_sgp *const *experts, const int32_t *expert_ids, int64_t n_local,
                                   int64_t n_experts, const double *probas, const double *xq, int64_t m, int64_t d,
                                   int32_t smooth, double *val, double *var) {
    return moe_valvar("egx_moe_predict_valvar_sgp", sw, experts, expert_ids, n_local, n_experts, probas, xq, m, d, smooth, val, var);
}

int32_t egx_moe_predict_valvar_gradients(egx_sweep *sw, egx_gp *const *experts, const int32_t *expert_ids, int64_t n_local,
                                         int64_t n_experts, const double *probas, const double *dprobas, const double *xq,
                                         int64_t m, int64_t d, int32_t smooth, double *grad_val, double *grad_var) {
    return moe_valvar_gradients("egx_moe_predict_valvar_gradients", sw, experts, expert_ids, n_local, n_experts, probas, dprobas, xq,
                                m, d, smooth, grad_val, grad_var);
}

int32_t egx_moe_predict_valvar_gradients_sgp(egx_sweep *sw, egx_sgp *const *experts, const int32_t *expert_ids, int64_t n_local,
                                             int64_t n_experts, const double *probas, const double *dprobas, const double *xq,
                                             int64_t m, int64_t d, int32_t smooth, double *grad_val, double *grad_var) {
    return moe_valvar_gradients("egx_moe_predict_valvar_gradients_sgp", sw, experts, expert_ids, n_local, n_experts, probas, dprobas,
                                xq, m, d, smooth, grad_val, grad_var);
}

}  // extern "C"
