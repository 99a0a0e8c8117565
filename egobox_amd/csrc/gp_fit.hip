// Optimiser drivers above the dense likelihood (GpValidParams::fit with ThetaTuning::Full / Partial, algorithm.rs:873-960,
// optimization.rs:26-169): multistart COBYLA on one model (egx_gp_fit, egx_gp_fit_partial, egx_sweep_fit) and on the models of a
// group (egx_gp_fit_multi), the theta-gradient of the likelihood and a projected L-BFGS on it.  Every
// driver is LOCK-STEP: multistart::run over one machine per start, a round's points in one evaluation call.  The box, the
// budget, the machines, the reduction and the winner are fit_starts.h's; this file holds only what touches a handle.
#include "gp_handle.h"

using namespace egx;

namespace egx {

// Multistart derivative-free fit over the ACTIVE theta components (all of them for ThetaTuning::Full; a subset for
// ThetaTuning::Partial, algorithm.rs:822-826, 873-960: the inactive components stay at theta_base), in two halves so that
// the starts can be SHARDED over the ranks of a sweep (egx_sweep_fit): fit_run_starts runs the COBYLA machines of the starts
// s with s mod world == rank, fit_reduce_finalize reduces all starts' results and keeps the winner's factor resident.
// Both halves expect the CALLER to hold gp->mu exclusively (one critical section from the first evaluation to the
// finalized model, as the header documents for a handle: fit_nm_core below, egx_sweep_fit around its all-gather).
int fit_run_starts(egx_gp *gp, const double *theta_base /*h*/, const std::vector<int> &active,
                   const double *theta0s /*n_starts x k*/, int64_t n_starts, const double *lo, const double *hi,
                   int64_t bounds_len, int64_t max_eval, int rank, int world, std::vector<StartResult> &results) {
    if (!theta0s || !lo || !hi || n_starts < 1 || active.empty()) {
        set_error("NULL argument / no start point");
        return EGX_ERR_INVALID_VALUE;
    }
    const int hfull = gp->h;
    const int h = (int)active.size();  // optimised dimensions
    fit::Log10Box box;
    EGX_RC(fit_box(lo, hi, bounds_len, h, theta0s, n_starts * h, fit::Dense, box));
    EGX_RC(set_device(gp));
    results.assign((size_t)n_starts, StartResult{std::numeric_limits<double>::quiet_NaN(), std::vector<double>(h, 0.0), 0});
    gp->fitted = false;
    // one COBYLA machine per start of this rank, all advanced in LOCK-STEP: their trial points form one likelihood batch per
    // round, pipelined over the handle's workspaces (the reference runs the starts as rayon tasks, algorithm.rs:928-945)
    const std::vector<int64_t> mine = fit::shard(n_starts, rank, world);
    std::vector<CobylaBox> mach = fit::cobyla_machines(theta0s, h, mine, box, fit::cobyla_budget(h, max_eval));
    std::vector<double> thetas, lk;
    std::vector<int32_t> st;
    int rc;
    multistart::run(
        mach,
        [&](const multistart::Round &r) {
            fit::round_thetas(r, theta_base, hfull, active, thetas);
            lk.assign(r.size(), 0.0);
            st.assign(r.size(), 0);
            return likelihood_batch_core(gp, thetas.data(), (int64_t)r.size(), hfull, lk.data(), st.data());
        },
        [&](const multistart::Round &, size_t q, CobylaBox &m) { m.tell(fit::cobyla_objective(st[q] == EGX_STATUS_OK, lk[q])); }, rc);
    EGX_RC(rc);
    for (size_t q = 0; q < mach.size(); q++) results[(size_t)mine[q]] = fit::cobyla_result(mach[q]);
    return EGX_SUCCESS;
}

int fit_reduce_finalize(egx_gp *gp, const double *theta_base, const std::vector<int> &active, const double *theta0s,
                        const std::vector<StartResult> &results, int64_t *n_evals_out) {
    // every start failed: the reference falls through with ones (algorithm.rs:943); start 0 is kept here
    const std::vector<double> th = fit::winner_theta(theta_base, gp->h, active, fit::best_start(results, n_evals_out), theta0s);
    EGX_RC(set_device(gp));
    return do_finalize(gp, th.data(), gp->h);
}

}  // namespace egx

extern "C" {

static int32_t fit_nm_core(egx_gp *gp, const double *theta_base /*h*/, const std::vector<int> &active,
                           const double *theta0s /*n_starts x k*/, int64_t n_starts, const double *lo,
                           const double *hi, int64_t bounds_len, int64_t max_eval, int64_t *n_evals_out) {
    std::vector<StartResult> results;
    std::unique_lock<std::shared_mutex> lock(gp->mu);  // the whole fit is one critical section
    EGX_RC(fit_run_starts(gp, theta_base, active, theta0s, n_starts, lo, hi, bounds_len, max_eval, 0, 1, results));
    return fit_reduce_finalize(gp, theta_base, active, theta0s, results, n_evals_out);
}

int32_t egx_gp_fit(egx_gp *gp, const double *theta0s, int64_t n_starts, const double *lo, const double *hi,
                   int64_t bounds_len, int64_t max_eval, int64_t *n_evals_out) {
    if (!gp || !theta0s || n_starts < 1) {
        set_error("NULL argument / no start point");
        return EGX_ERR_INVALID_VALUE;
    }
    return fit_nm_core(gp, theta0s, fit::all_active(gp->h), theta0s, n_starts, lo, hi, bounds_len, max_eval, n_evals_out);
}

int32_t egx_gp_fit_partial(egx_gp *gp, const double *theta_init, const int64_t *active_idx, int64_t n_active,
                           const double *theta0s, int64_t n_starts, const double *lo, const double *hi,
                           int64_t bounds_len, int64_t max_eval, int64_t *n_evals_out) {
    if (!gp || !theta_init || !active_idx || n_active < 1 || n_active > gp->h) {
        set_error("NULL argument / bad active set");
        return EGX_ERR_INVALID_VALUE;
    }
    std::vector<int> active((size_t)n_active);
    for (int64_t i = 0; i < n_active; i++) {
        if (active_idx[i] < 0 || active_idx[i] >= gp->h || (i > 0 && active_idx[i] <= active_idx[i - 1])) {
            set_error("active theta components must be strictly increasing indices in [0, h)");
            return EGX_ERR_INVALID_VALUE;
        }
        active[(size_t)i] = (int)active_idx[i];
    }
    for (int i = 0; i < gp->h; i++)
        if (!(theta_init[i] > 0.0)) {
            set_error("theta_init must be > 0");
            return EGX_ERR_INVALID_VALUE;
        }
    return fit_nm_core(gp, theta_init, active, theta0s, n_starts, lo, hi, bounds_len, max_eval, n_evals_out);
}
}  // extern "C"

namespace egx {

// ---------------------------------------------------------------------------------------------
// K7, host side: likelihood AND dL/dtheta of k candidates (the reference has no gradient,
// algorithm.rs:880 ignores `_gradient`).  Per candidate, after the evaluation of the likelihood left the factor C in the
// workspace:   W = C^-T (rows of the identity through the forward block substitution, n^3/3 flop; round 4: it RIDES ALONG
//                                          the factorisation, group of panels by group of panels on a stream of its own --
//                                          PotrfInverse, egx_internal.h)
//              gamma = W rho                       (one pass over W)
//              -R^-1 = -(W W^T), lower triangle    (LDS-DMA stream kernel with per-tile K ranges, n^3/3 flop; written
//                                                   OVER the factor: no second n^2 buffer)
//              dL/dc_o = (1 / ln 10) sum_{i>j} 2 R_ij (gamma_i gamma_j / sigma2 - R^-1_ij) dlogR_ij/dc_o   (k_grad_accum)
// Round 4: everything is enqueued on the evaluation's stream behind the likelihood (round 3 had three blocking host
// round trips per gradient), the candidates of a batch are pipelined over the handle's workspaces like a likelihood
// batch, and a slot's candidates run every stage in LOCK-STEP (grid.z over consecutive workspaces and consecutive C^-T
// buffers of `slab_W`).  Every stage is deterministic and its kernel choice depends on one matrix' size only, so a
// candidate's (likelihood, gradient) are the same bits alone and in any batch.
// ---------------------------------------------------------------------------------------------
static int ensure_grad_scratch(egx_gp *gp, int ws_lo, int nuse) {
    const size_t sq = (size_t)gp->n_pad * gp->n_pad;
    if (gp->slab_W_count < nuse) {
        gp->slab_W_count = 0;
        EGX_RC(gp->slab_W.alloc(sq * (size_t)nuse));
        gp->slab_W_count = nuse;
    }
    for (int i = ws_lo; i < ws_lo + nuse; i++) {
        Workspace &w = gp->ws[i];
        EGX_RC(w.d_gpart.alloc((size_t)grad_partial_doubles(gp->d)));
        EGX_RC(w.d_gout.alloc((size_t)(gp->d + 64)));
        EGX_RC(w.h_gout.alloc((size_t)(gp->d + 64)));
    }
    if (gp->has_w && !gp->d_wabs) {
        std::vector<double> wabs(gp->w_star.size());
        for (size_t e = 0; e < wabs.size(); e++) wabs[e] = std::fabs(gp->w_star[e]);
        EGX_RC(gp->d_wabs.alloc(wabs.size()));
        EGX_HIP_CHECK(hipMemcpy(gp->d_wabs, wabs.data(), sizeof(double) * wabs.size(), hipMemcpyHostToDevice));
    }
    return EGX_SUCCESS;
}

// the gradient stages of `count` consecutive workspaces from w0 (their factors in place, rho in d_rhs) on stream st;
// C^-T buffers slot0 .. of slab_W
// pre != 0: every candidate of the run has hcols == 1 and positive coefficients -- the trace kernel takes the prescaled form
static int enqueue_grad_run(egx_gp *gp, hipStream_t st, int w0, int count, int slot0, const double *inv_s2, int hcols, int pre) {
    const int n = gp->n, n_pad = gp->n_pad;
    const int64_t sq = (int64_t)n_pad * n_pad;
    Workspace &lead = gp->ws[w0];
    double *W0 = gp->slab_W + (int64_t)slot0 * sq;  // C^-T of these candidates: rode along their factorisation
    for (int j = 0; j < count; j++) {
        Workspace &w = gp->ws[w0 + j];
        EGX_RC(launch_uptri_gemv(st, W0 + (int64_t)j * sq, n_pad, n, w.d_rhs, w.d_vec));
    }
    GemmBatch gbm;
    gbm.count = count;
    gbm.sC = gp->stride_M;
    gbm.sA = gbm.sB = sq;
    EGX_RC(launch_syrk_uptri_neg(st, lead.M, gp->ld, W0, n_pad, n_pad, &gbm));
    const int nout = (hcols == 1) ? gp->d : gp->h;
    GradBatch gb;
    gb.count = count;
    for (int j = 0; j < count; j++) {
        Workspace &w = gp->ws[w0 + j];
        if (pre) EGX_RC(launch_scale_rows(st, gp->d_xT, n_pad, gp->d, w.d_coef, w.d_xs));  // (K1 may have taken its LDS-only form)
        gb.xs[j] = w.d_xs;
        gb.coef[j] = w.d_coef;
        gb.gamma[j] = w.d_vec;
        gb.rneg[j] = w.M;
        gb.inv_s2[j] = inv_s2[j];
        gb.part[j] = w.d_gpart;
        gb.out[j] = w.d_gout;
    }
    for (int j = count; j < kLockstepMax; j++) {
        gb.xs[j] = gb.coef[j] = gb.gamma[j] = gb.rneg[j] = nullptr;
        gb.inv_s2[j] = 0.0;
        gb.part[j] = gb.out[j] = nullptr;
    }
    EGX_RC(launch_grad_accum(st, gp->corr, gp->d_xT, n_pad, n, gp->d, hcols, hcols > 1 ? gp->d_wabs : nullptr, nout, gp->ld, gb,
                             pre));
    for (int j = 0; j < count; j++) {
        Workspace &w = gp->ws[w0 + j];
        EGX_HIP_CHECK(hipMemcpyAsync(w.h_gout, w.d_gout, sizeof(double) * nout, hipMemcpyDeviceToHost, st));
    }
    return EGX_SUCCESS;
}

// dL/dtheta (h) from the kernel's sums over the coefficients (nout): the chain rule of make_coef
static void grad_chain_rule(const egx_gp *gp, const double *gsum, int hcols, const std::vector<double> &coef,
                            const std::vector<double> &thfull, double *grad) {
    const int d = gp->d, h = gp->h;
    const double ln10 = std::log(10.0);
    if (!gp->has_w || hcols > 1) {
        for (int k = 0; k < h; k++) grad[k] = gsum[k] / ln10;  // w = I (c = theta), or KPLS + Matern (outputs are per theta)
        return;
    }
    // KPLS with a collapsed per-dimension coefficient c_j (make_coef): chain rule dc_j / dtheta_l
    //   sq-exp : c_j = sqrt(sum_l (theta_l w_jl)^2)  ->  theta_l w_jl^2 / c_j     (correlation_models.rs:97-98)
    //   abs-exp: c_j = sum_l theta_l |w_jl|           ->  |w_jl|                   (:191)
    const double *wm = gp->w_star.data();
    for (int l = 0; l < h; l++) {
        double sacc = 0.0;
        for (int j = 0; j < d; j++) {
            const double wjl = wm[(size_t)j * h + l], pk = gsum[j] / ln10;
            if (gp->corr == EGX_CORR_SQUARED_EXPONENTIAL) {
                if (coef[j] > 0.0) sacc += pk * thfull[l] * wjl * wjl / coef[j];
            } else {
                sacc += pk * std::fabs(wjl);
            }
        }
        grad[l] = sacc;
    }
}

// likelihood + gradient of the rows of thetas (k x theta_len) that `src` hands out: lkh[c], grad[c * h ..], status[c].  Caller
// holds gp->mu exclusively and has set the device.  A fitted model keeps workspace 0 as long as another workspace exists.
// The two-phase client of the slot pipeline (slot_pipeline.h): a slot's candidates are enqueued as a likelihood batch's are
// (C^-T riding along, into the slot's buffers of slab_W), phase 1 ends with the host halves of the likelihoods and enqueues the
// gradient stages, phase 2 ends with the chain rule.  It uses min(workspaces, k) workspaces: that many C^-T buffers.
int likelihood_grad_batch_core(egx_gp *gp, const double *thetas, int64_t k, int64_t theta_len, double *lkh, double *grad,
                               int32_t *status, CandidateSource *src) {
    if (k <= 0) return EGX_SUCCESS;
    const int h = gp->h;
    const int ws_lo = (gp->fitted && gp->ws.size() > 1) ? 1 : 0;
    const int nuse = (int)std::min<int64_t>((int64_t)gp->ws.size() - ws_lo, k);
    const SlotGeometry g = slot_geometry(ws_lo, nuse, gp->lockstep, kLockstepMax);
    EGX_RC(ensure_grad_scratch(gp, ws_lo, nuse));
    if (ws_lo == 0) gp->fitted = false;
    struct Slot {
        std::vector<int64_t> cand;
        std::vector<std::vector<double>> coefs, thfull;
        std::vector<char> ok, pre;  // ok: has a gradient; pre: eligible for the prescaled trace kernel
        int hcols = 1;
    };
    std::vector<Slot> slots(g.nslots);
    for (auto &sl : slots) {
        sl.coefs.resize(g.width);
        sl.thfull.resize(g.width);
    }
    auto admit = [&](int i, int j, int64_t c, bool &valid) -> int {
        Slot &sl = slots[i];
        const double *th = thetas + c * theta_len;
        EGX_RC(make_coef(gp, th, theta_len, sl.coefs[j], sl.hcols, &sl.thfull[j]));
        for (int l = 0; l < h; l++) grad[c * h + l] = 0.0;
        valid = !has_nan(th, theta_len);  // (a NaN theta is answered at once, algorithm.rs:885-891)
        if (valid) sl.cand.push_back(c);
        else lkh[c] = -std::numeric_limits<double>::infinity(), status[c] = EGX_STATUS_NAN_THETA;
        return EGX_SUCCESS;
    };
    auto enqueue = [&](int i, int count) -> int {
        return enqueue_eval_group(gp, g.first_ws(i), count, slots[i].coefs.data(), slots[i].hcols,
                                  gp->slab_W + (int64_t)(i * g.width) * gp->n_pad * gp->n_pad);
    };
    auto advance = [&](int i, int phase, bool &idle) -> int {
        Slot &sl = slots[i];
        const int w0 = g.first_ws(i);
        hipStream_t st = gp->ws[w0].stream;
        const int cnt = (int)sl.cand.size();
        idle = phase == 2;
        if (phase == 2) {
            EGX_HIP_CHECK(hipStreamSynchronize(st));
            for (int j = 0; j < cnt; j++)
                if (sl.ok[j]) grad_chain_rule(gp, gp->ws[w0 + j].h_gout, sl.hcols, sl.coefs[j], sl.thfull[j], grad + sl.cand[j] * h);
            sl.cand.clear();
            return EGX_SUCCESS;
        }
        // host half of the likelihoods (GLS, sigma2), then the gradient stages for the candidates that have one
        std::vector<double> inv_s2(cnt, 0.0);
        sl.ok.assign(cnt, 0);
        sl.pre.assign(cnt, 0);
        for (int j = 0; j < cnt; j++) {
            Workspace &w = gp->ws[w0 + j];
            EvalResult res;
            EGX_RC(finish_eval(gp, w, res, 2));
            const int64_t c = sl.cand[j];
            lkh[c] = res.lkh;
            status[c] = res.status;
            if (res.status != EGX_STATUS_OK || !(res.sigma2n > 0.0) || !std::isfinite(res.lkh)) continue;
            sl.ok[j] = 1;
            inv_s2[j] = 1.0 / res.sigma2n;
            // the prescaled form divides by the coefficient once per output: a candidate's OWN coefficients decide
            // (never its companions': the kernel choice must not depend on the batch)
            sl.pre[j] = sl.hcols == 1 ? 1 : 0;
            for (double cj : sl.coefs[j])
                if (!(cj > 0.0) || !std::isfinite(cj)) sl.pre[j] = 0;
            EGX_RC(upload_rho(gp, w, res, st));
        }
        // maximal runs of consecutive candidates with a gradient (and the same form of the trace kernel): each run is one
        // lock-step launch sequence
        for (int j = 0; j < cnt;) {
            if (!sl.ok[j]) {
                j++;
                continue;
            }
            int e = j;
            while (e < cnt && sl.ok[e] && sl.pre[e] == sl.pre[j]) e++;
            EGX_RC(enqueue_grad_run(gp, st, w0 + j, e - j, i * g.width + j, inv_s2.data() + j, sl.hcols, sl.pre[j]));
            j = e;
        }
        return EGX_SUCCESS;
    };
    return run_slots(gp, g, src, k, admit, enqueue, advance);
}
}  // namespace egx

extern "C" {

int32_t egx_gp_likelihood_grad(egx_gp *gp, const double *theta, int64_t theta_len, double *lkh, double *grad,
                               int32_t *status) {
    if (!gp || !theta || !lkh || !grad || !status) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    if (theta_len != 1 && theta_len != gp->h) {
        set_error("theta should be either 1-dim or dim of xtrain (w_star.ncols()), got " + std::to_string(theta_len));
        return EGX_ERR_INVALID_VALUE;
    }
    std::unique_lock<std::shared_mutex> lock(gp->mu);
    EGX_RC(set_device(gp));
    return likelihood_grad_batch_core(gp, theta, 1, theta_len, lkh, grad, status);
}

int32_t egx_gp_likelihood_grad_batch(egx_gp *gp, const double *thetas, int64_t k, int64_t theta_len, double *lkh,
                                     double *grads, int32_t *status) {
    if (!gp || k < 0 || (k > 0 && (!thetas || !lkh || !grads || !status))) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    if (theta_len != 1 && theta_len != gp->h) {
        set_error("theta should be either 1-dim or dim of xtrain (w_star.ncols()), got " + std::to_string(theta_len));
        return EGX_ERR_INVALID_VALUE;
    }
    std::unique_lock<std::shared_mutex> lock(gp->mu);
    EGX_RC(set_device(gp));
    return likelihood_grad_batch_core(gp, thetas, k, theta_len, lkh, grads, status);
}

/* Gradient-based alternative to egx_gp_fit (new: uses the theta-gradient the reference does not have).
 * Projected L-BFGS on x = log10(theta) inside the box, one ask / tell machine per start (LbfgsStart, lbfgs.h), ALL starts in
 * lock-step: a round's trial points (one per start that is still running) are ONE likelihood + gradient batch
 * (egx_gp_likelihood_grad_batch), as the COBYLA starts of egx_gp_fit are one likelihood batch.  Each start walks exactly the
 * points it walks alone.  Best start wins (the first on ties), then finalize.  max_iter bounds the iterations per start;
 * *n_evals_out is the number of points asked. */
int32_t egx_gp_fit_lbfgs(egx_gp *gp, const double *theta0s, int64_t n_starts, const double *lo, const double *hi,
                         int64_t bounds_len, int64_t max_iter, int64_t *n_evals_out) {
    if (!gp || !theta0s || !lo || !hi || n_starts < 1) {
        set_error("NULL argument / no start point");
        return EGX_ERR_INVALID_VALUE;
    }
    const int h = gp->h;
    fit::Log10Box box;
    EGX_RC(fit_box(lo, hi, bounds_len, h, theta0s, n_starts * h, fit::Dense, box));
    if (max_iter < 1) max_iter = 50;
    std::unique_lock<std::shared_mutex> lock(gp->mu);
    EGX_RC(set_device(gp));
    gp->fitted = false;
    const double ln10 = std::log(10.0), inf = std::numeric_limits<double>::infinity();
    const std::vector<int> active = fit::all_active(h);
    std::vector<LbfgsStart> mach = fit::lbfgs_machines(theta0s, h, fit::shard(n_starts), box, max_iter);
    int64_t evals = 0;
    std::vector<double> thetas, lk, gr, gx(h);
    std::vector<int32_t> stv;
    int rc;
    multistart::run(
        mach,
        [&](const multistart::Round &r) {
            fit::round_thetas(r, theta0s, h, active, thetas);
            lk.assign(r.size(), 0.0);
            gr.assign(r.size() * (size_t)h, 0.0);
            stv.assign(r.size(), 0);
            evals += (int64_t)r.size();
            return likelihood_grad_batch_core(gp, thetas.data(), (int64_t)r.size(), h, lk.data(), gr.data(), stv.data());
        },
        [&](const multistart::Round &, size_t q, LbfgsStart &m) {  // f(x) = -L(10^x), g = -dL/dx = -theta ln10 dL/dtheta
            const bool ok = stv[q] == EGX_STATUS_OK && std::isfinite(lk[q]);
            for (int i = 0; i < h; i++) gx[i] = ok ? -thetas[q * h + i] * ln10 * gr[q * h + i] : 0.0;
            m.tell(ok ? -lk[q] : inf, gx);
        },
        rc);
    EGX_RC(rc);
    std::vector<StartResult> results;
    for (const LbfgsStart &m : mach) results.push_back(StartResult{m.f, m.x, 0});
    if (n_evals_out) *n_evals_out = evals;
    const std::vector<double> th = fit::winner_theta(theta0s, h, active, fit::best_start(results), theta0s);
    return do_finalize(gp, th.data(), h);
}

// ThetaTuning::Full across MODELS: the tuned fit of every expert of a mixture (crates/moe/src/algorithm.rs:167-177 -> :209-262 ->
// GpValidParams::fit -> the multistart COBYLA of crates/gp/src/algorithm.rs:921-945), the k x n_starts COBYLA machines advanced
// in lock-step: per round and start index, the trial points of all models whose machine still asks are ONE lock-step
// evaluation across the group's slab (what egx_gp_likelihood_multi does).  A machine only ever sees the values of its own
// model, and a model's evaluation does not depend on its companions, so every member walks the trajectory it walks under
// egx_gp_fit on a one-workspace handle: theta*, likelihood and predictions are the same bits.
int32_t egx_gp_fit_multi(egx_gp *const *gps, int32_t k, const double *theta0s, int64_t n_starts, const double *lo, const double *hi,
                         int64_t bounds_len, int64_t max_eval, int64_t *n_evals_out) {
    if (!gps || k < 1 || !theta0s || !lo || !hi || n_starts < 1) {
        set_error("NULL argument / no start point");
        return EGX_ERR_INVALID_VALUE;
    }
    std::vector<std::unique_lock<std::shared_mutex>> locks;
    EGX_RC(lock_multi(gps, k, locks));
    const int h = gps[0]->h;
    for (int32_t m = 0; m < k; m++)
        if (gps[m]->h != h) {
            set_error("egx_gp_fit_multi: the models must have the same number of hyperparameters");
            return EGX_ERR_INVALID_VALUE;
        }
    fit::Log10Box box;
    EGX_RC(fit_box(lo, hi, bounds_len, h, theta0s, (int64_t)k * n_starts * h, fit::Dense, box));
    // the machines START-MAJOR, model-minor (theta0s is model-major): a round's points are contiguous per start index
    std::vector<int64_t> rows;
    for (int64_t st = 0; st < n_starts; st++)
        for (int32_t m = 0; m < k; m++) rows.push_back((int64_t)m * n_starts + st);
    std::vector<CobylaBox> mach = fit::cobyla_machines(theta0s, h, rows, box, fit::cobyla_budget(h, max_eval));
    const std::vector<int> active = fit::all_active(h);
    std::vector<egx_gp *> sub;
    std::vector<int32_t> stt;
    std::vector<double> thetas, lk;
    int rc;
    multistart::run(
        mach,
        [&](const multistart::Round &r) {
            fit::round_thetas(r, theta0s, h, active, thetas);
            lk.assign(r.size(), 0.0), stt.assign(r.size(), 0);
            // start index st of every model whose machine still asks: one lock-step evaluation
            return fit::for_each_start(r, k, [&](int64_t, size_t q0, size_t count) {
                sub.clear();
                for (size_t q = q0; q < q0 + count; q++) sub.push_back(gps[r.who[q] % (size_t)k]);
                return eval_multi_locked(sub.data(), (int32_t)count, thetas.data() + q0 * (size_t)h, h, false, lk.data() + q0,
                                         stt.data() + q0);
            });
        },
        [&](const multistart::Round &, size_t q, CobylaBox &m) { m.tell(fit::cobyla_objective(stt[q] == EGX_STATUS_OK, lk[q])); }, rc);
    EGX_RC(rc);
    // the reduction over every model's starts, then ONE lock-step finalize
    std::vector<double> best;
    for (int32_t m = 0; m < k; m++) {
        std::vector<StartResult> results;
        for (int64_t st = 0; st < n_starts; st++) results.push_back(fit::cobyla_result(mach[(size_t)(st * k + m)]));
        const double *theta0 = theta0s + (size_t)m * n_starts * h;
        const std::vector<double> th = fit::winner_theta(theta0, h, active, fit::best_start(results, n_evals_out ? n_evals_out + m : nullptr), theta0);
        best.insert(best.end(), th.begin(), th.end());
    }
    return eval_multi_locked(gps, k, best.data(), h, true, nullptr, nullptr);
}

// ---- kernel-level entry points ------------------------------------------------------------------
}  // extern "C"
