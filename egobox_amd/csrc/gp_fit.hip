// Optimiser drivers above the dense likelihood (GpValidParams::fit with ThetaTuning::Full / Partial, algorithm.rs:873-960,
// optimization.rs:26-169): multistart COBYLA on one model (egx_gp_fit, egx_gp_fit_partial, egx_sweep_fit) and on the models of a
// group (egx_gp_fit_multi), the theta-gradient of the likelihood and a projected L-BFGS on it -- both of
// one handle's candidates and of a group's members (egx_gp_likelihood_grad_multi, egx_gp_fit_lbfgs_multi).  Every
// driver is LOCK-STEP: multistart::run over one machine per start, a round's points in one evaluation call.  The box, the
// budget, the machines, the reduction and the winner are fit_starts.h's; this file holds only what touches a handle.
#include "gp_handle.h"
#include "kpls_coef.h"
#include "grad_runs.h"

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
// the gradient scratch of one evaluation's workspace, and |w_star| of its owner on the device (KPLS + Matern)
static int ensure_grad_ws(egx_gp *gp, Workspace &w) {
    EGX_RC(w.d_gpart.alloc((size_t)grad_partial_doubles(gp->d)));
    EGX_RC(w.d_gout.alloc((size_t)(gp->d + 64)));
    EGX_RC(w.h_gout.alloc((size_t)(gp->d + 64)));
    if (gp->has_w && !gp->d_wabs) {
        std::vector<double> wabs(gp->w_star.size());
        for (size_t e = 0; e < wabs.size(); e++) wabs[e] = std::fabs(gp->w_star[e]);
        EGX_RC(gp->d_wabs.alloc(wabs.size()));
        EGX_HIP_CHECK(hipMemcpy(gp->d_wabs, wabs.data(), sizeof(double) * wabs.size(), hipMemcpyHostToDevice));
    }
    return EGX_SUCCESS;
}
// ... of the workspaces ws_lo .. ws_lo + nuse - 1 of ONE handle, with as many C^-T buffers in its slab_W
static int ensure_grad_scratch(egx_gp *gp, int ws_lo, int nuse) {
    const size_t sq = (size_t)gp->n_pad * gp->n_pad;
    if (gp->slab_W_count < nuse) {
        gp->slab_W_count = 0;
        EGX_RC(gp->slab_W.alloc(sq * (size_t)nuse));
        gp->slab_W_count = nuse;
    }
    for (int i = ws_lo; i < ws_lo + nuse; i++) EGX_RC(ensure_grad_ws(gp, gp->ws[i]));
    return EGX_SUCCESS;
}

// The gradient stages of `count` evaluations in LOCK-STEP on stream st: evaluation j is of the training set of owners[j] on the
// workspace wss[j] (its factor in place, rho in d_rhs), its C^-T -- it rode along the factorisation -- in W0 + j n_pad^2.  The
// workspaces are consecutive slots of ONE slab, like enqueue_eval_core's (gp_host.hip): the candidates of one handle
// (owners[j] = gp, wss[j] = &gp->ws[w0 + j], W0 in gp->slab_W), or the members of a run of a group (owners[j] = gps[j], wss[j] =
// &gps[j]->ws[0], W0 in GroupSlabs::W).  Every stage has the entry as a grid coordinate and reads nothing of its companions.
// pre != 0: every entry of the run has hcols == 1 and positive coefficients -- the trace kernel takes the prescaled form
static int enqueue_grad_run(egx_gp *const *owners, Workspace *const *wss, int count, hipStream_t st, double *W0, const double *inv_s2,
                            int hcols, int pre) {
    const egx_gp *gp = owners[0];  // (the shape is every owner's)
    const int n = gp->n, n_pad = gp->n_pad;
    const int64_t sq = (int64_t)n_pad * n_pad;
    GemvBatchPtrs gv;
    EvalBatchPtrs sc;  // (xT, coef, xs alone are read: launch_scale_rows_batch)
    GradBatch gb;
    gb.count = count;
    for (int j = 0; j < count; j++) {
        Workspace &w = *wss[j];
        gv.y[j] = w.d_rhs, gv.z[j] = w.d_vec;
        sc.xT[j] = owners[j]->d_xT, sc.coef[j] = w.d_coef, sc.xs[j] = w.d_xs;
        gb.xT[j] = owners[j]->d_xT;
        gb.xs[j] = w.d_xs;
        gb.coef[j] = w.d_coef;
        gb.gamma[j] = w.d_vec;
        gb.rneg[j] = w.M;
        gb.inv_s2[j] = inv_s2[j];
        gb.part[j] = w.d_gpart;
        gb.out[j] = w.d_gout;
    }
    for (int j = count; j < kLockstepMax; j++) {
        gv.y[j] = nullptr, gv.z[j] = nullptr;
        sc.xT[j] = sc.coef[j] = nullptr, sc.xs[j] = nullptr;
        gb.xT[j] = gb.xs[j] = gb.coef[j] = gb.gamma[j] = gb.rneg[j] = nullptr;
        gb.inv_s2[j] = 0.0;
        gb.part[j] = gb.out[j] = nullptr;
    }
    EGX_RC(launch_uptri_gemv_batch(st, W0, sq, n_pad, n, gv, count));  // gamma = W rho
    GemmBatch gbm;
    gbm.count = count;
    gbm.sC = gp->stride_M;
    gbm.sA = gbm.sB = sq;
    EGX_RC(launch_syrk_uptri_neg(st, wss[0]->M, gp->ld, W0, n_pad, n_pad, &gbm));
    const int nout = (hcols == 1) ? gp->d : gp->h;
    if (pre) EGX_RC(launch_scale_rows_batch(st, sc, count, n_pad, gp->d));  // (K1 may have taken its LDS-only form)
    EGX_RC(launch_grad_accum(st, gp->corr, n_pad, n, gp->d, hcols, hcols > 1 ? gp->d_wabs.p : nullptr, nout, gp->ld, gb, pre));
    for (int j = 0; j < count; j++) {
        Workspace &w = *wss[j];
        EGX_HIP_CHECK(hipMemcpyAsync(w.h_gout, w.d_gout, sizeof(double) * nout, hipMemcpyDeviceToHost, st));
    }
    return EGX_SUCCESS;
}

// What the host half of entry j's likelihood (finish_eval with keep = 2) means for its gradient: the result row, whether it has
// a gradient, 1 / sigma2, and which form of the trace kernel ITS OWN coefficients allow
static bool grad_entry(const EvalResult &res, int hcols, const std::vector<double> &coef, double &lkh, int32_t &status, double &inv_s2,
                       char &pre) {
    lkh = res.lkh;
    status = res.status;
    inv_s2 = 0.0, pre = 0;
    if (res.status != EGX_STATUS_OK || !(res.sigma2n > 0.0) || !std::isfinite(res.lkh)) return false;
    inv_s2 = 1.0 / res.sigma2n;
    // the prescaled form divides by the coefficient once per output: an entry's OWN coefficients decide (never its
    // companions': the kernel choice must not depend on the batch)
    pre = gradruns::prescaled(hcols, coef.data(), (int)coef.size()) ? 1 : 0;
    return true;
}

// dL/dtheta (h) from the kernel's sums over the coefficients (nout): the chain rule of make_coef
static void grad_chain_rule(const egx_gp *gp, const double *gsum, int hcols, const std::vector<double> &coef,
                            const std::vector<double> &thfull, double *grad) {
    kpls::chain_rule(gp->corr, gp->d, gp->h, gp->has_w ? gp->w_star.data() : nullptr, hcols, coef.data(), thfull.data(), gsum,
                     std::log(10.0), grad);  // kpls_coef.h
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
        std::vector<egx_gp *> owners((size_t)cnt, gp);
        std::vector<Workspace *> wss((size_t)cnt);
        for (int j = 0; j < cnt; j++) {
            Workspace &w = gp->ws[w0 + j];
            wss[(size_t)j] = &w;
            EvalResult res;
            EGX_RC(finish_eval(gp, w, res, 2));
            const int64_t c = sl.cand[j];
            if (!grad_entry(res, sl.hcols, sl.coefs[j], lkh[c], status[c], inv_s2[j], sl.pre[j])) continue;
            sl.ok[j] = 1;
            EGX_RC(upload_rho(gp, w, res, st));
        }
        // each run (grad_runs.h) is one lock-step launch sequence
        const int64_t sq = (int64_t)gp->n_pad * gp->n_pad;
        for (const gradruns::Run &r : gradruns::split(sl.ok.data(), sl.pre.data(), cnt))
            EGX_RC(enqueue_grad_run(owners.data() + r.first, wss.data() + r.first, r.count, st,
                                    gp->slab_W + (int64_t)(i * g.width + r.first) * sq, inv_s2.data() + r.first, sl.hcols, r.pre));
        return EGX_SUCCESS;
    };
    return run_slots(gp, g, src, k, admit, enqueue, advance);
}

// Likelihood + gradient of `len` members of ONE group in consecutive slots (1 <= len <= run_len_multi's cap), none with a NaN
// theta, in LOCK-STEP: member j at row j of thetas, on its own workspace 0, its C^-T in its slot of the group's slab
// (GroupSlabs::W).  Caller holds every member's lock and has set the device.  The sequence is likelihood_grad_batch_core's for
// one slot -- the evaluation with the rider, the host halves, the gradient stages, the chain rule -- on the same kernels, so a
// member's row is bit for bit its own egx_gp_likelihood_grad.  A member whose host half FAILS (a HIP error, not a status) keeps
// its zero gradient and gives first_rc; the others finish.
static int grad_run_members(egx_gp *const *gps, int len, const double *thetas, int64_t theta_len, double *lkh, double *grad,
                            int32_t *status, int &first_rc) {
    egx_gp *lead = gps[0];
    const int h = lead->h;
    const int64_t sq = (int64_t)lead->n_pad * lead->n_pad;
    std::vector<std::vector<double>> coefs((size_t)len), thfull((size_t)len);
    int hcols = 1;
    for (int j = 0; j < len; j++) EGX_RC(make_coef(gps[j], thetas + (size_t)j * theta_len, theta_len, coefs[(size_t)j], hcols, &thfull[(size_t)j]));
    {   // the group's C^-T slab, as ensure_winv allocates it (members of a group may be called from different threads)
        std::lock_guard<std::mutex> lk(lead->group->winv_mu);
        EGX_RC(lead->group->W.alloc((size_t)sq * lead->group->k));
    }
    std::vector<Workspace *> wss((size_t)len);
    for (int j = 0; j < len; j++) {
        egx_gp *gp = gps[j];
        wss[(size_t)j] = &gp->ws[0];
        EGX_RC(ensure_grad_ws(gp, gp->ws[0]));
        // the rider overwrites this member's slot of the slab, which also caches C^-T of its FITTED factor for the x-gradients
        // (ensure_winv): the member is un-fitted, and the slot no longer is that of any fit of it
        gp->fitted = false;
        gp->winv_epoch = ~(uint64_t)0;
    }
    double *W0 = lead->group->W.p + (int64_t)lead->group_slot * sq;
    RunGuard guard{gps, len};
    EGX_RC(enqueue_eval_members(gps, len, coefs.data(), hcols, W0));
    const hipStream_t st = lead->ws[0].eval_stream;
    std::vector<HostHalf> hh((size_t)len);
    host_halves(gps, len, 2, hh.data());
    std::vector<double> inv_s2((size_t)len, 0.0);
    std::vector<char> ok((size_t)len, 0), pre((size_t)len, 0);
    for (int j = 0; j < len; j++) {
        if (hh[j].rc != EGX_SUCCESS) {
            lkh[j] = -std::numeric_limits<double>::infinity(), status[j] = EGX_STATUS_OK;  // (the call returns the error)
            set_error(hh[j].err);
            if (first_rc == EGX_SUCCESS) first_rc = hh[j].rc;
            continue;
        }
        if (!grad_entry(hh[j].res, hcols, coefs[(size_t)j], lkh[j], status[j], inv_s2[(size_t)j], pre[(size_t)j])) continue;
        ok[(size_t)j] = 1;
        EGX_RC(upload_rho(gps[j], *wss[(size_t)j], hh[j].res, st));
    }
    for (const gradruns::Run &r : gradruns::split(ok.data(), pre.data(), len))
        EGX_RC(enqueue_grad_run(gps + r.first, wss.data() + r.first, r.count, st, W0 + (int64_t)r.first * sq, inv_s2.data() + r.first,
                                hcols, r.pre));
    EGX_HIP_CHECK(hipStreamSynchronize(st));
    guard.synced = true;
    for (int j = 0; j < len; j++)
        if (ok[(size_t)j]) grad_chain_rule(gps[j], wss[(size_t)j]->h_gout, hcols, coefs[(size_t)j], thfull[(size_t)j], grad + (size_t)j * h);
    return EGX_SUCCESS;
}

// egx_gp_likelihood_grad_multi under the members' locks: row j of thetas for gps[j]
int likelihood_grad_multi_locked(egx_gp *const *gps, int32_t k, const double *thetas, int64_t theta_len, double *lkh, double *grad,
                                 int32_t *status) {
    const int h = gps[0]->h;
    int first_rc = EGX_SUCCESS;
    for (int i = 0; i < k;) {
        const int len = run_len_multi(gps, k, i);
        EGX_RC(set_device(gps[i]));
        if (!gps[i]->group) {  // a lone handle: the lone core on its workspace 0
            gps[i]->fitted = false;
            EGX_RC(likelihood_grad_batch_core(gps[i], thetas + (size_t)i * theta_len, 1, theta_len, lkh + i, grad + (size_t)i * h, status + i));
            i++;
            continue;
        }
        // a run of members: a NaN theta is answered at once (algorithm.rs:885-891) and cuts the run -- the lock-step launches
        // take CONSECUTIVE slots
        for (int j = 0; j < len;) {
            egx_gp *gp = gps[i + j];
            const double *th = thetas + (size_t)(i + j) * theta_len;
            for (int l = 0; l < h; l++) grad[(size_t)(i + j) * h + l] = 0.0;
            if (has_nan(th, theta_len)) {
                gp->fitted = false;
                lkh[i + j] = -std::numeric_limits<double>::infinity(), status[i + j] = EGX_STATUS_NAN_THETA;
                j++;
                continue;
            }
            int e = j + 1;
            while (e < len && !has_nan(thetas + (size_t)(i + e) * theta_len, theta_len)) {
                for (int l = 0; l < h; l++) grad[(size_t)(i + e) * h + l] = 0.0;
                e++;
            }
            EGX_RC(grad_run_members(gps + i + j, e - j, th, theta_len, lkh + i + j, grad + (size_t)(i + j) * h, status + i + j, first_rc));
            j = e;
        }
        i += len;
    }
    return first_rc;
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

// the locks of a multi-model call whose models must agree on h
static int32_t lock_same_h(const char *who, egx_gp *const *gps, int32_t k, std::vector<std::unique_lock<std::shared_mutex>> &locks) {
    EGX_RC(lock_multi(gps, k, locks));
    for (int32_t m = 1; m < k; m++)
        if (gps[m]->h != gps[0]->h) {
            set_error(std::string(who) + ": the models must have the same number of hyperparameters");
            return EGX_ERR_INVALID_VALUE;
        }
    return EGX_SUCCESS;
}

int32_t egx_gp_likelihood_grad_multi(egx_gp *const *gps, int32_t k, const double *thetas, int64_t theta_len, double *lkh,
                                     double *grads, int32_t *status) {
    if (!gps || k < 1 || !thetas || !lkh || !grads || !status) {
        set_error("NULL argument / no model");
        return EGX_ERR_INVALID_VALUE;
    }
    std::vector<std::unique_lock<std::shared_mutex>> locks;
    EGX_RC(lock_same_h("egx_gp_likelihood_grad_multi", gps, k, locks));
    if (theta_len != 1 && theta_len != gps[0]->h) {
        set_error("theta should be either 1-dim or dim of xtrain (w_star.ncols()), got " + std::to_string(theta_len));
        return EGX_ERR_INVALID_VALUE;
    }
    return likelihood_grad_multi_locked(gps, k, thetas, theta_len, lkh, grads, status);
}

// egx_gp_fit_lbfgs across MODELS: the k x n_starts LbfgsStart machines START-MAJOR, model-minor as egx_gp_fit_multi lays out its
// COBYLA machines; per round and start index, the trial points of all models whose machine still asks are ONE
// egx_gp_likelihood_grad_multi evaluation.  A machine only ever sees the values of its own model, and those are the bits of the
// model's lone call, so every member walks the trajectory it walks under egx_gp_fit_lbfgs on a one-workspace handle.
int32_t egx_gp_fit_lbfgs_multi(egx_gp *const *gps, int32_t k, const double *theta0s, int64_t n_starts, const double *lo, const double *hi,
                               int64_t bounds_len, int64_t max_iter, int64_t *n_evals_out) {
    if (!gps || k < 1 || !theta0s || !lo || !hi || n_starts < 1) {
        set_error("NULL argument / no start point");
        return EGX_ERR_INVALID_VALUE;
    }
    std::vector<std::unique_lock<std::shared_mutex>> locks;
    EGX_RC(lock_same_h("egx_gp_fit_lbfgs_multi", gps, k, locks));
    const int h = gps[0]->h;
    fit::Log10Box box;
    EGX_RC(fit_box(lo, hi, bounds_len, h, theta0s, (int64_t)k * n_starts * h, fit::Dense, box));
    if (max_iter < 1) max_iter = 50;
    std::vector<int64_t> rows;
    for (int64_t st = 0; st < n_starts; st++)
        for (int32_t m = 0; m < k; m++) rows.push_back((int64_t)m * n_starts + st);
    std::vector<LbfgsStart> mach = fit::lbfgs_machines(theta0s, h, rows, box, max_iter);
    const double ln10 = std::log(10.0), inf = std::numeric_limits<double>::infinity();
    const std::vector<int> active = fit::all_active(h);
    std::vector<int64_t> evals((size_t)k, 0);
    std::vector<egx_gp *> sub;
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
            return fit::for_each_start(r, k, [&](int64_t, size_t q0, size_t count) {
                sub.clear();
                for (size_t q = q0; q < q0 + count; q++) {
                    sub.push_back(gps[r.who[q] % (size_t)k]);
                    evals[r.who[q] % (size_t)k]++;
                }
                return likelihood_grad_multi_locked(sub.data(), (int32_t)count, thetas.data() + q0 * (size_t)h, h, lk.data() + q0,
                                                    gr.data() + q0 * (size_t)h, stv.data() + q0);
            });
        },
        [&](const multistart::Round &, size_t q, LbfgsStart &m) {  // f(x) = -L(10^x), g = -dL/dx = -theta ln10 dL/dtheta
            const bool ok = stv[q] == EGX_STATUS_OK && std::isfinite(lk[q]);
            for (int i = 0; i < h; i++) gx[i] = ok ? -thetas[q * h + i] * ln10 * gr[q * h + i] : 0.0;
            m.tell(ok ? -lk[q] : inf, gx);
        },
        rc);
    EGX_RC(rc);
    // the reduction over every model's starts, then ONE lock-step finalize
    std::vector<double> best;
    for (int32_t m = 0; m < k; m++) {
        std::vector<StartResult> results;
        for (int64_t st = 0; st < n_starts; st++) {
            const LbfgsStart &ms = mach[(size_t)(st * k + m)];
            results.push_back(StartResult{ms.f, ms.x, 0});
        }
        if (n_evals_out) n_evals_out[m] = evals[(size_t)m];
        const double *theta0 = theta0s + (size_t)m * n_starts * h;
        const std::vector<double> th = fit::winner_theta(theta0, h, active, fit::best_start(results), theta0);
        best.insert(best.end(), th.begin(), th.end());
    }
    return eval_multi_locked(gps, k, best.data(), h, true, nullptr, nullptr);
}

// ---- kernel-level entry points ------------------------------------------------------------------
}  // extern "C"
