// PENDING POINTS of an infill handle (egx_infill_push_pending; the q_points loop of crates/ego/src/solver/solver_impl.rs:622-791).
// The handle keeps up to 16 virtual observations and conditions every (lone, dense) surrogate on them in closed form
// (pending_math.h) instead of refitting it: right after expert_tile (infill_eval.hip), while h->xqT still holds the model's
// normalised tile, k_pending_cross contracts the tile against the model's training points followed by the pending ones with
// the extended weight matrix W^ = [W_v ; I_q] and k_pending_finish rewrites the tile's mean / var / gmean / gvar in place
// (kernels_pending.hip) -- nothing downstream changes.  A push runs the new point's own sequence once (a tile holding one
// point) WITHOUT the conditioning, keeps the weight column posterior_weights / posterior_weights_trend made for it and its
// -dneg as column q of W^ / t_q, takes its covariances with the points already pending from the same two kernels, and borders
// chol(S), alpha and sigma2' on the host.  With q = 0 none of this runs: the launch sequence is that of infill_eval.hip, bit
// for bit.
#include "infill_handle.h"

using namespace egx;

namespace egx {

std::atomic<int> g_pending_composed{0};

// the fused contraction where it applies, unless the composed form is asked for (egx_set_tuning "pending_composed")
static bool pending_composed(int d) { return d > kPendingMaxD || g_pending_composed.load() != 0; }

// A push (cap) takes the tile's cross-covariances with the points already pending, then captures query 0's weights.
int pending_tile(egx_infill *h, hipStream_t st, int js, const TileOut &o, PushCapture *cap) {
    const int d = h->d;
    PendModel &pm = h->pend[js];
    const egx_gp *gp = h->models[h->surr[js].first].gp;
    if (h->q > 0) {
        const int nz = gp->n + h->q;
        const bool g = o.gmean && !cap;
        PendingFinish f;
        f.composed = pending_composed(d);
        if (!f.composed) {
            f.nsplit_c = f.nsplit_g = pending_splits(nz);
            EGX_RC(launch_pending_cross(st, gp->corr, h->xqT.p, pm.ZT.p, pm.ldz, nz, d, gp->d_fit_coef, gp->fit_hcols, pm.W.p, h->q,
                                        f.nsplit_c, h->pc_c.p, g ? h->pc_g.p : nullptr));
        } else {  // what one writes without the kernel: per column the existing contractions over Z with w_v as the weight vector
            f.nsplit_c = mean_splits((int)pm.ldz, kTile), f.nsplit_g = xgrad_splits(nz, kTile);
            for (int v = 0; v < h->q; v++) {
                const double *wv = pm.Wc.p + (size_t)v * pm.ldz;
                EGX_RC(launch_predict_mean(st, gp->corr, h->xqT.p, kTile, kTile, pm.ZT.p, pm.ldz, (int)pm.ldz, d, gp->d_fit_coef,
                                           gp->fit_hcols, wv, h->pc_c.p + (size_t)v * f.nsplit_c * kTile, f.nsplit_c));
                if (g)
                    EGX_RC(launch_xgrad(st, gp->corr, h->xqT.p, kTile, kTile, pm.ZT.p, pm.ldz, nz, d, gp->d_fit_coef, gp->fit_hcols, wv,
                                        0, 1, f.nsplit_g, h->pc_g.p + (size_t)v * f.nsplit_g * kTile * d));
            }
        }
        f.q = h->q, f.d = d, f.p = gp->p;
        f.xqT = h->xqT.p, f.fidx = gp->d_fidx, f.tv = pm.tv.p, f.small = pm.small.p, f.outc = h->pc_c.p, f.outg = g ? h->pc_g.p : nullptr;
        f.x_std = dev_xnorm(gp) + d;
        f.sigma2 = gp->sigma2, f.sigma2c = pm.sigma2c, f.y_std = gp->y_std;
        if (cap) {
            f.emit = cap->emit.p + (size_t)js * kTile * pending::kLd;
        } else {
            f.mean = o.mean, f.var = o.var, f.gmean = g ? o.gmean : nullptr, f.gvar = g ? o.gvar : nullptr;
        }
        EGX_RC(launch_pending_finish(st, f));
    }
    if (cap)
        EGX_RC(launch_pending_capture(st, h->Wt.p, h->dneg.p, h->xqT.p, gp->n, d, gp->p, h->q, pm.W.p, pm.Wc.p, pm.tv.p, pm.ZT.p,
                                      pm.ldz));
    return EGX_SUCCESS;
}

int check_pending(const egx_infill *h) {
    for (size_t js = 0; js < h->pend.size() && h->q > 0; js++) {
        const egx_gp *gp = h->models[h->surr[js].first].gp;
        if (gp->fit_epoch != h->pend[js].epoch || gp->n != h->pend[js].n)
            return fail(EGX_ERR_INVALID_VALUE, "infill: " + infill_who(h, h->surr[js].first) +
                " was refitted since its pending points were pushed (call egx_infill_clear_pending)");
    }
    return EGX_SUCCESS;
}

}  // namespace egx

namespace {

// every surrogate a lone dense model, d within the contraction's reach
int pending_supported(const egx_infill *h) {
    for (size_t js = 0; js < h->surr.size(); js++) {
        const Surrogate &sg = h->surr[js];
        if (sg.k >= 2 || h->models[sg.first].sparse())
            return fail(EGX_ERR_UNSUPPORTED, "infill: pending points are not supported on surrogate " + std::to_string(js) +
                (sg.k >= 2 ? " (a mixture of " + std::to_string(sg.k) + " experts)" : " (a sparse model)"));
    }
    if (h->d > 1024)  // (the finish keeps 16 d doubles of one point in LDS)
        return fail(EGX_ERR_UNSUPPORTED, "infill: pending points need d <= 1024 (d " + std::to_string(h->d) + ")");
    return EGX_SUCCESS;
}

// the first push of a batch: Z <- the model's normalised training points, W^ and t_v zeroed, for the model's current fitted state
int pending_begin(egx_infill *h, hipStream_t st) {
    const int d = h->d;
    h->pend.resize(h->surr.size());
    for (size_t js = 0; js < h->surr.size(); js++) {
        PendModel &pm = h->pend[js];
        const egx_gp *gp = h->models[h->surr[js].first].gp;
        pm.ldz = round_up((int64_t)gp->n + pending::kMaxPending, 64);
        EGX_RC(pm.ZT.alloc((size_t)d * pm.ldz));
        EGX_RC(pm.W.alloc((size_t)(gp->n + pending::kMaxPending) * pending::kLd));
        EGX_RC(pm.Wc.alloc((size_t)pending::kMaxPending * pm.ldz));
        EGX_HIP_CHECK(hipMemsetAsync(pm.Wc.p, 0, sizeof(double) * (size_t)pending::kMaxPending * pm.ldz, st));
        EGX_RC(pm.tv.alloc((size_t)pending::kMaxPending * gp->p));
        EGX_RC(pm.small.alloc((size_t)pending::kLd * pending::kLd + pending::kMaxPending));
        EGX_HIP_CHECK(hipMemsetAsync(pm.ZT.p, 0, sizeof(double) * (size_t)d * pm.ldz, st));
        EGX_HIP_CHECK(hipMemsetAsync(pm.W.p, 0, sizeof(double) * (size_t)(gp->n + pending::kMaxPending) * pending::kLd, st));
        EGX_HIP_CHECK(hipMemsetAsync(pm.tv.p, 0, sizeof(double) * (size_t)pending::kMaxPending * gp->p, st));
        EGX_HIP_CHECK(hipMemcpy2DAsync(pm.ZT.p, sizeof(double) * pm.ldz, gp->d_xT, sizeof(double) * gp->n_pad, sizeof(double) * gp->n,
                                       d, hipMemcpyDeviceToDevice, st));
        pm.n = gp->n, pm.epoch = gp->fit_epoch, pm.sigma2c = gp->sigma2;
        std::fill(pm.L.begin(), pm.L.end(), 0.0);
        std::fill(pm.alpha.begin(), pm.alpha.end(), 0.0);
        std::fill(pm.delta.begin(), pm.delta.end(), 0.0);
    }
    return EGX_SUCCESS;
}

// the handle's and the models' locks are held
int push_locked(egx_infill *h, const double *x, const double *y) {
    const int nm = (int)h->surr.size(), d = h->d, q = h->q;
    EGX_RC(check_fitted(h));
    EGX_RC(pending_supported(h));
    EGX_RC(check_specs(h));
    EGX_RC(check_pending(h));
    if (q >= pending::kMaxPending) return fail(EGX_ERR_INVALID_VALUE, "infill: at most " + std::to_string(pending::kMaxPending) + " pending points");
    for (int i = 0; i < d; i++)
        if (!std::isfinite(x[i])) return fail(EGX_ERR_INVALID_VALUE, "infill: pending point has a non-finite coordinate " + std::to_string(i));
    for (int j = 0; j < nm; j++)
        if (!std::isfinite(y[j]))
            return fail(EGX_ERR_INVALID_VALUE, "infill: pending point has a non-finite value for surrogate " + std::to_string(j));
    EGX_HIP_CHECK(hipSetDevice(h->device));
    hipStream_t st = h->models[0].stream();
    std::vector<double> xc((size_t)d);
    for (int i = 0; i < d; i++) xc[i] = query_coord(h->models[0].gp, x, i);
    if (q == 0) {
        const int rc = pending_begin(h, st);
        if (rc) return settle_failed(h, rc);
    }
    // the point's own sequence on every model, unconditioned and with gradients (the weights), and its covariances with the
    // points already pending
    PushCapture cap;
    EGX_RC(cap.emit.alloc((size_t)nm * kTile * pending::kLd));
    std::vector<double> mean((size_t)nm), var((size_t)nm), gm((size_t)nm * d), gv((size_t)nm * d);
    egx_infill_parts parts{mean.data(), var.data(), gm.data(), gv.data()};
    EGX_RC(eval_guarded(h, xc.data(), 1, nullptr, nullptr, &parts, nullptr, nullptr, &cap));
    std::vector<double> c((size_t)nm * pending::kLd, 0.0);
    if (q > 0)
        EGX_HIP_CHECK(hipMemcpy2D(c.data(), sizeof(double) * pending::kLd, cap.emit.p, sizeof(double) * kTile * pending::kLd,
                                  sizeof(double) * pending::kLd, nm, hipMemcpyDeviceToHost));
    // border chol(S), alpha and sigma2' of every model on copies: nothing is kept unless every pivot holds
    std::vector<std::vector<double>> Ln((size_t)nm), an((size_t)nm), dn((size_t)nm);
    std::vector<double> s2((size_t)nm);
    for (int js = 0; js < nm; js++) {
        PendModel &pm = h->pend[js];
        const egx_gp *gp = h->models[h->surr[js].first].gp;
        Ln[js] = pm.L, dn[js] = pm.delta, an[js].assign(pending::kMaxPending, 0.0);
        const double unit = gp->sigma2 > 0.0 ? var[js] / gp->sigma2 : 0.0;  // k(x_v, x_v) = s^2(x_v)
        if (!pending::chol_border(Ln[js].data(), q, c.data() + (size_t)js * pending::kLd, unit + gp->nugget))
            return fail(EGX_ERR_LINALG, "infill: pending point " + std::to_string(q) +
                ": the covariance of the pending points is not positive " "definite for surrogate " + std::to_string(js) +
                " (a point pushed twice, or on a training point)");
        dn[js][q] = (y[js] - mean[js]) / gp->y_std;
        const double quad = pending::solve_alpha(Ln[js].data(), q + 1, dn[js].data(), an[js].data());
        s2[js] = pending::sigma2_conditioned(gp->sigma2, gp->y_std, gp->n, q + 1, quad);
    }
    std::vector<double> up((size_t)pending::kLd * pending::kLd + pending::kMaxPending);
    for (int js = 0; js < nm; js++) {
        std::copy(Ln[js].begin(), Ln[js].end(), up.begin());
        std::copy(an[js].begin(), an[js].end(), up.begin() + (size_t)pending::kLd * pending::kLd);
        EGX_HIP_CHECK(hipMemcpy(h->pend[js].small.p, up.data(), sizeof(double) * up.size(), hipMemcpyHostToDevice));
    }
    for (int js = 0; js < nm; js++) {
        PendModel &pm = h->pend[js];
        pm.L = Ln[js], pm.alpha = an[js], pm.delta = dn[js], pm.sigma2c = s2[js];
    }
    h->pend_x.insert(h->pend_x.end(), xc.begin(), xc.end());
    h->pend_y.insert(h->pend_y.end(), y, y + nm);
    h->q = q + 1;
    return EGX_SUCCESS;
}

}  // namespace

extern "C" {

int32_t egx_infill_push_pending(egx_infill *h, const double *x, const double *y) {
    if (!h || !x || !y) return fail(EGX_ERR_INVALID_VALUE, "NULL argument");
    std::lock_guard<std::mutex> lock(h->mu);
    ModelLocks locks(h);
    return push_locked(h, x, y);
}

int32_t egx_infill_clear_pending(egx_infill *h) {
    if (!h) return fail(EGX_ERR_INVALID_VALUE, "NULL handle");
    std::lock_guard<std::mutex> lock(h->mu);
    h->q = 0;
    h->pend_x.clear();
    h->pend_y.clear();
    return EGX_SUCCESS;
}

int32_t egx_infill_get_pending(egx_infill *h, int32_t *q, double *x, double *y, double *sigma2) {
    if (!h || !q) return fail(EGX_ERR_INVALID_VALUE, "NULL argument");
    std::lock_guard<std::mutex> lock(h->mu);
    ModelLocks locks(h);
    *q = h->q;
    if (x) std::copy(h->pend_x.begin(), h->pend_x.end(), x);
    if (y) std::copy(h->pend_y.begin(), h->pend_y.end(), y);
    if (sigma2)
        for (size_t js = 0; js < h->surr.size(); js++) {
            const Surrogate &sg = h->surr[js];
            if (h->q > 0) sigma2[js] = h->pend[js].sigma2c;
            else if (sg.k < 2) sigma2[js] = h->models[sg.first].sparse() ? h->models[sg.first].sg->sigma2 : h->models[sg.first].gp->sigma2;
            else sigma2[js] = std::numeric_limits<double>::quiet_NaN();  // a mixture has no single process variance
        }
    return EGX_SUCCESS;
}

int32_t egx_infill_virtual_point(egx_infill *h, const double *x, int32_t strategy, double *y) {
    if (!h || !y || (strategy != EGX_QEI_CL_MIN && !x)) return fail(EGX_ERR_INVALID_VALUE, "NULL argument");
    if (strategy < EGX_QEI_KB || strategy > EGX_QEI_CL_MIN) return fail(EGX_ERR_INVALID_VALUE, "infill: unknown q-EI strategy");
    std::lock_guard<std::mutex> lock(h->mu);
    ModelLocks locks(h);
    const int nm = (int)h->surr.size();
    if (strategy == EGX_QEI_CL_MIN) {  // y_data[[index_min, ic]] (solver_computations.rs:269-275)
        for (int js = 0; js < nm; js++) {
            const Surrogate &sg = h->surr[js];
            if (sg.k >= 2 || h->models[sg.first].sparse())
                return fail(EGX_ERR_UNSUPPORTED, "infill: the constant-liar minimum needs lone dense models (surrogate " + std::to_string(js) + ")");
            if (h->models[sg.first].gp->n != h->models[0].gp->n)
                return fail(EGX_ERR_INVALID_VALUE, "infill: the constant-liar minimum needs every model on the same rows (surrogate " +
                    std::to_string(js) + " has " + std::to_string(h->models[sg.first].gp->n) + ", the objective " +
                    std::to_string(h->models[0].gp->n) + ")");
        }
        const std::vector<double> &y0 = h->models[0].gp->y_raw;
        size_t imin = 0;
        for (size_t i = 1; i < y0.size(); i++)
            if (y0[i] < y0[imin]) imin = i;
        for (int js = 0; js < nm; js++) y[js] = h->models[h->surr[js].first].gp->y_raw[imin];
        return EGX_SUCCESS;
    }
    for (int i = 0; i < h->d; i++)
        if (!std::isfinite(x[i])) return fail(EGX_ERR_INVALID_VALUE, "infill: virtual point at a non-finite coordinate " + std::to_string(i));
    std::vector<double> mean((size_t)nm), var((size_t)nm);
    egx_infill_parts parts{mean.data(), var.data(), nullptr, nullptr};
    EGX_RC(eval_guarded(h, x, 1, nullptr, nullptr, &parts));
    const double conf = strategy == EGX_QEI_KB ? 0.0 : (strategy == EGX_QEI_KB_LB ? -3.0 : 3.0);
    y[0] = mean[0] + conf * std::sqrt(var[0]);
    for (int js = 1; js < nm; js++) y[js] = mean[js];
    return EGX_SUCCESS;
}

}  // extern "C"
