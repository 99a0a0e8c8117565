// EGO's infill criterion on fitted GPs, dense or sparse (crates/ego/src/criteria/{ei,wb2}.rs, utils/{logei_helper,cstr_pof}.rs,
// solver/solver_computations.rs:132-193, 297-475): the minimised objective and its x-gradient for m points in one call, from
// one objective model and k constraint models; the scaling pass.  (The lock-step multistarts on top of it: infill_optimize.hip;
// the pending points of a q-point batch: infill_pending.hip; the handle: infill_handle.h.)
//
// A call walks the points in tiles of EXACTLY kTile = 128 and, per tile, the models through the launch
// sequence of predict_impl / xgrad_impl (posterior_solve, posterior_weights, the split rules: gp_predict.hip); what those
// do on the host between their launches runs in the kernels of kernels_infill.hip, and k_infill_combine applies
// infill_math.h across the models.  One upload, one launch sequence per (tile, RUN of models), one combine, the copies back, ONE
// synchronisation: the count depends on the runs and on the number of tiles only.
//
// RUNS (infill_runs.h, egx_infill_get_runs).  Consecutive lone dense surrogates of one shape go through ONE launch sequence per
// tile, run_tile: the member is a grid coordinate of every kernel of it (the posterior batch of gp_predict.hip, the by-value
// member blocks of kernels_infill.hip), its blocks of the tile buffers sit at the strides of the run's shape.  A mean-only run
// takes the members' own pointers only; a full-sequence run reads factors, C^-T and -R^-1 F at one stride -- members of one
// group in consecutive slots.  With pending points, or while a push is captured, every run has length 1.  A member's arithmetic
// does not depend on its companions and the splits come from one member's shape: every output has the bits of runs of one.
// Every launch of a tile has the padded batch size 128, and the splits of the training range are functions of the model
// alone: the bits of a point do not depend on where it sits nor on its companions (tests/test_gpu_infill.py).
//
// The walk is tile -> run; a mixture or a sparse surrogate is a run of one walked expert by expert (a dense expert: run_tile with
// one member).  A lone expert writes the surrogate's slot of the tables,
// the experts of a mixture write the expert tables and ONE k_infill_mix launch per (tile, surrogate) recombines them into the
// slot (smooth: the weighted sums; hard: the expert of the first maximum of the responsibilities -- every expert still
// evaluates the whole tile, so that every launch keeps the padded batch of 128).
//
// A sparse expert writes the same table slots from its own tile sequence, sgp_expert_tile: the batched route of sgp_query
// (sgp_predict.hip) at the padded batch of 128 -- raw x, K(x, z) . (sigma2 vec) in split partial sums, K(x, z), the two block
// solves with their row reductions, k_infill_sgp_finish (var = egx_sgp_predict_var's: clamp, then + noise); with gradients the
// two transposed products with the cached inverse factors, launch_xgrad twice, k_infill_sgp_xgrad_finish (exactly 0 under the
// clamp).  Everything downstream reads slots only.  Its mean-only branch runs no solve and keeps the means' bits.
//
// CONSTRAINT STRATEGIES (egx_infill_set_cstr_strategy).  EGX_CSTR_INFILL folds the constraint surrogates into the objective (the
// above).  Under EGX_CSTR_MEAN / _UTB the objective carries no feasibility factor and the constraints are handed to the
// optimiser as c(x) <= 0 (egx_infill_eval_cstr, egx_infill_optimize_cstr; solver_infill_optim.rs:148-204).  Under MEAN nobody
// reads a constraint surrogate's variance, and its experts run the MEAN-ONLY branch of their sequence: prepare, predict_mean,
// the mean half of the trend tail (and, for gradients, ONE launch_xgrad with gamma and the mean half of its finish) -- no
// posterior_solve, no weights, no second contraction; the means keep the bits of the full sequence, which forms r . gamma
// before its solve as well.  A call that does not ask for anything of the constraint surrogates (egx_infill_eval without parts
// under MEAN / UTB) does not run them at all.
//
// ACTIVE COORDINATES (egx_infill_set_active; CoEGO).  While an activity is set, egx_infill_eval, egx_infill_eval_cstr and the
// optimisers' rounds go through eval_active: the compact rows are expanded on the host (infill_active.h), the call above runs
// full width with the experts' x-gradient contractions restricted to the listed columns (launch_xgrad's column list: the pair
// correlation once per pass of LISTED columns, +0.0 in the others), and the listed gradient columns are gathered on the host.
// Nothing else of the sequence changes, and every other caller of eval_guarded launches what it launched before.
#include "gmx_point.h"
#include "infill_handle.h"
#include "infill_runs.h"

using namespace egx;

static_assert(runs::kRunMax == kLockstepMax && runs::kRunTile == kTile, "infill_runs.h restates the launch widths");

namespace egx {

std::string infill_who(const egx_infill *h, int idx) {
    if (!h->mix_api) return "model " + std::to_string(idx);
    for (size_t j = 0; j < h->surr.size(); j++)
        if (idx < h->surr[j].first + h->surr[j].k)
            return "surrogate " + std::to_string(j) + " expert " + std::to_string(idx - h->surr[j].first);
    return "model " + std::to_string(idx);
}

int check_fitted(const egx_infill *h) {
    for (size_t e = 0; e < h->models.size(); e++)
        if (!h->models[e].fitted())
            return fail(EGX_ERR_NOT_FITTED, "infill: " + infill_who(h, (int)e) + " is not fitted (call " +
                (h->models[e].sparse() ? "egx_sgp_finalize or egx_sgp_fit" : "egx_gp_finalize or egx_gp_fit") + " first)");
    return EGX_SUCCESS;
}

// Mixed-integer models: every expert of every surrogate carries the same xtypes as expert 0 of the objective, or none does -- the
// points of a call are one design space.  Read from the models at EVERY call (as their fitted state is), under their locks.
// A sparse model carries none.
int check_specs(const egx_infill *h) {
    static const MixSpec none;
    auto spec = [](const ModelRef &r) -> const MixSpec & { return r.sparse() ? none : r.gp->xspec; };
    for (size_t e = 1; e < h->models.size(); e++)
        if (!spec(h->models[e]).same(spec(h->models[0])))
            return fail(EGX_ERR_INVALID_VALUE, "infill: " + infill_who(h, (int)e) + " and " + infill_who(h, 0) +
                " carry different xtypes (egx_gp_set_xtypes): all or none, the same spec");
    return EGX_SUCCESS;
}

int settle_failed(const egx_infill *h, int rc) {
    (void)hipStreamSynchronize(h->models[0].stream());
    (void)hipGetLastError();
    return rc;
}

}  // namespace egx

namespace {

// same d, same device as expert 0 of the objective
int check_shapes(egx_infill *h) {
    h->d = h->models[0].d();
    h->device = h->models[0].device();
    for (size_t e = 1; e < h->models.size(); e++) {
        if (h->models[e].d() != h->d)
            return fail(EGX_ERR_INVALID_VALUE, "infill: " + infill_who(h, (int)e) + " has " + std::to_string(h->models[e].d()) + " inputs, " +
                infill_who(h, 0) + " has " + std::to_string(h->d));
        if (h->models[e].device() != h->device)
            return fail(EGX_ERR_INVALID_VALUE, "infill: " + infill_who(h, (int)e) + " lives on device " + std::to_string(h->models[e].device()) +
                ", " + infill_who(h, 0) + " on device " + std::to_string(h->device));
    }
    // the x-gradient contraction of a sparse expert stages d * (hcols + 5) doubles; hcols = 1 unless it carries KPLS weights under
    // a Matern correlation (sgp_predict.hip)
    for (size_t e = 0; e < h->models.size(); e++) {
        if (!h->models[e].sparse()) continue;
        const int hc = h->models[e].sg->hcols;
        if (hc == 1 && (int64_t)h->d * 6 > 20480)
            return fail(EGX_ERR_UNSUPPORTED, "infill: " + infill_who(h, (int)e) + ": the x-gradients of a sparse model need 6 d <= 20480 (d " +
                std::to_string(h->d) + ")");
        if ((int64_t)h->d * (hc + 5) > 20480)
            return fail(EGX_ERR_UNSUPPORTED, "infill: " + infill_who(h, (int)e) + ": the x-gradients of a sparse KPLS model need d (hcols + 5) <= 20480 (d " +
                std::to_string(h->d) + ", hcols " + std::to_string(hc) + ")");
    }
    return EGX_SUCCESS;
}

// The launch sequence of a RUN of `len` dense models of one shape (infill_runs.h; ONE model is a run of one: an expert of a
// mixture, a surrogate that forms no run) for one tile: model jm[z] into o[z].  Every kernel takes the member as a grid
// coordinate and does a member's arithmetic the same way whatever its companions, and the splits come from one member's shape:
// a member's tables have the bits of its own run of one.  The tile buffers are laid out per member at the strides of the run's
// shape.  flag: the tile's flags, written by member 0 -- the first expert of the call, which can only lead a run -- or nullptr.
// The MEAN-ONLY branch (o[0].var nullptr: all members alike) is what the full sequence launches for mean / gmean and nothing
// else; it runs for constraint surrogates only, which never own the call's flags nor its cast points.
int run_tile(egx_infill *h, hipStream_t st, const int *jm, int len, int64_t t0, int mt, const TileOut *o, int *flag) {
    const int d = h->d;
    egx_gp *gps[kLockstepMax];
    for (int z = 0; z < len; z++) gps[z] = h->models[jm[z]].gp;
    const egx_gp *lead = gps[0];
    const int n = lead->n, n_pad = lead->n_pad, p = lead->p, rp = lead->rhs_pad, hcols = lead->fit_hcols;
    const int msplit = mean_splits(n_pad, kTile), nsplit = xgrad_splits(n, kTile);
    const bool mean_only = !o[0].var, want_g = o[0].gmean != nullptr;
    const int *cols = h->use_cols ? h->d_active.p : nullptr;  // active coordinates: the contractions' column list
    const int ncols = h->use_cols ? (int)h->active.size() : 0;
    if (mean_only) flag = nullptr;
    const bool prescaled = hcols == 1 && predict_mean_prescaled(d, hcols);
    PosteriorBatch pb, pm;  // pm: launch_predict_mean's, whose training inputs are the prescaled ones where that form exists
    pb.count = len;
    pb.sq = (int64_t)d * kTile, pb.sracc = (int64_t)msplit * kTile, pb.sW = (int64_t)n_pad * kTile, pb.sout = (int64_t)nsplit * kTile * d;
    for (int z = 0; z < len; z++) {
        const egx_gp *g = gps[z];
        pb.ptrs.par[z] = dev_xnorm(g), pb.ptrs.spec[z] = dev_spec(g);
        pb.ptrs.xT[z] = g->d_xT, pb.ptrs.coef[z] = g->d_fit_coef, pb.ptrs.gamma[z] = g->d_gamma;
    }
    pm = pb;
    if (prescaled)
        for (int z = 0; z < len; z++) pm.ptrs.xT[z] = dev_xs_fit(gps[z]);
    // (xtypes: cast in the same launch; the expert that writes the flags leaves the cast raw tile for k_infill_mix as well)
    EGX_RC(launch_infill_prepare(st, pb, h->xraw.p + (size_t)t0 * d, mt, d, h->xqT.p, flag,
                                 flag && h->n_eslots > 0 && dev_spec(lead) ? h->xcast.p + (size_t)t0 * d : nullptr));
    // r . gamma in split partial sums (algorithm.rs:260-262), before the solve overwrites r
    EGX_RC(launch_predict_mean(st, lead->corr, pm, h->xqT.p, kTile, kTile, n_pad, n_pad, d, hcols, h->racc.p, msplit, prescaled ? 1 : 0));
    InfillTrend tr[kLockstepMax];
    InfillFinish fin[kLockstepMax];
    for (int z = 0; z < len; z++) {
        const egx_gp *g = gps[z];
        InfillTrend &t = tr[z];
        t.p = p, t.rp = rp, t.msplit = msplit;
        t.xqT = h->xqT.p + (size_t)z * pb.sq, t.fidx = g->d_fidx, t.beta = g->d_tbeta;
        t.racc = h->racc.p + (size_t)z * pb.sracc;
        t.y_mean = g->y_mean, t.y_std = g->y_std;
        t.mean = o[z].mean;
        fin[z].x_std = dev_xnorm(g) + d, fin[z].gmean = o[z].gmean;
        if (want_g) fin[z].out_y = h->out_y.p + (size_t)z * pb.sout;
        if (mean_only) continue;
        t.R = g->d_rq, t.Rt = g->d_rqT;
        t.s0 = h->s0.p + (size_t)z * kTile, t.sl = h->sl.p + (size_t)z * kTile * p;
        t.sigma2 = g->sigma2;
        t.var = o[z].var;
        if (!want_g) continue;
        t.dneg = h->dneg.p + (size_t)z * kTile * rp;
        fin[z].out_v = h->out_v.p + (size_t)z * pb.sout, fin[z].gvar = o[z].gvar;
    }
    if (mean_only) {
        EGX_RC(launch_infill_trend_mean(st, tr, len));
        if (!want_g) return EGX_SUCCESS;
        EGX_RC(launch_xgrad(st, lead->corr, pb, h->xqT.p, kTile, kTile, n_pad, n, d, hcols, nullptr, 0, 1, nsplit, h->out_y.p, cols, ncols));
        return launch_infill_xgrad_finish_mean(st, tr, fin, len, d, nsplit);
    }
    // rt = C^-1 r (held transposed), sum rt^2 and ft^T rt (:337-352)
    EGX_RC(posterior_solve_run(gps, len, st, h->xqT.p, kTile, h->RT.p, h->s0.p, h->sl.p));
    EGX_RC(launch_infill_trend(st, tr, len));
    if (!want_g) return EGX_SUCCESS;
    // -(R^-1 r + R^-1 F D)^T as an (n_pad x 128) weight matrix, then the two contractions
    EGX_RC(posterior_weights_run(gps, len, st, h->RT.p, kTile, h->Wt.p));
    EGX_RC(posterior_weights_trend_run(gps, len, st, h->dneg.p, kTile, h->Wt.p));
    EGX_RC(launch_xgrad(st, lead->corr, pb, h->xqT.p, kTile, kTile, n_pad, n, d, hcols, nullptr, 0, 1, nsplit, h->out_y.p, cols, ncols));
    EGX_RC(launch_xgrad(st, lead->corr, pb, h->xqT.p, kTile, kTile, n_pad, n, d, hcols, h->Wt.p, kTile, 0, nsplit, h->out_v.p, cols, ncols));
    return launch_infill_xgrad_finish(st, tr, fin, len, d, nsplit);
}

// A SPARSE expert's launch sequence for one tile, the batched route of sgp_query (sgp_predict.hip) at the padded batch of 128
// whatever the call's size: raw x, K(x, z) . (sigma2 vec) in split partial sums, K(x, z), the two block solves with their row
// reductions, the finish; with gradients the two transposed products with the cached inverse factors (sgp_ensure_inverse_factors,
// built by ensure_device_state), the two contractions and their finish.  Arguments as run_tile's, for ONE model j.  The MEAN-ONLY branch: no
// K(x, z) block, no solve; the same partial sums in the same order, so the means keep the full sequence's bits.
int sgp_expert_tile(egx_infill *h, hipStream_t st, int j, int64_t t0, int mt, const TileOut &o, int *flag) {
    const int d = h->d;
    egx_sgp *g = h->models[j].sg;
    const int nz = g->nz, z_pad = g->z_pad, vfe = g->method != 0;
    const int msplit = mean_splits(z_pad, kTile), nsplit = xgrad_splits(nz, kTile);
    const size_t blk = (size_t)kTile * z_pad;
    const bool mean_only = !o.var, want_g = o.gmean != nullptr;
    const int *cols = h->use_cols ? h->d_active.p : nullptr;
    const int ncols = h->use_cols ? (int)h->active.size() : 0;
    if (mean_only) flag = nullptr;
    EGX_RC(launch_infill_prepare(st, h->xraw.p + (size_t)t0 * d, mt, d, h->ident.p, h->xqT.p, flag));
    EGX_RC(launch_predict_mean(st, g->corr, h->xqT.p, kTile, kTile, g->zT.p, z_pad, z_pad, d, g->coef.p, g->hcols, g->vec.p, h->racc.p, msplit));
    if (mean_only) {
        EGX_RC(launch_infill_sgp_finish(st, h->racc.p, msplit, nullptr, nullptr, g->sigma2, g->noise, 0, o.mean, nullptr));
        if (!want_g) return EGX_SUCCESS;
        EGX_RC(launch_xgrad(st, g->corr, h->xqT.p, kTile, kTile, g->zT.p, z_pad, nz, d, g->coef.p, g->hcols, g->vec.p, 0, 1, nsplit, h->out_y.p, cols,
                            ncols));
        return launch_infill_sgp_xgrad_finish(st, h->out_y.p, nullptr, nsplit, d, nullptr, nullptr, g->sigma2, 0, 0.0, o.gmean, nullptr);
    }
    EGX_RC(launch_cross_corr(st, g->corr, h->xqT.p, kTile, kTile, g->zT.p, z_pad, z_pad, d, g->coef.p, g->hcols, h->RT.p, z_pad));
    EGX_RC(launch_trsm_rows(st, g->Kz.p, z_pad, z_pad, g->dinv_z.p, h->RT.p, z_pad, kTile));  // a~ = C_z^-1 r
    EGX_RC(launch_row_reduce(st, h->RT.p, z_pad, kTile, nz, nullptr, 0, 0, h->s0.p, nullptr));
    if (want_g) EGX_RC(sgp_launch_scale_copy(st, h->RT.p, vfe ? -1.0 : 1.0, (int64_t)blk, h->sE.p));  // E = -s a~: the GEMMs subtract
    EGX_RC(launch_trsm_rows(st, g->A.p, z_pad, z_pad, g->dinv_a.p, h->RT.p, z_pad, kTile));  // b~ = L^-1 a~
    EGX_RC(launch_row_reduce(st, h->RT.p, z_pad, kTile, nz, nullptr, 0, 0, h->s1.p, nullptr));
    EGX_RC(launch_infill_sgp_finish(st, h->racc.p, msplit, h->s0.p, h->s1.p, g->sigma2, g->noise, vfe, o.mean, o.var));
    if (!want_g) return EGX_SUCCESS;
    // E -= b~ (L^-T)^T, then Ct = 0 - C_z^-T E^T = s c transposed (z_pad x 128): the weight layout of launch_xgrad
    EGX_RC(launch_gemm_nt_sub(st, h->sE.p, z_pad, h->RT.p, z_pad, g->Wa.p, z_pad, kTile, z_pad, z_pad, 0, 0));
    EGX_HIP_CHECK(hipMemsetAsync(h->Wt.p, 0, sizeof(double) * blk, st));
    EGX_RC(launch_gemm_nt_sub(st, h->Wt.p, kTile, g->Wz.p, z_pad, h->sE.p, z_pad, z_pad, kTile, z_pad, 0, 1));
    EGX_RC(launch_xgrad(st, g->corr, h->xqT.p, kTile, kTile, g->zT.p, z_pad, nz, d, g->coef.p, g->hcols, g->vec.p, 0, 1, nsplit, h->out_y.p, cols,
                        ncols));
    EGX_RC(launch_xgrad(st, g->corr, h->xqT.p, kTile, kTile, g->zT.p, z_pad, nz, d, g->coef.p, g->hcols, h->Wt.p, kTile, 0, nsplit,
                        h->out_v.p, cols, ncols));
    return launch_infill_sgp_xgrad_finish(st, h->out_y.p, h->out_v.p, nsplit, d, h->s0.p, h->s1.p, g->sigma2, vfe,
                                          (vfe ? -2.0 : 2.0) * g->sigma2, o.gmean, o.gvar);
}

// ---- the evaluation, stage by stage (eval_locked) ----

// What a call runs, decided once.  m points, padded to M in whole tiles; want_g: somebody reads a gradient; folded:
// EGX_CSTR_INFILL, the constraint surrogates are inside the objective (all of them, the full sequence); run_c: they run at all --
// folded, or something of theirs is asked for; mean_c: and then mean-only, since no variance of theirs is read; pending: (q = 0
// and no push: nothing differs from a handle without pending points); typed: the models carry xtypes; diag_mix:
// egx_infill_eval_experts on a mixture, dsg its surrogate
struct EvalPlan {
    int64_t m = 0, M = 0;
    bool want_g = false, folded = false, run_c = false, mean_c = false, pending = false, typed = false, any_sparse = false, diag_mix = false;
    const Surrogate *dsg = nullptr;
};

EvalPlan make_plan(const egx_infill *h, int64_t m, const double *grad, const egx_infill_parts *parts, const ExpertDiag *diag,
                   const CstrOut *co, const PushCapture *cap) {
    EvalPlan p;
    p.m = m, p.M = round_up(m, kTile);
    p.pending = h->q > 0 || cap;
    p.want_g = grad || (parts && (parts->grad_mean || parts->grad_var)) || (diag && (diag->gmean || diag->gvar || diag->dprobas)) ||
               (co && co->gcstr);
    p.folded = h->strategy == infill::kCstrInfill;
    p.run_c = p.folded || parts || diag || (co && (co->cstr || co->gcstr));
    p.mean_c = h->strategy == infill::kCstrMean && !diag && !(parts && (parts->var || parts->grad_var));
    for (const ModelRef &r : h->models) p.any_sparse |= r.sparse();
    p.typed = !h->models[0].sparse() && !h->models[0].gp->xspec.empty();
    p.dsg = diag ? &h->surr[diag->j] : nullptr;
    p.diag_mix = p.dsg && p.dsg->k >= 2;
    return p;
}

// the surrogates as infill_runs.h reads them, and the runs of a walk over them (mean_c: the constraints' sequence is mean-only)
std::vector<runs::Shape> run_shapes(const egx_infill *h) {
    std::vector<runs::Shape> out(h->surr.size());
    for (size_t js = 0; js < h->surr.size(); js++) {
        const Surrogate &sg = h->surr[js];
        const ModelRef &r = h->models[sg.first];
        runs::Shape &s = out[js];
        s.lone_dense = sg.k < 2 && !r.sparse();
        if (!s.lone_dense) continue;
        const egx_gp *g = r.gp;
        s.n = g->n, s.n_pad = g->n_pad, s.corr = g->corr, s.mean = g->mean, s.fit_hcols = g->fit_hcols, s.has_w = g->has_w;
        s.group = g->group.get(), s.slot = g->group_slot;
    }
    return out;
}
// pending: the walk conditions on pending points or captures a push (EvalPlan::pending) -- every run has length 1
std::vector<int> walk_runs(const egx_infill *h, bool mean_c, bool pending) {
    const std::vector<runs::Shape> sh = run_shapes(h);
    return runs::run_lengths(sh.data(), (int)sh.size(), mean_c, pending ? std::max(h->q, 1) : 0);
}

// a host array the handle uploads on first use (and again after it changed: the owner clears on_device)
int upload_once(DevBuf &buf, bool &on_device, const double *src, size_t count, hipStream_t st) {
    if (on_device) return EGX_SUCCESS;
    EGX_RC(buf.alloc(count));
    EGX_HIP_CHECK(hipMemcpyAsync(buf.p, src, sizeof(double) * count, hipMemcpyHostToDevice, st));
    on_device = true;
    return EGX_SUCCESS;
}

// what the tile sequences read beside the models' fitted state: inverse factors, trend state, the handle's small arrays
int ensure_device_state(egx_infill *h, hipStream_t st, const EvalPlan &p) {
    const int ne = (int)h->models.size(), k = (int)h->surr.size() - 1, d = h->d;
    if (p.want_g)  // once per fitted state (synchronises the model's stream); the mean-only sequence does not read C^-T
        for (int e = 0; e < (p.run_c && !p.mean_c ? ne : h->surr[0].k); e++) {
            const ModelRef &r = h->models[e];
            if (!r.sparse()) {
                EGX_RC(ensure_winv(r.gp));
            } else if (!r.sg->winv_ok) {  // built on the model's own stream: wait before the call's stream reads them
                EGX_RC(sgp_ensure_inverse_factors(r.sg));
                EGX_HIP_CHECK(hipStreamSynchronize(r.sg->stream));
            }
        }
    for (int e = 0; e < ne; e++)
        if (!h->models[e].sparse()) EGX_RC(ensure_trend_state(h->models[e].gp, st));
    if (p.any_sparse && !h->ident_on_device) {
        std::vector<double> id((size_t)2 * d, 0.0);
        std::fill(id.begin() + d, id.end(), 1.0);
        bool sent = false;
        EGX_RC(upload_once(h->ident, sent, id.data(), id.size(), st));
        EGX_HIP_CHECK(hipStreamSynchronize(st));  // id is a local
        h->ident_on_device = true;
    }
    for (Surrogate &sg : h->surr)
        if (sg.k >= 2) EGX_RC(upload_once(sg.d_gmx, sg.on_device, sg.gmx.data(), sg.gmx.size(), st));
    if (k > 0 && !p.folded) EGX_RC(upload_once(h->d_scale, h->scale_on_device, h->scale_cstr.data(), (size_t)k, st));
    if (k > 0) EGX_RC(upload_once(h->d_tol, h->tol_on_device, h->tol.data(), (size_t)k, st));
    if (h->use_cols && p.want_g && !h->active_on_device) {  // (h->active stays as it is until the next egx_infill_set_active)
        EGX_RC(h->d_active.alloc(h->active.size()));
        EGX_HIP_CHECK(hipMemcpyAsync(h->d_active.p, h->active.data(), sizeof(int) * h->active.size(), hipMemcpyHostToDevice, st));
        h->active_on_device = true;
    }
    return EGX_SUCCESS;
}

// the call's tables and the scratch of one (tile, run) step, sized by the largest model and the longest run
int reserve_scratch(egx_infill *h, const EvalPlan &p, const ExpertDiag *diag, const CstrOut *co, const PushCapture *cap) {
    const int nm = (int)h->surr.size(), k = nm - 1, d = h->d, ns = h->n_eslots;
    size_t rl = 1;  // members of the longest run: the tile buffers hold one block per member
    for (int len : walk_runs(h, p.mean_c, p.pending)) rl = std::max(rl, (size_t)len);
    const int64_t m = p.m, M = p.M;
    int n_pad_max = 0, p_max = 1, rp_max = 1, ms_max = 0, ns_max = 0, z_pad_max = 0;
    for (const ModelRef &r : h->models) {  // (the inducing points of a sparse model stand where a dense model's training points do)
        const int rows = r.sparse() ? r.sg->nz : r.gp->n, rows_pad = r.sparse() ? r.sg->z_pad : r.gp->n_pad;
        n_pad_max = std::max(n_pad_max, rows_pad);
        ms_max = std::max(ms_max, mean_splits(rows_pad, kTile));
        ns_max = std::max(ns_max, xgrad_splits(rows, kTile));
        if (r.sparse()) z_pad_max = std::max(z_pad_max, rows_pad);
        else p_max = std::max(p_max, r.gp->p), rp_max = std::max(rp_max, r.gp->rhs_pad);
    }
    EGX_RC(h->xraw.alloc((size_t)m * d));
    if (p.typed && ns > 0) EGX_RC(h->xcast.alloc((size_t)m * d));
    EGX_RC(h->flag.alloc((size_t)(M + 1) / 2));
    EGX_RC(h->mean.alloc((size_t)nm * M));
    EGX_RC(h->var.alloc((size_t)nm * M));
    EGX_RC(h->value.alloc((size_t)M));
    EGX_RC(h->xqT.alloc(rl * d * kTile));
    EGX_RC(h->racc.alloc(rl * ms_max * kTile));
    EGX_RC(h->RT.alloc(rl * kTile * n_pad_max));
    EGX_RC(h->s0.alloc(rl * kTile));
    EGX_RC(h->sl.alloc(rl * kTile * p_max));
    if (p.any_sparse) EGX_RC(h->s1.alloc(kTile));
    if (p.want_g) {
        if (p.any_sparse) EGX_RC(h->sE.alloc((size_t)kTile * z_pad_max));
        EGX_RC(h->gmean.alloc((size_t)nm * M * d));
        EGX_RC(h->gvar.alloc((size_t)nm * M * d));
        EGX_RC(h->grad.alloc((size_t)M * d));
        EGX_RC(h->Wt.alloc(rl * n_pad_max * kTile));
        EGX_RC(h->dneg.alloc(rl * kTile * rp_max));
        EGX_RC(h->out_y.alloc(rl * ns_max * kTile * d));
        EGX_RC(h->out_v.alloc(rl * ns_max * kTile * d));
    }
    if (ns > 0) {
        EGX_RC(h->emean.alloc((size_t)ns * M));
        EGX_RC(h->evar.alloc((size_t)ns * M));
        if (p.want_g) {
            EGX_RC(h->egmean.alloc((size_t)ns * M * d));
            EGX_RC(h->egvar.alloc((size_t)ns * M * d));
            EGX_RC(h->dprob.alloc((size_t)kTile * h->k_max * d));
        }
    }
    if (co && k > 0) {
        if (co->cstr) EGX_RC(h->cstr.alloc((size_t)M * k));
        if (co->gcstr) EGX_RC(h->gcstr.alloc((size_t)M * k * d));
    }
    if (p.pending && h->q > 0) {
        int ns_p = 1;  // the larger of the fused form's splits and the composed form's (per column: mean_splits, xgrad_splits)
        for (int js = 0; js < nm; js++) {
            const int nz = h->models[h->surr[js].first].gp->n + h->q;
            ns_p = std::max(ns_p, std::max(pending_splits(nz), std::max(mean_splits((int)h->pend[js].ldz, kTile), xgrad_splits(nz, kTile))));
        }
        EGX_RC(h->pc_c.alloc((size_t)ns_p * kTile * pending::kLd));
        if (p.want_g && !cap) EGX_RC(h->pc_g.alloc((size_t)ns_p * kTile * pending::kLd * d));
    }
    if (p.diag_mix) {
        EGX_RC(h->dg_probas.alloc((size_t)M * p.dsg->k));
        if (diag->dprobas) EGX_RC(h->dg_dprobas.alloc((size_t)M * p.dsg->k * d));
    }
    return EGX_SUCCESS;
}

// Where expert e of surrogate js writes the tile at t0: a lone expert the surrogate's slot of the tables, the experts of a mixture
// their slots of the expert tables.  The mean-only sequence gets no variance tables.
TileOut tile_out(const egx_infill *h, const EvalPlan &p, int js, int e, int64_t t0, bool mean_only) {
    const Surrogate &sg = h->surr[js];
    const bool lone = sg.k < 2;
    const size_t row = (lone ? (size_t)js : (size_t)(sg.eslot + e)) * p.M + t0, d = (size_t)h->d;
    TileOut o;
    o.mean = (lone ? h->mean.p : h->emean.p) + row;
    if (!mean_only) o.var = (lone ? h->var.p : h->evar.p) + row;
    if (p.want_g) o.gmean = (lone ? h->gmean.p : h->egmean.p) + row * d;
    if (p.want_g && !mean_only) o.gvar = (lone ? h->gvar.p : h->egvar.p) + row * d;
    return o;
}

// one (tile, surrogate) recombination of a mixture's expert tables into the surrogate's slot
int mix_tile(egx_infill *h, hipStream_t st, const EvalPlan &p, int js, int64_t t0, int mt, bool mean_only, const ExpertDiag *diag) {
    const Surrogate &sg = h->surr[js];
    const int d = h->d;
    const int64_t M = p.M;
    int *flag = reinterpret_cast<int *>(h->flag.p);
    InfillMix mx;
    mx.mt = mt, mx.d = d, mx.k = sg.k, mx.smooth = sg.smooth, mx.want_g = p.want_g;
    mx.xq = (p.typed ? h->xcast.p : h->xraw.p) + (size_t)t0 * d, mx.flag = flag + t0;
    mx.means = sg.d_gmx.p, mx.precs = sg.d_gmx.p + (size_t)sg.k * d, mx.par = mx.precs + (size_t)sg.k * d * d;
    mx.emean = h->emean.p + (size_t)sg.eslot * M + t0, mx.evar = h->evar.p + (size_t)sg.eslot * M + t0;
    mx.estride = M;
    mx.mean = h->mean.p + (size_t)js * M + t0, mx.var = h->var.p + (size_t)js * M + t0;
    if (p.want_g) {
        mx.egmean = h->egmean.p + ((size_t)sg.eslot * M + t0) * d, mx.egvar = h->egvar.p + ((size_t)sg.eslot * M + t0) * d;
        mx.gmean = h->gmean.p + ((size_t)js * M + t0) * d, mx.gvar = h->gvar.p + ((size_t)js * M + t0) * d;
        if (sg.smooth) mx.dp = h->dprob.p;
    }
    if (p.diag_mix && p.dsg == &sg) {
        mx.probas = h->dg_probas.p + (size_t)t0 * sg.k;
        if (diag->dprobas) mx.dp = h->dg_dprobas.p + (size_t)t0 * sg.k * d;
    }
    return mean_only ? launch_infill_mix_mean(st, mx) : launch_infill_mix(st, mx);
}

// tile -> run -> (a mixture, a sparse model: expert): the run's sequence, the conditioning on the pending points, the mixture's
// recombination.  A lone dense surrogate that forms no run, and a dense expert of a mixture, is a run of one through the same code.
int walk_tiles(egx_infill *h, hipStream_t st, const EvalPlan &p, const ExpertDiag *diag, PushCapture *cap) {
    const int nm = p.run_c ? (int)h->surr.size() : 1;
    const std::vector<int> lens = walk_runs(h, p.mean_c, p.pending);
    int *flag = reinterpret_cast<int *>(h->flag.p);
    for (int64_t t0 = 0; t0 < p.m; t0 += kTile) {
        const int mt = (int)std::min<int64_t>(kTile, p.m - t0);
        size_t r = 0;
        for (int js = 0; js < nm; js += lens[r++]) {
            const Surrogate &sg = h->surr[js];
            const bool mean_only = js > 0 && p.mean_c;  // (the objective always runs the full sequence)
            if (sg.k < 2 && !h->models[sg.first].sparse()) {
                const int len = std::min(lens[r], nm - js);  // (a call that runs the objective alone)
                int jm[kLockstepMax];
                TileOut o[kLockstepMax];
                for (int z = 0; z < len; z++) jm[z] = h->surr[js + z].first, o[z] = tile_out(h, p, js + z, 0, t0, mean_only);
                EGX_RC(run_tile(h, st, jm, len, t0, mt, o, jm[0] == 0 ? flag + t0 : nullptr));
                if (p.pending) EGX_RC(pending_tile(h, st, js, o[0], cap));  // (pending points: every run has length 1)
                continue;
            }
            for (int e = 0; e < sg.k; e++) {
                const int j = sg.first + e;
                const TileOut o = tile_out(h, p, js, e, t0, mean_only);
                if (h->models[j].sparse()) EGX_RC(sgp_expert_tile(h, st, j, t0, mt, o, j == 0 ? flag + t0 : nullptr));
                else EGX_RC(run_tile(h, st, &j, 1, t0, mt, &o, j == 0 ? flag + t0 : nullptr));
                if (p.pending) EGX_RC(pending_tile(h, st, js, o, cap));  // (lone dense surrogates only: o is the surrogate's slot)
            }
            if (sg.k >= 2) EGX_RC(mix_tile(h, st, p, js, t0, mt, mean_only, diag));
        }
    }
    return EGX_SUCCESS;
}

// m points of slot `slot` of a device table (M points per slot, `per` doubles per point) into block `blk` of a host array
int slot_back(hipStream_t st, double *dst, size_t blk, const double *tab, size_t slot, const EvalPlan &p, size_t per) {
    if (!dst) return EGX_SUCCESS;
    EGX_HIP_CHECK(hipMemcpyAsync(dst + blk * p.m * per, tab + slot * p.M * per, sizeof(double) * (size_t)p.m * per, hipMemcpyDeviceToHost, st));
    return EGX_SUCCESS;
}

// the criterion across the models of a point, then everything the caller asked for back to the host; ONE synchronisation
int combine_and_copy_back(egx_infill *h, hipStream_t st, const EvalPlan &p, double *value, double *grad, const egx_infill_parts *parts,
                          const ExpertDiag *diag, const CstrOut *co) {
    const int nm = (int)h->surr.size(), k = nm - 1, d = h->d;
    const int64_t m = p.m, M = p.M;
    const int *flag = reinterpret_cast<const int *>(h->flag.p);
    const double *gmean = p.want_g ? h->gmean.p : nullptr, *gvar = p.want_g ? h->gvar.p : nullptr;
    if (value && p.folded)
        EGX_RC(launch_infill_combine(st, h->prm, k, d, m, M, h->mean.p, h->var.p, gmean, gvar, h->d_tol.p, flag, h->value.p,
                                     grad ? h->grad.p : nullptr));
    if (value && !p.folded) {  // the objective model alone; the constraint values beside it for egx_infill_eval_cstr
        const int kc = co ? k : 0;
        EGX_RC(launch_infill_cstr(st, h->prm, h->strategy, kc, d, m, M, h->mean.p, h->var.p, gmean, gvar, h->d_scale.p, flag, h->value.p,
                                  kc && co->cstr ? h->cstr.p : nullptr, grad ? h->grad.p : nullptr,
                                  kc && co->gcstr ? h->gcstr.p : nullptr));
        if (kc) EGX_RC(slot_back(st, co->cstr, 0, h->cstr.p, 0, p, (size_t)k));
        if (kc) EGX_RC(slot_back(st, co->gcstr, 0, h->gcstr.p, 0, p, (size_t)k * d));
    }
    if (value) EGX_HIP_CHECK(hipMemcpyAsync(value, h->value.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, st));
    if (grad) EGX_HIP_CHECK(hipMemcpyAsync(grad, h->grad.p, sizeof(double) * (size_t)m * d, hipMemcpyDeviceToHost, st));
    if (parts)
        for (int j = 0; j < nm; j++) {
            EGX_RC(slot_back(st, parts->mean, j, h->mean.p, j, p, 1));
            EGX_RC(slot_back(st, parts->var, j, h->var.p, j, p, 1));
            EGX_RC(slot_back(st, parts->grad_mean, j, h->gmean.p, j, p, (size_t)d));
            EGX_RC(slot_back(st, parts->grad_var, j, h->gvar.p, j, p, (size_t)d));
        }
    if (diag) {  // expert c of the surrogate: its slot of the expert tables, or (a lone expert) the surrogate's own slot
        const Surrogate *dsg = p.dsg;
        auto back = [&](double *dst, const double *tab_e, const double *tab_s, size_t per) -> int {
            for (int c = 0; c < dsg->k; c++)
                EGX_RC(slot_back(st, dst, c, p.diag_mix ? tab_e : tab_s, p.diag_mix ? (size_t)(dsg->eslot + c) : (size_t)diag->j, p, per));
            return EGX_SUCCESS;
        };
        EGX_RC(back(diag->mean, h->emean.p, h->mean.p, 1));
        EGX_RC(back(diag->var, h->evar.p, h->var.p, 1));
        EGX_RC(back(diag->gmean, h->egmean.p, h->gmean.p, (size_t)d));
        EGX_RC(back(diag->gvar, h->egvar.p, h->gvar.p, (size_t)d));
        if (p.diag_mix && diag->probas)
            EGX_HIP_CHECK(hipMemcpyAsync(diag->probas, h->dg_probas.p, sizeof(double) * (size_t)m * dsg->k, hipMemcpyDeviceToHost, st));
        if (p.diag_mix && diag->dprobas)
            EGX_HIP_CHECK(hipMemcpyAsync(diag->dprobas, h->dg_dprobas.p, sizeof(double) * (size_t)m * dsg->k * d,
                                         hipMemcpyDeviceToHost, st));
    }
    EGX_HIP_CHECK(hipStreamSynchronize(st));
    if (diag && !p.diag_mix) {  // one cluster: the responsibilities are ones (gaussian_mixture.rs:115-116)
        if (diag->probas) std::fill(diag->probas, diag->probas + m, 1.0);
        if (diag->dprobas) std::fill(diag->dprobas, diag->dprobas + (size_t)m * d, 0.0);
    }
    return EGX_SUCCESS;
}

// The evaluation proper; the handle's and the models' locks are held.  value / grad / every member of parts may be nullptr.
int eval_locked(egx_infill *h, const double *xq, int64_t m, double *value, double *grad, const egx_infill_parts *parts,
                const ExpertDiag *diag, const CstrOut *co, PushCapture *cap) {
    if (m < 0 || (m > 0 && !xq)) return fail(EGX_ERR_INVALID_VALUE, "bad query array");
    EGX_RC(check_fitted(h));
    EGX_RC(check_specs(h));
    EGX_RC(check_pending(h));
    if (m == 0) return EGX_SUCCESS;
    const EvalPlan p = make_plan(h, m, grad, parts, diag, co, cap);
    EGX_HIP_CHECK(hipSetDevice(h->device));
    hipStream_t st = h->models[0].stream();
    EGX_RC(ensure_device_state(h, st, p));
    EGX_RC(reserve_scratch(h, p, diag, co, cap));
    EGX_HIP_CHECK(hipMemcpyAsync(h->xraw.p, xq, sizeof(double) * (size_t)m * h->d, hipMemcpyHostToDevice, st));
    EGX_RC(walk_tiles(h, st, p, diag, cap));
    return combine_and_copy_back(h, st, p, value, grad, parts, diag, co);
}

bool params_ok(double fmin, double sigma_weight, double scale_ic, double scale) {
    if (std::isnan(fmin) || !(sigma_weight > 0.0) || std::isnan(scale_ic) || !(scale > 0.0) || std::isinf(scale)) {
        set_error("infill: fmin and scale_ic must not be NaN, sigma_weight and scale must be positive and finite");
        return false;
    }
    return true;
}

int config_ok(const egx_infill_config &cfg) {
    if (cfg.criterion < EGX_INFILL_EI || cfg.criterion > EGX_INFILL_WB2S) return fail(EGX_ERR_INVALID_VALUE, "infill: unknown criterion");
    return params_ok(cfg.fmin, cfg.sigma_weight, cfg.scale_ic, cfg.scale) ? EGX_SUCCESS : EGX_ERR_INVALID_VALUE;
}

// the checks over all experts, the criterion's parameters
int finish_create(egx_infill *h, const egx_infill_config &cfg) {
    EGX_RC(check_shapes(h));
    EGX_RC(check_fitted(h));
    EGX_RC(check_specs(h));
    h->prm.kind = cfg.criterion;
    h->prm.fmin = cfg.fmin;
    h->prm.sigma_weight = cfg.sigma_weight;
    h->prm.scale_ic = cfg.scale_ic;
    h->prm.scale = cfg.scale;
    h->prm.feasibility = cfg.feasibility != 0;
    h->scale_cstr.assign(h->surr.size() - 1, 1.0);
    return EGX_SUCCESS;
}

// expert e of a surrogate as a ModelRef: egx_infill_create_mix's dense handles, egx_infill_create_any's tagged references
int expert_ref(const egx_infill_surrogate &sv, int e, const std::string &name, ModelRef &out) {
    if (!sv.experts[e]) return fail(EGX_ERR_INVALID_VALUE, name + " expert " + std::to_string(e) + " is NULL");
    out = ModelRef(sv.experts[e]);
    return EGX_SUCCESS;
}
int expert_ref(const egx_infill_surrogate_any &sv, int e, const std::string &name, ModelRef &out) {
    const egx_model_ref &r = sv.experts[e];
    if (r.kind != EGX_MODEL_GP && r.kind != EGX_MODEL_SGP)
        return fail(EGX_ERR_INVALID_VALUE, name + " expert " + std::to_string(e) + " has the unknown kind " + std::to_string(r.kind) +
            " (EGX_MODEL_GP or EGX_MODEL_SGP)");
    if (!r.handle) return fail(EGX_ERR_INVALID_VALUE, name + " expert " + std::to_string(e) + " is NULL");
    out = r.kind == EGX_MODEL_SGP ? ModelRef(static_cast<egx_sgp *>(r.handle)) : ModelRef(static_cast<egx_gp *>(r.handle));
    return EGX_SUCCESS;
}

// the Gaussian mixture of a surrogate with k >= 2 experts: checked, packed as the kernels read it, its slots of the expert tables
template <class SurrogateView>
int add_mixture(egx_infill *h, Surrogate &sg, const SurrogateView &sv, const std::string &name) {
    if (!sv.weights || !sv.means || !sv.precisions_chol) return fail(EGX_ERR_INVALID_VALUE, name + ": NULL weights, means or precisions_chol");
    if (!(sv.heaviside_factor > 0.0) || std::isinf(sv.heaviside_factor))
        return fail(EGX_ERR_INVALID_VALUE, name + ": heaviside_factor must be positive and finite");
    const int64_t kk = sg.k, d = h->models[sg.first].d();  // (the first read of a model: the pointer checks are done)
    bool finite = true, positive = true;
    for (int64_t i = 0; i < kk; i++) finite &= std::isfinite(sv.weights[i]), positive &= sv.weights[i] > 0.0;
    for (int64_t i = 0; i < kk * d; i++) finite &= std::isfinite(sv.means[i]);
    for (int64_t i = 0; i < kk * d * d; i++) finite &= std::isfinite(sv.precisions_chol[i]);
    if (!finite) return fail(EGX_ERR_INVALID_VALUE, name + ": non-finite weight, mean or precision factor");
    if (!positive) return fail(EGX_ERR_INVALID_VALUE, name + ": weights must be positive");
    if (infill_mix_lds_bytes((int)d, (int)kk) > kInfillMixMaxLds)
        return fail(EGX_ERR_UNSUPPORTED, name + ": 3 (d | 1) + 2 (k | 1) exceeds 320 doubles of LDS scratch per point (d " + std::to_string(d) +
            ", k " + std::to_string(kk) + ")");
    sg.gmx = gmx_pack(sv.weights, sv.means, sv.precisions_chol, kk, d, sv.heaviside_factor);
    for (int64_t c = 0; c < kk; c++)
        if (!std::isfinite(sg.gmx[(size_t)(kk * d + kk * d * d + c)]))
            return fail(EGX_ERR_INVALID_VALUE, name + ": cluster " + std::to_string(c) + " has no positive diagonal in its precision factor");
    sg.eslot = h->n_eslots;
    h->n_eslots += sg.k;
    h->k_max = std::max(h->k_max, sg.k);
    return EGX_SUCCESS;
}

// egx_infill_create_mix and egx_infill_create_any: the same checks in the same order, the same handle
template <class SurrogateView>
int32_t create_from_surrogates(const egx_infill_config *cfg_in, const SurrogateView *surrogates, const double *cstr_tols,
                               int32_t n_cstr, egx_infill **out) {
    if (!out) return fail(EGX_ERR_INVALID_VALUE, "out handle pointer is NULL");
    *out = nullptr;
    egx_infill_config cfg;
    if (cfg_in) cfg = *cfg_in; else egx_infill_config_default(&cfg);
    if (!surrogates || n_cstr < 0 || (n_cstr > 0 && !cstr_tols)) return fail(EGX_ERR_INVALID_VALUE, "infill: NULL surrogate or tolerance array");
    EGX_RC(config_ok(cfg));
    std::unique_ptr<egx_infill> h(new egx_infill);
    h->mix_api = true;
    for (int j = 0; j <= n_cstr; j++) {
        const SurrogateView &sv = surrogates[j];
        const std::string name = "infill: surrogate " + std::to_string(j);
        if (sv.n_experts < 1 || !sv.experts) return fail(EGX_ERR_INVALID_VALUE, name + " needs at least one expert");
        if (j > 0 && std::isnan(cstr_tols[j - 1])) return fail(EGX_ERR_INVALID_VALUE, "infill: tolerance " + std::to_string(j - 1) + " is NaN");
        h->surr.emplace_back();
        Surrogate &sg = h->surr.back();
        sg.first = (int)h->models.size(), sg.k = sv.n_experts, sg.smooth = sv.smooth != 0;
        for (int e = 0; e < sv.n_experts; e++) {
            ModelRef ref;
            EGX_RC(expert_ref(sv, e, name, ref));
            h->models.push_back(ref);
        }
        if (j > 0) h->tol.push_back(cstr_tols[j - 1]);
        // (one cluster: the responsibilities are ones, the mixture is not read)
        if (sg.k >= 2) EGX_RC(add_mixture(h.get(), sg, sv, name));
    }
    EGX_RC(finish_create(h.get(), cfg));
    *out = h.release();
    return EGX_SUCCESS;
}

// The criterion's terms of the scaling pass, formed on the device from the tables of the pass and copied to the host: ei, or base
// and fac (npts each; h->value holds [0, M): ei or base, [M, 2 M): fac); `what` names them in the error text
int scale_terms(egx_infill *h, hipStream_t st, const infill::Params &prm, int k, int64_t npts, double *ei, double *base, double *fac,
                const char *what) {
    const int64_t M = round_up(npts, kTile);
    double *v = h->value.p;
    const int rc = launch_infill_scale_terms(st, prm, k, npts, M, h->mean.p, h->var.p, h->d_tol.p, reinterpret_cast<const int *>(h->flag.p),
                                             ei ? v : nullptr, base ? v : nullptr, fac ? v + M : nullptr);
    if (rc) return settle_failed(h, rc);
    auto back = [&](double *dst, const double *src) {
        return !dst || hipMemcpyAsync(dst, src, sizeof(double) * (size_t)npts, hipMemcpyDeviceToHost, st) == hipSuccess;
    };
    if (!back(ei, v) || !back(base, v) || !back(fac, v + M) || hipStreamSynchronize(st) != hipSuccess) {
        set_error(std::string("infill scaling: copying ") + what + " back failed");
        return settle_failed(h, EGX_ERR_HIP);
    }
    return EGX_SUCCESS;
}

// compute_cstr_scales, utils/misc.rs:10-28: the largest finite |mean| of every constraint surrogate over the points
void cstr_scales(egx_infill *h, const double *mean, int64_t npts, bool folded, double *scale_cstr) {
    for (size_t j = 1; j < h->surr.size(); j++) {
        double best = -1.0;
        for (int64_t i = 0; i < npts; i++) {
            const double v = mean[j * npts + i];
            if (!std::isinf(v) && std::fabs(v) > best) best = std::fabs(v);
        }
        const double sc = best < 0.0 ? 1.0 : best;
        if (scale_cstr) scale_cstr[j - 1] = sc;
        // kept for egx_infill_eval_cstr (a scale the handle could not divide by -- 0, NaN -- leaves the stored one)
        if (!folded && sc > 0.0 && std::isfinite(sc)) {
            h->scale_cstr[j - 1] = sc;
            h->scale_on_device = false;
        }
    }
}

}  // namespace

namespace egx {

int eval_guarded(egx_infill *h, const double *xq, int64_t m, double *value, double *grad, const egx_infill_parts *parts,
                 const ExpertDiag *diag, const CstrOut *co, PushCapture *cap) {
    const int rc = eval_locked(h, xq, m, value, grad, parts, diag, co, cap);
    return rc ? settle_failed(h, rc) : rc;  // nothing may still run on the handle's buffers
}

int eval_active(egx_infill *h, const double *xq, int64_t m, double *value, double *grad, const egx_infill_parts *parts,
                const CstrOut *co) {
    if (h->active.empty() || m <= 0 || !xq) return eval_guarded(h, xq, m, value, grad, parts, nullptr, co);
    const int d = h->d;
    const size_t mm = (size_t)m, nm = h->surr.size(), k = nm - 1;
    h->act_x.resize(mm * d);
    active::expand(xq, m, h->active, h->x_base, h->act_x.data());
    // full-width stand-ins for what is width() wide in the caller's arrays
    egx_infill_parts full{};
    CstrOut cfull;
    if (grad) h->act_g.resize(mm * d);
    if (parts) {
        full = *parts;
        if (parts->grad_mean) h->act_gm.resize(nm * mm * d), full.grad_mean = h->act_gm.data();
        if (parts->grad_var) h->act_gv.resize(nm * mm * d), full.grad_var = h->act_gv.data();
    }
    if (co) {
        cfull = *co;
        if (co->gcstr) h->act_gc.resize(mm * k * d + 1), cfull.gcstr = h->act_gc.data();
    }
    h->use_cols = true;
    const int rc = eval_guarded(h, h->act_x.data(), m, value, grad ? h->act_g.data() : nullptr, parts ? &full : nullptr, nullptr,
                                co ? &cfull : nullptr);
    h->use_cols = false;
    EGX_RC(rc);
    if (grad) active::gather(h->act_g.data(), m, d, h->active, grad);
    if (parts && parts->grad_mean) active::gather(h->act_gm.data(), (int64_t)(nm * mm), d, h->active, parts->grad_mean);
    if (parts && parts->grad_var) active::gather(h->act_gv.data(), (int64_t)(nm * mm), d, h->active, parts->grad_var);
    if (co && co->gcstr) active::gather(h->act_gc.data(), (int64_t)(mm * k), d, h->active, co->gcstr);
    return EGX_SUCCESS;
}

}  // namespace egx

extern "C" {

void egx_infill_config_default(egx_infill_config *cfg) {
    if (!cfg) return;
    cfg->criterion = EGX_INFILL_LOG_EI;
    cfg->feasibility = 1;
    cfg->fmin = 0.0;
    cfg->sigma_weight = 1.0;
    cfg->scale_ic = 1.0;
    cfg->scale = 1.0;
}

int32_t egx_infill_create(const egx_infill_config *cfg_in, egx_gp *obj_model, egx_gp *const *cstr_models, const double *cstr_tols,
                          int32_t n_cstr, egx_infill **out) {
    if (!out) return fail(EGX_ERR_INVALID_VALUE, "out handle pointer is NULL");
    *out = nullptr;
    egx_infill_config cfg;
    if (cfg_in) cfg = *cfg_in; else egx_infill_config_default(&cfg);
    if (!obj_model || n_cstr < 0 || (n_cstr > 0 && (!cstr_models || !cstr_tols)))
        return fail(EGX_ERR_INVALID_VALUE, "infill: NULL model or tolerance array");
    EGX_RC(config_ok(cfg));
    std::unique_ptr<egx_infill> h(new egx_infill);
    h->models.emplace_back(obj_model);
    for (int j = 0; j < n_cstr; j++) {
        if (!cstr_models[j]) return fail(EGX_ERR_INVALID_VALUE, "infill: model " + std::to_string(j + 1) + " is NULL");
        if (std::isnan(cstr_tols[j])) return fail(EGX_ERR_INVALID_VALUE, "infill: tolerance " + std::to_string(j) + " is NaN");
        h->models.emplace_back(cstr_models[j]);
        h->tol.push_back(cstr_tols[j]);
    }
    for (size_t j = 0; j < h->models.size(); j++) {  // every surrogate a lone expert
        h->surr.emplace_back();
        h->surr.back().first = (int)j;
    }
    EGX_RC(finish_create(h.get(), cfg));
    *out = h.release();
    return EGX_SUCCESS;
}

int32_t egx_infill_create_mix(const egx_infill_config *cfg, const egx_infill_surrogate *surrogates, const double *cstr_tols,
                              int32_t n_cstr, egx_infill **out) {
    return create_from_surrogates(cfg, surrogates, cstr_tols, n_cstr, out);
}

int32_t egx_infill_create_any(const egx_infill_config *cfg, const egx_infill_surrogate_any *surrogates, const double *cstr_tols,
                              int32_t n_cstr, egx_infill **out) {
    return create_from_surrogates(cfg, surrogates, cstr_tols, n_cstr, out);
}

void egx_infill_destroy(egx_infill *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

int32_t egx_infill_set_params(egx_infill *h, double fmin, double sigma_weight, double scale_ic, double scale, int32_t feasibility) {
    if (!h) return fail(EGX_ERR_INVALID_VALUE, "NULL handle");
    if (!params_ok(fmin, sigma_weight, scale_ic, scale)) return EGX_ERR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(h->mu);
    h->prm.fmin = fmin;
    h->prm.sigma_weight = sigma_weight;
    h->prm.scale_ic = scale_ic;
    h->prm.scale = scale;
    h->prm.feasibility = feasibility != 0;
    return EGX_SUCCESS;
}

int32_t egx_infill_get_params(egx_infill *h, egx_infill_config *cfg) {
    if (!h || !cfg) return fail(EGX_ERR_INVALID_VALUE, "NULL argument");
    std::lock_guard<std::mutex> lock(h->mu);
    cfg->criterion = h->prm.kind;
    cfg->feasibility = h->prm.feasibility;
    cfg->fmin = h->prm.fmin;
    cfg->sigma_weight = h->prm.sigma_weight;
    cfg->scale_ic = h->prm.scale_ic;
    cfg->scale = h->prm.scale;
    return EGX_SUCCESS;
}

int32_t egx_infill_set_cstr_strategy(egx_infill *h, int32_t strategy, const double *scale_cstr) {
    if (!h) return fail(EGX_ERR_INVALID_VALUE, "NULL handle");
    if (strategy < EGX_CSTR_INFILL || strategy > EGX_CSTR_UTB) return fail(EGX_ERR_INVALID_VALUE, "infill: unknown constraint strategy");
    std::lock_guard<std::mutex> lock(h->mu);
    const size_t k = h->surr.size() - 1;
    if (scale_cstr) {
        for (size_t j = 0; j < k; j++)
            if (!(scale_cstr[j] > 0.0) || std::isinf(scale_cstr[j]))
                return fail(EGX_ERR_INVALID_VALUE, "infill: scale_cstr " + std::to_string(j) + " must be positive and finite");
        h->scale_cstr.assign(scale_cstr, scale_cstr + k);
        h->scale_on_device = false;
    }
    h->strategy = strategy;
    return EGX_SUCCESS;
}

int32_t egx_infill_get_cstr_strategy(egx_infill *h, int32_t *strategy, double *scale_cstr) {
    if (!h || !strategy) return fail(EGX_ERR_INVALID_VALUE, "NULL argument");
    std::lock_guard<std::mutex> lock(h->mu);
    *strategy = h->strategy;
    if (scale_cstr) std::copy(h->scale_cstr.begin(), h->scale_cstr.end(), scale_cstr);
    return EGX_SUCCESS;
}

int32_t egx_infill_eval(egx_infill *h, const double *xq, int64_t m, double *value, double *grad, const egx_infill_parts *parts) {
    if (!h || (m > 0 && !value)) return fail(EGX_ERR_INVALID_VALUE, "NULL argument");
    std::lock_guard<std::mutex> lock(h->mu);
    ModelLocks locks(h);
    return eval_active(h, xq, m, value, grad, parts);
}

int32_t egx_infill_eval_cstr(egx_infill *h, const double *xq, int64_t m, double *value, double *cstr, double *grad,
                             double *grad_cstr) {
    if (!h || (m > 0 && !value) || (m > 0 && h->surr.size() > 1 && !cstr)) return fail(EGX_ERR_INVALID_VALUE, "NULL argument");
    std::lock_guard<std::mutex> lock(h->mu);
    if (h->strategy == infill::kCstrInfill)
        return fail(EGX_ERR_INVALID_VALUE,
                    "infill: the handle folds its constraints into the objective (EGX_CSTR_INFILL); set EGX_CSTR_MEAN or EGX_CSTR_UTB");
    ModelLocks locks(h);
    CstrOut co;
    co.cstr = cstr, co.gcstr = grad_cstr;
    return eval_active(h, xq, m, value, grad, nullptr, &co);
}

int32_t egx_infill_set_active(egx_infill *h, const int32_t *active, int32_t n_active, const double *x_base) {
    if (!h) return fail(EGX_ERR_INVALID_VALUE, "NULL handle");
    std::lock_guard<std::mutex> lock(h->mu);
    std::string msg;
    if (!active::check(active, n_active, x_base, h->d, msg)) return fail(EGX_ERR_INVALID_VALUE, msg);
    h->active.assign(active, active + n_active);
    h->x_base.assign(x_base, x_base + h->d);
    h->active_on_device = false;
    return EGX_SUCCESS;
}

int32_t egx_infill_clear_active(egx_infill *h) {
    if (!h) return fail(EGX_ERR_INVALID_VALUE, "NULL handle");
    std::lock_guard<std::mutex> lock(h->mu);
    h->active.clear();
    h->x_base.clear();
    h->active_on_device = false;
    return EGX_SUCCESS;
}

int32_t egx_infill_get_active(egx_infill *h, int32_t *n_active, int32_t *active, double *x_base) {
    if (!h || !n_active) return fail(EGX_ERR_INVALID_VALUE, "NULL argument");
    std::lock_guard<std::mutex> lock(h->mu);
    *n_active = (int32_t)h->active.size();
    if (active) std::copy(h->active.begin(), h->active.end(), active);
    if (x_base) std::copy(h->x_base.begin(), h->x_base.end(), x_base);
    return EGX_SUCCESS;
}

int32_t egx_infill_get_runs(egx_infill *h, int32_t *n_runs, int32_t *run_len) {
    if (!h || !n_runs) return fail(EGX_ERR_INVALID_VALUE, "NULL argument");
    std::lock_guard<std::mutex> lock(h->mu);
    ModelLocks locks(h);  // (the shapes are read from the models)
    const std::vector<int> lens = walk_runs(h, h->strategy == infill::kCstrMean, h->q > 0);
    *n_runs = (int32_t)lens.size();
    if (run_len) std::copy(lens.begin(), lens.end(), run_len);
    return EGX_SUCCESS;
}

int32_t egx_infill_eval_experts(egx_infill *h, int32_t j, const double *xq, int64_t m, double *mean, double *var, double *grad_mean,
                                double *grad_var, double *probas, double *dprobas) {
    if (!h) return fail(EGX_ERR_INVALID_VALUE, "NULL handle");
    if (j < 0 || j >= (int32_t)h->surr.size()) return fail(EGX_ERR_INVALID_VALUE, "infill: surrogate " + std::to_string(j) + " out of range");
    std::lock_guard<std::mutex> lock(h->mu);
    ModelLocks locks(h);
    ExpertDiag dg;
    dg.j = j, dg.mean = mean, dg.var = var, dg.gmean = grad_mean, dg.gvar = grad_var, dg.probas = probas, dg.dprobas = dprobas;
    return eval_guarded(h, xq, m, nullptr, nullptr, nullptr, &dg);
}

int32_t egx_infill_scaling(egx_infill *h, const double *pts, int64_t npts, double *scale_ic_out, double *scale_out,
                           double *scale_cstr) {
    if (!h || npts < 1 || !pts) return fail(EGX_ERR_INVALID_VALUE, "infill scaling: needs a handle and at least one point");
    std::lock_guard<std::mutex> lock(h->mu);
    ModelLocks locks(h);
    const int nm = (int)h->surr.size(), n_cstr = nm - 1;
    // under EGX_CSTR_MEAN / _UTB the scale is that of the objective alone (compute_infill_obj_scale with cstr_infill = false,
    // solver_computations.rs:322-330): the terms below are formed as for a handle without constraint models
    const bool folded = h->strategy == infill::kCstrInfill;
    const int k = folded ? n_cstr : 0;
    // ONE values-only pass over all points (means and variances of every model stay on the device); the criterion's terms are
    // then formed ON THE DEVICE with the text of k_infill_combine, so that what is stored is bit for bit the largest |value|
    // egx_infill_eval returns at scale = 1 (all values finite).  The host does the NaN / inf -> 1 replacement, the last
    // multiplication / subtraction, max and argmax.
    std::vector<double> mean((size_t)nm * npts);
    egx_infill_parts parts{mean.data(), nullptr, nullptr, nullptr};
    EGX_RC(eval_guarded(h, pts, npts, nullptr, nullptr, &parts));
    hipStream_t st = h->models[0].stream();
    EGX_RC(h->value.alloc((size_t)2 * round_up(npts, kTile)));
    infill::Params prm = h->prm;
    prm.scale = 1.0;
    prm.feasibility = 1;
    std::vector<double> base((size_t)npts), fac((size_t)npts);
    double scale_ic = 1.0;
    if (prm.kind == infill::kWB2S) {  // compute_wb2s_scale, criteria/wb2.rs:67-88 (argmax: the first maximum)
        EGX_RC(scale_terms(h, st, prm, k, npts, base.data(), nullptr, nullptr, "the EI values"));
        int64_t i_max = 0;
        for (int64_t i = 1; i < npts; i++)
            if (base[i] > base[i_max] || std::isnan(base[i_max])) i_max = i;
        if (std::fabs(base[i_max]) > 100.0 * infill::kEps) scale_ic = 100.0 * std::fabs(mean[i_max]) / base[i_max];
    }
    prm.scale_ic = scale_ic;
    EGX_RC(scale_terms(h, st, prm, k, npts, nullptr, base.data(), fac.data(), "the criterion's terms"));
    double scale = 0.0;  // compute_infill_obj_scale, solver_computations.rs:297-351
    for (int64_t i = 0; i < npts; i++) {
        double v = base[i];
        if (std::isnan(v) || std::isinf(v)) v = 1.0;
        if (k > 0) v = (prm.kind == infill::kLogEI) ? v - fac[i] : v * fac[i];
        scale = std::fmax(scale, std::fabs(v));
    }
    if (scale < 100.0 * infill::kEps || std::isnan(scale) || std::isinf(scale)) scale = 1.0;
    if (scale_cstr || !folded) cstr_scales(h, mean.data(), npts, folded, scale_cstr);
    h->prm.scale_ic = scale_ic;
    h->prm.scale = scale;
    if (scale_ic_out) *scale_ic_out = scale_ic;
    if (scale_out) *scale_out = scale;
    return EGX_SUCCESS;
}

}  // extern "C"
