// EGO's infill criterion on fitted GPs, dense or sparse (crates/ego/src/criteria/{ei,wb2}.rs, utils/{logei_helper,cstr_pof}.rs,
// solver/solver_computations.rs:132-193, 297-475, solver/solver_infill_optim.rs:148-236): the minimised objective and its
// x-gradient for m points in one call, from one objective model and k constraint models; the scaling pass; the lock-step
// COBYLA multistart.
//
// A call walks the points in tiles of EXACTLY kTile = 128 and, per tile, the models one after the other through the launch
// sequence of predict_impl / xgrad_impl (posterior_solve, posterior_weights, the split rules: gp_predict.hip); what those
// do on the host between their launches runs in the kernels of kernels_infill.hip, and k_infill_combine applies
// infill_math.h across the models.  One upload, one launch sequence per (tile, model), one combine, the copies back, ONE
// synchronisation: the count depends on k and on the number of tiles only.
// Every launch of a tile has the padded batch size 128, and the splits of the training range are functions of the model
// alone: the bits of a point do not depend on where it sits nor on its companions (tests/test_gpu_infill.py).
//
// A SURROGATE -- the objective, a constraint -- is one dense GP or a mixture of k experts with its Gaussian mixture
// (egx_infill_create_mix; GpMixture, crates/moe/src/algorithm.rs).  The walk is tile -> surrogate -> expert through the same
// sequence; a lone expert writes the surrogate's slot of the tables, the experts of a mixture write the expert tables and ONE
// k_infill_mix launch per (tile, surrogate) recombines them into the slot (smooth: the weighted sums; hard: the expert of the
// first maximum of the responsibilities -- every expert still evaluates the whole tile, so that every launch keeps the padded
// batch of 128).  Locks, caches, checks and scratch sizes run over the flat list of all experts.
//
// An EXPERT is a dense GP or a SPARSE one (egx_infill_create_any: tagged references, mixed freely).  A sparse expert writes the
// same table slots from its own tile sequence, sgp_expert_tile: the batched route of sgp_query (sgp_predict.hip) at the padded
// batch of 128 -- raw x, K(x, z) . (sigma2 vec) in split partial sums, K(x, z), the two block solves with their row reductions,
// k_infill_sgp_finish (var = egx_sgp_predict_var's: clamp, then + noise); with gradients the two transposed products with the
// cached inverse factors, launch_xgrad twice, k_infill_sgp_xgrad_finish (exactly 0 under the clamp).  Everything downstream
// reads slots only.  Its mean-only twin runs no solve and keeps the means' bits.
//
// CONSTRAINT STRATEGIES (egx_infill_set_cstr_strategy).  EGX_CSTR_INFILL folds the constraint surrogates into the objective (the
// above).  Under EGX_CSTR_MEAN / _UTB the objective carries no feasibility factor and the constraints are handed to the
// optimiser as c(x) <= 0 (egx_infill_eval_cstr, egx_infill_optimize_cstr; solver_infill_optim.rs:148-204).  Under MEAN nobody
// reads a constraint surrogate's variance, and its experts run the MEAN-ONLY sequence: prepare, predict_mean, the mean half of
// the trend tail (and, for gradients, ONE launch_xgrad with gamma and the mean half of its finish) -- no posterior_solve, no
// weights, no second contraction; the means keep the bits of the full sequence, which forms r . gamma before its solve as
// well.  A call that does not ask for anything of the constraint surrogates (egx_infill_eval without parts under MEAN / UTB)
// does not run them at all.
#include <map>

#include "gmx_point.h"
#include "sgp_handle.h"
#include "infill_math.h"
#include "slsqp.h"

using namespace egx;

namespace {

// A tagged reference to an expert: a dense model or a sparse one (egx_model_ref); exactly one of the two pointers is set
struct ModelRef {
    egx_gp *gp = nullptr;
    egx_sgp *sg = nullptr;
    ModelRef() = default;
    explicit ModelRef(egx_gp *g) : gp(g) {}
    explicit ModelRef(egx_sgp *g) : sg(g) {}
    bool sparse() const { return sg != nullptr; }
    const void *addr() const { return sg ? static_cast<const void *>(sg) : static_cast<const void *>(gp); }
    int d() const { return sg ? sg->d : gp->d; }
    int device() const { return sg ? sg->device : gp->device; }
    bool fitted() const { return sg ? sg->fitted : (bool)gp->fitted; }
    hipStream_t stream() const { return sg ? sg->stream : gp->ws[0].stream; }
};

// models[first .. first + k) are the surrogate's experts; with k >= 2 they own the slots [eslot, eslot + k) of the expert tables
struct Surrogate {
    int first = 0, k = 1, eslot = -1;
    bool smooth = true;
    std::vector<double> gmx;  // means (k d) | scaled precision factors (k d d) | par (k), as k_gmx_probas reads them
    DevBuf d_gmx;             // uploaded on the first evaluation
    bool on_device = false;
};

}  // namespace

struct egx_infill {
    std::mutex mu;
    std::vector<ModelRef> models;  // every expert of every surrogate, surrogate by surrogate (borrowed)
    std::vector<Surrogate> surr;   // [0] the objective, then the constraints
    bool mix_api = false;          // created by egx_infill_create_mix: messages name surrogate and expert
    int n_eslots = 0, k_max = 1;
    std::vector<double> tol;       // one per constraint
    infill::Params prm{};
    int d = 0, device = 0;
    DevBuf d_tol;
    bool tol_on_device = false;
    // buffers of a call (grow-only): the whole call's points and results, then the scratch of ONE (tile, model) step
    DevBuf xraw, flag, mean, var, gmean, gvar, value, grad;
    DevBuf xcast;  // models with xtypes and a mixture among the surrogates: the call's CAST raw points (k_infill_prepare_mixint)
    DevBuf xqT, racc, RT, s0, sl, Wt, dneg, out_y, out_v;
    // sparse experts: x_mean = 0 | x_std = 1 (the prepare kernel's parameters for RAW points), |b~|^2 of a tile, the copy of a~
    DevBuf ident, s1, sE;
    bool ident_on_device = false;
    // the experts of the mixtures: their tables (slot-major like mean / var), d p / d x of one tile, the diagnostics of a call
    DevBuf emean, evar, egmean, egvar, dprob, dg_probas, dg_dprobas;
    // how the constraint surrogates enter (infill::CstrStrategy), their scales, the tables of egx_infill_eval_cstr
    int strategy = infill::kCstrInfill;
    std::vector<double> scale_cstr;  // one per constraint, ones until set
    DevBuf d_scale, cstr, gcstr;
    bool scale_on_device = false;
};

namespace {

// The distinct models' locks (a model may serve twice, e.g. as objective and as a constraint), taken in ADDRESS order, not in
// index order: two handles that hold the same models in opposite roles and are evaluated from two threads would otherwise
// take the exclusive locks in opposite orders.
// Dense and sparse models share ONE order (a dense model's lock is a shared mutex, a sparse model's a plain one).
struct ModelLocks {
    std::vector<std::unique_lock<std::shared_mutex>> held;
    std::vector<std::unique_lock<std::mutex>> held_sparse;
    explicit ModelLocks(egx_infill *h) {
        std::map<const void *, ModelRef, std::less<const void *>> distinct;
        for (const ModelRef &r : h->models) distinct.emplace(r.addr(), r);
        for (const auto &kv : distinct) {
            if (kv.second.sparse()) held_sparse.emplace_back(kv.second.sg->mu);
            else held.emplace_back(kv.second.gp->mu);
        }
    }
};

// "model j" for a handle of egx_infill_create, "surrogate j expert e" for one of egx_infill_create_mix
std::string who(const egx_infill *h, int idx) {
    if (!h->mix_api) return "model " + std::to_string(idx);
    for (size_t j = 0; j < h->surr.size(); j++)
        if (idx < h->surr[j].first + h->surr[j].k)
            return "surrogate " + std::to_string(j) + " expert " + std::to_string(idx - h->surr[j].first);
    return "model " + std::to_string(idx);
}

int check_fitted(const egx_infill *h) {
    for (size_t e = 0; e < h->models.size(); e++)
        if (!h->models[e].fitted()) {
            set_error("infill: " + who(h, (int)e) + " is not fitted (call " +
                      (h->models[e].sparse() ? "egx_sgp_finalize or egx_sgp_fit" : "egx_gp_finalize or egx_gp_fit") + " first)");
            return EGX_ERR_NOT_FITTED;
        }
    return EGX_SUCCESS;
}

// same d, same device as expert 0 of the objective
int check_shapes(egx_infill *h) {
    h->d = h->models[0].d();
    h->device = h->models[0].device();
    for (size_t e = 1; e < h->models.size(); e++) {
        if (h->models[e].d() != h->d) {
            set_error("infill: " + who(h, (int)e) + " has " + std::to_string(h->models[e].d()) + " inputs, " + who(h, 0) + " has " +
                      std::to_string(h->d));
            return EGX_ERR_INVALID_VALUE;
        }
        if (h->models[e].device() != h->device) {
            set_error("infill: " + who(h, (int)e) + " lives on device " + std::to_string(h->models[e].device()) + ", " + who(h, 0) +
                      " on device " + std::to_string(h->device));
            return EGX_ERR_INVALID_VALUE;
        }
    }
    // the x-gradient contraction of a sparse expert stages d * (hcols + 5) doubles, hcols = 1 (sgp_predict.hip)
    for (size_t e = 0; e < h->models.size(); e++)
        if (h->models[e].sparse() && (int64_t)h->d * 6 > 20480) {
            set_error("infill: " + who(h, (int)e) + ": the x-gradients of a sparse model need 6 d <= 20480 (d " + std::to_string(h->d) + ")");
            return EGX_ERR_UNSUPPORTED;
        }
    return EGX_SUCCESS;
}

// Mixed-integer models: every expert of every surrogate carries the same xtypes as expert 0 of the objective, or none does -- the
// points of a call are one design space.  Read from the models at EVERY call (as their fitted state is), under their locks.
// A sparse model carries none.
int check_specs(const egx_infill *h) {
    static const MixSpec none;
    auto spec = [](const ModelRef &r) -> const MixSpec & { return r.sparse() ? none : r.gp->xspec; };
    for (size_t e = 1; e < h->models.size(); e++)
        if (!spec(h->models[e]).same(spec(h->models[0]))) {
            set_error("infill: " + who(h, (int)e) + " and " + who(h, 0) + " carry different xtypes (egx_gp_set_xtypes): all or none, the same spec");
            return EGX_ERR_INVALID_VALUE;
        }
    return EGX_SUCCESS;
}

// what egx_infill_eval_experts asks for: the parts of surrogate j's experts and its responsibilities (host pointers, any nullptr)
struct ExpertDiag {
    int j = 0;
    double *mean = nullptr, *var = nullptr, *gmean = nullptr, *gvar = nullptr, *probas = nullptr, *dprobas = nullptr;
};

// One expert's launch sequence for one tile: mean / var (and gmean / gvar when want_g) point at the tile's kTile entries of the
// table the expert writes; flag: the tile's flags, written by the first expert of the call only (else nullptr).
int expert_tile(egx_infill *h, hipStream_t st, int j, int64_t t0, int mt, bool want_g, double *mean, double *var, double *gmean,
                double *gvar, int *flag) {
    const int d = h->d;
    egx_gp *gp = h->models[j].gp;
    const int n = gp->n, n_pad = gp->n_pad;
    const int msplit = mean_splits(n_pad, kTile), nsplit = xgrad_splits(n, kTile);
    // (xtypes: cast in the same launch; the expert that writes the flags leaves the cast raw tile for k_infill_mix as well)
    EGX_RC(launch_infill_prepare(st, h->xraw.p + (size_t)t0 * d, mt, d, dev_xnorm(gp), h->xqT.p, flag, dev_spec(gp),
                                 flag && h->n_eslots > 0 && dev_spec(gp) ? h->xcast.p + (size_t)t0 * d : nullptr));
    // r . gamma in split partial sums (algorithm.rs:260-262), before the solve overwrites r
    EGX_RC(launch_predict_mean(st, gp->corr, h->xqT.p, kTile, kTile, gp->d_xT, n_pad, n_pad, d, gp->d_fit_coef,
                               gp->fit_hcols, gp->d_gamma, h->racc.p, msplit,
                               gp->fit_hcols == 1 ? dev_xs_fit(gp) : nullptr));
    // rt = C^-1 r (held transposed), sum rt^2 and ft^T rt (:337-352)
    EGX_RC(posterior_solve(gp, st, h->xqT.p, kTile, h->RT.p, h->s0.p, h->sl.p));
    InfillTrend tr;
    tr.p = gp->p, tr.rp = gp->rhs_pad, tr.msplit = msplit;
    tr.xqT = h->xqT.p, tr.fidx = gp->d_fidx, tr.beta = gp->d_tbeta, tr.R = gp->d_rq, tr.Rt = gp->d_rqT;
    tr.racc = h->racc.p, tr.s0 = h->s0.p, tr.sl = h->sl.p;
    tr.sigma2 = gp->sigma2, tr.y_mean = gp->y_mean, tr.y_std = gp->y_std;
    tr.mean = mean, tr.var = var;
    tr.dneg = want_g ? h->dneg.p : nullptr;
    EGX_RC(launch_infill_trend(st, tr));
    if (!want_g) return EGX_SUCCESS;
    // -(R^-1 r + R^-1 F D)^T as an (n_pad x 128) weight matrix, then the two contractions
    EGX_RC(posterior_weights(gp, st, h->RT.p, kTile, h->Wt.p));
    EGX_RC(posterior_weights_trend(gp, st, h->dneg.p, kTile, h->Wt.p));
    EGX_RC(launch_xgrad(st, gp->corr, h->xqT.p, kTile, kTile, gp->d_xT, n_pad, n, d, gp->d_fit_coef, gp->fit_hcols,
                        gp->d_gamma, 0, 1, nsplit, h->out_y.p));
    EGX_RC(launch_xgrad(st, gp->corr, h->xqT.p, kTile, kTile, gp->d_xT, n_pad, n, d, gp->d_fit_coef, gp->fit_hcols,
                        h->Wt.p, kTile, 0, nsplit, h->out_v.p));
    return launch_infill_xgrad_finish(st, tr, d, nsplit, h->out_y.p, h->out_v.p, dev_xnorm(gp) + d, gmean, gvar);
}

// The mean-only sequence of one expert for one tile: what expert_tile launches for mean / gmean and nothing else.
int expert_tile_mean(egx_infill *h, hipStream_t st, int j, int64_t t0, int mt, bool want_g, double *mean, double *gmean, int *flag) {
    const int d = h->d;
    egx_gp *gp = h->models[j].gp;
    const int n = gp->n, n_pad = gp->n_pad;
    const int msplit = mean_splits(n_pad, kTile), nsplit = xgrad_splits(n, kTile);
    EGX_RC(launch_infill_prepare(st, h->xraw.p + (size_t)t0 * d, mt, d, dev_xnorm(gp), h->xqT.p, flag, dev_spec(gp)));
    EGX_RC(launch_predict_mean(st, gp->corr, h->xqT.p, kTile, kTile, gp->d_xT, n_pad, n_pad, d, gp->d_fit_coef,
                               gp->fit_hcols, gp->d_gamma, h->racc.p, msplit,
                               gp->fit_hcols == 1 ? dev_xs_fit(gp) : nullptr));
    InfillTrend tr;
    tr.p = gp->p, tr.rp = gp->rhs_pad, tr.msplit = msplit;
    tr.xqT = h->xqT.p, tr.fidx = gp->d_fidx, tr.beta = gp->d_tbeta;
    tr.racc = h->racc.p;
    tr.y_mean = gp->y_mean, tr.y_std = gp->y_std;
    tr.mean = mean;
    EGX_RC(launch_infill_trend_mean(st, tr));
    if (!want_g) return EGX_SUCCESS;
    EGX_RC(launch_xgrad(st, gp->corr, h->xqT.p, kTile, kTile, gp->d_xT, n_pad, n, d, gp->d_fit_coef, gp->fit_hcols,
                        gp->d_gamma, 0, 1, nsplit, h->out_y.p));
    return launch_infill_xgrad_finish_mean(st, tr, d, nsplit, h->out_y.p, dev_xnorm(gp) + d, gmean);
}

// A SPARSE expert's launch sequence for one tile, the batched route of sgp_query (sgp_predict.hip) at the padded batch of 128
// whatever the call's size: raw x, K(x, z) . (sigma2 vec) in split partial sums, K(x, z), the two block solves with their row
// reductions, the finish; with gradients the two transposed products with the cached inverse factors (sgp_ensure_inverse_factors,
// built by eval_locked), the two contractions and their finish.  Arguments as expert_tile.
int sgp_expert_tile(egx_infill *h, hipStream_t st, int j, int64_t t0, int mt, bool want_g, double *mean, double *var, double *gmean,
                    double *gvar, int *flag) {
    const int d = h->d;
    egx_sgp *g = h->models[j].sg;
    const int nz = g->nz, z_pad = g->z_pad, vfe = g->method != 0;
    const int msplit = mean_splits(z_pad, kTile), nsplit = xgrad_splits(nz, kTile);
    const size_t blk = (size_t)kTile * z_pad;
    EGX_RC(launch_infill_prepare(st, h->xraw.p + (size_t)t0 * d, mt, d, h->ident.p, h->xqT.p, flag));
    EGX_RC(launch_predict_mean(st, g->corr, h->xqT.p, kTile, kTile, g->zT.p, z_pad, z_pad, d, g->coef.p, 1, g->vec.p, h->racc.p, msplit));
    EGX_RC(launch_cross_corr(st, g->corr, h->xqT.p, kTile, kTile, g->zT.p, z_pad, z_pad, d, g->coef.p, 1, h->RT.p, z_pad));
    EGX_RC(launch_trsm_rows(st, g->Kz.p, z_pad, z_pad, g->dinv_z.p, h->RT.p, z_pad, kTile));  // a~ = C_z^-1 r
    EGX_RC(launch_row_reduce(st, h->RT.p, z_pad, kTile, nz, nullptr, 0, 0, h->s0.p, nullptr));
    if (want_g) EGX_RC(sgp_launch_scale_copy(st, h->RT.p, vfe ? -1.0 : 1.0, (int64_t)blk, h->sE.p));  // E = -s a~: the GEMMs subtract
    EGX_RC(launch_trsm_rows(st, g->A.p, z_pad, z_pad, g->dinv_a.p, h->RT.p, z_pad, kTile));  // b~ = L^-1 a~
    EGX_RC(launch_row_reduce(st, h->RT.p, z_pad, kTile, nz, nullptr, 0, 0, h->s1.p, nullptr));
    EGX_RC(launch_infill_sgp_finish(st, h->racc.p, msplit, h->s0.p, h->s1.p, g->sigma2, g->noise, vfe, mean, var));
    if (!want_g) return EGX_SUCCESS;
    // E -= b~ (L^-T)^T, then Ct = 0 - C_z^-T E^T = s c transposed (z_pad x 128): the weight layout of launch_xgrad
    EGX_RC(launch_gemm_nt_sub(st, h->sE.p, z_pad, h->RT.p, z_pad, g->Wa.p, z_pad, kTile, z_pad, z_pad, 0, 0));
    EGX_HIP_CHECK(hipMemsetAsync(h->Wt.p, 0, sizeof(double) * blk, st));
    EGX_RC(launch_gemm_nt_sub(st, h->Wt.p, kTile, g->Wz.p, z_pad, h->sE.p, z_pad, z_pad, kTile, z_pad, 0, 1));
    EGX_RC(launch_xgrad(st, g->corr, h->xqT.p, kTile, kTile, g->zT.p, z_pad, nz, d, g->coef.p, 1, g->vec.p, 0, 1, nsplit, h->out_y.p));
    EGX_RC(launch_xgrad(st, g->corr, h->xqT.p, kTile, kTile, g->zT.p, z_pad, nz, d, g->coef.p, 1, h->Wt.p, kTile, 0, nsplit,
                        h->out_v.p));
    return launch_infill_sgp_xgrad_finish(st, h->out_y.p, h->out_v.p, nsplit, d, h->s0.p, h->s1.p, g->sigma2, vfe,
                                          (vfe ? -2.0 : 2.0) * g->sigma2, gmean, gvar);
}

// The mean-only sequence of a sparse expert: what sgp_expert_tile launches for mean / gmean and nothing else -- no K(x, z) block,
// no solve; the same partial sums in the same order, so the means keep the full sequence's bits.
int sgp_expert_tile_mean(egx_infill *h, hipStream_t st, int j, int64_t t0, int mt, bool want_g, double *mean, double *gmean, int *flag) {
    const int d = h->d;
    egx_sgp *g = h->models[j].sg;
    const int nz = g->nz, z_pad = g->z_pad;
    const int msplit = mean_splits(z_pad, kTile), nsplit = xgrad_splits(nz, kTile);
    EGX_RC(launch_infill_prepare(st, h->xraw.p + (size_t)t0 * d, mt, d, h->ident.p, h->xqT.p, flag));
    EGX_RC(launch_predict_mean(st, g->corr, h->xqT.p, kTile, kTile, g->zT.p, z_pad, z_pad, d, g->coef.p, 1, g->vec.p, h->racc.p, msplit));
    EGX_RC(launch_infill_sgp_finish(st, h->racc.p, msplit, nullptr, nullptr, g->sigma2, g->noise, 0, mean, nullptr));
    if (!want_g) return EGX_SUCCESS;
    EGX_RC(launch_xgrad(st, g->corr, h->xqT.p, kTile, kTile, g->zT.p, z_pad, nz, d, g->coef.p, 1, g->vec.p, 0, 1, nsplit, h->out_y.p));
    return launch_infill_sgp_xgrad_finish(st, h->out_y.p, nullptr, nsplit, d, nullptr, nullptr, g->sigma2, 0, 0.0, gmean, nullptr);
}

// what egx_infill_eval_cstr asks for beside value / grad (host pointers, any nullptr)
struct CstrOut {
    double *cstr = nullptr, *gcstr = nullptr;
};

// The evaluation proper; the handle's and the models' locks are held.  value / grad / every member of parts may be nullptr.
int eval_locked(egx_infill *h, const double *xq, int64_t m, double *value, double *grad, const egx_infill_parts *parts,
                const ExpertDiag *diag = nullptr, const CstrOut *co = nullptr) {
    if (m < 0 || (m > 0 && !xq)) {
        set_error("bad query array");
        return EGX_ERR_INVALID_VALUE;
    }
    const int ne = (int)h->models.size(), nm = (int)h->surr.size(), k = nm - 1, d = h->d;
    EGX_RC(check_fitted(h));
    EGX_RC(check_specs(h));
    if (m == 0) return EGX_SUCCESS;
    const bool want_g = grad || (parts && (parts->grad_mean || parts->grad_var)) ||
                        (diag && (diag->gmean || diag->gvar || diag->dprobas)) || (co && co->gcstr);
    // the constraint surrogates: folded into the objective (all of them, the full sequence), or run only when something of
    // theirs is asked for, and then mean-only when no variance of theirs is read
    const bool folded = h->strategy == infill::kCstrInfill;
    const bool run_c = folded || parts || diag || (co && (co->cstr || co->gcstr));
    const bool mean_c = h->strategy == infill::kCstrMean && !diag && !(parts && (parts->var || parts->grad_var));
    const int n_obj = h->surr[0].k;  // models[0 .. n_obj) are the objective's experts
    EGX_HIP_CHECK(hipSetDevice(h->device));
    hipStream_t st = h->models[0].stream();
    bool any_sparse = false;
    for (const ModelRef &r : h->models) any_sparse |= r.sparse();
    if (want_g)  // once per fitted state (synchronises the model's stream); the mean-only sequence does not read C^-T
        for (int e = 0; e < (run_c && !mean_c ? ne : n_obj); e++) {
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
    if (any_sparse && !h->ident_on_device) {
        std::vector<double> id((size_t)2 * d, 0.0);
        std::fill(id.begin() + d, id.end(), 1.0);
        EGX_RC(h->ident.alloc(id.size()));
        EGX_HIP_CHECK(hipMemcpyAsync(h->ident.p, id.data(), sizeof(double) * id.size(), hipMemcpyHostToDevice, st));
        EGX_HIP_CHECK(hipStreamSynchronize(st));  // id is a local
        h->ident_on_device = true;
    }
    for (Surrogate &sg : h->surr)
        if (sg.k >= 2 && !sg.on_device) {
            EGX_RC(sg.d_gmx.alloc(sg.gmx.size()));
            EGX_HIP_CHECK(hipMemcpyAsync(sg.d_gmx.p, sg.gmx.data(), sizeof(double) * sg.gmx.size(), hipMemcpyHostToDevice, st));
            sg.on_device = true;
        }
    if (k > 0 && !folded && !h->scale_on_device) {
        EGX_RC(h->d_scale.alloc(k));
        EGX_HIP_CHECK(hipMemcpyAsync(h->d_scale.p, h->scale_cstr.data(), sizeof(double) * k, hipMemcpyHostToDevice, st));
        h->scale_on_device = true;
    }
    if (k > 0 && !h->tol_on_device) {
        EGX_RC(h->d_tol.alloc(k));
        EGX_HIP_CHECK(hipMemcpyAsync(h->d_tol.p, h->tol.data(), sizeof(double) * k, hipMemcpyHostToDevice, st));
        h->tol_on_device = true;
    }
    const int64_t M = round_up(m, kTile);
    int n_pad_max = 0, p_max = 1, rp_max = 1, ms_max = 0, ns_max = 0, z_pad_max = 0;
    for (const ModelRef &r : h->models) {
        if (r.sparse()) {  // the inducing points stand where a dense model's training points do
            n_pad_max = std::max(n_pad_max, r.sg->z_pad);
            z_pad_max = std::max(z_pad_max, r.sg->z_pad);
            ms_max = std::max(ms_max, mean_splits(r.sg->z_pad, kTile));
            ns_max = std::max(ns_max, xgrad_splits(r.sg->nz, kTile));
            continue;
        }
        const egx_gp *gp = r.gp;
        n_pad_max = std::max(n_pad_max, gp->n_pad);
        p_max = std::max(p_max, gp->p);
        rp_max = std::max(rp_max, gp->rhs_pad);
        ms_max = std::max(ms_max, mean_splits(gp->n_pad, kTile));
        ns_max = std::max(ns_max, xgrad_splits(gp->n, kTile));
    }
    EGX_RC(h->xraw.alloc((size_t)m * d));
    const bool typed = !h->models[0].sparse() && !h->models[0].gp->xspec.empty();
    if (typed && h->n_eslots > 0) EGX_RC(h->xcast.alloc((size_t)m * d));
    EGX_RC(h->flag.alloc((size_t)(M + 1) / 2));
    EGX_RC(h->mean.alloc((size_t)nm * M));
    EGX_RC(h->var.alloc((size_t)nm * M));
    EGX_RC(h->value.alloc((size_t)M));
    EGX_RC(h->xqT.alloc((size_t)d * kTile));
    EGX_RC(h->racc.alloc((size_t)ms_max * kTile));
    EGX_RC(h->RT.alloc((size_t)kTile * n_pad_max));
    EGX_RC(h->s0.alloc(kTile));
    EGX_RC(h->sl.alloc((size_t)kTile * p_max));
    if (any_sparse) EGX_RC(h->s1.alloc(kTile));
    if (want_g) {
        if (any_sparse) EGX_RC(h->sE.alloc((size_t)kTile * z_pad_max));
        EGX_RC(h->gmean.alloc((size_t)nm * M * d));
        EGX_RC(h->gvar.alloc((size_t)nm * M * d));
        EGX_RC(h->grad.alloc((size_t)M * d));
        EGX_RC(h->Wt.alloc((size_t)n_pad_max * kTile));
        EGX_RC(h->dneg.alloc((size_t)kTile * rp_max));
        EGX_RC(h->out_y.alloc((size_t)ns_max * kTile * d));
        EGX_RC(h->out_v.alloc((size_t)ns_max * kTile * d));
    }
    const int ns = h->n_eslots;
    const Surrogate *dsg = diag ? &h->surr[diag->j] : nullptr;
    const bool diag_mix = dsg && dsg->k >= 2;
    if (ns > 0) {
        EGX_RC(h->emean.alloc((size_t)ns * M));
        EGX_RC(h->evar.alloc((size_t)ns * M));
        if (want_g) {
            EGX_RC(h->egmean.alloc((size_t)ns * M * d));
            EGX_RC(h->egvar.alloc((size_t)ns * M * d));
            EGX_RC(h->dprob.alloc((size_t)kTile * h->k_max * d));
        }
    }
    if (co && k > 0) {
        if (co->cstr) EGX_RC(h->cstr.alloc((size_t)M * k));
        if (co->gcstr) EGX_RC(h->gcstr.alloc((size_t)M * k * d));
    }
    if (diag_mix) {
        EGX_RC(h->dg_probas.alloc((size_t)M * dsg->k));
        if (diag->dprobas) EGX_RC(h->dg_dprobas.alloc((size_t)M * dsg->k * d));
    }
    int *flag = reinterpret_cast<int *>(h->flag.p);
    EGX_HIP_CHECK(hipMemcpyAsync(h->xraw.p, xq, sizeof(double) * (size_t)m * d, hipMemcpyHostToDevice, st));
    for (int64_t t0 = 0; t0 < m; t0 += kTile) {
        const int mt = (int)std::min<int64_t>(kTile, m - t0);
        for (int js = 0; js < (run_c ? nm : 1); js++) {
            const Surrogate &sg = h->surr[js];
            const bool lone = sg.k < 2;  // a lone expert writes the surrogate's slot, the experts of a mixture their own tables
            const bool mean_only = js > 0 && mean_c;
            for (int e = 0; e < sg.k; e++) {
                const size_t row = (lone ? (size_t)js : (size_t)(sg.eslot + e)) * M + t0;
                const bool sparse = h->models[sg.first + e].sparse();
                if (mean_only) {
                    EGX_RC((sparse ? sgp_expert_tile_mean : expert_tile_mean)(
                        h, st, sg.first + e, t0, mt, want_g, (lone ? h->mean.p : h->emean.p) + row,
                        want_g ? (lone ? h->gmean.p : h->egmean.p) + row * d : nullptr, nullptr));
                    continue;
                }
                EGX_RC((sparse ? sgp_expert_tile : expert_tile)(
                    h, st, sg.first + e, t0, mt, want_g, (lone ? h->mean.p : h->emean.p) + row, (lone ? h->var.p : h->evar.p) + row,
                    want_g ? (lone ? h->gmean.p : h->egmean.p) + row * d : nullptr,
                    want_g ? (lone ? h->gvar.p : h->egvar.p) + row * d : nullptr, sg.first + e == 0 ? flag + t0 : nullptr));
            }
            if (lone) continue;
            InfillMix mx;
            mx.mt = mt, mx.d = d, mx.k = sg.k, mx.smooth = sg.smooth, mx.want_g = want_g;
            mx.xq = (typed ? h->xcast.p : h->xraw.p) + (size_t)t0 * d, mx.flag = flag + t0;
            mx.means = sg.d_gmx.p, mx.precs = sg.d_gmx.p + (size_t)sg.k * d, mx.par = mx.precs + (size_t)sg.k * d * d;
            mx.emean = h->emean.p + (size_t)sg.eslot * M + t0, mx.evar = h->evar.p + (size_t)sg.eslot * M + t0;
            mx.estride = M;
            mx.mean = h->mean.p + (size_t)js * M + t0, mx.var = h->var.p + (size_t)js * M + t0;
            if (want_g) {
                mx.egmean = h->egmean.p + ((size_t)sg.eslot * M + t0) * d, mx.egvar = h->egvar.p + ((size_t)sg.eslot * M + t0) * d;
                mx.gmean = h->gmean.p + ((size_t)js * M + t0) * d, mx.gvar = h->gvar.p + ((size_t)js * M + t0) * d;
                if (sg.smooth) mx.dp = h->dprob.p;
            }
            if (diag_mix && dsg == &sg) {
                mx.probas = h->dg_probas.p + (size_t)t0 * sg.k;
                if (diag->dprobas) mx.dp = h->dg_dprobas.p + (size_t)t0 * sg.k * d;
            }
            EGX_RC(mean_only ? launch_infill_mix_mean(st, mx) : launch_infill_mix(st, mx));
        }
    }
    if (value && folded)
        EGX_RC(launch_infill_combine(st, h->prm, k, d, m, M, h->mean.p, h->var.p, want_g ? h->gmean.p : nullptr,
                                     want_g ? h->gvar.p : nullptr, h->d_tol.p, flag, h->value.p, grad ? h->grad.p : nullptr));
    if (value && !folded) {  // the objective model alone; the constraint values beside it for egx_infill_eval_cstr
        const int kc = co ? k : 0;
        EGX_RC(launch_infill_cstr(st, h->prm, h->strategy, kc, d, m, M, h->mean.p, h->var.p, want_g ? h->gmean.p : nullptr,
                                  want_g ? h->gvar.p : nullptr, h->d_scale.p, flag, h->value.p, kc && co->cstr ? h->cstr.p : nullptr,
                                  grad ? h->grad.p : nullptr, kc && co->gcstr ? h->gcstr.p : nullptr));
        if (kc && co->cstr)
            EGX_HIP_CHECK(hipMemcpyAsync(co->cstr, h->cstr.p, sizeof(double) * (size_t)m * k, hipMemcpyDeviceToHost, st));
        if (kc && co->gcstr)
            EGX_HIP_CHECK(hipMemcpyAsync(co->gcstr, h->gcstr.p, sizeof(double) * (size_t)m * k * d, hipMemcpyDeviceToHost, st));
    }
    if (value) EGX_HIP_CHECK(hipMemcpyAsync(value, h->value.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, st));
    if (grad) EGX_HIP_CHECK(hipMemcpyAsync(grad, h->grad.p, sizeof(double) * (size_t)m * d, hipMemcpyDeviceToHost, st));
    if (parts)
        for (int j = 0; j < nm; j++) {
            if (parts->mean)
                EGX_HIP_CHECK(hipMemcpyAsync(parts->mean + (size_t)j * m, h->mean.p + (size_t)j * M, sizeof(double) * (size_t)m,
                                             hipMemcpyDeviceToHost, st));
            if (parts->var)
                EGX_HIP_CHECK(hipMemcpyAsync(parts->var + (size_t)j * m, h->var.p + (size_t)j * M, sizeof(double) * (size_t)m,
                                             hipMemcpyDeviceToHost, st));
            if (parts->grad_mean)
                EGX_HIP_CHECK(hipMemcpyAsync(parts->grad_mean + (size_t)j * m * d, h->gmean.p + (size_t)j * M * d,
                                             sizeof(double) * (size_t)m * d, hipMemcpyDeviceToHost, st));
            if (parts->grad_var)
                EGX_HIP_CHECK(hipMemcpyAsync(parts->grad_var + (size_t)j * m * d, h->gvar.p + (size_t)j * M * d,
                                             sizeof(double) * (size_t)m * d, hipMemcpyDeviceToHost, st));
        }
    if (diag) {  // expert c of the surrogate: its slot of the expert tables, or (a lone expert) the surrogate's own slot
        auto back = [&](double *dst, const double *tab_e, const double *tab_s, size_t per) {
            if (!dst) return hipSuccess;
            for (int c = 0; c < dsg->k; c++) {
                const double *src = diag_mix ? tab_e + (size_t)(dsg->eslot + c) * M * per : tab_s + (size_t)diag->j * M * per;
                const hipError_t e = hipMemcpyAsync(dst + (size_t)c * m * per, src, sizeof(double) * (size_t)m * per,
                                                    hipMemcpyDeviceToHost, st);
                if (e != hipSuccess) return e;
            }
            return hipSuccess;
        };
        EGX_HIP_CHECK(back(diag->mean, h->emean.p, h->mean.p, 1));
        EGX_HIP_CHECK(back(diag->var, h->evar.p, h->var.p, 1));
        EGX_HIP_CHECK(back(diag->gmean, h->egmean.p, h->gmean.p, (size_t)d));
        EGX_HIP_CHECK(back(diag->gvar, h->egvar.p, h->gvar.p, (size_t)d));
        if (diag_mix && diag->probas)
            EGX_HIP_CHECK(hipMemcpyAsync(diag->probas, h->dg_probas.p, sizeof(double) * (size_t)m * dsg->k, hipMemcpyDeviceToHost, st));
        if (diag_mix && diag->dprobas)
            EGX_HIP_CHECK(hipMemcpyAsync(diag->dprobas, h->dg_dprobas.p, sizeof(double) * (size_t)m * dsg->k * d,
                                         hipMemcpyDeviceToHost, st));
    }
    EGX_HIP_CHECK(hipStreamSynchronize(st));
    if (diag && !diag_mix) {  // one cluster: the responsibilities are ones (gaussian_mixture.rs:115-116)
        if (diag->probas) std::fill(diag->probas, diag->probas + m, 1.0);
        if (diag->dprobas) std::fill(diag->dprobas, diag->dprobas + (size_t)m * d, 0.0);
    }
    return EGX_SUCCESS;
}

int eval_guarded(egx_infill *h, const double *xq, int64_t m, double *value, double *grad, const egx_infill_parts *parts,
                 const ExpertDiag *diag = nullptr, const CstrOut *co = nullptr) {
    const int rc = eval_locked(h, xq, m, value, grad, parts, diag, co);
    if (rc) {  // nothing may still run on the handle's buffers
        (void)hipStreamSynchronize(h->models[0].stream());
        (void)hipGetLastError();
    }
    return rc;
}

bool params_ok(double fmin, double sigma_weight, double scale_ic, double scale) {
    if (std::isnan(fmin) || !(sigma_weight > 0.0) || std::isnan(scale_ic) || !(scale > 0.0) || std::isinf(scale)) {
        set_error("infill: fmin and scale_ic must not be NaN, sigma_weight and scale must be positive and finite");
        return false;
    }
    return true;
}

int config_ok(const egx_infill_config &cfg) {
    if (cfg.criterion < EGX_INFILL_EI || cfg.criterion > EGX_INFILL_WB2S) {
        set_error("infill: unknown criterion");
        return EGX_ERR_INVALID_VALUE;
    }
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

}  // namespace

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
    if (!out) {
        set_error("out handle pointer is NULL");
        return EGX_ERR_INVALID_VALUE;
    }
    *out = nullptr;
    egx_infill_config cfg;
    if (cfg_in) cfg = *cfg_in; else egx_infill_config_default(&cfg);
    if (!obj_model || n_cstr < 0 || (n_cstr > 0 && (!cstr_models || !cstr_tols))) {
        set_error("infill: NULL model or tolerance array");
        return EGX_ERR_INVALID_VALUE;
    }
    EGX_RC(config_ok(cfg));
    std::unique_ptr<egx_infill> h(new egx_infill);
    h->models.emplace_back(obj_model);
    for (int j = 0; j < n_cstr; j++) {
        if (!cstr_models[j]) {
            set_error("infill: model " + std::to_string(j + 1) + " is NULL");
            return EGX_ERR_INVALID_VALUE;
        }
        if (std::isnan(cstr_tols[j])) {
            set_error("infill: tolerance " + std::to_string(j) + " is NaN");
            return EGX_ERR_INVALID_VALUE;
        }
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

}  // extern "C"

namespace {

// expert e of a surrogate as a ModelRef: egx_infill_create_mix's dense handles, egx_infill_create_any's tagged references
int expert_ref(const egx_infill_surrogate &sv, int e, const std::string &name, ModelRef &out) {
    if (!sv.experts[e]) {
        set_error(name + " expert " + std::to_string(e) + " is NULL");
        return EGX_ERR_INVALID_VALUE;
    }
    out = ModelRef(sv.experts[e]);
    return EGX_SUCCESS;
}
int expert_ref(const egx_infill_surrogate_any &sv, int e, const std::string &name, ModelRef &out) {
    const egx_model_ref &r = sv.experts[e];
    if (r.kind != EGX_MODEL_GP && r.kind != EGX_MODEL_SGP) {
        set_error(name + " expert " + std::to_string(e) + " has the unknown kind " + std::to_string(r.kind) +
                  " (EGX_MODEL_GP or EGX_MODEL_SGP)");
        return EGX_ERR_INVALID_VALUE;
    }
    if (!r.handle) {
        set_error(name + " expert " + std::to_string(e) + " is NULL");
        return EGX_ERR_INVALID_VALUE;
    }
    out = r.kind == EGX_MODEL_SGP ? ModelRef(static_cast<egx_sgp *>(r.handle)) : ModelRef(static_cast<egx_gp *>(r.handle));
    return EGX_SUCCESS;
}

// egx_infill_create_mix and egx_infill_create_any: the same checks in the same order, the same handle
template <class SurrogateView>
int32_t create_from_surrogates(const egx_infill_config *cfg_in, const SurrogateView *surrogates, const double *cstr_tols,
                               int32_t n_cstr, egx_infill **out) {
    if (!out) {
        set_error("out handle pointer is NULL");
        return EGX_ERR_INVALID_VALUE;
    }
    *out = nullptr;
    egx_infill_config cfg;
    if (cfg_in) cfg = *cfg_in; else egx_infill_config_default(&cfg);
    if (!surrogates || n_cstr < 0 || (n_cstr > 0 && !cstr_tols)) {
        set_error("infill: NULL surrogate or tolerance array");
        return EGX_ERR_INVALID_VALUE;
    }
    EGX_RC(config_ok(cfg));
    std::unique_ptr<egx_infill> h(new egx_infill);
    h->mix_api = true;
    for (int j = 0; j <= n_cstr; j++) {
        const SurrogateView &sv = surrogates[j];
        const std::string name = "infill: surrogate " + std::to_string(j);
        if (sv.n_experts < 1 || !sv.experts) {
            set_error(name + " needs at least one expert");
            return EGX_ERR_INVALID_VALUE;
        }
        if (j > 0 && std::isnan(cstr_tols[j - 1])) {
            set_error("infill: tolerance " + std::to_string(j - 1) + " is NaN");
            return EGX_ERR_INVALID_VALUE;
        }
        h->surr.emplace_back();
        Surrogate &sg = h->surr.back();
        sg.first = (int)h->models.size(), sg.k = sv.n_experts, sg.smooth = sv.smooth != 0;
        for (int e = 0; e < sv.n_experts; e++) {
            ModelRef ref;
            EGX_RC(expert_ref(sv, e, name, ref));
            h->models.push_back(ref);
        }
        if (j > 0) h->tol.push_back(cstr_tols[j - 1]);
        if (sg.k < 2) continue;  // one cluster: the responsibilities are ones, the mixture is not read
        if (!sv.weights || !sv.means || !sv.precisions_chol) {
            set_error(name + ": NULL weights, means or precisions_chol");
            return EGX_ERR_INVALID_VALUE;
        }
        if (!(sv.heaviside_factor > 0.0) || std::isinf(sv.heaviside_factor)) {
            set_error(name + ": heaviside_factor must be positive and finite");
            return EGX_ERR_INVALID_VALUE;
        }
        const int64_t kk = sg.k, d = h->models[sg.first].d();  // (the first read of a model: the pointer checks are done)
        bool finite = true, positive = true;
        for (int64_t i = 0; i < kk; i++) finite &= std::isfinite(sv.weights[i]), positive &= sv.weights[i] > 0.0;
        for (int64_t i = 0; i < kk * d; i++) finite &= std::isfinite(sv.means[i]);
        for (int64_t i = 0; i < kk * d * d; i++) finite &= std::isfinite(sv.precisions_chol[i]);
        if (!finite) {
            set_error(name + ": non-finite weight, mean or precision factor");
            return EGX_ERR_INVALID_VALUE;
        }
        if (!positive) {
            set_error(name + ": weights must be positive");
            return EGX_ERR_INVALID_VALUE;
        }
        if (infill_mix_lds_bytes((int)d, (int)kk) > kInfillMixMaxLds) {
            set_error(name + ": 3 (d | 1) + 2 (k | 1) exceeds 320 doubles of LDS scratch per point (d " + std::to_string(d) + ", k " +
                      std::to_string(kk) + ")");
            return EGX_ERR_UNSUPPORTED;
        }
        sg.gmx = gmx_pack(sv.weights, sv.means, sv.precisions_chol, kk, d, sv.heaviside_factor);
        for (int64_t c = 0; c < kk; c++)
            if (!std::isfinite(sg.gmx[(size_t)(kk * d + kk * d * d + c)])) {
                set_error(name + ": cluster " + std::to_string(c) + " has no positive diagonal in its precision factor");
                return EGX_ERR_INVALID_VALUE;
            }
        sg.eslot = h->n_eslots;
        h->n_eslots += sg.k;
        h->k_max = std::max(h->k_max, sg.k);
    }
    EGX_RC(finish_create(h.get(), cfg));
    *out = h.release();
    return EGX_SUCCESS;
}

}  // namespace

extern "C" {

int32_t egx_infill_create_mix(const egx_infill_config *cfg, const egx_infill_surrogate *surrogates, const double *cstr_tols,
                              int32_t n_cstr, egx_infill **out) {
    return create_from_surrogates(cfg, surrogates, cstr_tols, n_cstr, out);
}

int32_t egx_infill_create_any(const egx_infill_config *cfg, const egx_infill_surrogate_any *surrogates, const double *cstr_tols,
                              int32_t n_cstr, egx_infill **out) {
    return create_from_surrogates(cfg, surrogates, cstr_tols, n_cstr, out);
}

int32_t egx_infill_eval_experts(egx_infill *h, int32_t j, const double *xq, int64_t m, double *mean, double *var, double *grad_mean,
                                double *grad_var, double *probas, double *dprobas) {
    if (!h) {
        set_error("NULL handle");
        return EGX_ERR_INVALID_VALUE;
    }
    if (j < 0 || j >= (int32_t)h->surr.size()) {
        set_error("infill: surrogate " + std::to_string(j) + " out of range");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    ModelLocks locks(h);
    ExpertDiag dg;
    dg.j = j, dg.mean = mean, dg.var = var, dg.gmean = grad_mean, dg.gvar = grad_var, dg.probas = probas, dg.dprobas = dprobas;
    return eval_guarded(h, xq, m, nullptr, nullptr, nullptr, &dg);
}

void egx_infill_destroy(egx_infill *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

int32_t egx_infill_set_params(egx_infill *h, double fmin, double sigma_weight, double scale_ic, double scale, int32_t feasibility) {
    if (!h) {
        set_error("NULL handle");
        return EGX_ERR_INVALID_VALUE;
    }
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
    if (!h || !cfg) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    cfg->criterion = h->prm.kind;
    cfg->feasibility = h->prm.feasibility;
    cfg->fmin = h->prm.fmin;
    cfg->sigma_weight = h->prm.sigma_weight;
    cfg->scale_ic = h->prm.scale_ic;
    cfg->scale = h->prm.scale;
    return EGX_SUCCESS;
}

int32_t egx_infill_eval(egx_infill *h, const double *xq, int64_t m, double *value, double *grad, const egx_infill_parts *parts) {
    if (!h || (m > 0 && !value)) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    ModelLocks locks(h);
    return eval_guarded(h, xq, m, value, grad, parts);
}

int32_t egx_infill_scaling(egx_infill *h, const double *pts, int64_t npts, double *scale_ic_out, double *scale_out,
                           double *scale_cstr) {
    if (!h || npts < 1 || !pts) {
        set_error("infill scaling: needs a handle and at least one point");
        return EGX_ERR_INVALID_VALUE;
    }
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
    const int64_t M = round_up(npts, kTile);
    const int *flag = reinterpret_cast<const int *>(h->flag.p);
    EGX_RC(h->value.alloc((size_t)2 * M));  // [0, M): ei, then base; [M, 2M): fac
    infill::Params prm = h->prm;
    prm.scale = 1.0;
    prm.feasibility = 1;
    std::vector<double> base((size_t)npts), fac((size_t)npts);
    auto fail = [&](int rc) {
        (void)hipStreamSynchronize(st);
        (void)hipGetLastError();
        return rc;
    };
    double scale_ic = 1.0;
    if (prm.kind == infill::kWB2S) {  // compute_wb2s_scale, criteria/wb2.rs:67-88 (argmax: the first maximum)
        int rc = launch_infill_scale_terms(st, prm, k, npts, M, h->mean.p, h->var.p, h->d_tol.p, flag, h->value.p, nullptr, nullptr);
        if (rc) return fail(rc);
        if (hipMemcpyAsync(base.data(), h->value.p, sizeof(double) * (size_t)npts, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            set_error("infill scaling: copying the EI values back failed");
            return fail(EGX_ERR_HIP);
        }
        int64_t i_max = 0;
        for (int64_t i = 1; i < npts; i++)
            if (base[i] > base[i_max] || std::isnan(base[i_max])) i_max = i;
        if (std::fabs(base[i_max]) > 100.0 * infill::kEps) scale_ic = 100.0 * std::fabs(mean[i_max]) / base[i_max];
    }
    prm.scale_ic = scale_ic;
    {
        int rc = launch_infill_scale_terms(st, prm, k, npts, M, h->mean.p, h->var.p, h->d_tol.p, flag, nullptr, h->value.p,
                                           h->value.p + M);
        if (rc) return fail(rc);
        if (hipMemcpyAsync(base.data(), h->value.p, sizeof(double) * (size_t)npts, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(fac.data(), h->value.p + M, sizeof(double) * (size_t)npts, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            set_error("infill scaling: copying the criterion's terms back failed");
            return fail(EGX_ERR_HIP);
        }
    }
    double scale = 0.0;  // compute_infill_obj_scale, solver_computations.rs:297-351
    for (int64_t i = 0; i < npts; i++) {
        double v = base[i];
        if (std::isnan(v) || std::isinf(v)) v = 1.0;
        if (k > 0) v = (prm.kind == infill::kLogEI) ? v - fac[i] : v * fac[i];
        scale = std::fmax(scale, std::fabs(v));
    }
    if (scale < 100.0 * infill::kEps || std::isnan(scale) || std::isinf(scale)) scale = 1.0;
    if (scale_cstr || !folded)  // compute_cstr_scales, utils/misc.rs:10-28
        for (int j = 1; j <= n_cstr; j++) {
            double best = -1.0;
            for (int64_t i = 0; i < npts; i++) {
                const double v = mean[(size_t)j * npts + i];
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
    h->prm.scale_ic = scale_ic;
    h->prm.scale = scale;
    if (scale_ic_out) *scale_ic_out = scale_ic;
    if (scale_out) *scale_out = scale;
    return EGX_SUCCESS;
}

int32_t egx_infill_set_cstr_strategy(egx_infill *h, int32_t strategy, const double *scale_cstr) {
    if (!h) {
        set_error("NULL handle");
        return EGX_ERR_INVALID_VALUE;
    }
    if (strategy < EGX_CSTR_INFILL || strategy > EGX_CSTR_UTB) {
        set_error("infill: unknown constraint strategy");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    const size_t k = h->surr.size() - 1;
    if (scale_cstr) {
        for (size_t j = 0; j < k; j++)
            if (!(scale_cstr[j] > 0.0) || std::isinf(scale_cstr[j])) {
                set_error("infill: scale_cstr " + std::to_string(j) + " must be positive and finite");
                return EGX_ERR_INVALID_VALUE;
            }
        h->scale_cstr.assign(scale_cstr, scale_cstr + k);
        h->scale_on_device = false;
    }
    h->strategy = strategy;
    return EGX_SUCCESS;
}

int32_t egx_infill_get_cstr_strategy(egx_infill *h, int32_t *strategy, double *scale_cstr) {
    if (!h || !strategy) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    *strategy = h->strategy;
    if (scale_cstr) std::copy(h->scale_cstr.begin(), h->scale_cstr.end(), scale_cstr);
    return EGX_SUCCESS;
}

int32_t egx_infill_eval_cstr(egx_infill *h, const double *xq, int64_t m, double *value, double *cstr, double *grad,
                             double *grad_cstr) {
    if (!h || (m > 0 && !value) || (m > 0 && h->surr.size() > 1 && !cstr)) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    if (h->strategy == infill::kCstrInfill) {
        set_error("infill: the handle folds its constraints into the objective (EGX_CSTR_INFILL); set EGX_CSTR_MEAN or EGX_CSTR_UTB");
        return EGX_ERR_INVALID_VALUE;
    }
    ModelLocks locks(h);
    CstrOut co;
    co.cstr = cstr, co.gcstr = grad_cstr;
    return eval_guarded(h, xq, m, value, grad, nullptr, nullptr, &co);
}

int32_t egx_infill_optimize_cstr(egx_infill *h, const double *lo, const double *hi, const double *x_start, int64_t n_start,
                                 int64_t max_eval, double *f_best, double *x_best, double *c_best, egx_infill_cstr_stats *stats) {
    if (!h || !lo || !hi || !x_start || !f_best || !x_best || n_start < 1 || (h->surr.size() > 1 && !c_best)) {
        set_error("infill optimize: NULL argument or no start point");
        return EGX_ERR_INVALID_VALUE;
    }
    const int d = h->d, k = (int)h->surr.size() - 1;
    for (int i = 0; i < d; i++)
        if (!(lo[i] <= hi[i]) || std::isinf(lo[i]) || std::isinf(hi[i])) {
            set_error("infill optimize: bounds must be finite with lo <= hi (coordinate " + std::to_string(i) + ")");
            return EGX_ERR_INVALID_VALUE;
        }
    for (int64_t s = 0; s < n_start; s++)
        for (int i = 0; i < d; i++)
            if (!std::isfinite(x_start[s * d + i])) {
                set_error("infill optimize: start point " + std::to_string(s) + " has a non-finite coordinate");
                return EGX_ERR_INVALID_VALUE;
            }
    std::lock_guard<std::mutex> lock(h->mu);
    if (h->strategy == infill::kCstrInfill) {
        set_error("infill optimize: the handle folds its constraints into the objective (EGX_CSTR_INFILL); use egx_infill_optimize");
        return EGX_ERR_INVALID_VALUE;
    }
    ModelLocks locks(h);
    // one general-constraint COBYLA per start, configured as egx_infill_optimize's (optimizer.rs:123-167: no constraint
    // tolerances; solver_infill_optim.rs:217-227)
    if (max_eval <= 0) max_eval = std::min<int64_t>(10 * n_start * d, 2000);
    const std::vector<double> blo(lo, lo + d), bhi(hi, hi + d);
    // a point is FEASIBLE when c_j <= cstr_tol_j / scale_cstr_j: Egor's acceptance tolerance in the units of c
    std::vector<double> cfeas((size_t)k);
    for (int j = 0; j < k; j++) cfeas[j] = h->tol[j] / h->scale_cstr[j];
    std::vector<Cobyla> mach;
    mach.reserve((size_t)n_start);
    for (int64_t s = 0; s < n_start; s++)
        mach.emplace_back(std::vector<double>(x_start + s * d, x_start + (s + 1) * d), blo, bhi, k, 0.5, 1e-4, 1e-4, max_eval, 0.0, true,
                          true, cfeas);
    std::vector<double> pts, vals, cvals, x;
    std::vector<size_t> who;
    int64_t rounds = 0;
    // all starts in LOCK-STEP: a round's trial points are ONE values-only egx_infill_eval_cstr
    for (;;) {
        pts.clear();
        who.clear();
        for (size_t q = 0; q < mach.size(); q++)
            if (mach[q].ask(x)) {
                who.push_back(q);
                pts.insert(pts.end(), x.begin(), x.end());
            }
        if (who.empty()) break;
        vals.assign(who.size(), 0.0);
        cvals.assign(who.size() * (size_t)k + 1, 0.0);
        CstrOut co;
        co.cstr = k > 0 ? cvals.data() : nullptr;
        EGX_RC(eval_guarded(h, pts.data(), (int64_t)who.size(), vals.data(), nullptr, nullptr, nullptr, &co));
        rounds++;
        for (size_t q = 0; q < who.size(); q++) mach[who[q]].tell(vals[q], cvals.data() + q * (size_t)k);
    }
    // The best EVALUATED point: feasible beats infeasible, then the smaller objective (feasible) or the smaller violation
    // max_j (c_j - cstr_tol_j / scale_cstr_j) (infeasible); the first point of a start and the first start win ties.  The
    // reference returns every run's final vertex and takes the smallest objective, feasible or not (:229-232).
    auto better = [&](const Cobyla &a, const Cobyla &b) {  // a strictly better than b
        if (a.best_feasible() != b.best_feasible()) return a.best_feasible();
        return a.best_feasible() ? a.best_key() < b.best_key() : a.best_violation() < b.best_violation();
    };
    int64_t best = 0;
    for (int64_t s = 1; s < n_start; s++)
        if (better(mach[(size_t)s], mach[(size_t)best])) best = s;
    const Cobyla &win = mach[(size_t)best];
    *f_best = win.best_f();
    std::copy(win.best_x().begin(), win.best_x().end(), x_best);
    if (k > 0) std::copy(win.best_c().begin(), win.best_c().end(), c_best);
    if (stats) {
        stats->rounds = rounds;
        stats->best_start = best;
        stats->feasible = win.best_feasible() ? 1 : 0;
        stats->violation = k > 0 ? win.best_violation() : 0.0;
        if (stats->evals)
            for (int64_t s = 0; s < n_start; s++) stats->evals[s] = mach[(size_t)s].evals();
    }
    bool any_finite = false;
    for (const Cobyla &c : mach) any_finite |= c.any_finite_f();
    if (!any_finite) {
        *f_best = std::numeric_limits<double>::infinity();
        set_error("infill optimize: no start met a finite objective value");
        return EGX_ERR_NO_FINITE_START;
    }
    return EGX_SUCCESS;
}

int32_t egx_infill_optimize_slsqp(egx_infill *h, const double *lo, const double *hi, const double *x_start, int64_t n_start,
                                  int64_t max_eval, double *f_best, double *x_best, double *c_best, egx_infill_slsqp_stats *stats) {
    if (!h || !lo || !hi || !x_start || !f_best || !x_best || n_start < 1) {
        set_error("infill optimize: NULL argument or no start point");
        return EGX_ERR_INVALID_VALUE;
    }
    const int d = h->d;
    for (int i = 0; i < d; i++)
        if (!(lo[i] <= hi[i]) || std::isinf(lo[i]) || std::isinf(hi[i])) {
            set_error("infill optimize: bounds must be finite with lo <= hi (coordinate " + std::to_string(i) + ")");
            return EGX_ERR_INVALID_VALUE;
        }
    for (int64_t s = 0; s < n_start; s++)
        for (int i = 0; i < d; i++)
            if (!std::isfinite(x_start[s * d + i])) {
                set_error("infill optimize: start point " + std::to_string(s) + " has a non-finite coordinate");
                return EGX_ERR_INVALID_VALUE;
            }
    std::lock_guard<std::mutex> lock(h->mu);
    // EGX_CSTR_INFILL: the constraint models are inside the objective, the machines see none
    const int k = h->strategy == infill::kCstrInfill ? 0 : (int)h->surr.size() - 1;
    if (k > 0 && !c_best) {
        set_error("infill optimize: NULL argument or no start point");
        return EGX_ERR_INVALID_VALUE;
    }
    ModelLocks locks(h);
    // one SLSQP per start: ftol_rel = ftol_abs = 1e-4, at most min(10 n_start d, 2000) evaluations each
    // (solver_infill_optim.rs:217-227).  The machine is told c_j as evaluated and solves c_j <= cstr_tol_j / scale_cstr_j: the
    // constraint c_j - cstr_tol_j / scale_cstr_j <= 0 that optimizer.rs:188-199 hands to slsqp::minimize.
    if (max_eval <= 0) max_eval = std::min<int64_t>(10 * n_start * d, 2000);
    const std::vector<double> blo(lo, lo + d), bhi(hi, hi + d);
    std::vector<double> cfeas((size_t)k);
    for (int j = 0; j < k; j++) cfeas[j] = h->tol[j] / h->scale_cstr[j];
    std::vector<Slsqp> mach;
    mach.reserve((size_t)n_start);
    for (int64_t s = 0; s < n_start; s++)
        mach.emplace_back(std::vector<double>(x_start + s * d, x_start + (s + 1) * d), blo, bhi, k, 1e-4, 1e-4, max_eval, cfeas);
    std::vector<double> pts, vals, grads, cvals, cgrads, x;
    std::vector<size_t> who;
    int64_t rounds = 0;
    // all starts in LOCK-STEP: a round's points, line-search trial points included, are ONE evaluation with gradients
    for (;;) {
        pts.clear();
        who.clear();
        bool want_grad = true;
        for (size_t q = 0; q < mach.size(); q++)
            if (mach[q].ask(x, want_grad)) {
                who.push_back(q);
                pts.insert(pts.end(), x.begin(), x.end());
            }
        if (who.empty()) break;
        const size_t m = who.size();
        vals.assign(m, 0.0);
        grads.assign(m * d, 0.0);
        cvals.assign(m * (size_t)k + 1, 0.0);
        cgrads.assign(m * (size_t)k * d + 1, 0.0);
        if (h->strategy == infill::kCstrInfill) {
            EGX_RC(eval_guarded(h, pts.data(), (int64_t)m, vals.data(), grads.data(), nullptr));
        } else {
            CstrOut co;
            co.cstr = k > 0 ? cvals.data() : nullptr, co.gcstr = k > 0 ? cgrads.data() : nullptr;
            EGX_RC(eval_guarded(h, pts.data(), (int64_t)m, vals.data(), grads.data(), nullptr, nullptr, &co));
        }
        rounds++;
        for (size_t q = 0; q < m; q++)
            mach[who[q]].tell(vals[q], cvals.data() + q * (size_t)k, grads.data() + q * d, cgrads.data() + q * (size_t)k * d);
    }
    // the best EVALUATED point, in egx_infill_optimize_cstr's ordering
    auto better = [&](const Slsqp &a, const Slsqp &b) {  // a strictly better than b
        if (a.best_feasible() != b.best_feasible()) return a.best_feasible();
        return a.best_feasible() ? a.best_key() < b.best_key() : a.best_violation() < b.best_violation();
    };
    bool any_finite = false;
    for (const Slsqp &c : mach) any_finite |= c.any_finite_f();
    int64_t best = 0;  // nothing finite anywhere: start 0, whose only point is the start clamped into the box
    for (int64_t s = 1; s < n_start && any_finite; s++)
        if (better(mach[(size_t)s], mach[(size_t)best])) best = s;
    const Slsqp &win = mach[(size_t)best];
    *f_best = win.best_f();
    std::copy(win.best_x().begin(), win.best_x().end(), x_best);
    if (k > 0) std::copy(win.best_c().begin(), win.best_c().end(), c_best);
    if (stats) {
        stats->rounds = rounds;
        stats->best_start = best;
        stats->feasible = win.best_feasible() ? 1 : 0;
        stats->violation = k > 0 ? win.best_violation() : 0.0;
        for (int64_t s = 0; s < n_start; s++) {
            if (stats->evals) stats->evals[s] = mach[(size_t)s].evals();
            if (stats->stop) stats->stop[s] = (int32_t)mach[(size_t)s].status();
        }
    }
    if (!any_finite) {
        *f_best = std::numeric_limits<double>::infinity();
        set_error("infill optimize: no start met a finite objective value");
        return EGX_ERR_NO_FINITE_START;
    }
    return EGX_SUCCESS;
}

int32_t egx_infill_optimize(egx_infill *h, const double *lo, const double *hi, const double *x_start, int64_t n_start,
                            int64_t max_eval, double *f_best, double *x_best, egx_infill_stats *stats) {
    if (!h || !lo || !hi || !x_start || !f_best || !x_best || n_start < 1) {
        set_error("infill optimize: NULL argument or no start point");
        return EGX_ERR_INVALID_VALUE;
    }
    const int d = h->d;
    for (int i = 0; i < d; i++)
        if (!(lo[i] <= hi[i]) || std::isinf(lo[i]) || std::isinf(hi[i])) {
            set_error("infill optimize: bounds must be finite with lo <= hi (coordinate " + std::to_string(i) + ")");
            return EGX_ERR_INVALID_VALUE;
        }
    for (int64_t s = 0; s < n_start; s++)
        for (int i = 0; i < d; i++)
            if (!std::isfinite(x_start[s * d + i])) {
                set_error("infill optimize: start point " + std::to_string(s) + " has a non-finite coordinate");
                return EGX_ERR_INVALID_VALUE;
            }
    std::lock_guard<std::mutex> lock(h->mu);
    ModelLocks locks(h);
    // one COBYLA per start: rhobeg 0.5, ftol_rel = ftol_abs = 1e-4 (crates/ego/src/optimizers/optimizer.rs:155-167,
    // solver_infill_optim.rs:222-227), at most min(10 n_start d, 2000) evaluations each (:217-221)
    if (max_eval <= 0) max_eval = std::min<int64_t>(10 * n_start * d, 2000);
    const std::vector<double> blo(lo, lo + d), bhi(hi, hi + d);
    std::vector<CobylaBox> mach;
    mach.reserve((size_t)n_start);
    for (int64_t s = 0; s < n_start; s++)
        mach.emplace_back(std::vector<double>(x_start + s * d, x_start + (s + 1) * d), blo, bhi, 0.5, 1e-4, max_eval, 0.0, true, true,
                          1e-4);
    // The best EVALUATED point of every start (the first on ties), kept here and not taken from CobylaBox::best_x(): that is
    // the pole of the final simplex, re-assembled by additions each time the pole moves, so it need not be bit for bit a point
    // that was evaluated -- and "f_best is egx_infill_eval at x_best" is part of this call's contract.
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> fb((size_t)n_start, inf), xb((size_t)n_start * d, 0.0);
    for (int64_t s = 0; s < n_start; s++)
        for (int i = 0; i < d; i++) xb[s * d + i] = std::fmin(hi[i], std::fmax(lo[i], x_start[s * d + i]));
    std::vector<double> pts, vals, x;
    std::vector<size_t> who;
    int64_t rounds = 0;
    // all starts in LOCK-STEP: a round's trial points are ONE values-only evaluation
    for (;;) {
        pts.clear();
        who.clear();
        for (size_t q = 0; q < mach.size(); q++)
            if (mach[q].ask(x)) {
                who.push_back(q);
                pts.insert(pts.end(), x.begin(), x.end());
            }
        if (who.empty()) break;
        vals.assign(who.size(), 0.0);
        EGX_RC(eval_guarded(h, pts.data(), (int64_t)who.size(), vals.data(), nullptr, nullptr));
        rounds++;
        for (size_t q = 0; q < who.size(); q++) {
            const size_t s = who[q];
            const double v = vals[q];
            if (v == v && v < 1e30 && v < fb[s]) {  // beyond COBYLA's barrier a value counts as +inf (optimizer.rs:153-157 style)
                fb[s] = v;
                std::copy(pts.begin() + q * d, pts.begin() + (q + 1) * d, xb.begin() + s * d);
            }
            mach[s].tell(v);
        }
    }
    int64_t best = 0;
    for (int64_t s = 1; s < n_start; s++)
        if (fb[s] < fb[best]) best = s;  // the first wins ties (solver_infill_optim.rs:229-236)
    *f_best = fb[best];
    std::copy(xb.begin() + best * d, xb.begin() + (best + 1) * d, x_best);
    if (stats) {
        stats->rounds = rounds;
        stats->best_start = best;
        if (stats->evals)
            for (int64_t s = 0; s < n_start; s++) stats->evals[s] = mach[(size_t)s].evals();
    }
    if (!std::isfinite(fb[best])) {
        set_error("infill optimize: no start ended at a finite value");
        return EGX_ERR_NO_FINITE_START;
    }
    return EGX_SUCCESS;
}

}  // extern "C"
