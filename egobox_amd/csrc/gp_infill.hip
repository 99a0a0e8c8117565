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
//
// PENDING POINTS (egx_infill_push_pending; the q_points loop of solver_impl.rs:622-791).  The handle keeps up to 16 virtual
// observations and conditions every (lone, dense) surrogate on them in closed form (pending_math.h) instead of refitting it:
// right after expert_tile / expert_tile_mean, while h->xqT still holds the model's normalised tile, k_pending_cross contracts
// the tile against the model's training points followed by the pending ones with the extended weight matrix W^ = [W_v ; I_q]
// and k_pending_finish rewrites the tile's mean / var / gmean / gvar in place (kernels_pending.hip) -- nothing downstream
// changes.  A push runs the new point's own sequence once (a tile holding one point) WITHOUT the conditioning, keeps the
// weight column posterior_weights / posterior_weights_trend made for it and its -dneg as column q of W^ / t_q, takes its
// covariances with the points already pending from the same two kernels, and borders chol(S), alpha and sigma2' on the host.
// With q = 0 none of this runs: the launch sequence is the one above, bit for bit.
#include <map>

#include "gmx_point.h"
#include "sgp_handle.h"
#include "infill_math.h"
#include "pending_math.h"
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

// A lone dense surrogate conditioned on the handle's q pending points (pending_math.h): the points after the model's training
// points in ITS normalisation, the extended weight matrix W^ = [W_v ; I_q], the trend columns t_v, chol(S) and alpha (host
// and device), the conditioned process variance.  Valid for ONE fitted state of the model (epoch).
struct PendModel {
    DevBuf ZT, W, tv, small;  // d x ldz | (n + 16) x 16 | 16 x p | L (16 x 16) and alpha (16)
    DevBuf Wc;                // W^ column-major (16 x ldz): the weight vectors of the composed form
    int64_t ldz = 0;
    int n = -1;
    uint64_t epoch = 0;
    double sigma2c = 0.0;
    std::vector<double> L = std::vector<double>((size_t)pending::kLd * pending::kLd, 0.0);
    std::vector<double> alpha = std::vector<double>(pending::kMaxPending, 0.0), delta = alpha;
};

// a push: the new point runs the models' own sequences WITHOUT the conditioning; its cross-covariances with the points already
// pending come back in emit (surrogate-major, kTile x 16 each; the point is row 0), its weights are captured as column q
struct PushCapture {
    DevBuf emit;
};

}  // namespace

namespace egx {
std::atomic<int> g_pending_composed{0};
}

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
    // the pending points of a q-point batch (egx_infill_push_pending): q of them, as stored (cast raw x, q x d; raw y, q x n_surr),
    // every surrogate's conditioning state, the partial sums of one (tile, model) step of k_pending_cross
    int q = 0;
    std::vector<double> pend_x, pend_y;
    std::vector<PendModel> pend;
    DevBuf pc_c, pc_g;
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

// the fused contraction where it applies, unless the composed form is asked for (egx_set_tuning "pending_composed")
bool pending_composed(int d) { return d > kPendingMaxD || g_pending_composed.load() != 0; }

// Right after expert_tile / expert_tile_mean of the lone dense surrogate js, while h->xqT holds its normalised tile: the tile's
// entries of the tables conditioned IN PLACE on the pending points (var / gvar nullptr: the mean shift alone).  A push (cap)
// rewrites nothing: it takes the tile's cross-covariances with the points already pending, then captures query 0's weights.
int pending_tile(egx_infill *h, hipStream_t st, int js, bool want_g, double *mean, double *var, double *gmean, double *gvar,
                 PushCapture *cap) {
    const int d = h->d;
    PendModel &pm = h->pend[js];
    const egx_gp *gp = h->models[h->surr[js].first].gp;
    if (h->q > 0) {
        const int nz = gp->n + h->q;
        const bool g = want_g && !cap;
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
            f.mean = mean, f.var = var, f.gmean = g ? gmean : nullptr, f.gvar = g ? gvar : nullptr;
        }
        EGX_RC(launch_pending_finish(st, f));
    }
    if (cap)
        EGX_RC(launch_pending_capture(st, h->Wt.p, h->dneg.p, h->xqT.p, gp->n, d, gp->p, h->q, pm.W.p, pm.Wc.p, pm.tv.p, pm.ZT.p,
                                      pm.ldz));
    return EGX_SUCCESS;
}

// pending points belong to one fitted state of every model
int check_pending(const egx_infill *h) {
    for (size_t js = 0; js < h->pend.size() && h->q > 0; js++) {
        const egx_gp *gp = h->models[h->surr[js].first].gp;
        if (gp->fit_epoch != h->pend[js].epoch || gp->n != h->pend[js].n) {
            set_error("infill: " + who(h, h->surr[js].first) + " was refitted since its pending points were pushed (call "
                      "egx_infill_clear_pending)");
            return EGX_ERR_INVALID_VALUE;
        }
    }
    return EGX_SUCCESS;
}

// what egx_infill_eval_cstr asks for beside value / grad (host pointers, any nullptr)
struct CstrOut {
    double *cstr = nullptr, *gcstr = nullptr;
};

// The evaluation proper; the handle's and the models' locks are held.  value / grad / every member of parts may be nullptr.
int eval_locked(egx_infill *h, const double *xq, int64_t m, double *value, double *grad, const egx_infill_parts *parts,
                const ExpertDiag *diag = nullptr, const CstrOut *co = nullptr, PushCapture *cap = nullptr) {
    if (m < 0 || (m > 0 && !xq)) {
        set_error("bad query array");
        return EGX_ERR_INVALID_VALUE;
    }
    const int ne = (int)h->models.size(), nm = (int)h->surr.size(), k = nm - 1, d = h->d;
    EGX_RC(check_fitted(h));
    EGX_RC(check_specs(h));
    EGX_RC(check_pending(h));
    if (m == 0) return EGX_SUCCESS;
    const bool pending = h->q > 0 || cap;  // (q = 0 and no push: nothing below differs from a handle without pending points)
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
    if (pending && h->q > 0) {
        int ns_p = 1;  // the larger of the fused form's splits and the composed form's (per column: mean_splits, xgrad_splits)
        for (int js = 0; js < nm; js++) {
            const int nz = h->models[h->surr[js].first].gp->n + h->q;
            ns_p = std::max(ns_p, std::max(pending_splits(nz), std::max(mean_splits((int)h->pend[js].ldz, kTile), xgrad_splits(nz, kTile))));
        }
        EGX_RC(h->pc_c.alloc((size_t)ns_p * kTile * pending::kLd));
        if (want_g && !cap) EGX_RC(h->pc_g.alloc((size_t)ns_p * kTile * pending::kLd * d));
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
                    if (pending)
                        EGX_RC(pending_tile(h, st, js, want_g, h->mean.p + row, nullptr, want_g ? h->gmean.p + row * d : nullptr, nullptr,
                                            cap));
                    continue;
                }
                EGX_RC((sparse ? sgp_expert_tile : expert_tile)(
                    h, st, sg.first + e, t0, mt, want_g, (lone ? h->mean.p : h->emean.p) + row, (lone ? h->var.p : h->evar.p) + row,
                    want_g ? (lone ? h->gmean.p : h->egmean.p) + row * d : nullptr,
                    want_g ? (lone ? h->gvar.p : h->egvar.p) + row * d : nullptr, sg.first + e == 0 ? flag + t0 : nullptr));
                if (pending)
                    EGX_RC(pending_tile(h, st, js, want_g, h->mean.p + row, h->var.p + row, want_g ? h->gmean.p + row * d : nullptr,
                                        want_g ? h->gvar.p + row * d : nullptr, cap));
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
                 const ExpertDiag *diag = nullptr, const CstrOut *co = nullptr, PushCapture *cap = nullptr) {
    const int rc = eval_locked(h, xq, m, value, grad, parts, diag, co, cap);
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

namespace {

// every surrogate a lone dense model, d within the contraction's reach
int pending_supported(const egx_infill *h) {
    for (size_t js = 0; js < h->surr.size(); js++) {
        const Surrogate &sg = h->surr[js];
        if (sg.k >= 2 || h->models[sg.first].sparse()) {
            set_error("infill: pending points are not supported on surrogate " + std::to_string(js) +
                      (sg.k >= 2 ? " (a mixture of " + std::to_string(sg.k) + " experts)" : " (a sparse model)"));
            return EGX_ERR_UNSUPPORTED;
        }
    }
    if (h->d > 1024) {  // (the finish keeps 16 d doubles of one point in LDS)
        set_error("infill: pending points need d <= 1024 (d " + std::to_string(h->d) + ")");
        return EGX_ERR_UNSUPPORTED;
    }
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
    if (q >= pending::kMaxPending) {
        set_error("infill: at most " + std::to_string(pending::kMaxPending) + " pending points");
        return EGX_ERR_INVALID_VALUE;
    }
    for (int i = 0; i < d; i++)
        if (!std::isfinite(x[i])) {
            set_error("infill: pending point has a non-finite coordinate " + std::to_string(i));
            return EGX_ERR_INVALID_VALUE;
        }
    for (int j = 0; j < nm; j++)
        if (!std::isfinite(y[j])) {
            set_error("infill: pending point has a non-finite value for surrogate " + std::to_string(j));
            return EGX_ERR_INVALID_VALUE;
        }
    EGX_HIP_CHECK(hipSetDevice(h->device));
    hipStream_t st = h->models[0].stream();
    std::vector<double> xc((size_t)d);
    for (int i = 0; i < d; i++) xc[i] = query_coord(h->models[0].gp, x, i);
    if (q == 0) {
        const int rc = pending_begin(h, st);
        if (rc) {
            (void)hipStreamSynchronize(st);
            (void)hipGetLastError();
            return rc;
        }
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
        if (!pending::chol_border(Ln[js].data(), q, c.data() + (size_t)js * pending::kLd, unit + gp->nugget)) {
            set_error("infill: pending point " + std::to_string(q) + ": the covariance of the pending points is not positive "
                      "definite for surrogate " + std::to_string(js) + " (a point pushed twice, or on a training point)");
            return EGX_ERR_LINALG;
        }
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
    if (!h || !x || !y) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    ModelLocks locks(h);
    return push_locked(h, x, y);
}

int32_t egx_infill_clear_pending(egx_infill *h) {
    if (!h) {
        set_error("NULL handle");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    h->q = 0;
    h->pend_x.clear();
    h->pend_y.clear();
    return EGX_SUCCESS;
}

int32_t egx_infill_get_pending(egx_infill *h, int32_t *q, double *x, double *y, double *sigma2) {
    if (!h || !q) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
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
    if (!h || !y || (strategy != EGX_QEI_CL_MIN && !x)) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    if (strategy < EGX_QEI_KB || strategy > EGX_QEI_CL_MIN) {
        set_error("infill: unknown q-EI strategy");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    ModelLocks locks(h);
    const int nm = (int)h->surr.size();
    if (strategy == EGX_QEI_CL_MIN) {  // y_data[[index_min, ic]] (solver_computations.rs:269-275)
        for (int js = 0; js < nm; js++) {
            const Surrogate &sg = h->surr[js];
            if (sg.k >= 2 || h->models[sg.first].sparse()) {
                set_error("infill: the constant-liar minimum needs lone dense models (surrogate " + std::to_string(js) + ")");
                return EGX_ERR_UNSUPPORTED;
            }
            if (h->models[sg.first].gp->n != h->models[0].gp->n) {
                set_error("infill: the constant-liar minimum needs every model on the same rows (surrogate " + std::to_string(js) +
                          " has " + std::to_string(h->models[sg.first].gp->n) + ", the objective " +
                          std::to_string(h->models[0].gp->n) + ")");
                return EGX_ERR_INVALID_VALUE;
            }
        }
        const std::vector<double> &y0 = h->models[0].gp->y_raw;
        size_t imin = 0;
        for (size_t i = 1; i < y0.size(); i++)
            if (y0[i] < y0[imin]) imin = i;
        for (int js = 0; js < nm; js++) y[js] = h->models[h->surr[js].first].gp->y_raw[imin];
        return EGX_SUCCESS;
    }
    for (int i = 0; i < h->d; i++)
        if (!std::isfinite(x[i])) {
            set_error("infill: virtual point at a non-finite coordinate " + std::to_string(i));
            return EGX_ERR_INVALID_VALUE;
        }
    std::vector<double> mean((size_t)nm), var((size_t)nm);
    egx_infill_parts parts{mean.data(), var.data(), nullptr, nullptr};
    EGX_RC(eval_guarded(h, x, 1, nullptr, nullptr, &parts));
    const double conf = strategy == EGX_QEI_KB ? 0.0 : (strategy == EGX_QEI_KB_LB ? -3.0 : 3.0);
    y[0] = mean[0] + conf * std::sqrt(var[0]);
    for (int js = 1; js < nm; js++) y[js] = mean[js];
    return EGX_SUCCESS;
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
    if (!h || !lo || !hi || !x_start || !x_out || !y_virtual || !f_out || !n_found || n_start < 1) {
        set_error("infill batch: NULL argument or no start point");
        return EGX_ERR_INVALID_VALUE;
    }
    egx_infill_batch_config cfg;
    if (cfg_in) cfg = *cfg_in; else egx_infill_batch_config_default(&cfg);
    if (q < 1 || q > EGX_INFILL_MAX_PENDING || cfg.strategy < EGX_QEI_KB || cfg.strategy > EGX_QEI_CL_MIN ||
        (cfg.optimizer != EGX_BATCH_COBYLA && cfg.optimizer != EGX_BATCH_SLSQP) || (cfg.scaling_points && cfg.n_scaling < 1)) {
        set_error("infill batch: q must be 1 .. 16, the strategy an egx_qei_strategy, the optimizer COBYLA or SLSQP");
        return EGX_ERR_INVALID_VALUE;
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
