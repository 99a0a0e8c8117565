// Internal header of the infill translation units (infill_eval.hip: handle, checks, tile sequences, the evaluation and the
// scaling pass; infill_pending.hip: the pending points of a q-point batch; infill_optimize.hip: the lock-step multistarts).
//
// A SURROGATE -- the objective, a constraint -- is one GP or a mixture of k experts with its Gaussian mixture
// (egx_infill_create_mix; GpMixture, crates/moe/src/algorithm.rs); an EXPERT is a dense GP or a SPARSE one
// (egx_infill_create_any: tagged references, mixed freely).  Locks, caches, checks and scratch sizes run over the flat list of
// all experts.
#pragma once
#include <map>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "sgp_handle.h"
#include "infill_active.h"
#include "infill_math.h"
#include "pending_math.h"

namespace egx {

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

// `return fail(EGX_ERR_INVALID_VALUE, "...")`: the error text is set, the code handed back
inline int fail(int rc, const std::string &msg) { set_error(msg); return rc; }

// what egx_infill_eval_experts asks for: the parts of surrogate j's experts and its responsibilities (host pointers, any nullptr)
struct ExpertDiag {
    int j = 0;
    double *mean = nullptr, *var = nullptr, *gmean = nullptr, *gvar = nullptr, *probas = nullptr, *dprobas = nullptr;
};

// what egx_infill_eval_cstr asks for beside value / grad (host pointers, any nullptr)
struct CstrOut {
    double *cstr = nullptr, *gcstr = nullptr;
};

// Where one expert's sequence writes ONE tile: the tile's kTile entries of the table it owns (device pointers).
// var == nullptr: the MEAN-ONLY sequence; gmean == nullptr: no gradients.
struct TileOut {
    double *mean = nullptr, *var = nullptr, *gmean = nullptr, *gvar = nullptr;
};

}  // namespace egx

struct egx_infill {
    std::mutex mu;
    std::vector<egx::ModelRef> models;  // every expert of every surrogate, surrogate by surrogate (borrowed)
    std::vector<egx::Surrogate> surr;   // [0] the objective, then the constraints
    bool mix_api = false;               // created by egx_infill_create_mix: messages name surrogate and expert
    int n_eslots = 0, k_max = 1;
    std::vector<double> tol;            // one per constraint
    egx::infill::Params prm{};
    int d = 0, device = 0;
    egx::DevBuf d_tol;
    bool tol_on_device = false;
    // buffers of a call (grow-only): the whole call's points and results, then the scratch of ONE (tile, model) step
    egx::DevBuf xraw, flag, mean, var, gmean, gvar, value, grad;
    egx::DevBuf xcast;  // models with xtypes and a mixture among the surrogates: the call's CAST raw points (k_infill_prepare_mixint)
    egx::DevBuf xqT, racc, RT, s0, sl, Wt, dneg, out_y, out_v;
    // sparse experts: x_mean = 0 | x_std = 1 (the prepare kernel's parameters for RAW points), |b~|^2 of a tile, the copy of a~
    egx::DevBuf ident, s1, sE;
    bool ident_on_device = false;
    // the experts of the mixtures: their tables (slot-major like mean / var), d p / d x of one tile, the diagnostics of a call
    egx::DevBuf emean, evar, egmean, egvar, dprob, dg_probas, dg_dprobas;
    // how the constraint surrogates enter (infill::CstrStrategy), their scales, the tables of egx_infill_eval_cstr
    int strategy = egx::infill::kCstrInfill;
    std::vector<double> scale_cstr;  // one per constraint, ones until set
    egx::DevBuf d_scale, cstr, gcstr;
    bool scale_on_device = false;
    // the pending points of a q-point batch (egx_infill_push_pending): q of them, as stored (cast raw x, q x d; raw y, q x n_surr),
    // every surrogate's conditioning state, the partial sums of one (tile, model) step of k_pending_cross
    int q = 0;
    std::vector<double> pend_x, pend_y;
    std::vector<egx::PendModel> pend;
    egx::DevBuf pc_c, pc_g;
    // the active coordinates (egx_infill_set_active, infill_active.h): empty = none.  The entry points whose width becomes
    // n_active expand their compact rows into act_x, evaluate full width with use_cols set -- the experts' x-gradient
    // contractions then take the column list d_active -- and gather the listed gradient columns out of act_g / act_gm /
    // act_gv / act_gc.  Every other caller of eval_guarded leaves use_cols clear and launches what it launched before.
    std::vector<int> active;
    std::vector<double> x_base;
    egx::DevMem<int> d_active;
    bool active_on_device = false, use_cols = false;
    std::vector<double> act_x, act_g, act_gm, act_gv, act_gc;
    int width() const { return active.empty() ? d : (int)active.size(); }  // of a trial point
};

namespace egx {

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

// ---- infill_eval.hip ----
// "model j" for a handle of egx_infill_create, "surrogate j expert e" for one of egx_infill_create_mix
std::string infill_who(const egx_infill *h, int idx);
// every expert fitted; every expert with the xtypes of expert 0 of the objective (read from the models at every call)
int check_fitted(const egx_infill *h);
int check_specs(const egx_infill *h);
// The evaluation of m points; the handle's and the models' locks are held.  value / grad / every member of parts may be nullptr.
// When it fails nothing runs on the handle's buffers any more.
int eval_guarded(egx_infill *h, const double *xq, int64_t m, double *value, double *grad, const egx_infill_parts *parts,
                 const ExpertDiag *diag = nullptr, const CstrOut *co = nullptr, PushCapture *cap = nullptr);
// egx_infill_eval / _eval_cstr and the optimisers' rounds: eval_guarded, and while an activity is set the same call on the
// expanded rows with the column-list contractions; xq, grad, the gradient fields of parts and co->gcstr are width() wide
int eval_active(egx_infill *h, const double *xq, int64_t m, double *value, double *grad, const egx_infill_parts *parts,
                const CstrOut *co = nullptr);
// after a failed step on the handle's stream: wait for what was launched, clear the runtime's last error; returns rc
int settle_failed(const egx_infill *h, int rc);

// ---- infill_pending.hip ----
// pending points belong to one fitted state of every model
int check_pending(const egx_infill *h);
// Right after expert_tile of the lone dense surrogate js, while h->xqT holds its normalised tile: the tile's entries conditioned
// IN PLACE on the pending points (o.var nullptr: the mean shift alone); a push (cap) rewrites nothing
int pending_tile(egx_infill *h, hipStream_t st, int js, const TileOut &o, PushCapture *cap);

}  // namespace egx
