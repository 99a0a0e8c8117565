// Internal header shared by the dense-GP host translation units (gp_host.hip: handle, evaluation, state;
// gp_predict.hip: predictions and their x-gradients; gp_fit.hip: optimiser drivers and the theta-gradient).
#pragma once
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <list>
#include <condition_variable>
#include <mutex>
#include <shared_mutex>
#include <thread>
#include <algorithm>
#include <vector>

#include "egx_internal.h"
#include "dev_mem.h"
#include "slot_pipeline.h"
#include "host_math.h"
#include "fit_starts.h"  // StartResult; cobyla.h, lbfgs.h, multistart.h

#define EGX_RC(call)              \
    do {                          \
        int _rc = (call);         \
        if (_rc) return _rc;      \
    } while (0)

namespace egx {

// Streams and events of a workspace.  Plain handles (the launchers take them as they are); WorkspaceHandles below owns them.
struct WorkspaceRaw {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t eval_stream = nullptr;  // the stream the evaluation in flight was enqueued on: the workspace's own, or
                                        // the leader's when it rides in a lock-step group (finish_eval waits on it)
    PotrfLookahead lk;  // look-ahead streams + events (lk.s2 == nullptr: look-ahead off)
    // the stream + events on which C^-T rides along a factorisation (theta-gradient; PotrfInverse, egx_internal.h)
    hipStream_t inv_stream = nullptr;
    hipEvent_t ev_inv_grp = nullptr, ev_inv_done = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    GemmTrace trace;
};
// Move-only owner of the above: the events are destroyed with it, the four streams go to the idle list of their device as a
// set (gp_host.hip; idle: whoever lets a workspace go has synchronised its streams)
struct WorkspaceHandles : WorkspaceRaw {
    WorkspaceHandles() = default;
    WorkspaceHandles(WorkspaceHandles &&o) noexcept : WorkspaceRaw(o) { static_cast<WorkspaceRaw &>(o) = WorkspaceRaw(); }
    WorkspaceHandles &operator=(WorkspaceHandles &&o) noexcept {
        std::swap(static_cast<WorkspaceRaw &>(*this), static_cast<WorkspaceRaw &>(o));
        return *this;
    }
    ~WorkspaceHandles() { release(); }
    void release_streams();
    void release();
};

struct Workspace : WorkspaceHandles {
    // M, dinv and d_info are VIEWS into the handle's slabs (egx_gp::slab_*): consecutive workspaces sit at fixed
    // strides, which is what lets a group of them be factored in lock-step by one launch sequence
    double *M = nullptr;       // (m_tot x ld): correlation matrix / factor + appended RHS rows
    double *dinv = nullptr;    // (n_pad/64) x 64 x 64 inverses of the diagonal tiles
    int *d_info = nullptr;
    DevMem<double> dW;      // (n_pad/256) x 256 x 256 transposed inverses of the diagonal blocks (lazy)
    DevMem<double> d_coef;  // d x hcols
    DevMem<double> d_xs;    // d x n_pad: the inputs times this candidate's coefficients (K1's scalar-row form)
    DevMem<double> d_vec;   // n_pad (gamma)
    DevMem<double> d_rhs;   // n_pad (rho, destroyed by the back-substitution)
    const int *sync_lead = nullptr;  // hand-off words of the lead of the lock-step group this evaluation ran in (diagnostics)
    // what finish_eval needs to enqueue this evaluation once more, alone and by separate launches, when a chain launch ran into
    // its wait bound: coefficient columns and count (the coefficients themselves are still in h_coef), the C^-T buffer of the
    // theta-gradient's rider, and whether this already IS the second attempt
    int retry_hcols = 1, retry_ncoef = 0;
    double *retry_W = nullptr;
    bool retried = false;
    // device-side GLS (p > 1 trend columns): Gram matrix of [ft | yt] and its factor, all (rhs_pad x rhs_pad)
    DevMem<double> d_gneg, d_gram, d_gdinv, d_gramP, d_beta, d_part;
    DevMem<int> d_ginfo;
    PinMem<double> h_gram, h_part, h_beta;
    PinMem<int> h_ginfo;
    bool gls_enqueued = false;  // this evaluation took the device GLS route (set by enqueue_eval)
    PinMem<double> h_coef;
    PinMem<double> h_rows;  // q x n_pad solved RHS rows (ft^T, yt^T)
    PinMem<double> h_diag;  // n
    PinMem<double> h_vec;   // n_pad
    PinMem<int> h_info;     // [0] the factorisation's info, [1..8] the abort word + diagnostics of its chain launches
    // theta-gradient scratch (lazy, gp_fit.hip): the workgroups' partial sums, the reduced sums, their pinned copy
    DevMem<double> d_gpart, d_gout;
    PinMem<double> h_gout;
    // device bytes held (what the resource pool counts): EVERY DevMem above
    size_t device_bytes() const {
        return dW.bytes + d_coef.bytes + d_xs.bytes + d_vec.bytes + d_rhs.bytes + d_gneg.bytes + d_gram.bytes +
               d_gdinv.bytes + d_gramP.bytes + d_beta.bytes + d_part.bytes + d_ginfo.bytes + d_gpart.bytes + d_gout.bytes;
    }
};

// The three slabs of a handle or of a group: one allocation each for all workspaces' (members') matrices, tile inverses, and
// failure flags + hand-off words
struct Slabs {
    DevMem<double> M, D;
    DevMem<int> I;  // one failure flag per workspace, then (from sync_off on) stride_S hand-off words per workspace
                    // for the pipelined chain kernel (kernels_pipe.hip; zeroed by every factorisation)
    size_t bytes() const { return M.bytes + D.bytes + I.bytes; }
    bool complete() const { return M.p && D.p && I.p; }
};
// The geometry of a shape: n training points, p trend columns, nws workspaces (members of a group) in one set of slabs
struct SlabGeometry {
    int n_pad = 0, rhs_pad = 0, m_tot = 0;
    int64_t stride_M = 0, stride_D = 0, stride_S = 0, sync_off = 0;  // elements per workspace; first hand-off word in I
    size_t doubles_M = 0, doubles_D = 0, ints_I = 0;                 // what the three slabs hold
};
SlabGeometry slab_geometry(int64_t n, int64_t p, int nws);  // gp_host.hip
// Everything device-side a handle hands to the resource pool when it is destroyed, and adopts from there when one of its
// shape is created: the training-set buffers, the slabs (none: a member of a group) and the workspaces
struct HandleRes {
    int device = 0;
    DevMem<double> d_xT;    // d x n_pad (k-major normalised inputs, zero padded), then the same times the fit's coefficients
    DevMem<double> d_rhsT;  // q x n_pad: columns of F then y (normalised), as rows
    DevMem<double> d_gamma;  // n_pad
    DevMem<double> d_fit_coef;  // d x hcols coefficients of the fit, then x_mean (d) | x_std (d): dev_xnorm()
    Slabs slabs;
    std::vector<Workspace> ws;
    size_t device_bytes() const {
        size_t b = d_xT.bytes + d_rhsT.bytes + d_gamma.bytes + d_fit_coef.bytes + slabs.bytes();
        for (const auto &w : ws) b += w.device_bytes();
        return b;
    }
};

struct EvalResult {
    double lkh = -std::numeric_limits<double>::infinity();
    int status = EGX_STATUS_OK;
    double sigma2n = 0.0;         // rho^2 / n in normalised units
    std::vector<double> beta;     // p
    bool rho_on_device = false;   // device GLS: rho already sits (zero padded) in the workspace's d_rhs
    std::vector<double> rho;      // n (host GLS)
    std::vector<double> ft;       // n x p row-major
    std::vector<double> ft_qr_r;  // p x p row-major
};

// A validated mixed-integer spec (egx_gp_set_xtypes, the egx_mixint_* helpers; mixint_host.hip): the caller's columns with the
// Ord values copied (xt[j].values is NOT kept), and the per-unfolded-column table mixint.h's arithmetic reads
struct MixSpec {
    std::vector<egx_xtype> xt;
    std::vector<mixint::Col> cols;  // d
    std::vector<double> vals;       // every Ord column's values, in column order
    bool empty() const { return cols.empty(); }
    bool same(const MixSpec &o) const {
        return cols.size() == o.cols.size() && vals.size() == o.vals.size() &&
               (cols.empty() || std::memcmp(cols.data(), o.cols.data(), sizeof(mixint::Col) * cols.size()) == 0) &&
               (vals.empty() || std::memcmp(vals.data(), o.vals.data(), sizeof(double) * vals.size()) == 0);
    }
    // the device table: the columns, then the values
    std::vector<double> table() const {
        std::vector<double> t(2 * cols.size() + vals.size());
        static_assert(sizeof(mixint::Col) == 2 * sizeof(double), "two doubles per column");
        if (!cols.empty()) std::memcpy(t.data(), cols.data(), sizeof(mixint::Col) * cols.size());
        if (!vals.empty()) std::memcpy(t.data() + 2 * cols.size(), vals.data(), sizeof(double) * vals.size());
        return t;
    }
};
// validates (EGX_ERR_INVALID_VALUE / _UNSUPPORTED with a message that starts with `who` and names the entry) and builds;
// d_expect >= 0: the unfolded dimension must be it
int mixspec_build(const char *who, const egx_xtype *xt, int32_t nx, int64_t d_expect, MixSpec &out);

}  // namespace egx

namespace egx {
// Slabs shared by the members of a GROUP of models (egx_gp_create_group): k models of one shape -- the experts of a mixture
// (crates/moe/src/algorithm.rs:167-177), an optimiser's objective and constraint surrogates -- whose matrices sit at the
// fixed strides a lock-step launch needs, although every member has its own training set.  Freed with the last member.
struct GroupSlabs {
    Slabs slabs;
    int device = 0, k = 0;
    int64_t sync_off = 0;  // of the group's I slab
    // x-gradient state of the members (lazy, ensure_winv): C^-T (n_pad^2 doubles per slot) and -R^-1 F (n_pad x rhs_pad per slot)
    // at one stride, so that a run of members takes its weight GEMMs in lock-step; winv_mu guards the allocation (members of a
    // group may be called from different threads)
    DevMem<double> W, NK;
    std::mutex winv_mu;
    ~GroupSlabs();  // gp_host.hip: the slabs go to the resource pool (the next group of this shape adopts them), or are freed
};
}  // namespace egx

struct egx_gp : egx::HandleRes {
    int n = 0, d = 0, p = 0, h = 0, corr = 0, mean = 0;
    double nugget = 0.0;
    int n_pad = 0, rhs_pad = 0, m_tot = 0, q = 0;
    int64_t ld = 0;
    bool has_w = false;
    bool gls_device = false;  // p >= 2: GLS through the Gram matrix on the device (gp_host.hip finish_eval)
    std::vector<double> w_star;  // d x h
    std::vector<double> x_raw, y_raw, xnorm, x_mean, x_std, ynorm, F;
    double y_mean = 0.0, y_std = 1.0;
    // VIEWS of workspace 0's part of the slabs (strides in elements): the handle's own `slabs`, or slot `group_slot` of the group's
    double *slab_M = nullptr, *slab_D = nullptr;
    int *slab_I = nullptr;
    int64_t stride_M = 0, stride_D = 0, stride_S = 0, sync_off = 0;
    std::shared_ptr<egx::GroupSlabs> group;  // member of a group: slab_M / slab_D / slab_I are VIEWS of slot `group_slot`
    int group_slot = -1;
    int lockstep = 1;  // candidates of a likelihood batch factored in lock-step (consecutive workspaces), <= ws.size()
    egx::PotrfSchedule sched;  // how this handle factors: decided at create / egx_gp_set_lockstep (schedule_for), kept by shrink
    // exclusive for everything that touches the fitted state or all workspaces; SHARED for egx_gp_likelihood, whose
    // concurrent callers (the reference's rayon multistart closures, algorithm.rs:928-945) each take a workspace
    // from the pool below
    std::shared_mutex mu;
    std::mutex pool_mu;
    std::condition_variable pool_cv;
    std::vector<char> ws_busy;
    // fitted state (lives in ws[0])
    std::atomic<bool> fitted{false};  // read by concurrent egx_gp_likelihood callers while another one clears it
    std::vector<double> theta;  // h
    double likelihood = 0.0, sigma2 = 0.0;
    std::vector<double> beta, gamma, ft, ft_qr_r;
    std::vector<double> fit_coef;
    int fit_hcols = 1;
    // theta-gradient scratch (allocated on first use, gp_fit.hip): C^-T of `slab_W_count` candidates at a fixed stride of
    // n_pad^2 doubles (lock-step), |w_star| on the device (KPLS + Matern)
    egx::DevMem<double> slab_W, d_wabs;
    int slab_W_count = 0;
    // x-gradient state (lazy, per fitted factor): d_W = C^-T of the FITTED factor and
    // -R^-1 F = -C^-T ft as an (n_pad x rhs_pad) matrix.  A lone handle's own; a member of a group has its slot of the group's
    // W / NK instead: read both through dev_winv() / dev_neg_invkf()
    egx::DevMem<double> d_W, d_neg_invkf;
    std::vector<double> h_neg_invkf;  // host copy (n x p) for the single-point path
    // device scratch of the single-point path, allocated once (a hipMalloc per call would cost more than the kernels)
    egx::DevMem<double> sp_R, sp_P, sp_y, sp_z, sp_wt, sp_out, sp_xq;
    int sp_nsplit = 0;
    int small_var_calls = 0;  // single-point predict_var calls since the fit: the third one builds W = C^-T
    // the small fitted state the trend kernels read (ensure_trend_state): d_tbeta = beta (p), Rq = ft_qr_r and Rq^T (p x p
    // row-major), host_math.h regression_index (2 p)
    egx::DevMem<double> d_tbeta, d_rq, d_rqT;
    egx::DevMem<int> d_fidx;
    uint64_t fit_epoch = 0, winv_epoch = ~(uint64_t)0, trend_epoch = ~(uint64_t)0;
    uint64_t winv_fail_epoch = ~(uint64_t)0;  // fit for which the C^-T cache could not be built (batched path serves it)
    egx_timings timings{};
    // mixed-integer spec (egx_gp_set_xtypes; empty: a continuous model) and its device table (mixint.h: d columns | Ord values)
    egx::MixSpec xspec;
    egx::DevMem<double> d_xspec;
};

namespace egx {
// the two halves of the multistart COBYLA fit (gp_fit.hip): the starts s = rank, rank + world, ... of this rank, then the
// reduction over ALL starts (results of the other ranks filled in by the caller) and the final factorisation
int fit_run_starts(egx_gp *gp, const double *theta_base, const std::vector<int> &active, const double *theta0s,
                   int64_t n_starts, const double *lo, const double *hi, int64_t bounds_len, int64_t max_eval, int rank,
                   int world, std::vector<StartResult> &results);
int fit_reduce_finalize(egx_gp *gp, const double *theta_base, const std::vector<int> &active, const double *theta0s,
                        const std::vector<StartResult> &results, int64_t *n_evals_out);
// the box of a fit and its `count` start values checked (fit_starts.h); a failed check's message is this thread's error
inline int fit_box(const double *lo, const double *hi, int64_t bounds_len, int h, const double *x0s, int64_t count, fit::Model what,
                   fit::Log10Box &box) {
    std::string msg;
    if (fit::log10_box(lo, hi, bounds_len, h, what, box, msg) && fit::positive_starts(x0s, count, what, msg)) return EGX_SUCCESS;
    set_error(msg);
    return EGX_ERR_INVALID_VALUE;
}
}  // namespace egx

// x_mean (d) | x_std (d) on the device, behind the coefficients of the fit in the same allocation
// the training inputs times the coefficients of the fit (d x n_pad, k-major; valid when fit_hcols == 1), behind d_xT in
// the same allocation: what the scalar-row prediction kernel reads (kernels_corr.hip k_predict_mean_srow)
// workspace i's hand-off words in slab_I
inline int *dev_sync(const egx_gp *gp, int i) { return gp->slab_I + gp->sync_off + (int64_t)i * gp->stride_S; }
inline double *dev_xs_fit(const egx_gp *gp) { return gp->d_xT + (size_t)gp->d * gp->n_pad; }
// the device table of the handle's xtypes, or nullptr: what the kernels that read raw query rows cast by
inline const egx::mixint::Col *dev_spec(const egx_gp *gp) {
    return gp->xspec.empty() ? nullptr : reinterpret_cast<const egx::mixint::Col *>(gp->d_xspec.p);
}
// coordinate j of the query row as the model sees it: cast when the handle carries xtypes (the same text as the device's)
inline double query_coord(const egx_gp *gp, const double *row, int j) {
    return gp->xspec.empty() ? row[j] : egx::mixint::cast_coord(gp->xspec.cols.data(), gp->xspec.vals.data(), row, 1, j);
}
// C^-T and -R^-1 F of the fitted factor (ensure_winv), or nullptr before the first use: the handle's own, or its slot of the
// group's slab
inline double *dev_winv(const egx_gp *gp) {
    if (!gp->group) return gp->d_W.p;
    return gp->group->W.p ? gp->group->W.p + (size_t)gp->group_slot * gp->n_pad * gp->n_pad : nullptr;
}
inline double *dev_neg_invkf(const egx_gp *gp) {
    if (!gp->group) return gp->d_neg_invkf.p;
    return gp->group->NK.p ? gp->group->NK.p + (size_t)gp->group_slot * gp->n_pad * gp->rhs_pad : nullptr;
}
inline double *dev_xnorm(const egx_gp *gp) { return gp->d_fit_coef + (size_t)gp->d * (gp->has_w ? gp->h : 1); }

namespace egx {

const std::string &last_error_string();  // this thread's message (egx_last_error)
int set_device(const egx_gp *gp);
int make_coef(const egx_gp *gp, const double *theta, int64_t theta_len, std::vector<double> &coef, int &hcols,
              std::vector<double> *theta_full);
int enqueue_eval(egx_gp *gp, Workspace &w, const std::vector<double> &coef, int hcols);
// `count` evaluations on the consecutive workspaces w0 .. w0 + count - 1, factored in lock-step on the streams of w0
// W0 != nullptr: the `count` buffers W0 + j n_pad^2 receive C^-T of the candidates, riding along the factorisation
int enqueue_eval_group(egx_gp *gp, int w0, int count, const std::vector<double> *coefs, int hcols, double *W0 = nullptr);
// the same for `count` MODELS of one group (consecutive slots): member j evaluates on its own workspace 0, its own training set
// W0 != nullptr: member 0's slot of the group's C^-T slab (GroupSlabs::W); member j's rider writes the slot j behind it
int enqueue_eval_members(egx_gp *const *gps, int count, const std::vector<double> *coefs, int hcols, double *W0 = nullptr);
// The host halves (finish_eval with `keep`) of a run evaluated by enqueue_eval_members, side by side on host threads where they
// issue no launches; RunGuard: whatever way such a run is left, nothing stays in flight on the lead's stream and every
// member's eval_stream is its own again (gp_host.hip)
struct HostHalf {
    EvalResult res;
    int rc = EGX_SUCCESS;
    std::string err;  // (the error text is per thread)
    std::chrono::steady_clock::time_point t0, t1;
};
void host_halves(egx_gp *const *gps, int len, int keep, HostHalf *hh);
struct RunGuard {
    egx_gp *const *gps;
    int len;
    bool synced = false;
    ~RunGuard();
};
int finish_eval(egx_gp *gp, Workspace &w, EvalResult &out, int keep);  // 0 scalars, 1 fitted state, 2 rho only
void record_timings(egx_gp *gp, Workspace &w, double host_ms, double solve_ms);
bool has_nan(const double *theta, int64_t len);
int eval_one(egx_gp *gp, int widx, const double *theta, int64_t theta_len, EvalResult &res, bool keep);
// the host GLS's rho into w.d_rhs, zero padded, on stream st (the device GLS leaves it there itself)
int upload_rho(egx_gp *gp, Workspace &w, const EvalResult &res, hipStream_t st);
int do_finalize(egx_gp *gp, const double *theta, int64_t theta_len);
// The slot pipeline (slot_pipeline.h) over the workspaces of a handle: what both batch cores below run.  Candidates come
// from `src` (nullptr: the sequence 0 .. k-1; a rank's static shard or the node-wide counter of a dynamic sweep, sweep.hip);
// slot i synchronises the stream of its first workspace; a source's index out of range is the error it always was.
// (The synchronisations after an error set no error text: the first error's stays.)
template <class Admit, class Enqueue, class Advance>
int run_slots(egx_gp *gp, const SlotGeometry &g, CandidateSource *src, int64_t k, Admit &&admit, Enqueue &&enqueue, Advance &&advance) {
    SequentialSource seq(k);
    const int rc = run_slot_pipeline(g, src ? *src : static_cast<CandidateSource &>(seq), k, admit, enqueue, advance,
                                     [&](int i) { (void)hipStreamSynchronize(gp->ws[g.first_ws(i)].stream); });
    if (rc) (void)hipGetLastError();
    if (rc == kSlotBadIndex) {
        set_error("likelihood batch: the candidate source returned an index out of range");
        return EGX_ERR_INVALID_VALUE;
    }
    return rc;
}
// Evaluates the candidates `src` hands out (rows of thetas, k x theta_len) pipelined over the handle's workspaces;
// results go to lkh[c] / status[c] of the candidate's own index, evaluated[c] (optional, k chars) is set for them.
int likelihood_batch_core(egx_gp *gp, const double *thetas, int64_t k, int64_t theta_len, double *lkh, int32_t *status,
                          CandidateSource *src = nullptr, char *evaluated = nullptr);
// likelihood + dL/dtheta of the candidates `src` hands out, pipelined over the workspaces in lock-step slots (gp_fit.hip)
int likelihood_grad_batch_core(egx_gp *gp, const double *thetas, int64_t k, int64_t theta_len, double *lkh, double *grad,
                               int32_t *status, CandidateSource *src = nullptr);
// gp_predict.hip
int predict_impl(egx_gp *gp, const double *xq, int64_t m, double *yout, double *vout);
int xgrad_impl(egx_gp *gp, const double *xq, int64_t m, double *gy, double *gv);
// d_W <- C^-T and d_neg_invkf <- -C^-T [ft | yt] of the fitted factor, cached per fitted state (fit_epoch)
int ensure_winv(egx_gp *gp);
// d_tbeta, d_rq, d_rqT, d_fidx of the fitted state, cached likewise; uploads on `st` and waits for it when the state has moved
int ensure_trend_state(egx_gp *gp, hipStream_t st);
// "not fitted" / "bad query array": what every posterior entry point checks first
int check_query(const egx_gp *gp, const double *xq, int64_t m);
// The dense posterior's device sequence on the factor resident in workspace 0, for a k-major query block xqT (d x m_pad):
//   posterior_solve    RT (m_pad x n_pad) = rt^T, rt = C^-1 r(x); s0 = sum rt^2; sl (m_pad x p) = ft^T rt
//   posterior_weights  Wt (n_pad x m_pad) = -(R^-1 r)^T from RT and the cached C^-T (ensure_winv) ...
//   posterior_weights_trend   ... then Wt -= (-R^-1 F) (-D)^T with dneg = -D (m_pad x rhs_pad, zero padded)
int posterior_solve(egx_gp *gp, hipStream_t st, const double *xqT, int m_pad, double *RT, double *s0, double *sl);
// posterior_solve for a run of `len` models of one shape whose factors sit at one stride (members of a group in consecutive
// slots): ONE launch sequence, the member a grid coordinate; every block at the fixed stride of its size (gp_predict.hip).
// posterior_solve is this with len = 1.
int posterior_solve_run(egx_gp *const *gps, int len, hipStream_t st, const double *xqT, int m_pad, double *RT, double *s0, double *sl);
// predict_impl's batched route for such a run: member j answers xq[j] (m rows) into yout[j] / vout[j]
int predict_run(egx_gp *const *gps, int len, const double *const *xq, int64_t m, double *const *yout, double *const *vout);
// gp_host.hip: the run of a multi-model call that starts at gps[i] (members of one group in consecutive slots), the exclusive
// locks of its k distinct handles in a fixed order, and -- under them -- model j's likelihood at row j of thetas (or its fit)
int run_len_multi(egx_gp *const *gps, int k, int i);
int lock_multi(egx_gp *const *gps, int32_t k, std::vector<std::unique_lock<std::shared_mutex>> &locks);
int eval_multi_locked(egx_gp *const *gps, int32_t k, const double *thetas, int64_t theta_len, bool finalize, double *lkh,
                      int32_t *status);
int posterior_weights(egx_gp *gp, hipStream_t st, const double *RT, int m_pad, double *Wt);
int posterior_weights_trend(egx_gp *gp, hipStream_t st, const double *dneg, int m_pad, double *Wt);
// ... for a run of `len` members of a group in consecutive slots (ensure_winv done for each): one GEMM launch each, the blocks
// of member j at RT + j m_pad n_pad, dneg + j m_pad rhs_pad, Wt + j n_pad m_pad; the two above are these with len = 1
int posterior_weights_run(egx_gp *const *gps, int len, hipStream_t st, const double *RT, int m_pad, double *Wt);
int posterior_weights_trend_run(egx_gp *const *gps, int len, hipStream_t st, const double *dneg, int m_pad, double *Wt);
// xgrad_impl's batched route for such a run: member j answers xq[j] (m rows) into gy[j] / gv[j] (m x d each)
int xgrad_run(egx_gp *const *gps, int len, const double *const *xq, int64_t m, double *const *gy, double *const *gv);
// how many parts the training range is split into so that few queries still fill the chip (the caller adds the partial sums
// in order): launch_predict_mean's over rows = n_pad, launch_xgrad's over rows = n
int mean_splits(int rows, int m_pad);
int xgrad_splits(int rows, int m_pad);
// gp_sample.hip: factor sigma2 (K(x, x) + G) (+ tau I) of m queries and draw nt trajectories around `mean` (m_pad host doubles).
// xqT is k-major (d x m_pad, m_pad = m rounded up to 128), G the (m_pad x m_pad) Gram term or nullptr, max_diag the largest
// diagonal entry of the covariance (EGX_SAMPLE_PSD's first jitter), `what` names the covariance in error messages
struct SampleCov {
    int corr;
    const double *xqT;
    int d;
    const double *coef;
    int hcols;
    const double *G;
    double sigma2, max_diag;
    const char *what;
};
int sample_draw(hipStream_t st, const SampleCov &c, int m, int nt, int method, uint64_t seed, const double *z,
                const double *mean, double *traj, double *tau_out);

}  // namespace egx
