// Internal declarations shared by the HIP translation units of libegx_gp_hip.so.
// gfx950 (MI355X / CDNA4) only: wave64, FP64 MFMA 16x16x4, 160 KiB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <string>

#include "../../include/egx_gp.h"
#include "schedule.h"
#include "mixint.h"

namespace egx {

// ---- error plumbing --------------------------------------------------------
void set_error(const std::string &msg);
#define EGX_HIP_CHECK(expr)                                                              \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            ::egx::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));         \
            (void)hipGetLastError(); /* the runtime's last error is sticky: reset it */ \
            return EGX_ERR_HIP;                                                          \
        }                                                                                \
    } while (0)

// From the run-time correlation kind to a template argument: CALL runs with C_ the kind as a constant expression; an unknown
// kind makes the enclosing function return EGX_ERR_INVALID_VALUE
#define EGX_DISPATCH_CORR(corr, CALL)                                                                           \
    switch (corr) {                                                                                             \
        case EGX_CORR_SQUARED_EXPONENTIAL: { constexpr int C_ = EGX_CORR_SQUARED_EXPONENTIAL; CALL; } break;    \
        case EGX_CORR_ABSOLUTE_EXPONENTIAL: { constexpr int C_ = EGX_CORR_ABSOLUTE_EXPONENTIAL; CALL; } break;  \
        case EGX_CORR_MATERN32: { constexpr int C_ = EGX_CORR_MATERN32; CALL; } break;                          \
        case EGX_CORR_MATERN52: { constexpr int C_ = EGX_CORR_MATERN52; CALL; } break;                          \
        default: ::egx::set_error("unknown correlation kind"); return EGX_ERR_INVALID_VALUE;                    \
    }

// hipMalloc that gives the pool of destroyed handles' resources on the current device back before it reports
// out-of-memory (gp_host.hip): every device allocation of the library goes through it
hipError_t dev_malloc_bytes(void **p, size_t bytes);
template <typename T>
inline hipError_t dev_malloc(T **p, size_t bytes) {
    return dev_malloc_bytes(reinterpret_cast<void **>(p), bytes);
}

// ---- geometry ---------------------------------------------------------------
constexpr int kTile = 128;      // row/col granularity of the padded correlation matrix
constexpr int kNB = 256;        // outer Cholesky block (K of the trailing update)
constexpr int kDiagTile = 64;   // diagonal tile factored in registers by one wave
constexpr int kRhsPad = 128;    // rows appended below R for the fused forward solves
// (round 4: no cap on the input dimension d any more -- the correlation kernels stage the dimensions in chunks of 64;
//  the x-gradient kernels need d * (hcols + 5) <= 20480: coefficients and one training point in LDS)

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// The widest lock-step launch: candidates of a slot (egx_gp_set_lockstep clamps the width to it), models of a run
// (egx_gp_finalize_multi).  It sizes the pointer blocks that such a launch takes by value: EvalBatchPtrs, SolveBatchPtrs, GradBatch
constexpr int kLockstepMax = 16;

// ---- kernels_corr.hip -------------------------------------------------------
// coef is (d x hcols) row-major: per-dimension scale (w = I: hcols = 1, coef[j] = theta_j;
// KPLS: sq-exp/abs-exp collapse to hcols = 1, Matern keeps theta_l*|w_jl|).
// xT is k-major (d x ldx): xT[k*ldx + i] = xnorm[i][k]; rows >= n are padding.
// xs_scratch (optional, d x ldx doubles): with it and hcols == 1 the scalar-row kernel runs on prescaled inputs
int launch_corr_sym(hipStream_t s, int corr, const double *xT, int64_t ldx, int n, int d,
                    const double *coef, int hcols, double nugget, double *M, int64_t ld, int n_pad,
                    double *xs_scratch = nullptr);
// per-member pointers of a posterior batch, passed by value to the kernels of the posterior sequence (blockIdx.z / .y = member):
// the members of a group predicting in lock-step (egx_gp_predict_valvar_multi), or ONE model -- a lone model is a batch of
// one.  What a member owns alone comes as a pointer; what the caller lays out per launch (queries, partial sums, the
// (m_pad x n_pad) blocks) sits at the fixed strides of PosteriorBatch.
struct PosteriorBatchPtrs {
    const double *par[kLockstepMax];    // x_mean (d) | x_std (d)                         launch_normalize_queries
    const double *xT[kLockstepMax];     // d x ldx training inputs (prescaled form: times the fit's coefficients)
    const double *coef[kLockstepMax];   // d x hcols
    const double *gamma[kLockstepMax];  // n_pad                                          launch_predict_mean
    const double *ftT[kLockstepMax];    // p rows, ldf apart                              launch_row_reduce
    const mixint::Col *spec[kLockstepMax];  // the member's typed columns (mixint.h: d of them | the Ord values) or nullptr: its
                                            // queries are cast where launch_normalize_queries reads them
};
struct PosteriorBatch {
    int count = 1;
    PosteriorBatchPtrs ptrs{};
    int64_t sq = 0, sracc = 0, sR = 0, ss0 = 0, ssl = 0;  // doubles between two members' xqT / racc / R (RT) / s0 / sl blocks
    int64_t sW = 0, sout = 0;  // ... their (n_pad x m_pad) weight matrices and their partial-sum blocks       launch_xgrad
};
// full (m_pad x n_pad) cross correlation block, row-major into R (ld), no diagonal handling
int launch_cross_corr(hipStream_t s, int corr, const PosteriorBatch &pb, const double *xqT, int64_t ldq, int m_pad, int64_t ldx,
                      int n_pad, int d, int hcols, double *R, int64_t ld);
inline int launch_cross_corr(hipStream_t s, int corr, const double *xqT, int64_t ldq, int m_pad,
                             const double *xT, int64_t ldx, int n_pad, int d, const double *coef,
                             int hcols, double *R, int64_t ld) {
    PosteriorBatch pb;
    pb.ptrs.xT[0] = xT, pb.ptrs.coef[0] = coef;
    return launch_cross_corr(s, corr, pb, xqT, ldq, m_pad, ldx, n_pad, d, hcols, R, ld);
}
// raw row-major queries -> normalised k-major (d x ldq, zero padded to m_pad); par = x_mean (d) | x_std (d) on the device;
// member z reads its m raw rows at xq + z * sxq.  A member with ptrs.spec gets every coordinate cast to its nearest admissible
// discrete value (mixint.h) as it is read: the typed instantiation of the same kernel, the same single launch
int launch_normalize_queries(hipStream_t s, const PosteriorBatch &pb, const double *xq, int64_t sxq, int m, int d, double *xqT,
                             int64_t ldq, int m_pad);
inline int launch_normalize_queries(hipStream_t s, const double *xq, int m, int d, const double *par, double *xqT, int64_t ldq,
                                    int m_pad, const mixint::Col *spec = nullptr) {
    PosteriorBatch pb;
    pb.ptrs.par[0] = par, pb.ptrs.spec[0] = spec;
    return launch_normalize_queries(s, pb, xq, 0, m, d, xqT, ldq, m_pad);
}
// racc[split * m_pad + q] = partial sum_i k(xq, x_i) * gamma[i] over the split's training range (gamma zero padded to
// n_pad); nsplit > 1 spreads a few queries over the chip, the caller adds the partial sums (racc: nsplit * m_pad)
// prescaled != 0: ptrs.xT holds the (d x ldx) training inputs times coef: the scalar-row form, which exists for hcols == 1
// and d <= 64 only -- predict_mean_prescaled says whether a shape takes it (otherwise ptrs.xT are the plain inputs)
bool predict_mean_prescaled(int d, int hcols);
int launch_predict_mean(hipStream_t s, int corr, const PosteriorBatch &pb, const double *xqT, int64_t ldq, int m_pad, int64_t ldx,
                        int n_pad, int d, int hcols, double *racc, int nsplit, int prescaled);
inline int launch_predict_mean(hipStream_t s, int corr, const double *xqT, int64_t ldq, int m_pad,
                               const double *xT, int64_t ldx, int n_pad, int d, const double *coef,
                               int hcols, const double *gamma, double *racc, int nsplit = 1,
                               const double *xs_prescaled = nullptr) {
    const bool pre = xs_prescaled != nullptr && predict_mean_prescaled(d, hcols);
    PosteriorBatch pb;
    pb.ptrs.xT[0] = pre ? xs_prescaled : xT, pb.ptrs.coef[0] = coef, pb.ptrs.gamma[0] = gamma;
    return launch_predict_mean(s, corr, pb, xqT, ldq, m_pad, ldx, n_pad, d, hcols, racc, nsplit, pre ? 1 : 0);
}
// xs[k][i] = coef[k] * xT[k][i] over a (d x ldx) k-major array
int launch_scale_rows(hipStream_t s, const double *xT, int64_t ldx, int d, const double *coef, double *xs);
// x-gradient contraction out[split][a][k] = sum_j w(j, a) d r(x_a, x_j) / d x_ak over the split's training range;
// the weights are the member's gamma (vec != 0: pb.ptrs.gamma, Wt and ldw ignored) or its transposed (n x m_pad) weight matrix
// at Wt + z * pb.sW; m_pad multiple of 128.  blockIdx.z = member of the posterior batch: its own training inputs and
// coefficients (pb.ptrs.xT / coef), its query block pb.sq and its partial sums (nsplit x m_pad x d) pb.sout doubles behind the
// previous member's.  nsplit is the caller's, from ONE member's shape (xgrad_splits): it fixes the order of the partial sums.
// cols (a DEVICE array of ncols distinct column indices in [0, d), or nullptr): the column-list form -- the listed columns k
// alone, with the bits of the full form, and +0.0 in every other column of out
int launch_xgrad(hipStream_t s, int corr, const PosteriorBatch &pb, const double *xqT, int64_t ldq, int m_pad, int64_t ldx, int n,
                 int d, int hcols, const double *Wt, int64_t ldw, int vec, int nsplit, double *out, const int *cols = nullptr,
                 int ncols = 0);
// ... of one model: a batch of one (Wt = gamma with vec != 0)
inline int launch_xgrad(hipStream_t s, int corr, const double *xqT, int64_t ldq, int m_pad, const double *xT, int64_t ldx,
                        int n, int d, const double *coef, int hcols, const double *Wt, int64_t ldw, int vec, int nsplit,
                        double *out, const int *cols = nullptr, int ncols = 0) {
    PosteriorBatch pb;
    pb.ptrs.xT[0] = xT, pb.ptrs.coef[0] = coef, pb.ptrs.gamma[0] = vec ? Wt : nullptr;
    return launch_xgrad(s, corr, pb, xqT, ldq, m_pad, ldx, n, d, hcols, Wt, ldw, vec, nsplit, out, cols, ncols);
}
// few-query form of launch_xgrad with a weight VECTOR: out (ceil(n / 256) x m x d) partial sums, lanes over training points
int launch_xgrad_point(hipStream_t s, int corr, const double *xqT, int64_t ldq, int m, const double *xT, int64_t ldx, int n,
                       int d, const double *coef, int hcols, const double *wvec, double *out);
// single right-hand side through the cached W = C^-T: y <- W^T r (= C^-1 r), z <- W y (= R^-1 r); P scratch 32 * n_pad
int launch_uptri_solve_pair(hipStream_t s, const double *W, int64_t ld, int n, int n_pad, const double *r, double *P,
                            double *y, double *z);
// dst[(r0 + l) * ld + i] = src[l * lds + i] for l < nrows, i < ncols; rest of [r0, r0+rows_pad) x [0, ld) zeroed
int launch_fill_rows(hipStream_t s, double *M, int64_t ld, int r0, int rows_pad, const double *src,
                     int64_t lds, int nrows, int ncols);
int launch_gather_diag(hipStream_t s, const double *M, int64_t ld, int n, double *out);
// per-candidate pointers of a lock-step batch, passed by value to the batched front-end / tail kernels (kernels_corr.hip)
struct EvalBatchPtrs {
    const double *xT[kLockstepMax], *coef[kLockstepMax], *rhsT[kLockstepMax];
    double *xs[kLockstepMax], *M[kLockstepMax];
    double *h_diag[kLockstepMax], *h_rows[kLockstepMax];  // pinned host memory, written by the device
    int *h_info[kLockstepMax];
    const int *d_info[kLockstepMax];
};
int launch_eval_front_batch(hipStream_t s, int corr, const EvalBatchPtrs &b, int count, int64_t ldx, int n, int d, int hcols,
                            double nugget, int64_t ld, int n_pad, int rhs_pad, int q);
int launch_eval_tail(hipStream_t s, const EvalBatchPtrs &b, int count, int64_t ld, int n, int n_pad, int q, int rows, const int *sync);
// per-row reductions over the first n columns of rows [0, m): s0[q] = sum rt^2, sl[q*p + l] = sum rt*ft_l
int launch_row_reduce(hipStream_t s, const PosteriorBatch &pb, const double *RT, int64_t ld, int m, int n, int64_t ldf, int p,
                      double *s0, double *sl);
inline int launch_row_reduce(hipStream_t s, const double *RT, int64_t ld, int m, int n, const double *ftT,
                             int64_t ldf, int p, double *s0, double *sl) {
    PosteriorBatch pb;
    pb.ptrs.ftT[0] = ftT;
    return launch_row_reduce(s, pb, RT, ld, m, n, ldf, p, s0, sl);
}
// device-side GLS helpers: G <- -Gneg (lower, leading q x q) + identity padding; rho <- yt - ft beta with block sums of rho^2
int launch_gram_finish(hipStream_t s, const double *Gneg, double *G, int64_t ldg, int rows, int q);
int launch_gls_residual(hipStream_t s, const double *ftT, int64_t ld, const double *yt, const double *beta, int p, int n,
                        int n_pad, double *rho, double *part);
// zero the strict upper triangle of the leading n x n block
int launch_zero_upper(hipStream_t s, double *M, int64_t ld, int n);
// likelihood-gradient accumulation (new capability; kernels_corr.hip K7): per candidate z of the lock-step batch and every
// output o < nout
//   out[z][o] = sum_{i > j} 2 R_ij (gamma_i gamma_j inv_s2 + rneg_ij) d log R_ij / d c_o
// hcols == 1: output o = input dimension o (nout = d; w = I: coef = theta);
// hcols  > 1 (KPLS + Matern): output o = theta_o, d log R / d theta_o = sum_j wabs[j][o] (d log m / dt)(coef[j][o] a_j) a_j
// Deterministic (fixed reduction order): a candidate's result does not depend on the batch it runs in.
struct GradBatch {
    int count = 1;
    const double *xT[kLockstepMax];     // d x ldx: the training inputs of the entry's OWNER (raw forms; the candidates of one
                                        // handle all name the same array, the members of a group each their own)
    const double *xs[kLockstepMax];     // d x ldx: the inputs times the candidate's coefficients (prescaled form only)
    const double *coef[kLockstepMax];   // d x hcols
    const double *gamma[kLockstepMax];  // n_pad
    const double *rneg[kLockstepMax];   // -R^-1, lower triangle, leading dimension ld
    double inv_s2[kLockstepMax];        // 1 / sigma2 (normalised units)
    double *part[kLockstepMax];         // grad_partial_doubles(nout) doubles of scratch
    double *out[kLockstepMax];          // nout
};
int grad_partial_doubles(int nout);
int launch_grad_accum(hipStream_t s, int corr, int64_t ldx, int n, int d, int hcols, const double *wabs, int nout, int64_t ld,
                      const GradBatch &batch, int prescaled = 0);
// xs[j][k][i] = coef[j][k] * xT[j][k][i] for the entries j < count of b (their xT, coef and xs alone are read): launch_scale_rows
// for every entry in ONE launch, the same product per element
int launch_scale_rows_batch(hipStream_t s, const EvalBatchPtrs &b, int count, int64_t ldx, int d);
// z (n) <- W y, W upper triangular row-major
int launch_uptri_gemv(hipStream_t s, const double *W, int64_t ld, int n, const double *y, double *z);
// ... for `count` matrices W + j sW, each with its own y[j] and z[j], in ONE launch (grid.y = matrix): row i of matrix j is summed
// by one wave in the order launch_uptri_gemv sums it, so z[j] is bit for bit the lone launch's
struct GemvBatchPtrs {
    const double *y[kLockstepMax];
    double *z[kLockstepMax];
};
int launch_uptri_gemv_batch(hipStream_t s, const double *W, int64_t sW, int64_t ld, int n, const GemvBatchPtrs &b, int count);
// the same for `rows` right-hand sides, rows of Y (ldr apart): Z[a] = W Y[a], or base[a] + sc * W Y[a] with base != nullptr
// (base may be Z)
int launch_uptri_gemv_rows(hipStream_t s, const double *W, int64_t ld, int n, const double *Y, const double *base, double sc,
                           double *Z, int64_t ldr, int rows);
// posterior covariance of the m queries (k-major xqT, m_pad a multiple of 64): S (m_pad x m_pad, lds) = sigma2 (K(xq, xq) + G)
// + tau I on the leading m x m block (K without nugget; G lower tiles read at i >= j only: S exactly symmetric), identity
// rows / columns beyond m
int launch_cov_assemble(hipStream_t s, int corr, const double *xqT, int64_t ldq, int m_pad, int d, const double *coef, int hcols,
                        const double *G, int64_t ldg, int m, double sigma2, double tau, double *S, int64_t lds);

// ---- kernels_sample.hip -----------------------------------------------------
// U / Uneg (m_pad x ldu, zero padded beyond p and below m) = +- Rq^-T (sl[q] - f(x_q))^T per query: the u of predict_var;
// fidx (2 p ints) names the coordinates of regression column l (-1: 1.0), R = ft_qr_r (p x p row-major) on the device
int launch_sample_u(hipStream_t s, const double *sl, int p, const double *xqT, int64_t ldq, const int *fidx, const double *R,
                    int m, int m_pad, double *U, double *Uneg, int64_t ldu);
// Z[i * si + j * sj] (i < m, j < nt) = the normals of philox.h for `seed`
int launch_normals(hipStream_t s, uint64_t seed, int64_t m, int64_t nt, double *Z, int64_t si, int64_t sj);
// T (m_pad x nt_pad, ldt) = mean 1^T + L Zt^T, L lower triangular with a zero strict upper triangle, Zt (nt_pad x m_pad, ldz)
int launch_trmm_mean(hipStream_t s, const double *L, int64_t ldl, int m_pad, const double *Zt, int64_t ldz, int nt_pad,
                     const double *mean, double *T, int64_t ldt);

// ---- kernels_infill.hip -----------------------------------------------------
// The host arithmetic of predict_impl / xgrad_impl as kernels over ONE tile of kTile query points of one model, and the
// criterion of infill_math.h across the models of a point (infill_eval.hip).
namespace infill {
struct Params;
}
// raw rows (mt x d, mt <= kTile) -> normalised k-major tile xqT (d x kTile); par = x_mean (d) | x_std (d); points with a
// non-finite coordinate are zeroed and flagged (flag: kTile ints or nullptr), the slots beyond mt are zero.
// spec != nullptr (mixint.h): the coordinates are cast as they are read, and xcast (mt x d, or nullptr) receives the tile's CAST
// raw rows -- what k_infill_mix reads in place of xq, so that the responsibilities see the cast point as the experts do
// The member of a RUN of models (infill_runs.h) is a grid coordinate of the five kernels below: pb.count models read the same raw
// tile, member z through pb.ptrs.par[z] (and .spec[z]: all typed alike, or none) into xqT + z * pb.sq; flag and xcast are member
// 0's to write.  One model is a run of one.
int launch_infill_prepare(hipStream_t s, const PosteriorBatch &pb, const double *xq, int mt, int d, double *xqT, int *flag,
                          double *xcast = nullptr);
inline int launch_infill_prepare(hipStream_t s, const double *xq, int mt, int d, const double *par, double *xqT, int *flag,
                                 const mixint::Col *spec = nullptr, double *xcast = nullptr) {
    PosteriorBatch pb;
    pb.ptrs.par[0] = par, pb.ptrs.spec[0] = spec;
    return launch_infill_prepare(s, pb, xq, mt, d, xqT, flag, xcast);
}
struct InfillTrend {
    int p = 1, rp = 0, msplit = 1;
    const double *xqT = nullptr;   // d x kTile
    const int *fidx = nullptr;     // 2 p ints: the coordinates of regression column l (-1: 1.0)
    const double *beta = nullptr;  // p
    const double *R = nullptr, *Rt = nullptr;  // ft_qr_r and its transpose (p x p row-major)
    const double *racc = nullptr;  // msplit x kTile partial sums of launch_predict_mean
    const double *s0 = nullptr, *sl = nullptr;  // launch_row_reduce's outputs
    double sigma2 = 0.0, y_mean = 0.0, y_std = 1.0;
    double *mean = nullptr, *var = nullptr;  // kTile each
    double *dneg = nullptr;        // kTile x rp: -D = -B^-1 A^T zero padded, or nullptr (values only)
};
// t[0 .. count): the members of a run, every pointer the member's own (its blocks of the caller's layout among them); the members
// have one trend and one split count
int launch_infill_trend(hipStream_t s, const InfillTrend *t, int count);
inline int launch_infill_trend(hipStream_t s, const InfillTrend &t) { return launch_infill_trend(s, &t, 1); }
// gmean / gvar (kTile x d) from launch_xgrad's partial sums (nsplit x kTile x d each), original units
struct InfillFinish {
    const double *out_y = nullptr, *out_v = nullptr;  // the member's partial sums
    const double *x_std = nullptr;                    // d
    double *gmean = nullptr, *gvar = nullptr;         // kTile x d each (this tile of this model)
};
int launch_infill_xgrad_finish(hipStream_t s, const InfillTrend *t, const InfillFinish *f, int count, int d, int nsplit);
inline int launch_infill_xgrad_finish(hipStream_t s, const InfillTrend &t, int d, int nsplit, const double *out_y, const double *out_v,
                                      const double *x_std, double *gmean, double *gvar) {
    const InfillFinish f{out_y, out_v, x_std, gmean, gvar};
    return launch_infill_xgrad_finish(s, &t, &f, 1, d, nsplit);
}
// A surrogate with k >= 2 experts, one tile: the mixture's responsibilities at the tile's raw points and the recombination of
// the experts' tables (expert c of point a at c * estride + a, gradients at (c * estride + a) * d) into the surrogate's slot.
struct InfillMix {
    int mt = 0, d = 0, k = 0;
    bool smooth = true, want_g = false;
    const double *xq = nullptr;    // the tile's mt raw rows
    const int *flag = nullptr;     // the tile's kTile flags
    const double *means = nullptr, *precs = nullptr, *par = nullptr;  // k x d, k x d x d scaled factors, k (gmx_point.h)
    const double *emean = nullptr, *evar = nullptr, *egmean = nullptr, *egvar = nullptr;
    int64_t estride = 0;
    double *mean = nullptr, *var = nullptr, *gmean = nullptr, *gvar = nullptr;  // the surrogate's tile
    double *dp = nullptr;          // kTile x k x d scratch for d p / d x: needed by smooth gradients, else optional
    double *probas = nullptr;      // kTile x k copy of the responsibilities, or nullptr
};
constexpr size_t kInfillMixMaxLds = 160 * 1024;
size_t infill_mix_lds_bytes(int d, int k);  // 64 lanes x (3 (d | 1) + 2 (k | 1)) doubles
int launch_infill_mix(hipStream_t s, const InfillMix &g);
// value[i] / grad[i * d ..] of the m points of a call; model j of point i at j * mstride + i; grad may be nullptr
int launch_infill_combine(hipStream_t s, const infill::Params &prm, int k, int d, int64_t m, int64_t mstride, const double *mean,
                          const double *var, const double *gmean, const double *gvar, const double *tol, const int *flag,
                          double *value, double *grad);
// The mean halves of launch_infill_trend / _xgrad_finish / _mix (a constraint surrogate under EGX_CSTR_MEAN): s0, sl, R, Rt,
// dneg, out_v, evar, egvar, var, gvar are not read or written; the means keep the bits of the full forms.
int launch_infill_trend_mean(hipStream_t s, const InfillTrend *t, int count);
inline int launch_infill_trend_mean(hipStream_t s, const InfillTrend &t) { return launch_infill_trend_mean(s, &t, 1); }
int launch_infill_xgrad_finish_mean(hipStream_t s, const InfillTrend *t, const InfillFinish *f, int count, int d, int nsplit);
inline int launch_infill_xgrad_finish_mean(hipStream_t s, const InfillTrend &t, int d, int nsplit, const double *out_y,
                                           const double *x_std, double *gmean) {
    const InfillFinish f{out_y, nullptr, x_std, gmean, nullptr};
    return launch_infill_xgrad_finish_mean(s, &t, &f, 1, d, nsplit);
}
int launch_infill_mix_mean(hipStream_t s, const InfillMix &g);
// A SPARSE expert's tails for one tile (sgp_predict.hip's host arithmetic): mean (kTile) = the msplit partial sums of
// launch_predict_mean (racc: msplit x kTile; the weight vector carries sigma2) in split order; var (kTile, or nullptr: the
// mean-only form) = max(sigma2 - sigma2 (p2 + s q2), 1e-15) + noise, p2 / q2 (kTile) the row reductions of the two block solves
int launch_infill_sgp_finish(hipStream_t s, const double *racc, int msplit, const double *p2, const double *q2, double sigma2,
                             double noise, int vfe, double *mean, double *var);
// gmean / gvar (kTile x d) from launch_xgrad's partial sums (nsplit x kTile x d each): gmean = sum, gvar = gv_scale * sum, exactly
// 0 where the raw variance is below the clamp; out_v / gvar nullptr: the mean-only form
int launch_infill_sgp_xgrad_finish(hipStream_t s, const double *out_y, const double *out_v, int nsplit, int d, const double *p2,
                                   const double *q2, double sigma2, int vfe, double gv_scale, double *gmean, double *gvar);
// EGX_CSTR_MEAN / _UTB: value[i] (the objective model's criterion, no feasibility factor), cstr[i * k + j], grad (m x d),
// gcstr (m x k x d); any output may be nullptr; scale: the k scale_cstr on the device
int launch_infill_cstr(hipStream_t s, const infill::Params &prm, int strategy, int k, int d, int64_t m, int64_t mstride,
                       const double *mean, const double *var, const double *gmean, const double *gvar, const double *scale,
                       const int *flag, double *value, double *cstr, double *grad, double *gcstr);
// the scaling pass' terms per point, on the device with k_infill_combine's text: ei (EI value; nullptr = skipped), base (the
// objective of prm without the feasibility factor) and fac (pofs, or logpofs for LogEI); base == nullptr skips both
int launch_infill_scale_terms(hipStream_t s, const infill::Params &prm, int k, int64_t m, int64_t mstride, const double *mean,
                              const double *var, const double *tol, const int *flag, double *ei, double *base, double *fac);

// ---- kernels_pending.hip ----------------------------------------------------
// A model conditioned on the q <= 16 pending points of its infill handle (pending_math.h), per tile of kTile queries.
constexpr int kPendingQV = 4;     // columns of W^ per pass of the contraction
constexpr int kPendingMaxD = 64;  // the lane's query coordinates and the finish's d c / d x live in LDS
int pending_splits(int nz);       // splits of the nz = n + q points of Z for one tile: a function of nz alone
// c[a, v] = sum_j r(x_a, Z_j) W^[j, v] and (outg != nullptr) its gradient in the tile's normalised coordinates, as partial sums
// per split: outc (nsplit x kTile x q), outg (nsplit x kTile x q x d).  ZT: d x ldz k-major, nz points; W: nz x 16 row-major
int launch_pending_cross(hipStream_t s, int corr, const double *xqT, const double *ZT, int64_t ldz, int nz, int d, const double *coef,
                         int hcols, const double *W, int q, int nsplit, double *outc, double *outg);
struct PendingFinish {
    int q = 0, d = 0, p = 0;
    int nsplit_c = 0, nsplit_g = 0;  // splits of the partial sums of c and of d c / d x
    bool composed = false;           // the layouts of the composed form: per column launch_predict_mean's and launch_xgrad's
    const double *xqT = nullptr;    // d x kTile
    const int *fidx = nullptr;      // 2 p
    const double *tv = nullptr;     // 16 x p: t_v = D_v
    const double *small = nullptr;  // chol(S) (16 x 16, lower) | alpha (16)
    const double *outc = nullptr, *outg = nullptr;
    const double *x_std = nullptr;  // d
    double sigma2 = 0.0, sigma2c = 0.0, y_std = 1.0;  // the fitted and the conditioned process variance (raw units)
    double *mean = nullptr, *var = nullptr, *gmean = nullptr, *gvar = nullptr;  // rewritten in place; var / gvar nullptr: mean only
    double *emit = nullptr;         // kTile x 16: the cross-covariances themselves and nothing rewritten
};
int launch_pending_finish(hipStream_t s, const PendingFinish &f);
// a push: column v of W^, t_v and the point's coordinates in Z from query 0 of the tile sequence that just ran
int launch_pending_capture(hipStream_t s, const double *Wt, const double *dneg, const double *xqT, int n, int d, int p, int v,
                           double *W, double *Wc, double *tv, double *ZT, int64_t ldz);
// egx_set_tuning "pending_composed": 1 = the composed form (q launches of launch_predict_mean / launch_xgrad over Z with a
// column of W^ as the weight vector) even where the fused contraction applies (d <= kPendingMaxD); 0 (default): fused there
extern std::atomic<int> g_pending_composed;

// ---- kernels_gmm.hip --------------------------------------------------------
// EM of a Gaussian mixture for R restarts in lock-step over one (n x D) data set (egx_gmm_fit).  DP = D rounded up to a
// multiple of 4; every per-cluster array on the device is padded to it with zeros.
constexpr int kGmmTileRows = 256;   // rows per workgroup of the E-step
constexpr int kGmmBlockAcc = 21;    // doubles per 4 x 4 moment block: 16 second moments, 4 first moments, sum of responsibilities
constexpr int kGmmMaxDim = 36;      // D <= DP <= 36
constexpr int kGmmMaxClusters = 16;
constexpr int kGmmMaxBlocks = (kGmmMaxDim / 4) * (kGmmMaxDim / 4 + 1) / 2;
struct GmmLaunch {
    const double *data = nullptr;  // n x D row-major
    int64_t n = 0;
    int D = 0, DP = 0, k = 0, R = 0;
    int T = 0;        // tiles of kGmmTileRows rows; the wide path: chunks (gmm_wide_plan.h)
    int tpc = 1;      // the wide path: consecutive tiles of a chunk
    int rsplit = 1;  // workgroups per tile; workgroup y serves the restarts y, y + rsplit, ..
    int init = 0;     // iteration 0: one-hot responsibilities on the nearest mean
    const int *active = nullptr;           // R: 0 = frozen, both kernels skip it
    double *means = nullptr;               // R x k x DP
    double *prec = nullptr;                // R x k x DP x DP, upper triangular precisions_chol
    double *cst = nullptr;                 // R x k: -D/2 ln 2 pi + sum ln diag P + ln w
    double *weights = nullptr;             // R x k
    double *covs = nullptr;                // R x k x D x D (not padded)
    double *part = nullptr;                // T x R x k x gmm_part_len(DP): the tiles' partial moments
    double *lpn_part = nullptr;            // T x R: the tiles' sums of log-prob-norm
    double *lbst = nullptr;                // R lower bounds | R failure flags (non-zero: failed)
};
inline size_t gmm_part_len(int DP) { return (size_t)(DP / 4) * (DP / 4 + 1) / 2 * kGmmBlockAcc; }
size_t gmm_estep_lds_bytes(int DP, int k);
int launch_gmm_estep(hipStream_t s, const GmmLaunch &g);
int launch_gmm_mstep(hipStream_t s, const GmmLaunch &g, double reg_covar);
// kernels_gmm_wide.hip: the same two steps for rows up to 128 wide on the FP64 matrix unit (egx_gmm_fit_wide).  DP = D rounded
// up to 16, T = chunks, part = chunks x R x k x gmm_wide::part_len(DP), prec starts as the identity (iteration 0 measures
// ||x - mu||^2 through the same product)
int launch_gmm_estep_wide(hipStream_t s, const GmmLaunch &g);
int launch_gmm_mstep_wide(hipStream_t s, const GmmLaunch &g, double reg_covar);
// The fitted mixture at m raw points (m x d on the device), one lane per point on the calling thread's default stream: the
// responsibilities (out: m x k) or, deriv, their x-derivatives (m x k x d).  blk = gmx_pack's block (gmx_point.h) on the device,
// lds = the dynamic LDS the caller has sized and bounded.  spec != nullptr (mixint.h, on the device): the points are cast as they
// are staged.
int launch_gmx_probas(bool deriv, const double *xq, int64_t m, int d, int k, const double *blk, size_t lds, double *out,
                      const mixint::Col *spec = nullptr);

// ---- kernels_chol.hip -------------------------------------------------------
// In-place blocked right-looking Cholesky of the leading n_pad x n_pad block (lower), applied to
// all m_tot >= n_pad rows (rows >= n_pad are right-hand sides: on return they hold (C^-1 B)^T).
// dinv receives the inverses of the 64x64 diagonal tiles ((n_pad/64) * 4096 doubles) followed by one flag per tile
// (1.0: ill-conditioned tile, the solves refine once; see k_panel_trsm): dinv_doubles(n_pad) doubles in all.
// info (device int): 0 or 1-based index of the first non-positive pivot.
// ev_syrk: optional accumulation of per-launch timings is done by the caller via events.
// Optional per-launch timing of the big-tile trailing-update kernel (the dominant kernel): event pairs recorded on
// the stream the kernel is launched on.  Filled by launch_potrf, read back by the caller after a stream sync.
inline size_t dinv_doubles(int n_pad) { return (size_t)(n_pad / 64) * 4096 + (size_t)(n_pad / 64); }
struct GemmTrace {
    static constexpr int kMax = 192;
    hipEvent_t e0[kMax], e1[kMax];
    double flops[kMax];
    int used = 0;
    bool ready = false;
};
// Look-ahead resources: s2 = chain stream (diagonal blocks, panel solves), s3 = side stream (the off-critical-path rest
// of the chain's updates), both high priority; events: ev_lu (next diagonal block updated), ev_lur (rest of the next
// group's columns updated), ev_panel (chain of the next group done), ev_a / ev_b (hand-offs between s2 and s3).
// Both streams or none: launch_potrf takes a look-ahead without s2 or without s3 as no look-ahead.
struct PotrfLookahead {
    hipStream_t s2 = nullptr, s3 = nullptr;
    hipEvent_t ev_lu = nullptr, ev_lur = nullptr, ev_panel = nullptr, ev_a = nullptr, ev_b = nullptr;
};
// The inverse of the factor riding along the factorisation (theta-gradient): W (n_pad x n_pad, ldw; holds the rows of the
// identity on entry, launch_identity_rows) becomes C^-T.  As soon as a group of panels is final, the forward block
// substitution of W's rows through THAT group -- panel solves with the 16 x 16 inverses the diagonal-block kernel left
// behind, the in-group updates and the update of all later columns -- is enqueued on the stream `sw`, beside the
// factorisation's own trailing update: the substitution's chip-filling GEMMs hide the factorisation's serial chain (most
// of all in its last ~5000 columns, where the trailing matrix is small and W's rows are many), and its small launches
// hide behind the factorisation's big ones.  Same flops as launch_trsm_rows(tri_rows) after the factorisation (n^3/3).
struct PotrfInverse {
    double *W = nullptr;
    int64_t ldw = 0, sW = 0;  // sW: doubles between consecutive matrices' W (lock-step batch)
    hipStream_t sw = nullptr;
    hipEvent_t ev_grp = nullptr, ev_done = nullptr;
};
// Lock-step batches: `count` matrices of one shape, matrix z at (pointer of matrix 0) + z * stride (elements).  Every
// kernel of the factorisation takes the batch as grid.z; a matrix gets the same arithmetic alone and in a batch.
struct GemmBatch {
    int count = 1;
    int64_t sC = 0, sA = 0, sB = 0;  // doubles between consecutive matrices' C / A / B
    int sInfo = 0;                   // ints between their failure flags
};
struct PotrfBatch {
    int count = 1;
    int64_t sM = 0, sD = 0;  // doubles between consecutive matrices / their dinv blocks
    int sI = 0;              // ints between their info words
    int left = 0;            // left-looking group updates (launch_potrf); chosen per handle: potrf_left_for()
    int w_left = 0;          // ... and the C^-T rider's (PotrfInverse) left-looking update: w_left_for()
    int *sync = nullptr;     // hand-off words of the pipelined chain kernel (kernels_pipe.hip): pipe_sync_ints() ints per matrix,
    int64_t sS = 0;          // sS ints apart; nullptr: the chain runs as separate launches (k_potf2_reg, k_panel_trsm16, updates)
    int pipe = 0;            // ... the chain of every group of panels is one chain launch (schedule.h: per handle)
    int whole = 0;           // ... the WHOLE factorisation is one chain launch (every update inside it)
    int flow = 0;            // ... the whole factorisation is one FLOW launch (pipe_flow.h; one matrix per launch)
    int flow_tail = 0;       // ... the LAST flow_tail columns of a right-looking factorisation by separate launches are one flow launch
    int group_panels = 0;    // panels per trailing update, from the handle's schedule (0: by size, potrf_group_panels): launch_potrf
                             // never reads the process-wide knobs for a handle that carries its schedule
    int seqs = 1;            // launch sequences of this handle that may be in flight at once (workspaces / lock-step width):
                             // beyond two, a look-ahead chain launch waits for its columns on the STREAM, not on the device
};
int potrf_left_for(int n_pad, int lockstep);
int w_left_for(int n_pad, int lockstep);
// the schedule of a handle's factorisations, decided once per handle shape: schedule.h (table, rationale, host test)
PotrfSchedule schedule_for(int n_pad, int lockstep, int n_workspaces);
int potrf_group_panels(int n_pad);
// the solves after a factorisation in lock-step: `count` factors (sM apart, tile inverses sD apart) and as many
// right-hand-side buffers (sR apart)
struct TrsmBatch {
    int count = 1;
    int64_t sM = 0, sD = 0, sR = 0;
};
// lk == nullptr runs everything in order on s.
int launch_potrf(hipStream_t s, double *M, int64_t ld, int n_pad, int m_tot, double *dinv, int *info,
                 const PotrfLookahead *lk = nullptr, GemmTrace *trace = nullptr, const PotrfBatch *batch = nullptr,
                 const PotrfInverse *inv = nullptr);
// rows [0, m) of RT (ld) are right-hand sides: RT <- RT * C^-T  (C = lower factor in M, n_pad cols)
// tri_rows != 0: the rows are those of the identity (solution upper triangular): zero blocks are skipped
int launch_trsm_rows(hipStream_t s, const double *M, int64_t ldm, int n_pad, const double *dinv,
                     double *RT, int64_t ldr, int m, int tri_rows = 0, const TrsmBatch *batch = nullptr);
// W (n_pad x n_pad, ld; `count` of them `stride` apart) <- the identity's rows, as far as the two calls below touch them
int launch_identity_rows(hipStream_t s, double *W, int64_t ld, int n_pad, int count = 1, int64_t stride = 0);
// C (lower tiles; n x n) <- -(W W^T), W upper triangular (C^-T): the theta-gradient's -R^-1; C is not read
int launch_syrk_uptri_neg(hipStream_t s, double *C, int64_t ldc, const double *W, int64_t ldw, int n,
                          const GemmBatch *batch = nullptr);
// dinv <- inverses of the 64x64 diagonal tiles of a given lower factor (model load path)
int launch_diag_tile_inverses(hipStream_t s, const double *M, int64_t ld, int n_pad, double *dinv);
// Wall ((n_pad/256) x 256 x 256) <- transposed inverses of the 256x256 diagonal blocks of the factor
// per-model pointers of a back-substitution, by value in the kernel arguments: the models of a run in lock-step
// (egx_gp_finalize_multi; blockIdx.y = model), or ONE factor -- a lone model is a batch of one
struct SolveBatchPtrs {
    const double *M[kLockstepMax], *dinv[kLockstepMax];
    double *dW[kLockstepMax], *rhs[kLockstepMax], *vec[kLockstepMax];
};
// the buffer of the 256 x 256 inverse blocks (launch_block_inverse: Wall / dW) carries, behind the blocks, the start ticket and
// the exchange buffer of the one-launch back-substitution (k_trsv_t_fused): allocate block_inverse_doubles(n_pad) doubles
inline size_t trsv_tail_doubles(int n_pad) { return 4 + (size_t)n_pad; }
inline size_t block_inverse_doubles(int n_pad) { return (size_t)((n_pad + kNB - 1) / kNB) * 65536 + trsv_tail_doubles(n_pad); }
long long pipe_timeout_ticks();  // EGX_PIPE_TIMEOUT_MS in ticks of the 100-MHz wall clock (kernels_pipe.hip)
// dW[j] <- the 256 x 256 inverse blocks of factor j (M[j], dinv[j]), j < count
int launch_block_inverse(hipStream_t s, const SolveBatchPtrs &b, int count, int64_t ld, int n_pad);
// vec[j] (n_pad) <- C_j^-T rhs[j]   (needs launch_block_inverse first).  One launch (k_trsv_t_fused; rhs is left alone) unless
// per_block or "trsv_fused" = 0: then one launch per 256-column block, and rhs is destroyed
int launch_trsv_t(hipStream_t s, const SolveBatchPtrs &b, int count, int64_t ld, int n_pad, bool per_block = false);
// ... of one factor
inline int launch_block_inverse(hipStream_t s, const double *M, int64_t ld, int n_pad, const double *dinv, double *Wall) {
    const SolveBatchPtrs b{{M}, {dinv}, {Wall}, {}, {}};
    return launch_block_inverse(s, b, 1, ld, n_pad);
}
inline int launch_trsv_t(hipStream_t s, const double *M, int64_t ld, int n_pad, double *Wall, double *v, double *xout,
                         bool per_block = false) {
    const SolveBatchPtrs b{{M}, {}, {Wall}, {v}, {xout}};
    return launch_trsv_t(s, b, 1, ld, n_pad, per_block);
}
// C (M x N, ldc) -= A (M x K, lda) * B (N x K, ldb)^T ; lower != 0 skips tiles strictly above the diagonal
// ktri != 0 (with lower): A and B are upper triangular, the K loop of tile (bx, by) starts at row bx*tile
// info != nullptr: device flag of the enclosing factorisation; the kernel returns at once when it is non-zero
int launch_gemm_nt_sub(hipStream_t s, double *C, int64_t ldc, const double *A, int64_t lda,
                       const double *B, int64_t ldb, int M, int N, int K, int lower, int ktri = 0,
                       bool *used_big_tile = nullptr, const int *info = nullptr, const GemmBatch *batch = nullptr,
                       int tag = 0);  // tag: kernel symbol of the stream kernel (profiling only; k_gemm_stream's TAG)
// Gneg (rows x rows, ldg; lower 64x64 tiles) <- -(W W^T) for a small output and a long contraction (split-K, partial
// tiles in the scratch P of gram_scratch_doubles(rows, K) doubles, summed in a fixed order)
size_t gram_scratch_doubles(int rows, int K);
int launch_gram_lower(hipStream_t s, const double *W, int64_t ldw, int rows, int K, double *Gneg, int64_t ldg, double *P);
int mfma_probe(double *max_abs_err);

// ---- kernels_pipe.hip -------------------------------------------------------
// The serial chain of a GROUP of panels -- diagonal blocks, panel solves, the updates of the group's own later columns -- as
// ONE persistent launch with device-side hand-offs (k_potrf_pipe): the group [g0, g0 + gw) of `pb.count` matrices in lock-step,
// whose columns have received every update of the earlier groups.  `pb.sync` = pipe_sync_ints(n_pad, m_tot) ints per matrix,
// ZEROED once per factorisation (launch_potrf does it) -- all hand-off words count upwards over the launches of one
// factorisation.  After the factorisation word 0 of the FIRST matrix' block is non-zero iff a bounded wait inside a launch
// ran out (EGX_PIPE_TIMEOUT_MS): the factors are then unusable and the caller reports EGX_ERR_HIP.
size_t pipe_sync_ints(int n_pad, int m_tot);
// ext_need != 0: the solves of the group's first panel wait, on the device, until pipe_signal(.., ext_need) has run (the rest
// of the group's columns is being updated by a launch beside this one); shared_chip: other launches of the factorisation run
// beside this one (look-ahead): the grid leaves them compute units.
int launch_potrf_pipe(hipStream_t s, double *M, int64_t ld, int n_pad, int m_tot, double *dinv, int *info,
                      const PotrfBatch &pb, int g0, int gw, int ext_need = 0, int shared_chip = 0);
int pipe_signal(hipStream_t s, const PotrfBatch &pb, int value);
// The WHOLE factorisation of ONE large matrix as a flow launch (k_potrf_flow; pipe_flow.h: critical stage lists + bulk-class
// rounds per column, round 6); pb.sync as for the chain launch (pipe_sync_ints covers both).  flow_fits: 256-column panels and
// a workgroup per diagonal block + workers on the current device.
// col_base != 0: (M, n_pad, m_tot, dinv) describe the trailing part of a larger matrix from that column on, which has received
// every update of the columns before it (launch_potrf's flow tail); only the reported pivot index uses it.
int launch_potrf_flow(hipStream_t s, double *M, int64_t ld, int n_pad, int m_tot, double *dinv, int *info, const PotrfBatch &pb,
                      int col_base = 0);
bool flow_fits(int n_pad);
int pipe_enabled();    // EGX_PIPE (default on); 0 as well when the launch cannot be set up on this device
bool pipe_fits(int nz, int np);  // one workgroup per diagonal block (np panels of nz matrices) + a worker fit the CURRENT device
int pipe_prepare(int n_pad, int m_tot, const PotrfSchedule &sched);  // build + upload the task lists a handle of this shape launches
size_t pipe_release_plans();     // egx_trim: free every task list (synchronises the devices that hold one); bytes freed
int pipe_set_knob(const char *name, int value);  // "pipe", "pipe_timeout_ms" (+ "pipe_stall" in test builds); INT_MIN = unknown
#ifdef EGX_TEST_HOOKS  // egobox_amd/lib/_dev/libegx_gp_hip_testhooks.so and tools/pipe_check only
void pipe_set_trace(long long *device_buf);  // profiling: 8 words per ticket of the next chain launches (nullptr: off)
void pipe_test_set_workgroups(int wgs);      // grid of the next chain launches (0 = the product's)
void pipe_set_trace_cap(int slots);          // slots of the trace buffer (flow launches take them from a counter)
void flow_test_set_leads(int lead_short, int lead_long);  // FlowArgs::lead_* of the next flow launches (-1: the product's)
#endif
int chol_init();  // one-time function attribute setup (dynamic LDS sizes)

// ---- kernels_pls.hip --------------------------------------------------------
// PLS1 rotations w (d x k, row-major) of the n rows of xT (d x ld, k-major; ld even and >= n) and y (n, readable up to an even
// count) on the device: column means, centred Gram matrix on the matrix unit (split-K, summed in chunk order), the O(d^2 k)
// deflation on the host (pls_host.h).  *status: 0, or 1 with zeros on a constant response.  Synchronises s.
int pls_device_rotations(hipStream_t s, const double *xT, int64_t ld, const double *y, int64_t n, int d, int k, double *w, int *status);
// the three launches alone between two events (a measurement aid: tools/pls_bench.py)
int pls_device_launch_ms(hipStream_t s, const double *xT, int64_t ld, const double *y, int64_t n, int d, double *ms);
int pls_check_k(int64_t k, int64_t d);  // the reference's two messages for k < 1 and k > d
int set_knob(const char *name, int value);  // kernels_chol.hip tuning knobs by name; INT_MIN = unknown

}  // namespace egx
