// Kernels of the fused infill evaluation (infill_eval.hip): everything predict_impl / xgrad_impl do on the HOST between their
// launches, per tile of kTile = 128 query points and per model, plus the criterion itself:
//   k_infill_prepare   raw queries -> normalised k-major tile (algorithm.rs:254), non-finite points flagged and zeroed
//   k_infill_trend     mean = f beta + sum of the split partial sums (algorithm.rs:260-262); A = f - ft^T rt, Rq^T u = A, Rq D = u,
//                      var = sigma2 (1 - sum rt^2 + sum u^2) clamped at 0 (:272-278, 352-367); -D zero padded for the GEMM
//   k_infill_xgrad_finish   reduction of launch_xgrad's split partial sums, the trend Jacobian terms, un-normalisation (:510-727)
//   k_infill_mix       a surrogate with several experts: the responsibilities of its Gaussian mixture at the point (gmx_point.h)
//                      and infill_mix_math.h across the experts, into the surrogate's slot of the tables k_infill_combine reads
//   k_infill_combine   infill_math.h across the 1 + k models of a point: value and gradient of the minimised objective
//   k_infill_trend_mean, k_infill_xgrad_finish_mean, k_infill_mix_mean   the MEAN halves of the three kernels above, for a
//                      constraint surrogate whose variance nobody reads (EGX_CSTR_MEAN): no substitution, no s0 / sl, no
//                      second contraction -- the same sums in the same order, so the means keep the full sequence's bits
//   k_infill_cstr      the objective without the feasibility factor and the constraint values handed to the optimiser
//   k_infill_sgp_finish, k_infill_sgp_xgrad_finish   a SPARSE expert's tails (sgp_predict.hip's host arithmetic): the split sums of
//                      the mean, the clamped variance + noise with the host's roundings, the gradients (0 under the clamp);
//                      var / gvar == nullptr is their mean-only form
// None of them is matrix-shaped: they are latency-bound tails whose point is to keep the call free of host round trips.
// Every reduction runs in a fixed order that depends on the model alone, and a workgroup (or thread) owns one point: a point's
// result does not depend on its position in the tile nor on its companions.
// The sums that predict_impl / xgrad_impl form on the host -- f beta, the split partial sums, sum u^2, the forward substitution
// Rq^T u = A, the Jacobian terms; NOT the back substitution Rq D = u, whose updates reach an entry in descending instead of
// ascending order -- are formed here in the HOST'S ORDER and without FMA contraction (the host build has none): a model whose
// gamma is large against its predictions -- an ill-conditioned correlation matrix -- amplifies a reordering of the split sums
// to 1e-5 of the mean, and a caller may compare egx_infill_eval's parts with egx_gp_predict*.
#include "egx_internal.h"
#pragma clang fp contract(off)
#include "infill_math.h"
#include "infill_mix_math.h"
#include "gmx_point.h"
#include "trend_column.h"

namespace egx {

constexpr int kInfThreads = 256;

// one thread per point of the tile; xq: the tile's mt <= 128 raw rows (mt x d); par = x_mean (d) | x_std (d).
// blockIdx.x = member of a run of models (infill_runs.h) that read the SAME raw tile, each through its own normalisation into its
// own block of xqT, sq doubles behind the previous member's; the flags (and the cast rows) are member 0's to write: the
// objective's, which owns the call's flags, can only lead a run
__global__ __launch_bounds__(kTile) void k_infill_prepare(PosteriorBatchPtrs b, const double *__restrict__ xq, int mt, int d,
                                                          double *__restrict__ xqT_all, int64_t sq, int *__restrict__ flag_lead) {
    const double *__restrict__ par = b.par[blockIdx.x];
    double *__restrict__ xqT = xqT_all + (int64_t)blockIdx.x * sq;
    int *flag = blockIdx.x == 0 ? flag_lead : nullptr;
    const int a = threadIdx.x;
    int bad = 0;
    if (a < mt)
        for (int j = 0; j < d; j++) bad |= !isfinite(xq[(int64_t)a * d + j]);
    const bool live = a < mt && !bad;
    for (int j = 0; j < d; j++) xqT[(int64_t)j * kTile + a] = live ? (xq[(int64_t)a * d + j] - par[j]) / par[d + j] : 0.0;
    if (flag) flag[a] = bad;
}
// ... of a model that carries xtypes (mixint.h): the same with every coordinate cast where it is read.  A finite coordinate
// stays finite under the cast and a non-finite one non-finite, so the flags are those of the raw rows.  xcast (mt x d, or
// nullptr) receives the cast raw rows (a flagged point: its raw row), for k_infill_mix.
__global__ __launch_bounds__(kTile) void k_infill_prepare_mixint(PosteriorBatchPtrs b, const double *__restrict__ xq, int mt, int d,
                                                                 double *__restrict__ xqT_all, int64_t sq,
                                                                 int *__restrict__ flag_lead, double *__restrict__ xcast_lead) {
    const double *__restrict__ par = b.par[blockIdx.x];
    const mixint::Col *__restrict__ spec = b.spec[blockIdx.x];
    double *__restrict__ xqT = xqT_all + (int64_t)blockIdx.x * sq;
    int *flag = blockIdx.x == 0 ? flag_lead : nullptr;
    double *xcast = blockIdx.x == 0 ? xcast_lead : nullptr;
    const int a = threadIdx.x;
    const double *vals = mixint::table_values(spec, d);
    int bad = 0;
    if (a < mt)
        for (int j = 0; j < d; j++) bad |= !isfinite(xq[(int64_t)a * d + j]);
    const bool live = a < mt && !bad;
    for (int j = 0; j < d; j++) {
        const double c = live ? mixint::cast_coord(spec, vals, xq + (int64_t)a * d, 1, j) : 0.0;
        xqT[(int64_t)j * kTile + a] = live ? (c - par[j]) / par[d + j] : 0.0;
        if (xcast && a < mt) xcast[(int64_t)a * d + j] = live ? c : xq[(int64_t)a * d + j];
    }
    if (flag) flag[a] = bad;
}

struct TrendArgs {
    int p, rp, msplit, want_d;
    const double *xqT;    // d x 128 normalised tile
    const int *fidx;      // 2 p: coordinates of regression column l (-1: 1.0)
    const double *beta;   // p
    const double *R;      // Rq (p x p row-major, upper)
    const double *Rt;     // Rq^T (p x p row-major)
    const double *racc;   // msplit x 128 partial sums r . gamma
    const double *s0;     // 128: sum rt^2
    const double *sl;     // 128 x p: ft^T rt
    double sigma2, y_mean, y_std;
    double *mean, *var;   // 128 each (this tile of this model)
    double *dneg;         // 128 x rp: -D, zero padded (want_d)
};
// the members of a run (infill_runs.h), by value: blockIdx.y = member, a workgroup serves one point of ONE member
struct TrendBatch {
    TrendArgs m[kLockstepMax];
};

// One workgroup per point (p reaches 561 for the quadratic trend at d = 32: Rq is streamed from L2 row by row).
// LDS: s[p] (A, then u, then D), diag[p], prod[p] (f_l beta_l), part[msplit]; thread 0 adds them in predict_impl's order.
__global__ __launch_bounds__(kInfThreads) void k_infill_trend(TrendBatch gb) {
    const TrendArgs &g = gb.m[blockIdx.y];
    extern __shared__ double lds[];
    const int p = g.p, a = blockIdx.x, t = threadIdx.x;
    double *s = lds, *diag = lds + p, *prod = lds + 2 * p, *part = lds + 3 * p;
    for (int l = t; l < p; l += kInfThreads) {
        const double f = trend_column(g.fidx, l, g.xqT, kTile, a);
        prod[l] = f * g.beta[l];
        s[l] = f - g.sl[(int64_t)a * p + l];
        diag[l] = g.R[(int64_t)l * p + l];
    }
    for (int sp = t; sp < g.msplit; sp += kInfThreads) part[sp] = g.racc[(int64_t)sp * kTile + a];
    __syncthreads();
    if (t == 0) {
        double fb = 0.0, rg = 0.0;
        for (int l = 0; l < p; l++) fb += prod[l];
        for (int sp = 0; sp < g.msplit; sp++) rg += part[sp];
        g.mean[a] = (fb + rg) * g.y_std + g.y_mean;
    }
    // Rq^T u = A: column by column (row i of Rq is contiguous); every s_j receives its subtractions in the order l = 0, 1, ...
    for (int i = 0; i < p; i++) {
        const double ui = s[i] / diag[i];
        __syncthreads();  // every thread has read s[i]
        if (t == 0) s[i] = ui;
        for (int j = i + 1 + t; j < p; j += kInfThreads) s[j] -= g.R[(int64_t)i * p + j] * ui;
        __syncthreads();
    }
    if (t == 0) {
        double usq = 0.0;
        for (int l = 0; l < p; l++) usq += s[l] * s[l];
        const double mse = g.sigma2 * (1.0 - g.s0[a] + usq);
        g.var[a] = mse < 0.0 ? 0.0 : mse;
    }
    if (!g.want_d) return;
    __syncthreads();
    // Rq D = u: from the last row up, column i of Rq is row i of Rq^T
    for (int i = p - 1; i >= 0; i--) {
        const double di = s[i] / diag[i];
        __syncthreads();
        if (t == 0) s[i] = di;
        for (int j = t; j < i; j += kInfThreads) s[j] -= g.Rt[(int64_t)i * p + j] * di;
        __syncthreads();
    }
    for (int l = t; l < g.rp; l += kInfThreads) g.dneg[(int64_t)a * g.rp + l] = l < p ? -s[l] : 0.0;
}

// The mean of k_infill_trend alone: prod[p], part[msplit] in LDS, thread 0 adds them in the same order.
__global__ __launch_bounds__(kInfThreads) void k_infill_trend_mean(TrendBatch gb) {
    const TrendArgs &g = gb.m[blockIdx.y];
    extern __shared__ double lds[];
    const int p = g.p, a = blockIdx.x, t = threadIdx.x;
    double *prod = lds, *part = lds + p;
    for (int l = t; l < p; l += kInfThreads) prod[l] = trend_column(g.fidx, l, g.xqT, kTile, a) * g.beta[l];
    for (int sp = t; sp < g.msplit; sp += kInfThreads) part[sp] = g.racc[(int64_t)sp * kTile + a];
    __syncthreads();
    if (t == 0) {
        double fb = 0.0, rg = 0.0;
        for (int l = 0; l < p; l++) fb += prod[l];
        for (int sp = 0; sp < g.msplit; sp++) rg += part[sp];
        g.mean[a] = (fb + rg) * g.y_std + g.y_mean;
    }
}

struct XgFinishArgs {
    int d, p, rp, nsplit;
    const double *xqT;
    const int *fidx;
    const double *beta;
    const double *dneg;     // 128 x rp (-D)
    const double *out_y;    // nsplit x 128 x d partial sums of the mean contraction
    const double *out_v;    // ... of the variance contraction
    const double *x_std;    // d
    double sigma2, y_std;
    double *gmean, *gvar;   // 128 x d each (this tile of this model)
};
struct XgFinishBatch {  // blockIdx.y = member of a run, as TrendBatch
    XgFinishArgs m[kLockstepMax];
};

// sum_l v_l d f_l / d x_k at the point's normalised coordinates (host_math.h regression_jac_dot); sign * v[l * 1]
__device__ inline double jac_dot(const XgFinishArgs &g, int a, int k, const double *v, double sign) {
    double acc = 0.0;
    for (int l = 1; l < g.p; l++) {
        const int ia = g.fidx[2 * l], ib = g.fidx[2 * l + 1];  // d (fa fb) / d x_k: the other factor (times 1.0 is exact)
        if (ia == k) acc += sign * v[l] * trend_factor(g.xqT, kTile, a, ib);
        if (ib == k) acc += sign * v[l] * trend_factor(g.xqT, kTile, a, ia);
    }
    return acc;
}

// One workgroup per point.  The partial sums of kc = kXgStage / nsplit coordinates at a time are staged in LDS by all threads;
// thread kk then adds the splits of its coordinate in order (xgrad_impl's reduce_out).
constexpr int kXgStage = 2048;
__global__ __launch_bounds__(kInfThreads) void k_infill_xgrad_finish(XgFinishBatch gb) {
    const XgFinishArgs &g = gb.m[blockIdx.y];
    __shared__ double st_y[kXgStage], st_v[kXgStage];
    const int a = blockIdx.x, t = threadIdx.x, d = g.d, ns = g.nsplit;
    int kc = kXgStage / ns;
    if (kc > kInfThreads) kc = kInfThreads;
    for (int k0 = 0; k0 < d; k0 += kc) {
        const int kn = d - k0 < kc ? d - k0 : kc;
        __syncthreads();
        for (int e = t; e < ns * kn; e += kInfThreads) {
            const int sp = e / kn, kk = e - sp * kn;
            const int64_t o = ((int64_t)sp * kTile + a) * d + k0 + kk;
            st_y[kk * ns + sp] = g.out_y[o];
            st_v[kk * ns + sp] = g.out_v[o];
        }
        __syncthreads();
        if (t < kn) {
            const int k = k0 + t;
            double sy = 0.0, sv = 0.0;
            for (int sp = 0; sp < ns; sp++) {
                sy += st_y[t * ns + sp];
                sv += st_v[t * ns + sp];
            }
            const double dfy = jac_dot(g, a, k, g.beta, 1.0);
            const double dfv = jac_dot(g, a, k, g.dneg + (int64_t)a * g.rp, -1.0);
            g.gmean[(int64_t)a * d + k] = (dfy + sy) * g.y_std / g.x_std[k];
            g.gvar[(int64_t)a * d + k] = 2.0 * g.sigma2 * (dfv + sv) / g.x_std[k];
        }
    }
}

// The gmean of k_infill_xgrad_finish alone (out_v, dneg, gvar are not read).
__global__ __launch_bounds__(kInfThreads) void k_infill_xgrad_finish_mean(XgFinishBatch gb) {
    const XgFinishArgs &g = gb.m[blockIdx.y];
    __shared__ double st_y[kXgStage];
    const int a = blockIdx.x, t = threadIdx.x, d = g.d, ns = g.nsplit;
    int kc = kXgStage / ns;
    if (kc > kInfThreads) kc = kInfThreads;
    for (int k0 = 0; k0 < d; k0 += kc) {
        const int kn = d - k0 < kc ? d - k0 : kc;
        __syncthreads();
        for (int e = t; e < ns * kn; e += kInfThreads) {
            const int sp = e / kn, kk = e - sp * kn;
            st_y[kk * ns + sp] = g.out_y[((int64_t)sp * kTile + a) * d + k0 + kk];
        }
        __syncthreads();
        if (t < kn) {
            const int k = k0 + t;
            double sy = 0.0;
            for (int sp = 0; sp < ns; sp++) sy += st_y[t * ns + sp];
            const double dfy = jac_dot(g, a, k, g.beta, 1.0);
            g.gmean[(int64_t)a * d + k] = (dfy + sy) * g.y_std / g.x_std[k];
        }
    }
}

// ---- a SPARSE expert's tails (sgp_predict.hip's host arithmetic per tile) ---------------------------------------------------
// One lane per point of the tile (two waves).  mean = the msplit partial sums of K(x, z) . (sigma2 vec) added in split order
// (the vector carries sigma2: egx_sgp's resident `vec`); var = max(sigma2 - sigma2 (p2 + s q2), 1e-15) + noise with the roundings
// of sgp_query's host loop, so the clamp falls where egx_sgp_predict_var's does.  A flagged point was zeroed by the prepare
// kernel and is evaluated like any other (the criterion kernels answer for it), as in k_infill_trend.
__global__ __launch_bounds__(kTile) void k_infill_sgp_finish(const double *__restrict__ racc, int msplit, const double *__restrict__ p2,
                                                            const double *__restrict__ q2, double sigma2, double noise, int vfe,
                                                            double *__restrict__ mean, double *__restrict__ var) {
    const int a = threadIdx.x;
    double rg = 0.0;
    for (int sp = 0; sp < msplit; sp++) rg = __dadd_rn(rg, racc[(int64_t)sp * kTile + a]);
    mean[a] = rg;
    if (!var) return;
    const double quad = vfe ? __dmul_rn(sigma2, __dadd_rn(p2[a], q2[a])) : __dmul_rn(sigma2, __dsub_rn(p2[a], q2[a]));
    double v = __dsub_rn(sigma2, quad);
    if (v < 1e-15) v = 1e-15;
    var[a] = __dadd_rn(v, noise);
}

// One thread per (point, coordinate) of the tile: the nsplit partial sums of the two contractions added in split order, then
// gmean = 1 * sum (the weights carry sigma2), gvar = gv_scale * sum -- exactly 0 where the raw variance is below the clamp
// (the decision of k_infill_sgp_finish, formed with the same roundings).  out_v / gvar nullptr: the mean half alone.
__global__ __launch_bounds__(kInfThreads) void k_infill_sgp_xgrad_finish(const double *__restrict__ out_y,
                                                                        const double *__restrict__ out_v, int nsplit, int d,
                                                                        const double *__restrict__ p2, const double *__restrict__ q2,
                                                                        double sigma2, int vfe, double gv_scale,
                                                                        double *__restrict__ gmean, double *__restrict__ gvar) {
    const int i = blockIdx.x * kInfThreads + threadIdx.x;
    if (i >= kTile * d) return;
    const int a = i / d;
    const int64_t s_split = (int64_t)kTile * d;
    double sy = 0.0;
    for (int sp = 0; sp < nsplit; sp++) sy = __dadd_rn(sy, out_y[(int64_t)sp * s_split + i]);
    gmean[i] = sy;
    if (!gvar) return;
    double sv = 0.0;
    for (int sp = 0; sp < nsplit; sp++) sv = __dadd_rn(sv, out_v[(int64_t)sp * s_split + i]);
    const double quad = vfe ? __dmul_rn(sigma2, __dadd_rn(p2[a], q2[a])) : __dmul_rn(sigma2, __dsub_rn(p2[a], q2[a]));
    gvar[i] = __dsub_rn(sigma2, quad) < 1e-15 ? 0.0 : __dmul_rn(gv_scale, sv);
}

int launch_infill_sgp_finish(hipStream_t s, const double *racc, int msplit, const double *p2, const double *q2, double sigma2,
                             double noise, int vfe, double *mean, double *var) {
    if (msplit < 1 || !racc || !mean || (var && (!p2 || !q2))) {
        set_error("infill: bad arguments of the sparse expert's finish");
        return EGX_ERR_INVALID_VALUE;
    }
    hipLaunchKernelGGL(k_infill_sgp_finish, dim3(1), dim3(kTile), 0, s, racc, msplit, p2, q2, sigma2, noise, vfe, mean, var);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_infill_sgp_xgrad_finish(hipStream_t s, const double *out_y, const double *out_v, int nsplit, int d, const double *p2,
                                   const double *q2, double sigma2, int vfe, double gv_scale, double *gmean, double *gvar) {
    if (nsplit < 1 || d < 1 || !out_y || !gmean || (gvar && (!out_v || !p2 || !q2))) {
        set_error("infill: bad arguments of the sparse expert's gradient finish");
        return EGX_ERR_INVALID_VALUE;
    }
    hipLaunchKernelGGL(k_infill_sgp_xgrad_finish, dim3((unsigned)((kTile * d + kInfThreads - 1) / kInfThreads)), dim3(kInfThreads), 0,
                       s, out_y, out_v, nsplit, d, p2, q2, sigma2, vfe, gv_scale, gmean, gvar);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

// A surrogate that is a mixture of k >= 2 experts, after the experts' sequences have written their tables for the tile: one
// lane per point, 64-lane workgroups (kTile / 64 of them).  The lane's raw coordinates (a flagged point: zeros, as the experts
// got), its responsibilities p and the scratch of the derivative (z, v': d each; u: k) live in LDS rows of odd stride; the
// mixture's means, scaled precision factors and par are read at wave-uniform addresses.  Expert c of point a: emean / evar at
// c * estride + a, egmean / egvar at (c * estride + a) * d.  dp (kTile x k x d): d p_c / d x, computed when not nullptr (smooth
// gradients need it); probas (kTile x k): a copy of p for egx_infill_eval_experts, or nullptr.
__global__ __launch_bounds__(64) void k_infill_mix(const double *__restrict__ xq, const int *__restrict__ flag, int mt, int d, int k,
                                                  int smooth, int want_g, const double *__restrict__ means,
                                                  const double *__restrict__ precs, const double *__restrict__ par,
                                                  const double *__restrict__ emean, const double *__restrict__ evar,
                                                  const double *__restrict__ egmean, const double *__restrict__ egvar,
                                                  int64_t estride, double *__restrict__ mean, double *__restrict__ var,
                                                  double *__restrict__ gmean, double *__restrict__ gvar, double *__restrict__ dp,
                                                  double *__restrict__ probas) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int q0 = blockIdx.x * 64, lane = threadIdx.x, ds = d | 1, ks = k | 1;
    const int rows = mt - q0 < 64 ? mt - q0 : 64;
    if (rows <= 0) return;
    double *xs = sm, *ps = xs + 64 * ds, *zs = ps + 64 * ks, *vps = zs + 64 * ds, *us = vps + 64 * ds;
    for (int e = lane; e < rows * d; e += 64) {
        const int i = e / d, j = e - i * d;
        xs[i * ds + j] = flag[q0 + i] ? 0.0 : xq[(int64_t)q0 * d + e];
    }
    __syncthreads();
    if (lane >= rows) return;
    const int64_t a = q0 + lane;
    const double *x = xs + lane * ds;
    double *p = ps + lane * ks, *dpa = dp ? dp + a * k * d : nullptr;
    gmx_probas_point(x, d, k, means, precs, par, p);
    if (probas)
        for (int c = 0; c < k; c++) probas[a * k + c] = p[c];
    if (dpa) gmx_probas_deriv_point(x, zs + lane * ds, vps + lane * ds, us + lane * ks, d, k, means, precs, par, dpa);
    infill::mix_value(smooth != 0, k, p, 1, emean + a, evar + a, estride, mean + a, var + a);
    if (want_g)
        infill::mix_grad(smooth != 0, k, d, p, 1, dpa, d, emean + a, evar + a, estride, egmean + a * d, egvar + a * d, estride * d,
                         gmean + a * d, gvar + a * d);
}

// The mean half of k_infill_mix: the same responsibilities, mix_mean / mix_grad_mean; evar / egvar / var / gvar do not exist.
__global__ __launch_bounds__(64) void k_infill_mix_mean(const double *__restrict__ xq, const int *__restrict__ flag, int mt, int d,
                                                       int k, int smooth, int want_g, const double *__restrict__ means,
                                                       const double *__restrict__ precs, const double *__restrict__ par,
                                                       const double *__restrict__ emean, const double *__restrict__ egmean,
                                                       int64_t estride, double *__restrict__ mean, double *__restrict__ gmean,
                                                       double *__restrict__ dp) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int q0 = blockIdx.x * 64, lane = threadIdx.x, ds = d | 1, ks = k | 1;
    const int rows = mt - q0 < 64 ? mt - q0 : 64;
    if (rows <= 0) return;
    double *xs = sm, *ps = xs + 64 * ds, *zs = ps + 64 * ks, *vps = zs + 64 * ds, *us = vps + 64 * ds;
    for (int e = lane; e < rows * d; e += 64) {
        const int i = e / d, j = e - i * d;
        xs[i * ds + j] = flag[q0 + i] ? 0.0 : xq[(int64_t)q0 * d + e];
    }
    __syncthreads();
    if (lane >= rows) return;
    const int64_t a = q0 + lane;
    const double *x = xs + lane * ds;
    double *p = ps + lane * ks, *dpa = dp ? dp + a * k * d : nullptr;
    gmx_probas_point(x, d, k, means, precs, par, p);
    if (dpa) gmx_probas_deriv_point(x, zs + lane * ds, vps + lane * ds, us + lane * ks, d, k, means, precs, par, dpa);
    mean[a] = infill::mix_mean(smooth != 0, k, p, 1, emean + a, estride);
    if (want_g) infill::mix_grad_mean(smooth != 0, k, d, p, 1, dpa, d, emean + a, estride, egmean + a * d, estride * d, gmean + a * d);
}

// one thread per point of the call; model j of point i at j * mstride + i (mean, var) and (j * mstride + i) * d (gradients)
__global__ __launch_bounds__(kInfThreads) void k_infill_combine(infill::Params prm, int k, int d, int64_t m, int64_t mstride,
                                                               const double *__restrict__ mean, const double *__restrict__ var,
                                                               const double *__restrict__ gmean, const double *__restrict__ gvar,
                                                               const double *__restrict__ tol, const int *__restrict__ flag,
                                                               double *__restrict__ value, double *__restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * kInfThreads + threadIdx.x;
    if (i >= m) return;
    if (flag[i]) {  // NaN in the point: +inf, gradient 0 (solver_infill_optim.rs:87-90)
        value[i] = INFINITY;
        if (grad)
            for (int c = 0; c < d; c++) grad[i * d + c] = 0.0;
        return;
    }
    value[i] = infill::objective(prm, k, mean + i, var + i, mstride, tol);
    if (grad)
        infill::objective_grad(prm, k, d, mean + i, var + i, mstride, gmean + i * d, gvar + i * d, mstride * d, tol, grad + i * d, 1);
}

// What the optimiser is handed when the constraint surrogates are NOT folded into the objective (EGX_CSTR_MEAN / _UTB), one
// thread per point: value = the objective of the objective model alone (k_infill_scale_terms' base: prm.feasibility = 1, no
// factor), cstr[i * k + j] = infill::cstr_value of constraint model j + 1, and optionally their gradients grad (m x d) and
// gcstr (m x k x d).  var / gvar of the constraint models are read under UTB only.  A flagged point: +inf, +inf, zeros.
__global__ __launch_bounds__(kInfThreads) void k_infill_cstr(infill::Params prm, int strategy, int k, int d, int64_t m,
                                                            int64_t mstride, const double *__restrict__ mean,
                                                            const double *__restrict__ var, const double *__restrict__ gmean,
                                                            const double *__restrict__ gvar, const double *__restrict__ scale,
                                                            const int *__restrict__ flag, double *__restrict__ value,
                                                            double *__restrict__ cstr, double *__restrict__ grad,
                                                            double *__restrict__ gcstr) {
    const int64_t i = (int64_t)blockIdx.x * kInfThreads + threadIdx.x;
    if (i >= m) return;
    const bool bad = flag[i] != 0, utb = strategy == infill::kCstrUtb;
    if (value) value[i] = bad ? INFINITY : infill::objective(prm, 0, mean + i, var + i, mstride, nullptr);
    if (grad) {
        if (bad)
            for (int c = 0; c < d; c++) grad[i * d + c] = 0.0;
        else
            infill::objective_grad(prm, 0, d, mean + i, var + i, mstride, gmean + i * d, gvar + i * d, mstride * d, nullptr,
                                   grad + i * d, 1);
    }
    for (int j = 1; j <= k; j++) {
        const int64_t o = j * mstride + i;
        const double v = utb ? var[o] : 0.0;
        if (cstr) cstr[i * k + j - 1] = bad ? INFINITY : infill::cstr_value(strategy, mean[o], v, scale[j - 1]);
        if (gcstr)
            for (int c = 0; c < d; c++)
                gcstr[(i * k + j - 1) * d + c] =
                    bad ? 0.0 : infill::cstr_grad(strategy, v, gmean[o * d + c], utb ? gvar[o * d + c] : 0.0, scale[j - 1]);
    }
}

// The terms of the scaling pass (egx_infill_scaling), one thread per point, with the text k_infill_combine runs:
//   ei[i]   EI(x_i) at the handle's fmin and sigma_weight (compute_wb2s_scale)                      -- when ei != nullptr
//   base[i] the objective WITHOUT the feasibility factor, fac[i] that factor (pofs, or logpofs for LogEI; 1 / 0 without
//           constraint models): the host replaces a NaN / infinite base by 1 and forms base * fac or base - fac, the one
//           IEEE operation infill::objective ends with                                              -- when base != nullptr
// A flagged (non-finite) point has base = +inf and the neutral factor.
__global__ __launch_bounds__(kInfThreads) void k_infill_scale_terms(infill::Params prm, int k, int64_t m, int64_t mstride,
                                                                   const double *__restrict__ mean, const double *__restrict__ var,
                                                                   const double *__restrict__ tol, const int *__restrict__ flag,
                                                                   double *__restrict__ ei, double *__restrict__ base,
                                                                   double *__restrict__ fac) {
    const int64_t i = (int64_t)blockIdx.x * kInfThreads + threadIdx.x;
    if (i >= m) return;
    const bool is_log = prm.kind == infill::kLogEI;
    const bool bad = flag[i] != 0;
    if (ei) ei[i] = bad ? 0.0 : infill::ei_value(mean[i], var[i], prm.fmin, prm.sigma_weight);
    if (base) {
        base[i] = bad ? INFINITY : infill::objective(prm, 0, mean + i, var + i, mstride, tol);
        if (k == 0 || bad)
            fac[i] = is_log ? 0.0 : 1.0;
        else
            fac[i] = is_log ? infill::logpofs(k, mean + i, var + i, mstride, tol) : infill::pofs(k, mean + i, var + i, mstride, tol);
    }
}

int launch_infill_scale_terms(hipStream_t s, const infill::Params &prm, int k, int64_t m, int64_t mstride, const double *mean,
                              const double *var, const double *tol, const int *flag, double *ei, double *base, double *fac) {
    if (m <= 0) return EGX_SUCCESS;
    hipLaunchKernelGGL(k_infill_scale_terms, dim3((unsigned)((m + kInfThreads - 1) / kInfThreads)), dim3(kInfThreads), 0, s, prm, k,
                       m, mstride, mean, var, tol, flag, ei, base, fac);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

static bool run_count_ok(int count) {
    if (count >= 1 && count <= kLockstepMax) return true;
    set_error("infill: run length out of range");
    return false;
}

int launch_infill_prepare(hipStream_t s, const PosteriorBatch &pb, const double *xq, int mt, int d, double *xqT, int *flag,
                          double *xcast) {
    if (!run_count_ok(pb.count)) return EGX_ERR_INVALID_VALUE;
    const dim3 grid((unsigned)pb.count);
    if (pb.ptrs.spec[0]) hipLaunchKernelGGL(k_infill_prepare_mixint, grid, dim3(kTile), 0, s, pb.ptrs, xq, mt, d, xqT, pb.sq, flag, xcast);
    else hipLaunchKernelGGL(k_infill_prepare, grid, dim3(kTile), 0, s, pb.ptrs, xq, mt, d, xqT, pb.sq, flag);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

static TrendArgs trend_args(const InfillTrend &t, bool mean_only) {
    TrendArgs g{};
    g.p = t.p, g.rp = t.rp, g.msplit = t.msplit, g.want_d = !mean_only && t.dneg != nullptr;
    g.xqT = t.xqT, g.fidx = t.fidx, g.beta = t.beta, g.racc = t.racc;
    g.y_mean = t.y_mean, g.y_std = t.y_std, g.mean = t.mean;
    if (mean_only) return g;
    g.R = t.R, g.Rt = t.Rt, g.s0 = t.s0, g.sl = t.sl;
    g.sigma2 = t.sigma2;
    g.var = t.var, g.dneg = t.dneg;
    return g;
}
// the members of a run have one trend and one split count: the launch's LDS is member 0's
static int launch_trend(hipStream_t s, const InfillTrend *t, int count, bool mean_only) {
    if (!run_count_ok(count)) return EGX_ERR_INVALID_VALUE;
    const size_t lds = sizeof(double) * ((size_t)(mean_only ? 1 : 3) * t[0].p + (size_t)t[0].msplit);
    if (lds > 65536) {
        set_error("infill: more than 2560 regression columns");
        return EGX_ERR_UNSUPPORTED;
    }
    TrendBatch gb{};
    for (int j = 0; j < count; j++) gb.m[j] = trend_args(t[j], mean_only);
    const dim3 grid(kTile, (unsigned)count);
    if (mean_only) hipLaunchKernelGGL(k_infill_trend_mean, grid, dim3(kInfThreads), lds, s, gb);
    else hipLaunchKernelGGL(k_infill_trend, grid, dim3(kInfThreads), lds, s, gb);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}
int launch_infill_trend(hipStream_t s, const InfillTrend *t, int count) { return launch_trend(s, t, count, false); }
int launch_infill_trend_mean(hipStream_t s, const InfillTrend *t, int count) { return launch_trend(s, t, count, true); }

static int launch_xgrad_finish(hipStream_t s, const InfillTrend *t, const InfillFinish *f, int count, int d, int nsplit, bool mean_only) {
    if (!run_count_ok(count)) return EGX_ERR_INVALID_VALUE;
    if (nsplit < 1 || nsplit > kXgStage) {
        set_error("infill: split count of the x-gradient contraction out of range");
        return EGX_ERR_INVALID_VALUE;
    }
    XgFinishBatch gb{};
    for (int j = 0; j < count; j++) {
        XgFinishArgs &g = gb.m[j];
        g.d = d, g.p = t[j].p, g.rp = t[j].rp, g.nsplit = nsplit;
        g.xqT = t[j].xqT, g.fidx = t[j].fidx, g.beta = t[j].beta, g.out_y = f[j].out_y, g.x_std = f[j].x_std;
        g.y_std = t[j].y_std, g.gmean = f[j].gmean;
        if (mean_only) continue;
        g.dneg = t[j].dneg, g.out_v = f[j].out_v;
        g.sigma2 = t[j].sigma2, g.gvar = f[j].gvar;
    }
    const dim3 grid(kTile, (unsigned)count);
    if (mean_only) hipLaunchKernelGGL(k_infill_xgrad_finish_mean, grid, dim3(kInfThreads), 0, s, gb);
    else hipLaunchKernelGGL(k_infill_xgrad_finish, grid, dim3(kInfThreads), 0, s, gb);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}
int launch_infill_xgrad_finish(hipStream_t s, const InfillTrend *t, const InfillFinish *f, int count, int d, int nsplit) {
    return launch_xgrad_finish(s, t, f, count, d, nsplit, false);
}
int launch_infill_xgrad_finish_mean(hipStream_t s, const InfillTrend *t, const InfillFinish *f, int count, int d, int nsplit) {
    return launch_xgrad_finish(s, t, f, count, d, nsplit, true);
}

int launch_infill_cstr(hipStream_t s, const infill::Params &prm, int strategy, int k, int d, int64_t m, int64_t mstride,
                       const double *mean, const double *var, const double *gmean, const double *gvar, const double *scale,
                       const int *flag, double *value, double *cstr, double *grad, double *gcstr) {
    if (m <= 0) return EGX_SUCCESS;
    if ((strategy != infill::kCstrMean && strategy != infill::kCstrUtb) || ((grad || gcstr) && !gmean) ||
        ((grad || (gcstr && strategy == infill::kCstrUtb)) && !gvar) || (k > 0 && (cstr || gcstr) && !scale)) {
        set_error("infill: bad arguments of the constraint evaluation");
        return EGX_ERR_INVALID_VALUE;
    }
    infill::Params p = prm;
    p.feasibility = 1;
    hipLaunchKernelGGL(k_infill_cstr, dim3((unsigned)((m + kInfThreads - 1) / kInfThreads)), dim3(kInfThreads), 0, s, p, strategy, k,
                       d, m, mstride, mean, var, gmean, gvar, scale, flag, value, cstr, grad, gcstr);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_infill_mix_mean(hipStream_t s, const InfillMix &g) {
    const size_t lds = infill_mix_lds_bytes(g.d, g.k);
    if (g.k < 2 || g.mt < 1 || g.mt > kTile || lds > kInfillMixMaxLds || (g.smooth && g.want_g && !g.dp)) {
        set_error("infill: bad arguments of the mixture recombination");
        return EGX_ERR_INVALID_VALUE;
    }
    if (lds > 64 * 1024)
        EGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_infill_mix_mean),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_infill_mix_mean, dim3(kTile / 64), dim3(64), lds, s, g.xq, g.flag, g.mt, g.d, g.k, g.smooth ? 1 : 0,
                       g.want_g ? 1 : 0, g.means, g.precs, g.par, g.emean, g.egmean, g.estride, g.mean, g.gmean, g.dp);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

size_t infill_mix_lds_bytes(int d, int k) { return sizeof(double) * 64 * (size_t)(3 * (d | 1) + 2 * (k | 1)); }

int launch_infill_mix(hipStream_t s, const InfillMix &g) {
    const size_t lds = infill_mix_lds_bytes(g.d, g.k);
    if (g.k < 2 || g.mt < 1 || g.mt > kTile || lds > kInfillMixMaxLds || (g.smooth && g.want_g && !g.dp)) {
        set_error("infill: bad arguments of the mixture recombination");
        return EGX_ERR_INVALID_VALUE;
    }
    if (lds > 64 * 1024)
        EGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_infill_mix), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)lds));
    hipLaunchKernelGGL(k_infill_mix, dim3(kTile / 64), dim3(64), lds, s, g.xq, g.flag, g.mt, g.d, g.k, g.smooth ? 1 : 0,
                       g.want_g ? 1 : 0, g.means, g.precs, g.par, g.emean, g.evar, g.egmean, g.egvar, g.estride, g.mean, g.var,
                       g.gmean, g.gvar, g.dp, g.probas);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_infill_combine(hipStream_t s, const infill::Params &prm, int k, int d, int64_t m, int64_t mstride, const double *mean,
                          const double *var, const double *gmean, const double *gvar, const double *tol, const int *flag,
                          double *value, double *grad) {
    if (m <= 0) return EGX_SUCCESS;
    hipLaunchKernelGGL(k_infill_combine, dim3((unsigned)((m + kInfThreads - 1) / kInfThreads)), dim3(kInfThreads), 0, s, prm, k, d,
                       m, mstride, mean, var, gmean, gvar, tol, flag, value, grad);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

}  // namespace egx
