// Kernels of the PENDING points of an infill handle (infill_pending.hip, pending_math.h): a fitted model conditioned on q <= 16
// virtual observations without a refit.  Per tile of kTile = 128 queries and per conditioned model, right after the model's own
// tile sequence (expert_tile, infill_eval.hip), while the normalised tile is still in place:
//   k_pending_cross    the rectangular multi-column contraction over Z = the training points followed by the pending ones,
//                          c[a, v]             = sum_j r(x_a, Z_j) W^[j, v]
//                          d c[a, v] / d x_ak  = sum_j d_k r(x_a, Z_j) W^[j, v]
//                      W^ = [W_v ; I_q] ((n + q) x 16, a row contiguous): column v holds the weights -(R^-1 r_v + R^-1 F D_v) that
//                      posterior_weights / posterior_weights_trend gave when point v was pushed, and the identity below them
//                      brings in the direct term r(x, x_v) and its gradient from the same sum.  The organisation is k_xgrad's
//                      (kernels_corr.hip): one lane per query, 64-point slabs of Z broadcast from LDS, the range split over
//                      grid.y.  The correlation and the d gradient factors of a (query, point) pair are formed ONCE and applied
//                      to the QV columns of the pass (their weights staged with the slab: a row of W^ is contiguous): QV (DK + 1)
//                      accumulators per lane, ceil(q / QV) passes; the partial sums are q wide.
//   k_pending_finish   one workgroup per point: the splits added in order, + f(x)^T t_v and (d f / d x)^T t_v (t_v = D_v, streamed:
//                      p reaches 561), then pending::point_terms and the tile's mean / var / gmean / gvar rewritten IN PLACE.
//                      var == nullptr is its mean-only twin (a constraint surrogate under EGX_CSTR_MEAN: the mean shift alone).
// A lane or a workgroup owns a point and every order of summation depends on the model and q alone: a point's bits do not depend
// on its companions.
//
// Nor on the INSTANCE of k_pending_cross that formed them: the values-only instance (<.., 1, false>), the gradient instances
// (DK = 8 / 16) and the three pass widths QV must give a column the same value sum bit for bit (InfillObjective.value against
// value_and_grad, a narrow last pass against a full one).  With the compiler free to fuse a multiply into an add ACROSS
// statements, which pairs it fuses depends on what else an instance computes from the same operands (xgrad_factor shares the
// subexpressions of PairAcc::add), and value() differed from value_and_grad() in the last bits at d > 8.  So this file is
// compiled with contraction inside one expression only -- a function of the source text, the same in every instance.  The
// pragma comes before the headers: it has to cover PairAcc, exp_nonpos and xgrad_factor as they are parsed.
#pragma clang fp contract(on)
#include "egx_internal.h"
#include "corr_pair.h"
#include "pending_math.h"
#include "trend_column.h"

namespace egx {

constexpr int kPcThreads = 128;
constexpr int kPfThreads = 256;
constexpr size_t kPcLdsMax = 160 * 1024;  // LDS of one CU (gfx950)

template <int CORR, int QV, int DK, bool GRAD>
__global__ __launch_bounds__(kPcThreads) void k_pending_cross(const double *__restrict__ xqT, const double *__restrict__ ZT,
                                                              int64_t ldz, int nz, int d, const double *__restrict__ coef,
                                                              int hcols, const double *__restrict__ W, int v0, int q,
                                                              int slabs_per_split, double *__restrict__ outc,
                                                              double *__restrict__ outg) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int LDW = pending::kLd;
    double *xa = sm;                    // [d][kPcThreads]
    double *xj = sm + d * kPcThreads;   // [d][64]
    double *cs = xj + d * 64;           // [d * hcols]
    double *ws = cs + d * hcols;        // [64][QV]: the slab's rows of W^, the pass's columns
    const int tid = threadIdx.x, a = tid;  // one tile: grid.x == 1
    for (int k = 0; k < d; k++) xa[k * kPcThreads + tid] = xqT[(int64_t)k * kTile + a];
    for (int e = tid; e < d * hcols; e += kPcThreads) cs[e] = coef[e];
    const int j_lo = blockIdx.y * slabs_per_split * 64;
    int j_hi = j_lo + slabs_per_split * 64;
    if (j_hi > nz) j_hi = nz;
    const int64_t row = ((int64_t)blockIdx.y * kTile + a) * q + v0;  // the partial sums are q wide, not 16: dense for the finish
    for (int k0 = 0; k0 < d; k0 += DK) {
        double cv[QV], acc[QV][DK], xr[DK];
#pragma unroll
        for (int v = 0; v < QV; v++) {
            cv[v] = 0.0;
#pragma unroll
            for (int kk = 0; kk < DK; kk++) acc[v][kk] = 0.0;
        }
#pragma unroll
        for (int kk = 0; kk < DK; kk++) xr[kk] = (k0 + kk < d) ? xa[(k0 + kk) * kPcThreads + tid] : 0.0;
        for (int j0 = j_lo; j0 < j_hi; j0 += 64) {
            __syncthreads();
            for (int e = tid; e < d * 64; e += kPcThreads) xj[e] = ZT[(int64_t)(e >> 6) * ldz + j0 + (e & 63)];
            for (int e = tid; e < 64 * QV; e += kPcThreads) {  // (a row of W^ is contiguous; rows beyond the n + q points: 0)
                const int jr = j0 + e / QV;
                ws[e] = jr < nz ? W[(int64_t)jr * LDW + v0 + e % QV] : 0.0;
            }
            __syncthreads();
            const int jn = (j_hi - j0 < 64) ? (j_hi - j0) : 64;
            for (int jj = 0; jj < jn; jj++) {
                PairAcc<CORR> pa;
                for (int k = 0; k < d; k++) pa.add(xa[k * kPcThreads + tid] - xj[k * 64 + jj], cs + k * hcols, hcols);
                const double r = pa.value();
                const double *w = ws + jj * QV;  // wave-uniform: QV contiguous weights, broadcast from LDS
                double rw[QV];
#pragma unroll
                for (int v = 0; v < QV; v++) {
                    rw[v] = r * w[v];
                    cv[v] += rw[v];
                }
                if (GRAD) {
#pragma unroll
                    for (int kk = 0; kk < DK; kk++)
                        if (k0 + kk < d) {
                            const double g = xgrad_factor<CORR>(xr[kk] - xj[(k0 + kk) * 64 + jj], cs + (k0 + kk) * hcols, hcols);
#pragma unroll
                            for (int v = 0; v < QV; v++) acc[v][kk] = __builtin_fma(rw[v], g, acc[v][kk]);
                        }
                }
            }
        }
        if (k0 == 0) {
#pragma unroll
            for (int v = 0; v < QV; v++)
                if (v0 + v < q) outc[row + v] = cv[v];
        }
        if (!GRAD) break;
#pragma unroll
        for (int v = 0; v < QV; v++)
#pragma unroll
            for (int kk = 0; kk < DK; kk++)
                if (k0 + kk < d && v0 + v < q) outg[(row + v) * d + k0 + kk] = acc[v][kk];
    }
}

struct PendFinishArgs {
    int q, d, p, nsplit_c, nsplit_g;
    int64_t sc_v, sc_sp, sc_a;   // outc[v sc_v + sp sc_sp + a sc_a]
    int64_t sg_v, sg_sp, sg_a;   // outg[v sg_v + sp sg_sp + a sg_a + k]
    const double *xqT;     // d x kTile normalised tile
    const int *fidx;       // 2 p
    const double *tv;      // 16 x p: t_v = D_v
    const double *small;   // L (16 x 16) | alpha (16)
    const double *outc;    // the partial sums of c, fused (nsplit x kTile x q) or composed (q x msplit x kTile)
    const double *outg;    // ... of d c / d x, fused (nsplit x kTile x q x d) or composed (q x nsplit x kTile x d), or nullptr
    const double *x_std;   // d
    double sigma2, sigma2c, y_std;
    double *mean, *var, *gmean, *gvar;  // the tile's entries of the tables; var / gvar nullptr: the mean-only twin
    double *emit;          // kTile x 16: the cross-covariances themselves, nothing rewritten (a push), or nullptr
};

__global__ __launch_bounds__(kPfThreads) void k_pending_finish(PendFinishArgs g) {
    constexpr int LD = pending::kLd;
    __shared__ double sL[LD * LD], sal[LD], sc[LD], sb[LD];
    extern __shared__ double sg[];  // d c_v / d x_k of the point, [v][k]: 16 d doubles
    const int a = blockIdx.x, t = threadIdx.x, q = g.q, d = g.d, p = g.p;
    for (int e = t; e < LD * LD; e += kPfThreads) sL[e] = g.small[e];
    if (t < LD) sal[t] = g.small[LD * LD + t];
    if (t < q) {
        double c = 0.0;
        for (int sp = 0; sp < g.nsplit_c; sp++) c += g.outc[t * g.sc_v + sp * g.sc_sp + a * g.sc_a];
        double ft = 0.0;
        for (int l = 0; l < p; l++) ft += trend_column(g.fidx, l, g.xqT, kTile, a) * g.tv[(int64_t)t * p + l];
        sc[t] = c + ft;
    }
    __syncthreads();
    if (g.emit) {
        if (t < LD) g.emit[(int64_t)a * LD + t] = t < q ? sc[t] : 0.0;
        return;
    }
    if (t == 0) {
        double dm, quad;
        pending::point_terms(sL, sal, q, sc, &dm, &quad, g.gvar ? sb : nullptr);
        g.mean[a] = pending::cond_mean(g.mean[a], g.y_std, dm);
        if (g.var) g.var[a] = pending::cond_var(g.var[a], g.sigma2, g.sigma2c, quad);
    }
    if (!g.gmean) return;
    for (int e = t; e < q * d; e += kPfThreads) {
        const int v = e / d, k = e - v * d;
        double s = 0.0;
        for (int sp = 0; sp < g.nsplit_g; sp++) s += g.outg[v * g.sg_v + sp * g.sg_sp + a * g.sg_a + k];
        const double *tv = g.tv + (int64_t)v * p;
        double jf = 0.0;
        for (int l = 1; l < p; l++) {  // d (fa fb) / d x_k: the other factor
            const int ia = g.fidx[2 * l], ib = g.fidx[2 * l + 1];
            if (ia == k) jf += tv[l] * trend_factor(g.xqT, kTile, a, ib);
            if (ib == k) jf += tv[l] * trend_factor(g.xqT, kTile, a, ia);
        }
        sg[v * d + k] = s + jf;
    }
    __syncthreads();
    for (int k = t; k < d; k += kPfThreads) {
        double gc = 0.0, gb = 0.0;
        for (int v = 0; v < q; v++) {
            gc += sal[v] * sg[v * d + k];
            if (g.gvar) gb += sb[v] * sg[v * d + k];
        }
        const int64_t o = (int64_t)a * d + k;
        g.gmean[o] = pending::cond_gmean(g.gmean[o], g.y_std, g.x_std[k], gc);
        if (g.gvar) g.gvar[o] = pending::cond_gvar(g.gvar[o], g.sigma2, g.sigma2c, g.x_std[k], gb);
    }
}

// What a push keeps of the new point's own tile sequence (the point is query 0 of the tile): column v of W^ <- column 0 of the
// (n_pad x kTile) weight matrix, the identity entry below it, t_v <- -(-D) of row 0, its normalised coordinates into Z.  Wc is
// W^ once more, column-major (16 x ldz): the contiguous weight VECTORS the composed form hands to the existing kernels.
__global__ __launch_bounds__(256) void k_pending_capture(const double *__restrict__ Wt, const double *__restrict__ dneg,
                                                         const double *__restrict__ xqT, int n, int d, int p, int v,
                                                         double *__restrict__ W, double *__restrict__ Wc, double *__restrict__ tv,
                                                         double *__restrict__ ZT, int64_t ldz) {
    constexpr int LD = pending::kLd;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) W[(int64_t)i * LD + v] = Wc[(int64_t)v * ldz + i] = Wt[(int64_t)i * kTile];
    if (i < LD) W[(int64_t)(n + i) * LD + v] = Wc[(int64_t)v * ldz + n + i] = i == v ? 1.0 : 0.0;
    if (i < LD && i != v) Wc[(int64_t)i * ldz + n + v] = 0.0;
    if (i < LD && i != v) W[(int64_t)(n + v) * LD + i] = 0.0;
    if (i < p) tv[(int64_t)v * p + i] = -dneg[i];
    if (i < d) ZT[(int64_t)i * ldz + n + v] = xqT[(int64_t)i * kTile];
}

int launch_pending_capture(hipStream_t s, const double *Wt, const double *dneg, const double *xqT, int n, int d, int p, int v,
                           double *W, double *Wc, double *tv, double *ZT, int64_t ldz) {
    const int rows = std::max(std::max(n, p), std::max(d, pending::kLd));
    hipLaunchKernelGGL(k_pending_capture, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, Wt, dneg, xqT, n, d, p, v, W, Wc,
                       tv, ZT, ldz);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int pending_splits(int nz) {  // a function of the model and q alone: ~512 workgroups for the one tile of a launch
    const int slabs = (nz + 63) / 64;
    const int want = slabs < 512 ? slabs : 512;
    const int per = (slabs + want - 1) / want;
    return (slabs + per - 1) / per;
}

// outc: nsplit x kTile x q, outg: nsplit x kTile x q x d partial sums (outg == nullptr: values only); nz = n + q points in ZT
int launch_pending_cross(hipStream_t s, int corr, const double *xqT, const double *ZT, int64_t ldz, int nz, int d, const double *coef,
                         int hcols, const double *W, int q, int nsplit, double *outc, double *outg) {
    if (q < 1 || q > pending::kMaxPending || d < 1 || d > kPendingMaxD || nz < 1 || ldz < round_up(nz, 64)) {
        set_error("pending points: bad arguments of the cross-covariance contraction");
        return EGX_ERR_INVALID_VALUE;
    }
    const int slabs = (nz + 63) / 64;
    if (nsplit < 1) nsplit = 1;
    if (nsplit > slabs) nsplit = slabs;
    const int per = (slabs + nsplit - 1) / nsplit;
    const size_t lds = sizeof(double) * ((size_t)d * kPcThreads + (size_t)d * 64 + (size_t)d * hcols + 64 * kPendingQV);
    if (lds > kPcLdsMax) {
        set_error("pending points: " + std::to_string(d) + " inputs x " + std::to_string(hcols) +
                  " coefficient columns do not fit the 160 KB of LDS");
        return EGX_ERR_UNSUPPORTED;
    }
    dim3 grid(1, (unsigned)nsplit);
#define EGX_PC1(C_, QV_, DK_, G_)                                                                                             \
    {                                                                                                                         \
        if (lds > 65536)                                                                                                      \
            EGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pending_cross<C_, QV_, DK_, G_>),             \
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                         \
        hipLaunchKernelGGL((k_pending_cross<C_, QV_, DK_, G_>), grid, dim3(kPcThreads), lds, s, xqT, ZT, ldz, nz, d, coef,    \
                           hcols, W, v0, q, per, outc, outg);                                                                    \
    }
#define EGX_PC2(C_, QV_)                                \
    if (!outg) EGX_PC1(C_, QV_, 1, false)               \
    else if (d <= 8) EGX_PC1(C_, QV_, 8, true)          \
    else EGX_PC1(C_, QV_, 16, true)
#define EGX_PC(C_)                                      \
    if (cols == 1) { EGX_PC2(C_, 1) }                   \
    else if (cols == 2) { EGX_PC2(C_, 2) }              \
    else { EGX_PC2(C_, kPendingQV) }
    // kPendingQV columns per pass; a last pass of one or two columns runs the narrower instance (a column's sums are its own:
    // its bits do not depend on the width of its pass)
    for (int v0 = 0; v0 < q; v0 += kPendingQV) {
        const int cols = q - v0 < kPendingQV ? q - v0 : kPendingQV;
        EGX_DISPATCH_CORR(corr, EGX_PC(C_));
    }
#undef EGX_PC1
#undef EGX_PC2
#undef EGX_PC
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_pending_finish(hipStream_t s, const PendingFinish &f) {
    const size_t lds = sizeof(double) * (size_t)pending::kLd * (size_t)(f.d > 0 ? f.d : 1);
    if (f.q < 1 || f.q > pending::kMaxPending || f.d < 1 || lds > kPcLdsMax - 4096 || f.nsplit_c < 1 || !f.outc || !f.small || !f.tv ||
        (f.outg && f.nsplit_g < 1) ||
        (!f.emit && !f.mean) || (f.gmean && !f.outg) || (f.gvar && (!f.var || !f.gmean))) {
        set_error("pending points: bad arguments of the finish");
        return EGX_ERR_INVALID_VALUE;
    }
    PendFinishArgs g;
    g.q = f.q, g.d = f.d, g.p = f.p, g.nsplit_c = f.nsplit_c, g.nsplit_g = f.nsplit_g;
    if (f.composed) {  // per column: launch_predict_mean's (msplit x kTile), launch_xgrad's (nsplit x kTile x d)
        g.sc_v = (int64_t)f.nsplit_c * kTile, g.sc_sp = kTile, g.sc_a = 1;
        g.sg_v = (int64_t)f.nsplit_g * kTile * f.d, g.sg_sp = (int64_t)kTile * f.d, g.sg_a = f.d;
    } else {
        g.sc_v = 1, g.sc_sp = (int64_t)kTile * f.q, g.sc_a = f.q;
        g.sg_v = f.d, g.sg_sp = (int64_t)kTile * f.q * f.d, g.sg_a = (int64_t)f.q * f.d;
    }
    g.xqT = f.xqT, g.fidx = f.fidx, g.tv = f.tv, g.small = f.small, g.outc = f.outc, g.outg = f.outg, g.x_std = f.x_std;
    g.sigma2 = f.sigma2, g.sigma2c = f.sigma2c, g.y_std = f.y_std;
    g.mean = f.mean, g.var = f.var, g.gmean = f.gmean, g.gvar = f.gvar, g.emit = f.emit;
    if (lds > 60000)
        EGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pending_finish), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)lds));
    hipLaunchKernelGGL(k_pending_finish, dim3(kTile), dim3(kPfThreads), lds, s, g);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

}  // namespace egx
