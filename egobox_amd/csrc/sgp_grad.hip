// Closed-form gradient of the sparse GP's likelihood (FITC / VFE) with respect to theta, sigma2 and noise (new capability: the
// reference tunes the sparse model derivative-free).  DESIGN.md 4.6 has the derivation; in the notation of sgp_host.hip
// (RT = R_nz C_z^-T, V^T = sigma RT, A = I + V D V^T = L L^T, b = L^-1 V (beta o y), Wz = C_z^-T, Wa = L^-T):
//   E~     = RT L^-T                                  launch_trsm_rows on a copy of RT
//   alpha  = beta o (y - sigma E~ b) = Sigma^-1 y,   e_t = sigma2 |E~_t|^2            launch_row_reduce + k_sgp_grad_rows
//   p_t    = beta_t - beta_t^2 e_t - alpha_t^2,      q = p (FITC), beta (VFE),        r = beta - q >= 0
//   T^T    = [diag(beta) E~ L^-1 - diag(q) RT] C_z^-1 - alpha w^T   (n x nz)          two launch_gemm_nt_sub
//   H      = V diag(q) V^T = (A - I) - V diag(r) V^T  -- r >= 0, so the signed weights of FITC cost ONE more Gram product
//            (launch_gram_lower on W, refilled with sqrt(r)); VFE has r = 0 and none
//   S^     = sigma2 S = Wz (I - Wa Wa^T - H) Wz^T - w~ w~^T,  w~ = sigma w = Wz Wa b   (nz x nz; three small GEMMs)
//   dL/dtheta_k = -sigma2 sum T^T o d_k R_nz + 1/2 sum S^ o d_k R_zz
//   dL/dsigma2  = -1/2 [2 sum T^T o R_nz - sum S^ o R_zz / sigma2 + c_sigma],   dL/dnoise = -1/2 c_nu
// The two sums over a rectangle of pairs are k_sgp_grad_rect, the rectangular counterpart of k_grad_accum (kernels_corr.hip K7):
// rows from one k-major point set, columns from another, a weight per pair; pass one recomputes R[t, i] from the coordinates
// (RT no longer holds it), pass two accumulates the d outputs with dlog_dc, output d is the plain sum of weight * R.  It serves
// R_nz (xT, zT, T^T) and R_zz (zT, zT, S^: the diagonal has R = 1 and d log R = 0, which is the unit diagonal without nugget that
// dL/dsigma2 wants and no term in dL/dtheta).  One partial vector per workgroup and a fixed-order reduce: no atomics, the same
// bits on every call.
// Extra device memory, allocated by the first gradient call and kept in the handle: ONE n_pad x z_pad buffer (E~, then T^T;
// 4.1 GB at n = 10^6, nz = 512), 7 n_pad vectors, one zext^2 and three z_pad^2 matrices.  diag(q) RT - diag(beta) E~ L^-1 lives
// in W, which is free after the Gram products.  Nothing n-long goes to the host.
// The gradient in the inducing points (sgp_grad_tail_z, k_sgp_grad_cols) contracts the same T^T and S^ once more.
#include "sgp_handle.h"
#include "corr_pair.h"
#include "kpls_coef.h"

#include <algorithm>
#include <cmath>

using namespace egx;

namespace {

constexpr int kRectDC = 64;       // input dimensions staged per pass (2 x 64 x 64 doubles = 64 KB of LDS)
constexpr int kRectMaxWG = 2048;  // workgroups (partial vectors) per output chunk

// MULTI (KPLS under a Matern correlation): coef is d x hcols (c_kl = theta_l |w_kl|) and the outputs are per
// theta, not per input: output o < hcols is sum_pairs wp sum_k |w_ko| dlog_dc(c_ko, |x_ik - z_jk|), output hcols the plain sum.
// Every theta output walks all d dimensions, so for d > kRectDC pass 2 stages the slabs again chunk by chunk.  coef and |w| are
// read at wave-uniform addresses.  MULTI == false is the kernel as it was: hcols and wabs are not read.
template <int CORR, int DK, bool MULTI = false>
__global__ __launch_bounds__(256) void k_sgp_grad_rect(const double *__restrict__ xT, int64_t ldx, int n,
                                                       const double *__restrict__ zT, int64_t ldz, int nz, int d,
                                                       const double *__restrict__ coef, const double *__restrict__ T, int64_t ldt,
                                                       int ntc, int ntiles, int nout, int nout_pad, double *__restrict__ part,
                                                       int hcols, const double *__restrict__ wabs) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int dc = d < kRectDC ? d : kRectDC;
    double *xi = sm, *xj = sm + dc * 64;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int o0 = blockIdx.y * DK;
    double acc[DK];
#pragma unroll
    for (int oo = 0; oo < DK; oo++) acc[oo] = 0.0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int bi = t / ntc, bj = t - bi * ntc;
        const SlabSrc si{xT, ldx, bi * 64}, sj{zT, ldz, bj * 64};
        // ---- pass 1: the correlations of the tile's 16 pairs per lane (all d dimensions, staged dc at a time)
        PairAcc<CORR> pa[4][4];
        tile_pairs_staged<CORR>(xi, xj, si, sj, d, dc, coef, MULTI ? hcols : 1, tid, ty, tx, true, pa);
        double wp[4][4];  // T[t, i] R[t, i] inside the n x nz rectangle, else 0
        rect_weights<CORR>(pa, T, ldt, bi * 64, bj * 64, n, nz, ty, tx, wp);
        if (MULTI) {
            // ---- pass 2, per theta: outputs o0 .. o0 + DK - 1, o < hcols <-> theta_o, o == hcols the plain sum.  d <= dc: the
            // slabs of pass 1 hold every dimension; else each chunk is staged again (none where the plain sum is alone)
            if (o0 < hcols) {
                for (int c0 = 0; c0 < d; c0 += dc) {
                    const int dn = (d - c0 < dc) ? (d - c0) : dc;
                    if (d > dc) stage_pair(xi, xj, si.from(c0), sj.from(c0), dn, tid, true);
                    for (int k = 0; k < dn; k++) {
                        double vi[4], vj[4], ad[4][4];
#pragma unroll
                        for (int a = 0; a < 4; a++) vi[a] = xi[k * 64 + ty * 4 + a];
#pragma unroll
                        for (int b = 0; b < 4; b++) vj[b] = xj[k * 64 + tx * 4 + b];
#pragma unroll
                        for (int a = 0; a < 4; a++)
#pragma unroll
                            for (int b = 0; b < 4; b++) ad[a][b] = fabs(vi[a] - vj[b]);
                        const double *ck = coef + (int64_t)(c0 + k) * hcols + o0, *wk = wabs + (int64_t)(c0 + k) * hcols + o0;
#pragma unroll
                        for (int oo = 0; oo < DK; oo++) {
                            if (o0 + oo < hcols) {
                                const double c = ck[oo], wa = wk[oo];
                                double t = 0.0;
#pragma unroll
                                for (int a = 0; a < 4; a++)
#pragma unroll
                                    for (int b = 0; b < 4; b++) t = __builtin_fma(wp[a][b], dlog_dc<CORR>(c, ad[a][b]), t);
                                acc[oo] = __builtin_fma(wa, t, acc[oo]);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int oo = 0; oo < DK; oo++) {
                if (o0 + oo == hcols) {
                    double sacc = acc[oo];
#pragma unroll
                    for (int a = 0; a < 4; a++)
#pragma unroll
                        for (int b = 0; b < 4; b++) sacc += wp[a][b];
                    acc[oo] = sacc;
                }
            }
            continue;
        }
        // ---- pass 2: this workgroup's outputs o0 .. o0 + DK - 1: o < d <-> input dimension o, o == d the plain sum.
        // d > dc: the chunk's dimensions are staged again, from slab row 0 (none where the plain sum is alone in its chunk)
        int base = 0;
        if (d > dc) {
            stage_pair(xi, xj, si.from(o0), sj.from(o0), (d - o0 < DK) ? (d - o0) : DK, tid, true);
            base = o0;
        }
#pragma unroll
        for (int oo = 0; oo < DK; oo++) {
            const int o = o0 + oo;
            if (o < d) {
                const double c = coef[o];
                double vi[4], vj[4];
#pragma unroll
                for (int a = 0; a < 4; a++) vi[a] = xi[(o - base) * 64 + ty * 4 + a];
#pragma unroll
                for (int b = 0; b < 4; b++) vj[b] = xj[(o - base) * 64 + tx * 4 + b];
                double sacc = acc[oo];
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int b = 0; b < 4; b++) sacc = __builtin_fma(wp[a][b], dlog_dc<CORR>(c, fabs(vi[a] - vj[b])), sacc);
                acc[oo] = sacc;
            } else if (o == d) {
                double sacc = acc[oo];
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int b = 0; b < 4; b++) sacc += wp[a][b];
                acc[oo] = sacc;
            }
        }
    }
    // ---- one reduction per workgroup: lanes of a wave (xor shuffles), then the four waves in a fixed order
    const double v = wg_sum_dk<DK>(acc, sm, tid);
    if (tid < DK && o0 + tid < nout) part[(int64_t)blockIdx.x * nout_pad + o0 + tid] = v;
}

// out[o] = sum over the nwg partial vectors, in a fixed order: 256 lanes take every 256th, then a tree in LDS
__global__ __launch_bounds__(256) void k_sgp_grad_reduce(const double *__restrict__ part, int nwg, int nout_pad,
                                                         double *__restrict__ out) {
    const double v = sum_partial_vectors(part, nwg, nout_pad, blockIdx.x, threadIdx.x);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// The per-point quantities, t < n_pad (zeros beyond n): alpha, beta, q, sqrt(r), p
__global__ __launch_bounds__(256) void k_sgp_grad_rows(int n, int n_pad, const double *__restrict__ s0, const double *__restrict__ e2,
                                                       const double *__restrict__ eb, const double *__restrict__ y, double sigma,
                                                       double sigma2, double noise, double nugget, int vfe,
                                                       double *__restrict__ alpha, double *__restrict__ beta, double *__restrict__ q,
                                                       double *__restrict__ sr, double *__restrict__ p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_pad) return;
    double al = 0.0, be = 0.0, qv = 0.0, rv = 0.0, pv = 0.0;
    if (t < n) {
        const double nu = vfe ? fmax(noise, nugget) : sigma2 * (1.0 - s0[t]) + noise;
        be = 1.0 / nu;
        al = be * (y[t] - sigma * eb[t]);
        rv = be * be * (sigma2 * e2[t]) + al * al;
        pv = be - rv;
        qv = vfe ? be : pv;
        if (vfe) rv = 0.0;
    }
    alpha[t] = al;
    beta[t] = be;
    q[t] = qv;
    sr[t] = sqrt(rv);
    p[t] = pv;
}

// part[b * 32 + 0 / 1] = block b's share of sum a[t] / sum c[t], t < n: elements b * 256 + tid + k * gridDim.x * 256, a tree in
// LDS -- a fixed order; k_sgp_grad_reduce adds the blocks
__global__ __launch_bounds__(256) void k_sgp_sum2(const double *__restrict__ a, const double *__restrict__ c, int n,
                                                  double *__restrict__ part) {
    __shared__ double ra[256], rc[256];
    const int tid = threadIdx.x;
    double va = 0.0, vc = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + tid; t < n; t += (int64_t)gridDim.x * 256) {
        va += a[t];
        vc += c[t];
    }
    ra[tid] = va;
    rc[tid] = vc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            ra[tid] += ra[tid + s];
            rc[tid] += rc[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        part[(int64_t)blockIdx.x * 32] = ra[0];
        part[(int64_t)blockIdx.x * 32 + 1] = rc[0];
    }
}

// F[t][i] = q[t] RT[t][i], E[t][i] *= beta[t] over the n_pad x z_pad rectangle (z_pad is even)
__global__ __launch_bounds__(256) void k_sgp_scale_pair(const double *__restrict__ RT, const double *__restrict__ q,
                                                        const double *__restrict__ beta, int z_pad, int64_t count,
                                                        double *__restrict__ F, double *__restrict__ E) {
    const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
    if (e >= count) return;
    const int t = (int)(e / z_pad);
    const double qt = q[t], bt = beta[t];
    const double2 r = *reinterpret_cast<const double2 *>(RT + e);
    const double2 v = *reinterpret_cast<const double2 *>(E + e);
    *reinterpret_cast<double2 *>(F + e) = make_double2(qt * r.x, qt * r.y);
    *reinterpret_cast<double2 *>(E + e) = make_double2(bt * v.x, bt * v.y);
}

// M[t][i] = -scale * a[t] * w[i] over rows x cols (cols even)
__global__ __launch_bounds__(256) void k_sgp_outer_neg(const double *__restrict__ a, const double *__restrict__ w, double scale,
                                                       int cols, int64_t count, double *__restrict__ M) {
    const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
    if (e >= count) return;
    const int t = (int)(e / cols), i = (int)(e - (int64_t)t * cols);
    const double at = -scale * a[t];
    *reinterpret_cast<double2 *>(M + e) = make_double2(at * w[i], at * w[i + 1]);
}

// M1 (z_pad x z_pad, both triangles) = I - H,  H = V D V^T - V diag(r) V^T = -G + G2 from the Gram kernels' lower tiles
// (read at i >= j only: exactly symmetric); G2 == nullptr: r = 0 (VFE)
__global__ __launch_bounds__(256) void k_sgp_form_m1(const double *__restrict__ G, const double *__restrict__ G2, int zext,
                                                     int z_pad, double *__restrict__ M1) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= z_pad) return;
    const int64_t lo = (int64_t)(i > j ? i : j) * zext + (i > j ? j : i);
    double h = -G[lo];
    if (G2) h += G2[lo];
    M1[(int64_t)i * z_pad + j] = ((i == j) ? 1.0 : 0.0) - h;
}

// out (nout doubles) = the sums over the n x nz rectangle with rows xT, columns zT and weights T
// hcols > 1 (Matern with KPLS weights; wabs = |w|, d x hcols like coef): nout = hcols + 1 sums, per theta (the MULTI form)
int launch_grad_rect(hipStream_t s, int corr, const double *xT, int64_t ldx, int n, const double *zT, int64_t ldz, int nz, int d,
                     const double *coef, int hcols, const double *wabs, const double *T, int64_t ldt, double *part, double *out) {
    const bool multi = hcols > 1;
    if (multi && corr != EGX_CORR_MATERN32 && corr != EGX_CORR_MATERN52) {
        set_error("sparse GP gradient: a coefficient table with hcols > 1 belongs to the Matern correlations");
        return EGX_ERR_INVALID_VALUE;
    }
    const int nout = (multi ? hcols : d) + 1, nout_pad = (int)round_up(nout, 32);
    const int ntc = (nz + 63) / 64;
    const int64_t nt = (int64_t)((n + 63) / 64) * ntc;
    if (nt > 0x7fffffff) {
        set_error("sparse GP gradient: too many tiles");
        return EGX_ERR_UNSUPPORTED;
    }
    const int ntiles = (int)nt, nwg = ntiles < kRectMaxWG ? ntiles : kRectMaxWG;
    const int dc = d < kRectDC ? d : kRectDC;
    // (the per-theta form walks every dimension per output: narrower chunks, so that a few thetas do not pay for 8 or 16)
    const int dk = multi ? (nout <= 4 ? 4 : (nout <= 8 ? 8 : 16)) : (nout <= 8 ? 8 : (nout <= 16 ? 16 : 32));
    const size_t lds = sizeof(double) * (size_t)std::max(2 * dc * 64, 4 * dk);
    const dim3 grid((unsigned)nwg, (unsigned)((nout + dk - 1) / dk));
#define EGX_RECT_M(C_, DK_)                                                                                                     \
    hipLaunchKernelGGL((k_sgp_grad_rect<C_, DK_, true>), grid, dim3(256), lds, s, xT, ldx, n, zT, ldz, nz, d, coef, T, ldt, ntc, \
                       ntiles, nout, nout_pad, part, hcols, wabs)
#define EGX_RECT_M_DK(C_)                \
    if (dk == 4) EGX_RECT_M(C_, 4);      \
    else if (dk == 8) EGX_RECT_M(C_, 8); \
    else EGX_RECT_M(C_, 16)
    if (multi) {
        if (corr == EGX_CORR_MATERN32) { EGX_RECT_M_DK(EGX_CORR_MATERN32); }
        else { EGX_RECT_M_DK(EGX_CORR_MATERN52); }
        hipLaunchKernelGGL(k_sgp_grad_reduce, dim3((unsigned)nout), dim3(256), 0, s, part, nwg, nout_pad, out);
        EGX_HIP_CHECK(hipGetLastError());
        return EGX_SUCCESS;
    }
#undef EGX_RECT_M_DK
#undef EGX_RECT_M
#define EGX_RECT(C_, DK_)                                                                                                    \
    hipLaunchKernelGGL((k_sgp_grad_rect<C_, DK_>), grid, dim3(256), lds, s, xT, ldx, n, zT, ldz, nz, d, coef, T, ldt, ntc, ntiles, \
                       nout, nout_pad, part, 1, (const double *)nullptr)
#define EGX_RECT_DK(C_)                 \
    if (dk == 8) EGX_RECT(C_, 8);       \
    else if (dk == 16) EGX_RECT(C_, 16); \
    else EGX_RECT(C_, 32)
    EGX_DISPATCH_CORR(corr, EGX_RECT_DK(C_));
#undef EGX_RECT_DK
#undef EGX_RECT
    hipLaunchKernelGGL(k_sgp_grad_reduce, dim3((unsigned)nout), dim3(256), 0, s, part, nwg, nout_pad, out);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

// ---- the gradient in the inducing points: the column-reducing counterpart of k_sgp_grad_rect
//   out[j, k] = scale * sum_i T[i, j] R(x_i, z_j) phi_k(x_ik - z_jk),   phi_k(dlt) = d ln r(a, b) / d a_k at dlt = a_k - b_k
// over the same rectangles and weights.  (xT, zT, T^T) with scale sigma2 is the first sum of dL/dz; (zT, zT, S^) with scale -1 is
// the second: S^ and R_zz are symmetric and phi is odd, so sum_b S^[j, b] R phi_k(z_j - z_b) = -sum_i S^[i, j] R phi_k(z_i - z_j),
// rows reduced as in the first -- one kernel serves both.
constexpr int kColsTargetWG = 1024;  // workgroups per output chunk that the runs of row tiles are sized for

// phi_k: odd in dlt and exactly 0 at dlt == 0, the kink of the absolute exponential included (sgn(0) = 0, what the central
// difference gives where an inducing point sits on a training point; xgrad_factor's copysign yields -c at +0, and other
// kernels depend on its bits).  Matern: c sgn(dlt) (ln(1 + ..) - ..)'(t) at t = c |dlt|, with t sgn(dlt) = c dlt.
template <int CORR>
__device__ __forceinline__ double dlog_da(double c, double dlt) {
    if (CORR == EGX_CORR_SQUARED_EXPONENTIAL) return -(c * c) * dlt;
    if (CORR == EGX_CORR_ABSOLUTE_EXPONENTIAL) return dlt > 0.0 ? -c : (dlt < 0.0 ? c : 0.0);
    const double t = c * fabs(dlt), cd = (c * c) * dlt;
    if (CORR == EGX_CORR_MATERN32) return -3.0 * cd * rcp_ge1(__builtin_fma(kSqrt3, t, 1.0));
    const double u = __builtin_fma(kSqrt5, t, 1.0);
    return -k5over3 * cd * u * rcp_ge1(__builtin_fma(k5over3 * t, t, u));
}

// A workgroup owns column tile blockIdx.y, the run of row tiles [blockIdx.x * tpc, .. + tpc) and the output dimensions
// blockIdx.z * DK ..; pass 1 is k_sgp_grad_rect's, pass 2 keeps one accumulator per (column, output dimension).  The sum over
// rows meets in a fixed order: a lane's four rows of a tile and its tiles one after the other in registers, the four lanes of
// a wave that share tx (xor shuffles over the ty bits 16, 32), the four waves through LDS; the partial [64 columns][d] goes to
// part[blockIdx.x], and k_sgp_grad_cols_reduce adds the runs in order.  No atomics: the same bits on every call.
// MULTI (KPLS under a Matern correlation): coef is d x hcols and r is a product over (k, l), so the factor of output (j, k) is
// sum_l dlog_da(c_kl, x_ik - z_jk); the outputs stay (column, input dimension).  MULTI == false: the kernel as it was.
template <int CORR, int DK, bool MULTI = false>
__global__ __launch_bounds__(256) void k_sgp_grad_cols(const double *__restrict__ xT, int64_t ldx, int n,
                                                       const double *__restrict__ zT, int64_t ldz, int nz, int d,
                                                       const double *__restrict__ coef, const double *__restrict__ T, int64_t ldt,
                                                       int nrt, int tpc, int ncol_pad, double *__restrict__ part, int hcols) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int dc = d < kRectDC ? d : kRectDC;
    double *xi = sm, *xj = sm + dc * 64;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int bj = blockIdx.y, o0 = blockIdx.z * DK;
    const int r0 = blockIdx.x * tpc, r1 = (r0 + tpc < nrt) ? r0 + tpc : nrt;
    double acc[4][DK];
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
        for (int oo = 0; oo < DK; oo++) acc[b][oo] = 0.0;
    for (int bi = r0; bi < r1; bi++) {
        const SlabSrc si{xT, ldx, bi * 64}, sj{zT, ldz, bj * 64};
        // ---- pass 1: the correlations of the tile's 16 pairs per lane (all d dimensions, staged dc at a time)
        PairAcc<CORR> pa[4][4];
        tile_pairs_staged<CORR>(xi, xj, si, sj, d, dc, coef, MULTI ? hcols : 1, tid, ty, tx, true, pa);
        double wp[4][4];  // T[i, j] R[i, j] inside the n x nz rectangle, else 0
        rect_weights<CORR>(pa, T, ldt, bi * 64, bj * 64, n, nz, ty, tx, wp);
        // ---- pass 2: output dimensions o0 .. o0 + DK - 1 of this lane's four columns.  d > dc: they are staged again, from
        // slab row 0
        int base = 0;
        if (d > dc) {
            stage_pair(xi, xj, si.from(o0), sj.from(o0), (d - o0 < DK) ? (d - o0) : DK, tid, true);
            base = o0;
        }
#pragma unroll
        for (int oo = 0; oo < DK; oo++) {
            const int o = o0 + oo;
            if (MULTI) {
                if (o < d) {
                    double vi[4], vj[4], fac[4][4];
#pragma unroll
                    for (int a = 0; a < 4; a++) vi[a] = xi[(o - base) * 64 + ty * 4 + a];
#pragma unroll
                    for (int b = 0; b < 4; b++) vj[b] = xj[(o - base) * 64 + tx * 4 + b];
#pragma unroll
                    for (int a = 0; a < 4; a++)
#pragma unroll
                        for (int b = 0; b < 4; b++) fac[a][b] = 0.0;
                    const double *ck = coef + (int64_t)o * hcols;
                    for (int l = 0; l < hcols; l++) {
                        const double c = ck[l];
#pragma unroll
                        for (int a = 0; a < 4; a++)
#pragma unroll
                            for (int b = 0; b < 4; b++) fac[a][b] += dlog_da<CORR>(c, vi[a] - vj[b]);
                    }
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        double sacc = acc[b][oo];
#pragma unroll
                        for (int a = 0; a < 4; a++) sacc = __builtin_fma(wp[a][b], fac[a][b], sacc);
                        acc[b][oo] = sacc;
                    }
                }
            } else if (o < d) {
                const double c = coef[o];
                double vi[4], vj[4];
#pragma unroll
                for (int a = 0; a < 4; a++) vi[a] = xi[(o - base) * 64 + ty * 4 + a];
#pragma unroll
                for (int b = 0; b < 4; b++) vj[b] = xj[(o - base) * 64 + tx * 4 + b];
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    double sacc = acc[b][oo];
#pragma unroll
                    for (int a = 0; a < 4; a++) sacc = __builtin_fma(wp[a][b], dlog_da<CORR>(c, vi[a] - vj[b]), sacc);
                    acc[b][oo] = sacc;
                }
            }
        }
    }
    // ---- one reduction per workgroup: the lanes of a wave that share tx, then the four waves in a fixed order
    __syncthreads();
    double *red = sm;  // [4 waves][64 columns][DK]
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
        for (int oo = 0; oo < DK; oo++) {
            double v = acc[b][oo];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if ((tid & 48) == 0) red[((tid >> 6) * 64 + tx * 4 + b) * DK + oo] = v;
        }
    __syncthreads();
    for (int e = tid; e < 64 * DK; e += 256) {
        const int col = e / DK, o = o0 + (e - col * DK);
        if (o < d)
            part[((int64_t)blockIdx.x * ncol_pad + bj * 64 + col) * d + o] =
                ((red[e] + red[64 * DK + e]) + red[2 * 64 * DK + e]) + red[3 * 64 * DK + e];
    }
}

// out[j * d + k] = scale * (the runs' partials of column j, dimension k, added in run order), j < nz
__global__ __launch_bounds__(256) void k_sgp_grad_cols_reduce(const double *__restrict__ part, int nruns, int64_t run_stride,
                                                              int64_t count, double scale, double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    double v = 0.0;
    for (int r = 0; r < nruns; r++) v += part[(int64_t)r * run_stride + e];
    out[e] = scale * v;
}

// The runs of row tiles of a rectangle with `rows` rows and `cols` columns: (tiles per run, number of runs) -- a function of
// the two sizes alone
void cols_runs(int rows, int cols, int &tpc, int &nruns) {
    const int nrt = (rows + 63) / 64, ntc = (cols + 63) / 64;
    const int want = std::max(1, std::min(nrt, (kColsTargetWG + ntc - 1) / ntc));
    tpc = std::max((nrt + want - 1) / want, std::min(nrt, 2));  // two tiles at least share a workgroup's reduction
    nruns = (nrt + tpc - 1) / tpc;
}
size_t cols_part_doubles(int rows, int cols, int d) {
    int tpc, nruns;
    cols_runs(rows, cols, tpc, nruns);
    return (size_t)nruns * (size_t)((cols + 63) / 64 * 64) * (size_t)d;
}

// out (nz x d) = scale * the column sums over the n x nz rectangle with rows xT, columns zT and weights T
int launch_grad_cols(hipStream_t s, int corr, const double *xT, int64_t ldx, int n, const double *zT, int64_t ldz, int nz, int d,
                     const double *coef, int hcols, const double *T, int64_t ldt, double scale, double *part, double *out) {
    const bool multi = hcols > 1;  // Matern with KPLS weights: coef is d x hcols
    if (multi && corr != EGX_CORR_MATERN32 && corr != EGX_CORR_MATERN52) {
        set_error("sparse GP gradient in the inducing points: a coefficient table with hcols > 1 belongs to the Matern correlations");
        return EGX_ERR_INVALID_VALUE;
    }
    const int nrt = (n + 63) / 64, ntc = (nz + 63) / 64, ncol_pad = ntc * 64;
    int tpc, nruns;
    cols_runs(n, nz, tpc, nruns);
    const int dc = d < kRectDC ? d : kRectDC;
    const int dk = d <= 4 ? 4 : (d <= 8 ? 8 : 16);
    const int nzc = (d + dk - 1) / dk;
    if (ntc > 65535 || nzc > 65535) {
        set_error("sparse GP gradient in the inducing points: too many column tiles or dimensions");
        return EGX_ERR_UNSUPPORTED;
    }
    const size_t lds = sizeof(double) * (size_t)std::max(2 * dc * 64, 4 * 64 * dk);
    const dim3 grid((unsigned)nruns, (unsigned)ntc, (unsigned)nzc);
#define EGX_COLS(C_, DK_, M_)                                                                                                       \
    hipLaunchKernelGGL((k_sgp_grad_cols<C_, DK_, M_>), grid, dim3(256), lds, s, xT, ldx, n, zT, ldz, nz, d, coef, T, ldt, nrt, tpc, \
                       ncol_pad, part, hcols)
#define EGX_COLS_DK(C_, M_)                \
    if (dk == 4) EGX_COLS(C_, 4, M_);      \
    else if (dk == 8) EGX_COLS(C_, 8, M_); \
    else EGX_COLS(C_, 16, M_)
    if (multi) {
        if (corr == EGX_CORR_MATERN32) { EGX_COLS_DK(EGX_CORR_MATERN32, true); }
        else { EGX_COLS_DK(EGX_CORR_MATERN52, true); }
    } else {
        EGX_DISPATCH_CORR(corr, EGX_COLS_DK(C_, false));
    }
#undef EGX_COLS_DK
#undef EGX_COLS
    const int64_t count = (int64_t)nz * d;
    hipLaunchKernelGGL(k_sgp_grad_cols_reduce, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, part, nruns,
                       (int64_t)ncol_pad * d, count, scale, out);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

}  // namespace

namespace egx {

// After a successful sgp_eval(theta, sigma2, noise) whose factors are resident (Kz, dinv_z, RT, s0, A with b in row z_pad,
// dinv_a, G): grad (h + 2; h = d without KPLS weights) = dL/dtheta_0..h-1, dL/dsigma2, dL/dnoise.  Caller holds g->mu.
int sgp_grad_tail(egx_sgp *g, double sigma2, double noise, double *grad) {
    const int n = g->n, d = g->d, nz = g->nz, n_pad = g->n_pad, z_pad = g->z_pad, zext = g->zext;
    const int vfe = g->method != 0;
    const double sigma = std::sqrt(sigma2);
    hipStream_t s = g->stream;
    const size_t rect = (size_t)n_pad * z_pad, sq = (size_t)z_pad * z_pad;
    // the kernels' sums: one per theta under KPLS with a Matern correlation (hcols > 1), else one per input dimension; + the plain sum
    const int hcols = g->hcols, nk = hcols > 1 ? hcols : d;
    const int nout = nk + 1, nout_pad = (int)round_up(nout, 32);
    EGX_RC(g->gr_E.alloc(rect));
    EGX_RC(g->gr_rows.alloc((size_t)7 * n_pad));
    EGX_RC(g->gr_sq.alloc(3 * sq));
    EGX_RC(g->gr_vec.alloc((size_t)2 * z_pad));
    EGX_RC(g->gr_part.alloc((size_t)kRectMaxWG * nout_pad));
    EGX_RC(g->gr_out.alloc((size_t)2 * nout_pad + 32));
    if (!vfe) EGX_RC(g->gr_G2.alloc((size_t)zext * zext));
    double *E = g->gr_E.p, *F = g->W.p;  // W (zext x n_pad) holds the n_pad x z_pad F once the Gram products are done
    double *e2 = g->gr_rows.p, *eb = e2 + n_pad, *alpha = eb + n_pad, *beta = alpha + n_pad, *q = beta + n_pad, *sr = q + n_pad,
           *p = sr + n_pad;
    double *M1 = g->gr_sq.p, *X = M1 + sq, *Sh = X + sq;
    double *t1 = g->gr_vec.p, *wt = t1 + z_pad;
    double *out_nz = g->gr_out.p, *out_zz = out_nz + nout_pad, *sums = out_zz + nout_pad;
    const double *b = g->A.p + (size_t)z_pad * z_pad;  // row z_pad of A: L^-1 V (beta o y), zero beyond nz
    EGX_RC(sgp_ensure_inverse_factors(g));  // Wz = C_z^-T, Wa = L^-T of the resident factors
    // E~ = RT L^-T, its row norms and E~ b
    EGX_HIP_CHECK(hipMemcpyAsync(E, g->RT.p, sizeof(double) * rect, hipMemcpyDeviceToDevice, s));
    EGX_RC(launch_trsm_rows(s, g->A.p, z_pad, z_pad, g->dinv_a.p, E, z_pad, n_pad));
    EGX_RC(launch_row_reduce(s, E, z_pad, n_pad, nz, b, z_pad, 1, e2, eb));
    hipLaunchKernelGGL(k_sgp_grad_rows, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s, n, n_pad, g->s0.p, e2, eb, g->y.p,
                       sigma, sigma2, noise, g->nugget, vfe, alpha, beta, q, sr, p);
    const int nsum = std::min(256, (n + 1023) / 1024);
    hipLaunchKernelGGL(k_sgp_sum2, dim3((unsigned)nsum), dim3(256), 0, s, p, g->s0.p, n, g->gr_part.p);
    hipLaunchKernelGGL(k_sgp_grad_reduce, dim3(2), dim3(256), 0, s, g->gr_part.p, nsum, 32, sums);
    // FITC: G2 = -V diag(r) V^T, the Gram product of the likelihood with sqrt(r) in place of sqrt(beta)
    if (!vfe) {
        EGX_RC(sgp_launch_transpose_scale(g, sr, sigma));
        EGX_RC(launch_gram_lower(s, g->W.p, n_pad, zext, n_pad, g->gr_G2.p, zext, g->P.p));
    }
    // w~ = Wz Wa b
    EGX_RC(launch_uptri_gemv(s, g->Wa.p, z_pad, z_pad, b, t1));
    EGX_RC(launch_uptri_gemv(s, g->Wz.p, z_pad, z_pad, t1, wt));
    // S^ = Wz (I - H - Wa Wa^T) Wz^T - w~ w~^T
    hipLaunchKernelGGL(k_sgp_form_m1, dim3((unsigned)((z_pad + 255) / 256), (unsigned)z_pad), dim3(256), 0, s, g->G.p,
                       vfe ? nullptr : g->gr_G2.p, zext, z_pad, M1);
    EGX_RC(launch_gemm_nt_sub(s, M1, z_pad, g->Wa.p, z_pad, g->Wa.p, z_pad, z_pad, z_pad, z_pad, 0));
    EGX_HIP_CHECK(hipMemsetAsync(X, 0, sizeof(double) * sq, s));
    EGX_RC(launch_gemm_nt_sub(s, X, z_pad, g->Wz.p, z_pad, M1, z_pad, z_pad, z_pad, z_pad, 0));  // X = -Wz M1 (M1 symmetric)
    hipLaunchKernelGGL(k_sgp_outer_neg, dim3((unsigned)((sq / 2 + 255) / 256)), dim3(256), 0, s, wt, wt, 1.0, z_pad, (int64_t)sq, Sh);
    EGX_RC(launch_gemm_nt_sub(s, Sh, z_pad, X, z_pad, g->Wz.p, z_pad, z_pad, z_pad, z_pad, 0));
    // T^T = -alpha w^T - F C_z^-1,  F = diag(q) RT - diag(beta) E~ L^-1
    hipLaunchKernelGGL(k_sgp_scale_pair, dim3((unsigned)((rect / 2 + 255) / 256)), dim3(256), 0, s, g->RT.p, q, beta, z_pad,
                       (int64_t)rect, F, E);
    EGX_RC(launch_gemm_nt_sub(s, F, z_pad, E, z_pad, g->Wa.p, z_pad, n_pad, z_pad, z_pad, 0));
    hipLaunchKernelGGL(k_sgp_outer_neg, dim3((unsigned)((rect / 2 + 255) / 256)), dim3(256), 0, s, alpha, wt, 1.0 / sigma, z_pad,
                       (int64_t)rect, E);
    EGX_RC(launch_gemm_nt_sub(s, E, z_pad, F, z_pad, g->Wz.p, z_pad, n_pad, z_pad, z_pad, 0));
    // the two rectangles of pairs
    EGX_RC(launch_grad_rect(s, g->corr, g->xT.p, n_pad, n, g->zT.p, z_pad, nz, d, g->coef.p, hcols, g->d_wabs.p, E, z_pad, g->gr_part.p,
                            out_nz));
    EGX_RC(launch_grad_rect(s, g->corr, g->zT.p, z_pad, nz, g->zT.p, z_pad, nz, d, g->coef.p, hcols, g->d_wabs.p, Sh, z_pad,
                            g->gr_part.p, out_zz));
    std::vector<double> h((size_t)2 * nout_pad + 32);
    EGX_HIP_CHECK(hipMemcpyAsync(h.data(), g->gr_out.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
    EGX_HIP_CHECK(hipStreamSynchronize(s));
    const double *hn = h.data(), *hz = hn + nout_pad;
    const double sum_p = h[(size_t)2 * nout_pad], sum_s0 = h[(size_t)2 * nout_pad + 1];
    const int nt = g->h;  // theta components: grad is nt + 2 long
    if (!g->has_w) {
        for (int k = 0; k < d; k++) grad[k] = -sigma2 * hn[k] + 0.5 * hz[k];
    } else {  // the sums are dL/dc_j of the collapsed coefficients, or per theta already: the chain rule of the table (kpls_coef.h)
        std::vector<double> gs(nk);
        for (int k = 0; k < nk; k++) gs[k] = -sigma2 * hn[k] + 0.5 * hz[k];
        kpls::chain_rule(g->corr, d, nt, g->w_ptr(), hcols, g->coef_host.data(), g->th_full.data(), gs.data(), 1.0, grad,
                          true);
    }
    const double nu = std::fmax(noise, g->nugget), be = 1.0 / nu;
    const double c_sigma = vfe ? (double)n * be : sum_p;
    grad[nt] = -0.5 * (2.0 * hn[nk] - hz[nk] / sigma2 + c_sigma);
    if (!vfe) grad[nt + 1] = -0.5 * sum_p;
    else grad[nt + 1] = (noise > g->nugget) ? -0.5 * (sum_p - be * be * ((double)n * sigma2 - sigma2 * sum_s0)) : 0.0;
    return EGX_SUCCESS;
}

// Right after a successful sgp_grad_tail (T^T still in gr_E, S^ in the third matrix of gr_sq, theta in coef):
//   dL/dz[j, k] = sigma2 sum_t T^T[t, j] R(x_t, z_j) phi_k(x_tk - z_jk) + sum_b S^[j, b] R(z_j, z_b) phi_k(z_jk - z_bk)
// two launches of k_sgp_grad_cols, the two nz x d results added on the host.  Caller holds g->mu.
int sgp_grad_tail_z(egx_sgp *g, double sigma2, double *grad_z) {
    const int n = g->n, d = g->d, nz = g->nz, n_pad = g->n_pad, z_pad = g->z_pad;
    hipStream_t s = g->stream;
    const size_t sq = (size_t)z_pad * z_pad, cnt = (size_t)nz * d;
    EGX_RC(g->gz_part.alloc(std::max(cols_part_doubles(n, nz, d), cols_part_doubles(nz, nz, d))));
    EGX_RC(g->gz_out.alloc(2 * cnt));
    const double *E = g->gr_E.p, *Sh = g->gr_sq.p + 2 * sq;
    double *out_nz = g->gz_out.p, *out_zz = out_nz + cnt;
    EGX_RC(launch_grad_cols(s, g->corr, g->xT.p, n_pad, n, g->zT.p, z_pad, nz, d, g->coef.p, g->hcols, E, z_pad, sigma2, g->gz_part.p,
                            out_nz));
    EGX_RC(launch_grad_cols(s, g->corr, g->zT.p, z_pad, nz, g->zT.p, z_pad, nz, d, g->coef.p, g->hcols, Sh, z_pad, -1.0, g->gz_part.p,
                            out_zz));
    std::vector<double> h(2 * cnt);
    EGX_HIP_CHECK(hipMemcpyAsync(h.data(), g->gz_out.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
    EGX_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t e = 0; e < cnt; e++) grad_z[e] = h[e] + h[cnt + e];
    return EGX_SUCCESS;
}

}  // namespace egx
