// Correlation kernels for gfx950: the device counterpart of
//   DiffMatrix::_cross_diff        crates/gp/src/utils.rs:80-104
//   pairwise_differences           crates/gp/src/utils.rs:110-131
//   CorrelationModel::value        crates/gp/src/correlation_models.rs:91-104 (sq-exp), :185-196
//                                  (abs-exp), :326-353 (Matern 3/2), :497-523 (Matern 5/2)
//   the R scatter loop             crates/gp/src/algorithm.rs:997-1001
//   _compute_correlation + predict crates/gp/src/algorithm.rs:253-263, 372-380
// fused so that the (n(n-1)/2, d) difference table (34 GB at n = 16384, d = 32) and the (m*n, d)
// prediction table never exist: every workgroup stages two 64-point slabs of the (k-major)
// normalised inputs in LDS and produces a 64x64 tile of correlations with DIRECT differences
// (no |a|^2+|b|^2-2ab trick: cancellation would break 1e-8 parity for near-duplicate points).
// HBM traffic is the algorithmic minimum: X read once per tile row/column from L2, R written once.
#include "egx_internal.h"
#include "corr_pair.h"  // the pieces of a pair tile, from staging to the fixed-order sums (shared with sgp_grad.hip, kernels_pending.hip)

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <string>

namespace egx {

// Input dimensions are staged in LDS in chunks of at most kCorrDC (round 4: any d; one chunk for d <= 64, where nothing
// changes): the pair accumulators (exponent sum, Matern product) simply run on across the chunks.
constexpr int kCorrDC = 64;

// K1: symmetric training correlation matrix, 64x64 tiles, 128x128-granular lower triangle.
template <int CORR, bool PRE, int RI>  // 64 x 64 tile per workgroup of 1024 / RI threads, RI x 4 pairs per lane
__global__ __launch_bounds__(1024 / RI) void k_corr_sym(const double *__restrict__ xT, int64_t ldx, int n, int d,
                                                        const double *__restrict__ coef, int hcols, double diag,
                                                        double *__restrict__ M, int64_t ld) {
    // 1-D grid over the 128x128 tiles of the LOWER triangle only (4 workgroups per tile): a 2-D grid with an early exit
    // for the strictly-upper tiles launches twice the workgroups and leaves the real ones unevenly spread over the CUs
    constexpr int NT = 1024 / RI;
    const int sub = blockIdx.x & 3;
    int I, J;
    tri_tile(blockIdx.x >> 2, I, J);
    const int bi = 2 * I + (sub >> 1), bj = 2 * J + (sub & 1);
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int dc = d < kCorrDC ? d : kCorrDC;
    double *xi = sm, *xj = sm + dc * 64;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    PairAcc<CORR> acc[RI][4];
    tile_pairs_staged<CORR, PRE, RI>(xi, xj, {xT, ldx, bi * 64}, {xT, ldx, bj * 64}, d, dc, coef, hcols, tid, ty, tx, false, acc,
                                     PRE ? coef : nullptr, NT);
    double r[RI][4];
#pragma unroll
    for (int a = 0; a < RI; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) r[a][b] = acc[a][b].value();
#pragma unroll
    for (int a = 0; a < RI; a++) {
        const int i = bi * 64 + ty * RI + a;
        double out[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int j = bj * 64 + tx * 4 + b;
            double v = r[a][b];
            if (i >= n || j >= n) v = (i == j) ? 1.0 : 0.0;  // identity padding
            else if (i == j) v = diag;                       // 1 + nugget, algorithm.rs:997
            out[b] = v;
        }
        double *p = M + (int64_t)i * ld + bj * 64 + tx * 4;
        *reinterpret_cast<double2 *>(p) = make_double2(out[0], out[1]);
        *reinterpret_cast<double2 *>(p + 2) = make_double2(out[2], out[3]);
    }
}
// K1, scalar-row form (round 3).  The 4x4-pairs-per-lane kernel above reads 8 doubles from LDS per 16 pairs and dimension:
// 4 ds_read_b128 per 32 FP64 instructions per wave keep the CU's one LDS pipe as busy as its four SIMDs, and the kernel
// sits at 0.78 of its FP64 VALU-issue bound.  Here a wave owns 16 ROWS x 64 columns (lane = column): the row coordinates
// are WAVE-UNIFORM, so they are fetched by the scalar unit (s_load) into SGPRs and enter the FP64 instructions as their
// scalar operand; only the lane's own column coordinate comes from LDS -- one ds_read_b64 per 32 instructions.  The inputs
// are read PRESCALED (xs[k][i] = c_k x[k][i], one tiny launch per candidate) so that nothing but the subtraction and the
// accumulation is left per pair and dimension.  Same 64x64 tile per workgroup, same grid, same stores (a row of 64 results
// per wave instruction: 512 contiguous bytes).
template <int CORR>
__device__ __forceinline__ void corr_sym_srow_body(const double *__restrict__ xs, int64_t ldx, int n, int d, double diag,
                                                   double *__restrict__ M, int64_t ld) {
    const int sub = blockIdx.x & 3;
    int I, J;
    tri_tile(blockIdx.x >> 2, I, J);
    const int bi = 2 * I + (sub >> 1), bj = 2 * J + (sub & 1);
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double *xj = sm;  // the 64 column points, k-major
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    stage_slab(xj, xs, ldx, bj * 64, d, tid);
    __syncthreads();
    const int i0 = bi * 64 + wave * 16;
    const double *xr = xs + i0;  // wave-uniform: rows i0 .. i0 + 15 of dimension k at xr[k * ldx + a]
    PairAcc<CORR> acc[16];
    for (int k = 0; k < d; k++) srow_step<CORR>(xr + (int64_t)k * ldx, xj[k * 64 + lane], acc);
    const int j = bj * 64 + lane;
#pragma unroll
    for (int a = 0; a < 16; a++) {
        const int i = i0 + a;
        double vv = acc[a].value();
        if (i >= n || j >= n) vv = (i == j) ? 1.0 : 0.0;  // identity padding
        else if (i == j) vv = diag;                       // 1 + nugget, algorithm.rs:997
        M[(int64_t)i * ld + j] = vv;
    }
}
template <int CORR>
__global__ __launch_bounds__(256) void k_corr_sym_srow(const double *__restrict__ xs, int64_t ldx, int n, int d, double diag,
                                                       double *__restrict__ M, int64_t ld) {
    corr_sym_srow_body<CORR>(xs, ldx, n, d, diag, M, ld);
}
// ... for the candidates of a lock-step batch in ONE launch (blockIdx.y = candidate): the same workgroups doing the same
// arithmetic, a twelfth of the launches (n = 4096 in lock-step 12: 12 x 3 front-end launches of ~20 + 5 + 5 us, serial on the
// lead's stream, were 4 % of a batch -- profiles/r05_n4096_lockstep12_timeline.txt)
template <int CORR>
__global__ __launch_bounds__(256) void k_corr_sym_srow_batch(EvalBatchPtrs b, int64_t ldx, int n, int d, double diag, int64_t ld) {
    corr_sym_srow_body<CORR>(b.xs[blockIdx.y], ldx, n, d, diag, b.M[blockIdx.y], ld);
}

__global__ void k_scale_rows_batch(EvalBatchPtrs b, int64_t ldx, int d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ldx) return;
    const double *xT = b.xT[blockIdx.y], *coef = b.coef[blockIdx.y];
    double *xs = b.xs[blockIdx.y];
    for (int k = 0; k < d; k++) xs[(int64_t)k * ldx + i] = coef[k] * xT[(int64_t)k * ldx + i];
}

// xs[k][i] = coef[k] * xT[k][i] over the (d x ldx) k-major array (hcols == 1)
__global__ void k_scale_rows(const double *__restrict__ xT, int64_t ldx, int d, const double *__restrict__ coef,
                             double *__restrict__ xs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ldx) return;
    for (int k = 0; k < d; k++) xs[(int64_t)k * ldx + i] = coef[k] * xT[(int64_t)k * ldx + i];
}

// Queries as the caller holds them (m x d row-major, raw) -> normalised and k-major (d x ldq, zero padded): what
// GaussianProcess::predict does first ((x - x_mean) / x_std, algorithm.rs:254).  The same IEEE subtraction and division
// as the host loop this replaces, so the bits are the same; a 64-query slab goes through LDS so that both the reads and
// the writes are contiguous.  par = x_mean (d) then x_std (d).
// blockIdx.z = member of a posterior batch (PosteriorBatchPtrs): its own normalisation, its query block sxq / sq doubles
// behind the previous member's.
// TYPED: a member with b.spec (mixint.h) gets its coordinates cast where they are read.  An Int / Ord coordinate is cast from
// itself; a coordinate of an Enum group needs the group's first maximum, and takes it over the WHOLE group from the raw row in
// global memory (a group may straddle the boundary between two chunks of kCorrDC dimensions: the chunk's part is not enough).
// The untyped instantiation is the kernel as it was.
template <bool TYPED>
__global__ __launch_bounds__(256) void k_normalize_queries(PosteriorBatchPtrs b, const double *__restrict__ xq_all, int64_t sxq,
                                                           int m, int d, double *__restrict__ xqT_all, int64_t ldq, int64_t sq) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const double *__restrict__ xq = xq_all + (int64_t)blockIdx.z * sxq;
    const double *__restrict__ par = b.par[blockIdx.z];
    double *__restrict__ xqT = xqT_all + (int64_t)blockIdx.z * sq;
    const int q0 = blockIdx.x * 64, tid = threadIdx.x;
    const int rows = (m - q0 < 64) ? (m - q0) : 64;
    // grid.y: chunks of kCorrDC dimensions (one for d <= 64)
    const int c0 = blockIdx.y * kCorrDC;
    const int dn = (d - c0 < kCorrDC) ? (d - c0) : kCorrDC;
    const int ds = dn | 1;  // odd row stride: the transposed reads below spread over the banks
    const mixint::Col *__restrict__ spec = TYPED ? b.spec[blockIdx.z] : nullptr;
    for (int e = tid; e < rows * dn; e += 256) {
        const int i = e / dn, k = e - i * dn;
        if (TYPED && spec)
            sm[i * ds + k] = mixint::cast_coord(spec, mixint::table_values(spec, d), xq + (int64_t)(q0 + i) * d, 1, c0 + k);
        else
            sm[i * ds + k] = xq[(int64_t)(q0 + i) * d + c0 + k];
    }
    __syncthreads();
    for (int e = tid; e < dn * 64; e += 256) {
        const int k = e >> 6, i = e & 63;
        xqT[(int64_t)(c0 + k) * ldq + q0 + i] = (i < rows) ? (sm[i * ds + k] - par[c0 + k]) / par[d + c0 + k] : 0.0;
    }
}

// blockIdx.z = member of a posterior batch: its own training inputs and coefficients, its query and output blocks sq / sR
// doubles behind the previous member's
template <int CORR, bool PRE>
__global__ __launch_bounds__(256) void k_cross_corr(PosteriorBatchPtrs b, const double *__restrict__ xqT_all, int64_t ldq, int64_t sq,
                                                    int64_t ldx, int d, int hcols, double *__restrict__ R_all, int64_t ld,
                                                    int64_t sR) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const double *__restrict__ xqT = xqT_all + (int64_t)blockIdx.z * sq;
    const double *__restrict__ xT = b.xT[blockIdx.z];
    const double *__restrict__ coef = b.coef[blockIdx.z];
    double *__restrict__ R = R_all + (int64_t)blockIdx.z * sR;
    const int dc = d < kCorrDC ? d : kCorrDC;
    double *xi = sm, *xj = sm + dc * 64;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    PairAcc<CORR> acc[4][4];
    tile_pairs_staged<CORR, PRE>(xi, xj, {xqT, ldq, (int)(blockIdx.x * 64)}, {xT, ldx, (int)(blockIdx.y * 64)}, d, dc, coef, hcols,
                                 tid, ty, tx, false, acc, PRE ? coef : nullptr);
    double r[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) r[a][b] = acc[a][b].value();
#pragma unroll
    for (int a = 0; a < 4; a++) {
        double *p = R + (int64_t)(blockIdx.x * 64 + ty * 4 + a) * ld + blockIdx.y * 64 + tx * 4;
        *reinterpret_cast<double2 *>(p) = make_double2(r[a][0], r[a][1]);
        *reinterpret_cast<double2 *>(p + 2) = make_double2(r[a][2], r[a][3]);
    }
}

// K2+K6 fused: racc[q] = sum_i k(xq, x_i) gamma_i ; one workgroup per 64 queries, loop over slabs.
// (blockIdx.z = member of a posterior batch, as in k_predict_mean_srow below)
template <int CORR, bool PRE>
__global__ __launch_bounds__(256) void k_predict_mean(PosteriorBatchPtrs b, const double *__restrict__ xqT_all, int64_t ldq,
                                                      int64_t sq, int64_t ldx, int n_pad, int d, int hcols,
                                                      double *__restrict__ racc_all, int64_t sracc, int slabs_per_split,
                                                      int m_pad) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const double *__restrict__ xqT = xqT_all + (int64_t)blockIdx.z * sq;
    const double *__restrict__ xT = b.xT[blockIdx.z];
    const double *__restrict__ coef = b.coef[blockIdx.z];
    const double *__restrict__ gamma = b.gamma[blockIdx.z];
    const int dc = d < kCorrDC ? d : kCorrDC;
    double *xi = sm, *xj = sm + dc * 64, *gs = sm + 2 * dc * 64;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    if (d <= dc) stage_slab(xi, xqT, ldq, blockIdx.x * 64, d, tid, PRE ? coef : nullptr);  // the queries: once
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    // grid.y splits the training range (a few queries must still fill the chip); partial sums per split
    const int j_lo = blockIdx.y * slabs_per_split * 64;
    int j_hi = j_lo + slabs_per_split * 64;
    if (j_hi > n_pad) j_hi = n_pad;
    for (int j0 = j_lo; j0 < j_hi; j0 += 64) {
        PairAcc<CORR> acc[4][4];
        for (int c0 = 0; c0 < d; c0 += dc) {
            const int dn = (d - c0 < dc) ? (d - c0) : dc;
            __syncthreads();
            if (d > dc) stage_slab(xi, xqT + (int64_t)c0 * ldq, ldq, blockIdx.x * 64, dn, tid, PRE ? coef + c0 : nullptr);
            stage_slab(xj, xT + (int64_t)c0 * ldx, ldx, j0, dn, tid, PRE ? coef + c0 : nullptr);
            if (c0 == 0 && tid < 64) gs[tid] = gamma[j0 + tid];
            __syncthreads();
            tile_pairs_acc<CORR, PRE>(xi, xj, coef + (int64_t)c0 * hcols, hcols, dn, ty, tx, acc);
        }
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) sum[a] = __builtin_fma(acc[a][b].value(), gs[tx * 4 + b], sum[a]);
    }
    // reduce over the 16 tx lanes that share the same queries (consecutive lanes of one wave)
#pragma unroll
    for (int a = 0; a < 4; a++) {
        double v = sum[a];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        v += __shfl_xor(v, 8);
        if (tx == 0) racc_all[(int64_t)blockIdx.z * sracc + (int64_t)blockIdx.y * m_pad + blockIdx.x * 64 + ty * 4 + a] = v;
    }
}

// K2+K6, scalar-row form (round 3; see k_corr_sym_srow): a lane owns ONE query of the workgroup's 64 (its prescaled
// coordinates in LDS, one ds_read_b64 per 32 FP64 instructions), the training points are the wave-uniform rows -- 16 at a
// time, fetched from the PRESCALED training inputs of the fit (xs = c_k x, k-major) by the scalar unit, gamma with them --
// and r . gamma accumulates in the lane's own register: no cross-lane reduction, no barrier inside the loop.  The four waves
// of a workgroup take every fourth 16-row block of the split's training range; their partial sums meet in LDS at the end.
// blockIdx.z = member of a posterior batch: a workgroup serves ONE member, so the member's prescaled rows and gamma stay
// wave-uniform (scalar loads); its query and partial-sum blocks sit sq / sracc doubles behind the previous member's.
template <int CORR>
__global__ __launch_bounds__(256) void k_predict_mean_srow(PosteriorBatchPtrs b, const double *__restrict__ xqT_all, int64_t ldq,
                                                           int64_t sq, int64_t ldx, int n_pad, int d,
                                                           double *__restrict__ racc_all, int64_t sracc, int slabs_per_split,
                                                           int m_pad) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const double *__restrict__ xqT = xqT_all + (int64_t)blockIdx.z * sq;
    const double *__restrict__ xs = b.xT[blockIdx.z];
    const double *__restrict__ coef = b.coef[blockIdx.z];
    const double *__restrict__ gamma = b.gamma[blockIdx.z];
    // (this workgroup's 64 sums: one pointer across the loop, not the five values it is made of)
    double *__restrict__ out = racc_all + ((int64_t)blockIdx.z * sracc + (int64_t)blockIdx.y * m_pad + blockIdx.x * 64);
    double *xq = sm, *part = sm + d * 64;  // 64 queries k-major, prescaled; 4 x 64 partial sums
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    stage_slab(xq, xqT, ldq, blockIdx.x * 64, d, tid, coef);
    __syncthreads();
    const int j_lo = blockIdx.y * slabs_per_split * 64;
    int j_hi = j_lo + slabs_per_split * 64;
    if (j_hi > n_pad) j_hi = n_pad;
    double sum = 0.0;
    for (int j0 = j_lo + wave * 16; j0 < j_hi; j0 += 64) {
        const double *xr = xs + j0;  // wave-uniform
        PairAcc<CORR> acc[16];
        for (int k = 0; k < d; k++) srow_step<CORR>(xr + (int64_t)k * ldx, xq[k * 64 + lane], acc);
        const double4 g0 = *reinterpret_cast<const double4 *>(gamma + j0);
        const double4 g1 = *reinterpret_cast<const double4 *>(gamma + j0 + 4);
        const double4 g2 = *reinterpret_cast<const double4 *>(gamma + j0 + 8);
        const double4 g3 = *reinterpret_cast<const double4 *>(gamma + j0 + 12);
        const double g[16] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w, g2.x, g2.y, g2.z, g2.w, g3.x, g3.y, g3.z, g3.w};
#pragma unroll
        for (int a = 0; a < 16; a++) sum = __builtin_fma(acc[a].value(), g[a], sum);
    }
    part[wave * 64 + lane] = sum;
    __syncthreads();
    if (tid < 64)
        out[tid] = (part[tid] + part[64 + tid]) + (part[128 + tid] + part[192 + tid]);
}

// ---------------------------------------------------------------------------------------------
// x-gradients of the predictions (CorrelationModel::jacobian, correlation_models.rs:106-123, 198-214,
// 355-413, 524-586, contracted as predict_jacobian / predict_var_gradients_single do, algorithm.rs:523-617):
//     out[a][k] = sum_j w(j, a) * d r(x_a, x_j) / d x_ak
// with w = gamma_j (mean, VEC) or a per-(j, a) weight matrix held TRANSPOSED (n x m: lanes <-> queries, coalesced).
// The (n, d) jacobian of one query never exists: one lane per query, training slabs broadcast from LDS, the d
// partial sums of a lane live in registers (DK at a time).  grid.y splits the training range for small batches
// (EGO asks for one point at a time); the partial sums of the splits are added on the host.
// d r / d x_k = r * g_k(x_ak - x_jk):
//   sq-exp   g = -c_k^2 diff                      abs-exp  g = -c_k sign(diff)
//   Matern   g = sign(diff) sum_l c_kl (f'(t_l) / f(t_l) - q),  t_l = c_kl |diff|,  f = 1 + q t [+ 5/3 t^2]
// (the closed form of the reference's product-over-all-but-one loops; sign(+0) = +1 like f64::signum).
// ---------------------------------------------------------------------------------------------
constexpr int kXgThreads = 128;
// A wave-uniform read of memory that nothing writes while the kernel runs, through the constant address space: a scalar load
// whatever the compiler can prove about aliasing (a pointer taken from a by-value pointer block carries no __restrict__)
__device__ __forceinline__ double uniform_ld(const double *p) {
    return *(const __attribute__((address_space(4))) double *)p;
}
constexpr size_t kLdsBytes = 160 * 1024;  // LDS of one CU (gfx950)

// blockIdx.z = member of a posterior batch (a workgroup serves ONE member): its own training inputs, coefficients and -- VEC --
// weight vector, its query block, weight matrix and partial sums sq / sW / sout doubles behind the previous member's.
// XAG (d > 64): the lane's own query coordinates come from global memory (L1 / L2) instead of a [d][kXgThreads] LDS
// image, which together with the training slab would not fit any more; the slab is [d][2^js_shift] training points,
// 64 wide up to d = 256 and narrower beyond (launch_xgrad picks the widest that fits the 160 KB of LDS)
// LIST: the COLUMN-LIST form (an infill handle with active coordinates, egx_infill_set_active): out[a][c] for the ncols listed
// columns c = cols[0 .. ncols) alone, DK of them per pass -- the pair correlation runs over all d coordinates once per DK LISTED
// columns instead of once per DK columns of d.  Every unlisted column of the lane's d-wide row is written +0.0 (the lane owns
// its row: the fill and the later stores of the listed columns are the same thread's, in program order), so whatever reads the
// partial sums downstream sees defined values everywhere.  The two forms differ in which columns a pass holds (cols[c0 + kk]
// against c0 + kk) and in that fill, nothing else: a listed column accumulates the same __builtin_fma sequence and has the
// full form's bits (tests/test_gpu_infill_active.py).  cols: distinct, in [0, d), in any order (checked on the host,
// infill_active.h); without LIST, cols and ncols are not read.
template <int CORR, int DK, bool VEC, bool XAG = false, bool LIST = false>
__global__ __launch_bounds__(kXgThreads) void k_xgrad(PosteriorBatchPtrs b, const double *__restrict__ xqT_all, int64_t ldq,
                                                      int64_t sq, int64_t ldx, int n, int d, int hcols,
                                                      const double *__restrict__ Wt_all, int64_t ldw, int64_t sW,
                                                      int slabs_per_split, double *__restrict__ out_all, int64_t sout,
                                                      int m_pad, int js_shift, const int *__restrict__ cols, int ncols) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const double *__restrict__ xqT = xqT_all + (int64_t)blockIdx.z * sq;
    const double *__restrict__ xT = b.xT[blockIdx.z];
    const double *__restrict__ coef = b.coef[blockIdx.z];
    const double *__restrict__ Wt = VEC ? b.gamma[blockIdx.z] : Wt_all + (int64_t)blockIdx.z * sW;
    double *__restrict__ out = out_all + (int64_t)blockIdx.z * sout;
    const int jsh = XAG ? js_shift : 6, JS = 1 << jsh;
    double *xa = sm;                                  // [d][kXgThreads]  (not with XAG)
    double *xj = sm + (XAG ? 0 : d * kXgThreads);     // [d][JS]
    double *cs = xj + d * JS;                         // [d * hcols]
    const int tid = threadIdx.x;
    const int a = blockIdx.x * kXgThreads + tid;
    const double *xag = xqT + a;
#define EGX_XA(k_) (XAG ? xag[(int64_t)(k_) * ldq] : xa[(k_) * kXgThreads + tid])
    if (!XAG)
        for (int k = 0; k < d; k++) xa[k * kXgThreads + tid] = xqT[(int64_t)k * ldq + a];
    for (int e = tid; e < d * hcols; e += kXgThreads) cs[e] = coef[e];
    const int j_lo = blockIdx.y * slabs_per_split * 64;
    int j_hi = j_lo + slabs_per_split * 64;
    if (j_hi > n) j_hi = n;
    double *o = out + ((int64_t)blockIdx.y * m_pad + a) * d;
    if (LIST)
        for (int k = 0; k < d; k++) o[k] = 0.0;
    const int nc = LIST ? ncols : d;  // the columns to produce, DK per pass
    for (int c0 = 0; c0 < nc; c0 += DK) {
        double acc[DK], xr[DK];
        int col[DK];
#pragma unroll
        for (int kk = 0; kk < DK; kk++) {
            col[kk] = !LIST ? c0 + kk : ((c0 + kk < nc) ? cols[c0 + kk] : 0);
            acc[kk] = 0.0;
            xr[kk] = (c0 + kk < nc) ? EGX_XA(col[kk]) : 0.0;
        }
        for (int j0 = j_lo; j0 < j_hi; j0 += JS) {
            __syncthreads();
            for (int e = tid; e < d * JS; e += kXgThreads) xj[e] = xT[(int64_t)(e >> jsh) * ldx + j0 + (e & (JS - 1))];
            __syncthreads();
            const int jn = (j_hi - j0 < JS) ? (j_hi - j0) : JS;
            for (int jj = 0; jj < jn; jj++) {
                PairAcc<CORR> pa;
                for (int k = 0; k < d; k++) pa.add(EGX_XA(k) - xj[k * JS + jj], cs + k * hcols, hcols);
                const double wv = VEC ? uniform_ld(Wt + j0 + jj) : Wt[(int64_t)(j0 + jj) * ldw + a];
                const double rw = pa.value() * wv;
#pragma unroll
                for (int kk = 0; kk < DK; kk++)
                    if (c0 + kk < nc)
                        acc[kk] = __builtin_fma(rw, xgrad_factor<CORR>(xr[kk] - xj[col[kk] * JS + jj],
                                                                       cs + col[kk] * hcols, hcols), acc[kk]);
            }
        }
#pragma unroll
        for (int kk = 0; kk < DK; kk++)
            if (c0 + kk < nc) o[col[kk]] = acc[kk];
    }
#undef EGX_XA
}

// Few-query form of the x-gradient contraction (single-point calls): the lanes run over TRAINING points instead of queries
// (one pair per lane, no sequential pair loop), the d partial sums are reduced across the workgroup.
//   out[(blockIdx.y * m + a) * d + k] = sum over the block's 256 training points of w_j d r(x_a, x_j) / d x_ak
template <int CORR>
__global__ __launch_bounds__(256) void k_xgrad_point(const double *__restrict__ xqT, int64_t ldq, const double *__restrict__ xT,
                                                     int64_t ldx, int n, int d, const double *__restrict__ coef, int hcols,
                                                     const double *__restrict__ wvec, double *__restrict__ out, int m) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double *xa = sm;            // [d]
    double *cs = sm + d;        // [d * hcols]
    double *red = cs + d * hcols;  // [4][d]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int a = blockIdx.x, j = blockIdx.y * 256 + tid;
    for (int k = tid; k < d; k += 256) xa[k] = xqT[(int64_t)k * ldq + a];
    for (int e = tid; e < d * hcols; e += 256) cs[e] = coef[e];
    __syncthreads();
    const bool live = j < n;
    double rw = 0.0;
    if (live) {
        PairAcc<CORR> pa;
        for (int k = 0; k < d; k++) pa.add(xa[k] - xT[(int64_t)k * ldx + j], cs + k * hcols, hcols);
        rw = pa.value() * wvec[j];
    }
    for (int k = 0; k < d; k++) {
        double v = live ? rw * xgrad_factor<CORR>(xa[k] - xT[(int64_t)k * ldx + j], cs + k * hcols, hcols) : 0.0;
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wave * d + k] = v;
    }
    __syncthreads();
    for (int k = tid; k < d; k += 256)
        out[((int64_t)blockIdx.y * m + a) * d + k] = ((red[k] + red[d + k]) + red[2 * d + k]) + red[3 * d + k];
}

// ---------------------------------------------------------------------------------------------
// Single-point path of the variance (and its x-gradient): with W = C^-T cached (upper triangular, row-major)
//   y = C^-1 r = W^T r      k_uptri_gemv_t  (rows split over grid.y, partial sums to P, summed in a fixed order)
//   z = C^-T y = W y        k_uptri_gemv    (one wave per row, coalesced)
// Two memory-bound passes over half of W instead of 2 x 64 dependent block solves: EGO asks for ONE point at a time.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_uptri_gemv_t(const double *__restrict__ W, int64_t ld, int n,
                                                      const double *__restrict__ r, int rows_per_split,
                                                      double *__restrict__ P, int n_pad) {
    __shared__ double red[4][64];
    const int tid = threadIdx.x, g = tid >> 6, jl = tid & 63;
    const int j = blockIdx.x * 64 + jl;
    const int i_lo = blockIdx.y * rows_per_split;
    int i_hi = i_lo + rows_per_split;
    const int jmax = blockIdx.x * 64 + 63;  // rows beyond the last column of this block are zero (upper triangular)
    if (i_hi > jmax + 1) i_hi = jmax + 1;
    if (i_hi > n) i_hi = n;
    double part = 0.0;
    for (int i0 = i_lo + g; i0 < i_hi; i0 += 32) {  // 8 independent loads in flight per lane
        double mv[8], rv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int i = i0 + 4 * u;
            const bool ok = i < i_hi;
            mv[u] = ok ? W[(int64_t)i * ld + j] : 0.0;
            rv[u] = ok ? r[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) part = __builtin_fma(mv[u], rv[u], part);
    }
    red[g][jl] = part;
    __syncthreads();
    if (g == 0) P[(int64_t)blockIdx.y * n_pad + j] = ((red[0][jl] + red[1][jl]) + red[2][jl]) + red[3][jl];
}

__global__ void k_sum_partials(const double *__restrict__ P, int nsplit, int n_pad, double *__restrict__ y) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_pad) return;
    double sacc = 0.0;
    for (int sp = 0; sp < nsplit; sp++) sacc += P[(int64_t)sp * n_pad + j];
    y[j] = sacc;
}

// z[a][i] = (base ? base[a][i] + sc * acc : acc), acc = sum_{k >= i} W[i][k] y[a][k], for the rows a = blockIdx.y of y / base / z
// (ldr apart): a wave per (row of W, right-hand side).  base may be z itself (an element is read by the lane that writes it).
// (one row's sum, complete in every lane of its wave: the ONE text both kernels below run)
__device__ __forceinline__ double uptri_row_dot(const double *__restrict__ W, int64_t ld, int n, const double *y, int i, int lane) {
    const double *row = W + (int64_t)i * ld;
    double acc = 0.0;
    for (int k = (i & ~63) + lane; k < n; k += 64) acc = __builtin_fma((k >= i) ? row[k] : 0.0, y[k], acc);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    return acc;
}
__global__ __launch_bounds__(256) void k_uptri_gemv(const double *__restrict__ W, int64_t ld, int n, const double *y,
                                                    const double *base, double sc, double *z, int64_t ldr) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    y += (int64_t)blockIdx.y * ldr;
    const double acc = uptri_row_dot(W, ld, n, y, i, lane);
    if (lane == 0) {
        const int64_t e = (int64_t)blockIdx.y * ldr + i;
        z[e] = base ? base[e] + sc * acc : acc;
    }
}
// z[j] = W_j y[j] for the matrices W_j = W + j sW of a lock-step run (blockIdx.y = j: a candidate of one handle, or a member of
// a group with its C^-T in the group's slab): the rows, the waves and the order of every sum are k_uptri_gemv's
__global__ __launch_bounds__(256) void k_uptri_gemv_batch(const double *__restrict__ W, int64_t sW, int64_t ld, int n, GemvBatchPtrs b) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const int j = blockIdx.y;
    const double acc = uptri_row_dot(W + (int64_t)j * sW, ld, n, b.y[j], i, lane);
    if (lane == 0) b.z[j][i] = acc;
}

__global__ void k_fill_rows(double *__restrict__ M, int64_t ld, int r0, int rows_pad, const double *__restrict__ src,
                            int64_t lds, int nrows, int ncols) {
    const int64_t total = (int64_t)rows_pad * ld;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int l = (int)(e / ld);
        const int i = (int)(e % ld);
        M[(int64_t)(r0 + l) * ld + i] = (l < nrows && i < ncols) ? src[(int64_t)l * lds + i] : 0.0;
    }
}

__global__ void k_gather_diag(const double *__restrict__ M, int64_t ld, int n, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = M[(int64_t)i * ld + i];
}

__global__ void k_fill_rows_batch(EvalBatchPtrs b, int64_t ld, int r0, int rows_pad, int64_t lds, int nrows, int ncols) {
    double *M = b.M[blockIdx.y];
    const double *src = b.rhsT[blockIdx.y];
    const int64_t total = (int64_t)rows_pad * ld;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int l = (int)(e / ld);
        const int i = (int)(e % ld);
        M[(int64_t)(r0 + l) * ld + i] = (l < nrows && i < ncols) ? src[(int64_t)l * lds + i] : 0.0;
    }
}

// What the host needs of `count` finished evaluations, written STRAIGHT into each candidate's pinned host buffers (device-
// visible, fine grained: complete when the launch is) by one launch: blockIdx.z = candidate, blockIdx.y = 0: the factor's
// diagonal (n), 1 .. q: the solved right-hand-side rows (q x n_pad, only with `rows`), plus `info` and the eight hand-off
// diagnostics words of the chain launches.  Replaces a gather kernel and four device-to-host copies PER CANDIDATE (~38 us
// each, serial on the lead's stream: 0.46 ms of the 8.7 ms of twelve n = 4096 candidates).
__global__ __launch_bounds__(256) void k_eval_tail(EvalBatchPtrs b, int64_t ld, int n, int n_pad, int rows, const int *__restrict__ sync) {
    const int z = blockIdx.z, y = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double *M = b.M[z];
    if (y == 0) {
        if (i < n) b.h_diag[z][i] = M[(int64_t)i * ld + i];
        if (i < 9) b.h_info[z][i] = (i == 0) ? *b.d_info[z] : (sync ? sync[i - 1] : 0);
    } else if (rows && i < n_pad) {
        b.h_rows[z][(int64_t)(y - 1) * n_pad + i] = M[(int64_t)(n_pad + y - 1) * ld + i];
    }
}

// Device-side GLS (algorithm.rs:1007-1032 for p > 1 trend columns), helpers around the Gram matrix of [ft | yt]:
// G (rows x rows, ldg) <- -Gneg on the lower triangle of the leading q x q block, identity on the padding diagonal
__global__ void k_gram_finish(const double *__restrict__ Gneg, double *__restrict__ G, int64_t ldg, int rows, int q) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= rows) return;
    double v = 0.0;
    if (i < q && j <= i) v = -Gneg[(int64_t)i * ldg + j];
    else if (i >= q && j == i) v = 1.0;
    G[(int64_t)i * ldg + j] = v;
}

// rho (n_pad, zero beyond n) <- yt - sum_l beta_l ft_l  (ft_l = row l of ftT);  part[block] <- sum of rho^2 over the
// block's 256 points, reduced in a fixed order (the host adds the n_pad / 256 partial sums in order: deterministic)
__global__ __launch_bounds__(256) void k_gls_residual(const double *__restrict__ ftT, int64_t ld, const double *__restrict__ yt,
                                                      const double *__restrict__ beta, int p, int n, int n_pad,
                                                      double *__restrict__ rho, double *__restrict__ part) {
    __shared__ double bs[256];
    __shared__ double red[256];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    double acc = (i < n) ? yt[i] : 0.0;
    for (int l0 = 0; l0 < p; l0 += 256) {
        const int cnt = (p - l0 < 256) ? (p - l0) : 256;
        __syncthreads();
        if (tid < cnt) bs[tid] = beta[l0 + tid];
        __syncthreads();
        if (i < n)
            for (int l = 0; l < cnt; l++) acc = __builtin_fma(-bs[l], ftT[(int64_t)(l0 + l) * ld + i], acc);
    }
    if (i < n_pad) rho[i] = acc;
    red[tid] = acc * acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) part[blockIdx.x] = red[0];
}

__global__ void k_zero_upper(double *__restrict__ M, int64_t ld, int n) {
    const int64_t total = (int64_t)n * n;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(e / n), j = (int)(e % n);
        if (j > i) M[(int64_t)i * ld + j] = 0.0;
    }
}

// one wave per query row: s0 = sum_i rt_i^2 ; sl[l] = sum_i rt_i * ft_l[i]
// blockIdx.y = member of a posterior batch: its own ft^T rows; its RT, s0 and sl blocks sR, ss0, ssl doubles apart
__global__ __launch_bounds__(256) void k_row_reduce(PosteriorBatchPtrs b, const double *__restrict__ RT_all, int64_t ld, int64_t sR,
                                                    int m, int n, int64_t ldf, int p, double *__restrict__ s0_all, int64_t ss0,
                                                    double *__restrict__ sl_all, int64_t ssl) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (q >= m) return;
    const double *__restrict__ RT = RT_all + (int64_t)blockIdx.y * sR;
    const double *__restrict__ ftT = b.ftT[blockIdx.y];
    double *__restrict__ s0 = s0_all + (int64_t)blockIdx.y * ss0;
    double *__restrict__ sl = sl_all + (int64_t)blockIdx.y * ssl;
    const double *row = RT + (int64_t)q * ld;
    double acc = 0.0;
    for (int i = lane; i < n; i += 64) acc = __builtin_fma(row[i], row[i], acc);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) s0[q] = acc;
    for (int l = 0; l < p; l++) {
        const double *f = ftT + (int64_t)l * ldf;
        double a2 = 0.0;
        for (int i = lane; i < n; i += 64) a2 = __builtin_fma(row[i], f[i], a2);
        for (int o = 32; o > 0; o >>= 1) a2 += __shfl_xor(a2, o);
        if (lane == 0) sl[(int64_t)q * p + l] = a2;
    }
}

// ---------------------------------------------------------------------------------------------
// K7: likelihood-gradient accumulation (new capability).  With Rneg = -R^-1 (lower triangle) and
// gamma = C^-T rho, for every output o < nout
//     out[o] = sum_{i > j} 2 R_ij (gamma_i gamma_j / sigma2 + Rneg_ij) * d log R_ij / d c_o
//            = gamma^T dR_o gamma / sigma2 - tr(R^-1 dR_o)
// hcols == 1 (HC1): output o = input dimension o, c_o its coefficient (w = I: theta_o; KPLS sq-exp / abs-exp: the collapsed
// coefficient, the chain rule to theta runs on the host);  hcols > 1 (KPLS + Matern): output o = theta_o,
//     d log R / d theta_o = sum_j |w_jo| (d log m / d t)(theta_o |w_jo| a_j) a_j.
// d log r / d c for one dimension (a = |x_i - x_j|, t = c a):
//     sq-exp -c a^2 ; abs-exp -a ; Matern-3/2 -3 a t / (1 + s3 t) ; Matern-5/2 -(5/3) a t (1 + s5 t) / (1 + s5 t + 5/3 t^2)
// (the Matern forms are m'(t) / m(t) - sqrt(nu') with the constants cancelled: one reciprocal, no subtraction of nearly
// equal terms).
// Round 4: DETERMINISTIC (round 3 added per-tile sums into `out` with atomics, whose order varies from run to run): a
// workgroup walks the 64 x 64 tiles t = blockIdx.x, + gridDim.x, ... of the lower triangle, keeps its DK partial sums
// per lane in registers over all of them, reduces them once (shuffles, then the four waves in a fixed order) and writes
// ONE partial vector; k_grad_reduce adds the workgroups' vectors in a fixed order.  A candidate's gradient is therefore
// the same bits alone and in a lock-step batch (grid.z), whatever else runs.  Two passes per tile: (1) all d dimensions
// -> R_ij and the pair's weight, (2) the DK outputs of this workgroup's chunk (grid.y) -> DK accumulations per pair.
// Dimensions are staged in LDS in chunks of at most 64 (any d).  The division of round 3 (~30 FP64 instructions per pair
// and dimension) is v_rcp_f64 + two Newton steps (m >= 1: no scaling needed).
// ---------------------------------------------------------------------------------------------
constexpr int kGradDC = 64;      // input dimensions staged per pass (2 x 64 x 64 doubles = 64 KB of LDS)
constexpr int kGradMaxWG = 2048;  // workgroups (partial vectors) per candidate and output chunk

// (rcp_ge1 and dlog_dc, the raw-coefficient form of d log r / d c: corr_pair.h)
// The same with the coefficient already inside the distance (t = c a; HC1 with every c > 0, inputs prescaled as for K1's
// scalar-row form): d log r / d c = F(c) G(t) with G below and F = -1/c (sq-exp, abs-exp), -3/c (Matern-3/2),
// -(5/3)/c (Matern-5/2) applied once per output when the partial sum is written.  One Newton step on v_rcp_f64 (2^-26
// or better, squared: the last bit of a double; the gradient is asserted at 1e-6).
__device__ __forceinline__ double rcp_ge1_fast(double m) {
    const double y = __builtin_amdgcn_rcp(m);
    return __builtin_fma(__builtin_fma(-m, y, 1.0), y, y);
}
template <int CORR>
__device__ __forceinline__ double dlog_g_scaled(double t) {  // t >= 0
    if (CORR == EGX_CORR_SQUARED_EXPONENTIAL) return t * t;
    if (CORR == EGX_CORR_ABSOLUTE_EXPONENTIAL) return t;
    const double t2 = t * t;
    if (CORR == EGX_CORR_MATERN32) return t2 * rcp_ge1_fast(__builtin_fma(kSqrt3, t, 1.0));
    const double u = __builtin_fma(kSqrt5, t, 1.0);
    return (t2 * u) * rcp_ge1_fast(__builtin_fma(k5over3, t2, u));
}
template <int CORR>
__device__ __forceinline__ double dlog_f_scaled(double c) {
    if (CORR == EGX_CORR_MATERN32) return -3.0 / c;
    if (CORR == EGX_CORR_MATERN52) return -k5over3 / c;
    return -1.0 / c;
}

// MODE 0: hcols > 1 (KPLS + Matern);  1: hcols == 1, raw inputs;  2: hcols == 1, inputs prescaled per candidate (gb.xs)
template <int CORR, int MODE, int DK>
__global__ __launch_bounds__(256) void k_grad_accum(int64_t ldx, int n, int d, int hcols, const double *__restrict__ wabs, int nout,
                                                    int64_t ld, int ntiles, int nout_pad, GradBatch gb) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int z = blockIdx.z;
    constexpr bool HC1 = MODE != 0, PRE = MODE == 2;
    // this entry's c_k x_k (k-major like xT), or its OWNER's inputs: one scalar load of a kernel argument either way -- the
    // members of a group have a training set each
    const double *__restrict__ xT = PRE ? gb.xs[z] : gb.xT[z];
    const double *__restrict__ coef = gb.coef[z];
    const double *__restrict__ gamma = gb.gamma[z];
    const double *__restrict__ Rneg = gb.rneg[z];
    const double inv_s2 = gb.inv_s2[z];
    const int dc = d < kGradDC ? d : kGradDC;
    double *xi = sm, *xj = sm + dc * 64;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int o0 = blockIdx.y * DK;
    double acc[DK];
#pragma unroll
    for (int oo = 0; oo < DK; oo++) acc[oo] = 0.0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int bi, bj;
        tri_tile(t, bi, bj);
        const SlabSrc si{xT, ldx, bi * 64}, sj{xT, ldx, bj * 64};
        // ---- pass 1: the correlations of the tile's 16 pairs per lane (all d dimensions, staged dc at a time; PRE: the
        // inputs come prescaled, nothing is applied while staging)
        PairAcc<CORR> pa[4][4];
        tile_pairs_staged<CORR, PRE>(xi, xj, si, sj, d, dc, coef, hcols, tid, ty, tx, true, pa);
        double wp[4][4];  // 2 R_ij (gamma_i gamma_j / sigma2 - Rinv_ij) for i > j inside the matrix, else 0
        {
            double gi[4], gj[4];
#pragma unroll
            for (int a = 0; a < 4; a++) gi[a] = gamma[bi * 64 + ty * 4 + a] * inv_s2;
#pragma unroll
            for (int b = 0; b < 4; b++) gj[b] = gamma[bj * 64 + tx * 4 + b];
#pragma unroll
            for (int a = 0; a < 4; a++) {
                const int i = bi * 64 + ty * 4 + a;
                const double *rrow = Rneg + (int64_t)i * ld + bj * 64 + tx * 4;
                const double2 r01 = *reinterpret_cast<const double2 *>(rrow);
                const double2 r23 = *reinterpret_cast<const double2 *>(rrow + 2);
                const double rn[4] = {r01.x, r01.y, r23.x, r23.y};
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int j = bj * 64 + tx * 4 + b;
                    const bool on = (i > j) && (i < n);
                    wp[a][b] = on ? 2.0 * pa[a][b].value() * __builtin_fma(gi[a], gj[b], rn[b]) : 0.0;
                }
            }
        }
        // ---- pass 2: this workgroup's outputs o0 .. o0 + DK - 1
        if (HC1) {
            // output o <-> input dimension o.  d > dc: the chunk's dimensions are staged again, from slab row 0
            int base = 0;
            if (d > dc) {
                stage_pair(xi, xj, si.from(o0), sj.from(o0), (nout - o0 < DK) ? (nout - o0) : DK, tid, true);
                base = o0;
            }
#pragma unroll
            for (int oo = 0; oo < DK; oo++) {
                const int o = o0 + oo;
                if (o < nout) {
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
                        for (int b = 0; b < 4; b++) {
                            const double ad = fabs(vi[a] - vj[b]);
                            sacc = __builtin_fma(wp[a][b], PRE ? dlog_g_scaled<CORR>(ad) : dlog_dc<CORR>(c, ad), sacc);
                        }
                    acc[oo] = sacc;
                }
            }
        } else {
            // KPLS + Matern: output o = theta_o gets a term from every input dimension j
            for (int c0 = 0; c0 < d; c0 += dc) {
                const int dn = (d - c0 < dc) ? (d - c0) : dc;
                if (d > dc) stage_pair(xi, xj, si.from(c0), sj.from(c0), dn, tid, true);
                for (int k = 0; k < dn; k++) {
                    double ad[4][4];
                    {
                        double vi[4], vj[4];
#pragma unroll
                        for (int a = 0; a < 4; a++) vi[a] = xi[k * 64 + ty * 4 + a];
#pragma unroll
                        for (int b = 0; b < 4; b++) vj[b] = xj[k * 64 + tx * 4 + b];
#pragma unroll
                        for (int a = 0; a < 4; a++)
#pragma unroll
                            for (int b = 0; b < 4; b++) ad[a][b] = fabs(vi[a] - vj[b]);
                    }
#pragma unroll
                    for (int oo = 0; oo < DK; oo++) {
                        const int o = o0 + oo;
                        if (o < nout) {
                            const double c = coef[(int64_t)(c0 + k) * hcols + o], wa = wabs[(int64_t)(c0 + k) * hcols + o];
                            if (wa != 0.0) {  // (wave-uniform)
                                double sacc = 0.0;
#pragma unroll
                                for (int a = 0; a < 4; a++)
#pragma unroll
                                    for (int b = 0; b < 4; b++) sacc = __builtin_fma(wp[a][b], dlog_dc<CORR>(c, ad[a][b]), sacc);
                                acc[oo] = __builtin_fma(wa, sacc, acc[oo]);
                            }
                        }
                    }
                }
            }
        }
    }
    // ---- one reduction per workgroup: lanes of a wave (xor shuffles), then the four waves in a fixed order
    double v = wg_sum_dk<DK>(acc, sm, tid);
    if (tid < DK && o0 + tid < nout) {
        if (PRE) v *= dlog_f_scaled<CORR>(coef[o0 + tid]);
        gb.part[z][(int64_t)blockIdx.x * nout_pad + o0 + tid] = v;
    }
}

// out[z][o] = sum over the nwg partial vectors, in a fixed order: 256 lanes take every 256th, then a tree in LDS
__global__ __launch_bounds__(256) void k_grad_reduce(int nwg, int nout, int nout_pad, GradBatch gb) {
    const int o = blockIdx.x, z = blockIdx.y, tid = threadIdx.x;
    const double v = sum_partial_vectors(gb.part[z], nwg, nout_pad, o, tid);
    if (tid == 0) gb.out[z][o] = v;
}

// =============================================================================================
// (EGX_DISPATCH_CORR, the switch from the run-time correlation kind to the template argument C_: egx_internal.h)
int launch_corr_sym(hipStream_t s, int corr, const double *xT, int64_t ldx, int n, int d, const double *coef,
                    int hcols, double nugget, double *M, int64_t ld, int n_pad, double *xs_scratch) {
    const int nt2 = n_pad / 128;  // n_pad is a multiple of 128
    dim3 grid((unsigned)(4 * (nt2 * (nt2 + 1) / 2)));
    const int dc = d < kCorrDC ? d : kCorrDC;  // dimensions staged at a time
    const size_t lds = (size_t)2 * dc * 64 * sizeof(double);
    // (the LDS-only form was measured against it: 0.51 vs 0.42 ms sq-exp, 1.10 vs 0.76 at d = 64: profiles/r03_run11_k1_scalar_rows_ab.txt)
    if (hcols == 1 && xs_scratch != nullptr && d <= kCorrDC) {
        // scalar-row form on prescaled inputs (xs_scratch: d x ldx doubles, owned by the caller's workspace); d > 64: the
        // LDS-only form below, which stages the dimensions in chunks
        hipLaunchKernelGGL(k_scale_rows, dim3((unsigned)((ldx + 255) / 256)), dim3(256), 0, s, xT, ldx, d, coef, xs_scratch);
        EGX_DISPATCH_CORR(corr, hipLaunchKernelGGL((k_corr_sym_srow<C_>), grid, dim3(256), lds / 2, s, (const double *)xs_scratch, ldx,
                                                   n, d, 1.0 + nugget, M, ld));
        EGX_HIP_CHECK(hipGetLastError());
        return EGX_SUCCESS;
    }
    // (forms with more pairs per lane -- 8 x 4 in a 128x128 tile or in the same tile with 128 threads -- were measured SLOWER:
    //  profiles/r03_run5_k1_tile128_discarded.jsonl, profiles/r03_run10_k1_rows8_discarded.txt)
    if (hcols == 1) {
        EGX_DISPATCH_CORR(corr, hipLaunchKernelGGL((k_corr_sym<C_, true, 4>), grid, dim3(256), lds, s, xT, ldx, n, d, coef, hcols,
                                                   1.0 + nugget, M, ld));
    } else {
        EGX_DISPATCH_CORR(corr, hipLaunchKernelGGL((k_corr_sym<C_, false, 4>), grid, dim3(256), lds, s, xT, ldx, n, d, coef, hcols,
                                                   1.0 + nugget, M, ld));
    }
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

static bool posterior_count_ok(const PosteriorBatch &pb) {
    if (pb.count >= 1 && pb.count <= kLockstepMax) return true;
    set_error("posterior batch: count out of range");
    return false;
}

int launch_cross_corr(hipStream_t s, int corr, const PosteriorBatch &pb, const double *xqT, int64_t ldq, int m_pad, int64_t ldx,
                      int n_pad, int d, int hcols, double *R, int64_t ld) {
    if (!posterior_count_ok(pb)) return EGX_ERR_INVALID_VALUE;
    dim3 grid(m_pad / 64, n_pad / 64, (unsigned)pb.count);
    const size_t lds = (size_t)2 * (d < kCorrDC ? d : kCorrDC) * 64 * sizeof(double);
    if (hcols == 1) {
        EGX_DISPATCH_CORR(corr, hipLaunchKernelGGL((k_cross_corr<C_, true>), grid, dim3(256), lds, s, pb.ptrs, xqT, ldq, pb.sq, ldx, d,
                                                   hcols, R, ld, pb.sR));
    } else {
        EGX_DISPATCH_CORR(corr, hipLaunchKernelGGL((k_cross_corr<C_, false>), grid, dim3(256), lds, s, pb.ptrs, xqT, ldq, pb.sq, ldx, d,
                                                   hcols, R, ld, pb.sR));
    }
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_normalize_queries(hipStream_t s, const PosteriorBatch &pb, const double *xq, int64_t sxq, int m, int d, double *xqT,
                             int64_t ldq, int m_pad) {
    if (!posterior_count_ok(pb)) return EGX_ERR_INVALID_VALUE;
    const size_t lds = (size_t)64 * ((d < kCorrDC ? d : kCorrDC) | 1) * sizeof(double);
    bool typed = false;
    for (int j = 0; j < pb.count; j++) typed = typed || pb.ptrs.spec[j] != nullptr;
    const dim3 grid(m_pad / 64, (unsigned)((d + kCorrDC - 1) / kCorrDC), (unsigned)pb.count);
    if (typed) hipLaunchKernelGGL(k_normalize_queries<true>, grid, dim3(256), lds, s, pb.ptrs, xq, sxq, m, d, xqT, ldq, pb.sq);
    else hipLaunchKernelGGL(k_normalize_queries<false>, grid, dim3(256), lds, s, pb.ptrs, xq, sxq, m, d, xqT, ldq, pb.sq);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_scale_rows(hipStream_t s, const double *xT, int64_t ldx, int d, const double *coef, double *xs) {
    hipLaunchKernelGGL(k_scale_rows, dim3((unsigned)((ldx + 255) / 256)), dim3(256), 0, s, xT, ldx, d, coef, xs);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

bool predict_mean_prescaled(int d, int hcols) { return hcols == 1 && d <= kCorrDC; }

// pb.ptrs.xT: the members' training inputs, or (prescaled != 0: predict_mean_prescaled) the same times the coefficients of the fit
int launch_predict_mean(hipStream_t s, int corr, const PosteriorBatch &pb, const double *xqT, int64_t ldq, int m_pad, int64_t ldx,
                        int n_pad, int d, int hcols, double *racc, int nsplit, int prescaled) {
    if (!posterior_count_ok(pb)) return EGX_ERR_INVALID_VALUE;
    const size_t lds = (size_t)(2 * (d < kCorrDC ? d : kCorrDC) * 64 + 64) * sizeof(double);
    const int slabs = n_pad / 64;
    if (nsplit < 1) nsplit = 1;
    if (nsplit > slabs) nsplit = slabs;
    const int per = (slabs + nsplit - 1) / nsplit;
    nsplit = (slabs + per - 1) / per;
    const dim3 grid(m_pad / 64, nsplit, (unsigned)pb.count);
    if (prescaled && !predict_mean_prescaled(d, hcols)) {
        set_error("predict_mean: the prescaled form needs hcols == 1 and d <= 64");
        return EGX_ERR_INVALID_VALUE;
    }
    if (prescaled) {
        const size_t lds_s = (size_t)(d * 64 + 256) * sizeof(double);
        EGX_DISPATCH_CORR(corr, hipLaunchKernelGGL((k_predict_mean_srow<C_>), grid, dim3(256), lds_s, s, pb.ptrs, xqT, ldq, pb.sq, ldx,
                                                   n_pad, d, racc, pb.sracc, per, m_pad));
        EGX_HIP_CHECK(hipGetLastError());
        return EGX_SUCCESS;
    }
    if (hcols == 1) {
        EGX_DISPATCH_CORR(corr, hipLaunchKernelGGL((k_predict_mean<C_, true>), grid, dim3(256), lds, s, pb.ptrs, xqT, ldq, pb.sq, ldx,
                                                   n_pad, d, hcols, racc, pb.sracc, per, m_pad));
    } else {
        EGX_DISPATCH_CORR(corr, hipLaunchKernelGGL((k_predict_mean<C_, false>), grid, dim3(256), lds, s, pb.ptrs, xqT, ldq, pb.sq, ldx,
                                                   n_pad, d, hcols, racc, pb.sracc, per, m_pad));
    }
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

// out: nsplit x m_pad x d partial sums per member; the weights are the members' gamma (vec != 0) or (n x m_pad) matrices
int launch_xgrad(hipStream_t s, int corr, const PosteriorBatch &pb, const double *xqT, int64_t ldq, int m_pad, int64_t ldx, int n,
                 int d, int hcols, const double *Wt, int64_t ldw, int vec, int nsplit, double *out, const int *cols, int ncols) {
    if (!posterior_count_ok(pb)) return EGX_ERR_INVALID_VALUE;
    const int slabs = (n + 63) / 64;
    if (nsplit < 1) nsplit = 1;
    if (nsplit > slabs) nsplit = slabs;
    const int per = (slabs + nsplit - 1) / nsplit;
    dim3 grid(m_pad / kXgThreads, nsplit, (unsigned)pb.count);
    // d <= 64: the lane's query coordinates in LDS; beyond: from global memory (XAG), the training slab alone in LDS,
    // as many training points wide (64, 32, ... 1) as fit beside the d x hcols coefficients
    const bool xag = d > kCorrDC;
    int js_shift = 6;
    auto lds_for = [&](int sh) { return (size_t)((xag ? 0 : d * kXgThreads) + ((size_t)d << sh) + (size_t)d * hcols) * sizeof(double); };
    while (js_shift > 0 && lds_for(js_shift) > kLdsBytes) js_shift--;
    const size_t lds = lds_for(js_shift);
    if (lds > kLdsBytes) {
        set_error("x-gradients: " + std::to_string(d) + " inputs x " + std::to_string(hcols) +
                  " coefficient columns do not fit the 160 KB of LDS (d * (hcols + 1) <= 20480)");
        return EGX_ERR_UNSUPPORTED;
    }
#define EGX_XG1(C_, DK_, VEC_, XAG_, LIST_)                                                                                  \
    {                                                                                                                        \
        if (lds > 65536)                                                                                                     \
            EGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_xgrad<C_, DK_, VEC_, XAG_, LIST_>),          \
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                        \
        hipLaunchKernelGGL((k_xgrad<C_, DK_, VEC_, XAG_, LIST_>), grid, dim3(kXgThreads), lds, s, pb.ptrs, xqT, ldq, pb.sq,  \
                           ldx, n, d, hcols, Wt, ldw, pb.sW, per, out, pb.sout, m_pad, js_shift, cols, ncols);              \
    }
#define EGX_XG(C_, DK_)                                    \
    if (xag) {                                             \
        if (vec) EGX_XG1(C_, 32, true, true, false)        \
        else EGX_XG1(C_, 32, false, true, false)           \
    } else if (vec) EGX_XG1(C_, DK_, true, false, false)   \
    else EGX_XG1(C_, DK_, false, false, false)
    // the column-list form (cols: ncols distinct device indices in [0, d)): the LIST instances, the pass width by the LIST's length
#define EGX_XGC(C_, DK_)                                   \
    if (xag) {                                             \
        if (vec) EGX_XG1(C_, DK_, true, true, true)        \
        else EGX_XG1(C_, DK_, false, true, true)           \
    } else if (vec) EGX_XG1(C_, DK_, true, false, true)    \
    else EGX_XG1(C_, DK_, false, false, true)
    if (cols) {
        if (ncols < 1 || ncols > d) {
            set_error("x-gradients: a column list of " + std::to_string(ncols) + " entries for " + std::to_string(d) + " inputs");
            return EGX_ERR_INVALID_VALUE;
        }
        if (ncols <= 8) {
            EGX_DISPATCH_CORR(corr, EGX_XGC(C_, 8));
        } else if (ncols <= 16) {
            EGX_DISPATCH_CORR(corr, EGX_XGC(C_, 16));
        } else {
            EGX_DISPATCH_CORR(corr, EGX_XGC(C_, 32));
        }
    } else if (d <= 8) {
        EGX_DISPATCH_CORR(corr, EGX_XG(C_, 8));
    } else if (d <= 16) {
        EGX_DISPATCH_CORR(corr, EGX_XG(C_, 16));
    } else {
        EGX_DISPATCH_CORR(corr, EGX_XG(C_, 32));
    }
#undef EGX_XG1
#undef EGX_XG
#undef EGX_XGC
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

// few queries (m <= 8), weights = a vector over the training points: out is (ceil(n / 256) x m x d) partial sums
int launch_xgrad_point(hipStream_t s, int corr, const double *xqT, int64_t ldq, int m, const double *xT, int64_t ldx, int n,
                       int d, const double *coef, int hcols, const double *wvec, double *out) {
    dim3 grid(m, (n + 255) / 256);
    const size_t lds = (size_t)(d + (size_t)d * hcols + 4 * (size_t)d) * sizeof(double);
    if (lds > kLdsBytes) {
        set_error("x-gradients: " + std::to_string(d) + " inputs x " + std::to_string(hcols) +
                  " coefficient columns do not fit the 160 KB of LDS (d * (hcols + 5) <= 20480)");
        return EGX_ERR_UNSUPPORTED;
    }
#define EGX_XGP(C_)                                                                                                          \
    {                                                                                                                        \
        if (lds > 65536)                                                                                                     \
            EGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_xgrad_point<C_>),                            \
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                        \
        hipLaunchKernelGGL(k_xgrad_point<C_>, grid, dim3(256), lds, s, xqT, ldq, xT, ldx, n, d, coef, hcols, wvec, out, m);  \
    }
    EGX_DISPATCH_CORR(corr, EGX_XGP(C_));
#undef EGX_XGP
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

// y (n_pad) <- W^T r, z (n_pad) <- W y for the upper-triangular W (n_pad x n_pad, ld); P: scratch of 32 * n_pad doubles
int launch_uptri_solve_pair(hipStream_t s, const double *W, int64_t ld, int n, int n_pad, const double *r, double *P,
                            double *y, double *z) {
    int nsplit = (n + 255) / 256;
    if (nsplit > 32) nsplit = 32;
    const int per = (int)round_up((n + nsplit - 1) / nsplit, 4);
    nsplit = (n + per - 1) / per;
    hipLaunchKernelGGL(k_uptri_gemv_t, dim3(n_pad / 64, nsplit), dim3(256), 0, s, W, ld, n, r, per, P, n_pad);
    hipLaunchKernelGGL(k_sum_partials, dim3((n_pad + 255) / 256), dim3(256), 0, s, (const double *)P, nsplit, n_pad, y);
    hipLaunchKernelGGL(k_uptri_gemv, dim3((n + 3) / 4), dim3(256), 0, s, W, ld, n, (const double *)y, (const double *)nullptr, 1.0, z,
                       (int64_t)0);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_fill_rows(hipStream_t s, double *M, int64_t ld, int r0, int rows_pad, const double *src, int64_t lds,
                     int nrows, int ncols) {
    hipLaunchKernelGGL(k_fill_rows, dim3(1024), dim3(256), 0, s, M, ld, r0, rows_pad, src, lds, nrows, ncols);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

// correlation matrices + right-hand-side rows of `count` candidates (scalar-row form only: hcols == 1, d <= 64; the caller
// falls back to launch_corr_sym / launch_fill_rows per candidate otherwise): returns EGX_ERR_UNSUPPORTED without launching
int launch_eval_front_batch(hipStream_t s, int corr, const EvalBatchPtrs &b, int count, int64_t ldx, int n, int d, int hcols,
                            double nugget, int64_t ld, int n_pad, int rhs_pad, int q) {
    if (hcols != 1 || d > kCorrDC || count < 1 || count > kLockstepMax) return EGX_ERR_UNSUPPORTED;
    const int nt2 = n_pad / 128;
    const dim3 grid((unsigned)(4 * (nt2 * (nt2 + 1) / 2)), (unsigned)count);
    const size_t lds = (size_t)d * 64 * sizeof(double);
    hipLaunchKernelGGL(k_scale_rows_batch, dim3((unsigned)((ldx + 255) / 256), (unsigned)count), dim3(256), 0, s, b, ldx, d);
    EGX_DISPATCH_CORR(corr, hipLaunchKernelGGL((k_corr_sym_srow_batch<C_>), grid, dim3(256), lds, s, b, ldx, n, d, 1.0 + nugget, ld));
    hipLaunchKernelGGL(k_fill_rows_batch, dim3(256, (unsigned)count), dim3(256), 0, s, b, ld, n_pad, rhs_pad, ldx, q, n_pad);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_scale_rows_batch(hipStream_t s, const EvalBatchPtrs &b, int count, int64_t ldx, int d) {
    if (count < 1 || count > kLockstepMax) {
        set_error("scale_rows_batch: batch count out of range");
        return EGX_ERR_INVALID_VALUE;
    }
    hipLaunchKernelGGL(k_scale_rows_batch, dim3((unsigned)((ldx + 255) / 256), (unsigned)count), dim3(256), 0, s, b, ldx, d);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_eval_tail(hipStream_t s, const EvalBatchPtrs &b, int count, int64_t ld, int n, int n_pad, int q, int rows, const int *sync) {
    hipLaunchKernelGGL(k_eval_tail, dim3((unsigned)((n_pad + 255) / 256), (unsigned)(rows ? 1 + q : 1), (unsigned)count), dim3(256), 0, s, b,
                       ld, n, n_pad, rows, sync);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_gather_diag(hipStream_t s, const double *M, int64_t ld, int n, double *out) {
    hipLaunchKernelGGL(k_gather_diag, dim3((n + 255) / 256), dim3(256), 0, s, M, ld, n, out);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_gram_finish(hipStream_t s, const double *Gneg, double *G, int64_t ldg, int rows, int q) {
    hipLaunchKernelGGL(k_gram_finish, dim3((rows + 255) / 256, rows), dim3(256), 0, s, Gneg, G, ldg, rows, q);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_gls_residual(hipStream_t s, const double *ftT, int64_t ld, const double *yt, const double *beta, int p, int n,
                        int n_pad, double *rho, double *part) {
    hipLaunchKernelGGL(k_gls_residual, dim3((n_pad + 255) / 256), dim3(256), 0, s, ftT, ld, yt, beta, p, n, n_pad, rho,
                       part);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_zero_upper(hipStream_t s, double *M, int64_t ld, int n) {
    hipLaunchKernelGGL(k_zero_upper, dim3(2048), dim3(256), 0, s, M, ld, n);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_row_reduce(hipStream_t s, const PosteriorBatch &pb, const double *RT, int64_t ld, int m, int n, int64_t ldf, int p,
                      double *s0, double *sl) {
    if (!posterior_count_ok(pb)) return EGX_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(k_row_reduce, dim3((m + 3) / 4, (unsigned)pb.count), dim3(256), 0, s, pb.ptrs, RT, ld, pb.sR, m, n, ldf, p, s0,
                       pb.ss0, sl, pb.ssl);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int grad_partial_doubles(int nout) { return kGradMaxWG * (int)round_up(nout, 32); }

// batch.count candidates (grid.z); per candidate: coef (d x hcols), gamma (n_pad), rneg (-R^-1, lower, ld), inv_s2,
// part (grad_partial_doubles(nout) doubles of scratch), out (nout doubles)
// prescaled != 0 (hcols == 1, every coefficient > 0): batch.xs[z] holds candidate z's inputs times its coefficients;
// otherwise batch.xT[z] the (d x ldx) inputs of its owner
int launch_grad_accum(hipStream_t s, int corr, int64_t ldx, int n, int d, int hcols, const double *wabs, int nout, int64_t ld,
                      const GradBatch &batch, int prescaled) {
    if (batch.count < 1 || batch.count > kLockstepMax) {
        set_error("grad_accum: batch count out of range");
        return EGX_ERR_INVALID_VALUE;
    }
    const int nt = (n + 63) / 64, ntiles = nt * (nt + 1) / 2;
    const int nwg = ntiles < kGradMaxWG ? ntiles : kGradMaxWG;
    const int nout_pad = (int)round_up(nout, 32);
    const int dc = d < kGradDC ? d : kGradDC;
    const int dk = nout <= 8 ? 8 : (nout <= 16 ? 16 : 32);
    const size_t lds = sizeof(double) * (size_t)std::max(2 * dc * 64, 4 * dk);
    const dim3 grid((unsigned)nwg, (unsigned)((nout + dk - 1) / dk), (unsigned)batch.count);
#define EGX_GA(C_, MODE_, DK_)                                                                                             \
    hipLaunchKernelGGL((k_grad_accum<C_, MODE_, DK_>), grid, dim3(256), lds, s, ldx, n, d, hcols, wabs, nout, ld, ntiles, \
                       nout_pad, batch)
#define EGX_GA_DK(C_, MODE_)                  \
    if (dk == 8) EGX_GA(C_, MODE_, 8);        \
    else if (dk == 16) EGX_GA(C_, MODE_, 16); \
    else EGX_GA(C_, MODE_, 32)
    if (hcols == 1 && prescaled) {
        EGX_DISPATCH_CORR(corr, EGX_GA_DK(C_, 2));
    } else if (hcols == 1) {
        EGX_DISPATCH_CORR(corr, EGX_GA_DK(C_, 1));
    } else {
        EGX_DISPATCH_CORR(corr, EGX_GA_DK(C_, 0));
    }
#undef EGX_GA_DK
#undef EGX_GA
    hipLaunchKernelGGL(k_grad_reduce, dim3((unsigned)nout, (unsigned)batch.count), dim3(256), 0, s, nwg, nout, nout_pad, batch);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

// z (n) <- W y for the upper triangular W (row-major): gamma = C^-T rho through the explicit C^-T of the theta-gradient
int launch_uptri_gemv(hipStream_t s, const double *W, int64_t ld, int n, const double *y, double *z) {
    return launch_uptri_gemv_rows(s, W, ld, n, y, nullptr, 1.0, z, 0, 1);
}

int launch_uptri_gemv_batch(hipStream_t s, const double *W, int64_t sW, int64_t ld, int n, const GemvBatchPtrs &b, int count) {
    if (count < 1 || count > kLockstepMax) {
        set_error("uptri_gemv_batch: batch count out of range");
        return EGX_ERR_INVALID_VALUE;
    }
    hipLaunchKernelGGL(k_uptri_gemv_batch, dim3((n + 3) / 4, (unsigned)count), dim3(256), 0, s, W, sW, ld, n, b);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_uptri_gemv_rows(hipStream_t s, const double *W, int64_t ld, int n, const double *Y, const double *base, double sc,
                           double *Z, int64_t ldr, int rows) {
    hipLaunchKernelGGL(k_uptri_gemv, dim3((n + 3) / 4, (unsigned)rows), dim3(256), 0, s, W, ld, n, Y, base, sc, Z, ldr);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

// Posterior covariance of m query points (GaussianProcess::_compute_covariance, algorithm.rs:310-326), one 64 x 64 tile of
// the lower triangle per workgroup: S[i][j] = S[j][i] = sigma2 (k(x_i, x_j) + G[i][j]) + tau [i == j] for i >= j, both < m,
// with k the handle's correlation WITHOUT nugget (k(x, x) = 1) and G = -rt^T rt + u^T u (nullptr: no such term; the Gram kernels' lower tiles, read
// at i >= j only: the result is exactly symmetric); rows and columns m .. m_pad - 1 become those of the identity, so that
// launch_potrf factors S as it stands.  Each unordered pair is evaluated once and stored twice.
template <int CORR, bool PRE>
__global__ __launch_bounds__(256) void k_cov_assemble(const double *__restrict__ xqT, int64_t ldq, int d,
                                                      const double *__restrict__ coef, int hcols, const double *__restrict__ G,
                                                      int64_t ldg, int m, double sigma2, double tau, double *__restrict__ S,
                                                      int64_t lds) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    int bx, by;
    tri_tile(blockIdx.x, bx, by);
    const int dc = d < kCorrDC ? d : kCorrDC;
    double *xi = sm, *xj = sm + dc * 64;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    PairAcc<CORR> acc[4][4];
    tile_pairs_staged<CORR, PRE>(xi, xj, {xqT, ldq, bx * 64}, {xqT, ldq, by * 64}, d, dc, coef, hcols, tid, ty, tx, false, acc,
                                 PRE ? coef : nullptr);
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int i = bx * 64 + ty * 4 + a, j = by * 64 + tx * 4 + b;
            if (j > i) continue;  // (diagonal tiles) the pair comes as (j, i)
            double v;
            if (i < m) {
                v = sigma2 * (acc[a][b].value() + (G ? G[(int64_t)i * ldg + j] : 0.0));
                if (i == j) v += tau;
            } else {
                v = (i == j) ? 1.0 : 0.0;
            }
            S[(int64_t)i * lds + j] = v;
            S[(int64_t)j * lds + i] = v;
        }
}

int launch_cov_assemble(hipStream_t s, int corr, const double *xqT, int64_t ldq, int m_pad, int d, const double *coef, int hcols,
                        const double *G, int64_t ldg, int m, double sigma2, double tau, double *S, int64_t lds) {
    if (m_pad % 64 || m > m_pad) {
        set_error("cov_assemble: m_pad must be a multiple of 64 and >= m");
        return EGX_ERR_INVALID_VALUE;
    }
    const int nb = m_pad / 64;
    const dim3 grid((unsigned)(nb * (nb + 1) / 2));
    const size_t lds_bytes = (size_t)2 * (d < kCorrDC ? d : kCorrDC) * 64 * sizeof(double);
    if (hcols == 1) {
        EGX_DISPATCH_CORR(corr, hipLaunchKernelGGL((k_cov_assemble<C_, true>), grid, dim3(256), lds_bytes, s, xqT, ldq, d, coef,
                                                   hcols, G, ldg, m, sigma2, tau, S, lds));
    } else {
        EGX_DISPATCH_CORR(corr, hipLaunchKernelGGL((k_cov_assemble<C_, false>), grid, dim3(256), lds_bytes, s, xqT, ldq, d, coef,
                                                   hcols, G, ldg, m, sigma2, tau, S, lds));
    }
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

}  // namespace egx
