// EM of a full-covariance Gaussian mixture on rows up to 128 wide, R restarts in lock-step (egx_gmm_fit_wide, gmm_host.hip;
// DESIGN.md 4.8 "Wide rows").  The algorithm is that of kernels_gmm.hip -- FP64, one-hot start on the nearest mean, moments
// about the current mean, no floating-point atomics, every sum in a fixed order, a frozen restart skipped on entry -- with
// the two O(D^2) products per row on v_mfma_f64_16x16x4_f64 (lane l: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15],
// C register q: row (l >> 4) + 4 q, column l & 15).  The shapes are those of gmm_wide_plan.h.
//
//   k_gmm_estep_wide<NT>  DP = 16 NT.  One workgroup of four waves per chunk of 64-row tiles (and per share of the restarts:
//                 grid.y).  A tile is staged ONCE in LDS and serves every live (restart, cluster):
//                 A  Z = (X - mu_c) P_c, wave w on the tile's rows 16 w .. 16 w + 15: for each 16-column tile of Z the K
//                    loop stops at the diagonal (P is upper triangular) and at D; ||z||^2 per row from the accumulators,
//                    the 16 lanes of a row added by a butterfly.  A = x - mu from LDS, B = P from global memory.
//                 B  log-sum-exp, responsibilities, the tile's sum of log-prob-norm (wave 0, one row per lane).
//                 C  S2_c += (r_c . Xc)^T Xc with the rows as K, lower triangle only, in 16 x 16 accumulator tiles dealt
//                    round-robin over the waves (tile t: wave t % 4); S1_c and sum r on the vector unit beside it.
//                 The chunk's first tile writes its slot of the workspace, the later ones add to it in tile order: the
//                 lane that owns an element is the same for every tile, so the slot is read and written by one lane only.
//   k_gmm_mstep_wide  one workgroup per (restart, cluster): the chunks' sums in chunk order, nk, weights, means, covariance,
//                 its Cholesky factor in LDS (D x (D + 1) doubles: 129 KiB at D = 128), L^-T by forward substitution on the
//                 identity INTO THE UPPER TRIANGLE of the same matrix (its diagonal beside it), the log-determinant, the
//                 failure flag, and by cluster 0's workgroup the lower bound.
//
// P in global memory: DP x DP row-major, upper triangular, zero beyond D -- row = the K index of Z = (X - mu) P, so a B
// fragment is four rows of 16 consecutive doubles.  Before iteration 0 the host stores the identity there: the first E-step
// measures ||x - mu||^2 through the same product.
#include "egx_internal.h"
#include "gmm_wide_plan.h"
#include "potf2_blocks.h"  // double4_t

namespace egx {

namespace {

namespace W = gmm_wide;

// (256, 2): two waves per SIMD, i.e. room for a second workgroup's MFMA-ready wave beside this one's
template <int NT>
__global__ __launch_bounds__(256, 2) void k_gmm_estep_wide(const double *__restrict__ data, int64_t n, int D, int k, int R,
                                                           int tpc, int init, const int *__restrict__ active,
                                                           const double *__restrict__ means, const double *__restrict__ prec,
                                                           const double *__restrict__ cst, double *__restrict__ part,
                                                           double *__restrict__ lpn_part) {
    constexpr int DP = W::kTile * NT, LDX = W::lds_stride(DP), TR = W::kTileRows;
    constexpr int NTRI = W::tri_tiles(DP), SLOTS = W::tiles_per_wave(DP);
    constexpr int TRI = (int)W::tri_len(DP), LEN = (int)W::part_len(DP);
    extern __shared__ double sm[];
    double *xs = sm;              // TR x LDX, zero beyond the tile's rows and beyond D
    double *lp = xs + TR * LDX;   // k x TR: log p, then the responsibilities
    double *mu = lp + k * TR;     // k x DP: the restart's means
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fi = lane & 15, fk = lane >> 4;
    const int64_t chunk = blockIdx.x;
    const int kd = (D + 3) / 4;  // K steps that reach a column below D

    int ti[SLOTS], tj[SLOTS];  // this wave's accumulator tiles of the lower triangle (ti < 0: none)
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int t = wave + W::kWaves * s;
        ti[s] = -1;
        tj[s] = 0;
        if (t < NTRI) W::tile_of(t, ti[s], tj[s]);
    }

    for (int tt = 0; tt < tpc; tt++) {  // gmm_wide_plan.h tile_rows(): the chunk's tiles, to the end of the data
        const int64_t row0 = (chunk * tpc + tt) * TR;
        if (row0 >= n) break;
        const int rows = (int)((n - row0 < TR) ? (n - row0) : TR);
        __syncthreads();
        for (int i = tid; i < TR * LDX; i += 256) xs[i] = 0.0;
        __syncthreads();
        for (int i = tid; i < rows * D; i += 256) xs[(i / D) * LDX + (i % D)] = data[row0 * D + i];

        for (int r = blockIdx.y; r < R; r += gridDim.y) {
            if (!active[r]) continue;
            __syncthreads();  // the tile is staged; the previous restart's readers of mu and lp are done
            for (int i = tid; i < k * DP; i += 256) mu[i] = means[(size_t)r * k * DP + i];
            __syncthreads();
            // ---- A: log p of the wave's 16 rows under every cluster
            const double *xrow = xs + (wave * 16 + fi) * LDX;
            for (int c = 0; c < k; c++) {
                const size_t rc = (size_t)r * k + c;
                const double *P = prec + rc * DP * DP + fi;
                const double *muc = mu + c * DP;
                double q[4] = {0.0, 0.0, 0.0, 0.0};
                for (int jt = 0; jt < NT; jt++) {
                    const int kend = 4 * (jt + 1) < kd ? 4 * (jt + 1) : kd;
                    double4_t acc = {0.0, 0.0, 0.0, 0.0};
                    for (int kk = 0; kk < kend; kk++) {
                        const int kx = 4 * kk + fk;
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xrow[kx] - muc[kx], P[kx * DP + 16 * jt], acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int e = 0; e < 4; e++) q[e] = fma(acc[e], acc[e], q[e]);
                }
#pragma unroll
                for (int e = 0; e < 4; e++) {
#pragma unroll
                    for (int off = 1; off < 16; off <<= 1) q[e] += __shfl_xor(q[e], off);
                    if (fi == 0) lp[c * TR + wave * 16 + fk + 4 * e] = init ? -q[e] : fma(-0.5, q[e], cst[rc]);
                }
            }
            __syncthreads();
            // ---- B: responsibilities (iteration 0: one-hot on the nearest mean, ties to the lowest index)
            if (tid < TR) {
                const bool valid = tid < rows;
                if (init) {
                    int best = 0;
                    double bv = lp[tid];
                    for (int c = 1; c < k; c++) {
                        const double v = lp[c * TR + tid];
                        if (v > bv) {
                            bv = v;
                            best = c;
                        }
                    }
                    for (int c = 0; c < k; c++) lp[c * TR + tid] = (valid && c == best) ? 1.0 : 0.0;
                } else {
                    double m = lp[tid];
                    for (int c = 1; c < k; c++) m = fmax(m, lp[c * TR + tid]);
                    double s = 0.0;
                    for (int c = 0; c < k; c++) s += exp(lp[c * TR + tid] - m);
                    double lse = m + log(s);
                    for (int c = 0; c < k; c++) lp[c * TR + tid] = valid ? exp(lp[c * TR + tid] - lse) : 0.0;
                    if (!valid) lse = 0.0;
                    for (int off = 32; off > 0; off >>= 1) lse += __shfl_down(lse, off);
                    if (tid == 0) {
                        double *o = lpn_part + chunk * R + r;
                        *o = tt == 0 ? lse : *o + lse;
                    }
                }
            }
            __syncthreads();
            // ---- C: moments about the cluster's current mean
            for (int c = 0; c < k; c++) {
                const double *muc = mu + c * DP, *w = lp + c * TR;
                double *out = part + ((size_t)(chunk * R + r) * k + c) * LEN;
                double4_t acc[SLOTS];
#pragma unroll
                for (int s = 0; s < SLOTS; s++) acc[s] = double4_t{0.0, 0.0, 0.0, 0.0};
                const double *mul = muc + fi;
#pragma unroll 1
                for (int kk = 0; kk < TR / 4; kk++) {
                    const int row = 4 * kk + fk;
                    const double wr = w[row];
                    const double *xr = xs + row * LDX + fi;
#pragma unroll
                    for (int s = 0; s < SLOTS; s++)
                        if (ti[s] >= 0)
                            acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(wr * (xr[16 * ti[s]] - mul[16 * ti[s]]),
                                                                          xr[16 * tj[s]] - mul[16 * tj[s]], acc[s], 0, 0, 0);
                }
                double *ot = out + wave * 256 + fk * 16 + fi;  // tile t = wave + 4 s whole, row-major
#pragma unroll
                for (int s = 0; s < SLOTS; s++)
                    if (ti[s] >= 0) {
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            double *o = ot + s * (W::kWaves * 256) + e * 64;
                            *o = tt == 0 ? acc[s][e] : *o + acc[s][e];
                        }
                    }
                if (tid < DP) {
                    double s1 = 0.0;
#pragma unroll 4
                    for (int row = 0; row < TR; row++) s1 += w[row] * (xs[row * LDX + tid] - muc[tid]);
                    double *o = out + TRI + tid;
                    *o = tt == 0 ? s1 : *o + s1;
                } else if (tid == 255) {
                    double s0 = 0.0;
#pragma unroll 4
                    for (int row = 0; row < TR; row++) s0 += w[row];
                    double *o = out + TRI + DP;
                    *o = tt == 0 ? s0 : *o + s0;
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_gmm_mstep_wide(int64_t n, int D, int DP, int k, int R, int T, int init, double reg,
                                                        const int *__restrict__ active, const double *__restrict__ part,
                                                        const double *__restrict__ lpn_part, double *__restrict__ means,
                                                        double *__restrict__ prec, double *__restrict__ cst,
                                                        double *__restrict__ weights, double *__restrict__ covs,
                                                        double *__restrict__ lbst) {
    const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    if (!active[r]) return;
    extern __shared__ double sm[];
    const int LDA = D + 1;
    double *s_A = sm;                 // D x LDA: the covariance, then L below and L^-T above the diagonal
    double *s_dinv = s_A + D * LDA;   // D: 1 / diag L
    double *s_delta = s_dinv + D;     // D
    double *s_nk = s_delta + D;       // 16
    double *s_red = s_nk + 16;        // 256
    __shared__ int s_fail;
    const size_t TRI = W::tri_len(DP), LEN = W::part_len(DP);
    const auto s2_at = [](int i, int j) { return (size_t)W::tile_index(i / 16, j / 16) * 256 + (i % 16) * 16 + j % 16; };
    const size_t rc = (size_t)r * k + c;
    if (tid == 0) s_fail = 0;
    // the chunks' partial sums, in chunk order
    if (tid < k) {
        double s = 0.0;
#pragma unroll 8
        for (int t = 0; t < T; t++) s += part[((size_t)((size_t)t * R + r) * k + tid) * LEN + TRI + DP];
        s_nk[tid] = s + 10.0 * 2.220446049250313e-16;
    }
    double s1 = 0.0;
    if (tid < D)
#pragma unroll 8
        for (int t = 0; t < T; t++) s1 += part[((size_t)((size_t)t * R + r) * k + c) * LEN + TRI + tid];
    if (c == 0 && !init) {  // the lower bound: mean log-prob-norm under the parameters this iteration started from
        double s = 0.0;
        for (int t = tid; t < T; t += 256) s += lpn_part[(size_t)t * R + r];
        s_red[tid] = s;
        for (int off = 128; off > 0; off >>= 1) {
            __syncthreads();
            if (tid < off) s_red[tid] += s_red[tid + off];
        }
        if (tid == 0) lbst[r] = s_red[0] / (double)n;
    }
    __syncthreads();
    const double nk = s_nk[c];
    if (tid < D) s_delta[tid] = s1 / nk;
    __syncthreads();
    bool bad = false;
    for (int e = tid; e < D * D; e += 256) {
        const int i = e / D, j = e % D;
        if (j > i) continue;
        double s = 0.0;
#pragma unroll 8
        for (int t = 0; t < T; t++) s += part[((size_t)((size_t)t * R + r) * k + c) * LEN + s2_at(i, j)];
        double v = s / nk - s_delta[i] * s_delta[j];
        if (i == j) v += reg;
        s_A[i * LDA + j] = v;
        covs[rc * D * D + (size_t)i * D + j] = v;
        covs[rc * D * D + (size_t)j * D + i] = v;
        bad |= !isfinite(v);
    }
    if (tid < D) {
        const double m = means[rc * DP + tid] + s_delta[tid];
        means[rc * DP + tid] = m;
        bad |= !isfinite(m);
    }
    double wsum = 0.0;
    for (int cc = 0; cc < k; cc++) wsum += s_nk[cc];
    const double w = nk / wsum;
    if (bad) s_fail = 1;
    // right-looking Cholesky of the D x D covariance, in place (lower)
    for (int j = 0; j < D; j++) {
        __syncthreads();
        const double d = s_A[j * LDA + j];
        const bool ok = d > 0.0 && isfinite(d);
        const double ljj = ok ? sqrt(d) : 1.0;
        __syncthreads();
        if (tid == 0) {
            s_A[j * LDA + j] = ljj;
            if (!ok) s_fail = 1;
        }
        for (int i = j + 1 + tid; i < D; i += 256) s_A[i * LDA + j] /= ljj;
        __syncthreads();
        const int m = D - j - 1;
        for (int e = tid; e < m * m; e += 256) {
            const int i = j + 1 + e / m, l = j + 1 + e % m;
            if (l <= i) s_A[i * LDA + l] -= s_A[i * LDA + j] * s_A[l * LDA + j];
        }
    }
    __syncthreads();
    // L^-1 by forward substitution on the identity, one column per lane: column `col` of L^-1 is row `col` of P = L^-T and
    // goes above the diagonal of row `col` of s_A, which nothing reads any more; the diagonal goes to s_dinv
    if (tid < D) {
        const int col = tid;
        double dcol = 0.0;
        for (int i = col; i < D; i++) {
            double v = (i == col) ? 1.0 : 0.0;
            for (int l = col; l < i; l++) v -= s_A[i * LDA + l] * (l == col ? dcol : s_A[col * LDA + l]);
            v /= s_A[i * LDA + i];
            if (i == col) {
                dcol = v;
                s_dinv[col] = v;
            } else {
                s_A[col * LDA + i] = v;
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < DP * DP; e += 256) {  // P = L^-T, upper triangular, zero padded to DP
        const int i = e / DP, j = e % DP;
        prec[rc * DP * DP + e] = (j >= D || i > j) ? 0.0 : (i == j ? s_dinv[i] : s_A[i * LDA + j]);
    }
    if (tid == 0) {
        double ld = 0.0;
        for (int i = 0; i < D; i++) ld += log(s_dinv[i]);
        const double cv = (-0.5 * (double)D * 1.8378770664093453 + ld) + log(w);
        cst[rc] = cv;
        weights[rc] = w;
        if (s_fail || !isfinite(cv)) lbst[R + r] = 1.0;
    }
}

template <int NT>
int launch_estep_nt(hipStream_t s, const GmmLaunch &g) {
    const size_t lds = W::estep_lds_bytes(W::kTile * NT, g.k);
    if (lds > 64 * 1024)
        EGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_gmm_estep_wide<NT>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_gmm_estep_wide<NT>, dim3((unsigned)g.T, (unsigned)g.rsplit), dim3(256), lds, s, g.data, g.n, g.D, g.k,
                       g.R, g.tpc, g.init, g.active, g.means, g.prec, g.cst, g.part, g.lpn_part);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

}  // namespace

int launch_gmm_estep_wide(hipStream_t s, const GmmLaunch &g) {
    const bool fits = g.DP == W::dp_of(g.D) && g.k <= kGmmMaxClusters && W::estep_lds_bytes(g.DP, g.k) <= W::kLdsLimit;
    switch (fits ? g.DP / W::kTile : 0) {
        case 1: return launch_estep_nt<1>(s, g);
        case 2: return launch_estep_nt<2>(s, g);
        case 3: return launch_estep_nt<3>(s, g);
        case 4: return launch_estep_nt<4>(s, g);
        case 5: return launch_estep_nt<5>(s, g);
        case 6: return launch_estep_nt<6>(s, g);
        case 7: return launch_estep_nt<7>(s, g);
        case 8: return launch_estep_nt<8>(s, g);
    }
    set_error("egx_gmm_fit_wide: dim beyond the kernel's limit");
    return EGX_ERR_INVALID_VALUE;
}

int launch_gmm_mstep_wide(hipStream_t s, const GmmLaunch &g, double reg_covar) {
    const size_t lds = W::mstep_lds_bytes(g.D);
    if (g.D > W::kMaxDim || g.k > kGmmMaxClusters || lds > W::kLdsLimit) {
        set_error("egx_gmm_fit_wide: dim beyond the kernel's limit");
        return EGX_ERR_INVALID_VALUE;
    }
    if (lds > 64 * 1024)
        EGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_gmm_mstep_wide),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_gmm_mstep_wide, dim3((unsigned)g.k, (unsigned)g.R), dim3(256), lds, s, g.n, g.D, g.DP, g.k, g.R, g.T,
                       g.init, reg_covar, g.active, g.part, g.lpn_part, g.means, g.prec, g.cst, g.weights, g.covs, g.lbst);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

}  // namespace egx
