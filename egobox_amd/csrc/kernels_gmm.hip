// EM of a full-covariance Gaussian mixture for R restarts in lock-step (egx_gmm_fit, gmm_host.hip).
//
//   k_gmm_estep   one workgroup per tile of 256 rows: the tile is read ONCE into LDS and serves every (restart, cluster)
//                 parameter set.  Phase A, one row per lane: z = (x - mu) P through the scalar unit (mu, P are uniform),
//                 log p per cluster into LDS.  Phase B: log-sum-exp, responsibilities, the tile's sum of log-prob-norm.
//                 Phase C, per cluster: the moments about mu -- sum r, sum r (x - mu), sum r (x - mu)(x - mu)^T -- as 4 x 4
//                 register blocks of the lower triangle, one block (and one subset of the wave's rows) per lane, the lanes'
//                 partial sums added in a fixed order and written to the workspace: part[tile][restart][cluster][..].
//   k_gmm_mstep   one workgroup per (restart, cluster): the tiles' partial sums in tile order, nk, weights, means,
//                 covariance = S2 / nk - delta delta^T + reg I (delta = new mean - old mean), its Cholesky factor in LDS,
//                 P = L^-T, the log-determinant, and the restart's failure flag.
//
// No floating-point atomics: a restart's numbers depend on n, D, k and its own start only -- not on R, not on its place in
// the batch, not on the run.  A frozen restart (active[r] == 0) is skipped on entry by both kernels.
//
// ... and the fitted mixture's predict side: k_gmx_probas / k_gmx_probas_deriv, the responsibilities and their x-derivatives
// at m points (egx_gmx_predict_probas(_derivatives), gmm_host.hip), one lane per point with the point text of gmx_point.h.
#include "egx_internal.h"
#include "gmx_point.h"

namespace egx {

namespace {

constexpr int kRows = kGmmTileRows;  // rows of a tile = lanes of the workgroup
constexpr int kAcc = kGmmBlockAcc;   // per 4 x 4 block: 16 second moments, 4 first moments, the sum of responsibilities

__device__ inline void block_of(int b, int &bi, int &bj) {  // b = bi (bi + 1) / 2 + bj, bj <= bi
    bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= b) bi++;
    bj = b - bi * (bi + 1) / 2;
}

// ||(x - mu) P||^2 with P upper triangular (DP x DP row-major), or ||x - mu||^2 (iteration 0)
template <int DP>
__device__ inline double maha(const double *xrow, const double *__restrict__ mu, const double *__restrict__ P, int init) {
    double diff[DP];
#pragma unroll
    for (int i = 0; i < DP; i++) diff[i] = xrow[i] - mu[i];
    double q = 0.0;
    if (init) {
#pragma unroll
        for (int i = 0; i < DP; i++) q = fma(diff[i], diff[i], q);
        return q;
    }
#pragma unroll
    for (int j = 0; j < DP; j++) {
        double z = 0.0;
#pragma unroll
        for (int i = 0; i <= j; i++) z = fma(diff[i], P[i * DP + j], z);
        q = fma(z, z, q);
    }
    return q;
}

template <int DP>
__global__ __launch_bounds__(256) void k_gmm_estep(const double *__restrict__ data, int64_t n, int D, int k, int R, int init,
                                                   const int *__restrict__ active, const double *__restrict__ means,
                                                   const double *__restrict__ prec, const double *__restrict__ cst,
                                                   double *__restrict__ part, double *__restrict__ lpn_part) {
    constexpr int LDX = DP + 1;  // odd: a row per lane walks the banks
    constexpr int NB = DP / 4, NBLK = NB * (NB + 1) / 2, NSPLIT = 64 / NBLK, LEN = NBLK * kAcc;
    extern __shared__ double sm[];
    double *xs = sm;                    // kRows x LDX, zero beyond the tile's rows and beyond D
    double *lp = xs + kRows * LDX;      // k x kRows: log p, then the responsibilities
    double *scr = lp + k * kRows;       // kRows x kAcc: the lanes' partial moments
    double *red = scr + kRows * kAcc;   // 4: the waves' sums of log-prob-norm
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t tile = blockIdx.x, row0 = tile * kRows;
    const int rows = (int)((n - row0 < kRows) ? (n - row0) : kRows);

    for (int i = tid; i < kRows * LDX; i += kRows) xs[i] = 0.0;
    __syncthreads();
    for (int i = tid; i < rows * D; i += kRows) xs[(i / D) * LDX + (i % D)] = data[row0 * D + i];
    __syncthreads();

    const int b = lane % NBLK, sp = lane / NBLK;
    int bi, bj;
    block_of(b, bi, bj);
    const bool valid = tid < rows;

    for (int r = blockIdx.y; r < R; r += gridDim.y) {
        if (!active[r]) continue;
        // ---- A: log p of this lane's row under every cluster
        for (int c = 0; c < k; c++) {
            const size_t rc = (size_t)r * k + c;
            const double q = maha<DP>(xs + tid * LDX, means + rc * DP, prec + rc * DP * DP, init);
            lp[c * kRows + tid] = init ? -q : fma(-0.5, q, cst[rc]);
        }
        // ---- B: responsibilities (iteration 0: one-hot on the nearest mean, ties to the lowest index)
        double lse = 0.0;
        if (init) {
            int best = 0;
            double bv = lp[tid];
            for (int c = 1; c < k; c++) {
                const double v = lp[c * kRows + tid];
                if (v > bv) {
                    bv = v;
                    best = c;
                }
            }
            for (int c = 0; c < k; c++) lp[c * kRows + tid] = (valid && c == best) ? 1.0 : 0.0;
        } else {
            double m = lp[tid];
            for (int c = 1; c < k; c++) m = fmax(m, lp[c * kRows + tid]);
            double s = 0.0;
            for (int c = 0; c < k; c++) s += exp(lp[c * kRows + tid] - m);
            lse = m + log(s);
            for (int c = 0; c < k; c++) lp[c * kRows + tid] = valid ? exp(lp[c * kRows + tid] - lse) : 0.0;
            if (!valid) lse = 0.0;
            for (int off = 32; off > 0; off >>= 1) lse += __shfl_down(lse, off);
            if (lane == 0) red[wave] = lse;
        }
        __syncthreads();
        if (!init && tid == 0) lpn_part[tile * R + r] = ((red[0] + red[1]) + red[2]) + red[3];
        // ---- C: moments about the cluster's current mean
        for (int c = 0; c < k; c++) {
            const size_t rc = (size_t)r * k + c;
            double acc[kAcc];
#pragma unroll
            for (int e = 0; e < kAcc; e++) acc[e] = 0.0;
            if (sp < NSPLIT) {
                double mua[4], mub[4];
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    mua[p] = means[rc * DP + 4 * bi + p];
                    mub[p] = means[rc * DP + 4 * bj + p];
                }
                for (int rr = sp; rr < 64; rr += NSPLIT) {
                    const int row = wave * 64 + rr;
                    const double w = lp[c * kRows + row];
                    const double *xr = xs + row * LDX;
                    double wa[4], bq[4];
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        wa[p] = w * (xr[4 * bi + p] - mua[p]);
                        bq[p] = xr[4 * bj + p] - mub[p];
                    }
#pragma unroll
                    for (int p = 0; p < 4; p++) {
#pragma unroll
                        for (int q = 0; q < 4; q++) acc[p * 4 + q] = fma(wa[p], bq[q], acc[p * 4 + q]);
                        acc[16 + p] += wa[p];
                    }
                    acc[20] += w;
                }
            }
#pragma unroll
            for (int e = 0; e < kAcc; e++) scr[tid * kAcc + e] = acc[e];
            __syncthreads();
            double *out = part + ((size_t)(tile * R + r) * k + c) * LEN;
            for (int item = tid; item < LEN; item += kRows) {
                const int b2 = item / kAcc, e = item % kAcc;
                double s = 0.0;
                for (int wv = 0; wv < 4; wv++)
                    for (int s2 = 0; s2 < NSPLIT; s2++) s += scr[(wv * 64 + s2 * NBLK + b2) * kAcc + e];
                out[item] = s;
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void k_gmm_mstep(int64_t n, int D, int DP, int k, int R, int T, int init, double reg,
                                                   const int *__restrict__ active, const double *__restrict__ part,
                                                   const double *__restrict__ lpn_part, double *__restrict__ means,
                                                   double *__restrict__ prec, double *__restrict__ cst,
                                                   double *__restrict__ weights, double *__restrict__ covs,
                                                   double *__restrict__ lbst) {
    const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    if (!active[r]) return;
    constexpr int LDA = kGmmMaxDim + 1;
    __shared__ double s_stat[kGmmMaxBlocks * kAcc], s_nk[kGmmMaxClusters], s_A[kGmmMaxDim * LDA], s_Li[kGmmMaxDim * LDA],
        s_delta[kGmmMaxDim], s_red[256];
    __shared__ int s_fail;
    const int NB = DP / 4, LEN = NB * (NB + 1) / 2 * kAcc;
    if (tid == 0) s_fail = 0;
    // the tiles' partial sums, in tile order
    if (tid < k) {
        double s = 0.0;
        for (int t = 0; t < T; t++) s += part[((size_t)((size_t)t * R + r) * k + tid) * LEN + 20];
        s_nk[tid] = s + 10.0 * 2.220446049250313e-16;
    }
    for (int item = tid; item < LEN; item += 256) {
        double s = 0.0;
        for (int t = 0; t < T; t++) s += part[((size_t)((size_t)t * R + r) * k + c) * LEN + item];
        s_stat[item] = s;
    }
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
    const size_t rc = (size_t)r * k + c;
    if (tid < D) {
        const int bi = tid / 4;
        const double delta = s_stat[(bi * (bi + 1) / 2) * kAcc + 16 + tid % 4] / nk;
        s_delta[tid] = delta;
    }
    __syncthreads();
    bool bad = false;
    for (int e = tid; e < D * D; e += 256) {
        const int i = e / D, j = e % D;
        const int hi = i > j ? i : j, lo = i > j ? j : i;
        const int bi = hi / 4, bj = lo / 4;
        double v = s_stat[(bi * (bi + 1) / 2 + bj) * kAcc + (hi % 4) * 4 + lo % 4] / nk - s_delta[hi] * s_delta[lo];
        if (i == j) v += reg;
        s_A[i * LDA + j] = v;
        covs[rc * D * D + e] = v;
        bad |= !isfinite(v);
    }
    if (tid < D) {
        const double mu = means[rc * DP + tid] + s_delta[tid];
        means[rc * DP + tid] = mu;
        bad |= !isfinite(mu);
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
    // L^-1 by forward substitution on the identity, one column per lane
    if (tid < D) {
        const int col = tid;
        for (int i = col; i < D; i++) {
            double v = (i == col) ? 1.0 : 0.0;
            for (int l = col; l < i; l++) v -= s_A[i * LDA + l] * s_Li[l * LDA + col];
            s_Li[i * LDA + col] = v / s_A[i * LDA + i];
        }
    }
    __syncthreads();
    for (int e = tid; e < DP * DP; e += 256) {  // P = L^-T, upper triangular, zero padded to DP
        const int i = e / DP, j = e % DP;
        prec[rc * DP * DP + e] = (i <= j && j < D) ? s_Li[j * LDA + i] : 0.0;
    }
    if (tid == 0) {
        double ld = 0.0;
        for (int i = 0; i < D; i++) ld += log(s_Li[i * LDA + i]);
        const double cv = (-0.5 * (double)D * 1.8378770664093453 + ld) + log(w);
        cst[rc] = cv;
        weights[rc] = w;
        if (s_fail || !isfinite(cv)) lbst[R + r] = 1.0;
    }
}

}  // namespace

size_t gmm_estep_lds_bytes(int DP, int k) {
    return sizeof(double) * ((size_t)kRows * (DP + 1) + (size_t)k * kRows + (size_t)kRows * kAcc + 4);
}

template <int DP>
static int launch_estep_dp(hipStream_t s, const GmmLaunch &g) {
    const size_t lds = gmm_estep_lds_bytes(DP, g.k);
    if (lds > 64 * 1024)
        EGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_gmm_estep<DP>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_gmm_estep<DP>, dim3((unsigned)g.T, (unsigned)g.rsplit), dim3(256), lds, s, g.data, g.n, g.D, g.k, g.R,
                       g.init, g.active, g.means, g.prec, g.cst, g.part, g.lpn_part);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_gmm_estep(hipStream_t s, const GmmLaunch &g) {
    switch (g.DP) {
        case 4: return launch_estep_dp<4>(s, g);
        case 8: return launch_estep_dp<8>(s, g);
        case 12: return launch_estep_dp<12>(s, g);
        case 16: return launch_estep_dp<16>(s, g);
        case 20: return launch_estep_dp<20>(s, g);
        case 24: return launch_estep_dp<24>(s, g);
        case 28: return launch_estep_dp<28>(s, g);
        case 32: return launch_estep_dp<32>(s, g);
        case 36: return launch_estep_dp<36>(s, g);
    }
    set_error("egx_gmm_fit: dim beyond the kernel's limit");
    return EGX_ERR_INVALID_VALUE;
}

int launch_gmm_mstep(hipStream_t s, const GmmLaunch &g, double reg_covar) {
    hipLaunchKernelGGL(k_gmm_mstep, dim3((unsigned)g.k, (unsigned)g.R), dim3(256), 0, s, g.n, g.D, g.DP, g.k, g.R, g.T, g.init,
                       reg_covar, g.active, g.part, g.lpn_part, g.means, g.prec, g.cst, g.weights, g.covs, g.lbst);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

// Responsibilities of a Gaussian mixture at m points (gmx_probas_point): one lane per point, the workgroup's 64 points staged
// in LDS (row stride d | 1: a lane walks its own row), means, scaled factors and par read as wave-uniform operands.
// TYPED (the two _mixint kernels below): the points are cast (mixint.h) as they are staged.
template <bool TYPED>
__device__ __forceinline__ void gmx_probas_body(const double *__restrict__ xq, int64_t m, int d, int k,
                                                const double *__restrict__ means, const double *__restrict__ precs,
                                                const double *__restrict__ par, double *__restrict__ probas,
                                                const mixint::Col *__restrict__ spec) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int64_t q0 = (int64_t)blockIdx.x * 64;
    const int lane = threadIdx.x, ds = d | 1;
    const int rows = (int)((m - q0 < 64) ? (m - q0) : 64);
    for (int e = lane; e < rows * d; e += 64) {
        const int i = e / d, j = e - i * d;
        if (TYPED) sm[i * ds + j] = mixint::cast_coord(spec, mixint::table_values(spec, d), xq + (q0 + i) * d, 1, j);
        else sm[i * ds + j] = xq[q0 * d + e];
    }
    __syncthreads();
    if (lane >= rows) return;
    gmx_probas_point(sm + lane * ds, d, k, means, precs, par, probas + (q0 + lane) * k);
}
__global__ __launch_bounds__(64) void k_gmx_probas(const double *__restrict__ xq, int64_t m, int d, int k,
                                                  const double *__restrict__ means, const double *__restrict__ precs,
                                                  const double *__restrict__ par, double *__restrict__ probas) {
    gmx_probas_body<false>(xq, m, d, k, means, precs, par, probas, nullptr);
}
__global__ __launch_bounds__(64) void k_gmx_probas_mixint(const double *__restrict__ xq, int64_t m, int d, int k,
                                                         const double *__restrict__ means, const double *__restrict__ precs,
                                                         const double *__restrict__ par, double *__restrict__ probas,
                                                         const mixint::Col *__restrict__ spec) {
    gmx_probas_body<true>(xq, m, d, k, means, precs, par, probas, spec);
}

// ... and their x-derivatives (gmx_probas_deriv_point), one lane per point: the lane's scratch (x, z, v': d each; u: k) in LDS.
template <bool TYPED>
__device__ __forceinline__ void gmx_probas_deriv_body(const double *__restrict__ xq, int64_t m, int d, int k,
                                                      const double *__restrict__ means, const double *__restrict__ precs,
                                                      const double *__restrict__ par, double *__restrict__ out,
                                                      const mixint::Col *__restrict__ spec) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int64_t q0 = (int64_t)blockIdx.x * 64;
    const int lane = threadIdx.x, ds = d | 1, ks = k | 1;
    const int rows = (int)((m - q0 < 64) ? (m - q0) : 64);
    double *xs = sm, *zs = sm + 64 * ds, *vps = zs + 64 * ds, *us = vps + 64 * ds;
    for (int e = lane; e < rows * d; e += 64) {
        const int i = e / d, j = e - i * d;
        if (TYPED) xs[i * ds + j] = mixint::cast_coord(spec, mixint::table_values(spec, d), xq + (q0 + i) * d, 1, j);
        else xs[i * ds + j] = xq[q0 * d + e];
    }
    __syncthreads();
    if (lane >= rows) return;
    gmx_probas_deriv_point(xs + lane * ds, zs + lane * ds, vps + lane * ds, us + lane * ks, d, k, means, precs, par,
                           out + (q0 + lane) * (int64_t)k * d);
}
__global__ __launch_bounds__(64) void k_gmx_probas_deriv(const double *__restrict__ xq, int64_t m, int d, int k,
                                                        const double *__restrict__ means, const double *__restrict__ precs,
                                                        const double *__restrict__ par, double *__restrict__ out) {
    gmx_probas_deriv_body<false>(xq, m, d, k, means, precs, par, out, nullptr);
}
__global__ __launch_bounds__(64) void k_gmx_probas_deriv_mixint(const double *__restrict__ xq, int64_t m, int d, int k,
                                                               const double *__restrict__ means, const double *__restrict__ precs,
                                                               const double *__restrict__ par, double *__restrict__ out,
                                                               const mixint::Col *__restrict__ spec) {
    gmx_probas_deriv_body<true>(xq, m, d, k, means, precs, par, out, spec);
}

int launch_gmx_probas(bool deriv, const double *xq, int64_t m, int d, int k, const double *blk, size_t lds, double *out,
                      const mixint::Col *spec) {
    const double *precs = blk + (size_t)k * d, *par = precs + (size_t)k * d * d;
    const dim3 grid((unsigned)((m + 63) / 64));
    if (deriv && lds > 64 * 1024)
        EGX_HIP_CHECK(hipFuncSetAttribute(spec ? reinterpret_cast<const void *>(&k_gmx_probas_deriv_mixint)
                                               : reinterpret_cast<const void *>(&k_gmx_probas_deriv),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (deriv && spec) hipLaunchKernelGGL(k_gmx_probas_deriv_mixint, grid, dim3(64), lds, 0, xq, m, d, k, blk, precs, par, out, spec);
    else if (deriv) hipLaunchKernelGGL(k_gmx_probas_deriv, grid, dim3(64), lds, 0, xq, m, d, k, blk, precs, par, out);
    else if (spec) hipLaunchKernelGGL(k_gmx_probas_mixint, grid, dim3(64), lds, 0, xq, m, d, k, blk, precs, par, out, spec);
    else hipLaunchKernelGGL(k_gmx_probas, grid, dim3(64), lds, 0, xq, m, d, k, blk, precs, par, out);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

}  // namespace egx
