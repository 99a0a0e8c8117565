// Kernels of posterior sampling (gp_sample.hip; GaussianProcess::sample*, crates/gp/src/algorithm.rs:383-395, 1153-1193):
//   k_sample_u       u = Rq^-T (ft^T rt - f(x)) per query, on the device (algorithm.rs:352-367)
//   k_normals        the Philox4x64-10 / Box-Muller stream of philox.h into any (row, column) strides
//   k_trmm_mean      traj = mean 1^T + L Z with L lower triangular: FP64 MFMA (mfma_gemm_core.h), zero upper tiles skipped
// The query-query covariance itself is assembled beside the other correlation kernels (kernels_corr.hip k_cov_assemble).
#include "egx_internal.h"
#include "mfma_gemm_core.h"
#include "philox.h"
#include "trend_column.h"

namespace egx {

// One wave per query q: s = sl[q] - f(x_q) in LDS, then the forward substitution with Rq^T (Rq = ft_qr_r, p x p row-major,
// upper) column by column: u_i = s_i / Rq_ii, s_j -= Rq_ij u_i (j > i) -- the subtractions of predict_impl's host loop, in
// its order.  f(x) from the normalised query (k-major xqT) by trend_column.h.  Rows q >= m of U are zero.
__global__ __launch_bounds__(64) void k_sample_u(const double *__restrict__ sl, int p, const double *__restrict__ xqT,
                                                 int64_t ldq, const int *__restrict__ fidx, const double *__restrict__ R, int m,
                                                 double *__restrict__ U, double *__restrict__ Uneg, int64_t ldu) {
    extern __shared__ double s[];
    const int q = blockIdx.x, lane = threadIdx.x;
    double *urow = U + (int64_t)q * ldu, *nrow = Uneg + (int64_t)q * ldu;
    if (q >= m) {
        for (int l = lane; l < ldu; l += 64) urow[l] = nrow[l] = 0.0;
        return;
    }
    for (int l = lane; l < p; l += 64) s[l] = sl[(int64_t)q * p + l] - trend_column(fidx, l, xqT, ldq, q);
    __syncthreads();
    for (int i = 0; i < p; i++) {
        const double ui = s[i] / R[(int64_t)i * p + i];
        __syncthreads();  // every lane has read s[i]
        if (lane == 0) s[i] = ui;
        for (int j = i + 1 + lane; j < p; j += 64) s[j] -= R[(int64_t)i * p + j] * ui;
        __syncthreads();
    }
    for (int l = lane; l < ldu; l += 64) {
        const double v = l < p ? s[l] : 0.0;
        urow[l] = v;
        nrow[l] = -v;
    }
}

// Z[i * si + j * sj] = normal (i, j) of philox.h for i < m, j < nt; one thread per block of four rows
__global__ __launch_bounds__(256) void k_normals(uint64_t seed, int64_t m, int64_t nt, double *__restrict__ Z, int64_t si,
                                                 int64_t sj) {
    const int64_t G = (m + 3) / 4, total = G * nt;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = e / G, g = e % G;
        double z[4];
        philox::normals4(seed, (uint64_t)g, (uint64_t)j, z);
#pragma unroll
        for (int h = 0; h < 4; h++)
            if (4 * g + h < m) Z[(4 * g + h) * si + j * sj] = z[h];
    }
}

// T (m_pad x nt_pad, ldt) = mean 1^T + L Zt^T: L (m_pad x m_pad, ldl) lower triangular with a ZERO strict upper triangle,
// Zt (nt_pad x m_pad, ldz) the normals transposed (K-contiguous, as the MFMA core reads both operands).  128 x 64 output tiles,
// 8 waves of 32 x 32; row tile bx contracts over columns [0, 128 (bx + 1)) only: the tiles right of the diagonal are zero.
// Every output's K loop is the same for any nt_pad (no split over K), so a column of T does not depend on how many follow.
using TrmmShape = GemmShape<128, 64, 32, 32, 512>;
__global__ __launch_bounds__(512, 2) void k_trmm_mean(const double *__restrict__ L, int64_t ldl, const double *__restrict__ Zt,
                                                      int64_t ldz, const double *__restrict__ mean, double *__restrict__ T,
                                                      int64_t ldt, int nbx, int nby) {
    using S = TrmmShape;
    // longest contractions first (the row tiles at the bottom), the short ones fill the tail of the launch
    const int t = blockIdx.x;
    const int bx = nbx - 1 - t / nby, by = t % nby;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x;
    double4_t acc[S::MT][S::NT];
#pragma unroll
    for (int mi = 0; mi < S::MT; mi++)
#pragma unroll
        for (int ni = 0; ni < S::NT; ni++) acc[mi][ni] = double4_t{0.0, 0.0, 0.0, 0.0};
    gemm_core<128, 64, 32, 32, 512>(L + (int64_t)bx * 128 * ldl, ldl, Zt + (int64_t)by * 64 * ldz, ldz, (bx + 1) * 128, acc,
                                    smem, tid);
    const int wave = tid >> 6, lane = tid & 63;
    const int r0 = bx * 128 + (wave / S::WAVES_N) * 32 + (lane >> 4);
    const int c0 = by * 64 + (wave % S::WAVES_N) * 32 + (lane & 15);
#pragma unroll
    for (int mi = 0; mi < S::MT; mi++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = r0 + mi * 16 + 4 * r;
            const double mu = mean[row];
#pragma unroll
            for (int ni = 0; ni < S::NT; ni++) T[(int64_t)row * ldt + c0 + ni * 16] = mu + acc[mi][ni][r];
        }
}

int launch_sample_u(hipStream_t s, const double *sl, int p, const double *xqT, int64_t ldq, const int *fidx, const double *R,
                    int m, int m_pad, double *U, double *Uneg, int64_t ldu) {
    if ((size_t)p * sizeof(double) > 65536) {
        set_error("sample: more than 8192 regression columns");
        return EGX_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(k_sample_u, dim3((unsigned)m_pad), dim3(64), (size_t)p * sizeof(double), s, sl, p, xqT, ldq, fidx, R, m,
                       U, Uneg, ldu);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_normals(hipStream_t s, uint64_t seed, int64_t m, int64_t nt, double *Z, int64_t si, int64_t sj) {
    const int64_t total = (m + 3) / 4 * nt;
    if (total <= 0) return EGX_SUCCESS;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_normals, dim3((unsigned)blocks), dim3(256), 0, s, seed, m, nt, Z, si, sj);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

int launch_trmm_mean(hipStream_t s, const double *L, int64_t ldl, int m_pad, const double *Zt, int64_t ldz, int nt_pad,
                     const double *mean, double *T, int64_t ldt) {
    if (m_pad % 128 || nt_pad % 64 || ldl % 2 || ldz % 2) {
        set_error("trmm_mean: m_pad must be a multiple of 128, nt_pad of 64, the leading dimensions even");
        return EGX_ERR_INVALID_VALUE;
    }
    if (m_pad == 0 || nt_pad == 0) return EGX_SUCCESS;
    const int nbx = m_pad / 128, nby = nt_pad / 64;
    hipLaunchKernelGGL(k_trmm_mean, dim3((unsigned)(nbx * nby)), dim3(512), TrmmShape::LDS_BYTES, s, L, ldl, Zt, ldz, mean, T,
                       ldt, nbx, nby);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

}  // namespace egx
