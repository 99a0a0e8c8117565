// PLS rotations (the KPLS weights w_star) from data on the device: egx_pls_rotations, and pls_device_rotations for the sparse
// handle's resident training set (egx_sgp_compute_w_star, sgp_host.hip).
//
//   k_pls_means   one workgroup per column of [X | y]: the column's mean over rows 0 .. n-1, summed in an order fixed by n.
//   k_pls_gram    C = A^T A for A = [X - mean | y - mean] (n x (d + 1), unscaled) on v_mfma_f64_16x16x4_f64.  The data rows are
//                 the K dimension; the input is k-major (one column contiguous over the rows, leading dimension ld), so both
//                 operands are K-contiguous: the shape of mfma_gemm_core.h, whose LDS layout and fragment reads this kernel keeps
//                 (lane l: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]; C reg r: row (l >> 4) + 4 r, col l & 15).  It has
//                 its own loader because the operands are centred -- and rows >= n forced to exactly 0 -- between the global load
//                 and the LDS store.  A workgroup owns one 64 x 64 block of the lower triangle (wave w: tile row w, 4 tile columns;
//                 tiles above the diagonal or wholly beyond column d are skipped) over one chunk of rows (split-K) and writes its
//                 own partial block: no atomics.
//   k_pls_sum     the partial blocks added in chunk order.
// The plan (rows per chunk, chunks, tiles, blocks) comes from pls_host.h alone; so does everything after the Gram matrix.
#include <cmath>
#include <cstring>
#include <vector>

#include "dev_mem.h"
#include "egx_internal.h"
#include "mfma_gemm_core.h"  // KC, LDS_LD, d2_t, double4_t
#include "pls_host.h"

using namespace egx;

namespace {

constexpr int kMeanThreads = 1024;
constexpr int kB = pls::kBlockCols;        // 64 columns per side of a workgroup's block
constexpr int kSide = kB * LDS_LD;         // doubles of one staged operand (64 columns x 16 rows, padded)
constexpr int kBlockElems = kB * kB;

// mean[c], c <= d (c == d: y).  Thread t adds the row pairs 2 t, 2 t + 2048, ..., four independent partial sums deep, then the
// 1024 sums meet in a binary tree: the order depends on n alone.  ld is even and >= n: the pair (n - 1, n) of an odd n is inside.
__global__ __launch_bounds__(kMeanThreads) void k_pls_means(const double *__restrict__ xT, int64_t ld, const double *__restrict__ y,
                                                            int64_t n, int d, double *__restrict__ mean) {
    __shared__ double sm[kMeanThreads];
    const int c = blockIdx.x, tid = threadIdx.x;
    const double *col = c < d ? xT + (int64_t)c * ld : y;
    constexpr int64_t step = 2 * kMeanThreads;
    int64_t r = 2 * (int64_t)tid;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, tail = 0.0;
    for (; r + 3 * step + 1 < n; r += 4 * step) {
        const d2_t v0 = *reinterpret_cast<const d2_t *>(col + r);
        const d2_t v1 = *reinterpret_cast<const d2_t *>(col + r + step);
        const d2_t v2 = *reinterpret_cast<const d2_t *>(col + r + 2 * step);
        const d2_t v3 = *reinterpret_cast<const d2_t *>(col + r + 3 * step);
        a0 += v0[0] + v0[1];
        a1 += v1[0] + v1[1];
        a2 += v2[0] + v2[1];
        a3 += v3[0] + v3[1];
    }
    for (; r < n; r += step) {
        const d2_t v = *reinterpret_cast<const d2_t *>(col + r);
        tail += v[0] + ((r + 1 < n) ? v[1] : 0.0);
    }
    sm[tid] = ((a0 + a1) + (a2 + a3)) + tail;
    __syncthreads();
    for (int h = kMeanThreads / 2; h > 0; h >>= 1) {
        if (tid < h) sm[tid] += sm[tid + h];
        __syncthreads();
    }
    if (tid == 0) mean[c] = sm[0] / (double)n;
}

// one side's share of a K chunk: the thread's two columns (cl, cl + 32 of the block), rows r and r + 1; rows >= r1 are exactly 0
struct PlsCols {
    const double *p[2];
    double m[2];
};
__device__ __forceinline__ void pls_cols(PlsCols &c, int block, int cl, const double *xT, int64_t ld, const double *y,
                                         const double *mean, int d) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int gc = block * kB + cl + 32 * i;
        c.p[i] = gc < d ? xT + (int64_t)gc * ld : (gc == d ? y : nullptr);
        c.m[i] = gc <= d ? mean[gc] : 0.0;
    }
}
__device__ __forceinline__ void pls_fetch(const PlsCols &c, int64_t r, int64_t r1, d2_t (&v)[2]) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
        v[i] = d2_t{0.0, 0.0};
        if (c.p[i] && r < r1) {
            const d2_t x = *reinterpret_cast<const d2_t *>(c.p[i] + r);
            v[i][0] = x[0] - c.m[i];
            v[i][1] = (r + 1 < r1) ? x[1] - c.m[i] : 0.0;
        }
    }
}
__device__ __forceinline__ void pls_stage(double *S, int cl, int ro, const d2_t (&v)[2]) {
#pragma unroll
    for (int i = 0; i < 2; i++) *reinterpret_cast<d2_t *>(S + (cl + 32 * i) * LDS_LD + ro) = v[i];
}

// grid.x = block pair (bi >= bj) of the lower triangle, grid.y = chunk of rows.  part: [chunk][pair][64][64]
__global__ __launch_bounds__(256, 4) void k_pls_gram(const double *__restrict__ xT, int64_t ld, const double *__restrict__ y,
                                                  const double *__restrict__ mean, int64_t n, int d, int64_t chunk_rows,
                                                  double *__restrict__ part) {
    __shared__ double smem[2 * 2 * kSide];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int bi = 0, bj = blockIdx.x;
    while (bj > bi) {
        bj -= bi + 1;
        bi++;
    }
    const bool diag = bi == bj;
    const int64_t r0 = (int64_t)blockIdx.y * chunk_rows;
    const int64_t r1 = (r0 + chunk_rows < n) ? r0 + chunk_rows : n;
    const int nk = (int)((r1 - r0 + KC - 1) / KC);
    const int cl = tid >> 3, ro = 2 * (tid & 7);
    PlsCols ca, cb;
    pls_cols(ca, bi, cl, xT, ld, y, mean, d);
    pls_cols(cb, bj, cl, xT, ld, y, mean, d);

    const int frow = lane & 15, fk = lane >> 4;
    const int d1 = d + 1;
    const bool row_live = bi * kB + wave * 16 < d1;
    // the wave's live tile columns are a prefix: on or below the diagonal, and not wholly beyond column d
    int nlive = row_live ? (d1 - bj * kB + 15) / 16 : 0;
    if (nlive > 4) nlive = 4;
    if (diag && nlive > wave + 1) nlive = wave + 1;
    double4_t acc[4];
#pragma unroll
    for (int ni = 0; ni < 4; ni++) acc[ni] = double4_t{0.0, 0.0, 0.0, 0.0};

    d2_t ra[2], rb[2];
    pls_fetch(ca, r0 + ro, r1, ra);
    pls_stage(smem, cl, ro, ra);
    if (!diag) {
        pls_fetch(cb, r0 + ro, r1, rb);
        pls_stage(smem + kSide, cl, ro, rb);
    }
    __syncthreads();
    for (int c = 0; c < nk; c++) {
        const double *As = smem + (c & 1) * 2 * kSide;
        const double *Bs = diag ? As : As + kSide;
        const bool more = c + 1 < nk;
        if (more) {
            const int64_t r = r0 + (int64_t)(c + 1) * KC + ro;
            pls_fetch(ca, r, r1, ra);
            if (!diag) pls_fetch(cb, r, r1, rb);
        }
#pragma unroll
        for (int kk = 0; kk < KC / 4; kk++) {
            const double a = As[(wave * 16 + frow) * LDS_LD + kk * 4 + fk];
#pragma unroll
            for (int ni = 0; ni < 4; ni++)
                if (ni < nlive) {
                    const double b = Bs[(ni * 16 + frow) * LDS_LD + kk * 4 + fk];
                    acc[ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[ni], 0, 0, 0);
                }
        }
        if (more) {
            double *Sn = smem + ((c + 1) & 1) * 2 * kSide;
            pls_stage(Sn, cl, ro, ra);
            if (!diag) pls_stage(Sn + kSide, cl, ro, rb);
        }
        __syncthreads();
    }
    double *out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kBlockElems;
#pragma unroll
    for (int ni = 0; ni < 4; ni++)
#pragma unroll
        for (int r = 0; r < 4; r++) out[(wave * 16 + fk + 4 * r) * kB + ni * 16 + frow] = acc[ni][r];
}

// out[e] = part[0][e] + part[1][e] + ... in chunk order, e < count
__global__ __launch_bounds__(256) void k_pls_sum(const double *__restrict__ part, int64_t count, int chunks, double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    double s = part[e];
    for (int c = 1; c < chunks; c++) s += part[(int64_t)c * count + e];
    out[e] = s;
}

// xT[k * ld + i] = x[i * d + k] (i < n, k < d), 0 for n <= i < ld: 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void k_pls_transpose(const double *__restrict__ x, int64_t n, int d, double *__restrict__ xT,
                                                       int64_t ld) {
    __shared__ double tile[32][33];
    const int64_t i0 = (int64_t)blockIdx.x * 32;
    const int k0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int64_t i = i0 + r;
        const int k = k0 + tx;
        tile[r][tx] = (i < n && k < d) ? x[i * d + k] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r;
        const int64_t i = i0 + tx;
        if (k < d && i < ld) xT[(int64_t)k * ld + i] = tile[tx][r];
    }
}

struct PlsWork {
    egx_pls_plan plan{};
    DevBuf mean, part, sum;
};

int pls_work_alloc(PlsWork &w, int64_t n, int d) {
    if (!pls::plan(n, d, &w.plan)) {
        set_error("PLS rotations: need n >= 1 and d >= 1");
        return EGX_ERR_INVALID_VALUE;
    }
    const size_t blk = (size_t)w.plan.blocks * kBlockElems;
    int rc = w.mean.alloc((size_t)d + 1);
    if (!rc) rc = w.part.alloc(blk * (size_t)w.plan.n_chunks);
    if (!rc) rc = w.sum.alloc(blk);
    return rc;
}

// the three launches; xT (d x ld, ld even and >= n, 16-byte aligned) and y (n rounded up to even doubles) on the device
int pls_launch(hipStream_t s, const double *xT, int64_t ld, const double *y, int64_t n, int d, PlsWork &w) {
    const egx_pls_plan &p = w.plan;
    if ((ld & 1) || ld < n) {
        set_error("PLS rotations: the leading dimension must be even and >= n");
        return EGX_ERR_INVALID_VALUE;
    }
    k_pls_means<<<dim3((unsigned)(d + 1)), dim3(kMeanThreads), 0, s>>>(xT, ld, y, n, d, w.mean.p);
    k_pls_gram<<<dim3((unsigned)p.blocks, (unsigned)p.n_chunks), dim3(256), 0, s>>>(xT, ld, y, w.mean.p, n, d, p.chunk_rows, w.part.p);
    const int64_t count = p.blocks * kBlockElems;
    k_pls_sum<<<dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s>>>(w.part.p, count, (int)p.n_chunks, w.sum.p);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

}  // namespace

namespace egx {

int pls_device_rotations(hipStream_t s, const double *xT, int64_t ld, const double *y, int64_t n, int d, int k, double *w,
                         int *status) {
    PlsWork wk;
    int rc = pls_work_alloc(wk, n, d);
    if (rc) return rc;
    rc = pls_launch(s, xT, ld, y, n, d, wk);
    if (rc) return rc;
    const int d1 = d + 1;
    const size_t blk = (size_t)wk.plan.blocks * kBlockElems;
    std::vector<double> sum(blk), mean((size_t)d1), C((size_t)d1 * d1, 0.0);
    EGX_HIP_CHECK(hipMemcpyAsync(sum.data(), wk.sum.p, sizeof(double) * blk, hipMemcpyDeviceToHost, s));
    EGX_HIP_CHECK(hipMemcpyAsync(mean.data(), wk.mean.p, sizeof(double) * d1, hipMemcpyDeviceToHost, s));
    EGX_HIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < d1; i++)
        for (int j = 0; j <= i; j++) {
            const int bi = i / kB, bj = j / kB;
            const size_t pair = (size_t)bi * (bi + 1) / 2 + bj;
            C[(size_t)i * d1 + j] = sum[pair * kBlockElems + (size_t)(i % kB) * kB + (j % kB)];
        }
    const int st = pls::rotations_from_centred(C.data(), mean.data(), n, d, k, w);
    if (status) *status = st;
    return EGX_SUCCESS;
}

int pls_device_launch_ms(hipStream_t s, const double *xT, int64_t ld, const double *y, int64_t n, int d, double *ms) {
    PlsWork wk;
    int rc = pls_work_alloc(wk, n, d);
    if (rc) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EGX_HIP_CHECK(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
        (void)hipEventDestroy(e0);
        set_error("hipEventCreate failed");
        return EGX_ERR_HIP;
    }
    float t = 0.0f;
    hipError_t e = hipEventRecord(e0, s);
    if (e == hipSuccess) rc = pls_launch(s, xT, ld, y, n, d, wk);
    if (e == hipSuccess && !rc) e = hipEventRecord(e1, s);
    if (e == hipSuccess && !rc) e = hipEventSynchronize(e1);
    if (e == hipSuccess && !rc) e = hipEventElapsedTime(&t, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (e != hipSuccess) {
        set_error(std::string("PLS launch timing: ") + hipGetErrorString(e));
        (void)hipGetLastError();
        return EGX_ERR_HIP;
    }
    *ms = (double)t;
    return EGX_SUCCESS;
}

int pls_check_k(int64_t k, int64_t d) {
    if (k < 1) {  // parameters.rs / sparse_parameters.rs:306-311
        set_error("`kpls_dim` canot be 0!");
        return EGX_ERR_INVALID_VALUE;
    }
    if (k > d) {  // sparse_algorithm.rs:430-438
        set_error("Dimension reduction " + std::to_string(k) + " should be smaller than actual training input dimensions " +
                  std::to_string(d));
        return EGX_ERR_INVALID_VALUE;
    }
    return EGX_SUCCESS;
}

}  // namespace egx

int32_t egx_pls_get_plan(int64_t n, int64_t d, egx_pls_plan *out) {
    if (!pls::plan(n, d, out)) {
        set_error("egx_pls_get_plan: need n >= 1, d >= 1 and an output");
        return EGX_ERR_INVALID_VALUE;
    }
    return EGX_SUCCESS;
}

int32_t egx_pls_rotations(int32_t device, const double *x, const double *y, int64_t n, int64_t d, int64_t k, double *w,
                          int32_t *status) {
    if (k < 1) return pls_check_k(k, 1);  // refused first, as egx_sgp_set_w_star refuses it
    if (!x || !y || !w) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    if (d < 1 || n < 2) {
        set_error("egx_pls_rotations: need x (n x d), y (n) with n >= 2, d >= 1");
        return EGX_ERR_INVALID_VALUE;
    }
    int rc = pls_check_k(k, d);
    if (rc) return rc;
    for (int64_t i = 0; i < n * d; i++)
        if (!std::isfinite(x[i])) {
            set_error("x contains non-finite values");
            return EGX_ERR_INVALID_VALUE;
        }
    for (int64_t i = 0; i < n; i++)
        if (!std::isfinite(y[i])) {
            set_error("y contains non-finite values");
            return EGX_ERR_INVALID_VALUE;
        }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device: libegx_gp_hip has no CPU fallback (needs an MI355X / gfx950 GPU)");
        return EGX_ERR_NO_DEVICE;
    }
    int dev = device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (dev >= ndev) {
        set_error("device ordinal out of range");
        return EGX_ERR_INVALID_VALUE;
    }
    EGX_HIP_CHECK(hipSetDevice(dev));
    const int64_t ld = round_up(n, 16);
    DevBuf xr, xT, yd;
    if ((rc = xr.alloc((size_t)n * d)) || (rc = xT.alloc((size_t)d * ld)) || (rc = yd.alloc((size_t)ld))) return rc;
    hipStream_t s = nullptr;  // the default stream: the copies below are synchronous
    EGX_HIP_CHECK(hipMemcpy(xr.p, x, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice));
    EGX_HIP_CHECK(hipMemsetAsync(yd.p, 0, sizeof(double) * (size_t)ld, s));
    EGX_HIP_CHECK(hipMemcpy(yd.p, y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    k_pls_transpose<<<dim3((unsigned)((ld + 31) / 32), (unsigned)((d + 31) / 32)), dim3(256), 0, s>>>(xr.p, n, (int)d, xT.p, ld);
    EGX_HIP_CHECK(hipGetLastError());
    int st = 0;
    rc = pls_device_rotations(s, xT.p, ld, yd.p, n, (int)d, (int)k, w, &st);
    if (rc) return rc;
    if (status) *status = st;
    return EGX_SUCCESS;
}
