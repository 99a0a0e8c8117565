// The factorisation's panel solve ALONE (HIP events around single launches): 8 matrices in lock-step, one factored 256 x 256
// diagonal block each, panels of 15360 / 8192 / 4096 / 2048 / 1024 rows below it at the row stride of an n = 16384 fit.
// Per height: us per launch of the column-strip kernel launch_potrf took before k_panel_trsm_rows (k_panel_trsm16<2> from
// 4096 rows, <1> below) and of k_panel_trsm_rows, against the MFMA floor (544 v_mfma_f64_16x16x4 of 64 cycles per 16-row
// tile, 1024 SIMDs, 2.4 GHz), and whether the two kernels leave the same bits (also for a 128-wide block).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/panel_solve_alone.hip -o tools/panel_solve_alone
#include "../egobox_amd/csrc/kernels_chol.hip"
#include "../egobox_amd/csrc/kernels_pipe.hip"  // (launch_potrf refers to the chain launch)
#include <cstdio>
#include <cstring>
#include <vector>
namespace egx {
void set_error(const std::string &m) { fprintf(stderr, "error: %s\n", m.c_str()); }
hipError_t dev_malloc_bytes(void **p, size_t bytes) { return hipMalloc(p, bytes); }
}  // namespace egx
using namespace egx;
#define CK(e)                                                                      \
    do {                                                                           \
        hipError_t e_ = (e);                                                       \
        if (e_ != hipSuccess) {                                                    \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

// columns [0, 256) of every matrix: an SPD diagonal block (1 / (1 + |i - j|), + 2 on the diagonal), hashed rows below
__global__ void k_fill(double *M, int64_t ld, int64_t sM, int n) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)n * 256) return;
    const int i = (int)(e >> 8), j = (int)(e & 255), z = blockIdx.y;
    double v;
    if (i < 256) {
        v = 1.0 / (1.0 + (i > j ? i - j : j - i)) + (i == j ? 2.0 + 0.01 * z : 0.0);
    } else {
        unsigned int h = (unsigned int)(e * 2654435761u) ^ (unsigned int)(z * 40503u + 12345u);
        h ^= h >> 15, h *= 2246822519u, h ^= h >> 13;
        v = (double)(h & 0xfffff) / 524288.0 - 1.0;
    }
    M[z * sM + (int64_t)i * ld + j] = v;
}

int main() {
    const int nz = 8, n = 16384, nbk = 256;
    const int64_t ld = n, sM = (int64_t)n * ld, sD = (int64_t)dinv_doubles(n);
    if (chol_init()) return 1;
    double *M, *dinv, *keep, *out[2];
    int *info;
    const size_t panel_bytes = sizeof(double) * 256 * (size_t)(n - 256);
    CK(hipMalloc(&M, sizeof(double) * sM * nz));
    CK(hipMalloc(&dinv, sizeof(double) * sD * nz));
    CK(hipMalloc(&keep, panel_bytes * nz));
    CK(hipMalloc(&out[0], panel_bytes * nz));
    CK(hipMalloc(&out[1], panel_bytes * nz));
    CK(hipMalloc(&info, sizeof(int) * nz));
    CK(hipMemset(info, 0, sizeof(int) * nz));
    CK(hipMemset(dinv, 0, sizeof(double) * sD * nz));
    hipLaunchKernelGGL(k_fill, dim3((unsigned)(((int64_t)n * 256 + 255) / 256), nz), dim3(256), 0, 0, M, ld, sM, n);
    hipLaunchKernelGGL(k_potf2_reg<16>, dim3(1, 1, nz), dim3(1024), RB_LDS_BYTES, 0, M, ld, nbk, dinv, info, 0, n, sM, sD, 1);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    int hinfo[nz];
    CK(hipMemcpy(hinfo, info, sizeof(hinfo), hipMemcpyDeviceToHost));
    for (int z = 0; z < nz; z++)
        if (hinfo[z]) {
            fprintf(stderr, "diagonal block of matrix %d failed: info %d\n", z, hinfo[z]);
            return 1;
        }
    double *P = M + (int64_t)nbk * ld;
    auto copy_panel = [&](double *dst, int64_t dld, int64_t dstride, const double *src, int64_t sld, int64_t sstride, int rows) {
        for (int z = 0; z < nz; z++)
            (void)hipMemcpy2DAsync(dst + z * dstride, dld * 8, src + z * sstride, sld * 8, 256 * 8, rows, hipMemcpyDeviceToDevice, 0);
    };
    const int64_t sK = 256 * (int64_t)(n - 256);
    copy_panel(keep, 256, sK, P, ld, sM, n - 256);
    CK(hipDeviceSynchronize());
    auto launch = [&](int which, int rows, int K) {
        if (which == 1)
            hipLaunchKernelGGL(k_panel_trsm_rows, dim3(rows / 64, 1, nz), dim3(256), PR_LDS_BYTES, 0, P, ld, (const double *)M, ld,
                               (const double *)dinv, K, (const int *)info, sM, sM, sD, 1);
        else if (rows >= 4096)
            hipLaunchKernelGGL((k_panel_trsm16<2, false>), dim3(rows / 32, 1, nz), dim3(256), 0, 0, P, ld, (const double *)M, ld,
                               (const double *)dinv, K, (const int *)info, sM, sM, sD, 1, (const double *)nullptr);
        else
            hipLaunchKernelGGL((k_panel_trsm16<1, false>), dim3(rows / 16, 1, nz), dim3(256), 0, 0, P, ld, (const double *)M, ld,
                               (const double *)dinv, K, (const int *)info, sM, sM, sD, 1, (const double *)nullptr);
    };
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::vector<double> h0, h1;
    // the same bits: 15360 rows under the 256-wide block, 4096 rows under its leading 128 x 128 block
    for (int K : {256, 128}) {
        const int rows = K == 256 ? 15360 : 4096;
        for (int which = 0; which < 2; which++) {
            copy_panel(P, ld, sM, keep, 256, sK, rows);
            launch(which, rows, K);
            copy_panel(out[which], 256, sK, P, ld, sM, rows);
        }
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        size_t differ = 0, changed = 0;
        for (int z = 0; z < nz; z++) {
            const size_t cnt = (size_t)rows * 256;
            h0.resize(cnt), h1.resize(cnt);
            std::vector<double> hk(cnt);
            CK(hipMemcpy(h0.data(), out[0] + z * sK, cnt * 8, hipMemcpyDeviceToHost));
            CK(hipMemcpy(h1.data(), out[1] + z * sK, cnt * 8, hipMemcpyDeviceToHost));
            CK(hipMemcpy(hk.data(), keep + z * sK, cnt * 8, hipMemcpyDeviceToHost));
            for (size_t e = 0; e < cnt; e++) {
                differ += std::memcmp(&h0[e], &h1[e], 8) != 0;
                changed += (int)(e & 255) < K && std::memcmp(&h0[e], &hk[e], 8) != 0;
            }
        }
        printf("K %3d rows %5d: %zu of %zu doubles differ between the kernels (%zu were changed by the solve)\n", K, rows, differ,
               (size_t)nz * rows * 256, changed);
    }
    for (int rows : {15360, 8192, 4096, 2048, 1024}) {
        double us[2] = {0.0, 0.0}, best[2] = {1e30, 1e30};
        const int reps = 12, warm = 2;
        for (int r = 0; r < reps; r++)
            for (int which = 0; which < 2; which++) {  // interleaved
                copy_panel(P, ld, sM, keep, 256, sK, rows);
                CK(hipEventRecord(e0, 0));
                launch(which, rows, nbk);
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                float ms = 0.f;
                CK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= warm) {
                    us[which] += 1e3 * ms / (reps - warm);
                    if (1e3 * ms < best[which]) best[which] = 1e3 * ms;
                }
            }
        CK(hipGetLastError());
        const double floor_us = (double)nz * rows / 16 * 544 * 64 / 1024 / 2.4e3;
        printf("rows %5d x %d matrices: k_panel_trsm16<%d> %.1f us (best %.1f), k_panel_trsm_rows %.1f us (best %.1f), MFMA floor %.1f us "
               "-> %.2fx / %.2fx of the floor\n",
               rows, nz, rows >= 4096 ? 2 : 1, us[0], best[0], us[1], best[1], floor_us, us[0] / floor_us, us[1] / floor_us);
    }
    return 0;
}
