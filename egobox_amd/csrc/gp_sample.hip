// Posterior covariance and trajectory sampling of a fitted dense GP (GpSurrogateExt::sample, crates/moe/src/surrogates.rs:66-81;
// GaussianProcess::_compute_covariance algorithm.rs:310-326, sample_chol / sample_eig / sample :383-395, helper :1153-1193).
// Everything of size m x m or m x n stays on the device; the host sees the m query points, m means and the result.
//   1. queries uploaded and normalised on the device (as predict_impl)
//   2. RT = C^-1 K(x, xt)^T, one row per query, and ft^T rt: posterior_solve (gp_predict.hip)
//   3. U = Rq^-T (ft^T rt - f(x)) per query (kernels_sample.hip k_sample_u; Rq and the column index: ensure_trend_state)
//   4. G = -RT RT^T + U U^T, lower tiles: two calls of the trailing-update GEMM (launch_gemm_nt_sub)
//   5. S = sigma2 (K(x, x) + G) + tau I, padded with the identity (kernels_corr.hip k_cov_assemble)
//   6. S = L L^T by launch_potrf; EGX_SAMPLE_PSD retries with tau x 10 on a failed pivot (the device info word)
//   7. Z: the philox.h stream (k_normals) or the caller's normals
//   8. traj = mean 1^T + L Z (k_trmm_mean: FP64 MFMA, zero upper tiles skipped)
// Steps 5-8 (sample_draw) also serve egx_sgp_sample, whose covariance is the prior sigma2 K(x, x) (sgp_host.hip).
#include <cstdio>

#include "gp_handle.h"

using namespace egx;

namespace egx {

// steps 5-8 for a covariance sigma2 (K(x, x) + G) described by `c` (G == nullptr: no Gram term), shared by the dense
// posterior (sample_impl) and the sparse GP's prior covariance (sgp_host.hip).  mean: m_pad doubles on the host.
int sample_draw(hipStream_t st, const SampleCov &c, int m, int nt, int method, uint64_t seed, const double *z,
                const double *mean, double *traj, double *tau_out) {
    const int m_pad = (int)round_up(m, kTile), nt_pad = (int)round_up(nt, 64);
    // EGX_SAMPLE_PSD: tau0 = max(1e-9, 1e-12 max_i Sigma_ii)
    double tau = method == EGX_SAMPLE_PSD ? std::max(1e-9, 1e-12 * c.max_diag) : 0.0;
    DevBuf S, dinv, info;
    EGX_RC(S.alloc((size_t)m_pad * m_pad));
    EGX_RC(dinv.alloc(dinv_doubles(m_pad)));
    EGX_RC(info.alloc(1));  // one int in a double-sized slot
    const int tries = method == EGX_SAMPLE_PSD ? 7 : 1;  // the first factorisation and at most six retries
    int piv = 0;
    for (int t = 0; t < tries; t++) {
        if (t) tau *= 10.0;
        EGX_RC(launch_cov_assemble(st, c.corr, c.xqT, m_pad, m_pad, c.d, c.coef, c.hcols, c.G, m_pad, m, c.sigma2, tau, S.p,
                                   m_pad));
        EGX_HIP_CHECK(hipMemsetAsync(info.p, 0, sizeof(double), st));
        EGX_RC(launch_potrf(st, S.p, m_pad, m_pad, m_pad, dinv.p, reinterpret_cast<int *>(info.p)));
        EGX_HIP_CHECK(hipMemcpyAsync(&piv, info.p, sizeof(int), hipMemcpyDeviceToHost, st));
        EGX_HIP_CHECK(hipStreamSynchronize(st));
        if (piv == 0) break;
    }
    if (piv != 0) {
        char msg[200];
        if (method == EGX_SAMPLE_CHOLESKY)
            std::snprintf(msg, sizeof msg, "sample_chol: the %s covariance is not positive definite (pivot %d)", c.what, piv);
        else
            std::snprintf(msg, sizeof msg, "sample: the %s covariance + %.3g I is not positive definite (pivot %d)", c.what, tau,
                          piv);
        set_error(msg);
        return EGX_ERR_LINALG;
    }
    EGX_RC(launch_zero_upper(st, S.p, m_pad, m_pad));
    // Z, transposed (nt_pad x m_pad, zero padded): the contraction operand the MFMA core reads K-contiguous
    DevBuf Zt, dmean, T;
    EGX_RC(Zt.alloc((size_t)nt_pad * m_pad));
    EGX_HIP_CHECK(hipMemsetAsync(Zt.p, 0, sizeof(double) * (size_t)nt_pad * m_pad, st));
    std::vector<double> zt;
    if (z) {
        zt.resize((size_t)nt * m);
        for (int64_t i = 0; i < m; i++)
            for (int j = 0; j < nt; j++) zt[(size_t)j * m + i] = z[(size_t)i * nt + j];
        EGX_HIP_CHECK(hipMemcpy2DAsync(Zt.p, sizeof(double) * m_pad, zt.data(), sizeof(double) * m, sizeof(double) * m, nt,
                                       hipMemcpyHostToDevice, st));
    } else {
        EGX_RC(launch_normals(st, seed, m, nt, Zt.p, 1, m_pad));
    }
    EGX_RC(dmean.alloc((size_t)m_pad));
    EGX_HIP_CHECK(hipMemcpyAsync(dmean.p, mean, sizeof(double) * m_pad, hipMemcpyHostToDevice, st));
    EGX_RC(T.alloc((size_t)m_pad * nt_pad));
    EGX_RC(launch_trmm_mean(st, S.p, m_pad, m_pad, Zt.p, m_pad, nt_pad, dmean.p, T.p, nt_pad));
    EGX_HIP_CHECK(hipMemcpy2DAsync(traj, sizeof(double) * nt, T.p, sizeof(double) * nt_pad, sizeof(double) * nt, m,
                                   hipMemcpyDeviceToHost, st));
    EGX_HIP_CHECK(hipStreamSynchronize(st));
    if (tau_out) *tau_out = tau;
    return EGX_SUCCESS;
}

namespace {

// device buffers of one covariance: the normalised queries, the solves and the Gram matrix G
struct CovBufs {
    DevBuf xraw, xqT, RT, s0, sl, U, Uneg, G;
    int m = 0, m_pad = 0;
};

// steps 1-4 on the handle's first workspace stream: leaves b.xqT (d x m_pad) and b.G (m_pad x m_pad, lower tiles)
int cov_prepare(egx_gp *gp, const double *xq, int m, CovBufs &b) {
    hipStream_t st = gp->ws[0].stream;
    const int n = gp->n, n_pad = gp->n_pad, d = gp->d, p = gp->p;
    const int m_pad = (int)round_up(m, kTile), pk = (int)round_up(p, 16);
    b.m = m, b.m_pad = m_pad;
    EGX_RC(ensure_trend_state(gp, st));
    EGX_RC(b.xraw.alloc((size_t)m * d));
    EGX_RC(b.xqT.alloc((size_t)d * m_pad));
    EGX_HIP_CHECK(hipMemcpyAsync(b.xraw.p, xq, sizeof(double) * (size_t)m * d, hipMemcpyHostToDevice, st));
    EGX_RC(launch_normalize_queries(st, b.xraw.p, m, d, dev_xnorm(gp), b.xqT.p, m_pad, m_pad, dev_spec(gp)));
    // rt (algorithm.rs:337-350), held transposed: the predict_var solve.  Its columns n .. n_pad - 1 (padding of the training
    // set) are not part of rt and are zeroed before the Gram matrix contracts over them.
    EGX_RC(b.RT.alloc((size_t)m_pad * n_pad));
    EGX_RC(b.s0.alloc(m_pad));
    EGX_RC(b.sl.alloc((size_t)m_pad * p));
    EGX_RC(posterior_solve(gp, st, b.xqT.p, m_pad, b.RT.p, b.s0.p, b.sl.p));
    if (n < n_pad)
        EGX_HIP_CHECK(hipMemset2DAsync(b.RT.p + n, sizeof(double) * n_pad, 0, sizeof(double) * (n_pad - n), m_pad, st));
    // u (algorithm.rs:352-367) on the device
    EGX_RC(b.U.alloc((size_t)m_pad * pk));
    EGX_RC(b.Uneg.alloc((size_t)m_pad * pk));
    EGX_RC(launch_sample_u(st, b.sl.p, p, b.xqT.p, m_pad, gp->d_fidx, gp->d_rq, m, m_pad, b.U.p, b.Uneg.p, pk));
    // G = 0 - RT RT^T - (-U) U^T, lower tiles
    EGX_RC(b.G.alloc((size_t)m_pad * m_pad));
    EGX_HIP_CHECK(hipMemsetAsync(b.G.p, 0, sizeof(double) * (size_t)m_pad * m_pad, st));
    EGX_RC(launch_gemm_nt_sub(st, b.G.p, m_pad, b.RT.p, n_pad, b.RT.p, n_pad, m_pad, m_pad, n_pad, 1));
    EGX_RC(launch_gemm_nt_sub(st, b.G.p, m_pad, b.Uneg.p, pk, b.U.p, pk, m_pad, m_pad, pk, 1));
    // (xq has been read, and a caller that fails from here on frees b with nothing in flight)
    EGX_HIP_CHECK(hipStreamSynchronize(st));
    return EGX_SUCCESS;
}

int check_cov_query(const egx_gp *gp, const double *xq, int64_t m) {
    EGX_RC(check_query(gp, xq, m));
    if (m > (int64_t)1 << 20) {
        set_error("covariance of more than 2^20 query points");
        return EGX_ERR_INVALID_VALUE;
    }
    return EGX_SUCCESS;
}

int covariance_impl(egx_gp *gp, const double *xq, int64_t m, double *cov) {
    EGX_RC(check_cov_query(gp, xq, m));
    if (m == 0) return EGX_SUCCESS;
    EGX_RC(set_device(gp));
    CovBufs b;
    EGX_RC(cov_prepare(gp, xq, (int)m, b));
    hipStream_t st = gp->ws[0].stream;
    DevBuf S;
    EGX_RC(S.alloc((size_t)b.m_pad * b.m_pad));
    EGX_RC(launch_cov_assemble(st, gp->corr, b.xqT.p, b.m_pad, b.m_pad, gp->d, gp->d_fit_coef, gp->fit_hcols, b.G.p, b.m_pad,
                               b.m, gp->sigma2, 0.0, S.p, b.m_pad));
    EGX_HIP_CHECK(hipMemcpy2DAsync(cov, sizeof(double) * m, S.p, sizeof(double) * b.m_pad, sizeof(double) * m, m,
                                   hipMemcpyDeviceToHost, st));
    EGX_HIP_CHECK(hipStreamSynchronize(st));
    return EGX_SUCCESS;
}

int sample_impl(egx_gp *gp, const double *xq, int64_t m, int64_t n_traj, int method, uint64_t seed, const double *z,
                double *traj, double *tau_out) {
    EGX_RC(check_cov_query(gp, xq, m));
    if (method != EGX_SAMPLE_CHOLESKY && method != EGX_SAMPLE_PSD) {
        set_error("sample: method must be EGX_SAMPLE_CHOLESKY or EGX_SAMPLE_PSD");
        return EGX_ERR_INVALID_VALUE;
    }
    if (n_traj < 0 || n_traj > ((int64_t)1 << 24)) {
        set_error("sample: bad number of trajectories");
        return EGX_ERR_INVALID_VALUE;
    }
    if (tau_out) *tau_out = 0.0;
    if (m == 0 || n_traj == 0) return EGX_SUCCESS;
    EGX_RC(set_device(gp));
    // mean(x): predict in original units (algorithm.rs:1158, `mean_x`)
    const int m_pad = (int)round_up(m, kTile), nt = (int)n_traj;
    std::vector<double> mean((size_t)m_pad, 0.0);
    EGX_RC(predict_impl(gp, xq, m, mean.data(), nullptr));
    CovBufs b;
    EGX_RC(cov_prepare(gp, xq, (int)m, b));
    hipStream_t st = gp->ws[0].stream;
    double max_diag = 0.0;
    if (method == EGX_SAMPLE_PSD) {  // Sigma_ii = sigma2 (1 + G_ii) as k_cov_assemble forms it
        DevBuf dg;
        EGX_RC(dg.alloc((size_t)m));
        EGX_RC(launch_gather_diag(st, b.G.p, m_pad, (int)m, dg.p));
        std::vector<double> g((size_t)m);
        EGX_HIP_CHECK(hipMemcpyAsync(g.data(), dg.p, sizeof(double) * m, hipMemcpyDeviceToHost, st));
        EGX_HIP_CHECK(hipStreamSynchronize(st));
        for (double v : g) max_diag = std::max(max_diag, gp->sigma2 * (1.0 + v));
    }
    const SampleCov c{gp->corr, b.xqT.p, gp->d, gp->d_fit_coef, gp->fit_hcols, b.G.p, gp->sigma2, max_diag, "posterior"};
    return sample_draw(st, c, (int)m, nt, method, seed, z, mean.data(), traj, tau_out);
}

}  // namespace
}  // namespace egx

extern "C" {

int32_t egx_gp_predict_covariance(egx_gp *gp, const double *xq, int64_t m, double *cov) {
    if (!gp || (m > 0 && !cov)) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::unique_lock<std::shared_mutex> lock(gp->mu);
    return covariance_impl(gp, xq, m, cov);
}

int32_t egx_gp_sample(egx_gp *gp, const double *xq, int64_t m, int64_t n_traj, int32_t method, uint64_t seed, const double *z,
                      double *traj, double *tau_out) {
    if (!gp || (m > 0 && n_traj > 0 && !traj)) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::unique_lock<std::shared_mutex> lock(gp->mu);
    return sample_impl(gp, xq, m, n_traj, method, seed, z, traj, tau_out);
}

int32_t egx_random_normals(int32_t device, uint64_t seed, int64_t m, int64_t n_traj, double *z) {
    if (m < 0 || n_traj < 0 || (m > 0 && n_traj > 0 && !z)) {
        set_error("egx_random_normals: bad arguments");
        return EGX_ERR_INVALID_VALUE;
    }
    if (m == 0 || n_traj == 0) return EGX_SUCCESS;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        set_error("egx_random_normals: no HIP device");
        return EGX_ERR_NO_DEVICE;
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= ndev) {
        set_error("egx_random_normals: device out of range");
        return EGX_ERR_INVALID_VALUE;
    }
    EGX_HIP_CHECK(hipSetDevice(device));
    DevBuf dz;
    EGX_RC(dz.alloc((size_t)m * n_traj));
    EGX_RC(launch_normals(nullptr, seed, m, n_traj, dz.p, n_traj, 1));
    EGX_HIP_CHECK(hipMemcpy(z, dz.p, sizeof(double) * (size_t)m * n_traj, hipMemcpyDeviceToHost));
    return EGX_SUCCESS;
}

}  // extern "C"
