// Predictions of a fitted sparse GP, their analytic x-gradients and trajectory sampling
// (SparseGaussianProcess::predict / predict_var / predict_gradients / predict_var_gradients / sample,
// crates/gp/src/sparse_algorithm.rs:237-362; the reference differentiates numerically, this is the closed form).
// Raw x, zero trend.  With r = r(x, z) (nz), a~ = C_z^-1 r, b~ = L^-1 a~ (U = sigma C_z, so a = sigma a~, b = sigma b~) and
// s = -1 (FITC) / +1 (VFE):
//   mean      = sigma2 r . vec
//   var_raw   = sigma2 - sigma2 (|a~|^2 + s |b~|^2),   var = max(var_raw, 1e-15) + noise
//   c         = W kx = C_z^-T (a~ + s L^-T b~)
//   d mean/dx = sigma2 sum_j vec_j dr_j/dx,   d var/dx = -2 sigma2 sum_j c_j dr_j/dx  (0 where var_raw is clamped)
// One sequence for every batch size up to the x-gradient contraction, on a grow-only workspace that lives in the handle (no
// allocation after the first call of a size, one host synchronisation per chunk of 65536 queries):
//   K(xq, z) once (launch_cross_corr), the two forward block solves (launch_trsm_rows) with their row reductions, then the
//   two TRANSPOSED solves as GEMMs with the explicit inverse factors C_z^-T and L^-T (upper triangular, cached per fitted
//   state: launch_trsm_rows on the identity's rows), the second of which leaves c transposed (nz x m_pad), the weight
//   layout of launch_xgrad; split sums, clamp mask and the factors sigma2 / -2 sigma2 on the device (k_sgp_grad_finish).
//   Up to 16 queries per call (EGO's one point at a time) end differently: the transposed solves are two memory-bound passes
//   over the same cached inverse factors (launch_uptri_gemv_rows: a GEMM of one tile of queries runs on a handful of
//   workgroups), c stays in row form, and the contraction is launch_xgrad_point, lanes over the inducing points, per query.
#include "sgp_handle.h"

using namespace egx;

namespace {

// E <- sgn * RT over `count` doubles (both (m_pad x z_pad) row-major)
__global__ __launch_bounds__(256) void k_sgp_scale_copy(const double *__restrict__ RT, double sgn, int64_t count,
                                                        double *__restrict__ E) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
    if (i + 1 < count) {
        const double2 v = *reinterpret_cast<const double2 *>(RT + i);
        *reinterpret_cast<double2 *>(E + i) = make_double2(sgn * v.x, sgn * v.y);
    } else if (i < count) {
        E[i] = sgn * RT[i];
    }
}

// out[a][k] (mc x d) = scale * sum_split part[split * s_split + a * s_query + k], summed in split order; with p2 / q2 (the
// squared norms of a~ and b~) the row of a query whose raw variance sigma2 - sigma2 (p2 + s q2) is below the clamp of
// predict_var is 0.  The variance is formed with the host's roundings (no contraction): same clamp decision as
// egx_sgp_predict_var.
__global__ __launch_bounds__(256) void k_sgp_grad_finish(const double *__restrict__ part, int nsplit, int64_t s_split,
                                                         int64_t s_query, int d, int mc, const double *__restrict__ p2,
                                                         const double *__restrict__ q2, double sigma2, int vfe, double scale,
                                                         double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)mc * d) return;
    const int a = (int)(i / d), k = (int)(i - (int64_t)a * d);
    const double *src = part + (int64_t)a * s_query + k;
    double acc = 0.0;
    for (int sp = 0; sp < nsplit; sp++) acc += src[(int64_t)sp * s_split];
    double v = scale * acc;
    if (p2) {
        const double quad = vfe ? __dmul_rn(sigma2, __dadd_rn(p2[a], q2[a])) : __dmul_rn(sigma2, __dsub_rn(p2[a], q2[a]));
        if (__dsub_rn(sigma2, quad) < 1e-15) v = 0.0;
    }
    out[i] = v;
}

// Up to this many queries per call take the few-query end of the gradient sequence (one contraction launch per query).
// Measured on an MI355X (n = 100000, Matern-5/2; few-query / batched, ms per call of value + variance gradients):
//   nz, d      m = 1          m = 4          m = 8          m = 16
//   512, 8     0.18 / 0.50    0.21 / 0.50    0.24 / 0.50    0.30 / 0.50
//   512, 32    0.24 / 1.34    0.31 / 1.34    0.41 / 1.35    0.61 / 1.35
//   2048, 8    0.70 / 1.53    0.73 / 1.54    0.78 / 1.54    0.86 / 1.54
//   2048, 32   0.77 / 2.39    0.84 / 2.39    0.96 / 2.39    1.18 / 2.39
// 16 is the largest size measured, ahead in every cell by 1.7x or more; the slopes (8 to 28 us per query) put the crossing
// between 40 and 80 queries, which was not measured.  (Builds with -DEGX_SGP_POINT_MAX=0 / =N reproduce the two columns.)
#ifndef EGX_SGP_POINT_MAX
#define EGX_SGP_POINT_MAX 16
#endif
constexpr int kSgpPointMax = EGX_SGP_POINT_MAX;

int check_sgp_query(egx_sgp *g, const double *xq, int64_t m) {
    if (!g->fitted) {
        set_error("sparse model is not fitted (call egx_sgp_finalize or egx_sgp_fit first)");
        return EGX_ERR_NOT_FITTED;
    }
    if (m < 0 || (m > 0 && !xq)) {
        set_error("bad query array");
        return EGX_ERR_INVALID_VALUE;
    }
    return EGX_SUCCESS;
}

}  // namespace

namespace egx {

int sgp_launch_scale_copy(hipStream_t s, const double *RT, double sgn, int64_t count, double *E) {
    hipLaunchKernelGGL(k_sgp_scale_copy, dim3((unsigned)((count / 2 + 255) / 256)), dim3(256), 0, s, RT, sgn, count, E);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}

// Wz <- C_z^-T, Wa <- L^-T for the resident factors; invalidated by every evaluation of the likelihood (sgp_eval)
int sgp_ensure_inverse_factors(egx_sgp *g) {
    if (g->winv_ok) return EGX_SUCCESS;
    const int z_pad = g->z_pad;
    const size_t sq = (size_t)z_pad * z_pad;
    hipStream_t s = g->stream;
    EGX_RC(g->Wz.alloc(sq));
    EGX_RC(g->Wa.alloc(sq));
    // (zeroed as a whole: launch_identity_rows leaves the tiles below the diagonal groups alone, the GEMMs read them)
    EGX_HIP_CHECK(hipMemsetAsync(g->Wz.p, 0, sizeof(double) * sq, s));
    EGX_HIP_CHECK(hipMemsetAsync(g->Wa.p, 0, sizeof(double) * sq, s));
    EGX_RC(launch_identity_rows(s, g->Wz.p, z_pad, z_pad));
    EGX_RC(launch_identity_rows(s, g->Wa.p, z_pad, z_pad));
    EGX_RC(launch_trsm_rows(s, g->Kz.p, z_pad, z_pad, g->dinv_z.p, g->Wz.p, z_pad, z_pad, 1));
    EGX_RC(launch_trsm_rows(s, g->A.p, z_pad, z_pad, g->dinv_a.p, g->Wa.p, z_pad, z_pad, 1));
    g->winv_ok = true;
    return EGX_SUCCESS;
}

int sgp_query(egx_sgp *g, const double *xq, int64_t m, double *yout, double *vout, double *gyout, double *gvout) {
    const int d = g->d, nz = g->nz, z_pad = g->z_pad;
    const bool grad = gyout || gvout, solves = vout || gvout;
    // (with KPLS weights the bound is known from egx_sgp_set_w_star on and is reported before anything else: no fit can lift it)
    if (!g->has_w) EGX_RC(check_sgp_query(g, xq, m));
    if (grad && (int64_t)d * (g->hcols + 5) > 20480) {
        set_error("x-gradients: " + std::to_string(d) + " inputs do not fit the 160 KB of LDS (d * (hcols + 5) <= 20480, hcols = " +
                  std::to_string(g->hcols) + ")");
        return EGX_ERR_UNSUPPORTED;
    }
    if (g->has_w) EGX_RC(check_sgp_query(g, xq, m));
    if (m == 0) return EGX_SUCCESS;
    hipStream_t s = g->stream;
    if (gvout) EGX_RC(sgp_ensure_inverse_factors(g));
    const int64_t cap = 65536;
    const int vfe = g->method != 0;
    const bool point = grad && m <= kSgpPointMax;  // few queries: another end of the gradient sequence (below)
    for (int64_t m0 = 0; m0 < m; m0 += cap) {
        const int mc = (int)((m - m0 < cap) ? (m - m0) : cap);
        const int m_pad = (int)round_up(mc, kTile);
        // the chunk's queries, k-major and zero padded
        g->h_x.assign((size_t)d * m_pad, 0.0);
        for (int a = 0; a < mc; a++)
            for (int k = 0; k < d; k++) g->h_x[(size_t)k * m_pad + a] = xq[(size_t)(m0 + a) * d + k];
        EGX_RC(g->q_x.alloc(g->h_x.size()));
        EGX_HIP_CHECK(hipMemcpyAsync(g->q_x.p, g->h_x.data(), sizeof(double) * g->h_x.size(), hipMemcpyHostToDevice, s));
        // every result of the chunk in one device block: mean | |a~|^2 | |b~|^2 | d mean / dx | d var / dx
        const size_t o_y = 0, o_p = m_pad, o_q = 2 * (size_t)m_pad, o_gy = 3 * (size_t)m_pad, o_gv = o_gy + (size_t)m_pad * d;
        const size_t out_sz = o_gv + (size_t)m_pad * d;
        EGX_RC(g->q_out.alloc(out_sz));
        double *dout = g->q_out.p;
        if (yout)  // Kx . vec  (:237-241), R never materialised; g->vec carries the factor sigma2
            EGX_RC(launch_predict_mean(s, g->corr, g->q_x.p, m_pad, m_pad, g->zT.p, z_pad, z_pad, d, g->coef.p, g->hcols, g->vec.p,
                                       dout + o_y));
        if (solves) {  // sigma2 - kx^T inv kx  (:245-257)
            const size_t blk = (size_t)m_pad * z_pad;
            EGX_RC(g->q_RT.alloc(blk));
            EGX_RC(launch_cross_corr(s, g->corr, g->q_x.p, m_pad, m_pad, g->zT.p, z_pad, z_pad, d, g->coef.p, g->hcols, g->q_RT.p, z_pad));
            EGX_RC(launch_trsm_rows(s, g->Kz.p, z_pad, z_pad, g->dinv_z.p, g->q_RT.p, z_pad, m_pad));  // a~ = C_z^-1 r
            EGX_RC(launch_row_reduce(s, g->q_RT.p, z_pad, m_pad, nz, nullptr, 0, 0, dout + o_p, nullptr));
            if (gvout) {  // E = sgn a~, sgn = -s: the GEMMs below subtract
                EGX_RC(g->q_E.alloc(blk));
                hipLaunchKernelGGL(k_sgp_scale_copy, dim3((unsigned)((blk / 2 + 255) / 256)), dim3(256), 0, s, g->q_RT.p,
                                   (vfe && !point) ? -1.0 : 1.0, (int64_t)blk, g->q_E.p);
                EGX_HIP_CHECK(hipGetLastError());
            }
            EGX_RC(launch_trsm_rows(s, g->A.p, z_pad, z_pad, g->dinv_a.p, g->q_RT.p, z_pad, m_pad));  // b~ = L^-1 a~
            EGX_RC(launch_row_reduce(s, g->q_RT.p, z_pad, m_pad, nz, nullptr, 0, 0, dout + o_q, nullptr));
        }
        const unsigned fin_blocks = (unsigned)(((int64_t)mc * d + 255) / 256);
        const double gv_scale = (vfe ? -2.0 : 2.0) * g->sigma2;  // d var / dx = -2 sigma2 sum c dr, the GEMMs leave -sgn c
        if (gvout && !point)  // E -= b~ (L^-T)^T: sgn (a~ + s L^-T b~), one row per query
            EGX_RC(launch_gemm_nt_sub(s, g->q_E.p, z_pad, g->q_RT.p, z_pad, g->Wa.p, z_pad, m_pad, z_pad, z_pad, 0, 0));
        if (point) {
            // few queries (EGO's one point at a time): the contraction with the lanes over the inducing points
            // (launch_xgrad_point), which wants a query's weights contiguous: c in ROW form, by two memory-bound passes over
            // the cached inverse factors instead of the GEMMs (which would run on a handful of workgroups)
            const int nblk = (nz + 255) / 256;
            EGX_RC(g->q_part.alloc((size_t)nblk * mc * d));
            if (gyout) {
                EGX_RC(launch_xgrad_point(s, g->corr, g->q_x.p, m_pad, mc, g->zT.p, z_pad, nz, d, g->coef.p, g->hcols, g->vec.p,
                                          g->q_part.p));
                hipLaunchKernelGGL(k_sgp_grad_finish, dim3(fin_blocks), dim3(256), 0, s, (const double *)g->q_part.p, nblk,
                                   (int64_t)mc * d, (int64_t)d, d, mc, (const double *)nullptr, (const double *)nullptr, g->sigma2,
                                   vfe, 1.0, dout + o_gy);
                EGX_HIP_CHECK(hipGetLastError());
            }
            if (gvout) {
                const size_t blk = (size_t)m_pad * z_pad;
                EGX_RC(g->q_Ct.alloc(blk));
                EGX_RC(launch_uptri_gemv_rows(s, g->Wa.p, z_pad, nz, g->q_RT.p, g->q_E.p, vfe ? 1.0 : -1.0, g->q_E.p, z_pad,
                                              mc));  // E = a~ + s L^-T b~
                EGX_RC(launch_uptri_gemv_rows(s, g->Wz.p, z_pad, nz, g->q_E.p, nullptr, 1.0, g->q_Ct.p, z_pad, mc));  // c
                for (int a = 0; a < mc; a++)
                    EGX_RC(launch_xgrad_point(s, g->corr, g->q_x.p + a, m_pad, 1, g->zT.p, z_pad, nz, d, g->coef.p, g->hcols,
                                              g->q_Ct.p + (size_t)a * z_pad, g->q_part.p + (size_t)a * nblk * d));
                hipLaunchKernelGGL(k_sgp_grad_finish, dim3(fin_blocks), dim3(256), 0, s, (const double *)g->q_part.p, nblk,
                                   (int64_t)d, (int64_t)nblk * d, d, mc, (const double *)(dout + o_p), (const double *)(dout + o_q),
                                   g->sigma2, vfe, -2.0 * g->sigma2, dout + o_gv);
                EGX_HIP_CHECK(hipGetLastError());
            }
        } else if (grad) {
            // enough workgroups for small batches: split the inducing points (partial sums added by k_sgp_grad_finish)
            const int nsplit = xgrad_splits(nz, m_pad);
            EGX_RC(g->q_part.alloc((size_t)nsplit * m_pad * d));
            if (gyout) {
                EGX_RC(launch_xgrad(s, g->corr, g->q_x.p, m_pad, m_pad, g->zT.p, z_pad, nz, d, g->coef.p, g->hcols, g->vec.p, 0, 1, nsplit,
                                    g->q_part.p));
                hipLaunchKernelGGL(k_sgp_grad_finish, dim3(fin_blocks), dim3(256), 0, s, (const double *)g->q_part.p, nsplit,
                                   (int64_t)m_pad * d, (int64_t)d, d, mc, (const double *)nullptr, (const double *)nullptr,
                                   g->sigma2, vfe, 1.0, dout + o_gy);
                EGX_HIP_CHECK(hipGetLastError());
            }
            if (gvout) {
                const size_t blk = (size_t)m_pad * z_pad;
                EGX_RC(g->q_Ct.alloc(blk));
                // Ct = 0 - C_z^-T E^T = -sgn c, (z_pad x m_pad): W upper triangular, the K range starts at the row tile
                EGX_HIP_CHECK(hipMemsetAsync(g->q_Ct.p, 0, sizeof(double) * blk, s));
                EGX_RC(launch_gemm_nt_sub(s, g->q_Ct.p, m_pad, g->Wz.p, z_pad, g->q_E.p, z_pad, z_pad, m_pad, z_pad, 0, 1));
                EGX_RC(launch_xgrad(s, g->corr, g->q_x.p, m_pad, m_pad, g->zT.p, z_pad, nz, d, g->coef.p, g->hcols, g->q_Ct.p, m_pad, 0,
                                    nsplit, g->q_part.p));
                hipLaunchKernelGGL(k_sgp_grad_finish, dim3(fin_blocks), dim3(256), 0, s, (const double *)g->q_part.p, nsplit,
                                   (int64_t)m_pad * d, (int64_t)d, d, mc, (const double *)(dout + o_p), (const double *)(dout + o_q),
                                   g->sigma2, vfe, gv_scale, dout + o_gv);
                EGX_HIP_CHECK(hipGetLastError());
            }
        }
        // one copy, one wait: the span of the block that holds what was asked for
        size_t lo = out_sz, hi = 0;
        auto want = [&](bool on, size_t off, size_t len) {
            if (!on) return;
            lo = std::min(lo, off);
            hi = std::max(hi, off + len);
        };
        want(yout != nullptr, o_y, mc);
        want(vout != nullptr, o_p, (size_t)m_pad + mc);
        want(gyout != nullptr, o_gy, (size_t)mc * d);
        want(gvout != nullptr, o_gv, (size_t)mc * d);
        if (g->h_out.size() < out_sz) g->h_out.resize(out_sz);
        EGX_HIP_CHECK(hipMemcpyAsync(g->h_out.data() + lo, dout + lo, sizeof(double) * (hi - lo), hipMemcpyDeviceToHost, s));
        EGX_HIP_CHECK(hipStreamSynchronize(s));
        const double *h = g->h_out.data();
        if (yout) std::memcpy(yout + m0, h + o_y, sizeof(double) * mc);
        if (vout) {
            // p = U^-1 kx = sigma C_z^-1 r  ->  |p|^2 = sigma2 |C_z^-1 r|^2, likewise q
            for (int a = 0; a < mc; a++) {
                const double p2 = h[o_p + a], q2 = h[o_q + a];
                const double quad = vfe ? g->sigma2 * (p2 + q2) : g->sigma2 * (p2 - q2);
                double var = g->sigma2 - quad;
                if (var < 1e-15) var = 1e-15;
                vout[m0 + a] = var + g->noise;
            }
        }
        if (gyout) std::memcpy(gyout + (size_t)m0 * d, h + o_gy, sizeof(double) * (size_t)mc * d);
        if (gvout) std::memcpy(gvout + (size_t)m0 * d, h + o_gv, sizeof(double) * (size_t)mc * d);
    }
    return EGX_SUCCESS;
}

}  // namespace egx

namespace {

// SparseGaussianProcess::sample (sparse_algorithm.rs:353-362) as the reference defines it: mean = predict(x), covariance =
// sigma2 r(x, x): the PRIOR covariance, without noise and without the Woodbury term.  Steps 5-8 of gp_sample.hip.
int sgp_sample(egx_sgp *g, const double *xq, int64_t m, int64_t n_traj, int method, uint64_t seed, const double *z, double *traj,
               double *tau_out) {
    EGX_RC(check_sgp_query(g, xq, m));
    if (m > (int64_t)1 << 20) {
        set_error("sample: more than 2^20 query points");
        return EGX_ERR_INVALID_VALUE;
    }
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
    const int m_pad = (int)round_up(m, kTile);
    std::vector<double> mean((size_t)m_pad, 0.0);
    EGX_RC(sgp_query(g, xq, m, mean.data(), nullptr, nullptr, nullptr));
    // (the workspace holds the queries of the last chunk only: upload all of them, k-major)
    const int d = g->d;
    g->h_x.assign((size_t)d * m_pad, 0.0);
    for (int64_t a = 0; a < m; a++)
        for (int k = 0; k < d; k++) g->h_x[(size_t)k * m_pad + a] = xq[(size_t)a * d + k];
    EGX_RC(g->q_x.alloc(g->h_x.size()));
    EGX_HIP_CHECK(hipMemcpyAsync(g->q_x.p, g->h_x.data(), sizeof(double) * g->h_x.size(), hipMemcpyHostToDevice, g->stream));
    const SampleCov c{g->corr, g->q_x.p, d, g->coef.p, g->hcols, nullptr, g->sigma2, g->sigma2, "prior"};
    return sample_draw(g->stream, c, (int)m, (int)n_traj, method, seed, z, mean.data(), traj, tau_out);
}

}  // namespace

extern "C" {

#define SGP_ENTRY(cond)                                      \
    if (!g || (m > 0 && (!xq || (cond)))) {                         \
        set_error("NULL argument");                          \
        return EGX_ERR_INVALID_VALUE;                        \
    }                                                        \
    std::lock_guard<std::mutex> lock(g->mu);                 \
    EGX_HIP_CHECK(hipSetDevice(g->device))

int32_t egx_sgp_predict(egx_sgp *g, const double *xq, int64_t m, double *y) {
    SGP_ENTRY(!y);
    return sgp_query(g, xq, m, y, nullptr, nullptr, nullptr);
}

int32_t egx_sgp_predict_var(egx_sgp *g, const double *xq, int64_t m, double *var) {
    SGP_ENTRY(!var);
    return sgp_query(g, xq, m, nullptr, var, nullptr, nullptr);
}

int32_t egx_sgp_predict_valvar(egx_sgp *g, const double *xq, int64_t m, double *y, double *var) {
    SGP_ENTRY(!y || !var);
    return sgp_query(g, xq, m, y, var, nullptr, nullptr);
}

int32_t egx_sgp_predict_gradients(egx_sgp *g, const double *xq, int64_t m, double *grad) {
    SGP_ENTRY(!grad);
    return sgp_query(g, xq, m, nullptr, nullptr, grad, nullptr);
}

int32_t egx_sgp_predict_var_gradients(egx_sgp *g, const double *xq, int64_t m, double *grad) {
    SGP_ENTRY(!grad);
    return sgp_query(g, xq, m, nullptr, nullptr, nullptr, grad);
}

int32_t egx_sgp_predict_valvar_gradients(egx_sgp *g, const double *xq, int64_t m, double *grad_y, double *grad_var) {
    SGP_ENTRY(!grad_y || !grad_var);
    return sgp_query(g, xq, m, nullptr, nullptr, grad_y, grad_var);
}

int32_t egx_sgp_sample(egx_sgp *g, const double *xq, int64_t m, int64_t n_traj, int32_t method, uint64_t seed, const double *z,
                       double *traj, double *tau_out) {
    SGP_ENTRY(n_traj > 0 && !traj);
    return sgp_sample(g, xq, m, n_traj, method, seed, z, traj, tau_out);
}
#undef SGP_ENTRY

}  // extern "C"
