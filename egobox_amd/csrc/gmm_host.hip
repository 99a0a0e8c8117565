// egx_gmm_fit: trains the Gaussian mixture of a mixture of experts on the GPU -- what egobox-moe asks of linfa-clustering with
// GaussianMixtureModel::params(n_clusters).n_runs(20).fit(..) (crates/moe/src/algorithm.rs:120-123, clustering.rs:126-130).
// The n_runs restarts are independent EM problems of one shape over the SAME data: they advance in lock-step, one E-step
// launch and one M-step launch per iteration for all of them (kernels_gmm.hip), the host reads the R lower bounds back and
// freezes the restarts that stopped.  A restart computes the same bits alone and in any batch.
// egx_gmm_fit_wide: the same training for rows up to 128 wide (kernels_gmm_wide.hip, gmm_wide_plan.h).  Both entry points are
// gmm_fit_driver with their shapes and their launch pair (GmmPath).
// ... and the fitted mixture's predict side: egx_gmx_precisions_chol (host) and egx_gmx_predict_probas(_derivatives).
#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "dev_mem.h"
#include "egx_internal.h"
#include "gmm_wide_plan.h"
#include "gmx_point.h"
#include "gp_handle.h"

using egx::set_error;

namespace {

bool all_finite(const double *p, size_t len) {
    for (size_t i = 0; i < len; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// The operands of k_gmx_probas / k_gmx_probas_deriv on `device` (< 0: the calling thread's current one): the query points and
// gmx_pack's block [means | scaled factors | par] (gaussian_mixture.rs:105-110, 253-283), one upload each.
int gmx_upload(const std::string &who, int32_t device, const double *weights, const double *means, const double *precisions_chol,
               int64_t k, int64_t d, double heaviside_factor, const double *xq, int64_t m, egx::DevBuf &d_x, egx::DevBuf &d_blk) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        set_error(who + ": no HIP device");
        return EGX_ERR_NO_DEVICE;
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= ndev) {
        set_error(who + ": device out of range");
        return EGX_ERR_INVALID_VALUE;
    }
    EGX_HIP_CHECK(hipSetDevice(device));
    const std::vector<double> blk = egx::gmx_pack(weights, means, precisions_chol, k, d, heaviside_factor);
    EGX_RC(d_x.alloc((size_t)m * d));
    EGX_RC(d_blk.alloc(blk.size()));
    EGX_HIP_CHECK(hipMemcpy(d_x.p, xq, sizeof(double) * (size_t)m * d, hipMemcpyHostToDevice));
    EGX_HIP_CHECK(hipMemcpy(d_blk.p, blk.data(), sizeof(double) * blk.size(), hipMemcpyHostToDevice));
    return EGX_SUCCESS;
}

// the typed calls' device table (mixint.h), on the device gmx_upload has selected; nothing for an untyped call
int spec_upload(const egx::MixSpec &sp, egx::DevBuf &d_spec) {
    if (sp.empty()) return EGX_SUCCESS;
    const std::vector<double> tab = sp.table();
    EGX_RC(d_spec.alloc(tab.size()));
    EGX_HIP_CHECK(hipMemcpy(d_spec.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    return EGX_SUCCESS;
}
const egx::mixint::Col *spec_ptr(const egx::MixSpec &sp, const egx::DevBuf &d_spec) {
    return sp.empty() ? nullptr : reinterpret_cast<const egx::mixint::Col *>(d_spec.p);
}

// The two trainings differ in their shapes and their launch pair only: the narrow path (kernels_gmm.hip: dim <= 36, 256-row
// tiles, 4 x 4 moment blocks on the vector unit) and the wide one (kernels_gmm_wide.hip, gmm_wide_plan.h: dim <= 128, the
// matrix unit).  fill() checks the width and sizes DP, T, tpc and the workspace before the device is touched.
struct GmmPath {
    std::string who;
    int (*fill)(const GmmPath &, int D, int k, int R, int64_t n, egx::GmmLaunch &g, size_t &part_doubles);
    int (*estep)(hipStream_t, const egx::GmmLaunch &);
    int (*mstep)(hipStream_t, const egx::GmmLaunch &, double);
    bool identity_prec;  // P before iteration 0: the identity (wide), or never read (narrow: zero)
};

int fill_narrow(const GmmPath &p, int D, int k, int R, int64_t n, egx::GmmLaunch &g, size_t &part_doubles) {
    const int DP = (D + 3) / 4 * 4;
    if (DP > egx::kGmmMaxDim || k > egx::kGmmMaxClusters) {
        set_error(p.who + ": dim <= 36 and n_clusters <= 16 expected (got dim " + std::to_string(D) + ", n_clusters " +
                  std::to_string(k) + "); egx_gmm_fit_wide takes dim <= 128");
        return EGX_ERR_INVALID_VALUE;
    }
    const int64_t T64 = (n + egx::kGmmTileRows - 1) / egx::kGmmTileRows;
    part_doubles = (size_t)T64 * R * k * egx::gmm_part_len(DP);
    if (T64 > (1 << 22) || part_doubles > ((size_t)1 << 29)) {  // (4 GiB of partial moments)
        set_error(p.who + ": n * n_runs * n_clusters * dim^2 beyond the workspace limit of 4 GiB");
        return EGX_ERR_INVALID_VALUE;
    }
    g.DP = DP;
    g.T = (int)T64;
    return EGX_SUCCESS;
}

int fill_wide(const GmmPath &p, int D, int k, int R, int64_t n, egx::GmmLaunch &g, size_t &part_doubles) {
    namespace W = egx::gmm_wide;
    if (D > W::kMaxDim || k > egx::kGmmMaxClusters) {
        set_error(p.who + ": dim <= 128 and n_clusters <= 16 expected (got dim " + std::to_string(D) + ", n_clusters " +
                  std::to_string(k) + ")");
        return EGX_ERR_INVALID_VALUE;
    }
    const W::Plan pl = W::plan(n, D);
    if (pl.tiles > ((int64_t)1 << 30) || !W::workspace_doubles(pl, R, k, part_doubles)) {
        set_error(p.who + ": n_runs * n_clusters * dim^2 beyond the workspace limit of 4 GiB");
        return EGX_ERR_INVALID_VALUE;
    }
    g.DP = pl.DP;
    g.T = (int)pl.chunks;
    g.tpc = (int)pl.tiles_per_chunk;
    return EGX_SUCCESS;
}

// Validation, the uploads, the round loop (the live mask up, an E-step and an M-step launch, the R lower bounds and flags
// back, the stopped restarts frozen), the best run and the all-failed error: one text for both entry points.
int gmm_fit_driver(const GmmPath &path, const egx_gmm_config *cfg, const double *data, int64_t n, int32_t dim,
                   const double *init_means, double *weights, double *means, double *covariances, double *lower_bounds,
                   int32_t *n_iters, int32_t *statuses, int32_t *best_run, double *all_weights, double *all_means,
                   double *all_covariances) {
    const std::string &who = path.who;
    if (!cfg || !data || !init_means || !weights || !means || !covariances || !lower_bounds || !n_iters || !statuses || !best_run) {
        set_error(who + ": NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    const int k = cfg->n_clusters, R = cfg->n_runs, D = dim;
    if (k < 1 || D < 1 || n < k || R < 1 || cfg->max_iter < 1 || !(cfg->tol >= 0.0) || !(cfg->reg_covar >= 0.0) ||
        !std::isfinite(cfg->reg_covar)) {
        set_error(who + ": n >= n_clusters >= 1, dim >= 1, n_runs >= 1, max_iter >= 1, tol >= 0 and reg_covar >= 0 expected");
        return EGX_ERR_INVALID_VALUE;
    }
    egx::GmmLaunch g;
    size_t part_doubles = 0;
    EGX_RC(path.fill(path, D, k, R, n, g, part_doubles));
    const int DP = g.DP;
    const int64_t T64 = g.T;
    if (!all_finite(data, (size_t)n * D) || !all_finite(init_means, (size_t)R * k * D)) {
        set_error(who + ": data and init_means must be finite");
        return EGX_ERR_INVALID_VALUE;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        set_error(who + ": no HIP device");
        return EGX_ERR_NO_DEVICE;
    }
    int device = cfg->device;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;  // the calling thread's current device
    if (device >= ndev) {
        set_error(who + ": device out of range");
        return EGX_ERR_INVALID_VALUE;
    }
    EGX_HIP_CHECK(hipSetDevice(device));

    const size_t rk = (size_t)R * k;
    egx::DevBuf d_data, d_means, d_prec, d_cst, d_w, d_cov, d_part, d_lpn, d_lbst;
    egx::DevMem<int> d_active;
    EGX_RC(d_data.alloc((size_t)n * D));
    EGX_RC(d_means.alloc(rk * DP));
    EGX_RC(d_prec.alloc(rk * DP * DP));
    EGX_RC(d_cst.alloc(rk));
    EGX_RC(d_w.alloc(rk));
    EGX_RC(d_cov.alloc(rk * D * D));
    EGX_RC(d_part.alloc(part_doubles));
    EGX_RC(d_lpn.alloc((size_t)T64 * R));
    EGX_RC(d_lbst.alloc(2 * (size_t)R));
    EGX_RC(d_active.alloc(R));
    std::vector<double> h_means(rk * DP, 0.0);
    for (size_t i = 0; i < rk; i++)
        for (int j = 0; j < D; j++) h_means[i * DP + j] = init_means[i * D + j];
    EGX_HIP_CHECK(hipMemcpy(d_data.p, data, sizeof(double) * (size_t)n * D, hipMemcpyHostToDevice));
    EGX_HIP_CHECK(hipMemcpy(d_means.p, h_means.data(), sizeof(double) * h_means.size(), hipMemcpyHostToDevice));
    if (path.identity_prec) {
        std::vector<double> h_prec(rk * DP * DP, 0.0);
        for (size_t i = 0; i < rk; i++)
            for (int j = 0; j < DP; j++) h_prec[(i * DP + j) * DP + j] = 1.0;
        EGX_HIP_CHECK(hipMemcpy(d_prec.p, h_prec.data(), sizeof(double) * h_prec.size(), hipMemcpyHostToDevice));
    } else {
        EGX_HIP_CHECK(hipMemset(d_prec.p, 0, sizeof(double) * rk * DP * DP));
    }
    EGX_HIP_CHECK(hipMemset(d_cst.p, 0, sizeof(double) * rk));
    EGX_HIP_CHECK(hipMemset(d_lbst.p, 0, sizeof(double) * 2 * R));

    g.data = d_data.p;
    g.n = n;
    g.D = D;
    g.k = k;
    g.R = R;
    // enough workgroups to fill the chip when the data has few tiles: the restarts are dealt over grid.y (a restart's
    // arithmetic does not depend on the deal)
    g.rsplit = (int)std::min<int64_t>(R, std::max<int64_t>(1, (1024 + T64 - 1) / T64));
    g.active = d_active.p;
    g.means = d_means.p;
    g.prec = d_prec.p;
    g.cst = d_cst.p;
    g.weights = d_w.p;
    g.covs = d_cov.p;
    g.part = d_part.p;
    g.lpn_part = d_lpn.p;
    g.lbst = d_lbst.p;

    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<int> active(R, 1);
    std::vector<double> h_lbst(2 * (size_t)R), prev(R, -std::numeric_limits<double>::infinity());
    int n_active = R;
    for (int r = 0; r < R; r++) {
        statuses[r] = 1;
        n_iters[r] = 0;
        lower_bounds[r] = nan;
    }
    for (int it = 0; it <= cfg->max_iter && n_active > 0; it++) {
        g.init = it == 0;
        EGX_HIP_CHECK(hipMemcpy(d_active.p, active.data(), sizeof(int) * R, hipMemcpyHostToDevice));
        EGX_RC(path.estep(nullptr, g));
        EGX_RC(path.mstep(nullptr, g, cfg->reg_covar));
        EGX_HIP_CHECK(hipMemcpy(h_lbst.data(), d_lbst.p, sizeof(double) * 2 * R, hipMemcpyDeviceToHost));
        for (int r = 0; r < R; r++) {
            if (!active[r]) continue;
            n_iters[r] = it;
            const double lb = h_lbst[r];
            bool stop = false;
            if (h_lbst[(size_t)R + r] != 0.0 || (it > 0 && !std::isfinite(lb))) {
                statuses[r] = 2;
                lower_bounds[r] = nan;
                stop = true;
            } else if (it > 0) {
                lower_bounds[r] = lb;
                if (std::fabs(lb - prev[r]) < cfg->tol) {
                    statuses[r] = 0;
                    stop = true;
                }
                prev[r] = lb;
            }
            if (stop) {
                active[r] = 0;
                n_active--;
            }
        }
    }
    int best = -1;
    for (int r = 0; r < R; r++)
        if (statuses[r] != 2 && (best < 0 || lower_bounds[r] > lower_bounds[best])) best = r;
    *best_run = best;
    std::vector<double> h_w(rk), h_cov(rk * D * D);
    EGX_HIP_CHECK(hipMemcpy(h_w.data(), d_w.p, sizeof(double) * rk, hipMemcpyDeviceToHost));
    EGX_HIP_CHECK(hipMemcpy(h_means.data(), d_means.p, sizeof(double) * h_means.size(), hipMemcpyDeviceToHost));
    EGX_HIP_CHECK(hipMemcpy(h_cov.data(), d_cov.p, sizeof(double) * h_cov.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < rk; i++) {
        if (all_weights) all_weights[i] = h_w[i];
        if (all_means)
            for (int j = 0; j < D; j++) all_means[i * D + j] = h_means[i * DP + j];
    }
    if (all_covariances) std::copy(h_cov.begin(), h_cov.end(), all_covariances);
    if (best < 0) {
        set_error(who + ": every restart failed (a covariance that is not positive definite, or a value that is not finite)");
        return EGX_ERR_LINALG;
    }
    for (int c = 0; c < k; c++) {
        const size_t i = (size_t)best * k + c;
        weights[c] = h_w[i];
        for (int j = 0; j < D; j++) means[(size_t)c * D + j] = h_means[i * DP + j];
        std::copy(h_cov.begin() + i * D * D, h_cov.begin() + (i + 1) * D * D, covariances + (size_t)c * D * D);
    }
    return EGX_SUCCESS;
}

}  // namespace

extern "C" {

void egx_gmm_config_default(egx_gmm_config *cfg) {
    if (!cfg) return;
    cfg->n_clusters = 1;
    cfg->n_runs = 20;  // crates/moe/src/algorithm.rs:121
    cfg->max_iter = 100;
    cfg->device = -1;
    cfg->tol = 1e-3;
    cfg->reg_covar = 1e-6;
}

int32_t egx_gmm_fit(const egx_gmm_config *cfg, const double *data, int64_t n, int32_t dim, const double *init_means,
                    double *weights, double *means, double *covariances, double *lower_bounds, int32_t *n_iters,
                    int32_t *statuses, int32_t *best_run, double *all_weights, double *all_means, double *all_covariances) {
    static const GmmPath narrow{"egx_gmm_fit", fill_narrow, egx::launch_gmm_estep, egx::launch_gmm_mstep, false};
    return gmm_fit_driver(narrow, cfg, data, n, dim, init_means, weights, means, covariances, lower_bounds, n_iters, statuses,
                          best_run, all_weights, all_means, all_covariances);
}

int32_t egx_gmm_fit_wide(const egx_gmm_config *cfg, const double *data, int64_t n, int32_t dim, const double *init_means,
                         double *weights, double *means, double *covariances, double *lower_bounds, int32_t *n_iters,
                         int32_t *statuses, int32_t *best_run, double *all_weights, double *all_means,
                         double *all_covariances) {
    static const GmmPath wide{"egx_gmm_fit_wide", fill_wide, egx::launch_gmm_estep_wide, egx::launch_gmm_mstep_wide, true};
    return gmm_fit_driver(wide, cfg, data, n, dim, init_means, weights, means, covariances, lower_bounds, n_iters, statuses,
                          best_run, all_weights, all_means, all_covariances);
}

// ---- Gaussian mixture responsibilities ----------------------------------------------------------
// precisions_chol[c] = (chol(cov_c)^-1)^T, crates/moe/src/gaussian_mixture.rs:182-205: d x d host arithmetic.
int32_t egx_gmx_precisions_chol(const double *covariances, int64_t k, int64_t d, double *precisions_chol) {
    if (!covariances || !precisions_chol || k < 1 || d < 1) {
        set_error("egx_gmx_precisions_chol: bad arguments");
        return EGX_ERR_INVALID_VALUE;
    }
    std::vector<double> L((size_t)d * d), Li((size_t)d * d);
    for (int64_t c = 0; c < k; c++) {
        const double *A = covariances + (size_t)c * d * d;
        std::fill(L.begin(), L.end(), 0.0);
        for (int64_t j = 0; j < d; j++) {  // lower Cholesky factor, column by column
            double dj = A[j * d + j];
            for (int64_t l = 0; l < j; l++) dj -= L[j * d + l] * L[j * d + l];
            if (!(dj > 0.0) || !std::isfinite(dj)) {
                set_error("egx_gmx_precisions_chol: covariance " + std::to_string((long long)c) + " is not positive definite");
                return EGX_ERR_LINALG;
            }
            L[j * d + j] = std::sqrt(dj);
            for (int64_t i = j + 1; i < d; i++) {
                double v = A[i * d + j];
                for (int64_t l = 0; l < j; l++) v -= L[i * d + l] * L[j * d + l];
                L[i * d + j] = v / L[j * d + j];
            }
        }
        std::fill(Li.begin(), Li.end(), 0.0);  // L^-1 by forward substitution on the identity
        for (int64_t col = 0; col < d; col++)
            for (int64_t i = col; i < d; i++) {
                double v = (i == col) ? 1.0 : 0.0;
                for (int64_t l = col; l < i; l++) v -= L[i * d + l] * Li[l * d + col];
                Li[i * d + col] = v / L[i * d + i];
            }
        double *out = precisions_chol + (size_t)c * d * d;
        for (int64_t i = 0; i < d; i++)
            for (int64_t j = 0; j < d; j++) out[i * d + j] = Li[j * d + i];  // transposed: upper triangular
    }
    return EGX_SUCCESS;
}

int32_t egx_gmx_predict_probas(int32_t device, const double *weights, const double *means, const double *precisions_chol,
                               int64_t k, int64_t d, double heaviside_factor, const double *xq, int64_t m, double *probas) {
    return egx_gmx_predict_probas_mixint(device, weights, means, precisions_chol, k, d, heaviside_factor, xq, m, probas, nullptr, 0);
}

int32_t egx_gmx_predict_probas_mixint(int32_t device, const double *weights, const double *means, const double *precisions_chol,
                                      int64_t k, int64_t d, double heaviside_factor, const double *xq, int64_t m, double *probas,
                                      const egx_xtype *xt, int32_t nx) {
    if (!weights || !means || !precisions_chol || k < 1 || d < 1 || d > 4096 || m < 0 || (m > 0 && (!xq || !probas)) ||
        !(heaviside_factor > 0.0)) {
        set_error("egx_gmx_predict_probas: bad arguments");
        return EGX_ERR_INVALID_VALUE;
    }
    egx::MixSpec sp;
    if (nx != 0) EGX_RC(egx::mixspec_build("egx_gmx_predict_probas_mixint", xt, nx, d, sp));
    if (m == 0) return EGX_SUCCESS;
    if (k == 1) {  // gaussian_mixture.rs:115-116
        for (int64_t a = 0; a < m; a++) probas[a] = 1.0;
        return EGX_SUCCESS;
    }
    egx::DevBuf d_x, d_blk, d_out, d_spec;
    EGX_RC(gmx_upload("egx_gmx_predict_probas", device, weights, means, precisions_chol, k, d, heaviside_factor, xq, m, d_x, d_blk));
    EGX_RC(spec_upload(sp, d_spec));
    EGX_RC(d_out.alloc((size_t)m * k));
    const size_t lds = sizeof(double) * 64 * (size_t)(d | 1);
    if (lds > 160 * 1024) {
        set_error("egx_gmx_predict_probas: d too large for one workgroup's LDS");
        return EGX_ERR_INVALID_VALUE;
    }
    EGX_RC(egx::launch_gmx_probas(false, d_x.p, m, (int)d, (int)k, d_blk.p, lds, d_out.p, spec_ptr(sp, d_spec)));
    EGX_HIP_CHECK(hipMemcpy(probas, d_out.p, sizeof(double) * (size_t)m * k, hipMemcpyDeviceToHost));
    return EGX_SUCCESS;
}

int32_t egx_gmx_predict_probas_derivatives(int32_t device, const double *weights, const double *means,
                                           const double *precisions_chol, int64_t k, int64_t d, double heaviside_factor,
                                           const double *xq, int64_t m, double *dprobas) {
    return egx_gmx_predict_probas_derivatives_mixint(device, weights, means, precisions_chol, k, d, heaviside_factor, xq, m, dprobas,
                                                     nullptr, 0);
}

int32_t egx_gmx_predict_probas_derivatives_mixint(int32_t device, const double *weights, const double *means,
                                                  const double *precisions_chol, int64_t k, int64_t d, double heaviside_factor,
                                                  const double *xq, int64_t m, double *dprobas, const egx_xtype *xt, int32_t nx) {
    if (!weights || !means || !precisions_chol || k < 1 || d < 1 || m < 0 || (m > 0 && (!xq || !dprobas)) ||
        !(heaviside_factor > 0.0)) {
        set_error("egx_gmx_predict_probas_derivatives: bad arguments");
        return EGX_ERR_INVALID_VALUE;
    }
    egx::MixSpec sp;
    if (nx != 0) EGX_RC(egx::mixspec_build("egx_gmx_predict_probas_derivatives_mixint", xt, nx, d, sp));
    if (m == 0) return EGX_SUCCESS;
    const size_t lds = sizeof(double) * 64 * (size_t)(3 * (d | 1) + (k | 1));
    if (lds > 160 * 1024) {
        set_error("egx_gmx_predict_probas_derivatives: d / k too large for one workgroup's LDS (3 d + k <= 320)");
        return EGX_ERR_INVALID_VALUE;
    }
    egx::DevBuf d_x, d_blk, d_out, d_spec;
    EGX_RC(gmx_upload("egx_gmx_predict_probas_derivatives", device, weights, means, precisions_chol, k, d, heaviside_factor, xq, m,
                      d_x, d_blk));
    EGX_RC(spec_upload(sp, d_spec));
    EGX_RC(d_out.alloc((size_t)m * k * d));
    EGX_RC(egx::launch_gmx_probas(true, d_x.p, m, (int)d, (int)k, d_blk.p, lds, d_out.p, spec_ptr(sp, d_spec)));
    EGX_HIP_CHECK(hipMemcpy(dprobas, d_out.p, sizeof(double) * (size_t)m * k * d, hipMemcpyDeviceToHost));
    return EGX_SUCCESS;
}

}  // extern "C"
