// Sparse Gaussian process (FITC / VFE) on gfx950 -- SURVEY 8f rank 4, the reference's own large-n model:
//   SgpValidParams::reduced_likelihood / fitc / vfe   crates/gp/src/sparse_algorithm.rs:654-831
//   SparseGaussianProcess::predict / predict_var       crates/gp/src/sparse_algorithm.rs:237-257
//   SgpValidParams::fit (objective, parameter layout)  crates/gp/src/sparse_algorithm.rs:422-650
// n training points, nz << n inducing points; everything O(n nz^2) runs on the kernels of the dense path:
//   R_nz                     k_cross_corr (rows = training points, columns = inducing points; raw x, no normalisation)
//   Kmm = sigma2 (R_zz + nugget/sigma2 I) = U U^T, U = sigma C_z      k_corr_sym + launch_potrf
//   V^T = sigma R_nz C_z^-T  (n x nz rows)                            launch_trsm_rows
//   nu_t = sigma2 (1 - |v~_t|^2) + noise                              k_row_reduce
//   G = V diag(beta) V^T, V (beta o y), y^T diag(beta) y              ONE NT GEMM on the transposed, scaled and
//                                                                     y-augmented copy W = [sigma V~ sqrt(beta); sqrt(beta) y]
//   A = I + G = L L^T,  b = L^-1 V (beta o y)                         launch_potrf with the right-hand side riding below A
// The Woodbury matrix of the reference (nz x nz inverses) is never formed for predictions:
//   kx^T Kmm^-1 kx = |U^-1 kx|^2,   kx^T U^-T (L L^T)^-1 U^-1 kx = |L^-1 U^-1 kx|^2   (two launch_trsm_rows + k_row_reduce)
// Predictions, their x-gradients and sampling: sgp_predict.hip.  The likelihood's closed-form gradient: sgp_grad.hip (its entry
// points, egx_sgp_likelihood_grad and egx_sgp_fit_lbfgs, are here beside the evaluation they extend, and so are those of the
// gradient in the inducing points: egx_sgp_likelihood_grad_z, egx_sgp_set_inducings / _get_inducings, egx_sgp_fit_lbfgs_z).
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <vector>

#include "sgp_handle.h"  // (gp_handle.h: fit_starts.h with the optimisers' machines and the rules of a multistart fit)
#include "kpls_coef.h"

using namespace egx;

namespace {

// W[i][t] = scale * sb[t] * RT[t][i]  (i < nz, t < n), row z_pad: W[z_pad][t] = sb[t] * y[t]; everything else 0.
// RT is (n_pad x z_pad) row-major, W is (zext x n_pad) row-major; 32x32 LDS transpose tiles.
__global__ __launch_bounds__(256) void k_sgp_transpose_scale(const double *__restrict__ RT, int z_pad, int n, int nz,
                                                             const double *__restrict__ sb, const double *__restrict__ y,
                                                             double scale, double *__restrict__ W, int n_pad) {
    __shared__ double tile[32][33];
    const int t0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    if (i0 < z_pad) {
        for (int r = ty; r < 32; r += 8) {
            const int t = t0 + r, i = i0 + tx;
            tile[r][tx] = (t < n && i < nz) ? RT[(int64_t)t * z_pad + i] * sb[t] * scale : 0.0;
        }
        __syncthreads();
        for (int r = ty; r < 32; r += 8) W[(int64_t)(i0 + r) * n_pad + t0 + tx] = tile[tx][r];
    } else {  // augmented block of 128 rows: only its first row carries data
        for (int r = ty; r < 32; r += 8) {
            const int i = i0 + r, t = t0 + tx;
            W[(int64_t)i * n_pad + t] = (i == z_pad && t < n) ? sb[t] * y[t] : 0.0;
        }
    }
}

// sb[t] = sqrt(beta_t): FITC beta_t = 1 / (sigma2 (1 - s0_t) + noise), VFE beta = 1 / max(noise, nugget)
__global__ void k_sgp_sqrt_beta(const double *__restrict__ s0, int n, double sigma2, double noise, double nugget,
                                int vfe, double *__restrict__ sb) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double nu = vfe ? fmax(noise, nugget) : sigma2 * (1.0 - s0[t]) + noise;
    sb[t] = (nu > 0.0) ? sqrt(1.0 / nu) : 0.0;  // nu <= 0 is reported by the host from s0
}

// A (zext rows x z_pad cols, ld = z_pad): lower part of I - Gneg for the first z_pad rows, rhs = -Gneg[z_pad][.] in row
// z_pad, zeros below.  Gneg is (zext x zext) with the LOWER tiles valid.
__global__ void k_sgp_form_a(const double *__restrict__ Gneg, int zext, int z_pad, double *__restrict__ A) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= z_pad) return;
    double v = 0.0;
    if (i < z_pad) {
        if (j <= i) v = ((i == j) ? 1.0 : 0.0) - Gneg[(int64_t)i * zext + j];
    } else if (i == z_pad) {
        v = -Gneg[(int64_t)i * zext + j];
    }
    A[(int64_t)i * z_pad + j] = v;
}

struct Eval {
    double lkh = -std::numeric_limits<double>::infinity();
    int status = EGX_STATUS_OK;
};

int sgp_eval(egx_sgp *g, const double *theta, int64_t theta_len, double sigma2, double noise, Eval &out, bool keep) {
    const int n = g->n, d = g->d, nz = g->nz, n_pad = g->n_pad, z_pad = g->z_pad, zext = g->zext;
    out = Eval();
    const int h = g->h;  // theta components: d, or the columns of the KPLS weights
    if (theta_len != 1 && theta_len != h) {
        set_error(std::string("theta should be either 1-dim or dim of xtrain") + (g->has_w ? " (w_star.ncols())" : "") + ", got " +
                  std::to_string(theta_len));
        return EGX_ERR_INVALID_VALUE;
    }
    std::vector<double> th(h);
    bool bad = !(sigma2 > 0.0) || !(noise >= 0.0) || !std::isfinite(sigma2) || !std::isfinite(noise);
    for (int k = 0; k < h; k++) {
        th[k] = theta[theta_len == 1 ? 0 : k];
        if (std::isnan(th[k])) bad = true;
    }
    if (bad) {  // sparse_algorithm.rs:521-527: NaN parameters are the worst value
        out.status = EGX_STATUS_NAN_THETA;
        return EGX_SUCCESS;
    }
    hipStream_t s = g->stream;
    const double sigma = std::sqrt(sigma2);
    g->fitted = false;  // the resident factors are about to be overwritten; set again below when `keep`
    g->winv_ok = false;  // ... and with them the cached inverse factors of the x-gradients (sgp_predict.hip)
    // the coefficient table (kpls_coef.h): theta itself without weights, d x hcols with them
    const int hcols = g->hcols = kpls::coef_table(g->corr, d, h, g->w_ptr(), th.data(), g->coef_host);
    g->th_full = th;
    EGX_HIP_CHECK(hipMemcpyAsync(g->coef.p, g->coef_host.data(), sizeof(double) * g->coef_host.size(), hipMemcpyHostToDevice, s));
    EGX_HIP_CHECK(hipStreamSynchronize(s));
    EGX_HIP_CHECK(hipMemsetAsync(g->d_info, 0, 2 * sizeof(int), s));
    // Kmm / sigma2 = R_zz + (nugget / sigma2) I  -> C_z
    int rc = launch_corr_sym(s, g->corr, g->zT.p, z_pad, nz, d, g->coef.p, hcols, g->nugget / sigma2, g->Kz.p, z_pad, z_pad);
    if (rc) return rc;
    rc = launch_potrf(s, g->Kz.p, z_pad, z_pad, z_pad, g->dinv_z.p, g->d_info);
    if (rc) return rc;
    // R_nz, then V~^T = R_nz C_z^-T
    rc = launch_cross_corr(s, g->corr, g->xT.p, n_pad, n_pad, g->zT.p, z_pad, z_pad, d, g->coef.p, hcols, g->RT.p, z_pad);
    if (rc) return rc;
    rc = launch_trsm_rows(s, g->Kz.p, z_pad, z_pad, g->dinv_z.p, g->RT.p, z_pad, n_pad);
    if (rc) return rc;
    rc = launch_row_reduce(s, g->RT.p, z_pad, n_pad, nz, nullptr, 0, 0, g->s0.p, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sgp_sqrt_beta, dim3((n + 255) / 256), dim3(256), 0, s, g->s0.p, n, sigma2, noise, g->nugget,
                       g->method, g->sb.p);
    hipLaunchKernelGGL(k_sgp_transpose_scale, dim3(n_pad / 32, zext / 32), dim3(256), 0, s, g->RT.p, z_pad, n, nz, g->sb.p,
                       g->y.p, sigma, g->W.p, n_pad);
    // Gneg = 0 - W W^T (lower tiles): G, V (beta o y) in row z_pad, y^T diag(beta) y in the corner
    rc = launch_gram_lower(s, g->W.p, n_pad, zext, n_pad, g->G.p, zext, g->P.p);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sgp_form_a, dim3((z_pad + 255) / 256, zext), dim3(256), 0, s, g->G.p, zext, z_pad, g->A.p);
    rc = launch_potrf(s, g->A.p, z_pad, z_pad, zext, g->dinv_a.p, g->d_info + 1);
    if (rc) return rc;
    rc = launch_gather_diag(s, g->A.p, z_pad, z_pad, g->diag.p);
    if (rc) return rc;
    std::vector<double> s0(n), diag(z_pad), brow(z_pad);
    double corner = 0.0;
    int info[2] = {0, 0};
    EGX_HIP_CHECK(hipMemcpyAsync(s0.data(), g->s0.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    EGX_HIP_CHECK(hipMemcpyAsync(diag.data(), g->diag.p, sizeof(double) * z_pad, hipMemcpyDeviceToHost, s));
    EGX_HIP_CHECK(hipMemcpyAsync(brow.data(), g->A.p + (size_t)z_pad * z_pad, sizeof(double) * z_pad, hipMemcpyDeviceToHost, s));
    EGX_HIP_CHECK(hipMemcpyAsync(&corner, g->G.p + (size_t)z_pad * zext + z_pad, sizeof(double), hipMemcpyDeviceToHost, s));
    EGX_HIP_CHECK(hipMemcpyAsync(info, g->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    EGX_HIP_CHECK(hipStreamSynchronize(s));
    if (info[0] != 0 || info[1] != 0) {  // the reference unwraps (panics); the objective wrapper turns it into +inf
        out.status = EGX_STATUS_NOT_POSITIVE_DEFINITE;
        return EGX_SUCCESS;
    }
    double term2 = 0.0, bb = 0.0;
    for (int i = 0; i < nz; i++) {
        term2 += 2.0 * std::log(diag[i]);
        bb += brow[i] * brow[i];
    }
    const double term3 = -corner;  // Gneg corner = -(y^T diag(beta) y)
    double lkh;
    if (g->method == 0) {  // FITC  sparse_algorithm.rs:747-754
        double term1 = 0.0;
        for (int t = 0; t < n; t++) {
            const double nu = sigma2 * (1.0 - s0[t]) + noise;
            if (!(nu > 0.0)) {
                out.status = EGX_STATUS_NOT_POSITIVE_DEFINITE;
                return EGX_SUCCESS;
            }
            term1 += std::log(nu);
        }
        lkh = -0.5 * (term1 + term2 + term3 - bb);
    } else {  // VFE  :813-821
        const double beta = 1.0 / std::fmax(noise, g->nugget);
        double tr = 0.0;
        for (int t = 0; t < n; t++) tr += s0[t];
        lkh = -0.5 * (-(double)n * std::log(beta) + term2 + term3 - bb + (double)n * beta * sigma2 - beta * sigma2 * tr);
    }
    if (std::isnan(lkh)) {
        out.status = EGX_STATUS_NAN_THETA;
        return EGX_SUCCESS;
    }
    out.lkh = lkh;
    if (keep) {
        // vec = U^-T L^-T b = (1 / sigma) C_z^-T (L^-T b): two backward substitutions with the resident factors
        std::vector<double> tmp(z_pad, 0.0);
        for (int i = 0; i < nz; i++) tmp[i] = brow[i];
        EGX_HIP_CHECK(hipMemcpyAsync(g->tmpv.p, tmp.data(), sizeof(double) * z_pad, hipMemcpyHostToDevice, s));
        rc = launch_block_inverse(s, g->A.p, z_pad, z_pad, g->dinv_a.p, g->wall.p);
        if (rc) return rc;
        rc = launch_trsv_t(s, g->A.p, z_pad, z_pad, g->wall.p, g->tmpv.p, g->vec.p, true);  // (a few blocks: launch per block)
        if (rc) return rc;
        EGX_HIP_CHECK(hipMemcpyAsync(g->tmpv.p, g->vec.p, sizeof(double) * z_pad, hipMemcpyDeviceToDevice, s));
        rc = launch_block_inverse(s, g->Kz.p, z_pad, z_pad, g->dinv_z.p, g->wall.p);
        if (rc) return rc;
        rc = launch_trsv_t(s, g->Kz.p, z_pad, z_pad, g->wall.p, g->tmpv.p, g->vec.p, true);
        if (rc) return rc;
        g->w_vec.assign(z_pad, 0.0);
        EGX_HIP_CHECK(hipMemcpyAsync(g->w_vec.data(), g->vec.p, sizeof(double) * z_pad, hipMemcpyDeviceToHost, s));
        EGX_HIP_CHECK(hipStreamSynchronize(s));
        for (int i = 0; i < z_pad; i++) g->w_vec[i] = (i < nz) ? g->w_vec[i] / sigma : 0.0;
        // sigma2 * vec is what the mean kernel contracts with R(x, z): predict = sigma2 R . vec
        std::vector<double> sv(z_pad);
        for (int i = 0; i < z_pad; i++) sv[i] = sigma2 * g->w_vec[i];
        EGX_HIP_CHECK(hipMemcpyAsync(g->vec.p, sv.data(), sizeof(double) * z_pad, hipMemcpyHostToDevice, s));
        EGX_HIP_CHECK(hipStreamSynchronize(s));
        g->theta = th;
        g->sigma2 = sigma2;
        g->noise = noise;
        g->likelihood = lkh;
        g->fitted = true;
    }
    return EGX_SUCCESS;
}

// The end of a fit: the keeping evaluation at the best start's point x = log10(params); nullptr: no start ended finite
int sgp_fit_keep(egx_sgp *g, const StartResult *best, int estimate_noise, double noise_fixed) {
    const int d = g->h;  // theta components
    if (!best) {
        set_error("sparse GP: no start point gave a finite likelihood");
        return EGX_ERR_LIKELIHOOD;
    }
    const std::vector<double> &best_x = best->x;
    std::vector<double> th(d);
    for (int i = 0; i < d; i++) th[i] = std::pow(10.0, best_x[i]);
    Eval ev;
    const int rc = sgp_eval(g, th.data(), d, std::pow(10.0, best_x[d]),
                            estimate_noise ? std::pow(10.0, best_x[d + 1]) : noise_fixed, ev, true);
    if (rc) return rc;
    if (ev.status != EGX_STATUS_OK) {
        set_error("sparse GP: final evaluation failed");
        return EGX_ERR_LINALG;
    }
    return EGX_SUCCESS;
}

// f(x) = -L(10^x) and its gradient in x = log10(params) for the L-BFGS machine: g_x = -p ln10 dL/dp, the noise component
// dropped when the noise is fixed.  A failed evaluation is f = +inf with a zero gradient.
int sgp_eval_grad_x(egx_sgp *g, const std::vector<double> &xv, int estimate_noise, double noise_fixed, double &f,
                    std::vector<double> &gx) {
    const int d = g->h, np = d + 1 + (estimate_noise ? 1 : 0);  // d: theta components
    std::vector<double> prm(d + 2), grad(d + 2, 0.0);
    for (int i = 0; i <= d; i++) prm[i] = std::pow(10.0, xv[i]);
    prm[d + 1] = estimate_noise ? std::pow(10.0, xv[d + 1]) : noise_fixed;
    Eval ev;
    EGX_RC(sgp_eval(g, prm.data(), d, prm[d], prm[d + 1], ev, false));
    f = std::numeric_limits<double>::infinity();
    gx.assign(np, 0.0);
    if (ev.status != EGX_STATUS_OK) return EGX_SUCCESS;
    EGX_RC(sgp_grad_tail(g, prm[d], prm[d + 1], grad.data()));
    f = -ev.lkh;
    const double ln10 = std::log(10.0);
    for (int i = 0; i < np; i++) gx[i] = -prm[i] * ln10 * grad[i];
    for (int i = 0; i < np; i++)
        if (!std::isfinite(gx[i])) {
            f = std::numeric_limits<double>::infinity();
            gx.assign(np, 0.0);
            break;
        }
    return EGX_SUCCESS;
}

// One L-BFGS machine after the other (fit_starts.h run_sequential: the handle has ONE workspace, and sgp_grad_tail reads what
// sgp_eval of the same point left in it), each point through eval(x, f, gx) -> rc.  results: (f, x) per machine; evals grows by
// the points asked.
template <class EvalGrad>
int sgp_lbfgs_run(std::vector<LbfgsStart> &mach, EvalGrad &&eval, std::vector<StartResult> &results, int64_t &evals) {
    double f = 0.0;
    std::vector<double> gx;
    int rc;
    fit::run_sequential(
        mach,
        [&](const multistart::Round &r) {
            evals++;
            return eval(r.pts, f, gx);
        },
        [&](const multistart::Round &, size_t, LbfgsStart &m) { m.tell(f, gx); }, rc);
    EGX_RC(rc);
    for (const LbfgsStart &m : mach) results.push_back(StartResult{m.f, m.x, 0});
    return EGX_SUCCESS;
}

// zT <- z (nz x d row-major; k-major and padded as at creation).  The resident factors belong to the old points: the handle is
// un-fitted and the cached inverse factors are dropped.
int sgp_upload_z(egx_sgp *g, const double *z) {
    const int d = g->d, nz = g->nz;
    const size_t zp = g->z_pad;
    std::vector<double> zT((size_t)d * zp, 0.0);
    for (int i = 0; i < nz; i++)
        for (int k = 0; k < d; k++) zT[(size_t)k * zp + i] = z[(size_t)i * d + k];
    EGX_HIP_CHECK(hipMemcpyAsync(g->zT.p, zT.data(), sizeof(double) * zT.size(), hipMemcpyHostToDevice, g->stream));
    EGX_HIP_CHECK(hipStreamSynchronize(g->stream));  // zT is a local
    if (z != g->z_host.data()) g->z_host.assign(z, z + (size_t)nz * d);
    g->fitted = false;
    g->winv_ok = false;
    return EGX_SUCCESS;
}

// The box of the inducing points in phase 2 of egx_sgp_fit_lbfgs_z and the map from its unit variables:
// z[j, k] = clamp(lo_k + u[j, k] (hi_k - lo_k)); a column with hi_k == lo_k keeps the points' own coordinates z0[., k]
struct ZBox {
    int nz = 0, d = 0;
    std::vector<double> lo, hi, z0;
    void to_z(const double *u, std::vector<double> &z) const {
        z.resize((size_t)nz * d);
        for (int j = 0; j < nz; j++)
            for (int k = 0; k < d; k++) {
                const size_t e = (size_t)j * d + k;
                z[e] = hi[k] > lo[k] ? std::fmin(hi[k], std::fmax(lo[k], lo[k] + u[e] * (hi[k] - lo[k]))) : z0[e];
            }
    }
};

// f = -L and its gradient at xv = [log10 params (np), u (nz d)] for phase 2: the points are set, then the likelihood and both
// gradients are evaluated.  g_u = -(hi_k - lo_k) dL/dz[j, k], 0 in a fixed column.  A failed evaluation is f = +inf.
int sgp_eval_grad_xz(egx_sgp *g, const std::vector<double> &xv, int np, int estimate_noise, double noise_fixed, const ZBox &box,
                     double &f, std::vector<double> &gx) {
    const int d = g->d, nz = g->nz, nt = g->h;  // nt: theta components; the points keep d coordinates
    const size_t h = (size_t)np + (size_t)nz * d;
    std::vector<double> prm(nt + 2), grad(nt + 2, 0.0), z, gz((size_t)nz * d, 0.0);
    box.to_z(xv.data() + np, z);
    EGX_RC(sgp_upload_z(g, z.data()));
    for (int i = 0; i <= nt; i++) prm[i] = std::pow(10.0, xv[i]);
    prm[nt + 1] = estimate_noise ? std::pow(10.0, xv[nt + 1]) : noise_fixed;
    Eval ev;
    EGX_RC(sgp_eval(g, prm.data(), nt, prm[nt], prm[nt + 1], ev, false));
    f = std::numeric_limits<double>::infinity();
    gx.assign(h, 0.0);
    if (ev.status != EGX_STATUS_OK) return EGX_SUCCESS;
    EGX_RC(sgp_grad_tail(g, prm[nt], prm[nt + 1], grad.data()));
    EGX_RC(sgp_grad_tail_z(g, prm[nt], gz.data()));
    f = -ev.lkh;
    const double ln10 = std::log(10.0);
    for (int i = 0; i < np; i++) gx[i] = -prm[i] * ln10 * grad[i];
    for (int j = 0; j < nz; j++)
        for (int k = 0; k < d; k++) {
            const size_t e = (size_t)j * d + k;
            gx[np + e] = box.hi[k] > box.lo[k] ? -(box.hi[k] - box.lo[k]) * gz[e] : 0.0;
        }
    for (size_t i = 0; i < h; i++)
        if (!std::isfinite(gx[i])) {
            f = std::numeric_limits<double>::infinity();
            gx.assign(h, 0.0);
            break;
        }
    return EGX_SUCCESS;
}

}  // namespace

namespace egx {
int sgp_launch_transpose_scale(egx_sgp *g, const double *sb, double scale) {
    hipLaunchKernelGGL(k_sgp_transpose_scale, dim3(g->n_pad / 32, g->zext / 32), dim3(256), 0, g->stream, g->RT.p, g->z_pad, g->n,
                       g->nz, sb, g->y.p, scale, g->W.p, g->n_pad);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_SUCCESS;
}
}  // namespace egx

extern "C" {

void egx_sgp_config_default(egx_sgp_config *cfg) {
    if (!cfg) return;
    cfg->corr = EGX_CORR_SQUARED_EXPONENTIAL;
    cfg->method = EGX_SGP_FITC;
    cfg->nugget = 100.0 * 2.220446049250313e-16;
    cfg->device = -1;
}

void egx_sgp_destroy(egx_sgp *g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
}

int32_t egx_sgp_create(const egx_sgp_config *cfg_in, const double *x, const double *y, int64_t n, int64_t d,
                       const double *z, int64_t nz, egx_sgp **out) {
    if (!out) {
        set_error("out handle pointer is NULL");
        return EGX_ERR_INVALID_VALUE;
    }
    *out = nullptr;
    egx_sgp_config cfg;
    if (cfg_in) cfg = *cfg_in; else egx_sgp_config_default(&cfg);
    if (!x || !y || !z || n < 2 || nz < 1 || nz > n || d < 1) {
        set_error("egx_sgp_create: need x (n x d), y (n), z (nz x d) with 1 <= nz <= n, n >= 2, d >= 1");
        return EGX_ERR_INVALID_VALUE;
    }
    if (cfg.corr < 0 || cfg.corr > 3 || (cfg.method != EGX_SGP_FITC && cfg.method != EGX_SGP_VFE) ||
        !(cfg.nugget >= 0.0) || !std::isfinite(cfg.nugget)) {
        set_error("egx_sgp_create: unknown correlation / method, or negative nugget");
        return EGX_ERR_INVALID_VALUE;
    }
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
    for (int64_t i = 0; i < nz * d; i++)
        if (!std::isfinite(z[i])) {
            set_error("z contains non-finite values");
            return EGX_ERR_INVALID_VALUE;
        }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device: libegx_gp_hip has no CPU fallback (needs an MI355X / gfx950 GPU)");
        return EGX_ERR_NO_DEVICE;
    }
    int dev = cfg.device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (dev >= ndev) {
        set_error("device ordinal out of range");
        return EGX_ERR_INVALID_VALUE;
    }
    egx_sgp *g = new egx_sgp();
    g->device = dev;
    g->corr = cfg.corr;
    g->method = cfg.method;
    g->nugget = cfg.nugget;
    g->n = (int)n;
    g->d = (int)d;
    g->h = (int)d;
    g->nz = (int)nz;
    g->n_pad = (int)round_up(n, kTile);
    g->z_pad = (int)round_up(nz, kTile);
    g->zext = g->z_pad + kTile;
    g->y_host.assign(y, y + n);
    for (int64_t i = 0; i < n; i++) g->yty += y[i] * y[i];
    g->z_host.assign(z, z + nz * d);
    g->x_lo.assign(x, x + d);
    g->x_hi.assign(x, x + d);
    for (int64_t i = 1; i < n; i++)
        for (int64_t k = 0; k < d; k++) {
            g->x_lo[k] = std::fmin(g->x_lo[k], x[i * d + k]);
            g->x_hi[k] = std::fmax(g->x_hi[k], x[i * d + k]);
        }
    auto fail = [&](int rc) {
        egx_sgp_destroy(g);
        return rc;
    };
#define SGP_TRY(expr)                       \
    do {                                    \
        int _rc = (expr);                   \
        if (_rc) return fail(_rc);          \
    } while (0)
#define SGP_HIP(expr)                                                             \
    do {                                                                          \
        hipError_t _e = (expr);                                                   \
        if (_e != hipSuccess) {                                                   \
            set_error(std::string(#expr) + ": " + hipGetErrorString(_e));         \
            (void)hipGetLastError();                                              \
            return fail(EGX_ERR_HIP);                                             \
        }                                                                         \
    } while (0)
    SGP_HIP(hipSetDevice(dev));
    SGP_TRY(chol_init());
    SGP_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    const size_t np = g->n_pad, zp = g->z_pad, ze = g->zext;
    std::vector<double> xT((size_t)d * np, 0.0), zT((size_t)d * zp, 0.0), yp(np, 0.0);
    for (int64_t i = 0; i < n; i++)
        for (int64_t k = 0; k < d; k++) xT[(size_t)k * np + i] = x[i * d + k];
    for (int64_t i = 0; i < nz; i++)
        for (int64_t k = 0; k < d; k++) zT[(size_t)k * zp + i] = z[i * d + k];
    for (int64_t i = 0; i < n; i++) yp[i] = y[i];
    SGP_TRY(g->xT.alloc(xT.size()));
    SGP_TRY(g->zT.alloc(zT.size()));
    SGP_TRY(g->y.alloc(np));
    SGP_TRY(g->coef.alloc((size_t)d));
    SGP_TRY(g->RT.alloc(np * zp));
    SGP_TRY(g->W.alloc(ze * np));
    SGP_TRY(g->G.alloc(ze * ze));
    SGP_TRY(g->P.alloc(gram_scratch_doubles((int)ze, (int)np)));
    SGP_TRY(g->Kz.alloc(zp * zp));
    SGP_TRY(g->A.alloc(ze * zp));
    SGP_TRY(g->dinv_z.alloc(dinv_doubles(zp)));
    SGP_TRY(g->dinv_a.alloc(dinv_doubles(zp)));
    SGP_TRY(g->s0.alloc(np));
    SGP_TRY(g->sb.alloc(np));
    SGP_TRY(g->diag.alloc(zp));
    SGP_TRY(g->brow.alloc(zp));
    SGP_TRY(g->vec.alloc(zp));
    SGP_TRY(g->tmpv.alloc(zp));
    SGP_TRY(g->wall.alloc(block_inverse_doubles(zp)));
    SGP_TRY(g->d_info.alloc(2));
    SGP_HIP(hipMemcpy(g->xT.p, xT.data(), sizeof(double) * xT.size(), hipMemcpyHostToDevice));
    SGP_HIP(hipMemcpy(g->zT.p, zT.data(), sizeof(double) * zT.size(), hipMemcpyHostToDevice));
    SGP_HIP(hipMemcpy(g->y.p, yp.data(), sizeof(double) * np, hipMemcpyHostToDevice));
#undef SGP_TRY
#undef SGP_HIP
    *out = g;
    return EGX_SUCCESS;
}

int32_t egx_sgp_dims(const egx_sgp *g, int64_t *n, int64_t *d, int64_t *nz) {
    if (!g) {
        set_error("NULL handle");
        return EGX_ERR_INVALID_VALUE;
    }
    if (n) *n = g->n;
    if (d) *d = g->d;
    if (nz) *nz = g->nz;
    return EGX_SUCCESS;
}

int32_t egx_sgp_likelihood(egx_sgp *g, const double *theta, int64_t theta_len, double sigma2, double noise, double *lkh,
                           int32_t *status) {
    if (!g || !theta || !lkh || !status) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    EGX_HIP_CHECK(hipSetDevice(g->device));
    Eval ev;
    const int rc = sgp_eval(g, theta, theta_len, sigma2, noise, ev, false);
    if (rc) return rc;
    *lkh = ev.lkh;
    *status = ev.status;
    return EGX_SUCCESS;
}

// The likelihood of egx_sgp_likelihood (the same launches first: the same bits) and its gradient, grad (d + 2) = dL/dtheta_0..d-1
// (of the broadcast theta when theta_len == 1), dL/dsigma2, dL/dnoise; zeros whenever *status != EGX_STATUS_OK
int32_t egx_sgp_likelihood_grad(egx_sgp *g, const double *theta, int64_t theta_len, double sigma2, double noise, double *lkh,
                                double *grad, int32_t *status) {
    if (!g || !theta || !lkh || !grad || !status) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    EGX_HIP_CHECK(hipSetDevice(g->device));
    Eval ev;
    EGX_RC(sgp_eval(g, theta, theta_len, sigma2, noise, ev, false));
    for (int i = 0; i < g->h + 2; i++) grad[i] = 0.0;
    if (ev.status == EGX_STATUS_OK) EGX_RC(sgp_grad_tail(g, sigma2, noise, grad));
    *lkh = ev.lkh;
    *status = ev.status;
    return EGX_SUCCESS;
}

int32_t egx_sgp_finalize(egx_sgp *g, const double *theta, int64_t theta_len, double sigma2, double noise) {
    if (!g || !theta) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    EGX_HIP_CHECK(hipSetDevice(g->device));
    Eval ev;
    const int rc = sgp_eval(g, theta, theta_len, sigma2, noise, ev, true);
    if (rc) return rc;
    if (ev.status != EGX_STATUS_OK) {
        set_error(ev.status == EGX_STATUS_NAN_THETA ? "sparse GP: NaN / non-positive parameters"
                                                    : "sparse GP: Kmm or I + V diag(beta) V^T is not positive definite");
        return ev.status == EGX_STATUS_NAN_THETA ? EGX_ERR_LIKELIHOOD : EGX_ERR_LINALG;
    }
    return EGX_SUCCESS;
}

// Multistart derivative-free fit over x = log10([theta_1..theta_d, sigma2, (noise)]) (sparse_algorithm.rs:488-650):
// params0s is (n_starts x np) in parameter space, lo/hi (np) its box, np = d + 1 + estimate_noise.  COBYLA as for the dense model
// (sparse_algorithm.rs:597-611), one start after the other.  An evaluation that fails with a HIP or argument error ends the fit
// AT ONCE with its code (it used to go on evaluating and return that same first code at the end).
int32_t egx_sgp_fit(egx_sgp *g, const double *params0s, int64_t n_starts, const double *lo, const double *hi,
                    int32_t estimate_noise, double noise_fixed, int64_t max_eval, int64_t *n_evals_out) {
    if (!g || !params0s || !lo || !hi || n_starts < 1) {
        set_error("NULL argument / no start point");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    EGX_HIP_CHECK(hipSetDevice(g->device));
    const int d = g->h, np = d + 1 + (estimate_noise ? 1 : 0);  // d: theta components
    fit::Log10Box box;
    EGX_RC(fit_box(lo, hi, np, np, params0s, n_starts * np, fit::Sparse, box));
    // the budget counts the theta dimensions, not np (sparse_algorithm.rs:601-603)
    std::vector<CobylaBox> mach = fit::cobyla_machines(params0s, np, fit::shard(n_starts), box, fit::cobyla_budget(d, max_eval));
    Eval ev;
    int rc;
    fit::run_sequential(
        mach,
        [&](const multistart::Round &r) {
            const double *xv = r.pts.data();
            std::vector<double> th(d);
            for (int i = 0; i < d; i++) th[i] = std::pow(10.0, xv[i]);
            const double s2 = std::pow(10.0, xv[d]);
            const double nv = estimate_noise ? std::pow(10.0, xv[d + 1]) : noise_fixed;
            ev = Eval();
            return sgp_eval(g, th.data(), d, s2, nv, ev, false);
        },
        [&](const multistart::Round &, size_t, CobylaBox &m) { m.tell(fit::cobyla_objective(ev.status == EGX_STATUS_OK, ev.lkh)); }, rc);
    EGX_RC(rc);
    std::vector<StartResult> results;
    for (const CobylaBox &m : mach) results.push_back(fit::cobyla_result(m));
    return sgp_fit_keep(g, fit::best_start(results, n_evals_out), estimate_noise, noise_fixed);
}

// The gradient-based counterpart of egx_sgp_fit (new: on the closed-form gradient, sgp_grad.hip): a projected L-BFGS (lbfgs.h) per
// start on x = log10(params), same parameter layout, box and checks.  The starts run one after the other -- the handle has one
// workspace --, the best wins (the first on ties), one keeping evaluation follows.  max_iter < 1: 50 iterations per start.
// It is egx_sgp_fit_lbfgs_z without a phase 2 (the points' default box, the range of the training inputs, always passes).
int32_t egx_sgp_fit_lbfgs(egx_sgp *g, const double *params0s, int64_t n_starts, const double *lo, const double *hi,
                          int32_t estimate_noise, double noise_fixed, int64_t max_iter, int64_t *n_evals_out) {
    return egx_sgp_fit_lbfgs_z(g, params0s, n_starts, lo, hi, estimate_noise, noise_fixed, max_iter, nullptr, nullptr, 0, n_evals_out);
}

// egx_sgp_likelihood_grad (the same launches first: the same bits of *lkh and grad) and the gradient in the inducing points,
// grad_z (nz x d, row-major like z), from two more launches over the pair weights that call leaves on the device (sgp_grad.hip)
int32_t egx_sgp_likelihood_grad_z(egx_sgp *g, const double *theta, int64_t theta_len, double sigma2, double noise, double *lkh,
                                  double *grad, double *grad_z, int32_t *status) {
    if (!g || !theta || !lkh || !grad || !grad_z || !status) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    EGX_HIP_CHECK(hipSetDevice(g->device));
    Eval ev;
    EGX_RC(sgp_eval(g, theta, theta_len, sigma2, noise, ev, false));
    for (int i = 0; i < g->h + 2; i++) grad[i] = 0.0;
    for (size_t e = 0; e < (size_t)g->nz * g->d; e++) grad_z[e] = 0.0;
    if (ev.status == EGX_STATUS_OK) {
        EGX_RC(sgp_grad_tail(g, sigma2, noise, grad));
        EGX_RC(sgp_grad_tail_z(g, sigma2, grad_z));
    }
    *lkh = ev.lkh;
    *status = ev.status;
    return EGX_SUCCESS;
}

int32_t egx_sgp_set_inducings(egx_sgp *g, const double *z) {
    if (!g || !z) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    for (size_t e = 0; e < (size_t)g->nz * g->d; e++)
        if (!std::isfinite(z[e])) {
            set_error("z contains non-finite values");
            return EGX_ERR_INVALID_VALUE;
        }
    EGX_HIP_CHECK(hipSetDevice(g->device));
    return sgp_upload_z(g, z);
}

int32_t egx_sgp_get_inducings(egx_sgp *g, double *z) {
    if (!g || !z) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    std::memcpy(z, g->z_host.data(), sizeof(double) * g->z_host.size());
    return EGX_SUCCESS;
}

// The KPLS weights (header).  They are checked before anything changes; the coefficient buffer grows to d x h and |w| goes to the
// device once, for the Matern form of the gradient kernel (sgp_grad.hip), as the dense model's d_wabs does.
namespace {
// caller holds g->mu; g, w and 1 <= h <= d are checked
int sgp_install_w_star(egx_sgp *g, const double *w, int64_t h) {
    const size_t cnt = (size_t)g->d * (size_t)h;
    for (size_t e = 0; e < cnt; e++)
        if (!std::isfinite(w[e])) {
            set_error("w_star contains non-finite values");
            return EGX_ERR_INVALID_VALUE;
        }
    EGX_HIP_CHECK(hipSetDevice(g->device));
    std::vector<double> wabs(cnt);
    for (size_t e = 0; e < cnt; e++) wabs[e] = std::fabs(w[e]);
    EGX_RC(g->coef.alloc(cnt));
    EGX_RC(g->d_wabs.alloc(cnt));
    EGX_HIP_CHECK(hipMemcpyAsync(g->d_wabs.p, wabs.data(), sizeof(double) * cnt, hipMemcpyHostToDevice, g->stream));
    EGX_HIP_CHECK(hipStreamSynchronize(g->stream));  // wabs is a local
    g->w_star.assign(w, w + cnt);
    g->has_w = true;
    g->h = (int)h;
    g->hcols = (g->corr == EGX_CORR_MATERN32 || g->corr == EGX_CORR_MATERN52) ? (int)h : 1;
    g->fitted = false;
    g->winv_ok = false;
    return EGX_SUCCESS;
}
}  // namespace

int32_t egx_sgp_set_w_star(egx_sgp *g, const double *w, int64_t h) {
    if (w && h == 0) {  // sparse_parameters.rs:306-311 (needs no handle: refused first)
        set_error("`kpls_dim` canot be 0!");
        return EGX_ERR_INVALID_VALUE;
    }
    if (!g) {
        set_error("NULL handle");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    const int d = g->d;
    if (!w && h == 0) {  // back to w = I
        g->has_w = false;
        g->w_star.clear();
        g->h = d;
        g->hcols = 1;
        g->fitted = false;
        g->winv_ok = false;
        return EGX_SUCCESS;
    }
    if (h < 0 || h > d) {  // sparse_algorithm.rs:430-438
        set_error("Dimension reduction " + std::to_string(h) + " should be smaller than actual training input dimensions " +
                  std::to_string(d));
        return EGX_ERR_INVALID_VALUE;
    }
    if (!w) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    return sgp_install_w_star(g, w, h);
}

// The PLS rotations of the resident training set (kernels_pls.hip), installed as egx_sgp_set_w_star installs a caller's
int32_t egx_sgp_compute_w_star(egx_sgp *g, int64_t k) {
    if (k < 1) return pls_check_k(k, 1);  // needs no handle: refused first, as in egx_sgp_set_w_star
    if (!g) {
        set_error("NULL handle");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    EGX_RC(pls_check_k(k, g->d));
    EGX_HIP_CHECK(hipSetDevice(g->device));
    std::vector<double> w((size_t)g->d * (size_t)k);
    int st = 0;
    EGX_RC(pls_device_rotations(g->stream, g->xT.p, g->n_pad, g->y.p, g->n, g->d, (int)k, w.data(), &st));
    return sgp_install_w_star(g, w.data(), k);
}

int32_t egx_sgp_pls_launch_ms(egx_sgp *g, double *ms) {
    if (!g || !ms) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    EGX_HIP_CHECK(hipSetDevice(g->device));
    return pls_device_launch_ms(g->stream, g->xT.p, g->n_pad, g->y.p, g->n, g->d, ms);
}

int32_t egx_sgp_get_w_star(egx_sgp *g, double *w, int64_t *h) {
    if (!g || !h) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    *h = g->h;
    if (w && g->has_w) std::memcpy(w, g->w_star.data(), sizeof(double) * g->w_star.size());
    return EGX_SUCCESS;
}

// egx_sgp_fit_lbfgs, then one more L-BFGS from its winner in which the inducing points move too (header: phase 2).  The phase-2
// point is kept only where its likelihood is strictly higher; otherwise the points go back, bit for bit, to where they were.
int32_t egx_sgp_fit_lbfgs_z(egx_sgp *g, const double *params0s, int64_t n_starts, const double *lo, const double *hi,
                            int32_t estimate_noise, double noise_fixed, int64_t max_iter, const double *z_lo, const double *z_hi,
                            int64_t max_iter_z, int64_t *n_evals_out) {
    if (!g || !params0s || !lo || !hi || n_starts < 1) {
        set_error("NULL argument / no start point");
        return EGX_ERR_INVALID_VALUE;
    }
    if ((z_lo == nullptr) != (z_hi == nullptr)) {
        set_error("z_lo and z_hi must be given together");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    EGX_HIP_CHECK(hipSetDevice(g->device));
    const int d = g->d, nz = g->nz, np = g->h + 1 + (estimate_noise ? 1 : 0);
    fit::Log10Box pbox;
    EGX_RC(fit_box(lo, hi, np, np, params0s, n_starts * np, fit::Sparse, pbox));
    ZBox box;
    box.nz = nz;
    box.d = d;
    box.lo = z_lo ? std::vector<double>(z_lo, z_lo + d) : g->x_lo;
    box.hi = z_hi ? std::vector<double>(z_hi, z_hi + d) : g->x_hi;
    for (int k = 0; k < d; k++)
        if (!std::isfinite(box.lo[k]) || !std::isfinite(box.hi[k]) || !(box.hi[k] >= box.lo[k])) {
            set_error("sparse GP inducing-point bounds must be finite with z_lo <= z_hi");
            return EGX_ERR_INVALID_VALUE;
        }
    if (max_iter_z < 0) max_iter_z = 50;
    std::vector<StartResult> results;
    int64_t evals = 0;
    std::vector<LbfgsStart> starts = fit::lbfgs_machines(params0s, np, fit::shard(n_starts), pbox, max_iter < 1 ? 50 : max_iter);
    EGX_RC(sgp_lbfgs_run(
        starts, [&](const std::vector<double> &xv, double &f, std::vector<double> &gx) { return sgp_eval_grad_x(g, xv, estimate_noise, noise_fixed, f, gx); },
        results, evals));
    const StartResult *best = fit::best_start(results);
    std::vector<StartResult> end;  // phase 2's
    if (max_iter_z > 0 && best) {
        box.z0 = g->z_host;
        const size_t nu = (size_t)nz * d;
        std::vector<double> x0(np + nu), xlo(np + nu, 0.0), xhi(np + nu, 1.0);
        for (int i = 0; i < np; i++) {
            x0[i] = best->x[i];
            xlo[i] = pbox.lo[i];
            xhi[i] = pbox.hi[i];
        }
        for (size_t e = 0; e < nu; e++) {
            const int k = (int)(e % (size_t)d);
            x0[np + e] = box.hi[k] > box.lo[k] ? (box.z0[e] - box.lo[k]) / (box.hi[k] - box.lo[k]) : 0.0;
        }
        std::vector<LbfgsStart> mach;
        mach.emplace_back(LbfgsStart::Linear(), x0.data(), (int)(np + nu), xlo, xhi, max_iter_z);
        EGX_RC(sgp_lbfgs_run(
            mach, [&](const std::vector<double> &xv, double &f, std::vector<double> &gx) { return sgp_eval_grad_xz(g, xv, np, estimate_noise, noise_fixed, box, f, gx); },
            end, evals));
        std::vector<double> z = box.z0;
        if (end[0].f < best->f) {
            box.to_z(end[0].x.data() + np, z);
            best = &end[0];  // (the keeping evaluation reads its first np variables)
        }
        EGX_RC(sgp_upload_z(g, z.data()));
    }
    if (n_evals_out) *n_evals_out = evals;
    return sgp_fit_keep(g, best, estimate_noise, noise_fixed);
}

// Fitted state: theta (d), sigma2, noise, likelihood, Woodbury vector (nz) and -- computed on the host from the two
// downloaded nz x nz factors, for serialisation only -- the Woodbury matrix (nz x nz, sparse_algorithm.rs:757-763, 823-829).
int32_t egx_sgp_get_state(egx_sgp *g, double *theta, double *sigma2, double *noise, double *likelihood, double *w_vec,
                          double *w_inv) {
    if (!g) {
        set_error("NULL handle");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    if (!g->fitted) {
        set_error("sparse model is not fitted");
        return EGX_ERR_NOT_FITTED;
    }
    EGX_HIP_CHECK(hipSetDevice(g->device));
    const int nz = g->nz, z_pad = g->z_pad;
    if (theta) std::memcpy(theta, g->theta.data(), sizeof(double) * g->h);
    if (sigma2) *sigma2 = g->sigma2;
    if (noise) *noise = g->noise;
    if (likelihood) *likelihood = g->likelihood;
    if (w_vec) std::memcpy(w_vec, g->w_vec.data(), sizeof(double) * nz);
    if (w_inv) {
        std::vector<double> cz((size_t)z_pad * z_pad), la((size_t)z_pad * z_pad);
        EGX_HIP_CHECK(hipMemcpy(cz.data(), g->Kz.p, sizeof(double) * cz.size(), hipMemcpyDeviceToHost));
        EGX_HIP_CHECK(hipMemcpy(la.data(), g->A.p, sizeof(double) * la.size(), hipMemcpyDeviceToHost));
        const double sigma = std::sqrt(g->sigma2);
        auto tri_inv = [&](const std::vector<double> &Lm, double scale, std::vector<double> &X) {  // X = (scale L)^-1
            X.assign((size_t)nz * nz, 0.0);
            for (int c = 0; c < nz; c++)
                for (int i = c; i < nz; i++) {
                    double sacc = (i == c) ? 1.0 : 0.0;
                    for (int k = c; k < i; k++) sacc -= Lm[(size_t)i * z_pad + k] * scale * X[(size_t)k * nz + c];
                    X[(size_t)i * nz + c] = sacc / (Lm[(size_t)i * z_pad + i] * scale);
                }
        };
        std::vector<double> ui, li, liui((size_t)nz * nz, 0.0);
        tri_inv(cz, sigma, ui);
        tri_inv(la, 1.0, li);
        for (int i = 0; i < nz; i++)
            for (int k = 0; k <= i; k++) {
                const double lik = li[(size_t)i * nz + k];
                if (lik == 0.0) continue;
                for (int j = 0; j <= k; j++) liui[(size_t)i * nz + j] += lik * ui[(size_t)k * nz + j];
            }
        for (int i = 0; i < nz; i++)
            for (int j = 0; j < nz; j++) {
                double uu = 0.0, ll = 0.0;
                for (int k = (i > j ? i : j); k < nz; k++) {
                    uu += ui[(size_t)k * nz + i] * ui[(size_t)k * nz + j];
                    ll += liui[(size_t)k * nz + i] * liui[(size_t)k * nz + j];
                }
                w_inv[(size_t)i * nz + j] = (g->method == 0) ? uu - ll : uu + ll;
            }
    }
    return EGX_SUCCESS;
}

}  // extern "C"
