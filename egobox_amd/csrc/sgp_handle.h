// Internal header of the sparse-GP translation units (sgp_host.hip: handle, likelihood, fit, state; sgp_predict.hip:
// predictions, their x-gradients, sampling; sgp_grad.hip: the likelihood's gradient).
#pragma once
#include <mutex>
#include <vector>

#include "gp_handle.h"

struct egx_sgp {
    int device = 0, corr = 0, method = 0;
    double nugget = 0.0;
    int n = 0, d = 0, nz = 0, n_pad = 0, z_pad = 0, zext = 0;
    std::vector<double> y_host;
    double yty = 0.0;
    hipStream_t stream = nullptr;
    egx::DevBuf xT, zT, y, coef, RT, W, G, P, Kz, A, dinv_z, dinv_a, s0, sb, diag, brow, vec, wall, tmpv;
    egx::DevMem<int> d_info;
    std::mutex mu;
    // fitted state
    bool fitted = false;
    std::vector<double> theta;
    double sigma2 = 0.0, noise = 0.0, likelihood = 0.0;
    std::vector<double> w_vec;
    // predictions (sgp_predict.hip): the explicit inverse factors C_z^-T and L^-T (upper triangular, z_pad x z_pad) of the
    // fitted state, built by the first gradient call after a fit, and the grow-only workspace of the query chunks
    bool winv_ok = false;
    egx::DevBuf Wz, Wa, q_x, q_RT, q_E, q_Ct, q_part, q_out;
    std::vector<double> h_x, h_out;
    // likelihood gradient (sgp_grad.hip): grow-only workspace of egx_sgp_likelihood_grad, allocated by its first call.  gr_E is
    // the one n_pad x z_pad buffer (E~, then T^T); gr_rows 7 n_pad vectors; gr_G2 zext^2 (FITC); gr_sq three z_pad^2 matrices
    egx::DevBuf gr_E, gr_rows, gr_G2, gr_sq, gr_vec, gr_part, gr_out;
    // gradient in the inducing points (sgp_grad.hip, sgp_grad_tail_z): the partial column sums [row chunk][column][d] and the
    // two reduced nz x d matrices, grow-only like gr_part; the current inducing points (nz x d, row-major: what zT holds) and
    // the per-column range of the training inputs, the default box of egx_sgp_fit_lbfgs_z
    egx::DevBuf gz_part, gz_out;
    std::vector<double> z_host, x_lo, x_hi;
    // KPLS (egx_sgp_set_w_star): h = the number of theta components (d without weights), w_star (d x h, row-major) and |w| on the
    // device for the Matern gradient kernel; hcols / coef_host / th_full: the table of the last evaluation (kpls_coef.h), d x hcols
    // in `coef`, and the theta it came from, which sgp_grad_tail's chain rule reads
    int h = 0, hcols = 1;
    bool has_w = false;
    std::vector<double> w_star, coef_host, th_full;
    egx::DevBuf d_wabs;
    const double *w_ptr() const { return has_w ? w_star.data() : nullptr; }
};


namespace egx {
// ---- sgp_predict.hip ----
// any subset of mean (m), variance (m), d mean / dx (m x d), d var / dx (m x d) of the m queries; caller holds g->mu
int sgp_query(egx_sgp *g, const double *xq, int64_t m, double *yout, double *vout, double *gyout, double *gvout);
// Wz <- C_z^-T, Wa <- L^-T for the resident factors (cached until the next evaluation of the likelihood); caller holds g->mu
int sgp_ensure_inverse_factors(egx_sgp *g);
// E <- sgn * RT over `count` doubles (an even count): the copy of a~ the transposed products subtract from
int sgp_launch_scale_copy(hipStream_t s, const double *RT, double sgn, int64_t count, double *E);
// ---- sgp_host.hip ----
// W <- [scale * diag(sb) RT]^T with the row sb o y below it: the operand of the likelihood's Gram product, for any weights sb (n)
int sgp_launch_transpose_scale(egx_sgp *g, const double *sb, double scale);
// ---- sgp_grad.hip ----
// grad (h + 2; h = d without KPLS weights) = dL/dtheta, dL/dsigma2, dL/dnoise at the parameters of the evaluation whose factors are resident
// (a successful sgp_eval that has just returned); caller holds g->mu
int sgp_grad_tail(egx_sgp *g, double sigma2, double noise, double *grad);
// grad_z (nz x d, row-major) = dL/dz right after a successful sgp_grad_tail, whose pair weights T^T (gr_E) and S^ (gr_sq) it
// contracts once more; caller holds g->mu
int sgp_grad_tail_z(egx_sgp *g, double sigma2, double *grad_z);
}  // namespace egx
