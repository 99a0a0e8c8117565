// PLS1 rotations from the centred Gram matrix (host only, no HIP: tests/c_host/pls_host_test.cpp compiles it alone).
//
// The data of a PLS1 regression (one response) enter the NIPALS recursion of egobox_amd/kpls.py only through G = X^T X and
// s = X^T y of the standardised columns.  With w = s / |s|, t = X w:
//     tt = t^T t = w^T G w,   p = X^T t / tt = G w / tt,   q = y^T t / tt = |s| / tt,
// and the deflation X <- X - t p^T = X (I - w p^T), y <- y - q t turns into
//     s <- (I - p w^T) (s - |s| p),   G <- (I - p w^T) G (I - w p^T),   |y|^2 <- |y|^2 - q^2 tt.
// The rotations are W (P^T W)^-1 (d x k).  P^T W is upper triangular with a unit diagonal in exact arithmetic, so the inverse
// exists whenever the recursion got through its k components; it is taken by Gauss-Jordan elimination with row pivoting.
// The device computes the unscaled centred Gram matrix C of [X | y] (kernels_pls.hip); everything below is O(d^2 k).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/egx_gp.h"

namespace egx {
namespace pls {

// ---- the launch plan: the ONLY place that decides the split of the rows and the tiling of the output ----------------------------
constexpr int kTile16 = 16;          // one MFMA output tile
constexpr int kBlockCols = 64;       // columns of [X | y] per workgroup side: a workgroup owns a 64 x 64 block of 4 x 4 tiles
constexpr int64_t kMinChunkRows = 256;
constexpr int64_t kMaxChunks = 256;
constexpr int64_t kTargetWorkgroups = 1024;  // ~4 per compute unit of an MI355X

// Rows [c * chunk_rows, min(n, (c + 1) * chunk_rows)) belong to chunk c < n_chunks: every row once, no chunk empty.
// chunk_rows is a multiple of 64 and never shrinks as n grows; tiles / out_tiles / blocks never shrink as d grows.
inline bool plan(int64_t n, int64_t d, egx_pls_plan *out) {
    if (!out || n < 1 || d < 1) return false;
    const int64_t cols = d + 1;
    const int64_t side = (cols + kBlockCols - 1) / kBlockCols;
    const int64_t blocks = side * (side + 1) / 2;
    int64_t want = (kTargetWorkgroups + blocks - 1) / blocks;
    if (want > kMaxChunks) want = kMaxChunks;
    if (want < 8) want = 8;
    int64_t rows = (n + want - 1) / want;
    rows = (rows + 63) / 64 * 64;
    if (rows < kMinChunkRows) rows = kMinChunkRows;
    out->n = n;
    out->d = d;
    out->chunk_rows = rows;
    out->n_chunks = (n + rows - 1) / rows;
    out->tiles = (cols + kTile16 - 1) / kTile16;
    out->out_tiles = out->tiles * (out->tiles + 1) / 2;
    out->block_side = side;
    out->blocks = blocks;
    return true;
}

// ---- the d-space recursion -------------------------------------------------------------------------------------------------------
enum { kOk = 0, kConstant = 1 };

inline double dot(const double *a, const double *b, int n) {
    long double s = 0.0L;
    for (int i = 0; i < n; i++) s += (long double)a[i] * (long double)b[i];
    return (double)s;
}

// a (k x k, row-major) <- a^-1 by Gauss-Jordan elimination with row pivoting; false when a pivot vanishes
inline bool invert_small(std::vector<double> &a, int k) {
    std::vector<double> inv((size_t)k * k, 0.0);
    for (int i = 0; i < k; i++) inv[(size_t)i * k + i] = 1.0;
    for (int c = 0; c < k; c++) {
        int piv = c;
        for (int r = c + 1; r < k; r++)
            if (std::fabs(a[(size_t)r * k + c]) > std::fabs(a[(size_t)piv * k + c])) piv = r;
        const double pv = a[(size_t)piv * k + c];
        if (pv == 0.0 || !std::isfinite(pv)) return false;
        if (piv != c)
            for (int j = 0; j < k; j++) {
                std::swap(a[(size_t)piv * k + j], a[(size_t)c * k + j]);
                std::swap(inv[(size_t)piv * k + j], inv[(size_t)c * k + j]);
            }
        for (int j = 0; j < k; j++) {
            a[(size_t)c * k + j] /= pv;
            inv[(size_t)c * k + j] /= pv;
        }
        for (int r = 0; r < k; r++) {
            if (r == c) continue;
            const double f = a[(size_t)r * k + c];
            if (f == 0.0) continue;
            for (int j = 0; j < k; j++) {
                a[(size_t)r * k + j] -= f * a[(size_t)c * k + j];
                inv[(size_t)r * k + j] -= f * inv[(size_t)c * k + j];
            }
        }
    }
    a.swap(inv);
    return true;
}

// G (d x d, row-major, symmetric), s (d) and yty of the STANDARDISED columns (G and s are consumed), n rows behind them.
// rot (d x k, row-major) = W (P^T W)^-1 and kOk, or all zeros and kConstant where kpls.py returns zeros inside its loop: a residual
// below its threshold, or |s| < eps.  kpls.py tests every element of the residual against 10 eps; here the residual exists only as
// its norm, |y_res|^2 = yty - sum q^2 tt, and the test is |y_res|^2 < n (10 eps)^2: what the element test implies, not its equal.
inline int rotations_from_gram(std::vector<double> &G, std::vector<double> &s, double yty, int64_t n, int d, int k, double *rot) {
    const double eps = std::numeric_limits<double>::epsilon();
    for (size_t e = 0; e < (size_t)d * k; e++) rot[e] = 0.0;
    std::vector<double> W((size_t)d * k, 0.0), P((size_t)d * k, 0.0), w(d), p(d), u(d);
    double res2 = yty;
    for (int a = 0; a < k; a++) {
        if (res2 < (double)n * (10.0 * eps) * (10.0 * eps)) return kConstant;
        const double nrm = std::sqrt(dot(s.data(), s.data(), d));
        if (!(nrm >= eps)) return kConstant;
        for (int j = 0; j < d; j++) w[j] = s[j] / nrm;
        for (int j = 0; j < d; j++) u[j] = dot(&G[(size_t)j * d], w.data(), d);  // G w
        const double tt = dot(w.data(), u.data(), d);
        if (!(tt > 0.0)) return kConstant;  // t = X w vanished: nothing left to regress on
        for (int j = 0; j < d; j++) p[j] = u[j] / tt;
        const double q = nrm / tt;
        res2 -= q * q * tt;
        // s <- (I - p w^T) (s - |s| p)
        for (int j = 0; j < d; j++) s[j] -= nrm * p[j];
        const double ws = dot(w.data(), s.data(), d);
        for (int j = 0; j < d; j++) s[j] -= p[j] * ws;
        // G <- (I - p w^T) G (I - w p^T): rows first (w^T G = (G w)^T = u^T), then columns
        for (int i = 0; i < d; i++)
            for (int j = 0; j < d; j++) G[(size_t)i * d + j] -= p[i] * u[j];
        for (int j = 0; j < d; j++) u[j] = dot(&G[(size_t)j * d], w.data(), d);  // (M w)
        for (int i = 0; i < d; i++)
            for (int j = 0; j < d; j++) G[(size_t)i * d + j] -= u[i] * p[j];
        for (int j = 0; j < d; j++) W[(size_t)j * k + a] = w[j], P[(size_t)j * k + a] = p[j];
    }
    std::vector<double> ptw((size_t)k * k);
    for (int i = 0; i < k; i++)
        for (int j = 0; j < k; j++) {
            long double acc = 0.0L;
            for (int r = 0; r < d; r++) acc += (long double)P[(size_t)r * k + i] * (long double)W[(size_t)r * k + j];
            ptw[(size_t)i * k + j] = (double)acc;
        }
    if (!invert_small(ptw, k)) return kConstant;
    for (int r = 0; r < d; r++)
        for (int j = 0; j < k; j++) {
            long double acc = 0.0L;
            for (int i = 0; i < k; i++) acc += (long double)W[(size_t)r * k + i] * (long double)ptw[(size_t)i * k + j];
            rot[(size_t)r * k + j] = (double)acc;
        }
    return kOk;
}

// C ((d + 1) x (d + 1), row-major, the lower triangle is read): the unscaled centred Gram matrix of [X | y] over n rows, and the
// d + 1 column means.  Standard deviations sqrt(C_jj / (n - 1)), a zero replaced by 1 as in kpls.py; a column whose spread is
// below the rounding of its own mean (C_jj <= n (8 eps |mean_j|)^2: the centred values are what the subtraction of a rounded mean
// leaves of a constant) counts as zero, and its row and column of G are exactly zero, so that its row of the rotations is.  A
// response that is constant up to rounding (std <= 1e-12 max(1, |mean|), kpls.py's first test) gives zeros and kConstant.
inline int rotations_from_centred(const double *C, const double *mean, int64_t n, int d, int k, double *rot) {
    const double eps = std::numeric_limits<double>::epsilon();
    const int d1 = d + 1;
    for (size_t e = 0; e < (size_t)d * k; e++) rot[e] = 0.0;
    auto spread = [&](int j, bool *flat) {
        const double cjj = C[(size_t)j * d1 + j], tol = 8.0 * eps * std::fabs(mean[j]);
        *flat = !(cjj > (double)n * tol * tol);
        return *flat ? 0.0 : std::sqrt(cjj / (double)(n - 1));
    };
    bool yflat = false;
    const double ys = spread(d, &yflat);
    if (yflat || ys <= 1e-12 * std::fmax(1.0, std::fabs(mean[d]))) return kConstant;
    std::vector<double> sd(d);
    std::vector<char> flat(d);
    for (int j = 0; j < d; j++) {
        bool f = false;
        sd[j] = spread(j, &f);
        flat[j] = f || sd[j] == 0.0;
        if (flat[j]) sd[j] = 1.0;
    }
    std::vector<double> G((size_t)d * d), s(d);
    for (int i = 0; i < d; i++) {
        for (int j = 0; j <= i; j++) {
            const double v = (flat[i] || flat[j]) ? 0.0 : C[(size_t)i * d1 + j] / sd[i] / sd[j];
            G[(size_t)i * d + j] = G[(size_t)j * d + i] = v;
        }
        s[i] = flat[i] ? 0.0 : C[(size_t)d * d1 + i] / sd[i] / ys;
    }
    const double yty = C[(size_t)d * d1 + d] / ys / ys;
    return rotations_from_gram(G, s, yty, n, d, k, rot);
}

}  // namespace pls
}  // namespace egx
