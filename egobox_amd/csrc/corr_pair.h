// Device-side pieces of the kernels that evaluate the correlation over a 64 x 64 tile of point pairs, shared by kernels_corr.hip
// (correlation matrices, posterior mean, dense theta-gradient, x-gradients), sgp_grad.hip (the sparse model's rectangular
// theta- and inducing-point gradients) and kernels_pending.hip (PairAcc, xgrad_factor).  In the order a tile kernel uses them:
//   tri_tile                         a lower-triangle tile index -> (row block, column block)
//   stage_slab, stage_pair           a 64-point slab (a pair of them, behind a barrier) into LDS
//   exp_nonpos, PairAcc              the exponential of a non-positive argument, the per-pair accumulator
//   tile_pairs_acc, tile_pairs       the 4 x 4 micro-tile of pairs per lane over staged dimensions
//   tile_pairs_staged                ... over all d dimensions of a tile, staged dc at a time
//   srow_step                        the scalar-row forms' step: sixteen wave-uniform rows against the lane's column
//   rect_weights                     wp = T[i, j] r inside an n x nz rectangle (the sparse gradients)
//   rcp_ge1, dlog_dc, xgrad_factor   d log r / d c and d r / d x of one dimension
//   wg_sum_dk, sum_partial_vectors   the workgroup's DK sums and the partial vectors' sum, each in a fixed order
// Every kernel that calls one of them gets the SAME expressions in the same order: the tests assert equal bits across kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/egx_gp.h"

namespace egx {

constexpr double kSqrt3 = 1.7320508075688772;
constexpr double kSqrt5 = 2.23606797749979;
constexpr double k5over3 = 5.0 / 3.0;

// Tile t of the lower triangle, counted row by row (t = bi (bi + 1) / 2 + bj, bj <= bi) -> its row and column block: the
// square root lands within one of bi, the two loops correct it whatever its rounding
__device__ __forceinline__ void tri_tile(int t, int &bi, int &bj) {
    bi = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while (bi * (bi + 1) / 2 > t) bi--;
    while ((bi + 1) * (bi + 2) / 2 <= t) bi++;
    bj = t - bi * (bi + 1) / 2;
}

// exp(x) for x <= 0 (every correlation is exp of a non-positive sum): round-to-nearest range reduction x = k ln2 + r,
// |r| <= ln2 / 2, degree-13 Taylor polynomial in Horner form (truncation 4e-18, all FMA), one v_ldexp_f64: ~20 VALU
// instructions and no branches or selects, against ~30 of the library exp with its special-case handling.  K1 is bound
// by FP64 VALU issue (profiles/r03_*_pmc_corr_*), so instructions per pair are what counts.  Error <= 2 ulp; underflow
// goes through ldexp (gradual, then 0); NaN propagates.
__device__ __forceinline__ double exp_nonpos(double x) {
    // exp(x) == 0 below -745.2: the clamp keeps -inf (a huge theta: the sum overflows) from turning into NaN in the
    // reduction (fma(-inf, -c, -inf)), keeps the cast of kf defined, and lets v_ldexp flush the result to 0 as the reference's
    // exp does.  A select, not fmax: a NaN argument must stay NaN (v_max_f64 would return the other operand).
    x = (x < -800.0) ? -800.0 : x;
    const double kf = __builtin_rint(x * 1.4426950408889634074);
    double r = __builtin_fma(kf, -6.93147180369123816490e-01, x);
    r = __builtin_fma(kf, -1.90821492927058770002e-10, r);
    double p = 1.6059043836821614599e-10;                  // 1 / 13!
    p = __builtin_fma(p, r, 2.0876756987868098979e-09);    // 1 / 12!
    p = __builtin_fma(p, r, 2.5052108385441718775e-08);    // 1 / 11!
    p = __builtin_fma(p, r, 2.7557319223985890653e-07);    // 1 / 10!
    p = __builtin_fma(p, r, 2.7557319223985892511e-06);    // 1 / 9!
    p = __builtin_fma(p, r, 2.4801587301587301566e-05);    // 1 / 8!
    p = __builtin_fma(p, r, 1.9841269841269841253e-04);    // 1 / 7!
    p = __builtin_fma(p, r, 1.3888888888888889419e-03);    // 1 / 6!
    p = __builtin_fma(p, r, 8.3333333333333332177e-03);    // 1 / 5!
    p = __builtin_fma(p, r, 4.1666666666666664354e-02);    // 1 / 4!
    p = __builtin_fma(p, r, 1.6666666666666665741e-01);    // 1 / 3!
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return __builtin_ldexp(p, (int)kf);
}

// Accumulator for one (i, j) pair, updated one input dimension at a time.
template <int CORR>
struct PairAcc {
    double s;  // sum inside the exponential
    double a;  // polynomial product (Matern)
    __device__ __forceinline__ PairAcc() : s(0.0), a(1.0) {}
    __device__ __forceinline__ void add(double diff, const double *__restrict__ coef, int hcols) {
        const double ad = fabs(diff);
        if (CORR == EGX_CORR_SQUARED_EXPONENTIAL) {
            const double t = coef[0] * diff;
            s = __builtin_fma(t, t, s);
        } else if (CORR == EGX_CORR_ABSOLUTE_EXPONENTIAL) {
            s = __builtin_fma(coef[0], ad, s);
        } else if (CORR == EGX_CORR_MATERN32) {
            for (int l = 0; l < hcols; l++) {
                const double t = coef[l] * ad;
                s += t;
                a *= __builtin_fma(kSqrt3, t, 1.0);
            }
        } else {
            for (int l = 0; l < hcols; l++) {
                const double t = coef[l] * ad;
                s += t;
                a *= 1.0 + kSqrt5 * t + k5over3 * (t * t);
            }
        }
    }
    // the same with the coefficient already applied to both coordinates (hcols == 1: diff = c x_i - c x_j, so that
    // c |x_i - x_j| costs no instruction per pair; the rounding of the two products perturbs the exponent by
    // <= 2 eps sum_k |t_k| max |c x|, below 1e-13 wherever r is not negligible): 2 VALU instructions per pair and dimension
    // for the squared exponential instead of 3, 5 instead of 8 for Matern-5/2
    __device__ __forceinline__ void add_scaled(double diff) {
        if (CORR == EGX_CORR_SQUARED_EXPONENTIAL) {
            s = __builtin_fma(diff, diff, s);
        } else if (CORR == EGX_CORR_ABSOLUTE_EXPONENTIAL) {
            s += fabs(diff);
        } else if (CORR == EGX_CORR_MATERN32) {
            const double t = fabs(diff);
            s += t;
            a *= __builtin_fma(kSqrt3, t, 1.0);
        } else {
            const double t = fabs(diff);
            s += t;
            a *= __builtin_fma(__builtin_fma(k5over3, t, kSqrt5), t, 1.0);
        }
    }
    __device__ __forceinline__ double value() const {
        if (CORR == EGX_CORR_SQUARED_EXPONENTIAL) return exp_nonpos(-0.5 * s);
        if (CORR == EGX_CORR_ABSOLUTE_EXPONENTIAL) return exp_nonpos(-s);
        if (CORR == EGX_CORR_MATERN32) return a * exp_nonpos(-kSqrt3 * s);
        return a * exp_nonpos(-kSqrt5 * s);
    }
};

// Stage a 64-point slab (all d dimensions, k-major) into LDS: dst[k*64 + i]; scale != nullptr: times scale[k]
// (PairAcc::add_scaled, hcols == 1).
__device__ __forceinline__ void stage_slab(double *dst, const double *__restrict__ xT, int64_t ldx, int i0,
                                           int d, int tid, const double *__restrict__ scale = nullptr, int nthreads = 256) {
    for (int e = tid; e < d * 64; e += nthreads) {
        const int k = e >> 6, i = e & 63;
        const double v = xT[(int64_t)k * ldx + i0 + i];
        dst[e] = scale ? scale[k] * v : v;
    }
}
// Points i0 .. i0 + 63 of a k-major array (its first staged dimension at xT, the next one ld doubles on): what a slab is staged from
struct SlabSrc {
    const double *xT;
    int64_t ld;
    int i0;
    __device__ __forceinline__ SlabSrc from(int k) const { return {xT + (int64_t)k * ld, ld, i0}; }  // the same from dimension k on
};
// Stage a pair of slabs, `dn` dimensions each, behind a barrier; lead: and a barrier in front (the previous readers of the
// slabs are done)
__device__ __forceinline__ void stage_pair(double *xi, double *xj, SlabSrc si, SlabSrc sj, int dn, int tid, bool lead,
                                           const double *__restrict__ scale = nullptr, int nthreads = 256) {
    if (lead) __syncthreads();
    stage_slab(xi, si.xT, si.ld, si.i0, dn, tid, scale, nthreads);
    stage_slab(xj, sj.xT, sj.ld, sj.i0, dn, tid, scale, nthreads);
    __syncthreads();
}

// 4x4 micro-tile of pair accumulators from two staged slabs: `dn` more dimensions (coef already points at the first one)
template <int CORR, bool PRE = false, int RI = 4>  // PRE: the slabs were staged with the coefficients applied (hcols == 1);
                                                    // RI x 4 pairs per lane (rows RI ty + a, columns 4 tx + b)
__device__ __forceinline__ void tile_pairs_acc(const double *xi, const double *xj, const double *__restrict__ coef,
                                               int hcols, int dn, int ty, int tx, PairAcc<CORR> (&acc)[RI][4]) {
    for (int k = 0; k < dn; k++) {
        double vi[RI], vj[4];
#pragma unroll
        for (int a = 0; a < RI; a++) vi[a] = xi[k * 64 + ty * RI + a];
#pragma unroll
        for (int b = 0; b < 4; b++) vj[b] = xj[k * 64 + tx * 4 + b];
        const double *ck = coef + k * hcols;
#pragma unroll
        for (int a = 0; a < RI; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                if (PRE) acc[a][b].add_scaled(vi[a] - vj[b]);
                else acc[a][b].add(vi[a] - vj[b], ck, hcols);
            }
    }
}
template <int CORR, bool PRE = false, int RI = 4>
__device__ __forceinline__ void tile_pairs(const double *xi, const double *xj, const double *__restrict__ coef,
                                           int hcols, int d, int ty, int tx, double (&r)[RI][4]) {
    PairAcc<CORR> acc[RI][4];
    tile_pairs_acc<CORR, PRE, RI>(xi, xj, coef, hcols, d, ty, tx, acc);
#pragma unroll
    for (int a = 0; a < RI; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) r[a][b] = acc[a][b].value();
}
// All d dimensions of a tile, staged dc at a time (si / sj at dimension 0): the pair accumulators run on across the chunks.
// scale != nullptr: the slabs are staged times scale[k] (PRE).  lead_first: whether the first chunk, too, gets a barrier in
// front -- a kernel that walks several tiles needs it, one that stages into untouched LDS does not.  ty, tx: the kernel's own
// (tid >> 4, tid & 15), handed in as tile_pairs_acc takes them: derived again in here, the same values cost eight
// instantiations up to 20 VGPRs and a wave per SIMD (profiles/pair_tile_ab.txt).
template <int CORR, bool PRE = false, int RI = 4>
__device__ __forceinline__ void tile_pairs_staged(double *xi, double *xj, SlabSrc si, SlabSrc sj, int d, int dc,
                                                  const double *__restrict__ coef, int hcols, int tid, int ty, int tx, bool lead_first,
                                                  PairAcc<CORR> (&acc)[RI][4], const double *__restrict__ scale = nullptr,
                                                  int nthreads = 256) {
    for (int c0 = 0; c0 < d; c0 += dc) {
        const int dn = (d - c0 < dc) ? (d - c0) : dc;
        stage_pair(xi, xj, si.from(c0), sj.from(c0), dn, tid, lead_first || c0, scale ? scale + c0 : nullptr, nthreads);
        tile_pairs_acc<CORR, PRE, RI>(xi, xj, coef + (int64_t)c0 * hcols, hcols, dn, ty, tx, acc);
    }
}

// The step of the scalar-row forms (k_corr_sym_srow, k_predict_mean_srow): one dimension of sixteen rows, wave-uniform at
// xr[0 .. 15] (prescaled; fetched by the scalar unit), against the lane's own prescaled column coordinate v
template <int CORR>
__device__ __forceinline__ void srow_step(const double *xr, double v, PairAcc<CORR> (&acc)[16]) {
    const double4 r0 = *reinterpret_cast<const double4 *>(xr);
    const double4 r1 = *reinterpret_cast<const double4 *>(xr + 4);
    const double4 r2 = *reinterpret_cast<const double4 *>(xr + 8);
    const double4 r3 = *reinterpret_cast<const double4 *>(xr + 12);
    const double r[16] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w};
#pragma unroll
    for (int a = 0; a < 16; a++) acc[a].add_scaled(r[a] - v);
}

// d log r / d c for one dimension (a = |x_i - x_j|, t = c a): the forms of kernels_corr.hip K7
__device__ __forceinline__ double rcp_ge1(double m) {  // 1 / m for m >= 1 (finite), <= 1 ulp-ish
    double y = __builtin_amdgcn_rcp(m);
    double e = __builtin_fma(-m, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-m, y, 1.0);
    return __builtin_fma(y, e, y);
}
template <int CORR>
__device__ __forceinline__ double dlog_dc(double c, double a) {
    if (CORR == EGX_CORR_SQUARED_EXPONENTIAL) return -c * a * a;
    if (CORR == EGX_CORR_ABSOLUTE_EXPONENTIAL) return -a;
    const double t = c * a;
    if (CORR == EGX_CORR_MATERN32) return -3.0 * a * t * rcp_ge1(__builtin_fma(kSqrt3, t, 1.0));
    const double u = __builtin_fma(kSqrt5, t, 1.0);
    return -k5over3 * (a * t) * u * rcp_ge1(__builtin_fma(k5over3 * t, t, u));
}

// d r / d x_k = r * xgrad_factor(x_ak - x_jk) (the closed forms above k_xgrad, kernels_corr.hip); shared with kernels_pending.hip
template <int CORR>
__device__ __forceinline__ double xgrad_factor(double diff, const double *__restrict__ c, int hcols) {
    if (CORR == EGX_CORR_SQUARED_EXPONENTIAL) return -(c[0] * c[0]) * diff;
    if (CORR == EGX_CORR_ABSOLUTE_EXPONENTIAL) return -copysign(c[0], diff);
    const double ad = fabs(diff);
    double sacc = 0.0;
    for (int l = 0; l < hcols; l++) {
        const double t = c[l] * ad;
        if (CORR == EGX_CORR_MATERN32)
            sacc += c[l] * (kSqrt3 / __builtin_fma(kSqrt3, t, 1.0) - kSqrt3);
        else
            sacc += c[l] * ((kSqrt5 + 2.0 * k5over3 * t) / (1.0 + kSqrt5 * t + k5over3 * (t * t)) - kSqrt5);
    }
    return copysign(1.0, diff) * sacc;
}

// The pair weights of the sparse model's two gradient kernels: wp[a][b] = T[i, j] r(i, j) for pair (i, j) = (i0 + 4 ty + a,
// j0 + 4 tx + b) inside the n x nz rectangle, else 0 (T: row-major, ldt, padded to whole tiles)
template <int CORR>
__device__ __forceinline__ void rect_weights(const PairAcc<CORR> (&pa)[4][4], const double *__restrict__ T, int64_t ldt, int i0,
                                             int j0, int n, int nz, int ty, int tx, double (&wp)[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int i = i0 + ty * 4 + a;
        const double *trow = T + (int64_t)i * ldt + j0 + tx * 4;
        const double2 t01 = *reinterpret_cast<const double2 *>(trow);
        const double2 t23 = *reinterpret_cast<const double2 *>(trow + 2);
        const double tv[4] = {t01.x, t01.y, t23.x, t23.y};
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int j = j0 + tx * 4 + b;
            wp[a][b] = (i < n && j < nz) ? pa[a][b].value() * tv[b] : 0.0;
        }
    }
}

// One reduction per workgroup of 256: acc[oo] summed over the lanes of a wave (xor shuffles), then over the four waves in a
// fixed order through red (4 x DK doubles of LDS, which the slabs' last readers must be allowed to give up: a barrier comes
// first).  Thread tid < DK returns the sum of acc[tid]; the others return 0.
template <int DK>
__device__ __forceinline__ double wg_sum_dk(const double (&acc)[DK], double *red, int tid) {
    __syncthreads();
#pragma unroll
    for (int oo = 0; oo < DK; oo++) {
        double v = acc[oo];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((tid & 63) == 0) red[(tid >> 6) * DK + oo] = v;
    }
    __syncthreads();
    return tid < DK ? ((red[tid] + red[DK + tid]) + red[2 * DK + tid]) + red[3 * DK + tid] : 0.0;
}

// Entry o of the sum of nwg partial vectors (nout_pad apart), in a fixed order: the 256 lanes of the workgroup take every
// 256th, then a tree in LDS.  Thread 0 returns the sum.
__device__ __forceinline__ double sum_partial_vectors(const double *__restrict__ part, int nwg, int nout_pad, int o, int tid) {
    __shared__ double red[256];
    double v = 0.0;
    for (int b = tid; b < nwg; b += 256) v += part[(int64_t)b * nout_pad + o];
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

}  // namespace egx
