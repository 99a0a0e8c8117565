// Mixed-integer design spaces as arithmetic on ONE point: the cast of a continuously relaxed query to its nearest admissible
// discrete point, and the fold / unfold between the user's columns and the relaxed ones.  Plain C++17 behind a host / device
// macro (as infill_math.h): g++ compiles it for the CPU suite (tests/c_host/mixint_test.cpp), k_normalize_queries
// (kernels_corr.hip), k_infill_prepare (kernels_infill.hip) and the k_gmx_probas pair (kernels_gmm.hip) use the same text, and so do
// the host loops that read a query's coordinates (gp_predict.hip): rounding, comparison and selection are exact, host and device
// agree bit for bit.  Paths are relative to the reference checkout (crates/ego/src/gpmix/mixint.rs).
//
// A spec is nx typed columns; its UNFOLDED (continuously relaxed) dimension is d = sum (Enum(v) ? v : 1).
//
//   cast (unfolded -> unfolded)    cast_to_discrete_values_mut :167-201
//       Float   unchanged
//       Int     round half away from zero (f64::round), sign of zero kept: round(-0.3) = -0.0.  No clamping to the bounds (none there)
//       Ord     the value with the smallest |x - v|; the FIRST one in list order wins a tie (ndarray-stats' argmin leaves the tie
//               unspecified: first-wins is this library's definition)
//       Enum    the group becomes the one-hot of its FIRST maximum
//       a NaN / +-inf coordinate of an Int or Ord column stays as it is; an Enum group with a non-finite entry becomes all NaN (the
//       reference panics): a non-finite point stays non-finite, so predict's NaN-in / NaN-out and infill's +inf rule hold
//   unfold (folded -> unfolded)    unfold_with_enum_mask :116-144    the enum index (usize)x becomes a one-hot group; an index outside
//                                  [0, v) or a non-finite one is refused (mixint_unfold_row returns the folded column)
//   fold (unfolded -> folded)      fold_with_enum_index :77-96       the index of the group's first maximum (a non-finite group: NaN)
//   to_discrete                    cast, then fold :220-226
//   continuous limits              as_continuous_limits :38-67       Ord: min / max of its values; Enum: [0, 1] per level
//
// WHERE THE REFERENCE IS NOT FOLLOWED.  Its fold slices the unfolded row at j..j+v with j the FOLDED index (:89) and its unfold
// reads the non-enum columns at the UNFOLDED index (:126).  Both are right only while no Enum column precedes the column in
// question, where folded and unfolded index are the same number.  So fold agrees with what is coded here on specs with at most
// one Enum column (nothing precedes the only group: the reference's own test spec [Float, Enum(3), Int, Ord] is one), and unfold
// on specs whose Enum columns all come LAST or that have none; on that test spec unfold would read Int / Ord at the columns 4 / 5
// of a 4-column row.  Here fold reads at the unfolded index and unfold at the folded one, which is what both mean to do.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EGX_MI_HD __host__ __device__ inline
#else
#define EGX_MI_HD inline
#endif

namespace egx {
namespace mixint {

enum Kind { kFloat = 0, kInt = 1, kOrd = 2, kEnum = 3 };  // egx_xtype_kind

// One UNFOLDED column of a spec, 16 bytes: what a kernel reads per coordinate.  g0 = the first unfolded column of the spec
// column it belongs to (its own index unless Enum), gn = levels (Enum) or number of values (Ord), off = the first of its values in
// the spec's value list (Ord).  A device table is d of these followed by the values (as doubles, 8-byte aligned behind them).
struct Col {
    int32_t kind, g0, gn, off;
};
EGX_MI_HD const double *table_values(const Col *cols, int d) { return reinterpret_cast<const double *>(cols + d); }

EGX_MI_HD bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // false for NaN and +-inf

// f64::round: trunc is exact, and so is x - trunc(x); NaN and +-inf fall through the comparison and come back as they are
EGX_MI_HD double round_half_away(double x) {
    const double t = trunc(x);
    return (fabs(x - t) >= 0.5) ? t + copysign(1.0, x) : t;
}

// take_closest :156-162 with the first minimum; a non-finite x stays
EGX_MI_HD double nearest_value(const double *vals, int n, double x) {
    if (!finite(x)) return x;
    int best = 0;
    double bd = fabs(x - vals[0]);
    for (int i = 1; i < n; i++) {
        const double dd = fabs(x - vals[i]);
        if (dd < bd) bd = dd, best = i;
    }
    return vals[best];
}

// index of the first maximum of the n entries g[0], g[stride], ..; -1 when one of them is not finite
EGX_MI_HD int first_max(const double *g, int n, int64_t stride) {
    int best = 0;
    double bv = g[0];
    bool ok = finite(bv);
    for (int i = 1; i < n; i++) {
        const double v = g[(int64_t)i * stride];
        ok = ok && finite(v);
        if (v > bv) bv = v, best = i;
    }
    return ok ? best : -1;
}

// coordinate k (unfolded) of the cast of the point whose unfolded coordinates are row[0], row[stride], ..
EGX_MI_HD double cast_coord(const Col *cols, const double *vals, const double *row, int64_t stride, int k) {
    const Col c = cols[k];
    const double x = row[(int64_t)k * stride];
    if (c.kind == kInt) return round_half_away(x);
    if (c.kind == kOrd) return nearest_value(vals + c.off, c.gn, x);
    if (c.kind == kEnum) {
        const int im = first_max(row + (int64_t)c.g0 * stride, c.gn, stride);
        return im < 0 ? NAN : (im == k - c.g0 ? 1.0 : 0.0);
    }
    return x;
}

// ---- whole rows (the C ABI's host helpers; d unfolded columns, nx folded ones) --------------------------------------------------
EGX_MI_HD void cast_row(const Col *cols, const double *vals, int d, const double *x, double *out) {
    for (int k = 0; k < d; k++) out[k] = cast_coord(cols, vals, x, 1, k);
}
// out (nx) from x (d): cols[u].g0 == u marks the first unfolded column of a spec column
EGX_MI_HD void fold_row(const Col *cols, int d, const double *x, double *out) {
    int j = 0;
    for (int u = 0; u < d; j++) {
        if (cols[u].kind == kEnum) {
            const int im = first_max(x + u, cols[u].gn, 1);
            out[j] = im < 0 ? NAN : (double)im;
            u += cols[u].gn;
        } else {
            out[j] = x[u++];
        }
    }
}
// out (d) from x (nx); returns -1, or the folded column whose enum index is non-finite or outside [0, v)
EGX_MI_HD int unfold_row(const Col *cols, int d, const double *x, double *out) {
    int j = 0;
    for (int u = 0; u < d; j++) {
        if (cols[u].kind == kEnum) {
            const int v = cols[u].gn;
            const double xi = x[j];
            if (!finite(xi) || xi < 0.0 || !(trunc(xi) < (double)v)) return j;
            const int idx = (int)xi;  // `as usize` truncates
            for (int l = 0; l < v; l++) out[u + l] = (l == idx) ? 1.0 : 0.0;
            u += v;
        } else {
            out[u++] = x[j];
        }
    }
    return -1;
}

}  // namespace mixint
}  // namespace egx
