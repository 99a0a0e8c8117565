// The ACTIVE COORDINATES of an infill handle (egx_infill_set_active; CoEGO, crates/ego/src/solver/coego.rs), without HIP: while an
// activity is set a trial point is a COMPACT row of n_active values, value j standing for column active[j] of a full row whose
// other columns are those of x_base.  Here: the argument check with its messages, the expansion of compact rows to full rows,
// and the gather of the active columns of full-width gradient rows.  Both are plain copies: no value is recomputed, so what a
// compact call returns is bit for bit the full-width call's value and its listed gradient columns.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace egx {
namespace active {

// n_active distinct indices in [0, d), 1 <= n_active <= d, in any order; d finite base values.  false with the message in msg
inline bool check(const int32_t *active, int32_t n_active, const double *x_base, int d, std::string &msg) {
    if (n_active < 1 || n_active > d) {
        msg = "infill active: n_active must be 1 .. " + std::to_string(d) + ", got " + std::to_string(n_active);
        return false;
    }
    if (!active || !x_base) {
        msg = "infill active: NULL index list or base point";
        return false;
    }
    std::vector<int32_t> first((size_t)d, -1);  // where an index was listed first
    for (int32_t j = 0; j < n_active; j++) {
        const int32_t c = active[j];
        if (c < 0 || c >= d) {
            msg = "infill active: entry " + std::to_string(j) + " is " + std::to_string(c) + ", not a column in [0, " + std::to_string(d) + ")";
            return false;
        }
        if (first[(size_t)c] >= 0) {
            msg = "infill active: entry " + std::to_string(j) + " repeats column " + std::to_string(c) + " of entry " +
                  std::to_string(first[(size_t)c]);
            return false;
        }
        first[(size_t)c] = j;
    }
    for (int i = 0; i < d; i++)
        if (!std::isfinite(x_base[i])) {
            msg = "infill active: x_base " + std::to_string(i) + " is not finite";
            return false;
        }
    return true;
}

// m compact rows (m x n_active) -> m full rows (m x d): x_base with value j of a row in column active[j]
inline void expand(const double *xc, int64_t m, const std::vector<int> &active, const std::vector<double> &x_base, double *full) {
    const size_t a = active.size(), d = x_base.size();
    for (int64_t i = 0; i < m; i++) {
        double *row = full + (size_t)i * d;
        for (size_t k = 0; k < d; k++) row[k] = x_base[k];
        for (size_t j = 0; j < a; j++) row[(size_t)active[j]] = xc[(size_t)i * a + j];
    }
}

// `rows` full-width rows (rows x d) -> their columns active[0 .. n_active) in that order (rows x n_active)
inline void gather(const double *full, int64_t rows, int d, const std::vector<int> &active, double *out) {
    const size_t a = active.size();
    for (int64_t i = 0; i < rows; i++)
        for (size_t j = 0; j < a; j++) out[(size_t)i * a + j] = full[(size_t)i * d + (size_t)active[j]];
}

}  // namespace active
}  // namespace egx
