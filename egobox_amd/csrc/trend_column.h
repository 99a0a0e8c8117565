// The trend f(x) = [1, x_j, x_j x_k (k <= j)] on the device, from the coordinate pairs of host_math.h regression_index and a
// k-major block of normalised queries (xqT[i * ldq + q]: coordinate i of query q).
#pragma once
#include <cstdint>

namespace egx {

// one factor of a column: coordinate i of query q (-1: 1.0)
__device__ inline double trend_factor(const double *xqT, int64_t ldq, int q, int i) {
    return i < 0 ? 1.0 : xqT[(int64_t)i * ldq + q];
}
// column l of f(x_q)
__device__ inline double trend_column(const int *fidx, int l, const double *xqT, int64_t ldq, int q) {
    const int b = fidx[2 * l + 1];
    const double fa = trend_factor(xqT, ldq, q, fidx[2 * l]);
    return b < 0 ? fa : xqT[(int64_t)b * ldq + q] * fa;
}

}  // namespace egx
