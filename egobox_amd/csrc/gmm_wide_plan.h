// The shape decisions of the wide-row Gaussian mixture EM (egx_gmm_fit_wide; kernels_gmm_wide.hip, DESIGN.md 4.8 "Wide rows")
// as plain host arithmetic: no HIP type, so a C++17 program checks them without a device
// (tests/c_host/gmm_wide_plan_test.cpp).  The kernels read the same constants.
//
//   DP      D rounded up to the 16-wide tile of v_mfma_f64_16x16x4_f64; every per-cluster array on the device is padded to
//           it with zeros.
//   tile    kTileRows = 64 rows of the data staged in LDS at row stride DP + 4 doubles (at DP = 128 a 256-row tile would be
//           264 KiB; 64 rows are 66 KiB and leave room for two workgroups on a compute unit up to k = 4).  Wave w of the
//           four owns the tile's rows 16 w .. 16 w + 15 in the Z = (X - mu) P product.
//   chunk   the consecutive tiles one workgroup walks; it adds their moments into ITS slot of the workspace in tile order.
//           tiles_per_chunk = ceil(tiles / kMaxChunks): a function of n alone, so a restart's sums have one order whatever
//           the batch.
//   moments per (chunk, restart, cluster) part_len(DP) doubles: the 16 x 16 tiles of S2's lower triangle, each whole and
//           row-major (element (i, j), j <= i, at 256 tile_index(i / 16, j / 16) + 16 (i % 16) + j % 16: a lane's address is
//           one offset plus constants), then S1 (DP), then the sum of responsibilities.
//   owner   the 16 x 16 accumulator tiles of S2's lower triangle, numbered t = ti (ti + 1) / 2 + tj (tj <= ti), are dealt
//           round-robin: wave t % 4 owns tile t, as its accumulator t / 4.  36 tiles at DP = 128: nine per wave.
#pragma once
#include <cstddef>
#include <cstdint>

namespace egx {
namespace gmm_wide {

constexpr int kTile = 16;        // the MFMA tile
constexpr int kMaxDim = 128;     // D <= DP <= 128
constexpr int kWaves = 4;        // waves of an E-step workgroup
constexpr int kTileRows = 64;    // rows of the data per LDS tile: 16 per wave
constexpr int kLdPad = 4;        // LDS row stride DP + 4: the 16 rows x 4 columns of an A fragment fall on distinct banks
constexpr int kMaxChunks = 256;  // workgroups along the rows: one per compute unit
constexpr size_t kMaxPartDoubles = (size_t)1 << 29;  // 4 GiB of partial moments
constexpr size_t kLdsLimit = 160 * 1024;

constexpr int dp_of(int D) { return (D + kTile - 1) / kTile * kTile; }
constexpr int rows_per_tile(int /*DP*/) { return kTileRows; }
constexpr int tiles_across(int DP) { return DP / kTile; }
constexpr int tri_tiles(int DP) { return tiles_across(DP) * (tiles_across(DP) + 1) / 2; }
constexpr int tiles_per_wave(int DP) { return (tri_tiles(DP) + kWaves - 1) / kWaves; }
constexpr int tile_owner(int t) { return t % kWaves; }
constexpr int tile_slot(int t) { return t / kWaves; }
// t = ti (ti + 1) / 2 + tj, tj <= ti
constexpr void tile_of(int t, int &ti, int &tj) {
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ti++;
    tj = t - ti * (ti + 1) / 2;
}
constexpr int tile_index(int ti, int tj) { return ti * (ti + 1) / 2 + tj; }
constexpr size_t tri_len(int DP) { return (size_t)tri_tiles(DP) * kTile * kTile; }
constexpr size_t part_len(int DP) { return tri_len(DP) + DP + 1; }
constexpr int lds_stride(int DP) { return DP + kLdPad; }
// E-step: the data tile, k rows of log p / responsibilities, the k means
constexpr size_t estep_lds_bytes(int DP, int k) {
    return sizeof(double) * ((size_t)rows_per_tile(DP) * lds_stride(DP) + (size_t)k * rows_per_tile(DP) + (size_t)k * DP);
}
// M-step: the D x D matrix at row stride D + 1 (L below, L^-T above the diagonal), 1 / diag L, delta, the k sums of
// responsibilities, 256 reduction slots
constexpr size_t mstep_lds_bytes(int D) { return sizeof(double) * ((size_t)D * (D + 1) + 2 * (size_t)D + 16 + 256); }

struct Plan {
    int D = 0, DP = 0;
    int rows = 0;                 // rows per tile
    int64_t tiles = 0;            // ceil(n / rows)
    int64_t tiles_per_chunk = 0;  // consecutive tiles of a workgroup
    int64_t chunks = 0;           // workgroups along the rows, <= kMaxChunks
    size_t len = 0;               // part_len(DP)
};

// a function of (n, D) alone
constexpr Plan plan(int64_t n, int D) {
    Plan p;
    p.D = D;
    p.DP = dp_of(D);
    p.rows = rows_per_tile(p.DP);
    p.tiles = (n + p.rows - 1) / p.rows;
    p.tiles_per_chunk = (p.tiles + kMaxChunks - 1) / kMaxChunks;
    if (p.tiles_per_chunk < 1) p.tiles_per_chunk = 1;
    p.chunks = (p.tiles + p.tiles_per_chunk - 1) / p.tiles_per_chunk;
    p.len = part_len(p.DP);
    return p;
}

// rows [row0, row1) of tile `tile_in_chunk` of chunk `chunk`; false beyond the chunk's tiles
constexpr bool tile_rows(const Plan &p, int64_t n, int64_t chunk, int64_t tile_in_chunk, int64_t &row0, int64_t &row1) {
    const int64_t tile = chunk * p.tiles_per_chunk + tile_in_chunk;
    if (tile_in_chunk >= p.tiles_per_chunk || tile >= p.tiles) return false;
    row0 = tile * p.rows;
    row1 = row0 + p.rows < n ? row0 + p.rows : n;
    return true;
}

// chunks x R x k x part_len doubles; false beyond the 4 GiB bound
constexpr bool workspace_doubles(const Plan &p, int64_t R, int64_t k, size_t &doubles) {
    const size_t per_chunk = (size_t)R * (size_t)k * p.len;
    if (R < 1 || k < 1 || per_chunk / p.len != (size_t)R * (size_t)k || per_chunk > kMaxPartDoubles) return false;
    if ((size_t)p.chunks > kMaxPartDoubles / per_chunk) return false;
    doubles = (size_t)p.chunks * per_chunk;
    return doubles <= kMaxPartDoubles;
}

}  // namespace gmm_wide
}  // namespace egx
