// csrc/gmm_wide_plan.h -- the shapes of the wide-row mixture EM -- checked on the host for every D in 1..128: the padding,
// the LDS budgets, the deal of the accumulator tiles over the waves, the cover of the rows by tiles and chunks, that the
// plan is a function of (n, D), and the workspace bound.  Stand-alone: prints "ok <what>" lines, then OK.
#include <cstdio>
#include <vector>

#include "../../egobox_amd/csrc/gmm_wide_plan.h"

namespace W = egx::gmm_wide;

static int failures = 0;
#define CHECK(cond, ...)             \
    do {                             \
        if (!(cond)) {               \
            std::printf("FAIL ");    \
            std::printf(__VA_ARGS__); \
            std::printf("\n");       \
            failures++;              \
        }                            \
    } while (0)

static void padding_and_lds() {
    for (int D = 1; D <= W::kMaxDim; D++) {
        const int DP = W::dp_of(D);
        CHECK(DP >= D && DP % W::kTile == 0 && DP - D < W::kTile && DP <= W::kMaxDim, "DP %d of D %d", DP, D);
        CHECK(W::rows_per_tile(DP) == W::kWaves * W::kTile, "rows per tile at DP %d", DP);
        for (int k = 1; k <= 16; k++) CHECK(W::estep_lds_bytes(DP, k) <= W::kLdsLimit, "E-step LDS at DP %d k %d", DP, k);
        CHECK(W::mstep_lds_bytes(D) <= W::kLdsLimit, "M-step LDS at D %d", D);
        // two E-step workgroups on a compute unit up to four clusters
        CHECK(2 * W::estep_lds_bytes(DP, 4) <= W::kLdsLimit, "two workgroups at DP %d", DP);
        CHECK(W::lds_stride(DP) % 32 == 4 || W::lds_stride(DP) % 32 == 20, "LDS stride at DP %d", DP);
    }
    std::printf("ok padding and LDS\n");
}

static void tile_owners() {
    for (int D = 1; D <= W::kMaxDim; D++) {
        const int DP = W::dp_of(D), nt = W::tiles_across(DP), ntri = W::tri_tiles(DP);
        std::vector<int> owned((size_t)nt * nt, 0), slots((size_t)W::kWaves * W::tiles_per_wave(DP), 0);
        for (int w = 0; w < W::kWaves; w++)
            for (int s = 0; s < W::tiles_per_wave(DP); s++) {  // as the kernel walks them
                const int t = w + W::kWaves * s;
                if (t >= ntri) continue;
                int ti = -1, tj = -1;
                W::tile_of(t, ti, tj);
                CHECK(ti >= 0 && ti < nt && tj >= 0 && tj <= ti, "tile %d of DP %d: (%d, %d)", t, DP, ti, tj);
                CHECK(W::tile_index(ti, tj) == t && W::tile_owner(t) == w && W::tile_slot(t) == s, "tile %d of DP %d", t, DP);
                if (ti >= 0 && ti < nt && tj >= 0 && tj < nt) owned[(size_t)ti * nt + tj]++;
                slots[(size_t)w * W::tiles_per_wave(DP) + s]++;
            }
        for (int ti = 0; ti < nt; ti++)
            for (int tj = 0; tj < nt; tj++)
                CHECK(owned[(size_t)ti * nt + tj] == (tj <= ti ? 1 : 0), "DP %d tile (%d, %d) owned %d times", DP, ti, tj,
                      owned[(size_t)ti * nt + tj]);
        for (int v : slots) CHECK(v <= 1, "DP %d: a slot used twice", DP);
        CHECK(W::part_len(DP) == (size_t)ntri * 256 + DP + 1, "part_len at DP %d", DP);
    }
    CHECK(W::tri_tiles(128) == 36 && W::tiles_per_wave(128) == 9, "36 tiles, nine per wave at DP 128");
    std::printf("ok tile owners\n");
}

static void cover_one(int64_t n, int D) {
    const W::Plan p = W::plan(n, D);
    CHECK(p.chunks >= 1 && p.chunks <= W::kMaxChunks && p.tiles_per_chunk >= 1, "n %lld: %lld chunks", (long long)n, (long long)p.chunks);
    CHECK((p.chunks - 1) * p.tiles_per_chunk < p.tiles, "n %lld: an empty chunk", (long long)n);
    int64_t next = 0;
    for (int64_t c = 0; c < p.chunks; c++)
        for (int64_t t = 0; t <= p.tiles_per_chunk; t++) {  // one past the end: refused
            int64_t r0 = -1, r1 = -1;
            if (!W::tile_rows(p, n, c, t, r0, r1)) continue;
            CHECK(r0 == next && r1 > r0 && r1 - r0 <= p.rows && r1 <= n, "n %lld chunk %lld tile %lld: rows [%lld, %lld)", (long long)n,
                  (long long)c, (long long)t, (long long)r0, (long long)r1);
            next = r1;
        }
    CHECK(next == n, "n %lld D %d: rows covered to %lld", (long long)n, D, (long long)next);
    int64_t r0, r1;
    CHECK(!W::tile_rows(p, n, p.chunks, 0, r0, r1), "n %lld: a chunk past the end", (long long)n);
}

static void row_cover() {
    const int64_t tile = W::kTileRows, full = tile * W::kMaxChunks;
    std::vector<int64_t> ns = {1, 2, 7};
    for (int64_t e : {tile, 2 * tile, 4 * tile, 17 * tile, full, 2 * full, 3 * full, 5 * full + 3 * tile})
        for (int64_t d = -2; d <= 2; d++) ns.push_back(e + d);
    for (int64_t n : ns)
        for (int D : {1, 16, 17, 48, 128}) cover_one(n, D);
    std::printf("ok row cover\n");
}

static void depends_on_n_and_d_only() {
    // the plan has no other input; what differs between two widths of one DP is D itself
    for (int64_t n : {1, 64, 65, 4099, 65536, 1000003}) {
        const W::Plan a = W::plan(n, 33), b = W::plan(n, 48), c = W::plan(n, 128);
        CHECK(a.DP == b.DP && a.tiles == b.tiles && a.chunks == b.chunks && a.tiles_per_chunk == b.tiles_per_chunk && a.len == b.len,
              "n %lld: D 33 and 48 share DP 48", (long long)n);
        CHECK(a.tiles == c.tiles && a.chunks == c.chunks && a.tiles_per_chunk == c.tiles_per_chunk, "n %lld: chunking is of n alone",
              (long long)n);
        size_t w1 = 0, w20 = 0;
        CHECK(W::workspace_doubles(a, 1, 4, w1) && W::workspace_doubles(a, 20, 4, w20) && w20 == 20 * w1, "n %lld: workspace in R",
              (long long)n);
    }
    std::printf("ok a function of n and D\n");
}

static void workspace_bound() {
    size_t w = 0;
    const W::Plan p = W::plan(65536, 128);  // 1024 tiles in 256 chunks of 4
    CHECK(p.chunks == 256 && p.tiles_per_chunk == 4, "the bench shape");
    CHECK(W::workspace_doubles(p, 20, 4, w) && w == (size_t)256 * 80 * W::part_len(128) && w <= W::kMaxPartDoubles, "R 20 k 4 fits");
    CHECK(!W::workspace_doubles(p, 20, 16, w), "R 20 k 16 at 256 chunks is 5.6 GiB: refused");
    CHECK(!W::workspace_doubles(p, 2147483647, 16, w), "R at the top of int32: refused, no overflow");
    CHECK(!W::workspace_doubles(p, 0, 4, w), "R 0");
    const W::Plan q = W::plan(64, 128);  // one chunk
    CHECK(W::workspace_doubles(q, 3000, 16, w) && w == (size_t)48000 * W::part_len(128), "one chunk, R 3000");
    CHECK(!W::workspace_doubles(q, 4000, 16, w), "one chunk, R 4000: beyond 4 GiB");
    std::printf("ok workspace bound\n");
}

int main() {
    padding_and_lds();
    tile_owners();
    row_cover();
    depends_on_n_and_d_only();
    workspace_bound();
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
