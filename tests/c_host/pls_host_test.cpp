// Stand-alone host test of egobox_amd/csrc/pls_host.h (no HIP): the launch plan, the d-space PLS recursion against cases the
// Python test writes (G, s, y^T y from numpy; the expected rotations from its long-double NIPALS), the three places that report a
// constant response, and the scaling of an unscaled centred Gram matrix with a constant column.  tests/test_pls_cpu.py builds it
// plain and with -fsanitize=address,undefined.
//
// Case file (float64, native order): count, then per case  n d k | G (d*d) | s (d) | yty | expected (d*k).
// Output: "case <i> err <e>" per case (the sign-insensitive column error of tests/pls_oracle.py), "ok <what>" per check, "OK".
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <string>
#include <vector>

#include "../../egobox_amd/csrc/pls_host.h"

using namespace egx;

static int failures = 0;
#define CHECK(cond, what)                                  \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAIL %s (line %d)\n", what, __LINE__); \
            failures++;                                    \
        }                                                  \
    } while (0)

static double col_err(const std::vector<double> &w, const std::vector<double> &ref, int d, int k) {
    double worst = 0.0;
    for (int j = 0; j < k; j++) {
        double scale = 0.0, ep = 0.0, em = 0.0, wmax = 0.0;
        for (int r = 0; r < d; r++) {
            scale = std::fmax(scale, std::fabs(ref[(size_t)r * k + j]));
            ep = std::fmax(ep, std::fabs(w[(size_t)r * k + j] - ref[(size_t)r * k + j]));
            em = std::fmax(em, std::fabs(w[(size_t)r * k + j] + ref[(size_t)r * k + j]));
            wmax = std::fmax(wmax, std::fabs(w[(size_t)r * k + j]));
        }
        worst = std::fmax(worst, scale == 0.0 ? wmax : std::fmin(ep, em) / scale);
    }
    return worst;
}

static bool read_doubles(std::FILE *f, double *p, size_t cnt) { return std::fread(p, sizeof(double), cnt, f) == cnt; }

static void test_plan() {
    egx_pls_plan p{};
    CHECK(!pls::plan(0, 3, &p) && !pls::plan(5, 0, &p) && !pls::plan(5, 3, nullptr), "plan refuses n < 1, d < 1, no output");
    const int64_t ns[] = {1, 2, 63, 64, 255, 256, 257, 300, 600, 4096, 65535, 65536, 65537, 100000, 1000000, 10000019};
    const int64_t ds[] = {1, 3, 15, 16, 17, 63, 64, 65, 127, 128, 130, 1000};
    for (int64_t d : ds) {
        int64_t last_rows = 0;
        for (int64_t n : ns) {
            CHECK(pls::plan(n, d, &p), "plan");
            CHECK(p.chunk_rows % 64 == 0 && p.chunk_rows >= last_rows, "chunk_rows: a multiple of 64 that does not shrink with n");
            last_rows = p.chunk_rows;
            // every row once, no chunk empty
            int64_t covered = 0;
            for (int64_t c = 0; c < p.n_chunks; c++) {
                const int64_t r0 = c * p.chunk_rows, r1 = (r0 + p.chunk_rows < n) ? r0 + p.chunk_rows : n;
                CHECK(r0 == covered && r1 > r0, "chunks are consecutive and not empty");
                covered = r1;
            }
            CHECK(covered == n, "chunks cover the n rows");
            CHECK(p.n_chunks <= pls::kMaxChunks, "chunks bounded");
            CHECK(p.tiles * 16 >= d + 1 && (p.tiles - 1) * 16 < d + 1, "tiles cover d + 1 columns");
            CHECK(p.out_tiles == p.tiles * (p.tiles + 1) / 2, "lower-triangle tiles");
            CHECK(p.block_side * 64 >= d + 1 && (p.block_side - 1) * 64 < d + 1 && p.blocks == p.block_side * (p.block_side + 1) / 2,
                  "blocks");
        }
    }
    egx_pls_plan a{}, b{};
    for (int64_t d = 1; d < 300; d++) {
        pls::plan(1000, d, &a);
        pls::plan(1000, d + 1, &b);
        CHECK(b.tiles >= a.tiles && b.out_tiles >= a.out_tiles && b.blocks >= a.blocks, "tiles and blocks do not shrink with d");
    }
    std::printf("ok plan\n");
}

static void test_constant() {
    const int d = 3, k = 2;
    std::vector<double> rot((size_t)d * k, 7.0);
    // (1) a constant response: C_yy = 0
    {
        const int d1 = d + 1;
        std::vector<double> C((size_t)d1 * d1, 0.0), mean(d1, 1.0);
        for (int j = 0; j < d; j++) C[(size_t)j * d1 + j] = 10.0;
        CHECK(pls::rotations_from_centred(C.data(), mean.data(), 11, d, k, rot.data()) == pls::kConstant, "constant response: status");
        for (double v : rot) CHECK(v == 0.0, "constant response: zeros");
    }
    // (2) a residual below the threshold before the first component
    {
        std::vector<double> G = {1, 0, 0, 0, 1, 0, 0, 0, 1}, s = {1, 0, 0};
        rot.assign(rot.size(), 7.0);
        CHECK(pls::rotations_from_gram(G, s, 1e-40, 11, d, k, rot.data()) == pls::kConstant, "tiny residual: status");
        for (double v : rot) CHECK(v == 0.0, "tiny residual: zeros");
    }
    // (3) |s| < eps: y orthogonal to every column
    {
        std::vector<double> G = {1, 0, 0, 0, 1, 0, 0, 0, 1}, s = {0, 0, 0};
        rot.assign(rot.size(), 7.0);
        CHECK(pls::rotations_from_gram(G, s, 10.0, 11, d, k, rot.data()) == pls::kConstant, "|s| < eps: status");
        for (double v : rot) CHECK(v == 0.0, "|s| < eps: zeros");
    }
    // the second component of an exhausted residual: one column explains y exactly
    {
        std::vector<double> G = {10, 0, 0, 0, 10, 0, 0, 0, 10}, s = {10, 0, 0};
        rot.assign(rot.size(), 7.0);
        CHECK(pls::rotations_from_gram(G, s, 10.0, 11, d, k, rot.data()) == pls::kConstant, "exhausted residual: status");
        for (double v : rot) CHECK(v == 0.0, "exhausted residual: zeros");
    }
    std::printf("ok constant response\n");
}

static void test_constant_column() {
    // x0 = (-1, 0, 1), x1 constant (C_11 = rounding of its mean only), y = 2 x0: the rotation is (1 / sd-scaled, 0)
    const int d = 2, k = 1;  // C is 3 x 3
    const double tiny = 3.0 * std::pow(8.0 * 2.220446049250313e-16 * 0.3, 2) * 0.5;
    std::vector<double> C = {2, 0, 0, 1e-17, tiny, 0, 4, 2e-17, 8}, mean = {0.0, 0.3, 0.0}, rot((size_t)d * k, 7.0);
    CHECK(pls::rotations_from_centred(C.data(), mean.data(), 3, d, k, rot.data()) == pls::kOk, "constant column: status");
    CHECK(rot[1] == 0.0, "constant column: its row is exactly zero");
    CHECK(std::fabs(std::fabs(rot[0]) - 1.0) < 1e-14, "constant column: the live row");
    std::printf("ok constant column\n");
}

int main(int argc, char **argv) {
    test_plan();
    test_constant();
    test_constant_column();
    if (argc > 1) {
        std::FILE *f = std::fopen(argv[1], "rb");
        if (!f) {
            std::printf("FAIL cannot open %s\n", argv[1]);
            return 2;
        }
        double cnt = 0.0;
        CHECK(read_doubles(f, &cnt, 1), "case count");
        for (int c = 0; c < (int)cnt; c++) {
            double hdr[3];
            if (!read_doubles(f, hdr, 3)) {
                CHECK(false, "case header");
                break;
            }
            const int64_t n = (int64_t)hdr[0];
            const int d = (int)hdr[1], k = (int)hdr[2];
            std::vector<double> G((size_t)d * d), s((size_t)d), want((size_t)d * k), rot((size_t)d * k);
            double yty = 0.0;
            const bool got = read_doubles(f, G.data(), G.size()) && read_doubles(f, s.data(), s.size()) && read_doubles(f, &yty, 1) &&
                             read_doubles(f, want.data(), want.size());
            if (!got) {
                CHECK(false, "case body");
                break;
            }
            const int st = pls::rotations_from_gram(G, s, yty, n, d, k, rot.data());
            std::printf("case %d status %d err %.17g\n", c, st, col_err(rot, want, d, k));
        }
        std::fclose(f);
        std::printf("ok cases\n");
    }
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures ? 1 : 0;
}
