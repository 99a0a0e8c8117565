// Host driver for egobox_amd/csrc/philox.h (tests/test_sample_cpu.py): reads lines from stdin and answers each on stdout
//   B k0 k1 c0 c1 c2 c3   -> the four 64-bit words of the Philox4x64-10 block, hex
//   N seed g j            -> the four normals of block (g, j, 0, 0) under key (seed, 0), %.17g
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "philox.h"

int main() {
    char tag[4];
    while (std::scanf("%3s", tag) == 1) {
        if (std::strcmp(tag, "B") == 0) {
            uint64_t k0, k1, c[4], w[4];
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &k0, &k1, &c[0], &c[1], &c[2],
                           &c[3]) != 6)
                return 2;
            egx::philox::block(c, k0, k1, w);
            std::printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", w[0], w[1], w[2], w[3]);
        } else if (std::strcmp(tag, "N") == 0) {
            uint64_t seed, g, j;
            double z[4];
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &seed, &g, &j) != 3) return 2;
            egx::philox::normals4(seed, g, j, z);
            std::printf("%.17g %.17g %.17g %.17g\n", z[0], z[1], z[2], z[3]);
        } else {
            return 1;
        }
    }
    return 0;
}
