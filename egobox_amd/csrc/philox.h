// The random stream of GP trajectory sampling (egx_gp_sample, egx_random_normals): Philox4x64-10 (Salmon et al., SC'11) with
// the constants numpy.random.Philox uses, and a Box-Muller transform.  Host- and device-compilable (no HIP in here), so that
// a host test checks the raw stream against numpy (tests/test_sample_cpu.py) and the device kernel draws the same numbers.
//
//   key             (seed, 0)
//   Z[i, j]         normal number (i mod 4) of the block with counter (i / 4, j, 0, 0)
//   word -> (0, 1)  u = ((w >> 11) + 0.5) 2^-53
//   Box-Muller      (w0, w1) -> z0 = sqrt(-2 ln u0) cos(2 pi u1), z1 = sqrt(-2 ln u0) sin(2 pi u1); (w2, w3) -> z2, z3 alike
//
// Z[i, j] depends on (seed, i, j) only: the first k trajectories of a sample of more are those of a sample of k.
// (numpy: Philox(key=[k0, k1], counter=[c0, c1, c2, c3]).random_raw(4) is the block of counter (c0 + 1, c1, c2, c3).)
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EGX_PHILOX_FN __host__ __device__ inline
#else
#define EGX_PHILOX_FN inline
#endif

namespace egx {
namespace philox {

constexpr uint64_t kM0 = 0xD2E7470EE14C6C93ull, kM1 = 0xCA5A826395121157ull;  // multipliers
constexpr uint64_t kW0 = 0x9E3779B97F4A7C15ull, kW1 = 0xBB67AE8584CAA73Bull;  // Weyl key increments
constexpr double kTwoPi = 6.283185307179586;                                  // 2 pi rounded (2 * numpy.pi exactly)

EGX_PHILOX_FN uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// out = Philox4x64-10(counter c, key (k0, k1))
EGX_PHILOX_FN void block(const uint64_t c[4], uint64_t k0, uint64_t k1, uint64_t out[4]) {
    uint64_t x0 = c[0], x1 = c[1], x2 = c[2], x3 = c[3];
    for (int r = 0; r < 10; r++) {
        if (r) {
            k0 += kW0;
            k1 += kW1;
        }
        const uint64_t hi0 = mulhi64(kM0, x0), lo0 = kM0 * x0;
        const uint64_t hi1 = mulhi64(kM1, x2), lo1 = kM1 * x2;
        x0 = hi1 ^ x1 ^ k0;
        x1 = lo1;
        x2 = hi0 ^ x3 ^ k1;
        x3 = lo0;
    }
    out[0] = x0, out[1] = x1, out[2] = x2, out[3] = x3;
}

EGX_PHILOX_FN double to_unit(uint64_t w) { return ((double)(w >> 11) + 0.5) * (1.0 / 9007199254740992.0); }

// z[0..3] = the four standard normals of the block with counter (g, j, 0, 0) under key (seed, 0): rows 4 g .. 4 g + 3 of
// column j of Z
EGX_PHILOX_FN void normals4(uint64_t seed, uint64_t g, uint64_t j, double z[4]) {
    const uint64_t c[4] = {g, j, 0, 0};
    uint64_t w[4];
    block(c, seed, 0, w);
    for (int h = 0; h < 2; h++) {
        const double rad = sqrt(-2.0 * log(to_unit(w[2 * h])));
        const double ang = kTwoPi * to_unit(w[2 * h + 1]);
        z[2 * h] = rad * cos(ang);
        z[2 * h + 1] = rad * sin(ang);
    }
}

}  // namespace philox
}  // namespace egx
