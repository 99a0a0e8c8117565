// Host test of csrc/infill_active.h (g++ alone: no HIP, no library, no GPU): the argument check of egx_infill_set_active with its
// messages, the expansion of compact rows and the gather of the active columns.  One line per check: "ok <group>: <what>" or
// "FAIL ..."; the exit status is the number of failures.
#include <cmath>
#include <cstdio>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "../../egobox_amd/csrc/infill_active.h"

static int failures = 0;
static void report(bool ok, const char *group, const std::string &what) {
    std::printf("%s %s: %s\n", ok ? "ok" : "FAIL", group, what.c_str());
    if (!ok) failures++;
}

static bool refused(const std::vector<int32_t> &a, const std::vector<double> &xb, int d, const std::string &needle) {
    std::string msg;
    const bool ok = egx::active::check(a.data(), (int32_t)a.size(), xb.data(), d, msg);
    return !ok && msg.find(needle) != std::string::npos;
}

// a deterministic shuffle of 0 .. d - 1 (no <random>: the same list everywhere)
static std::vector<int> shuffled(int d, unsigned seed) {
    std::vector<int> v((size_t)d);
    std::iota(v.begin(), v.end(), 0);
    unsigned s = seed;
    for (int i = d - 1; i > 0; i--) {
        s = s * 1664525u + 1013904223u;
        std::swap(v[(size_t)i], v[(size_t)((s >> 8) % (unsigned)(i + 1))]);
    }
    return v;
}

static void round_trip(int d, int a, int64_t m, unsigned seed) {
    std::vector<int> act = shuffled(d, seed);
    act.resize((size_t)a);
    std::vector<double> xb((size_t)d), xc((size_t)(m * a)), full((size_t)(m * d), -1.0), back((size_t)(m * a), -2.0);
    for (int k = 0; k < d; k++) xb[(size_t)k] = 100.0 + k;
    for (size_t i = 0; i < xc.size(); i++) xc[i] = 0.25 * (double)i - 3.0;
    egx::active::expand(xc.data(), m, act, xb, full.data());
    bool placed = true;
    for (int64_t i = 0; i < m; i++) {
        std::vector<bool> listed((size_t)d, false);
        for (int j = 0; j < a; j++) {
            listed[(size_t)act[(size_t)j]] = true;
            placed &= full[(size_t)(i * d + act[(size_t)j])] == xc[(size_t)(i * a + j)];
        }
        for (int k = 0; k < d; k++)
            if (!listed[(size_t)k]) placed &= full[(size_t)(i * d + k)] == xb[(size_t)k];
    }
    egx::active::gather(full.data(), m, d, act, back.data());
    const std::string tag = "d " + std::to_string(d) + " a " + std::to_string(a) + " m " + std::to_string(m);
    report(placed, "expand", tag);
    report(back == xc, "round trip", tag);
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const std::vector<double> xb5 = {0.1, 0.2, 0.3, 0.4, 0.5};
    std::string msg;
    report(egx::active::check(std::vector<int32_t>{4, 0, 2}.data(), 3, xb5.data(), 5, msg), "check", "a shuffled list passes");
    report(egx::active::check(std::vector<int32_t>{3, 1, 4, 0, 2}.data(), 5, xb5.data(), 5, msg), "check", "all d columns pass");
    report(refused({1, 3, 1}, xb5, 5, "entry 2 repeats column 1 of entry 0"), "check", "a duplicate index names both entries");
    report(refused({1, 5}, xb5, 5, "entry 1 is 5"), "check", "an index of d names the entry");
    report(refused({-1}, xb5, 5, "entry 0 is -1"), "check", "a negative index names the entry");
    report(refused({}, xb5, 5, "got 0"), "check", "n_active 0");
    report(refused({0, 1, 2, 3, 4, 0}, xb5, 5, "got 6"), "check", "n_active d + 1");
    report(refused({0}, {0.1, 0.2, nan, 0.4, 0.5}, 5, "x_base 2"), "check", "a NaN base value names the entry");
    report(refused({0}, {0.1, 0.2, 0.3, 0.4, -inf}, 5, "x_base 4"), "check", "an infinite base value names the entry");
    report(!egx::active::check(nullptr, 1, xb5.data(), 5, msg) && !egx::active::check(std::vector<int32_t>{0}.data(), 1, nullptr, 5, msg),
           "check", "NULL arguments");
    round_trip(9, 1, 3, 1u);
    round_trip(9, 9, 3, 2u);
    round_trip(33, 7, 5, 3u);
    round_trip(1, 1, 2, 4u);
    round_trip(72, 33, 129, 5u);
    {  // gather on rows that are not points: (nm * m) rows of a parts table
        const std::vector<int> act = {2, 0};
        const std::vector<double> full = {1, 2, 3, 4, 5, 6};
        std::vector<double> out(4, 0.0);
        egx::active::gather(full.data(), 2, 3, act, out.data());
        report(out == std::vector<double>{3, 1, 6, 4}, "gather", "the list's order, not the columns'");
    }
    return failures;
}
