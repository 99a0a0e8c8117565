// The RUNS of an infill handle's walk, without HIP: which consecutive surrogates go through ONE launch sequence per tile, the
// member a grid coordinate of every kernel of it (infill_eval.hip run_tile).  The rule reads a description of each surrogate
// and nothing else, so it can be tested on described shapes without a device (tests/c_host/infill_runs_test.cpp).
//
// Surrogates js .. js + len - 1 form a run when
//   * each is a lone dense model (no mixture, not sparse),
//   * all have the same n, n_pad, correlation, trend, coefficient columns (fit_hcols) and input weights or none (has_w),
//   * all take the same sequence kind -- the objective always the full one, a constraint the mean-only one exactly when the
//     evaluation is mean_c,
//   * the handle has no pending points (q == 0): with pending points every run has length 1,
//   * len <= kRunMax, and the run's (kTile x n_pad) blocks stay within a bound of doubles.
// A MEAN-ONLY run needs no more: its launches take the members' own pointers, so separately created models of one shape qualify.
// A FULL-sequence run also reads the members' factors, C^-T and -R^-1 F at ONE stride: members of one group in consecutive slots.
// Surrogates are never reordered; same-shape models that are not adjacent do not merge.  A run of one is always allowed.
#pragma once
#include <cstdint>
#include <vector>

namespace egx {
namespace runs {

constexpr int kRunMax = 16;                         // == kLockstepMax: the by-value pointer blocks of the kernels
constexpr int kRunTile = 128;                       // == kTile
constexpr int64_t kRunDoubles = (int64_t)1 << 27;   // the bound of one chunk of the batched posterior (gp_predict.hip), 1 GiB

struct Shape {
    bool lone_dense = true;      // one expert, and that a dense GP
    int n = 0, n_pad = 0, corr = 0, mean = 0, fit_hcols = 1;
    bool has_w = false;
    const void *group = nullptr; // the group the model is a member of, or nullptr
    int slot = -1;               // ... and its slot there
};

// is surrogate j's sequence the mean-only one?  (the objective, j == 0, always runs the full sequence)
inline bool mean_only(int j, bool mean_c) { return j > 0 && mean_c; }

inline bool same_shape(const Shape &a, const Shape &b) {
    return a.n == b.n && a.n_pad == b.n_pad && a.corr == b.corr && a.mean == b.mean && a.fit_hcols == b.fit_hcols && a.has_w == b.has_w;
}

// the length of the run that starts at surrogate js of `count` (>= 1)
inline int run_len(const Shape *s, int count, int js, bool mean_c, int q, int64_t bound_doubles = kRunDoubles) {
    if (!s[js].lone_dense || q > 0) return 1;
    const bool mo = mean_only(js, mean_c);
    const int64_t blk = (int64_t)kRunTile * (s[js].n_pad > 0 ? s[js].n_pad : 1);
    int len = 1;
    while (js + len < count && len < kRunMax) {
        const Shape &c = s[js + len];
        if (!c.lone_dense || !same_shape(s[js], c) || mean_only(js + len, mean_c) != mo) break;
        if (!mo && (!s[js].group || c.group != s[js].group || c.slot != s[js].slot + len)) break;
        if ((int64_t)(len + 1) * blk > bound_doubles) break;
        len++;
    }
    return len;
}

// the runs of a walk over surrogates [0, count), in order
inline std::vector<int> run_lengths(const Shape *s, int count, bool mean_c, int q, int64_t bound_doubles = kRunDoubles) {
    std::vector<int> out;
    for (int js = 0; js < count; js += out.back()) out.push_back(run_len(s, count, js, mean_c, q, bound_doubles));
    return out;
}

}  // namespace runs
}  // namespace egx
