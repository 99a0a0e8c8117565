// Host test of csrc/infill_runs.h (g++ alone: no HIP, no library, no GPU): the run rule of an infill handle's walk on described
// surrogates.  One line per check: "ok <what>" or "FAIL ..."; the exit status is the number of failures.
#include <cstdio>
#include <string>
#include <vector>

#include "../../egobox_amd/csrc/infill_runs.h"

using egx::runs::Shape;

static int failures = 0;
static std::string show(const std::vector<int> &v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + std::to_string(v[i]);
    return s + "]";
}
static void expect(const char *what, const std::vector<Shape> &s, bool mean_c, int q, const std::vector<int> &want,
                   int64_t bound = egx::runs::kRunDoubles) {
    const std::vector<int> got = egx::runs::run_lengths(s.data(), (int)s.size(), mean_c, q, bound);
    int sum = 0;
    for (int v : got) sum += v;
    const bool ok = got == want && sum == (int)s.size();
    std::printf("%s %s: %s%s\n", ok ? "ok" : "FAIL", what, show(got).c_str(), ok ? "" : (" expected " + show(want)).c_str());
    if (!ok) failures++;
}

// `count` surrogates of one shape (n = 150: n_pad 256); group != nullptr: members of that group in consecutive slots from 0
static std::vector<Shape> equal(int count, int n, const void *group) {
    std::vector<Shape> s((size_t)count);
    for (int j = 0; j < count; j++) {
        s[(size_t)j].n = n, s[(size_t)j].n_pad = (n + 127) / 128 * 128;
        s[(size_t)j].group = group, s[(size_t)j].slot = group ? j : -1;
    }
    return s;
}

int main() {
    int ga = 0, gb = 0;  // two groups (their addresses)
    expect("1 + 4 equal shapes, all full, one group", equal(5, 150, &ga), false, 0, {5});
    expect("the same, not a group", equal(5, 150, nullptr), false, 0, {1, 1, 1, 1, 1});
    expect("mean-only constraints, not a group", equal(5, 150, nullptr), true, 0, {1, 4});
    expect("mean-only constraints of a group: the objective's sequence is the full one", equal(5, 150, &ga), true, 0, {1, 4});
    expect("1 + 17 mean-only", equal(18, 70, nullptr), true, 0, {1, 16, 1});
    expect("1 + 17 full, one group", equal(18, 70, &ga), false, 0, {16, 2});
    {
        std::vector<Shape> s = equal(5, 150, nullptr);
        s[3].n = 100, s[3].n_pad = 128;
        expect("one constraint with another n in the middle", s, true, 0, {1, 2, 1, 1});
    }
    {
        std::vector<Shape> s = equal(5, 150, nullptr);
        s[2].lone_dense = false;  // a sparse model, or a mixture
        expect("a sparse model or a mixture cuts the run", s, true, 0, {1, 1, 1, 2});
        s = equal(5, 150, &ga);
        s[2].lone_dense = false;
        expect("... a full run as well", s, false, 0, {2, 1, 2});
    }
    expect("pending points, q = 1: a group", equal(5, 150, &ga), false, 1, {1, 1, 1, 1, 1});
    expect("pending points, q = 1: mean-only", equal(5, 150, nullptr), true, 1, {1, 1, 1, 1, 1});
    // the byte bound: blocks of 128 x 256 doubles; room for three of them
    expect("the byte bound cuts the run", equal(5, 150, &ga), false, 0, {3, 2}, (int64_t)3 * 128 * 256);
    expect("... below one block every run is one", equal(5, 150, &ga), false, 0, {1, 1, 1, 1, 1}, 1);
    {
        std::vector<Shape> s = equal(5, 150, &ga);
        s[3].group = &gb, s[3].slot = 3;
        expect("a member of another group cuts a full run", s, false, 0, {3, 1, 1});
        s = equal(5, 150, &ga);
        s[2].slot = 3, s[3].slot = 2;
        expect("slots out of order cut a full run", s, false, 0, {2, 1, 1, 1});
        expect("... and leave a mean-only run alone", s, true, 0, {1, 4});
    }
    {
        std::vector<Shape> s = equal(4, 150, nullptr);
        s[2].corr = 3;
        expect("another kernel", s, true, 0, {1, 1, 1, 1});
        s = equal(4, 150, nullptr);
        s[3].mean = 1;
        expect("another trend", s, true, 0, {1, 2, 1});
        s = equal(4, 150, nullptr);
        s[1].fit_hcols = 2, s[1].has_w = true;
        expect("other coefficient columns", s, true, 0, {1, 1, 2});
        s = equal(5, 150, nullptr);
        s[2].n = 100, s[2].n_pad = 128, s[4].n = 100, s[4].n_pad = 128;
        expect("same shapes that are not adjacent do not merge", s, true, 0, {1, 1, 1, 1, 1});
    }
    expect("the objective alone", equal(1, 150, nullptr), false, 0, {1});
    return failures;
}
