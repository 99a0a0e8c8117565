// egobox_amd/csrc/grad_runs.h on the host (no HIP): how the entries of one lock-step evaluation are cut into launch sequences of
// the gradient stages -- maximal runs of consecutive entries that have a gradient and take the same form of the trace kernel.
// Hand-written patterns with their expected runs, then every pattern against a brute-force restatement: an entry belongs to a
// run iff it has a gradient, and two neighbours share a run iff both have one and their forms agree.  Built with
// -fsanitize=address,undefined by tests/test_grad_runs_cpu.py; prints one "ok <pattern>" line per pattern and "OK" at the end.
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../egobox_amd/csrc/grad_runs.h"

using egx::gradruns::Run;

static int failures = 0;
constexpr int kLockstepMax = 16;  // egx_internal.h: what one launch sequence takes

// the restatement: label every entry with the index of its run (-1: none) by looking at neighbours only
static std::vector<int> labels_brute(const std::vector<char> &ok, const std::vector<char> &pre) {
    std::vector<int> lab(ok.size(), -1);
    int next = 0;
    for (size_t j = 0; j < ok.size(); j++) {
        if (!ok[j]) continue;
        const bool joins = j > 0 && ok[j - 1] && (pre[j - 1] != 0) == (pre[j] != 0);
        lab[j] = joins ? lab[j - 1] : next++;
    }
    return lab;
}
static std::vector<int> labels_of(const std::vector<Run> &runs, size_t cnt) {
    std::vector<int> lab(cnt, -1);
    for (size_t r = 0; r < runs.size(); r++)
        for (int j = runs[r].first; j < runs[r].first + runs[r].count; j++) lab[(size_t)j] = (int)r;
    return lab;
}

static void pattern(const std::string &what, const std::vector<char> &ok, const std::vector<char> &pre, const std::vector<Run> &expect) {
    const std::vector<Run> got = egx::gradruns::split(ok.data(), pre.data(), (int)ok.size());
    bool good = got == expect && labels_of(got, ok.size()) == labels_brute(ok, pre);
    for (const Run &r : got) {  // every run: non-empty, in range, of one form, and that form reported
        good = good && r.count >= 1 && r.first >= 0 && r.first + r.count <= (int)ok.size();
        for (int j = r.first; good && j < r.first + r.count; j++) good = ok[(size_t)j] && (pre[(size_t)j] != 0) == (r.pre != 0);
    }
    if (!good) failures++;
    std::printf("%s %s: %zu runs\n", good ? "ok" : "FAIL", what.c_str(), got.size());
}

int main() {
    pattern("all ok, one form", {1, 1, 1, 1, 1}, {1, 1, 1, 1, 1}, {{0, 5, 1}});
    pattern("all ok, the raw form", {1, 1, 1}, {0, 0, 0}, {{0, 3, 0}});
    pattern("a failed entry in the middle", {1, 1, 0, 1, 1}, {1, 1, 1, 1, 1}, {{0, 2, 1}, {3, 2, 1}});
    pattern("alternating forms", {1, 1, 1, 1}, {1, 0, 1, 0}, {{0, 1, 1}, {1, 1, 0}, {2, 1, 1}, {3, 1, 0}});
    pattern("a raw entry between prescaled ones", {1, 1, 1, 1, 1, 1}, {1, 1, 0, 1, 1, 1}, {{0, 2, 1}, {2, 1, 0}, {3, 3, 1}});
    pattern("the form of a failed entry does not matter", {1, 0, 1}, {1, 0, 1}, {{0, 1, 1}, {2, 1, 1}});
    pattern("failures at both ends", {0, 1, 1, 0}, {0, 1, 1, 0}, {{1, 2, 1}});
    pattern("empty input", {}, {}, {});
    pattern("all failed", {0, 0, 0, 0}, {1, 1, 0, 0}, {});
    pattern("one entry", {1}, {0}, {{0, 1, 0}});
    pattern("kLockstepMax entries, one run", std::vector<char>(kLockstepMax, 1), std::vector<char>(kLockstepMax, 1), {{0, kLockstepMax, 1}});
    {
        std::vector<char> ok(kLockstepMax, 1), pre(kLockstepMax, 1);
        ok[5] = 0, pre[11] = 0;
        pattern("kLockstepMax entries, a failure and a raw entry", ok, pre, {{0, 5, 1}, {6, 5, 1}, {11, 1, 0}, {12, 4, 1}});
    }
    // any non-zero char is "true"
    pattern("truth values other than 1", {2, 1, 7}, {3, 1, 0}, {{0, 2, 1}, {2, 1, 0}});
    // every pattern of five entries against the restatement
    int exhaustive = 0;
    for (int a = 0; a < 32; a++)
        for (int b = 0; b < 32; b++) {
            std::vector<char> ok(5), pre(5);
            for (int j = 0; j < 5; j++) ok[(size_t)j] = (char)((a >> j) & 1), pre[(size_t)j] = (char)((b >> j) & 1);
            if (labels_of(egx::gradruns::split(ok.data(), pre.data(), 5), 5) == labels_brute(ok, pre)) exhaustive++;
        }
    if (exhaustive != 1024) failures++;
    std::printf("%s all 1024 patterns of five entries\n", exhaustive == 1024 ? "ok" : "FAIL");
    // the form an entry may take: one coefficient column, every coefficient positive and finite
    const double pos[] = {0.5, 2.0}, zero[] = {0.5, 0.0}, neg[] = {-1.0, 2.0}, inf[] = {1.0, std::numeric_limits<double>::infinity()},
                 nan[] = {std::numeric_limits<double>::quiet_NaN(), 1.0};
    const bool forms = egx::gradruns::prescaled(1, pos, 2) && !egx::gradruns::prescaled(2, pos, 2) && !egx::gradruns::prescaled(1, zero, 2) &&
                       !egx::gradruns::prescaled(1, neg, 2) && !egx::gradruns::prescaled(1, inf, 2) && !egx::gradruns::prescaled(1, nan, 2) &&
                       egx::gradruns::prescaled(1, pos, 0);
    if (!forms) failures++;
    std::printf("%s prescaled form\n", forms ? "ok" : "FAIL");
    if (failures == 0) std::printf("OK\n");
    return failures == 0 ? 0 : 1;
}
