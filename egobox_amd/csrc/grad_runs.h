// How the entries of one lock-step evaluation -- the candidates of a slot (likelihood_grad_batch_core) or the members of a run
// of a group (egx_gp_likelihood_grad_multi), gp_fit.hip -- are cut into launch sequences of the gradient stages.  Host only: no
// HIP in here, so that tests/c_host/grad_runs_test.cpp compiles it with the host compiler alone.
//
// Entry j has a gradient when ok[j] != 0 (its likelihood ended finite with a positive variance), and takes the prescaled form
// of the trace kernel when pre[j] != 0 (one coefficient column, every coefficient positive and finite: ITS OWN coefficients
// decide, never its companions').  A launch sequence takes consecutive entries -- their matrices and C^-T buffers sit at one
// stride -- of one form.  The rule: MAXIMAL runs of consecutive entries that have a gradient and the same form, in order.
#pragma once
#include <cmath>
#include <vector>

namespace egx {
namespace gradruns {

struct Run {
    int first, count, pre;
};
inline bool operator==(const Run &a, const Run &b) { return a.first == b.first && a.count == b.count && a.pre == b.pre; }

inline std::vector<Run> split(const char *ok, const char *pre, int cnt) {
    std::vector<Run> runs;
    for (int j = 0; j < cnt;) {
        if (!ok[j]) {
            j++;
            continue;
        }
        int e = j;
        while (e < cnt && ok[e] && (pre[e] != 0) == (pre[j] != 0)) e++;
        runs.push_back(Run{j, e - j, pre[j] != 0 ? 1 : 0});
        j = e;
    }
    return runs;
}

// whether an entry may take the prescaled form: hcols == 1 and every one of its ncoef coefficients positive and finite
inline bool prescaled(int hcols, const double *coef, int ncoef) {
    if (hcols != 1) return false;
    for (int i = 0; i < ncoef; i++)
        if (!(coef[i] > 0.0) || !std::isfinite(coef[i])) return false;
    return true;
}

}  // namespace gradruns
}  // namespace egx
