// The sharded fold of a mixture of experts' predict side (egx_moe_predict_valvar, egx_moe_predict_valvar_gradients:
// moe_host.hip), written once at width w -- 1 for values, d for x-gradients.  Free of HIP and of the sweep: plain C++17 with
// <thread>, so that tests/c_host/moe_fold_test.cpp runs it with closed-form experts under ASan / UBSan / TSan.
// A rank owns n_local of the n_experts experts.  The caller supplies
//     eval(expert, xin, me, scratch, msg) -> rc   the expert's quantities at me points into the worker's scratch (msg on failure)
//     acc(g, scratch, rows, me, ta, tb)           smooth (rows == nullptr): add expert g's terms of all m points to the sums
//                                                 ta / tb; hard: copy its me rows to the points rows[0 .. me)
// (accumulate_values / accumulate_gradients below are the library's) and the fold owns the rest:
//   routing   hard mode answers a point by the expert of the FIRST maximum of its responsibilities (infill::mix_first_max: a
//             NaN never beats entry 0).  The points are routed once; an expert without points is skipped without a call.
//   workers   up to two experts in flight: worker A (the calling thread) takes the local experts 0, 2, 4, .., worker B (a
//             second thread, only with two or more local experts) 1, 3, 5, ...
//   ORDER OF ADDITIONS (smooth): A adds its experts' terms in that order into the payload, B into vectors of its own, then
//             A + B, then the ranks in rank order (fold_sum_ranks): ((e0 + e2 + e4) + (e1 + e3)) + the next rank's.  It
//             depends on the shard alone, so every rank and every run returns the same bits.  Hard mode adds nothing: both
//             workers write disjoint rows of the payload.
//   failure   the first eval that fails wins: its rc and message come back, and neither worker starts another expert.  The
//             rc rides in front of the payload (sweep_status_word), so a failed rank still takes part in the collective.
//   payload   [status | A (m w) | B (m w)]; an output the caller does not want stays zero and is skipped by the rank sum.
#pragma once
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/egx_gp.h"
#include "infill_mix_math.h"
#include "sweep_shard.h"

namespace egx {
namespace moe {

// The variance term of the host fold, (p p) v.  k_infill_mix's infill::mix_var_term is (v p) p: the same value up to one
// rounding, NOT the same bits.  Each is pinned by its own tests; changing either association is a behaviour change.
inline double fold_var_term(double p, double v) { return (p * p) * v; }

template <class Expert>
struct Fold {
    Expert *const *experts = nullptr;     // n_local handles ..
    const int32_t *expert_ids = nullptr;  // .. and their indices among the n_experts
    int64_t n_local = 0, n_experts = 1;
    const double *probas = nullptr;       // m x n_experts
    const double *xq = nullptr;           // m x d
    int64_t m = 0, d = 1, w = 1;
    bool smooth = true;
};

struct LocalFold {
    std::vector<double> part;  // [status | A (m w) | B (m w)]
    int rc = 0;
    std::string msg;
};

template <class Scratch, class Expert, class Eval, class Acc>
LocalFold fold_local(const char *who, const Fold<Expert> &f, Eval eval, Acc acc) {
    const size_t mw = (size_t)f.m * f.w;
    LocalFold out;
    out.part.assign(2 * mw + 1, 0.0);
    double *pa = out.part.data() + 1, *pb = pa + mw;
    for (int64_t e = 0; e < f.n_local && !out.rc; e++)
        if (!f.experts[e] || f.expert_ids[e] < 0 || f.expert_ids[e] >= f.n_experts) {
            out.msg = std::string(who) + ": NULL expert handle or expert id out of range";
            out.rc = EGX_ERR_INVALID_VALUE;
        }
    std::vector<std::vector<int64_t>> rows;  // hard: the points of every cluster, ascending
    if (!f.smooth && !out.rc) {
        rows.resize((size_t)f.n_experts);
        for (int64_t a = 0; a < f.m; a++) rows[(size_t)infill::mix_first_max((int)f.n_experts, f.probas + a * f.n_experts, 1)].push_back(a);
    }
    if (!out.rc) {
        std::mutex mu;  // out.rc / out.msg
        auto worker = [&](int64_t first, double *ta, double *tb) {
            Scratch s;
            std::vector<double> xs;
            for (int64_t e = first; e < f.n_local; e += 2) {
                {
                    std::lock_guard<std::mutex> l(mu);
                    if (out.rc) return;
                }
                const int32_t g = f.expert_ids[e];
                const double *xin = f.xq;
                const int64_t *idx = nullptr;
                int64_t me = f.m;
                if (!f.smooth) {
                    idx = rows[(size_t)g].data();
                    me = (int64_t)rows[(size_t)g].size();
                    if (me == 0) continue;
                    xs.resize((size_t)me * f.d);
                    for (int64_t i = 0; i < me; i++) std::memcpy(&xs[(size_t)i * f.d], f.xq + idx[i] * f.d, sizeof(double) * f.d);
                    xin = xs.data();
                }
                std::string msg;
                const int rc = eval(f.experts[e], xin, me, s, msg);
                if (rc) {
                    std::lock_guard<std::mutex> l(mu);
                    if (!out.rc) {
                        out.rc = rc;
                        out.msg = msg;
                    }
                    return;
                }
                acc(g, s, idx, me, ta, tb);
            }
        };
        if (f.n_local > 1) {
            std::vector<double> part_b(f.smooth ? 2 * mw : 0, 0.0);
            double *ba = f.smooth ? part_b.data() : pa, *bb = f.smooth ? part_b.data() + mw : pb;
            std::thread tb(worker, (int64_t)1, ba, bb);
            worker(0, pa, pb);
            tb.join();
            if (f.smooth)
                for (size_t i = 0; i < mw; i++) {
                    pa[i] += part_b[i];
                    pb[i] += part_b[mw + i];
                }
        } else {
            worker(0, pa, pb);
        }
    }
    out.part[0] = sweep_status_word(out.rc);
    return out;
}

// the payloads of all ranks, concatenated in rank order, into the caller's outputs (either may be NULL)
inline void fold_sum_ranks(const double *all, int world, size_t mw, double *out_a, double *out_b) {
    const size_t len = 2 * mw + 1;
    for (size_t i = 0; i < mw; i++) {
        double sa = 0.0, sb = 0.0;
        for (int r = 0; r < world; r++) {
            const double *pr = all + (size_t)r * len + 1;
            sa += pr[i];
            sb += pr[mw + i];
        }
        if (out_a) out_a[i] = sa;
        if (out_b) out_b[i] = sb;
    }
}

// ---- the two accumulations of the library: expert g's (ys, vs) / (gy, gv) of its me points, NULL = not wanted ----
inline void accumulate_values(const double *probas, int64_t n_experts, int64_t m, int32_t g, const double *ys, const double *vs,
                              const int64_t *rows, int64_t me, double *tv, double *tw) {
    if (rows) {
        for (int64_t i = 0; i < me; i++) {
            if (ys) tv[rows[i]] = ys[i];
            if (vs) tw[rows[i]] = vs[i];
        }
        return;
    }
    for (int64_t a = 0; a < m; a++) {
        const double p = probas[a * n_experts + g];
        if (ys) tv[a] += infill::mix_mean_term(p, ys[a]);
        if (vs) tw[a] += fold_var_term(p, vs[a]);
    }
}

// dprobas (m x n_experts x d) == NULL: a lone expert, whose p' terms are not formed -- the sums then take `+ 0.0` in their
// place, which is not nothing (it turns a -0.0 into +0.0) and stays
inline void accumulate_gradients(const double *probas, const double *dprobas, int64_t n_experts, int64_t m, int64_t d, int32_t g,
                                 const double *gy, const double *gv, const double *ys, const double *vs, const int64_t *rows,
                                 int64_t me, double *tv, double *tw) {
    if (rows) {
        for (int64_t i = 0; i < me; i++) {
            if (gy) std::memcpy(tv + rows[i] * d, gy + i * d, sizeof(double) * d);
            if (gv) std::memcpy(tw + rows[i] * d, gv + i * d, sizeof(double) * d);
        }
        return;
    }
    for (int64_t a = 0; a < m; a++) {
        const double p = probas[a * n_experts + g];
        const double *pp = dprobas ? dprobas + ((size_t)a * n_experts + g) * d : nullptr;
        for (int64_t j = 0; j < d; j++) {
            if (gy) tv[a * d + j] += pp ? infill::mix_grad_mean_term(p, pp[j], ys[a], gy[a * d + j]) : gy[a * d + j] * p + 0.0;
            if (gv) tw[a * d + j] += pp ? infill::mix_grad_var_term(p, pp[j], vs[a], gv[a * d + j]) : gv[a * d + j] * (p * p) + 0.0;
        }
    }
}

}  // namespace moe
}  // namespace egx
