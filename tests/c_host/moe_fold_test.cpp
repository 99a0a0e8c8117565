// CPU test of the mixture's sharded fold (csrc/moe_fold.h) with closed-form experts: the order of additions against an
// independent serial restatement, bit for bit and run after run; hard-mode routing (first maximum, NaN, empty clusters, rows at
// their own indices); NULL outputs; a failing expert (rc, message, nothing started after it, the status word); two and three
// simulated ranks through the payload layout and the rank-order sum.  Built by tests/test_moe_cpu.py with ASan + UBSan and
// with TSan, and run as its own process.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../egobox_amd/csrc/moe_fold.h"
using namespace egx;

#define REQUIRE(cond)                                                \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("line %d: %s\n", __LINE__, #cond);           \
            std::exit(1);                                            \
        }                                                            \
    } while (0)

// ---- closed-form experts: signs, magnitudes over many binades and exact zeros, so that the order of additions shows
struct Fake {
    int id;
    int fail_rc = 0;  // != 0: eval fails with it
};
static double f_val(int g, const double *x, int64_t d) {
    double s = 0.3 * (g + 1);
    for (int64_t j = 0; j < d; j++) s += std::sin((g + 1.7) * x[j] + j);
    return s * std::ldexp(1.0, (g * 7) % 11 - 5);
}
static double f_var(int g, const double *x, int64_t d) { return 1e-3 * (g + 1) + std::fabs(std::cos(x[0] * (g + 2))) + 0.01 * d; }
static double f_gval(int g, const double *x, int64_t j) { return (g % 2 ? -1.0 : 1.0) * std::cos((g + 0.3) * x[j] - j) / 3.0; }
static double f_gvar(int g, const double *x, int64_t j) { return (j == 1 && g == 0) ? -0.0 : std::sin(x[j] * (g + 1) + 0.1 * j) * 1e-2; }

struct Rows {
    std::vector<double> y, v, gy, gv;
};
static std::atomic<int> g_calls[16];     // eval calls per expert id
static std::atomic<int> g_seq{0};        // order in which evals START
static std::atomic<int> g_started[16];   // 1 + that order
static std::atomic<bool> g_b_exited{false};
struct ExitFlag {
    bool armed = false;
    ~ExitFlag() {
        if (armed) g_b_exited.store(true);
    }
};
static thread_local ExitFlag t_exit;
static int g_wait_for_b = -1;  // the expert whose eval returns only when the failing worker's thread is gone

static void reset_counters() {
    for (auto &c : g_calls) c.store(0);
    for (auto &c : g_started) c.store(0);
    g_seq.store(0);
    g_b_exited.store(false);
}

struct Case {
    int64_t m, d, w, n_experts;
    bool smooth, want_a = true, want_b = true, with_dp = true;
    std::vector<double> probas, dprobas, xq;
};
static Case make_case(int64_t m, int64_t d, int64_t w, int64_t n_experts, bool smooth) {
    Case c{m, d, w, n_experts, smooth};
    c.xq.resize((size_t)m * d);
    for (size_t i = 0; i < c.xq.size(); i++) c.xq[i] = std::sin(0.37 * (double)i) * 2.0 + 0.01 * (double)(i % 7);
    c.probas.resize((size_t)m * n_experts);
    c.dprobas.resize((size_t)m * n_experts * d);
    for (int64_t a = 0; a < m; a++) {
        double tot = 0.0;
        for (int64_t g = 0; g < n_experts; g++) tot += (c.probas[a * n_experts + g] = 0.05 + std::fabs(std::sin(1.3 * a + 2.1 * g)));
        for (int64_t g = 0; g < n_experts; g++) c.probas[a * n_experts + g] /= tot;
    }
    for (size_t i = 0; i < c.dprobas.size(); i++) c.dprobas[i] = std::cos(0.11 * (double)i) * 0.5;
    return c;
}

// one rank's fold over `mine` (its experts, in local order) -- values at w == 1, gradients at w == d
static moe::LocalFold run_local(const Case &c, const std::vector<Fake> &mine, const std::vector<int32_t> &ids_override = {}) {
    std::vector<Fake *> hs;
    std::vector<int32_t> ids;
    for (const Fake &fk : mine) hs.push_back(const_cast<Fake *>(&fk)), ids.push_back(fk.id);
    if (!ids_override.empty()) ids = ids_override;
    const bool grad = c.w != 1;
    const bool need_pp = grad && c.smooth && c.with_dp;
    const moe::Fold<Fake> f{hs.data(), ids.data(), (int64_t)hs.size(), c.n_experts, c.probas.data(), c.xq.data(), c.m, c.d, c.w, c.smooth};
    auto eval = [&](Fake *fk, const double *xin, int64_t me, Rows &s, std::string &msg) {
        g_started[fk->id].store(1 + g_seq.fetch_add(1));
        g_calls[fk->id].fetch_add(1);
        if (fk->fail_rc) {
            t_exit.armed = true;
            msg = "fake expert " + std::to_string(fk->id) + " failed";
            return fk->fail_rc;
        }
        if (fk->id == g_wait_for_b)
            for (long spin = 0; !g_b_exited.load(); spin++) {
                REQUIRE(spin < 20000000L);  // the failing worker never ran: no second thread
                std::this_thread::yield();
            }
        s.y.resize(me), s.v.resize(me);
        for (int64_t i = 0; i < me; i++) s.y[i] = f_val(fk->id, xin + i * c.d, c.d), s.v[i] = f_var(fk->id, xin + i * c.d, c.d);
        if (grad) {
            s.gy.resize((size_t)me * c.d), s.gv.resize((size_t)me * c.d);
            for (int64_t i = 0; i < me; i++)
                for (int64_t j = 0; j < c.d; j++)
                    s.gy[i * c.d + j] = f_gval(fk->id, xin + i * c.d, j), s.gv[i * c.d + j] = f_gvar(fk->id, xin + i * c.d, j);
        }
        return 0;
    };
    auto acc = [&](int32_t g, const Rows &s, const int64_t *rows, int64_t me, double *ta, double *tb) {
        if (!grad)
            moe::accumulate_values(c.probas.data(), c.n_experts, c.m, g, c.want_a ? s.y.data() : nullptr, c.want_b ? s.v.data() : nullptr,
                                   rows, me, ta, tb);
        else
            moe::accumulate_gradients(c.probas.data(), need_pp ? c.dprobas.data() : nullptr, c.n_experts, c.m, c.d, g,
                                      c.want_a ? s.gy.data() : nullptr, c.want_b ? s.gv.data() : nullptr, s.y.data(), s.v.data(), rows,
                                      me, ta, tb);
    };
    return moe::fold_local<Rows>("fold_test", f, eval, acc);
}

// ---- the documented order, restated serially and independently of the header's term functions:
//      per rank ((e0 + e2 + e4) + (e1 + e3)), starting from 0.0; then 0.0 + rank 0 + rank 1 + ..
static void term(const Case &c, int g, int64_t a, int64_t j, double *ta, double *tb) {
    const double *x = &c.xq[(size_t)a * c.d];
    const double p = c.probas[a * c.n_experts + g];
    if (c.w == 1) {
        *ta = p * f_val(g, x, c.d);
        *tb = (p * p) * f_var(g, x, c.d);
    } else if (c.with_dp) {
        const double dp = c.dprobas[((size_t)a * c.n_experts + g) * c.d + j];
        *ta = f_gval(g, x, j) * p + dp * f_val(g, x, c.d);
        *tb = f_gvar(g, x, j) * (p * p) + ((2.0 * p) * dp) * f_var(g, x, c.d);
    } else {
        *ta = f_gval(g, x, j) * p + 0.0;
        *tb = f_gvar(g, x, j) * (p * p) + 0.0;
    }
}
static void restate_smooth(const Case &c, const std::vector<std::vector<int>> &ranks, std::vector<double> &out_a,
                           std::vector<double> &out_b) {
    const size_t mw = (size_t)c.m * c.w;
    out_a.assign(mw, 0.0), out_b.assign(mw, 0.0);
    for (size_t i = 0; i < mw; i++) {
        const int64_t a = (int64_t)i / c.w, j = (int64_t)i % c.w;
        double ra = 0.0, rb = 0.0;
        for (const std::vector<int> &mine : ranks) {
            double wa[2] = {0.0, 0.0}, wb[2] = {0.0, 0.0};
            for (size_t e = 0; e < mine.size(); e++) {
                double ta, tb;
                term(c, mine[e], a, j, &ta, &tb);
                wa[e & 1] += ta, wb[e & 1] += tb;
            }
            ra += mine.size() > 1 ? wa[0] + wa[1] : wa[0];
            rb += mine.size() > 1 ? wb[0] + wb[1] : wb[0];
        }
        out_a[i] = ra, out_b[i] = rb;
    }
}
static bool same_bits(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}
static std::vector<Fake> fakes(const std::vector<int> &ids) {
    std::vector<Fake> v;
    for (int g : ids) v.push_back(Fake{g});
    return v;
}

static int test_order_of_additions() {
    int n = 0;
    for (int K : {0, 1, 2, 3, 5})
        for (int64_t w : {1, 3})
            for (int64_t m : {1, 7, 64, 65})
                for (bool with_dp : {true, false}) {
                    if (!with_dp && (w == 1 || K != 1)) continue;  // the `+ 0.0` form: gradients of a lone expert
                    Case c = make_case(m, 3, w, K ? K : 1, true);
                    c.with_dp = with_dp;
                    std::vector<int> ids;
                    for (int e = 0; e < K; e++) ids.push_back(K - 1 - e);  // the order is that of the LOCAL index, not of the id
                    std::vector<double> want_a, want_b, first;
                    restate_smooth(c, {ids}, want_a, want_b);
                    const std::vector<Fake> mine = fakes(ids);
                    for (int run = 0; run < 20; run++) {
                        const moe::LocalFold lf = run_local(c, mine);
                        REQUIRE(lf.rc == 0 && lf.part[0] == 0.0 && lf.part.size() == 2 * (size_t)m * w + 1);
                        std::vector<double> a((size_t)m * w), b((size_t)m * w);
                        moe::fold_sum_ranks(lf.part.data(), 1, (size_t)m * w, a.data(), b.data());
                        REQUIRE(same_bits(a, want_a) && same_bits(b, want_b));
                        if (run == 0) first = lf.part;
                        REQUIRE(same_bits(lf.part, first));
                    }
                    n++;
                }
    return n;
}

static int test_hard_mode() {
    int n = 0;
    for (int64_t w : {1, 2})
        for (int64_t m : {1, 7, 65}) {
            Case c = make_case(m, 2, w, 5, false);
            for (int64_t a = 0; a < m; a++) {
                double *p = &c.probas[a * 5];
                p[4] = 0.0;                                 // cluster 4 owns no point
                if (a % 3 == 0) p[1] = p[2] = 0.9;          // a tie: the first maximum, cluster 1
                if (a % 5 == 1) p[3] = std::nan("");        // a NaN never wins ...
                if (a % 7 == 2) p[0] = std::nan("");        // ... and nothing beats a NaN in entry 0
            }
            reset_counters();
            const std::vector<Fake> mine = fakes({0, 1, 2, 3, 4});
            const moe::LocalFold lf = run_local(c, mine);
            REQUIRE(lf.rc == 0);
            std::vector<double> a((size_t)m * w), b((size_t)m * w);
            moe::fold_sum_ranks(lf.part.data(), 1, (size_t)m * w, a.data(), b.data());
            std::vector<int> owned(5, 0);
            for (int64_t q = 0; q < m; q++) {
                const double *p = &c.probas[q * 5];
                int g = 0;
                if (!(q % 7 == 2))
                    for (int e = 1; e < 5; e++)
                        if (!std::isnan(p[e]) && p[e] > p[g]) g = e;
                if (q % 3 == 0 && q % 7 != 2) REQUIRE(g != 2);
                owned[g]++;
                const double *x = &c.xq[(size_t)q * c.d];
                for (int64_t j = 0; j < w; j++) {
                    // (0.0 + row: the rank sum starts from zero, which turns a -0.0 row into +0.0)
                    const double ea = 0.0 + (w == 1 ? f_val(g, x, c.d) : f_gval(g, x, j)), eb = 0.0 + (w == 1 ? f_var(g, x, c.d) : f_gvar(g, x, j));
                    REQUIRE(std::memcmp(&a[q * w + j], &ea, 8) == 0 && std::memcmp(&b[q * w + j], &eb, 8) == 0);
                }
            }
            for (int g = 0; g < 5; g++) REQUIRE(g_calls[g].load() == (owned[g] ? 1 : 0));  // routed once, empty ones skipped
            REQUIRE(g_calls[4].load() == 0);
            n++;
        }
    return n;
}

static int test_null_outputs() {
    int n = 0;
    for (bool smooth : {true, false})
        for (int64_t w : {1, 3}) {
            Case c = make_case(65, 3, w, 3, smooth);
            const std::vector<Fake> mine = fakes({0, 1, 2});
            const size_t mw = (size_t)c.m * w;
            std::vector<double> both_a(mw), both_b(mw);
            moe::fold_sum_ranks(run_local(c, mine).part.data(), 1, mw, both_a.data(), both_b.data());
            for (int which = 0; which < 2; which++) {
                c.want_a = which == 0, c.want_b = which == 1;
                const moe::LocalFold lf = run_local(c, mine);
                std::vector<double> got(mw), canary(mw, 12345.0);
                moe::fold_sum_ranks(lf.part.data(), 1, mw, which == 0 ? got.data() : nullptr, which == 1 ? got.data() : nullptr);
                REQUIRE(same_bits(got, which == 0 ? both_a : both_b));
                // the half of the payload nobody asked for was never written
                for (size_t i = 0; i < mw; i++) REQUIRE(lf.part[1 + (which == 0 ? mw : 0) + i] == 0.0);
                n++;
            }
        }
    return n;
}

static int test_failing_expert() {
    int n = 0;
    Case c = make_case(7, 2, 1, 5, true);
    // (a) the failure on worker A's first expert: A's later experts are never started
    {
        std::vector<Fake> mine = fakes({0, 1, 2, 3, 4});
        mine[0].fail_rc = EGX_ERR_LINALG;
        reset_counters();
        const moe::LocalFold lf = run_local(c, mine);
        REQUIRE(lf.rc == EGX_ERR_LINALG && lf.msg == "fake expert 0 failed");
        REQUIRE(lf.part[0] == sweep_status_word(EGX_ERR_LINALG) && lf.part[0] == -(double)(kSweepPoison + EGX_ERR_LINALG));
        REQUIRE(g_calls[2].load() == 0 && g_calls[4].load() == 0);
        n++;
    }
    // (b) the failure on worker B's first expert: if A's first is in flight it ends only after B has recorded the failure and
    //     left (the thread's exit is observed), so A starts nothing more -- expert 1 ran, expert 0 at most once, nobody else
    {
        std::vector<Fake> mine = fakes({0, 1, 2, 3, 4});
        mine[1].fail_rc = EGX_ERR_HIP;
        reset_counters();
        g_wait_for_b = 0;
        const moe::LocalFold lf = run_local(c, mine);
        g_wait_for_b = -1;
        REQUIRE(lf.rc == EGX_ERR_HIP && lf.msg == "fake expert 1 failed" && lf.part[0] == sweep_status_word(EGX_ERR_HIP));
        REQUIRE(g_calls[0].load() <= 1 && g_calls[1].load() == 1);
        REQUIRE(g_calls[2].load() == 0 && g_calls[3].load() == 0 && g_calls[4].load() == 0);
        n++;
    }
    // (c) a lone failing expert, no second thread; hard mode
    {
        Case h = make_case(7, 2, 2, 1, false);
        std::vector<Fake> mine = fakes({0});
        mine[0].fail_rc = EGX_ERR_NOT_FITTED;
        const moe::LocalFold lf = run_local(h, mine);
        REQUIRE(lf.rc == EGX_ERR_NOT_FITTED && lf.part[0] == sweep_status_word(EGX_ERR_NOT_FITTED));
        n++;
    }
    return n;
}

static int test_ranks() {
    int n = 0;
    for (int world : {2, 3})
        for (int64_t w : {1, 3})
            for (bool smooth : {true, false}) {
                const int K = 5;
                Case c = make_case(65, 3, w, K, smooth);
                const size_t mw = (size_t)c.m * w, len = 2 * mw + 1;
                std::vector<std::vector<int>> shard(world);
                for (int e = 0; e < K; e++) shard[e % world].push_back(e);  // expert e on rank e mod world
                std::vector<double> all;
                for (int r = 0; r < world; r++) {
                    const moe::LocalFold lf = run_local(c, fakes(shard[r]));
                    REQUIRE(lf.rc == 0 && lf.part.size() == len);
                    all.insert(all.end(), lf.part.begin(), lf.part.end());
                }
                REQUIRE(sweep_first_failure(all.data(), world, len).rank == -1);
                std::vector<double> want_a, want_b;
                if (smooth) {
                    restate_smooth(c, shard, want_a, want_b);
                } else {  // hard: the single-rank answer (sums of one row and zeros)
                    std::vector<int> every;
                    for (int e = 0; e < K; e++) every.push_back(e);
                    want_a.resize(mw), want_b.resize(mw);
                    moe::fold_sum_ranks(run_local(c, fakes(every)).part.data(), 1, mw, want_a.data(), want_b.data());
                }
                for (int r = 0; r < world; r++) {  // every rank sums the same concatenation
                    std::vector<double> a(mw), b(mw);
                    moe::fold_sum_ranks(all.data(), world, mw, a.data(), b.data());
                    REQUIRE(same_bits(a, want_a) && same_bits(b, want_b));
                }
                // an expert id out of range on the last rank: that rank's own error, a peer failure everywhere else
                std::vector<double> bad = all;
                const moe::LocalFold lf = run_local(c, fakes(shard[world - 1]), std::vector<int32_t>(shard[world - 1].size(), K));
                REQUIRE(lf.rc == EGX_ERR_INVALID_VALUE && lf.msg == "fold_test: NULL expert handle or expert id out of range");
                std::copy(lf.part.begin(), lf.part.end(), bad.begin() + (size_t)(world - 1) * len);
                const SweepFailure sf = sweep_first_failure(bad.data(), world, len);
                REQUIRE(sf.rank == world - 1 && sf.rc == EGX_ERR_INVALID_VALUE);
                n++;
            }
    return n;
}

int main() {
    const int a = test_order_of_additions(), b = test_hard_mode(), c = test_null_outputs(), d = test_failing_expert(), e = test_ranks();
    std::printf("OK %d order, %d hard, %d null-output, %d failure, %d rank cases\n", a, b, c, d, e);
    return 0;
}
