// Host-only checks of csrc/fit_starts.h (no HIP, no library): the box in log10 and its messages, the COBYLA budget, the
// lock-step drivers the fits build from it (as fit_run_starts, egx_gp_fit_lbfgs and egx_gp_fit_multi do, gp_fit.hip) against
// every start alone, sharding, a partial active set, the reduction and the winner, the one-after-the-other driver of the
// sparse fits.  Analytic objectives in x = log10(theta).  Prints "ok <name>" or "FAILED <name>" per check; exit status 1 on a
// failure.  tests/test_fit_starts_cpu.py builds and runs it, once more under the address and UB sanitizers.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <tuple>

#include "../../egobox_amd/csrc/fit_starts.h"
using namespace egx;

typedef std::vector<double> vec;
typedef std::function<double(const double *theta, int h)> Objective;  // f = -likelihood at a full-width theta

static const double kInf = std::numeric_limits<double>::infinity(), kNan = std::numeric_limits<double>::quiet_NaN();
static int failures = 0;
static void check(bool ok, const char *name) {
    printf("%s %s\n", ok ? "ok" : "FAILED", name);
    if (!ok) failures++;
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool same_bits(const vec &a, const vec &b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0); }
static bool same(const StartResult &a, const StartResult &b) { return same_bits(a.f, b.f) && same_bits(a.x, b.x) && a.evals == b.evals; }

// shifted quadratic in log10 space; centre 0.9 lies beyond the box's upper bound log10(5): that bound is active
static double quadratic(const double *th, int h) {
    const double c[4] = {0.9, -0.4, 0.2, -0.7};
    double s = 1.5;
    for (int i = 0; i < h; i++) s += (i + 1.0) * (std::log10(th[i]) - c[i]) * (std::log10(th[i]) - c[i]);
    return s;
}
static double nan_left_of_zero(const double *th, int h) { return std::log10(th[0]) < 0.0 ? kNan : quadratic(th, h); }
static double barrier_everywhere(const double *th, int h) { return 1e30 + 1e30 * quadratic(th, h); }
static double nan_everywhere(const double *, int) { return kNan; }

// ---- the box, the starts, the budget ----

static void box_and_budget() {
    const char *dense = "theta bounds must satisfy 0 < lo <= hi", *sparse = "sparse GP parameter bounds must satisfy 0 < lo <= hi";
    const double lo1[1] = {0.05}, hi1[1] = {5.0}, lo3[3] = {0.05, 0.05, 0.05}, hi3[3] = {5.0, 5.0, 5.0};
    fit::Log10Box a, b;
    std::string msg = "untouched";
    check(fit::log10_box(lo1, hi1, 1, 3, fit::Dense, a, msg) && fit::log10_box(lo3, hi3, 3, 3, fit::Sparse, b, msg) && msg == "untouched" &&
              a.lo.size() == 3 && same_bits(a.lo, b.lo) && same_bits(a.hi, b.hi) && same_bits(a.lo[2], std::log10(0.05)) && same_bits(a.hi[0], std::log10(5.0)),
          "box: one bound for all parameters is the full-length box, bit for bit");
    check(!fit::log10_box(lo3, hi3, 2, 3, fit::Dense, a, msg) && msg == "Bounds for theta should be either 1-dim or dim of xtrain (3), got 2",
          "box: a length that is neither 1 nor h");
    const double lo_zero[3] = {0.05, 0.0, 0.05}, hi_low[3] = {5.0, 5.0, 0.01}, lo_nan[3] = {kNan, 0.05, 0.05}, hi_nan[3] = {5.0, kNan, 5.0};
    check(!fit::log10_box(lo_zero, hi3, 3, 3, fit::Dense, a, msg) && msg == dense, "box: lo = 0, the dense text");
    check(!fit::log10_box(lo_zero, hi3, 3, 3, fit::Sparse, a, msg) && msg == sparse, "box: lo = 0, the sparse text");
    check(!fit::log10_box(lo3, hi_low, 3, 3, fit::Dense, a, msg) && msg == dense, "box: hi < lo, the dense text");
    check(!fit::log10_box(lo3, hi_low, 3, 3, fit::Sparse, a, msg) && msg == sparse, "box: hi < lo, the sparse text");
    check(!fit::log10_box(lo_nan, hi3, 3, 3, fit::Dense, a, msg) && msg == dense && !fit::log10_box(lo3, hi_nan, 3, 3, fit::Dense, a, msg) && msg == dense,
          "box: a NaN bound, the dense text");
    check(!fit::log10_box(lo_nan, hi3, 3, 3, fit::Sparse, a, msg) && msg == sparse && !fit::log10_box(lo3, hi_nan, 3, 3, fit::Sparse, a, msg) && msg == sparse,
          "box: a NaN bound, the sparse text");
    const double zero[4] = {1.0, 2.0, 0.0, 1.0}, neg[4] = {1.0, 2.0, 3.0, -1e-300}, tiny[4] = {1e-300, 1.0, 1e-300, 2.0};
    check(!fit::positive_starts(zero, 4, fit::Dense, msg) && msg == "theta start points must be > 0" &&
              !fit::positive_starts(zero, 4, fit::Sparse, msg) && msg == "sparse GP start points must be > 0",
          "starts: 0 is refused with the dense and the sparse text");
    check(!fit::positive_starts(neg, 4, fit::Dense, msg) && !fit::positive_starts(neg, 4, fit::Sparse, msg), "starts: a negative value is refused");
    msg = "untouched";
    check(fit::positive_starts(tiny, 4, fit::Dense, msg) && fit::positive_starts(zero, 2, fit::Sparse, msg) && msg == "untouched", "starts: 1e-300 passes");
    check(fit::cobyla_budget(1, 1000) == 25, "budget: h = 1 is the minimum 25");
    check(fit::cobyla_budget(3, 1000) == 30, "budget: h = 3 is 10 h");
    check(fit::cobyla_budget(200, 1000) == 1000, "budget: h = 200 is cut to max_eval = 1000");
    check(fit::cobyla_budget(1, 10) == 25 && fit::cobyla_budget(4, 10) == 40 && fit::cobyla_budget(4, 25) == 25, "budget: a max_eval below 25 is ignored");
}

// ---- the lock-step COBYLA driver, as fit_run_starts builds it ----

struct Trace {
    std::vector<vec> thetas;  // every full-width theta evaluated, in order
    int64_t rounds = 0;
};

static std::vector<StartResult> run_cobyla(const Objective &f, const vec &base, const std::vector<int> &active, const vec &theta0s, int64_t n_starts,
                                           const fit::Log10Box &box, int64_t max_eval, int rank, int world, Trace *trace = nullptr) {
    const int hfull = (int)base.size(), h = (int)active.size();
    std::vector<StartResult> results((size_t)n_starts, StartResult{kNan, vec((size_t)h, 0.0), 0});
    const std::vector<int64_t> mine = fit::shard(n_starts, rank, world);
    std::vector<CobylaBox> mach = fit::cobyla_machines(theta0s.data(), h, mine, box, fit::cobyla_budget(h, max_eval));
    vec thetas, lk;
    int rc = -1;
    const int64_t rounds = multistart::run(
        mach,
        [&](const multistart::Round &r) {
            fit::round_thetas(r, base.data(), hfull, active, thetas);
            lk.resize(r.size());
            for (size_t q = 0; q < r.size(); q++) {
                lk[q] = -f(thetas.data() + q * hfull, hfull);
                if (trace) trace->thetas.push_back(vec(thetas.begin() + q * hfull, thetas.begin() + (q + 1) * hfull));
            }
            return 0;
        },
        [&](const multistart::Round &, size_t q, CobylaBox &m) { m.tell(fit::cobyla_objective(true, lk[q])); }, rc);
    if (trace) trace->rounds = rounds;
    for (size_t q = 0; q < mach.size(); q++) results[(size_t)mine[q]] = fit::cobyla_result(mach[q]);
    return results;
}

// start s on a fresh machine of its own, by the plain loop
static StartResult cobyla_alone(const Objective &f, const vec &base, const std::vector<int> &active, const double *theta0, const fit::Log10Box &box,
                                int64_t budget) {
    const int h = (int)active.size();
    vec x0((size_t)h), x, th;
    for (int i = 0; i < h; i++) x0[i] = std::log10(theta0[i]);
    CobylaBox m(x0, box.lo, box.hi, 0.5, 1e-4, budget);
    while (m.ask(x)) {
        th = base;
        for (int i = 0; i < h; i++) th[active[i]] = std::pow(10.0, x[i]);
        const double v = f(th.data(), (int)th.size());
        m.tell(v == v ? v : kInf);
    }
    double fb = m.best_f();
    if (fb != fb || fb >= 1e30) fb = kInf;
    return StartResult{fb, m.best_x(), m.evals()};
}

static const vec kStarts5 = {0.05, 0.05, 0.05, 1.0, 0.5, 2.0, 0.3, 3.0, 0.8, 5.0, 0.4, 1.6, 2.0, 2.0, 0.1};  // 5 x 3; the first ON the lower bound

static void cobyla_driver() {
    const double lo1[1] = {0.05}, hi1[1] = {5.0};
    fit::Log10Box box;
    std::string msg;
    fit::log10_box(lo1, hi1, 1, 3, fit::Dense, box, msg);
    const std::vector<int> all = fit::all_active(3);
    const vec base = {1.0, 1.0, 1.0};
    for (int64_t n : {1, 2, 5}) {
        Trace tr;
        const std::vector<StartResult> got = run_cobyla(quadratic, base, all, kStarts5, n, box, 1000, 0, 1, &tr);
        bool ok = (int64_t)got.size() == n;
        int64_t longest = 0, shortest = 1 << 30, total = 0;
        for (int64_t s = 0; s < n; s++) {
            ok &= same(got[s], cobyla_alone(quadratic, base, all, kStarts5.data() + 3 * s, box, 30)) && std::isfinite(got[s].f);
            longest = std::max(longest, got[s].evals), shortest = std::min(shortest, got[s].evals), total += got[s].evals;
        }
        int64_t summed = -1;
        fit::best_start(got, &summed);
        ok &= tr.rounds == longest && (int64_t)tr.thetas.size() == total && summed == total && (n < 5 || shortest < longest);
        const std::string name = "cobyla: " + std::to_string(n) + " start(s) in lock-step end at the bits of each start alone";
        check(ok, name.c_str());
    }
    {  // starts 1 and 2 are the same point: equal minima, the first wins
        vec twice(kStarts5.begin(), kStarts5.begin() + 9);
        for (int i = 0; i < 3; i++) twice[6 + i] = twice[3 + i];
        twice[0] = 5.0, twice[1] = 0.05, twice[2] = 5.0;  // start 0 far from the optimum: it ends higher
        const std::vector<StartResult> got = run_cobyla(quadratic, base, all, twice, 3, box, 25, 0, 1);
        check(same(got[1], got[2]) && got[1].f < got[0].f && fit::best_start(got) == &got[1], "cobyla: the first of two equal minima wins");
    }
    {
        const std::vector<StartResult> bar = run_cobyla(barrier_everywhere, base, all, kStarts5, 1, box, 1000, 0, 1);
        const std::vector<StartResult> nan = run_cobyla(nan_everywhere, base, all, kStarts5, 1, box, 1000, 0, 1);
        const std::vector<StartResult> good = run_cobyla(nan_left_of_zero, base, all, vec(kStarts5.begin() + 3, kStarts5.end()), 1, box, 1000, 0, 1);
        check(bar[0].f == kInf && nan[0].f == kInf && bar[0].evals > 0 && std::isfinite(good[0].f) &&
                  same(good[0], cobyla_alone(nan_left_of_zero, base, all, kStarts5.data() + 3, box, 30)),
              "cobyla: a start that met only NaN or values >= 1e30 ends at +inf, NaN in a region is survived");
        std::vector<StartResult> mixed = {StartResult{kNan, {0, 0, 0}, 3}, bar[0], good[0], StartResult{kNan, {0, 0, 0}, 0}};
        int64_t evals = -1;
        check(fit::best_start(mixed, &evals) == &mixed[2] && evals == 3 + bar[0].evals + good[0].evals, "cobyla: a NaN and a 1e30 result are never the winner");
        const std::vector<StartResult> failed = {bar[0], nan[0]};
        const vec th = fit::winner_theta(base.data(), 3, all, fit::best_start(failed), kStarts5.data());
        check(fit::best_start(failed) == nullptr && same_bits(th, vec(kStarts5.begin(), kStarts5.begin() + 3)),
              "cobyla: when every start failed the winner is start 0's theta");
    }
}

static void sharding() {
    const double lo1[1] = {0.05}, hi1[1] = {5.0};
    fit::Log10Box box;
    std::string msg;
    fit::log10_box(lo1, hi1, 1, 3, fit::Dense, box, msg);
    const std::vector<int> all = fit::all_active(3);
    const vec base = {1.0, 1.0, 1.0};
    for (int64_t n : {2, 5}) {
        const std::vector<StartResult> whole = run_cobyla(quadratic, base, all, kStarts5, n, box, 1000, 0, 1);
        std::vector<StartResult> again((size_t)n, StartResult{kInf, vec(3, 0.0), 0});
        bool ok = true;
        for (int rank = 0; rank < 3; rank++) {
            Trace tr;
            const std::vector<StartResult> part = run_cobyla(quadratic, base, all, kStarts5, n, box, 1000, rank, 3, &tr);
            int64_t evals = -1;
            const StartResult *local = fit::best_start(part, &evals);  // (placeholders of the other ranks' starts: NaN, never the best)
            ok &= rank < n ? local && (local - part.data()) % 3 == rank : !local && evals == 0 && tr.rounds == 0;
            for (int64_t s = 0; s < n; s++)
                if (s % 3 == rank) again[s] = part[s];
                else ok &= part[s].f != part[s].f && part[s].evals == 0;
        }
        int64_t evals_a = -1, evals_b = -2;
        const StartResult *a = fit::best_start(whole, &evals_a), *b = fit::best_start(again, &evals_b);
        for (int64_t s = 0; s < n; s++) ok &= same(whole[s], again[s]);
        ok &= a && b && a - whole.data() == b - again.data() && evals_a == evals_b;
        const std::string name = "sharding: world 3, " + std::to_string(n) + " starts re-assembled are the unsharded run";
        check(ok, name.c_str());
    }
}

static void partial_active_set() {
    const double lo2[2] = {0.05, 0.1}, hi2[2] = {5.0, 3.0};
    fit::Log10Box box;
    std::string msg;
    fit::log10_box(lo2, hi2, 2, 2, fit::Dense, box, msg);
    const std::vector<int> active = {1, 3};
    const vec base = {0.7, 9.0, 0.4, 9.0}, starts = {0.05, 0.1, 1.0, 2.0, 0.3, 0.8};
    Trace tr;
    const std::vector<StartResult> got = run_cobyla(quadratic, base, active, starts, 3, box, 1000, 0, 1, &tr);
    bool ok = !tr.thetas.empty(), moved = false;
    for (const vec &th : tr.thetas) {
        ok &= th.size() == 4 && same_bits(th[0], base[0]) && same_bits(th[2], base[2]);
        moved |= th[1] != 9.0 && th[3] != 9.0;
    }
    check(ok && moved, "partial: inactive components of every evaluated theta are theta_base, bit for bit");
    const StartResult *b = fit::best_start(got);
    const vec th = fit::winner_theta(base.data(), 4, active, b, starts.data());
    const StartResult alone = cobyla_alone(quadratic, base, active, starts.data() + 2 * (b ? b - got.data() : 0), box, 25);
    check(b && same(*b, alone) && same_bits(th[0], base[0]) && same_bits(th[2], base[2]) &&
              same_bits(th[1], std::pow(10.0, alone.x[0])) && same_bits(th[3], std::pow(10.0, alone.x[1])),
          "partial: the winner is theta_base with 10^x of the best start in the active components");
    const vec keep = fit::winner_theta(base.data(), 4, active, nullptr, starts.data());
    check(same_bits(keep, vec({0.7, 0.05, 0.4, 0.1})), "partial: with no finite start, start 0 in the active components");
}

// ---- the lock-step L-BFGS driver, as egx_gp_fit_lbfgs builds it ----

// f and its gradient in x = log10(theta); fails (+inf, zero gradient) where theta_0 > 4
static bool quadratic_grad(const double *th, int h, double &f, vec &gx) {
    const double c[3] = {0.9, -0.4, 0.2};
    gx.assign((size_t)h, 0.0);
    f = kInf;
    if (th[0] > 4.0) return false;
    f = 1.5;
    for (int i = 0; i < h; i++) {
        const double t = std::log10(th[i]) - c[i];
        f += (i + 1.0) * t * t + 0.1 * t * t * t * t;
        gx[i] = 2.0 * (i + 1.0) * t + 0.4 * t * t * t;
    }
    return true;
}

static void lbfgs_driver() {
    const double lo1[1] = {0.05}, hi1[1] = {5.0};
    fit::Log10Box box;
    std::string msg;
    fit::log10_box(lo1, hi1, 1, 3, fit::Dense, box, msg);
    const vec starts = {0.05, 0.05, 0.05, 4.5, 0.5, 2.0, 0.3, 3.0, 0.8};  // start 1 begins where the evaluation fails
    const std::vector<int> all = fit::all_active(3);
    std::vector<LbfgsStart> mach = fit::lbfgs_machines(starts.data(), 3, fit::shard(3, 0, 1), box, 50);
    std::vector<int64_t> asked(3, 0);
    vec thetas, fs, gs, gx;
    int rc = -1;
    int64_t evals = 0;
    multistart::run(
        mach,
        [&](const multistart::Round &r) {
            fit::round_thetas(r, starts.data(), 3, all, thetas);
            fs.resize(r.size()), gs.clear();
            evals += (int64_t)r.size();
            for (size_t q = 0; q < r.size(); q++) {
                quadratic_grad(thetas.data() + 3 * q, 3, fs[q], gx);
                gs.insert(gs.end(), gx.begin(), gx.end());
                asked[r.who[q]]++;
            }
            return 0;
        },
        [&](const multistart::Round &, size_t q, LbfgsStart &m) { m.tell(fs[q], vec(gs.begin() + 3 * q, gs.begin() + 3 * (q + 1))); }, rc);
    bool ok = rc == 0 && evals == asked[0] + asked[1] + asked[2];
    std::vector<StartResult> results;
    for (int s = 0; s < 3; s++) {
        LbfgsStart m(starts.data() + 3 * s, 3, box.lo, box.hi, 50);
        vec x, th(3);
        double f;
        int64_t n = 0;
        while (m.ask(x)) {
            for (int i = 0; i < 3; i++) th[i] = std::pow(10.0, x[i]);
            quadratic_grad(th.data(), 3, f, gx);
            m.tell(f, gx);
            n++;
        }
        ok &= same_bits(m.f, mach[s].f) && same_bits(m.x, mach[s].x) && n == asked[s];
        results.push_back(StartResult{mach[s].f, mach[s].x, 0});
    }
    check(ok && asked[0] > 2 && asked[2] > 2 && asked[0] != asked[2], "lbfgs: three starts in lock-step end at the bits of each start alone");
    const StartResult *b = fit::best_start(results);
    check(asked[1] == 1 && mach[1].f == kInf && b && b != &results[1], "lbfgs: a start whose first evaluation fails ends after one point and never wins");
}

// ---- machines start-major, model-minor, as egx_gp_fit_multi lays them out ----

typedef std::tuple<int64_t, std::vector<int>> Call;  // (start index, the models evaluated together)

static void fit_multi_layout() {
    const int k = 3, h = 2;
    const int64_t n_starts = 2;
    // three models: another centre and another curvature each, so their machines end after different numbers of rounds
    auto model = [](int m, const double *th) {
        const double cx[3] = {0.9, -0.2, 0.1}, cy[3] = {-0.4, 0.3, -1.1}, w[3] = {1.0, 30.0, 0.05};
        const double a = std::log10(th[0]) - cx[m], b = std::log10(th[1]) - cy[m];
        return 2.0 + w[m] * (a * a + 3.0 * b * b) + 0.5 * m;
    };
    const double lo1[1] = {0.05}, hi1[1] = {5.0};
    fit::Log10Box box;
    std::string msg;
    fit::log10_box(lo1, hi1, 1, h, fit::Dense, box, msg);
    const vec theta0s = {0.05, 0.05, 1.0, 0.4, 0.5, 0.5, 1.0, 0.4, 0.05, 5.0, 2.5, 0.06};  // k x n_starts x h, model-major
    const int64_t budget = 40;
    std::vector<int64_t> rows;
    for (int64_t st = 0; st < n_starts; st++)
        for (int m = 0; m < k; m++) rows.push_back(m * n_starts + st);
    std::vector<CobylaBox> mach = fit::cobyla_machines(theta0s.data(), h, rows, box, budget);
    const std::vector<int> all = fit::all_active(h);
    std::vector<Call> calls;
    vec thetas, lk;
    bool contiguous = true;
    int rc = -1;
    multistart::run(
        mach,
        [&](const multistart::Round &r) {
            fit::round_thetas(r, theta0s.data(), h, all, thetas);
            lk.assign(r.size(), kNan);
            size_t covered = 0;
            int64_t last = -1;
            const int rc_each = fit::for_each_start(r, k, [&](int64_t st, size_t q0, size_t count) {
                std::vector<int> members;
                for (size_t q = q0; q < q0 + count; q++) {
                    contiguous &= (int64_t)(r.who[q] / k) == st && (q == q0 || r.who[q] > r.who[q - 1]);
                    members.push_back((int)(r.who[q] % k));
                    lk[q] = -model(members.back(), thetas.data() + q * h);
                }
                contiguous &= q0 == covered && st > last && count > 0;
                covered += count, last = st;
                calls.push_back(Call(st, members));
                return 0;
            });
            contiguous &= covered == r.size();
            return rc_each;
        },
        [&](const multistart::Round &, size_t q, CobylaBox &m) { m.tell(fit::cobyla_objective(true, lk[q])); }, rc);
    check(rc == 0 && contiguous && !calls.empty(), "fit_multi: a round's points are contiguous per start index, starts and models in increasing order");
    bool own = true;
    std::vector<int64_t> lens;
    for (int m = 0; m < k; m++)
        for (int64_t st = 0; st < n_starts; st++) {
            const Objective f = [&](const double *th, int) { return model(m, th); };
            const StartResult alone = cobyla_alone(f, vec(2, 1.0), all, theta0s.data() + (m * n_starts + st) * h, box, budget);
            own &= same(fit::cobyla_result(mach[(size_t)(st * k + m)]), alone);
            lens.push_back(alone.evals);
        }
    bool unequal = false;
    for (int64_t l : lens) unequal |= l != lens[0];
    check(own && unequal, "fit_multi: every machine walked its own model's trajectory (it saw no other model's value)");
    // the nested loop egx_gp_fit_multi was before it shared the driver
    std::vector<Call> want;
    {
        std::vector<std::vector<CobylaBox>> old((size_t)k);
        for (int m = 0; m < k; m++)
            for (int64_t st = 0; st < n_starts; st++) old[m].push_back(fit::cobyla_machines(theta0s.data(), h, {m * n_starts + st}, box, budget)[0]);
        vec x, th(2);
        for (bool any = true; any;) {
            any = false;
            for (int64_t st = 0; st < n_starts; st++) {
                std::vector<int> members;
                std::vector<vec> pts;
                for (int m = 0; m < k; m++)
                    if (old[m][st].ask(x)) members.push_back(m), pts.push_back(x);
                if (members.empty()) continue;
                any = true;
                want.push_back(Call(st, members));
                for (size_t q = 0; q < members.size(); q++) {
                    th[0] = std::pow(10.0, pts[q][0]), th[1] = std::pow(10.0, pts[q][1]);
                    old[members[q]][st].tell(model(members[q], th.data()));
                }
            }
        }
    }
    bool partial = false;
    for (const Call &c : calls) partial |= (int)std::get<1>(c).size() < k;
    check(calls == want && partial, "fit_multi: the (start index, member subset) calls are those of the nested loop it replaced");
}

// ---- one machine after the other, as the sparse fits run ----

static void sequential() {
    const double lo1[1] = {0.05}, hi1[1] = {5.0};
    fit::Log10Box box;
    std::string msg;
    fit::log10_box(lo1, hi1, 1, 3, fit::Sparse, box, msg);
    const std::vector<int> all = fit::all_active(3);
    const vec base = {1.0, 1.0, 1.0};
    std::vector<CobylaBox> mach = fit::cobyla_machines(kStarts5.data(), 3, fit::shard(3, 0, 1), box, 30);
    std::vector<size_t> sizes;
    double f = 0.0;
    int rc = -1;
    fit::run_sequential(
        mach,
        [&](const multistart::Round &r) {
            vec th(3);
            fit::set_active(r.pts.data(), all, th.data());
            f = quadratic(th.data(), 3);
            sizes.push_back(r.size());
            return 0;
        },
        [&](const multistart::Round &, size_t, CobylaBox &m) { m.tell(f); }, rc);
    bool ok = rc == 0;
    int64_t total = 0;
    for (int s = 0; s < 3; s++) {
        const StartResult alone = cobyla_alone(quadratic, base, all, kStarts5.data() + 3 * s, box, 30);
        ok &= same(fit::cobyla_result(mach[s]), alone);
        total += alone.evals;
    }
    for (size_t n : sizes) ok &= n == 1;
    check(ok && (int64_t)sizes.size() == total, "sequential: one point per round, every start ends at the bits of the start alone");
    std::vector<CobylaBox> again = fit::cobyla_machines(kStarts5.data(), 3, fit::shard(3, 0, 1), box, 30);
    int calls = 0;
    fit::run_sequential(
        again, [&](const multistart::Round &) { return ++calls == 4 ? 7 : 0; }, [&](const multistart::Round &, size_t, CobylaBox &m) { m.tell(1.0); }, rc);
    check(rc == 7 && calls == 4 && again[0].evals() == 3 && again[1].evals() == 0 && again[2].evals() == 0,
          "sequential: a failed evaluation ends the fit at once, later starts never run");
}

int main() {
    box_and_budget();
    cobyla_driver();
    sharding();
    partial_active_set();
    lbfgs_driver();
    fit_multi_layout();
    sequential();
    return failures ? 1 : 0;
}
