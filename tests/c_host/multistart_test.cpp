// Host-only checks of csrc/multistart.h (no HIP, no library): the lock-step round loop on scripted machines and on the real
// CobylaBox / Cobyla / Slsqp, the winner rules, the argument check.  Prints "ok <name>" or "FAILED <name>" per check; exit
// status 1 on a failure.  tests/test_multistart_cpu.py builds and runs it, once more under the address and UB sanitizers.
// The analytic problems are A..D of cobyla_cstr_trace.cpp / slsqp_trace.cpp (c(x) <= 0 feasible).
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <string>

#include "../../egobox_amd/csrc/cobyla.h"
#include "../../egobox_amd/csrc/slsqp.h"
#include "../../egobox_amd/csrc/multistart.h"
using namespace egx;

typedef std::vector<double> vec;

static int failures = 0;
static void check(bool ok, const char *name) {
    printf("%s %s\n", ok ? "ok" : "FAILED", name);
    if (!ok) failures++;
}

// ---- scripted machines ----

// replays a fixed list of points; remembers what it was told
struct Scripted {
    std::vector<vec> asks;
    size_t next = 0;
    vec told;
    bool ask(vec &x) {
        if (next >= asks.size()) return false;
        x = asks[next];
        return true;
    }
    void tell(double v) {
        told.push_back(v);
        next++;
    }
};

static double tag(const double *x) { return 1000.0 * x[0] + x[1]; }  // point (machine, step) -> a value of its own

static void scripted_rounds() {
    const size_t len[3] = {1, 3, 5};
    std::vector<Scripted> mach(3);
    for (size_t s = 0; s < 3; s++)
        for (size_t i = 0; i < len[s]; i++) mach[s].asks.push_back({(double)s, (double)i});
    std::vector<std::vector<size_t>> who;
    std::vector<vec> pts;
    vec vals;
    int rc = -1;
    const int64_t rounds = multistart::run(
        mach,
        [&](const multistart::Round &r) {
            who.push_back(r.who);
            pts.push_back(r.pts);
            vals.resize(r.size());
            for (size_t q = 0; q < r.size(); q++) vals[q] = tag(r.pts.data() + 2 * q);
            return 0;
        },
        [&](const multistart::Round &, size_t q, Scripted &m) { m.tell(vals[q]); }, rc);
    check(rc == 0 && rounds == 5 && who.size() == 5, "scripted: rounds equals the longest list");
    bool order = true, points = true;
    for (size_t r = 0; r < who.size(); r++) {
        std::vector<size_t> expect;
        vec xs;
        for (size_t s = 0; s < 3; s++)
            if (len[s] > r) expect.push_back(s), xs.push_back((double)s), xs.push_back((double)r);
        order &= who[r] == expect;
        points &= pts[r] == xs;
    }
    check(order, "scripted: machine-index order, finished machines skipped");
    check(points, "scripted: the evaluator sees the round's points in that order");
    bool answers = true;
    for (size_t s = 0; s < 3; s++) {
        answers &= mach[s].told.size() == len[s];
        for (size_t i = 0; i < mach[s].told.size(); i++) answers &= mach[s].told[i] == 1000.0 * s + i;
    }
    check(answers, "scripted: every answer reaches the machine that asked");
    // a failed evaluation ends the loop: its code comes back, nothing of that round is told
    std::vector<Scripted> again(2);
    again[0].asks = {{0, 0}, {0, 1}}, again[1].asks = {{1, 0}, {1, 1}};
    int calls = 0;
    const int64_t r2 = multistart::run(
        again, [&](const multistart::Round &) { return ++calls == 2 ? 7 : 0; }, [&](const multistart::Round &, size_t, Scripted &m) { m.tell(0.0); }, rc);
    check(rc == 7 && r2 == 1 && again[0].told.size() == 1 && again[1].told.size() == 1, "scripted: a failed evaluation stops the rounds");
    std::vector<Scripted> none;
    check(multistart::run(none, [&](const multistart::Round &) { return 0; }, [&](const multistart::Round &, size_t, Scripted &) {}, rc) == 0 && rc == 0,
          "scripted: no machine, no round");
}

// ---- the real machines ----

struct Problem {
    int m = 0;
    vec x0, lo, hi;
    std::function<double(const vec &, double *)> f;          // value; gradient into the pointer
    std::function<void(const vec &, double *, double *)> c;  // values; Jacobian (m x n, row-major)
};

static Problem make_case(int cs) {
    Problem p;
    if (cs == 0) {  // A: the unit disc cuts off the unconstrained optimum
        p.f = [](const vec &x, double *g) {
            g[0] = 2 * (x[0] - 1.2), g[1] = 2 * (x[1] - 0.9);
            return (x[0] - 1.2) * (x[0] - 1.2) + (x[1] - 0.9) * (x[1] - 0.9);
        };
        p.c = [](const vec &x, double *o, double *J) {
            o[0] = -(1.0 - x[0] * x[0] - x[1] * x[1]);
            J[0] = 2 * x[0], J[1] = 2 * x[1];
        };
        p.m = 1, p.x0 = {0.1, 0.2}, p.lo = {-2, -2}, p.hi = {2, 2};
    } else if (cs == 1) {  // B: one active, one inactive constraint
        p.f = [](const vec &x, double *g) {
            g[0] = 1 + 0.3 * std::cos(3 * x[0]), g[1] = 1;
            return x[0] + x[1] + 0.1 * std::sin(3 * x[0]);
        };
        p.c = [](const vec &x, double *o, double *J) {
            o[0] = -(x[0] * x[1] - 0.25);
            o[1] = -(1.5 - x[0] - 0.5 * x[1] * x[1]);
            J[0] = -x[1], J[1] = -x[0], J[2] = 1, J[3] = x[1];
        };
        p.m = 2, p.x0 = {1, 1}, p.lo = {0, 0}, p.hi = {2, 2};
    } else if (cs == 2) {  // C: four variables, three constraints
        p.f = [](const vec &x, double *g) {
            double s = 0;
            for (int i = 0; i < 4; i++) {
                const double t = x[i] - 0.3 * i + 0.5;
                s += (i + 1) * t * t;
                g[i] = 2 * (i + 1) * t;
            }
            return s;
        };
        p.c = [](const vec &x, double *o, double *J) {
            double ss = 0, s = 0;
            for (int i = 0; i < 4; i++) ss += x[i] * x[i], s += x[i];
            o[0] = -(0.5 - ss);
            o[1] = -(s + 0.2);
            o[2] = -(std::cos(x[1]) - 0.8 - x[3]);
            for (int i = 0; i < 4; i++) J[i] = 2 * x[i], J[4 + i] = -1, J[8 + i] = 0;
            J[8 + 1] = std::sin(x[1]), J[8 + 3] = 1;
        };
        p.m = 3, p.x0 = {0.1, 0.1, 0.1, 0.1}, p.lo = {-2, -2, -2, -2}, p.hi = {2, 2, 2, 2};
    } else {  // D: the upper bound of x0 is active beside the nonlinear constraint
        p.f = [](const vec &x, double *g) {
            g[0] = -x[1] * x[2], g[1] = -x[0] * x[2], g[2] = -x[0] * x[1];
            return -x[0] * x[1] * x[2];
        };
        p.c = [](const vec &x, double *o, double *J) {
            o[0] = -(1.0 - x[0] * x[0] - 2 * x[1] * x[1] - 3 * x[2] * x[2]);
            J[0] = 2 * x[0], J[1] = 4 * x[1], J[2] = 6 * x[2];
        };
        p.m = 1, p.x0 = {0.3, 0.3, 0.3}, p.lo = {0, 0, 0}, p.hi = {0.45, 1, 1};
    }
    return p;
}

// three starts of a problem: its own, one towards the lower corner, one outside the box (the machines clamp it)
static std::vector<vec> starts_of(const Problem &p) {
    std::vector<vec> s(3, p.x0);
    for (size_t i = 0; i < p.x0.size(); i++) {
        s[1][i] = p.lo[i] + 0.25 * (p.hi[i] - p.lo[i]) + 0.01 * i;
        s[2][i] = p.hi[i] + 0.5 - 0.3 * i;
    }
    return s;
}

static const int64_t kBudget = 60;
static CobylaBox make_box(const Problem &p, const vec &x0) { return CobylaBox(x0, p.lo, p.hi, 0.5, 1e-4, kBudget, 0.0, true, true, 1e-4); }
static Cobyla make_cobyla(const Problem &p, const vec &x0) { return Cobyla(x0, p.lo, p.hi, p.m, 0.5, 1e-4, 1e-4, kBudget, 0.0, true, true, {}); }
static Slsqp make_slsqp(const Problem &p, const vec &x0) { return Slsqp(x0, p.lo, p.hi, p.m, 1e-4, 1e-4, kBudget, {}); }

// the tells of the three machine types from one evaluation of the problem at x
static void answer(const Problem &p, const vec &x, CobylaBox &m) {
    vec g(x.size());
    m.tell(p.f(x, g.data()));
}
static void answer(const Problem &p, const vec &x, Cobyla &m) {
    vec g(x.size()), c((size_t)p.m + 1), J((size_t)p.m * x.size() + 1);
    const double v = p.f(x, g.data());
    p.c(x, c.data(), J.data());
    m.tell(v, c.data());
}
static void answer(const Problem &p, const vec &x, Slsqp &m) {
    vec g(x.size()), c((size_t)p.m + 1), J((size_t)p.m * x.size() + 1);
    const double v = p.f(x, g.data());
    p.c(x, c.data(), J.data());
    m.tell(v, c.data(), g.data(), J.data());
}

// every start of every problem: the points it walks in lock-step with two companions are the points it walks alone
template <class Machine, class Make>
static bool lockstep_walks_alone(Make make) {
    bool same = true;
    for (int cs = 0; cs < 4; cs++) {
        const Problem p = make_case(cs);
        const std::vector<vec> starts = starts_of(p);
        const size_t n = p.x0.size();
        std::vector<std::vector<vec>> alone(3), together(3);
        std::vector<int64_t> evals_alone(3);
        for (size_t s = 0; s < 3; s++) {
            std::vector<Machine> one;
            one.push_back(make(p, starts[s]));
            int rc = 0;
            multistart::run(
                one, [&](const multistart::Round &r) { alone[s].push_back(r.pts); return 0; },
                [&](const multistart::Round &r, size_t q, Machine &m) { answer(p, vec(r.pts.begin() + q * n, r.pts.begin() + (q + 1) * n), m); }, rc);
            evals_alone[s] = one[0].evals();
        }
        std::vector<Machine> mach;
        for (size_t s = 0; s < 3; s++) mach.push_back(make(p, starts[s]));
        int rc = 0;
        const int64_t rounds = multistart::run(
            mach,
            [&](const multistart::Round &r) {
                for (size_t q = 0; q < r.size(); q++) together[r.who[q]].push_back(vec(r.pts.begin() + q * n, r.pts.begin() + (q + 1) * n));
                return 0;
            },
            [&](const multistart::Round &r, size_t q, Machine &m) { answer(p, vec(r.pts.begin() + q * n, r.pts.begin() + (q + 1) * n), m); }, rc);
        int64_t longest = 0;
        for (size_t s = 0; s < 3; s++) {
            same &= together[s] == alone[s] && mach[s].evals() == evals_alone[s] && !alone[s].empty();  // vector<double> ==: bit for bit but for -0 / NaN, which no point holds
            longest = std::max<int64_t>(longest, (int64_t)alone[s].size());
        }
        same &= rounds == longest;
    }
    return same;
}

static void real_machines() {
    check(lockstep_walks_alone<CobylaBox>(make_box), "CobylaBox: three starts in lock-step walk the points each walks alone");
    check(lockstep_walks_alone<Cobyla>(make_cobyla), "Cobyla: three starts in lock-step walk the points each walks alone");
    check(lockstep_walks_alone<Slsqp>(make_slsqp), "Slsqp: three starts in lock-step walk the points each walks alone");
}

// ---- the winner rules ----

// a Cobyla over [0, 1]^2 with one constraint (feasible: c <= 0.25) that has been told one point
static Cobyla told_once(double f, double c) {
    Cobyla m({0.5, 0.5}, {0, 0}, {1, 1}, 1, 0.5, 1e-4, 1e-4, 10, 0.0, true, true, {0.25});
    vec x;
    m.ask(x);
    m.tell(f, &c);
    return m;
}
static Slsqp told_once_slsqp(double f, double c) {
    Slsqp m({0.5, 0.5}, {0, 0}, {1, 1}, 1, 1e-4, 1e-4, 10, {0.25});
    vec x;
    bool want = false;
    m.ask(x, want);
    const double g[2] = {1.0, -0.5}, J[2] = {0.3, 0.2};
    m.tell(f, &c, g, J);
    return m;
}

static void winner_rules() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    {
        std::vector<Cobyla> a = {told_once(1.0, 0.9), told_once(9.0, 0.1), told_once(0.5, 0.5)};
        check(multistart::winner(a) == 1 && multistart::better(a[1], a[0]) && !multistart::better(a[0], a[1]), "winner: feasible beats infeasible");
        std::vector<Cobyla> b = {told_once(3.0, 0.2), told_once(2.0, 0.25), told_once(2.5, -1.0)};
        check(multistart::winner(b) == 1, "winner: among feasible starts the smaller key");
        std::vector<Cobyla> c = {told_once(1.0, 0.9), told_once(5.0, 0.4), told_once(0.1, 0.6)};
        check(multistart::winner(c) == 1, "winner: among infeasible starts the smaller violation");
        std::vector<Cobyla> d = {told_once(7.0, 0.5), told_once(2.0, 0.1), told_once(2.0, 0.1), told_once(2.0, 0.0)};
        check(multistart::winner(d) == 1 && !multistart::better(d[2], d[1]) && !multistart::better(d[1], d[2]), "winner: the first start on an exact tie");
        std::vector<Cobyla> e = {told_once(4.0, 0.9), told_once(4.0, 0.9)};
        check(multistart::winner(e) == 0, "winner: the first start on an infeasible tie");
    }
    {  // nothing finite anywhere: "all starts" (egx_infill_optimize_cstr) against "start 0" (egx_infill_optimize_slsqp)
        std::vector<Cobyla> a = {told_once(nan, 0.9), told_once(1e30, 0.5), told_once(nan, 0.3)};
        check(!multistart::any_finite(a) && multistart::winner(a) == 2, "no finite value: the ordering over all starts still picks");
        std::vector<Slsqp> s = {told_once_slsqp(nan, 0.9), told_once_slsqp(1e30, 0.5), told_once_slsqp(nan, 0.3)};
        check(!multistart::any_finite(s) && multistart::winner(s, multistart::any_finite(s)) == 0 && multistart::winner(s) == 2,
              "no finite value: the start-0 rule stays at start 0");
        std::vector<Slsqp> t = {told_once_slsqp(nan, 0.9), told_once_slsqp(3.0, 0.5), told_once_slsqp(2.0, 0.3)};
        check(multistart::any_finite(t) && multistart::winner(t, multistart::any_finite(t)) == 2, "one finite value: the start-0 rule compares");
    }
    {  // the own-best rule of egx_infill_optimize
        const double lo[2] = {0, 0}, hi[2] = {1, 2}, xs[6] = {-3.0, 0.5, 0.25, 7.0, 0.5, 0.5};
        multistart::BestEvaluated seen(lo, hi, xs, 3, 2);
        check(seen.x == vec({0.0, 0.5, 0.25, 2.0, 0.5, 0.5}) && std::isinf(seen.f[0]) && seen.winner() == 0,
              "own best: begins at the start clamped into the box, start 0 while nothing is finite");
        const double p0[2] = {0.1, 0.1}, p1[2] = {0.2, 0.2}, p2[2] = {0.3, 0.3}, p3[2] = {0.4, 0.4};
        seen.told(1, nan, p0);
        seen.told(1, 1e30, p1);
        seen.told(2, std::numeric_limits<double>::infinity(), p2);
        check(seen.x == vec({0.0, 0.5, 0.25, 2.0, 0.5, 0.5}) && seen.winner() == 0, "own best: NaN and values at or beyond 1e30 do not count");
        seen.told(2, 4.0, p2);
        seen.told(1, 4.0, p1);
        seen.told(1, 4.0, p3);
        check(seen.winner() == 1 && seen.f[1] == 4.0 && seen.x[2] == 0.2 && seen.x[3] == 0.2, "own best: the first point of a start and the first start win ties");
        seen.told(2, 9.99e29, p3);
        seen.told(0, 3.5, p0);
        check(seen.winner() == 0 && seen.f[2] == 4.0 && seen.x[0] == 0.1, "own best: the smallest value told");
    }
}

// ---- the argument check ----

static void argument_check() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1}, xs[6] = {0.5, 0.5, 0.5, 2.0, -1.0, 0.5};
    std::string msg = "untouched";
    check(multistart::check_box_and_starts(lo, hi, xs, 2, 3, msg) && msg == "untouched", "arguments: a box and starts outside it pass");
    const double lo_bad[3] = {0, 2, 0};
    check(!multistart::check_box_and_starts(lo_bad, hi, xs, 2, 3, msg) && msg == "infill optimize: bounds must be finite with lo <= hi (coordinate 1)",
          "arguments: lo > hi names the coordinate");
    const double hi_inf[3] = {1, 1, inf};
    check(!multistart::check_box_and_starts(lo, hi_inf, xs, 2, 3, msg) && msg == "infill optimize: bounds must be finite with lo <= hi (coordinate 2)",
          "arguments: an infinite bound names the coordinate");
    const double lo_nan[3] = {nan, 0, 0};
    check(!multistart::check_box_and_starts(lo_nan, hi, xs, 2, 3, msg) && msg == "infill optimize: bounds must be finite with lo <= hi (coordinate 0)",
          "arguments: a NaN bound names the coordinate");
    const double xs_nan[6] = {0.5, 0.5, 0.5, 0.5, nan, 0.5};
    check(!multistart::check_box_and_starts(lo, hi, xs_nan, 2, 3, msg) && msg == "infill optimize: start point 1 has a non-finite coordinate",
          "arguments: a NaN start coordinate names the start");
    const double xs_inf[6] = {-inf, 0.5, 0.5, 0.5, 0.5, 0.5};
    check(!multistart::check_box_and_starts(lo, hi, xs_inf, 2, 3, msg) && msg == "infill optimize: start point 0 has a non-finite coordinate",
          "arguments: an infinite start coordinate names the start");
    check(multistart::budget(0, 5, 3) == 150 && multistart::budget(-1, 100, 3) == 2000 && multistart::budget(60, 5, 3) == 60,
          "arguments: the budget defaults to min(10 n_start d, 2000)");
}

int main() {
    scripted_rounds();
    real_machines();
    winner_rules();
    argument_check();
    return failures ? 1 : 0;
}
