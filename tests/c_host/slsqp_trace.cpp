// Host-only harness for egx::Slsqp (csrc/slsqp.h, no HIP).  tests/test_slsqp_cpu.py drives it:
//   slsqp_trace <case 0..3 = A..D> <ftol> <maxeval>
//       the four problems of cobyla_cstr_trace.cpp with analytic gradients.  Prints "P x.. f c.." for every point asked,
//       "I x.." whenever a point becomes the iterate (the start point first), then two summary lines.
//   slsqp_trace qp <seed> <count>
//       random strictly convex subproblems against a dense enumeration of active sets; one line per problem:
//       "Q n m kkt <residual / scale> dx <|s - s_enum|> enum <0|1: the enumeration found the constraints consistent> mode"
//   slsqp_trace ldl <seed> <count>      rank-one updates of the packed factor against the dense matrix: "L <error>"
//   slsqp_trace contracts               the machine's contracts; "ok <name>" per check, exit status 1 on a failure
// Constraints are in the class's convention, c(x) <= 0 feasible.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <string>

#include "../../egobox_amd/csrc/slsqp.h"
using namespace egx;

typedef std::vector<double> vec;

struct Problem {
    int m = 0;
    vec x0, lo, hi;
    std::function<double(const vec &, double *)> f;           // value; gradient into the pointer
    std::function<void(const vec &, double *, double *)> c;   // values; Jacobian (m x n, row-major)
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

static void print_vec(const vec &v) {
    for (double t : v) printf(" %.17g", t);
}

static int run_case(int cs, double ftol, long maxeval) {
    Problem p = make_case(cs);
    const int n = (int)p.x0.size(), m = p.m;
    Slsqp opt(p.x0, p.lo, p.hi, m, ftol, ftol, maxeval);
    vec x, g((size_t)n), cv((size_t)m + 1), J((size_t)m * n + 1);
    bool want = false;
    int64_t acc = 0;
    while (opt.ask(x, want)) {
        const double v = p.f(x, g.data());
        p.c(x, cv.data(), J.data());
        printf("P");
        print_vec(x);
        printf(" %.17g", v);
        for (int j = 0; j < m; j++) printf(" %.17g", cv[j]);
        printf("\n");
        opt.tell(v, cv.data(), g.data(), J.data());
        if (opt.accepted() != acc) {
            acc = opt.accepted();
            printf("I");
            print_vec(opt.current_x());
            printf("\n");
        }
    }
    printf("# final status %d evals %ld iters %ld augmented %ld f %.17g x", (int)opt.status(), (long)opt.evals(),
           (long)opt.iterations(), (long)opt.augmented(), opt.current_f());
    print_vec(opt.current_x());
    printf("\n# best feasible %d violation %.17g f %.17g x", opt.best_feasible() ? 1 : 0, opt.best_violation(), opt.best_f());
    print_vec(opt.best_x());
    printf(" c");
    print_vec(opt.best_c());
    printf("\n");
    return 0;
}

// ---- dense helpers for the subproblem checks ----

// Gaussian elimination with partial pivoting; false when singular
static bool solve_dense(int n, vec A, vec b, vec &x) {
    for (int c = 0; c < n; c++) {
        int piv = c;
        for (int r = c + 1; r < n; r++)
            if (std::fabs(A[(size_t)r * n + c]) > std::fabs(A[(size_t)piv * n + c])) piv = r;
        if (std::fabs(A[(size_t)piv * n + c]) < 1e-11) return false;
        if (piv != c) {
            for (int j = 0; j < n; j++) std::swap(A[(size_t)piv * n + j], A[(size_t)c * n + j]);
            std::swap(b[piv], b[c]);
        }
        for (int r = c + 1; r < n; r++) {
            const double f = A[(size_t)r * n + c] / A[(size_t)c * n + c];
            if (f == 0.0) continue;
            for (int j = c; j < n; j++) A[(size_t)r * n + j] -= f * A[(size_t)c * n + j];
            b[r] -= f * b[c];
        }
    }
    x.assign((size_t)n, 0.0);
    for (int r = n - 1; r >= 0; r--) {
        double s = b[r];
        for (int j = r + 1; j < n; j++) s -= A[(size_t)r * n + j] * x[j];
        x[r] = s / A[(size_t)r * n + r];
    }
    return true;
}

// packed L D L^T of a dense positive definite matrix
static vec factor(int n, const vec &B) {
    vec L((size_t)n * n, 0.0), D((size_t)n), out((size_t)n * (n + 1) / 2);
    for (int j = 0; j < n; j++) {
        double d = B[(size_t)j * n + j];
        for (int k = 0; k < j; k++) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k] * D[k];
        D[j] = d;
        for (int i = j + 1; i < n; i++) {
            double v = B[(size_t)i * n + j];
            for (int k = 0; k < j; k++) v -= L[(size_t)i * n + k] * L[(size_t)j * n + k] * D[k];
            L[(size_t)i * n + j] = v / d;
        }
    }
    for (int i = 0; i < n; i++) {
        out[slsqp_detail::ldl_diag(n, i)] = D[i];
        for (int j = i + 1; j < n; j++) out[slsqp_detail::ldl_diag(n, i) + (size_t)(j - i)] = L[(size_t)j * n + i];
    }
    return out;
}

static vec unpack(int n, const vec &p) {
    vec B((size_t)n * n, 0.0);
    auto L = [&](int j, int i) { return j == i ? 1.0 : p[slsqp_detail::ldl_diag(n, i) + (size_t)(j - i)]; };
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            double s = 0;
            for (int k = 0; k <= std::min(i, j); k++) s += L(i, k) * p[slsqp_detail::ldl_diag(n, k)] * L(j, k);
            B[(size_t)i * n + j] = s;
        }
    return B;
}

// The minimiser of 1/2 s^T B s + g^T s, A s + b >= 0, lo <= s <= hi by enumeration: every assignment of the variables to
// {free, at lo, at hi} and every subset of the general constraints held as equalities; the (unique) candidate that is
// feasible with multipliers of the right sign is the solution.  False when no active set passes: inconsistent.
static bool enumerate(int n, const vec &B, const vec &g, int m, const vec &A, const vec &b, const vec &lo, const vec &hi, vec &s) {
    const double tol = 1e-9;
    std::vector<int> state((size_t)n, 0);
    for (;;) {
        std::vector<int> fr;
        vec base((size_t)n, 0.0);
        for (int i = 0; i < n; i++) {
            if (state[i] == 0) fr.push_back(i);
            else base[i] = state[i] == 1 ? lo[i] : hi[i];
        }
        const int nf = (int)fr.size();
        for (int mask = 0; mask < (1 << m); mask++) {
            std::vector<int> act;
            for (int j = 0; j < m; j++)
                if (mask >> j & 1) act.push_back(j);
            const int na = (int)act.size();
            if (na > nf) continue;
            const int N = nf + na;
            vec K((size_t)N * N, 0.0), rhs((size_t)N, 0.0), sol;
            for (int a = 0; a < nf; a++) {
                for (int c = 0; c < nf; c++) K[(size_t)a * N + c] = B[(size_t)fr[a] * n + fr[c]];
                double v = -g[fr[a]];
                for (int i = 0; i < n; i++) v -= B[(size_t)fr[a] * n + i] * base[i];
                rhs[a] = v;
                for (int q = 0; q < na; q++) K[(size_t)a * N + nf + q] = -A[(size_t)act[q] * n + fr[a]], K[(size_t)(nf + q) * N + a] = A[(size_t)act[q] * n + fr[a]];
            }
            for (int q = 0; q < na; q++) {
                double v = -b[act[q]];
                for (int i = 0; i < n; i++) v -= A[(size_t)act[q] * n + i] * base[i];
                rhs[nf + q] = v;
            }
            if (N > 0 && !solve_dense(N, K, rhs, sol)) continue;
            vec cand = base;
            for (int a = 0; a < nf; a++) cand[fr[a]] = sol[a];
            bool ok = true;
            for (int q = 0; q < na && ok; q++) ok = sol[nf + q] >= -tol;
            for (int i = 0; i < n && ok; i++) ok = cand[i] >= lo[i] - tol && cand[i] <= hi[i] + tol;
            for (int j = 0; j < m && ok; j++) {
                double v = b[j];
                for (int i = 0; i < n; i++) v += A[(size_t)j * n + i] * cand[i];
                ok = v >= -tol;
            }
            for (int i = 0; i < n && ok; i++) {  // the multiplier of a held bound: the Lagrangian gradient's component there
                if (state[i] == 0) continue;
                double v = g[i];
                for (int c = 0; c < n; c++) v += B[(size_t)i * n + c] * cand[c];
                for (int q = 0; q < na; q++) v -= A[(size_t)act[q] * n + i] * sol[nf + q];
                ok = state[i] == 1 ? v >= -tol : v <= tol;
            }
            if (ok) {
                s = cand;
                return true;
            }
        }
        int i = 0;
        while (i < n && ++state[i] == 3) state[i++] = 0;
        if (i == n) return false;
    }
}

static int run_qp(unsigned seed, int count) {
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    for (int t = 0; t < count; t++) {
        const int n = 1 + (int)(rng() % 8), m = (int)(rng() % 7);
        vec Mx((size_t)n * n), B((size_t)n * n, 0.0), g((size_t)n), A((size_t)m * n), b((size_t)m), lo((size_t)n), hi((size_t)n), xin((size_t)n);
        for (double &v : Mx) v = U(rng);
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
                double s = i == j ? 0.05 : 0.0;
                for (int k = 0; k < n; k++) s += Mx[(size_t)k * n + i] * Mx[(size_t)k * n + j];
                B[(size_t)i * n + j] = s;
            }
        for (int i = 0; i < n; i++) {
            g[i] = 3.0 * U(rng);
            lo[i] = -0.2 - 0.8 * std::fabs(U(rng)), hi[i] = 0.2 + 0.8 * std::fabs(U(rng));
            if (rng() % 11 == 0) hi[i] = lo[i];  // a coordinate the box fixes
            xin[i] = lo[i] + (hi[i] - lo[i]) * 0.5 * (1.0 + U(rng));
        }
        const bool broken = t % 10 == 9 && m >= 2;  // every tenth problem: two constraints that contradict each other
        for (int j = 0; j < m; j++) {
            double v = 0;
            for (int i = 0; i < n; i++) A[(size_t)j * n + i] = U(rng), v += A[(size_t)j * n + i] * xin[i];
            b[j] = -v + 0.3 * std::fabs(U(rng));  // A xin + b >= 0: consistent, often active at the optimum
        }
        if (broken) {
            for (int i = 0; i < n; i++) A[(size_t)n + i] = -A[i];
            b[1] = -b[0] - 0.5;
        }
        const vec ldl = factor(n, B);
        vec s((size_t)n, 0.0), mult((size_t)m + 2 * n, 0.0), se;
        const int mode = slsqp_detail::solve_qp(n, ldl.data(), g.data(), m, A.data(), b.data(), lo.data(), hi.data(), s.data(), mult.data());
        const bool found = enumerate(n, B, g, m, A, b, lo, hi, se);
        double scale = 1.0, kkt = 0.0, dx = 0.0;
        for (double v : B) scale = std::fmax(scale, std::fabs(v));
        for (double v : g) scale = std::fmax(scale, std::fabs(v));
        for (double v : A) scale = std::fmax(scale, std::fabs(v));
        for (double v : b) scale = std::fmax(scale, std::fabs(v));
        if (mode == 0 && found) {
            for (double v : mult) kkt = std::fmax(kkt, -v), scale = std::fmax(scale, std::fabs(v));
            for (int i = 0; i < n; i++) {
                double v = g[i];  // stationarity
                for (int c = 0; c < n; c++) v += B[(size_t)i * n + c] * s[c];
                for (int j = 0; j < m; j++) v -= A[(size_t)j * n + i] * mult[j];
                v -= mult[m + i] - mult[m + n + i];
                kkt = std::fmax(kkt, std::fabs(v));
                kkt = std::fmax(kkt, std::fmax(lo[i] - s[i], s[i] - hi[i]));                                   // feasibility
                kkt = std::fmax(kkt, std::fmax(std::fabs(mult[m + i] * (s[i] - lo[i])), std::fabs(mult[m + n + i] * (hi[i] - s[i]))));
                dx = std::fmax(dx, std::fabs(s[i] - se[i]));
            }
            for (int j = 0; j < m; j++) {
                double v = b[j];
                for (int i = 0; i < n; i++) v += A[(size_t)j * n + i] * s[i];
                kkt = std::fmax(kkt, std::fmax(-v, std::fabs(mult[j] * v)));  // feasibility, complementarity
            }
        }
        printf("Q %d %d kkt %.3e dx %.3e enum %d mode %d\n", n, m, kkt / scale, dx, found ? 1 : 0, mode);
    }
    return 0;
}

static int run_ldl(unsigned seed, int count) {
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    for (int t = 0; t < count; t++) {
        const int n = 1 + (int)(rng() % 8);
        vec Mx((size_t)n * n), B((size_t)n * n, 0.0), z((size_t)n), w((size_t)n);
        for (double &v : Mx) v = U(rng);
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
                double s = i == j ? 0.1 : 0.0;
                for (int k = 0; k < n; k++) s += Mx[(size_t)k * n + i] * Mx[(size_t)k * n + j];
                B[(size_t)i * n + j] = s;
            }
        vec p = factor(n, B);
        for (double &v : z) v = U(rng);
        // positive, then a negative update that keeps the matrix positive definite: sigma = -0.5 / (z^T B^-1 z)
        double sigma = 0.7;
        if (t % 2) {
            vec y;
            solve_dense(n, B, z, y);
            double q = 0;
            for (int i = 0; i < n; i++) q += z[i] * y[i];
            sigma = -0.5 / q;
        }
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) B[(size_t)i * n + j] += sigma * z[i] * z[j];
        vec zz = z;
        slsqp_detail::ldl_update(n, p.data(), zz.data(), sigma, w.data());
        const vec B2 = unpack(n, p);
        double err = 0, big = 1;
        for (size_t i = 0; i < B.size(); i++) err = std::fmax(err, std::fabs(B[i] - B2[i])), big = std::fmax(big, std::fabs(B[i]));
        printf("L %.3e\n", err / big);
    }
    return 0;
}

// ---- the machine's contracts ----

static int failures = 0;
static void check(bool ok, const char *name) {
    printf("%s %s\n", ok ? "ok" : "FAILED", name);
    if (!ok) failures++;
}

struct Run {
    std::vector<vec> pts;
    Slsqp::Status status;
    int64_t evals;
    bool any_finite;
    vec best_x;
    double best_f;
    int64_t augmented;
};

// runs a problem to the end; `spoil` may replace a value by index of evaluation
static Run run_problem(const Problem &p, long maxeval, const std::function<double(long, double)> &spoil = nullptr, double ftol = 1e-4) {
    const int n = (int)p.x0.size(), m = p.m;
    Slsqp opt(p.x0, p.lo, p.hi, m, ftol, ftol, maxeval);
    Run r;
    vec x, g((size_t)n), cv((size_t)m + 1), J((size_t)m * n + 1);
    bool want = false;
    long i = 0;
    while (opt.ask(x, want)) {
        r.pts.push_back(x);
        double v = p.f(x, g.data());
        if (m > 0) p.c(x, cv.data(), J.data());
        if (spoil) v = spoil(i, v);
        i++;
        opt.tell(v, cv.data(), g.data(), J.data());
    }
    r.status = opt.status(), r.evals = opt.evals(), r.any_finite = opt.any_finite_f(), r.best_x = opt.best_x(), r.best_f = opt.best_f();
    r.augmented = opt.augmented();
    return r;
}

static bool in_box(const Run &r, const Problem &p) {
    for (const vec &x : r.pts)
        for (size_t i = 0; i < x.size(); i++)
            if (!(x[i] >= p.lo[i] && x[i] <= p.hi[i])) return false;
    return true;
}

static int run_contracts() {
    // two machines interleaved ask bit for bit what each asks alone
    {
        bool same = true;
        for (int a = 0; a < 4; a++) {
            const int bcase = (a + 1) % 4;
            Problem pa = make_case(a), pb = make_case(bcase);
            const Run ra = run_problem(pa, 200), rb = run_problem(pb, 200);
            Slsqp oa(pa.x0, pa.lo, pa.hi, pa.m, 1e-4, 1e-4, 200), ob(pb.x0, pb.lo, pb.hi, pb.m, 1e-4, 1e-4, 200);
            std::vector<vec> qa, qb;
            vec x, g(8), cv(8), J(32);
            bool want = false;
            for (bool more = true; more;) {
                more = false;
                if (oa.ask(x, want)) {
                    qa.push_back(x), more = true;
                    const double v = pa.f(x, g.data());
                    pa.c(x, cv.data(), J.data());
                    oa.tell(v, cv.data(), g.data(), J.data());
                }
                if (ob.ask(x, want)) {
                    qb.push_back(x), more = true;
                    const double v = pb.f(x, g.data());
                    pb.c(x, cv.data(), J.data());
                    ob.tell(v, cv.data(), g.data(), J.data());
                }
            }
            same &= qa == ra.pts && qb == rb.pts && oa.evals() == ra.evals && ob.status() == rb.status;
        }
        check(same, "interleaved machines walk their own points");
    }
    // the box, lo = hi in one coordinate included, and a start outside it
    {
        bool ok = true;
        for (int cs = 0; cs < 4; cs++) {
            Problem p = make_case(cs);
            ok &= in_box(run_problem(p, 200), p);
            p.lo[1] = p.hi[1] = p.x0[1];
            const Run r = run_problem(p, 200);
            ok &= in_box(r, p) && r.status != Slsqp::RUNNING;
            p.x0[0] = p.hi[0] + 5.0;
            const Run r2 = run_problem(p, 200);
            ok &= in_box(r2, p) && r2.pts[0][0] == p.hi[0];
        }
        check(ok, "every asked point lies in the box");
    }
    // d = 1, k = 0
    {
        Problem p;
        p.m = 0, p.x0 = {2.5}, p.lo = {-1}, p.hi = {3};
        p.f = [](const vec &x, double *g) {
            g[0] = 4 * (x[0] - 0.5) * (x[0] - 0.5) * (x[0] - 0.5) + 0.2 * (x[0] - 0.5);
            return std::pow(x[0] - 0.5, 4) + 0.1 * (x[0] - 0.5) * (x[0] - 0.5);
        };
        const Run r = run_problem(p, 200, nullptr, 1e-12);
        check(r.status == Slsqp::FTOL && std::fabs(r.best_x[0] - 0.5) < 1e-4 && in_box(r, p), "d = 1 without constraints");
        p.f = [](const vec &x, double *g) { g[0] = -1; return -x[0]; };  // ends on the bound
        const Run r2 = run_problem(p, 200);
        check(r2.status == Slsqp::FTOL && r2.best_x[0] == 3.0, "d = 1 ends on its bound");
    }
    // tiny budgets
    {
        bool ok = true;
        for (int cs = 0; cs < 4; cs++)
            for (long b = 1; b <= 3; b++) {
                const Run r = run_problem(make_case(cs), b);
                ok &= r.evals == b && (long)r.pts.size() == b && r.status == Slsqp::MAXEVAL;
            }
        check(ok, "max_eval 1, 2, 3 stop at the budget");
    }
    // non-finite values
    {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        bool ok = true;
        for (double bad : {nan, 1e30, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::max()}) {
            Problem p = make_case(0);
            const Run clean = run_problem(p, 200);
            const Run r = run_problem(p, 200, [&](long i, double v) { return i == 1 ? bad : v; });
            // the second point asked is the full step; the third must be that step shortened to a tenth
            ok &= r.pts.size() >= 3 && r.pts[1] == clean.pts[1];
            for (int i = 0; i < 2 && ok; i++)
                ok &= std::fabs((r.pts[2][i] - r.pts[0][i]) - 0.1 * (r.pts[1][i] - r.pts[0][i])) < 1e-15;
            ok &= r.any_finite && r.status == Slsqp::FTOL && std::isfinite(r.best_f);
            const Run r0 = run_problem(p, 200, [&](long i, double v) { return i == 0 ? bad : v; });
            ok &= !r0.any_finite && r0.evals == 1 && r0.status == Slsqp::NO_FINITE;
            const Run rall = run_problem(p, 200, [&](long i, double v) { return i == 0 ? v : bad; });
            ok &= rall.status == Slsqp::LINESEARCH && rall.evals == 12 && rall.any_finite && rall.best_x == rall.pts[0];
        }
        check(ok, "non-finite values shorten the step or end the run");
    }
    // the best-point ordering on a scripted sequence of tells
    {
        Slsqp o({0.5, 0.5}, {0, 0}, {1, 1}, 1, 1e-4, 1e-4, 100, {0.25});
        const double g[2] = {1.0, -0.5}, J[2] = {0.3, 0.2};
        struct Step { double f, c; int best; };  // best: index of the step whose point must be the best afterwards
        const Step script[] = {{5.0, 0.9, 0}, {7.0, 0.5, 1}, {9.0, 0.5, 1}, {3.0, 0.25, 3}, {3.0, 0.1, 3}, {2.0, 0.3, 3}, {1e31, 0.0, 3}, {2.5, 0.25, 7}};
        std::vector<vec> asked;
        vec x;
        bool want = false, ok = true;
        for (const Step &st : script) {
            if (!o.ask(x, want)) break;
            asked.push_back(x);
            o.tell(st.f, &st.c, g, J);
            ok &= o.best_f() == script[st.best].f && o.best_c()[0] == script[st.best].c && o.best_x() == asked[(size_t)st.best];
            ok &= o.best_feasible() == (script[st.best].c <= 0.25) && o.best_violation() == script[st.best].c - 0.25;
        }
        check(ok && asked.size() >= 4, "best point: feasible first, then f or the violation, the first on ties");
    }
    // an inconsistent linearisation takes the slack-variable route: x0 >= 1 and x0 <= -1 cannot both hold
    {
        const double ldl[3] = {1, 0, 1}, g[2] = {0.3, -0.2}, A[4] = {1, 0, -1, 0}, b[2] = {-1, -1}, lo[2] = {-3, -3}, hi[2] = {3, 3};
        double s[2], mult[6];
        check(slsqp_detail::solve_qp(2, ldl, g, 2, A, b, lo, hi, s, mult) == 4, "the subproblem solver reports an inconsistent linearisation");
        Problem p;
        p.m = 2, p.x0 = {0.2, 0.1}, p.lo = {-3, -3}, p.hi = {3, 3};
        p.f = [](const vec &x, double *gg) { gg[0] = 2 * x[0], gg[1] = 2 * (x[1] - 1); return x[0] * x[0] + (x[1] - 1) * (x[1] - 1); };
        p.c = [](const vec &x, double *o, double *J) { o[0] = 1 - x[0], o[1] = 1 + x[0], J[0] = -1, J[1] = 0, J[2] = 1, J[3] = 0; };
        const Run r = run_problem(p, 60);
        check(r.augmented >= 1 && r.status != Slsqp::RUNNING && in_box(r, p), "the machine augments an inconsistent subproblem");
        // two strongly curved constraints, x0^2 <= 0.25 and 100 x0^3 >= 0.1, from a start far outside the first
        Problem q;
        q.m = 2, q.x0 = {2.0, 0.0}, q.lo = {-4, -4}, q.hi = {4, 4};
        q.f = [](const vec &x, double *gg) { gg[0] = 1, gg[1] = 2 * x[1]; return x[0] + x[1] * x[1]; };
        q.c = [](const vec &x, double *o, double *J) { o[0] = x[0] * x[0] - 0.25, o[1] = 0.1 - x[0] * x[0] * x[0] * 100, J[0] = 2 * x[0], J[1] = 0, J[2] = -300 * x[0] * x[0], J[3] = 0; };
        const Run rq = run_problem(q, 100, nullptr, 1e-8);
        check(rq.status == Slsqp::FTOL && std::fabs(rq.best_x[0] - std::cbrt(0.001)) < 1e-5 && in_box(rq, q), "curved constraints from a far start converge");
    }
    return failures ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "contracts")) return run_contracts();
    if (argc >= 4 && !strcmp(argv[1], "qp")) return run_qp((unsigned)atol(argv[2]), atoi(argv[3]));
    if (argc >= 4 && !strcmp(argv[1], "ldl")) return run_ldl((unsigned)atol(argv[2]), atoi(argv[3]));
    if (argc < 4) return 2;
    const int cs = atoi(argv[1]);
    if (cs < 0 || cs > 3) return 2;
    return run_case(cs, atof(argv[2]), atol(argv[3]));
}
