// Host build of egobox_amd/csrc/mixint.h (no HIP): tests/test_mixint_cpu.py compiles this with g++ -fsanitize=address,undefined,
// runs it as a process of its own and compares what it prints with tests/mixint_oracle.py.
//   stdin, one request per line:   <A|B> <cast|fold|disc|unfold> v0 v1 ...     (the unfolded or folded row)
//   stdout, one line per request:  the result row as %.17g ("nan", "-0" as printf writes them), or "bad <column>" for an unfold
//                                  the header refuses
// Before it reads anything it checks the scalar rules on the edge values itself and exits 2 when one fails.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "mixint.h"

using namespace egx::mixint;

struct Spec {
    std::vector<Col> cols;
    std::vector<double> vals;
    int nx = 0;
    void scalar(int kind) {
        cols.push_back({kind, (int32_t)cols.size(), 1, 0});
        nx++;
    }
    void ord(std::initializer_list<double> v) {
        cols.push_back({kOrd, (int32_t)cols.size(), (int32_t)v.size(), (int32_t)vals.size()});
        vals.insert(vals.end(), v);
        nx++;
    }
    void en(int n) {
        const int32_t u = (int32_t)cols.size();
        for (int l = 0; l < n; l++) cols.push_back({kEnum, u, n, 0});
        nx++;
    }
};

static Spec spec_a() {  // [Float, Enum(3), Int, Ord{1,3,5,8}]: d = 6
    Spec s;
    s.scalar(kFloat), s.en(3), s.scalar(kInt), s.ord({1.0, 3.0, 5.0, 8.0});
    return s;
}
static Spec spec_b() {  // d = 70: Int at 0, Enum(5) on 62..66, Ord at 68, Int at 69
    Spec s;
    s.scalar(kInt);
    for (int i = 0; i < 61; i++) s.scalar(kFloat);
    s.en(5), s.scalar(kFloat), s.ord({-0.5, 0.0, 0.25, 1.0}), s.scalar(kInt);
    return s;
}

static int fails = 0;
static void expect(bool ok, const char *what) {
    if (!ok) fprintf(stderr, "FAILED: %s\n", what), fails++;
}
static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0 || (std::isnan(a) && std::isnan(b)); }

static void self_check() {
    expect(same(round_half_away(0.5), 1.0) && same(round_half_away(-0.5), -1.0), "round +-0.5");
    expect(same(round_half_away(1.5), 2.0) && same(round_half_away(-1.5), -2.0) && same(round_half_away(2.5), 3.0), "round 1.5 2.5");
    expect(same(round_half_away(-0.3), -0.0) && std::signbit(round_half_away(-0.3)), "round(-0.3) = -0.0");
    expect(same(round_half_away(0.49999999999999994), 0.0), "round below one half");
    expect(same(round_half_away(9007199254740992.0), 9007199254740992.0), "round 2^53");
    expect(std::isnan(round_half_away(NAN)) && same(round_half_away(INFINITY), INFINITY) && same(round_half_away(-INFINITY), -INFINITY),
           "round keeps non-finite values");
    const double v[4] = {1.0, 3.0, 5.0, 8.0};
    expect(same(nearest_value(v, 4, 2.0), 1.0) && same(nearest_value(v, 4, 4.0), 3.0) && same(nearest_value(v, 4, 6.5), 5.0), "ord ties");
    expect(same(nearest_value(v, 4, -40.0), 1.0) && same(nearest_value(v, 4, 1e9), 8.0), "ord outside the range");
    expect(std::isnan(nearest_value(v, 4, NAN)) && same(nearest_value(v, 4, INFINITY), INFINITY), "ord keeps non-finite values");
    const double two[3] = {0.7, 0.2, 0.7}, three[3] = {0.4, 0.4, 0.4}, bad[3] = {0.1, NAN, 0.3}, inf[3] = {0.1, INFINITY, 0.3};
    expect(first_max(two, 3, 1) == 0 && first_max(three, 3, 1) == 0, "enum ties go to the first");
    expect(first_max(bad, 3, 1) == -1 && first_max(inf, 3, 1) == -1, "enum group with a non-finite entry");
    const Spec a = spec_a();
    const double row[6] = {0.25, 0.1, NAN, 0.2, 2.5, 4.0};
    double out[6], folded[4];
    cast_row(a.cols.data(), a.vals.data(), 6, row, out);
    expect(same(out[0], 0.25) && std::isnan(out[1]) && std::isnan(out[2]) && std::isnan(out[3]) && same(out[4], 3.0) && same(out[5], 3.0),
           "cast of a row with a NaN enum group");
    fold_row(a.cols.data(), 6, out, folded);
    expect(std::isnan(folded[1]) && same(folded[2], 3.0) && same(folded[3], 3.0), "fold reads Int / Ord at the unfolded index");
    const double fx[4] = {1.5, 2.9, -7.0, 8.0};
    expect(unfold_row(a.cols.data(), 6, fx, out) == -1 && same(out[3], 1.0) && same(out[1], 0.0) && same(out[4], -7.0) && same(out[5], 8.0),
           "unfold reads Int / Ord at the folded index");
    const double f3[4] = {0.0, 3.0, 0.0, 1.0}, fn[4] = {0.0, NAN, 0.0, 1.0}, fm[4] = {0.0, -1.0, 0.0, 1.0};
    expect(unfold_row(a.cols.data(), 6, f3, out) == 1 && unfold_row(a.cols.data(), 6, fn, out) == 1 &&
               unfold_row(a.cols.data(), 6, fm, out) == 1, "unfold refuses an index outside [0, v)");
}

int main() {
    self_check();
    if (fails) return 2;
    const Spec sa = spec_a(), sb = spec_b();
    char buf[1 << 16];
    while (fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string which, op, tok;
        if (!(in >> which >> op)) continue;
        const Spec &s = which == "B" ? sb : sa;
        const int d = (int)s.cols.size();
        std::vector<double> x;
        while (in >> tok) x.push_back(strtod(tok.c_str(), nullptr));
        std::vector<double> out;
        if (op == "cast" && (int)x.size() == d) {
            out.resize(d);
            cast_row(s.cols.data(), s.vals.data(), d, x.data(), out.data());
        } else if (op == "fold" && (int)x.size() == d) {
            out.resize(s.nx);
            fold_row(s.cols.data(), d, x.data(), out.data());
        } else if (op == "disc" && (int)x.size() == d) {
            std::vector<double> c(d);
            cast_row(s.cols.data(), s.vals.data(), d, x.data(), c.data());
            out.resize(s.nx);
            fold_row(s.cols.data(), d, c.data(), out.data());
        } else if (op == "unfold" && (int)x.size() == s.nx) {
            out.resize(d);
            const int bad = unfold_row(s.cols.data(), d, x.data(), out.data());
            if (bad >= 0) {
                printf("bad %d\n", bad);
                continue;
            }
        } else {
            fprintf(stderr, "bad request: %s", buf);
            return 3;
        }
        for (size_t i = 0; i < out.size(); i++) printf("%s%.17g", i ? " " : "", out[i]);
        printf("\n");
    }
    return 0;
}
