// Stand-alone host program for csrc/kpls_coef.h (tests/test_sgp_kpls_cpu.py builds it with g++, plain and under
// -fsanitize=address,undefined, and compares what it prints to numpy):
//   kpls_coef_test d h  w[d*h]  theta[h]  gsum_d[d]  gsum_h[h]  div
// For each of the four correlations it prints one line
//   corr <c> hcols <hcols> coef <d * hcols values> grad <h values> nograd <d values>
// coef: the table with the weights; grad: the chain rule on gsum_d (collapsed, hcols == 1) or gsum_h (hcols > 1), each divided by
// div; nograd: table and chain rule without weights (w = I, theta = gsum_d reused as a d-long theta) -- the table is theta itself.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kpls_coef.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int d = std::atoi(argv[1]), h = std::atoi(argv[2]);
    if (d < 1 || h < 1 || argc != 3 + d * h + h + d + h + 1) return 2;
    int a = 3;
    auto take = [&](int n) {
        std::vector<double> v(n);
        for (int i = 0; i < n; i++) v[i] = std::strtod(argv[a++], nullptr);
        return v;
    };
    const std::vector<double> w = take(d * h), th = take(h), gd = take(d), gh = take(h);
    const double div = std::strtod(argv[a++], nullptr);
    for (int corr = 0; corr < 4; corr++) {
        std::vector<double> coef, grad(h, 0.0), coef1, grad1(d, 0.0);
        const int hcols = egx::kpls::coef_table(corr, d, h, w.data(), th.data(), coef);
        if ((int)coef.size() != d * hcols) return 3;
        egx::kpls::chain_rule(corr, d, h, w.data(), hcols, coef.data(), th.data(), hcols > 1 ? gh.data() : gd.data(), div, grad.data());
        const int hc1 = egx::kpls::coef_table(corr, d, d, nullptr, gd.data(), coef1);
        if (hc1 != 1 || (int)coef1.size() != d) return 3;
        egx::kpls::chain_rule(corr, d, d, nullptr, 1, coef1.data(), gd.data(), coef1.data(), div, grad1.data());
        std::printf("corr %d hcols %d coef", corr, hcols);
        for (double v : coef) std::printf(" %.17g", v);
        std::printf(" grad");
        for (double v : grad) std::printf(" %.17g", v);
        std::printf(" nograd");
        for (double v : grad1) std::printf(" %.17g", v);
        std::printf("\n");
    }
    return 0;
}
