// CPU host of egobox_amd/csrc/infill_mix_math.h (tests/test_infill_mix_cpu.py): one recombination per input line
//   smooth k d  p[k]  dp[k*d]  mu[k]  v[k]  gmu[k*d]  gv[k*d]
// answered by one line  mean var gmean[d] gvar[d]  (17 significant digits: exact round trip).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "infill_mix_math.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        int smooth = 0, k = 0, d = 0;
        in >> smooth >> k >> d;
        if (!in || k < 1 || d < 1) return 2;
        std::vector<double> p(k), dp((size_t)k * d), mu(k), v(k), gmu((size_t)k * d), gv((size_t)k * d), gm(d), gvar(d);
        for (std::vector<double> *a : {&p, &dp, &mu, &v, &gmu, &gv})
            for (double &x : *a) {
                std::string tok;
                in >> tok;
                x = std::stod(tok);
            }
        if (!in) return 3;
        double mean = 0.0, var = 0.0;
        egx::infill::mix_value(smooth != 0, k, p.data(), 1, mu.data(), v.data(), 1, &mean, &var);
        egx::infill::mix_grad(smooth != 0, k, d, p.data(), 1, dp.data(), d, mu.data(), v.data(), 1, gmu.data(), gv.data(), d, gm.data(),
                              gvar.data());
        std::printf("%.17g %.17g", mean, var);
        for (int l = 0; l < d; l++) std::printf(" %.17g", gm[l]);
        for (int l = 0; l < d; l++) std::printf(" %.17g", gvar[l]);
        std::printf("\n");
    }
    return 0;
}
