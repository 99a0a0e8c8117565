// Host driver of egobox_amd/csrc/infill_math.h for tests/test_infill_cpu.py: lines in, numbers out (%.17g).
//   H u                                     -> log_ei_helper(u) d_log_ei_helper(u)
//   O kind fmin sigma_weight scale_ic scale feasibility k d  tol[k]  then per model j = 0..k: mu var dmu[d] dvar[d]
//                                           -> objective, then the d components of its gradient
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "infill_math.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "H") {
            double u;
            in >> u;
            std::printf("%.17g %.17g\n", egx::infill::log_ei_helper(u), egx::infill::d_log_ei_helper(u));
        } else if (cmd == "O") {
            egx::infill::Params p;
            int k, d;
            in >> p.kind >> p.fmin >> p.sigma_weight >> p.scale_ic >> p.scale >> p.feasibility >> k >> d;
            std::vector<double> tol(k > 0 ? k : 1), mu(1 + k), var(1 + k), dmu((size_t)(1 + k) * d), dvar((size_t)(1 + k) * d), g(d);
            for (int j = 0; j < k; j++) in >> tol[j];
            for (int j = 0; j <= k; j++) {
                in >> mu[j] >> var[j];
                for (int c = 0; c < d; c++) in >> dmu[(size_t)j * d + c];
                for (int c = 0; c < d; c++) in >> dvar[(size_t)j * d + c];
            }
            if (!in) {
                std::printf("ERR short line\n");
                return 2;
            }
            std::printf("%.17g", egx::infill::objective(p, k, mu.data(), var.data(), 1, tol.data()));
            egx::infill::objective_grad(p, k, d, mu.data(), var.data(), 1, dmu.data(), dvar.data(), d, tol.data(), g.data(), 1);
            for (int c = 0; c < d; c++) std::printf(" %.17g", g[c]);
            std::printf("\n");
        } else {
            std::printf("ERR unknown command\n");
            return 2;
        }
    }
    return 0;
}
