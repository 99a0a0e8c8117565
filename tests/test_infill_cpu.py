"""CPU checks of the infill criteria: egobox_amd/csrc/infill_math.h compiled with g++ (tests/c_host/infill_math_test.cpp, no GPU)
against 60-digit truths (tests/golden/infill_kat.json), against the numpy restatement of the reference (tests/infill_oracle.py)
and, for the three deviations, against derivatives of the value formulas; and the C ABI of the feature."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import infill_oracle as IO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egobox_amd", "csrc")
EPS = IO.EPS


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("infill") / "infill_math_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "c_host", "infill_math_test.cpp"), "-o", str(out)], check=True)
    return str(out)


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(ROOT, "tests", "golden", "infill_kat.json")) as f:
        return json.load(f)


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    rows = [[float(v) for v in ln.split()] for ln in out.strip().splitlines()]
    assert len(rows) == len(lines)
    return rows


def _objective_line(kind, fmin, sw, scale_ic, scale, feas, tols, parts):
    mu, var, dmu, dvar = parts
    k, d = len(tols), np.asarray(dmu).shape[1]
    tok = ["O", kind, repr(float(fmin)), repr(float(sw)), repr(float(scale_ic)), repr(float(scale)), int(feas), k, d]
    tok += [repr(float(t)) for t in tols]
    for j in range(1 + k):
        tok += [repr(float(mu[j])), repr(float(var[j]))] + [repr(float(v)) for v in dmu[j]] + [repr(float(v)) for v in dvar[j]]
    return " ".join(str(t) for t in tok)


def _rel(got, want):
    return abs(got - want) / max(1.0, abs(want))


def _rel_inf(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float(np.max(np.abs(got - want)) / max(1.0, float(np.max(np.abs(want)))))


# ---- 1. helper accuracy on the whole line ------------------------------------------------------------------------------
def test_log_ei_helper_is_accurate_on_the_whole_line(exe, kat):
    h = kat["helper"]
    assert {-1.0, -37.0, -37.6, -38.0, -40.0, -1e3, -1e6 - 1, -1e6 + 1, -1e8} <= set(h["u"])
    assert min(h["u"]) == -1e8 and max(h["u"]) == 10.0
    rows = _run(exe, [f"H {u!r}" for u in h["u"]])
    worst_v = worst_d = 0.0
    for u, (v, dv), tv, td in zip(h["u"], rows, h["value"], h["derivative"]):
        worst_v, worst_d = max(worst_v, _rel(v, tv)), max(worst_d, _rel(dv, td))
        assert _rel(v, tv) <= 1e-12, (u, v, tv)
        assert _rel(dv, td) <= 1e-9, (u, dv, td)
    print(f"log_ei_helper: worst value error {worst_v:.3g}, worst derivative error {worst_d:.3g} (bounds 1e-12, 1e-9)")
    # the bounds are ~10x what the reference-shaped double formulas reach where they work at all (recorded by the generator)
    assert kat["ref_error"]["value"] < 1e-12 and kat["ref_error"]["derivative"] < 1e-9


def test_reference_helper_pinned_values(exe, kat):
    p = kat["pinned"]
    rows = _run(exe, [f"H {u!r}" for u in p["u"]])
    for u, (v, _), want in zip(p["u"], rows, p["log_ei_helper"]):
        assert abs(v - want) <= 1e-6, (u, v, want)
        assert abs(IO.ref_log_ei_helper(u) - want) <= 1e-6


def test_reference_helper_fails_beyond_its_range(exe, kat):
    """Deviation 1 stays visible: the reference's exp(z^2) erfc(z) overflows at u = -40 (a domain error, or an error above 1)."""
    truth = kat["helper"]["value"][kat["helper"]["u"].index(-40.0)]
    try:
        got = IO.ref_log_ei_helper(-40.0)
        failed = not math.isfinite(got) or abs(got - truth) > 1.0
    except (OverflowError, ValueError):
        failed = True
    assert failed
    ((v, _),) = _run(exe, ["H -40.0"])
    assert _rel(v, truth) <= 1e-12


# ---- 2. every row of the table against the numpy restatement -----------------------------------------------------------
def _random_parts(rng, d, k, fmin, tol, special):
    nm = 1 + k
    var = np.exp(rng.uniform(np.log(1e-4), np.log(10.0), nm))
    if special is not None:
        var[rng.integers(nm)] = special
    mu = np.empty(nm)
    u0 = rng.uniform(-30.0, 8.0)
    mu[0] = fmin - u0 * math.sqrt(var[0])
    for j in range(1, nm):
        mu[j] = tol - rng.uniform(-6.0, 6.0) * math.sqrt(var[j])
    return mu, var, rng.standard_normal((nm, d)), rng.standard_normal((nm, d)) * var[:, None]


def test_objective_matches_the_restatement(exe):
    rng = np.random.default_rng(20240917)
    specials = [None, None, None, None, 0.0, EPS / 2, 2 * EPS, None]
    cases, lines = [], []
    for d in (1, 4, 32):
        for k in (0, 1, 3):
            for sw in (1.0, 0.75):
                for tol in (0.0, 0.3):
                    for feas in (True, False):
                        for kind in (IO.EI, IO.LOG_EI, IO.WB2, IO.WB2S):
                            for rep in range(8):
                                fmin, scale_ic, scale = rng.uniform(-1, 1), rng.uniform(0.5, 3.0), rng.uniform(1.0, 3.0)
                                parts = _random_parts(rng, d, k, fmin, tol, specials[rep])
                                cases.append((kind, fmin, sw, scale_ic, scale, feas, [tol] * k, parts))
                                lines.append(_objective_line(*cases[-1]))
    assert len(cases) >= 2000
    rows = _run(exe, lines)
    n_ref = 0
    for (kind, fmin, sw, scale_ic, scale, feas, tols, parts), row in zip(cases, rows):
        mu, var = parts[0], parts[1]
        line_by_line = sw == 1.0 and (not tols or tols[0] == 0.0)
        # (without constraint models the reference's gradient ignores `feasibility` while its value is the constant -1 / 0:
        #  that combination is compared with the derivative-consistent named function)
        grad_ref = line_by_line and not (len(tols) == 0 and not feas)
        want_v = IO.objective(kind, mu, var, tols, fmin, sw, scale_ic, scale, feas, dev=not line_by_line)
        want_g = (IO.ref_objective_grad if grad_ref else IO.dev_objective_grad)(kind, parts, tols, fmin, sw, scale_ic, scale, feas)
        n_ref += grad_ref
        assert _rel(row[0], want_v) <= 1e-11, (kind, sw, tols, feas, row[0], want_v)
        assert _rel_inf(row[1:], want_g) <= 1e-8, (kind, sw, tols, feas, row[1:], want_g)
    assert n_ref >= 300


# ---- 3. the deviations are derivatives -----------------------------------------------------------------------------------
def test_gradients_are_derivatives_of_the_values(exe, kat):
    toy = kat["toy"]
    combos = {(c["kind"], c["k"]) for c in toy["cases"] if c["feasibility"]}
    assert combos == {(kind, k) for kind in range(4) for k in (0, 2)}
    lines = []
    for c in toy["cases"]:
        assert c["sigma_weight"] == 0.75 and c["tol"] == 0.3
        parts = (np.array(c["mu"]), np.array(c["var"]), np.array(c["dmu"]), np.array(c["dvar"]))
        lines.append(_objective_line(c["kind"], c["fmin"], c["sigma_weight"], c["scale_ic"], c["scale"], c["feasibility"],
                                     [c["tol"]] * c["k"], parts))
    rows = _run(exe, lines)
    missed = 0
    for c, row in zip(toy["cases"], rows):
        assert _rel(row[0], c["value"]) <= 1e-11, (c["kind"], c["k"], row[0], c["value"])
        assert _rel_inf(row[1:], c["grad"]) <= 1e-8, (c["kind"], c["k"], row[1:], c["grad"])
        parts = (np.array(c["mu"]), np.array(c["var"]), np.array(c["dmu"]), np.array(c["dvar"]))
        ref = IO.ref_objective_grad(c["kind"], parts, [c["tol"]] * c["k"], c["fmin"], c["sigma_weight"], c["scale_ic"], c["scale"],
                                    c["feasibility"])
        if c["ref_must_miss"]:  # the reference's pof_grad at tol = 0.3 / its k-less gradient are NOT this derivative
            assert _rel_inf(ref, c["grad"]) > 1e-8
            assert _rel_inf(ref, c["grad"]) >= 1e-3
            missed += 1
    assert missed >= 24


def test_pof_grad_deviation_vanishes_at_zero_tolerance():
    rng = np.random.default_rng(3)
    for _ in range(50):
        mu, var, dmu, dvar = rng.standard_normal(), rng.uniform(0.1, 2.0), rng.standard_normal(4), rng.standard_normal(4)
        np.testing.assert_allclose(IO.dev_pof_grad(mu, var, dmu, dvar, 0.0), IO.ref_pof_grad(mu, var, dmu, dvar, 0.0), rtol=1e-14,
                                   atol=1e-16)


# ---- 4. the ABI ----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["egx_infill_config_default", "egx_infill_create", "egx_infill_destroy", "egx_infill_set_params",
               "egx_infill_get_params", "egx_infill_eval", "egx_infill_scaling", "egx_infill_optimize"]


def test_header_declares_and_library_exports_the_infill_symbols():
    import egobox_amd as egx
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egx_gp.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(egx_[a-z0-9_]+)\s*\(", txt))
    lib = C.CDLL(egx._lib.LIB_PATH)
    bound = {s[0] for s in egx._lib.SIGNATURES}
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in bound, name
    for name in ("EGX_INFILL_EI", "EGX_INFILL_LOG_EI", "EGX_INFILL_WB2", "EGX_INFILL_WB2S", "EGX_ERR_NO_FINITE_START"):
        assert name in txt
    assert (egx.EI, egx.LOG_EI, egx.WB2, egx.WB2S) == (0, 1, 2, 3)
    cfg = egx._lib.InfillConfig()
    egx._lib.load().egx_infill_config_default(C.byref(cfg))
    assert (cfg.criterion, cfg.feasibility, cfg.sigma_weight, cfg.scale_ic, cfg.scale) == (egx.LOG_EI, 1, 1.0, 1.0, 1.0)


def test_infill_driver_and_cpp_wrapper_compile(tmp_path):
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{inc}",
                    os.path.join(ROOT, "tests", "c_host", "infill_driver.c")], check=True)
    cpp = tmp_path / "t.cpp"
    cpp.write_text('#include "egx_gp.hpp"\nint use(egobox::GaussianProcess &gp) { egobox::InfillObjective o(gp, {}, {}, EGX_INFILL_EI, 0.0); '
                   'double x[1] = {0.0}; return (int)o.value(x, 1).size(); }\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{inc}", str(cpp)], check=True)


def test_cobyla_ftol_abs_defaults_to_the_old_behaviour(tmp_path):
    """CobylaBox's new trailing ftol_abs = 0 leaves a run bit for bit as it was; a positive value can only stop it earlier."""
    src = tmp_path / "c.cpp"
    src.write_text(r'''
#include <cstdio>
#include "cobyla.h"
static double f(const std::vector<double> &x) { return (x[0] - 0.3) * (x[0] - 0.3) + 2.0 * (x[1] + 0.2) * (x[1] + 0.2) + 1.0; }
static void run(double ftol_abs, bool dflt) {
    std::vector<double> x0 = {0.9, 0.9}, lo = {-1, -1}, hi = {1, 1}, x;
    egx::CobylaBox m = dflt ? egx::CobylaBox(x0, lo, hi, 0.5, 1e-4, 200) : egx::CobylaBox(x0, lo, hi, 0.5, 1e-4, 200, 0.0, true, true, ftol_abs);
    while (m.ask(x)) m.tell(f(x));
    std::printf("%lld %a %a %a\n", (long long)m.evals(), m.best_f(), m.best_x()[0], m.best_x()[1]);
}
int main() { run(0.0, true); run(0.0, false); run(1e-2, false); return 0; }
''')
    out = tmp_path / "c"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(src), "-o", str(out)], check=True)
    a, b, c = subprocess.run([str(out)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert a == b
    assert int(c.split()[0]) <= int(a.split()[0])
