"""egx::Slsqp (csrc/slsqp.h) against Kraft's own SLSQP.

The class behind egx_infill_optimize_slsqp is checked against the original Fortran SLSQP that scipy < 1.16 ships, on the four
problems of test_cobyla_cstr_cpu.py given with analytic gradients.  scipy evaluates the objective at the start point and at
every line-search trial point, and the gradient at every point that becomes the iterate; the class asks for both at once, so
its sequence of asked points is scipy's sequence of objective calls, and its iterates are scipy's gradient calls."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "slsqp_trace.cpp")

# objective, its gradient, constraints g(x) >= 0 in scipy's sense with their gradients (the class is told c = -g), x0, lo, hi:
# CASES 0-3 of test_cobyla_cstr_cpu.py
CASES = {
    0: (lambda x: (x[0] - 1.2) ** 2 + (x[1] - 0.9) ** 2, lambda x: np.array([2 * (x[0] - 1.2), 2 * (x[1] - 0.9)]),
        [(lambda x: 1.0 - x[0] ** 2 - x[1] ** 2, lambda x: np.array([-2 * x[0], -2 * x[1]]))], [0.1, 0.2], [-2, -2], [2, 2]),
    1: (lambda x: x[0] + x[1] + 0.1 * np.sin(3 * x[0]), lambda x: np.array([1 + 0.3 * np.cos(3 * x[0]), 1.0]),
        [(lambda x: x[0] * x[1] - 0.25, lambda x: np.array([x[1], x[0]])),
         (lambda x: 1.5 - x[0] - 0.5 * x[1] ** 2, lambda x: np.array([-1.0, -x[1]]))], [1.0, 1.0], [0, 0], [2, 2]),
    2: (lambda x: sum((i + 1) * (x[i] - 0.3 * i + 0.5) ** 2 for i in range(4)),
        lambda x: np.array([2 * (i + 1) * (x[i] - 0.3 * i + 0.5) for i in range(4)]),
        [(lambda x: 0.5 - sum(x[i] ** 2 for i in range(4)), lambda x: -2 * np.array(x)),
         (lambda x: x[0] + x[1] + x[2] + x[3] + 0.2, lambda x: np.ones(4)),
         (lambda x: np.cos(x[1]) - 0.8 - x[3], lambda x: np.array([0.0, -np.sin(x[1]), 0.0, -1.0]))], [0.1] * 4, [-2] * 4, [2] * 4),
    3: (lambda x: -x[0] * x[1] * x[2], lambda x: np.array([-x[1] * x[2], -x[0] * x[2], -x[0] * x[1]]),
        [(lambda x: 1 - x[0] ** 2 - 2 * x[1] ** 2 - 3 * x[2] ** 2, lambda x: np.array([-2 * x[0], -4 * x[1], -6 * x[2]]))],
        [0.3, 0.3, 0.3], [0, 0, 0], [0.45, 1, 1]),
}
# The longest prefix of asked points that equals scipy's to 1e-9 at ftol = 1e-10: the WHOLE run on every case (10, 9, 10 and
# 8 points on both sides; the largest difference is 6.5e-10, at the last point of case 3, 1e-13 before it).
PREFIX = {0: 10, 1: 9, 2: 10, 3: 8}


@pytest.fixture(scope="module")
def trace_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("slsqp") / "slsqp_trace"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", SRC, "-o", str(exe)], check=True)
    return str(exe)


def _mine(exe, cs, ftol, maxeval=500):
    n, m = len(CASES[cs][3]), len(CASES[cs][2])
    out = subprocess.run([exe, str(cs), repr(ftol), str(maxeval)], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    rows = np.array([[float(v) for v in ln.split()[1:]] for ln in out if ln.startswith("P")]).reshape(-1, n + 1 + m)
    its = np.array([[float(v) for v in ln.split()[1:]] for ln in out if ln.startswith("I")]).reshape(-1, n)
    t = out[-2].split()
    final = {"status": int(t[3]), "evals": int(t[5]), "iters": int(t[7]), "augmented": int(t[9]), "f": float(t[11]),
             "x": np.array([float(v) for v in t[13:13 + n]])}
    t = out[-1].split()
    best = {"feasible": int(t[3]), "violation": float(t[5]), "f": float(t[7]), "x": np.array([float(v) for v in t[9:9 + n]]),
            "c": np.array([float(v) for v in t[10 + n:10 + n + m]])}
    return rows[:, :n], rows[:, n], rows[:, n + 1:], its, final, best


def _scipy_slsqp(cs, ftol):
    import scipy
    from scipy.optimize import minimize
    if tuple(int(v) for v in scipy.__version__.split(".")[:2]) >= (1, 16):
        pytest.skip("scipy >= 1.16 replaced Kraft's Fortran SLSQP")
    f, g, cons, x0, lo, hi = CASES[cs]
    pts, its = [], []

    def fw(x):
        pts.append(np.array(x))
        return f(x)

    def gw(x):
        its.append(np.array(x))
        return g(x)
    r = minimize(fw, x0, jac=gw, method="SLSQP", bounds=list(zip(lo, hi)),
                 constraints=[{"type": "ineq", "fun": c, "jac": j} for c, j in cons], options={"ftol": ftol, "maxiter": 200})
    assert r.status == 0
    return np.array(pts), np.array(its), r


def _violation(cs, x):
    return max(0.0, max(-c(x) for c, _ in CASES[cs][2]))


def _rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


@pytest.mark.parametrize("cs", [0, 1, 2, 3])
def test_krafts_sequence_and_optimum(trace_exe, cs):
    sp, sit, r = _scipy_slsqp(cs, 1e-10)
    x, f, c, its, final, _ = _mine(trace_exe, cs, 1e-10)
    lo, hi = np.array(CASES[cs][4]), np.array(CASES[cs][5])
    assert np.all(sp >= lo - 1e-15) and np.all(sp <= hi + 1e-15)
    # iteration 1: the first QP step from B = I and its line search, up to the first accepted point
    n1 = next(i for i in range(1, len(x)) if np.array_equal(x[i], its[1])) + 1
    assert len(sit) >= 2 and np.array_equal(sp[n1 - 1], sit[1])           # scipy accepted the same trial point
    for i in range(n1):
        assert _rel(x[i], sp[i]) <= 1e-12, (i, x[i], sp[i])
    # beyond: the prefix pinned above, here scipy's whole run
    k = PREFIX[cs]
    assert len(sp) == len(x) == k
    for i in range(k):
        assert _rel(x[i], sp[i]) <= 1e-9, (i, x[i], sp[i])
    ni = len(sit)                                                           # scipy asks no gradient at its last iterate
    np.testing.assert_allclose(its[:ni], sit, rtol=0, atol=1e-9)
    assert final["status"] == 2
    np.testing.assert_allclose(final["x"], r.x, rtol=0, atol=1e-6)
    assert _violation(cs, final["x"]) <= 1e-9
    assert final["evals"] == len(x) and final["augmented"] == 0


@pytest.mark.parametrize("cs", [0, 1, 2, 3])
def test_at_the_infill_optimisers_tolerance(trace_exe, cs):
    """ftol = 1e-4, the stop tolerance both sides use: no worse than Kraft's code, inside his own bound on the violation."""
    sp, _, r = _scipy_slsqp(cs, 1e-4)
    x, f, c, its, final, best = _mine(trace_exe, cs, 1e-4)
    lo, hi = np.array(CASES[cs][4]), np.array(CASES[cs][5])
    assert np.all(x >= lo) and np.all(x <= hi)                              # every asked point in the box, exactly
    assert final["status"] == 2
    assert final["f"] <= r.fun + 1e-4 * max(1.0, abs(r.fun))
    assert _violation(cs, final["x"]) <= 1e-4
    assert len(x) == len(sp)                                                # ... and after as many evaluations
    # best: the best evaluated point in the documented ordering
    keys = [((0, f[i]) if not np.max(c[i]) > 0.0 else (1, np.max(c[i])), i) for i in range(len(x))]
    i_best = min(keys)[1]
    assert best["feasible"] == 1 and best["f"] == f[i_best]
    assert np.array_equal(best["x"], x[i_best]) and np.array_equal(best["c"], c[i_best])
    assert best["violation"] == np.max(c[i_best])


def test_subproblem_solver_is_exact(trace_exe):
    """200 random strictly convex subproblems (d <= 8, <= 6 inequalities plus bounds, some coordinates fixed by the box, every
    tenth with two contradicting constraints) against a dense enumeration of active sets."""
    out = subprocess.run([trace_exe, "qp", "20240607", "200"], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == 200
    n_incons = 0
    dims = set()
    for ln in out:
        t = ln.split()
        n, m, kkt, dx, found, mode = int(t[1]), int(t[2]), float(t[4]), float(t[6]), int(t[8]), int(t[10])
        dims.add(n)
        if not found:
            assert mode == 4, ln                                            # the slack-variable route is taken from here
            n_incons += 1
            continue
        assert mode == 0 and kkt <= 1e-10 and dx <= 1e-9, ln
    assert n_incons >= 5 and dims == set(range(1, 9))
    out = subprocess.run([trace_exe, "ldl", "5", "60"], capture_output=True, text=True, check=True).stdout.split("\n")
    errs = [float(ln.split()[1]) for ln in out if ln.startswith("L")]
    assert len(errs) == 60 and max(errs) <= 1e-13                          # the factor's rank-one updates, both signs


def test_machine_contracts(trace_exe):
    """Interleaved machines, the box (lo = hi included), d = 1 and k = 0, tiny budgets, non-finite values, the best-point
    ordering on scripted tells, an inconsistent linearisation: checked inside the harness, one line each."""
    out = subprocess.run([trace_exe, "contracts"], capture_output=True, text=True)
    lines = out.stdout.strip().split("\n")
    assert out.returncode == 0 and len(lines) == 10 and all(ln.startswith("ok ") for ln in lines), out.stdout


def test_under_address_and_ub_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined, run stand-alone: all four cases, tiny budgets included, the
    subproblem checks and the contracts."""
    exe = tmp_path / "slsqp_trace_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", SRC, "-o", str(exe)], check=True)
    runs = [[str(cs), ftol, str(b)] for cs in range(4) for ftol in ("1e-4", "1e-10") for b in (1, 2, 3, 300)]
    runs += [["qp", "3", "40"], ["ldl", "3", "20"], ["contracts"]]
    for args in runs:
        out = subprocess.run([str(exe)] + args, capture_output=True, text=True)
        assert out.returncode == 0 and "runtime error" not in out.stderr, (args, out.stderr[-400:])


def test_header_declares_and_library_exports_the_entry_point():
    """egx_infill_optimize_slsqp in the header, the shared object and the ctypes table (equal in number and names), the layout
    ctypes assumes for egx_infill_slsqp_stats, the mirrors, and a NULL handle refused before any device is touched."""
    import ctypes as C
    import re
    import egobox_amd as egx
    L = egx._lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egx_gp.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(egx_[a-z0-9_]+)\s*\(", txt))
    bound = {s[0] for s in L.SIGNATURES}
    lib = C.CDLL(L.LIB_PATH)
    assert "egx_infill_optimize_slsqp" in declared and "egx_infill_optimize_slsqp" in bound
    assert hasattr(lib, "egx_infill_optimize_slsqp")
    assert declared == bound and len(L.SIGNATURES) == len(bound)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()[-1].startswith("egx_")}
    assert exported == declared, exported ^ declared
    st = L.InfillSlsqpStats
    assert (st.rounds.offset, st.best_start.offset, st.feasible.offset, st.violation.offset, st.evals.offset, st.stop.offset) == \
        (0, 8, 16, 24, 32, 40)
    assert re.search(r"int64_t rounds, best_start;\s*int32_t feasible;\s*double violation;\s*int64_t \*evals;[^}]*int32_t \*stop;", txt)
    assert callable(egx.InfillObjective.optimize_slsqp)
    hpp = open(os.path.join(ROOT, "include", "egx_gp.hpp")).read()
    assert "optimize_slsqp(" in hpp and "struct SlsqpOptimum : ConstrainedOptimum" in hpp
    assert L.load().egx_infill_optimize_slsqp(None, None, None, None, 1, 0, None, None, None, None) == L.ERR_INVALID_VALUE
