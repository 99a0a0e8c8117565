"""egx::Cobyla (csrc/cobyla.h: general nonlinear constraints, Powell's full TRSTLP) against Powell's own COBYLA.

The class behind egx_infill_optimize_cstr is checked against the original Fortran COBYLA that scipy < 1.16 ships.  scipy is
given the class's problem in the class's order: the m nonlinear constraints, then the bounds as 2n linear constraints
(lo_0, hi_0, lo_1, ...) IN THE RESCALED UNITS THE CLASS STATES THEM IN, (x_i - lo_i) / rhobeg -- the NLopt wrapper rescales
the variables by the initial step, so a bound's residual is measured in steps; Powell's code sees the same numbers either way
only if it is handed that statement (with unscaled bounds it solves case D, whose bound is active, in 71 evaluations along
another path; with the class's statement in 75).  With the NLopt additions switched off the SEQUENCE OF EVALUATED POINTS is
Powell's over the whole run on all four cases; with them on, the box, budget and best-point contracts are checked."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "cobyla_cstr_trace.cpp")
RHOBEG = 0.5

# objective, constraints g(x) >= 0 in scipy's sense (the class is told c = -g), x0, lo, hi
CASES = {
    0: (lambda x: (x[0] - 1.2) ** 2 + (x[1] - 0.9) ** 2, [lambda x: 1.0 - x[0] ** 2 - x[1] ** 2], [0.1, 0.2], [-2, -2], [2, 2]),
    1: (lambda x: x[0] + x[1] + 0.1 * np.sin(3 * x[0]),
        [lambda x: x[0] * x[1] - 0.25, lambda x: 1.5 - x[0] - 0.5 * x[1] ** 2], [1.0, 1.0], [0, 0], [2, 2]),
    2: (lambda x: sum((i + 1) * (x[i] - 0.3 * i + 0.5) ** 2 for i in range(4)),
        [lambda x: 0.5 - sum(x[i] ** 2 for i in range(4)), lambda x: x[0] + x[1] + x[2] + x[3] + 0.2,
         lambda x: np.cos(x[1]) - 0.8 - x[3]], [0.1] * 4, [-2] * 4, [2] * 4),
    3: (lambda x: -x[0] * x[1] * x[2], [lambda x: 1 - x[0] ** 2 - 2 * x[1] ** 2 - 3 * x[2] ** 2], [0.3, 0.3, 0.3], [0, 0, 0],
        [0.45, 1, 1]),
}
# The longest prefix of evaluated points that equals scipy's to 1e-9: the WHOLE run on every case (49, 57, 100 and 75
# evaluations), so the prefix pinned is the run's length; the existing bound-active test's shortest prefix is 20.
PREFIX = {0: 49, 1: 57, 2: 100, 3: 75}


@pytest.fixture(scope="module")
def trace_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cobyla_cstr") / "cobyla_cstr_trace"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", SRC, "-o", str(exe)], check=True)
    return str(exe)


def _summary(line, n, m):
    t = line.split()
    ix = t.index("x")
    return t, np.array([float(v) for v in t[ix + 1:ix + 1 + n]]), np.array([float(v) for v in t[ix + 2 + n:ix + 2 + n + m]])


def _mine(exe, cs, rhoend, maxeval, mode):
    n, m = len(CASES[cs][2]), len(CASES[cs][1])
    out = subprocess.run([exe, str(cs), repr(RHOBEG), repr(rhoend), str(maxeval), str(mode)], capture_output=True, text=True,
                         check=True).stdout.strip().split("\n")
    rows = np.array([[float(v) for v in ln.split()] for ln in out if not ln.startswith("#")]).reshape(-1, n + 1 + m)
    t, xf, cf = _summary(out[-2], n, m)
    final = {"status": int(t[3]), "evals": int(t[5]), "f": float(t[7]), "x": xf, "c": cf}
    t, xb, cb = _summary(out[-1], n, m)
    best = {"feasible": int(t[3]), "violation": float(t[5]), "f": float(t[7]), "x": xb, "c": cb}
    return rows[:, :n], rows[:, n], rows[:, n + 1:], final, best


def _scipy_cobyla(cs, rhoend, maxeval):
    import scipy
    from scipy.optimize import minimize
    if tuple(int(v) for v in scipy.__version__.split(".")[:2]) >= (1, 16):
        pytest.skip("scipy >= 1.16 replaced Powell's Fortran COBYLA with PRIMA")
    f, gs, x0, lo, hi = CASES[cs]
    pts = []

    def fw(x):
        pts.append(np.array(x))
        return f(x)
    cons = [{"type": "ineq", "fun": g} for g in gs]           # the class's order: nonlinear first ...
    for i in range(len(x0)):                                   # ... then (lo_0, hi_0, lo_1, ...), in steps of rhobeg
        cons.append({"type": "ineq", "fun": (lambda x, i=i: (x[i] - lo[i]) / RHOBEG)})
        cons.append({"type": "ineq", "fun": (lambda x, i=i: (hi[i] - x[i]) / RHOBEG)})
    r = minimize(fw, x0, method="COBYLA", constraints=cons, options={"rhobeg": RHOBEG, "tol": rhoend, "maxiter": maxeval})
    return np.array(pts), r


@pytest.mark.parametrize("cs", [0, 1, 2, 3])
def test_powells_sequence_and_optimum(trace_exe, cs):
    sp, r = _scipy_cobyla(cs, 1e-6, 2000)
    x, f, c, final, _ = _mine(trace_exe, cs, 1e-6, 2000, 0)
    k = PREFIX[cs]
    assert k >= 20 and len(x) >= k and len(sp) >= k
    if cs == 0:
        assert len(x) == len(sp) == final["evals"] == k       # the whole run
    np.testing.assert_allclose(x[:k], sp[:k], rtol=0, atol=1e-9)
    assert final["status"] == 3                                # rho reached rhoend
    assert final["f"] == pytest.approx(r.fun, abs=1e-9)
    np.testing.assert_allclose(final["x"], r.x, atol=2e-5)
    assert final["c"].max() <= 1e-9                            # greatest violation at the returned point
    gs = CASES[cs][1]
    np.testing.assert_allclose(final["c"], [-g(final["x"]) for g in gs], atol=1e-12)
    assert max(-g(r.x) for g in gs) <= 5e-12                   # ... and at scipy's
    assert abs(final["evals"] - len(sp)) <= 0.25 * len(sp)


def _order_key(f, c, cfeas=0.0):
    viol = np.max(c - cfeas) if len(c) else 0.0
    return (0, f) if not viol > 0.0 else (1, viol)


@pytest.mark.parametrize("cs", [0, 1, 2, 3])
def test_configured_as_the_infill_optimiser(trace_exe, cs):
    """Clamped evaluation, rho doubling, ftol_rel = ftol_abs = 1e-4: the box, the budget and the best-point contracts."""
    f, gs, x0, lo, hi = CASES[cs]
    x, fv, c, final, best = _mine(trace_exe, cs, 0.0, 400, 1)
    assert np.all(x >= np.array(lo)) and np.all(x <= np.array(hi))     # every trial point in the box, exactly
    np.testing.assert_allclose(x[0], x0)
    assert final["status"] in (1, 2)
    assert final["evals"] == len(x) <= 400
    # the returned point is the best evaluated one: feasible first, then f, or the violation; the first on ties
    keys = [_order_key(fv[i], c[i]) for i in range(len(x))]
    i_best = min(range(len(x)), key=lambda i: (keys[i], i))
    assert best["feasible"] == (keys[i_best][0] == 0) == 1
    assert best["f"] == fv[i_best] and np.array_equal(best["x"], x[i_best]) and np.array_equal(best["c"], c[i_best])
    assert best["violation"] == np.max(c[i_best])
    _, _, _, exact, _ = _mine(trace_exe, cs, 1e-8, 5000, 0)
    assert best["f"] - exact["f"] <= 2e-3 * max(1.0, abs(exact["f"]))   # ftol 1e-4 stops near the optimum
    for budget in (1, 3, 25):
        x2, _, _, fin2, _ = _mine(trace_exe, cs, 0.0, budget, 1)
        assert fin2["evals"] == len(x2) <= budget


def test_infeasible_problem_returns_the_least_violation(trace_exe):
    """An external problem (values fed through standard input) whose constraint no point of the box satisfies."""
    def run(args, fun):
        p = subprocess.Popen([trace_exe] + args, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        pts, vals = [], []
        while True:
            ln = p.stdout.readline()
            if not ln or ln.startswith("#"):
                rest = [ln] + p.stdout.readlines()
                break
            xx = np.array([float(v) for v in ln.split()])
            fv, cv = fun(xx)
            pts.append(xx), vals.append((fv, cv))
            p.stdin.write(f"{fv!r} {cv!r}\n")
            p.stdin.flush()
        p.stdin.close()
        assert p.wait() == 0
        return np.array(pts), vals, rest
    fun = lambda x: (float(x[0] + x[1]), float(1.0 + (x[0] - 0.5) ** 2 + (x[1] - 0.25) ** 2))   # c >= 1 everywhere
    pts, vals, rest = run(["9", "0.5", "0", "200", "1", "2", "1", "0.9", "0.9", "0", "0", "1", "1"], fun)
    t, xb, cb = _summary(rest[-1], 2, 1)
    assert int(t[3]) == 0                                      # infeasible
    assert cb[0] == min(v[1] for v in vals) == float(t[5])     # the smallest violation among the evaluated points
    assert cb[0] - 1.0 < 1e-3                                  # ... which COBYLA's first stage drove to the least one
    assert np.all(pts >= 0.0) and np.all(pts <= 1.0)


def test_under_address_and_ub_sanitizers(tmp_path):
    """The same trace program built with -fsanitize=address,undefined, run stand-alone on all four cases in both modes, tiny
    budgets (the initial simplex is cut short) included."""
    exe = tmp_path / "cobyla_cstr_trace_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", SRC, "-o", str(exe)], check=True)
    for cs in range(4):
        for mode in (0, 1):
            for maxeval in (1, 2, 4, 300):
                out = subprocess.run([str(exe), str(cs), "0.5", "1e-7", str(maxeval), str(mode)], capture_output=True, text=True)
                assert out.returncode == 0 and "runtime error" not in out.stderr, (cs, mode, maxeval, out.stderr[-400:])
                assert int(out.stdout.strip().split("\n")[-2].split()[5]) <= maxeval
