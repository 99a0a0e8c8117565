"""Writes tests/golden/infill_kat.json: known answers for egobox_amd/csrc/infill_math.h (tests/test_infill_cpu.py).
Needs mpmath (60 digits); the tests that read the file need numpy only.

  pinned     the reference's own test values of log_ei_helper (crates/ego/src/utils/logei_helper.rs:88-95), to 1e-6
  helper     60-digit truths of  log(phi(u) + u Phi(u))  and  Phi(u) / (phi(u) + u Phi(u))  on a grid over [-1e8, 10]
  ref_error  the error of the reference-shaped double formulas (tests/infill_oracle.py ref_*) against those truths on (-37, 10]
  toy        smooth toy models mu_j(x), var_j(x): the parts at seeded points with the 60-digit value of every objective
             variant and its mpmath.diff gradient, so that the gradient formulas are checked as DERIVATIVES of the values
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import infill_oracle as IO  # noqa: E402

mp.mp.dps = 60
EI, LOG_EI, WB2, WB2S = 0, 1, 2, 3
EPS = mp.mpf(2) ** -52


def h_true(u):
    u = mp.mpf(u)
    return mp.log(mp.npdf(u) + u * mp.ncdf(u))


def dh_true(u):
    u = mp.mpf(u)
    return mp.ncdf(u) / (mp.npdf(u) + u * mp.ncdf(u))


def helper_grid():
    named = [-1.0, -37.0, -37.6, -38.0, -40.0, -1e3, -1e6 - 1, -1e6, -1e6 + 1, -1e8,
             -19.999, -20.0, -20.001, -25.0, -30.0, -50.0, -100.0, -1e4, -1e5, -1e7, -0.999, -1.001, 0.0, 10.0]
    lin = [float(v) for v in np.linspace(-36.9, 9.9, 118)]
    return sorted(set(named + lin))


def ref_error(grid, truths):
    worst_v, worst_d = (0.0, None), (0.0, None)
    for u, (tv, td) in zip(grid, truths):
        if not (-37.0 < u <= 10.0):
            continue
        ev = abs(mp.mpf(IO.ref_log_ei_helper(u)) - tv) / max(1, abs(tv))
        ed = abs(mp.mpf(IO.ref_d_log_ei_helper(u)) - td) / max(1, abs(td))
        if ev > worst_v[0]:
            worst_v = (float(ev), u)
        if ed > worst_d[0]:
            worst_d = (float(ed), u)
    return {"value": worst_v[0], "value_at": worst_v[1], "derivative": worst_d[0], "derivative_at": worst_d[1]}


# ---- the toy: mu_j(x) = a_j + sum_c b_jc sin(w_jc x_c),  var_j(x) = s_j (1 + sum_c c_jc x_c^2) --------------------------
def toy_models(rng, d, nm):
    return [dict(a=float(rng.uniform(-0.3, 0.6)), b=rng.uniform(-0.5, 0.5, d).tolist(), w=rng.uniform(0.5, 2.0, d).tolist(),
                 s=float(rng.uniform(0.05, 0.4)), c=rng.uniform(0.1, 1.0, d).tolist()) for _ in range(nm)]


def toy_mu(mdl, x):
    return mdl["a"] + sum(mp.mpf(b) * mp.sin(mp.mpf(w) * xc) for b, w, xc in zip(mdl["b"], mdl["w"], x))


def toy_var(mdl, x):
    return mp.mpf(mdl["s"]) * (1 + sum(mp.mpf(c) * xc * xc for c, xc in zip(mdl["c"], x)))


def ei_mp(mu, var, fmin, k):
    s = k * mp.sqrt(var)
    a = (fmin - mu) / s
    return s * (a * mp.ncdf(a) + mp.npdf(a))


def crit_mp(kind, mu, var, fmin, k, scale_ic):
    if kind == EI:
        return ei_mp(mu, var, fmin, k)
    if kind == LOG_EI:
        s = mp.sqrt(var)
        u = (fmin - mu) / s
        return mp.log(mp.npdf(u) + u * mp.ncdf(u)) + mp.log(s)
    return (1 if kind == WB2 else scale_ic) * ei_mp(mu, var, fmin, k) - mu


def objective_mp(case, models, x):
    kind, k = case["kind"], case["k"]
    mu0, var0 = toy_mu(models[0], x), toy_var(models[0], x)
    if case["feasibility"]:
        obj = -crit_mp(kind, mu0, var0, mp.mpf(case["fmin"]), mp.mpf(case["sigma_weight"]), mp.mpf(case["scale_ic"])) / mp.mpf(case["scale"])
    else:
        obj = mp.mpf(0) if kind == LOG_EI else mp.mpf(-1)
    if k == 0:
        return obj
    pofs = [mp.ncdf((mp.mpf(case["tol"]) - toy_mu(models[1 + j], x)) / mp.sqrt(toy_var(models[1 + j], x))) for j in range(k)]
    if kind == LOG_EI:
        return obj - sum(mp.log(max(p, EPS)) for p in pofs)
    out = obj
    for p in pofs:
        out *= p
    return out


def toy_parts(models, x, d):
    """mu, var, dmu, dvar of every model at x, 60 digits rounded to doubles"""
    mu = [float(toy_mu(m, x)) for m in models]
    var = [float(toy_var(m, x)) for m in models]
    dmu = [[float(mp.mpf(m["b"][c]) * mp.mpf(m["w"][c]) * mp.cos(mp.mpf(m["w"][c]) * x[c])) for c in range(d)] for m in models]
    dvar = [[float(2 * mp.mpf(m["s"]) * mp.mpf(m["c"][c]) * x[c]) for c in range(d)] for m in models]
    return mu, var, dmu, dvar


def norm_err(got, want):
    want = np.asarray(want, float)
    return float(np.max(np.abs(np.asarray(got, float) - want)) / max(1.0, np.max(np.abs(want))))


def make_toy():
    d = 3
    out = {"d": d, "cases": []}
    for seed in range(1000):
        rng = np.random.default_rng(2024 + seed)
        models = toy_models(rng, d, 3)
        xs = [[mp.mpf(float(v)) for v in rng.uniform(-1.0, 1.0, d)] for _ in range(3)]
        cases, ok = [], True
        for kind in (EI, LOG_EI, WB2, WB2S):
            for k, feas in ((0, 1), (2, 1), (2, 0)):
                for x in xs:
                    case = dict(kind=kind, k=k, tol=0.3, fmin=0.2, sigma_weight=0.75, scale_ic=2.3, scale=1.7, feasibility=feas)
                    mu, var, dmu, dvar = toy_parts(models[:1 + k], x, d)
                    case.update(x=[float(v) for v in x], mu=mu, var=var, dmu=dmu, dvar=dvar)
                    case["value"] = float(objective_mp(case, models, x))
                    grad = []
                    for c in range(d):
                        order = tuple(1 if i == c else 0 for i in range(d))
                        grad.append(float(mp.diff(lambda *xx: objective_mp(case, models, xx), tuple(x), order)))
                    case["grad"] = grad
                    # the reference's formulas must MISS this derivative where they deviate: pof_grad at tol != 0 (k = 2) and the
                    # k-less objective gradient (feasible cases of the criteria that use sigma_weight)
                    parts = (np.array(mu), np.array(var), np.array(dmu), np.array(dvar))
                    tols = [case["tol"]] * k
                    ref = IO.ref_objective_grad(kind, parts, tols, case["fmin"], case["sigma_weight"], case["scale_ic"], case["scale"], feas)
                    case["ref_grad_error"] = norm_err(ref, grad)
                    dev = IO.dev_objective_grad(kind, parts, tols, case["fmin"], case["sigma_weight"], case["scale_ic"], case["scale"], feas)
                    if norm_err(dev, grad) > 1e-9:
                        raise SystemExit(f"the named deviations are not the derivative: {case}")
                    must_miss = k == 2 or (feas and kind != LOG_EI)
                    case["ref_must_miss"] = bool(must_miss)
                    if must_miss and case["ref_grad_error"] < 1e-3:
                        ok = False
                    cases.append(case)
        if ok:
            out["cases"], out["seed"] = cases, 2024 + seed
            return out
    raise SystemExit("no seed gives inputs at which the reference's formulas miss by 1e-3")


def main():
    grid = helper_grid()
    truths = [(h_true(u), dh_true(u)) for u in grid]
    kat = {
        "pinned": {"u": [-2.0, -1.0, 0.0, 1.0, 2.0], "log_ei_helper": [-4.7687836, -2.4851208, -0.9189385, 0.08002624, 0.69738346]},
        "helper": {"u": grid, "value": [float(t[0]) for t in truths], "derivative": [float(t[1]) for t in truths]},
        "ref_error": ref_error(grid, truths),
        "toy": make_toy(),
    }
    with open(os.path.join(HERE, "infill_kat.json"), "w") as f:
        json.dump(kat, f, indent=0)
    print("ref_error", kat["ref_error"], "toy cases", len(kat["toy"]["cases"]), "seed", kat["toy"]["seed"])


if __name__ == "__main__":
    main()
