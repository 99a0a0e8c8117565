"""The constraint surrogates as constraints of the infill optimiser (cstr_infill = false; egx_infill_set_cstr_strategy,
egx_infill_eval_cstr, egx_infill_optimize_cstr; infill_eval.hip, infill_optimize.hip, kernels_infill.hip, cobyla.h): the constraint values and
their gradients against the handle's own parts (the mean-only launch sequence against the full one, bit for bit), against
oracle.gp_oracle and against central differences; the modes; the lock-step multistart with general constraints; a compiled
host of the C ABI and of the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_sample import oracle_from_handle

KINDS = ["SquaredExponential", "AbsoluteExponential", "Matern32", "Matern52"]
MEANS = ["Constant", "Linear", "Quadratic"]
PRED_RTOL = 1e-6  # tests/test_gpu_parity.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 127, 128, 129, 300)


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


def _data(n, d, seed, yscale=1.0):
    from egobox_amd import workload
    x, y = workload.make_training_set(n, d, seed=seed)
    return x, yscale * y


# (n, regression, correlation) of: the objective, constraint 1, constraint 2, the two experts of the mixture constraint
SPECS = {2: [(120, 0, 0), (40, 1, 3), (77, 2, 2), (60, 0, 0), (45, 0, 3)],
         5: [(300, 0, 0), (40, 1, 3), (77, 2, 2), (60, 0, 0), (45, 0, 3)]}
SCALES2 = np.array([2.0, 0.5, 4.0])   # powers of two: (mu / s) * s is mu exactly
SCALESX = np.array([1.7, 0.3, 2.9])


class _Fix:
    pass


def _gmx2(egx, d):
    means = np.full((2, d), 0.5)
    means[:, d - 1] = [0.3, 0.7]
    return egx.GaussianMixture([0.45, 0.55], means, np.stack([np.eye(d) * 0.08, np.eye(d) * 0.06]), 1.0)


@pytest.fixture(scope="module", params=[2, 5])
def fix(request, egx):
    d = request.param
    f = _Fix()
    f.d, f.sets, f.handles = d, [], []
    for e, (n, mean, corr) in enumerate(SPECS[d]):
        x, y = _data(n, d, seed=300 + 10 * d + e, yscale=1e-3 if e == 0 else 1.0)
        if e:
            y = y - np.quantile(y, 0.6)
        h = egx.GpHandle(x, y, mean=mean, corr=corr)
        h.finalize(np.full(d, 1.2 + 0.1 * e))
        f.sets.append((x, y)), f.handles.append(h)
    gps = [egx.GaussianProcess(h, None) for h in f.handles]
    f.mix = {mode: egx.GpMixture(gps[3:5], _gmx2(egx, d), mode) for mode in ("smooth", "hard")}
    f.fmin = float(np.quantile(f.sets[0][1], 0.1))
    rng = np.random.default_rng(900 + d)
    lo, hi = f.sets[0][0].min(axis=0), f.sets[0][0].max(axis=0)
    f.xq = lo + (hi - lo) * rng.random((300, d))
    kw = dict(criterion=egx.WB2, fmin=f.fmin, sigma_weight=0.75, scale=1.3)
    f.kw = kw
    # the constraint lists: n_cstr = 1 (single models: egx_infill_create) and n_cstr = 3 with a smooth / a hard mixture
    f.cstr = {"k1": [f.handles[1]], "k3s": [f.handles[1], f.handles[2], f.mix["smooth"]],
              "k3h": [f.handles[1], f.handles[2], f.mix["hard"]]}
    # references, computed once and left unchanged: the constraint-free handle and the parts of EGX_CSTR_INFILL handles
    with egx.InfillObjective(f.handles[0], **kw) as bare:
        f.bare_v, f.bare_g = bare.value_and_grad(f.xq)
    f.parts = {}
    for name, cs in f.cstr.items():
        with egx.InfillObjective(f.handles[0], cs, [0.0] * len(cs), **kw) as full:
            f.parts[name] = full.parts(f.xq)
    yield f
    for h in f.handles:
        h.close()


def _handle(egx, f, name, strategy, scales):
    cs = f.cstr[name]
    obj = egx.InfillObjective(f.handles[0], cs, [0.0] * len(cs), **f.kw)
    obj.set_cstr_strategy(strategy, scales[:len(cs)])
    return obj


# ---- 1. values and gradients ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["k1", "k3s", "k3h"])
def test_values_mean_and_utb(egx, O, fix, name):
    f, k = fix, len(fix.cstr[name])
    p = f.parts[name]
    for scales in (SCALES2, SCALESX):
        s = scales[:k]
        with _handle(egx, f, name, "mean", scales) as obj:
            for m in SIZES:
                v, c = obj.constraints(f.xq[:m])
                assert v.shape == (m,) and c.shape == (m, k)
                np.testing.assert_array_equal(v, f.bare_v[:m])            # the objective surrogate alone, bit for bit
                np.testing.assert_array_equal(c, p["mean"][1:, :m].T / s)  # the mean-only sequence against the full one
                if scales is SCALES2:
                    np.testing.assert_array_equal(c * s, p["mean"][1:, :m].T)
            np.testing.assert_array_equal(obj.value(f.xq), f.bare_v)      # egx_infill_eval in this mode
            empty = obj.constraints(np.zeros((0, f.d)))
            assert empty[0].shape == (0,) and empty[1].shape == (0, k)
        with _handle(egx, f, name, "utb", scales) as obj:
            for m in SIZES:
                v, c = obj.constraints(f.xq[:m])
                np.testing.assert_array_equal(v, f.bare_v[:m])
                np.testing.assert_array_equal(c, (p["mean"][1:, :m].T + 3.0 * np.sqrt(p["var"][1:, :m].T)) / s)
    # the means against the oracle on the handles' own fitted state, at the project's 1e-6
    with _handle(egx, f, name, "mean", SCALES2) as obj:
        c = obj.constraints(f.xq)[1] * SCALES2[:k]
    refs = [oracle_from_handle(O, f.handles[e], MEANS[SPECS[f.d][e][1]], KINDS[SPECS[f.d][e][2]], *f.sets[e]) for e in range(1, 5)]
    mus = [np.ravel(r.predict(f.xq)) for r in refs]
    np.testing.assert_allclose(c[:, 0], mus[0], rtol=PRED_RTOL, atol=1e-9)
    if k == 3:
        np.testing.assert_allclose(c[:, 1], mus[1], rtol=PRED_RTOL, atol=1e-9)
        pr = f.mix["smooth"].gmx.predict_probas(f.xq)
        want = pr[:, 0] * mus[2] + pr[:, 1] * mus[3] if name == "k3s" else np.where(np.argmax(pr, axis=1) == 0, mus[2], mus[3])
        np.testing.assert_allclose(c[:, 2], want, rtol=PRED_RTOL, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["k1", "k3s", "k3h"])
@pytest.mark.parametrize("strategy", ["mean", "utb"])
def test_gradients(egx, fix, name, strategy):
    f, k, d = fix, len(fix.cstr[name]), fix.d
    p, s, m = f.parts[name], SCALESX[:len(fix.cstr[name])], 129
    x = f.xq[:m]
    with _handle(egx, f, name, strategy, SCALESX) as obj:
        v, c, g, gc = obj.constraints(x, grad=True)
        v0, c0 = obj.constraints(x)
        np.testing.assert_array_equal(v, v0)                # the values do not depend on the gradient work
        np.testing.assert_array_equal(c, c0)
        np.testing.assert_array_equal(g, f.bare_g[:m])      # the objective surrogate's gradient alone
        vg = obj.value_and_grad(x)
        np.testing.assert_array_equal(vg[1], g)
        gm, gv = p["grad_mean"][1:, :m].transpose(1, 0, 2), p["grad_var"][1:, :m].transpose(1, 0, 2)
        if strategy == "mean":                              # the mean-only gradient sequence against the full one
            np.testing.assert_array_equal(gc, gm / s[None, :, None])
        else:
            sigma = np.sqrt(p["var"][1:, :m].T)[:, :, None]
            assert np.all(sigma >= np.finfo(float).eps)
            np.testing.assert_array_equal(gc, (gm + 3.0 * (gv / (2.0 * sigma))) / s[None, :, None])
        # central differences of cstr through the same entry point; tolerance and step of tests/c_host/infill_driver.c
        e = 1e-5
        pr = f.mix["smooth"].gmx.predict_probas(x)
        clear = np.abs(pr[:, 0] - pr[:, 1]) > 0.05          # a hard mixture jumps where its experts change over
        worst = 0.0
        for l in range(d):
            xp, xm = x.copy(), x.copy()
            xp[:, l] += e
            xm[:, l] -= e
            fd = (obj.constraints(xp)[1] - obj.constraints(xm)[1]) / (2.0 * e)
            err = np.abs(fd - gc[:, :, l]) / (1.0 + np.abs(fd))
            if name == "k3h":
                err[~clear, 2] = 0.0
            worst = max(worst, float(err.max()))
        print(f"d {d} {name} {strategy}: worst gradient error against central differences {worst:.2e}")
        assert worst <= 1e-5
        assert clear.sum() >= m // 2


@pytest.mark.gpu
def test_sigma_prime_is_zero_where_the_variance_is(egx):
    """A constraint model WITHOUT nugget: at its training points the posterior variance is rounding noise and is clamped to
    exactly 0 at some of them; there sigma < f64::EPSILON and the upper trust bound's gradient is the mean's."""
    d = 2
    xo, yo = _data(60, d, seed=411, yscale=1e-3)
    xc, yc = _data(40, d, seed=412)
    with egx.GpHandle(xo, yo) as ho, egx.GpHandle(xc, yc - np.median(yc), corr=2, nugget=0.0) as hc:
        ho.finalize(np.full(d, 1.3))
        hc.finalize(np.full(d, 2.5))
        with egx.InfillObjective(ho, [hc], [0.0], criterion=egx.EI, fmin=float(yo.min())) as obj:
            p = obj.parts(xc)
            obj.set_cstr_strategy("utb", [1.7])
            _, c, _, gc = obj.constraints(xc, grad=True)
        var, gm, gv = p["var"][1], p["grad_mean"][1], p["grad_var"][1]
        zero = var == 0.0
        print(f"variance clamped to 0 at {int(zero.sum())} of {len(var)} training points; largest {var.max():.2e}")
        assert zero.sum() >= 1
        np.testing.assert_array_equal(gc[zero, 0], gm[zero] / 1.7)
        np.testing.assert_array_equal(c[zero, 0], p["mean"][1][zero] / 1.7)
        live = np.sqrt(var) >= np.finfo(float).eps
        assert np.all(live | zero)
        np.testing.assert_array_equal(gc[live, 0], (gm[live] + 3.0 * (gv[live] / (2.0 * np.sqrt(var[live])[:, None]))) / 1.7)


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", ["mean", "utb"])
def test_a_point_does_not_depend_on_its_companions(egx, fix, strategy):
    f, d = fix, fix.d
    pts = f.xq[:64]
    big = f.xq[64:264].copy()
    big[100:164] = pts                                      # across the boundary of the 128-point tiles
    bad = pts.copy()
    bad[5, d - 1] = np.nan                                  # one NaN row
    with _handle(egx, f, "k3s", strategy, SCALESX) as obj:
        base = obj.constraints(pts, grad=True)
        rev = obj.constraints(pts[::-1].copy(), grad=True)
        inb = obj.constraints(big, grad=True)
        nan = obj.constraints(bad, grad=True)
        for a, b, c, n in zip(base, rev, inb, nan):
            np.testing.assert_array_equal(a, b[::-1])
            np.testing.assert_array_equal(a, c[100:164])
            keep = np.arange(64) != 5
            np.testing.assert_array_equal(a[keep], n[keep])
        assert nan[0][5] == np.inf and np.all(nan[1][5] == np.inf) and np.all(nan[2][5] == 0.0) and np.all(nan[3][5] == 0.0)
        for i in (0, 17, 63):
            one = obj.constraints(pts[i:i + 1], grad=True)
            for a, b in zip(base, one):
                np.testing.assert_array_equal(a[i], b[0])


# ---- 2. modes -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_modes(egx, fix):
    f = fix
    cs = f.cstr["k3s"]
    pts = f.xq[:200]
    kw = dict(criterion=egx.WB2S, fmin=f.fmin, sigma_weight=0.75)
    with egx.InfillObjective(f.handles[0], **kw) as bare, egx.InfillObjective(f.handles[0], cs, [0.1, 0.2, 0.3], **kw) as obj:
        assert obj.cstr_strategy()[0] == "infill"
        np.testing.assert_array_equal(obj.cstr_strategy()[1], np.ones(3))
        before = obj.parts(pts)
        sic0, sc0, scs0 = obj.scaling(pts)
        with pytest.raises(egx.InvalidValueError, match="EGX_CSTR_INFILL"):
            obj.constraints(pts)
        with pytest.raises(egx.InvalidValueError, match="EGX_CSTR_INFILL"):
            obj.optimize_constrained(np.array([[0.0, 1.0]] * f.d), pts[:2])
        np.testing.assert_array_equal(obj.cstr_strategy()[1], np.ones(3))  # "infill" stores no scales
        for bad in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [np.inf, 1.0, 1.0], [np.nan, 1.0, 1.0]):
            with pytest.raises(egx.InvalidValueError, match="scale_cstr"):
                obj.set_cstr_strategy("mean", bad)
        with pytest.raises(egx.InvalidValueError):
            obj.set_cstr_strategy("mean", [1.0, 1.0])
        with pytest.raises(egx.InvalidValueError):
            obj.set_cstr_strategy("median")
        assert obj.cstr_strategy()[0] == "infill"
        obj.set_params(scale_ic=1.0, scale=1.0)
        for strategy in ("mean", "utb"):
            obj.set_cstr_strategy(strategy)
            assert obj.cstr_strategy()[0] == strategy
            sic_b, sc_b, _ = bare.scaling(pts)
            sic, sc, scs = obj.scaling(pts)
            assert (sic, sc) == (sic_b, sc_b)                              # the scale of the constraint-free handle
            np.testing.assert_array_equal(scs, scs0)
            np.testing.assert_array_equal(obj.cstr_strategy()[1], scs)     # ... and scale_cstr is stored
            np.testing.assert_array_equal(obj.value(pts), bare.value(pts))
            v, g = obj.value_and_grad(pts)
            vb, gb = bare.value_and_grad(pts)
            np.testing.assert_array_equal(v, vb)
            np.testing.assert_array_equal(g, gb)
            np.testing.assert_array_equal(obj.constraints(pts)[1], before["mean"][1:].T / scs if strategy == "mean" else
                                          (before["mean"][1:].T + 3.0 * np.sqrt(before["var"][1:].T)) / scs)
            now = obj.parts(pts)                                           # parts stay as they are (the full sequence)
            for key in ("mean", "var", "grad_mean", "grad_var"):
                np.testing.assert_array_equal(now[key], before[key])
            obj.set_cstr_strategy(strategy, [3.0, 5.0, 7.0])
            np.testing.assert_array_equal(obj.cstr_strategy()[1], [3.0, 5.0, 7.0])
        obj.set_cstr_strategy("infill")                                    # today's bits come back
        obj.set_params(scale_ic=1.0, scale=1.0)
        assert obj.scaling(pts)[:2] == (sic0, sc0)
        obj.set_params(scale_ic=1.0, scale=1.0)
        again = obj.parts(pts)
        for key in ("value", "grad", "mean", "var", "grad_mean", "grad_var"):
            np.testing.assert_array_equal(again[key], before[key])
    # n_cstr = 0: the constraint table is empty, the optimiser is a bound-constrained run of the same class
    with egx.InfillObjective(f.handles[0], **f.kw) as bare:
        bare.set_cstr_strategy("mean")
        v, c = bare.constraints(pts)
        assert c.shape == (200, 0)
        np.testing.assert_array_equal(v, f.bare_v[:200])
        lim = np.array([[0.0, 1.0]] * f.d)
        x, fb, cb, st = bare.optimize_constrained(lim, pts[:2], max_eval=30)
        assert cb.shape == (0,) and st["feasible"] and st["violation"] == 0.0 and st["finite"]
        assert bare.constraints(x)[0][0] == fb and fb <= f.bare_v[:2].min()


# ---- 3. the optimiser -----------------------------------------------------------------------------------------------------
def opt_problem(which="active"):
    """d = 2 on [0, 1]^2: one objective GP, one constraint GP, three starts.  "active": the minimiser of the unconstrained
    criterion sits where the constraint surrogate is positive.  "infeasible": the constraint is positive on the whole box."""
    from egobox_amd import workload
    xo, xc = workload.lhs(60, 2, 501), workload.lhs(50, 2, 502)
    yo = (xo[:, 0] - 0.8) ** 2 + (xo[:, 1] - 0.7) ** 2 + 0.2 * np.sin(4.0 * xo[:, 0])
    yc = xc[:, 0] + xc[:, 1] - 1.0 + 0.1 * np.sin(3.0 * xc[:, 0]) + (3.0 if which == "infeasible" else 0.0)
    starts = np.array([[0.2, 0.3], [0.5, 0.9], [0.9, 0.2]])
    return dict(xo=xo, yo=yo, xc=xc, yc=yc, theta_o=np.array([0.9, 0.9]), theta_c=np.array([0.6, 0.6]), starts=starts,
                lim=np.array([[0.0, 1.0], [0.0, 1.0]]), fmin=float(yo.min()), tol=1e-4, scale_cstr=2.0)


# How far the multistart may end above the best feasible value of a 101 x 101 grid.  Provenance: the CPU trace program
# (tests/c_host/cobyla_cstr_trace.cpp, external problem, the additions on, 60 evaluations per start, feasibility tolerance
# tol / scale_cstr) run over the oracle's restatement of the same two functions (oracle.gp_oracle.fit_fixed at the same theta,
# tests/infill_oracle.py's WB2 objective) from the same three starts ends at 0.3090057, 0.3090135 and 0.3090300 (all three
# feasible), the grid's best feasible value is 0.3100031: the largest gap observed is GRID_GAP_OBSERVED, NEGATIVE -- the
# multistart ends 1e-3 BELOW the grid.  Doubling a negative gap would ask for more than was observed, so the margin is twice
# the larger of that gap and of the 1e-6 oracle / GPU parity on a value of the optimum's size.
GRID_GAP_OBSERVED = -9.97e-4
GRID_PARITY = 1e-6 * 0.31
GRID_MARGIN = 2.0 * max(GRID_GAP_OBSERVED, GRID_PARITY)


@pytest.mark.gpu
def test_constrained_multistart(egx):
    pb = opt_problem()
    with egx.GpHandle(pb["xo"], pb["yo"]) as ho, egx.GpHandle(pb["xc"], pb["yc"]) as hc:
        ho.finalize(pb["theta_o"])
        hc.finalize(pb["theta_c"])
        with egx.InfillObjective(ho, [hc], [pb["tol"]], criterion=egx.WB2, fmin=pb["fmin"]) as obj:
            obj.set_cstr_strategy("mean", [pb["scale_cstr"]])
            cfeas = pb["tol"] / pb["scale_cstr"]
            # not vacuous: the unconstrained optimum violates the constraint
            _, xu, _ = obj.optimize(pb["lim"], pb["starts"])
            vu, cu = obj.constraints(xu)
            assert cu[0, 0] > 100 * cfeas, cu
            x, fb, cb, st = obj.optimize_constrained(pb["lim"], pb["starts"])
            assert st["feasible"] and st["finite"] and cb[0] <= cfeas
            assert st["violation"] == cb[0] - cfeas
            v1, c1 = obj.constraints(x)
            assert v1[0] == fb and c1[0, 0] == cb[0]                       # bit for bit eval_cstr at x_best
            assert np.all(x >= 0.0) and np.all(x <= 1.0)
            assert fb > vu[0]                                              # the constraint costs something
            assert np.all(st["evals"] >= 1) and np.all(st["evals"] <= 60) and st["rounds"] == st["evals"].max()
            # each start alone walks the same points: the same evaluation counts and the same best point
            # (the default budget min(10 n_start d, 2000) depends on the number of starts: the lone runs get the 60 of the three)
            singles = [obj.optimize_constrained(pb["lim"], pb["starts"][i:i + 1], max_eval=60) for i in range(3)]
            np.testing.assert_array_equal(st["evals"], [s[3]["evals"][0] for s in singles])
            keys = [(0, s[1]) if s[3]["feasible"] else (1, s[3]["violation"]) for s in singles]
            best = min(range(3), key=lambda i: (keys[i], i))              # feasible first, then f / violation, then the first
            assert st["best_start"] == best
            np.testing.assert_array_equal(x, singles[best][0])
            assert fb == singles[best][1] and cb[0] == singles[best][2][0]
            # against the best feasible value of a 101 x 101 grid evaluated by the same entry point
            g = np.linspace(0.0, 1.0, 101)
            grid = np.array([[a, b] for a in g for b in g])
            vg, cg = obj.constraints(grid)
            ok = cg[:, 0] <= cfeas
            assert ok.sum() > 1000 and (~ok).sum() > 1000
            print(f"constrained optimum {fb:.9g} at {x}, c = {cb[0]:.3e}; grid {vg[ok].min():.9g}; unconstrained {vu[0]:.9g} "
                  f"at {xu} (c = {cu[0, 0]:.3e}); evals {st['evals']}")
            assert fb <= vg[ok].min() + GRID_MARGIN


@pytest.mark.gpu
def test_infeasible_box_returns_the_least_violation(egx):
    pb = opt_problem("infeasible")
    with egx.GpHandle(pb["xo"], pb["yo"]) as ho, egx.GpHandle(pb["xc"], pb["yc"]) as hc:
        ho.finalize(pb["theta_o"])
        hc.finalize(pb["theta_c"])
        with egx.InfillObjective(ho, [hc], [pb["tol"]], criterion=egx.WB2, fmin=pb["fmin"]) as obj:
            obj.set_cstr_strategy("utb", [pb["scale_cstr"]])
            x, fb, cb, st = obj.optimize_constrained(pb["lim"], pb["starts"], max_eval=40)   # EGX_SUCCESS: no exception
            assert not st["feasible"] and st["finite"] and cb[0] > 0.5
            v1, c1 = obj.constraints(x)
            assert v1[0] == fb and c1[0, 0] == cb[0]
            # the smallest violation among the evaluated points: no start alone found a smaller one, and the winner is the
            # first start with that violation
            singles = [obj.optimize_constrained(pb["lim"], pb["starts"][i:i + 1], max_eval=40) for i in range(3)]
            viol = [s[3]["violation"] for s in singles]
            assert st["violation"] == min(viol) == cb[0] - pb["tol"] / pb["scale_cstr"]
            assert st["best_start"] == int(np.argmin(viol))
            g = np.linspace(0.0, 1.0, 101)
            cg = obj.constraints(np.array([[a, b] for a in g for b in g]))[1]
            assert cg.min() > 0.5                                           # no point of the box satisfies it
            print(f"least violation found {cb[0]:.6g} at {x}; over the grid {cg.min():.6g}")
            assert cb[0] <= cg.min() + 0.05 * abs(cg.min())                 # stage one went for the least violation


# ---- 4. C and C++ hosts ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_compiled_host_drives_the_cstr_entry_points_and_the_cpp_mirror(tmp_path):
    exe = tmp_path / "infill_cstr_driver"
    libdir = os.path.join(ROOT, "egobox_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "c_host", "infill_cstr_driver.cpp"), f"-L{libdir}", "-legx_gp_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert out.stdout.startswith("OK"), out.stdout
