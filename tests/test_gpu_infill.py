"""The fused infill evaluation on the GPU (egx_infill_*; egobox_amd/csrc/infill_eval.hip, kernels_infill.hip): its parts against
oracle.gp_oracle on the handle's own fitted state, the criterion against tests/infill_oracle.py applied to those parts, the
bit-independence of a point from its companions, the scaling pass, the lock-step multistart, errors and state."""
import os
import subprocess

import numpy as np
import pytest

import infill_oracle as IO
from test_gpu_sample import oracle_from_handle

pytestmark = pytest.mark.gpu

KINDS = ["SquaredExponential", "AbsoluteExponential", "Matern32", "Matern52"]
MEANS = ["Constant", "Linear", "Quadratic"]
PRED_RTOL = 1e-6  # tests/test_gpu_parity.py
CRITERIA = [IO.EI, IO.LOG_EI, IO.WB2, IO.WB2S]


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


def _data(n, d, seed=0, yscale=1.0):
    """The project's training set.  OBJECTIVE models take yscale = 1e-3: the posterior variance at a training point is
    ~ nugget * sigma2 (1.6e-11 for the unscaled outputs at n = 600), and the cases here ask for training points at the
    f64::EPSILON rule (var < EPSILON: EI = 0, LogEI = f64::MIN), which the tests assert.  Just above EPSILON the LogEI gradient
    formula of the reference, d_log_ei_helper(u) u' + sigma'/sigma at u ~ -1e7, cancels ~13 digits in any double evaluation."""
    from egobox_amd import workload
    x, y = workload.make_training_set(n, d, seed=seed)
    return x, yscale * y


def _assert_rule_points(p):
    """the last three queries are training points of the objective model: variance below f64::EPSILON"""
    assert np.all(p["var"][0, -3:] < IO.EPS), p["var"][0, -3:]
    assert np.all(p["var"][0, :-3] > IO.EPS)


def _grad_tol(ref):  # tests/test_gpu_parity.py
    return dict(rtol=PRED_RTOL, atol=PRED_RTOL * np.abs(ref).max())


def _queries(x, m, seed):
    """m points uniform in the box of the training inputs plus three training points"""
    rng = np.random.default_rng(seed)
    lo, hi = x.min(axis=0), x.max(axis=0)
    return np.vstack([lo + (hi - lo) * rng.random((m, x.shape[1])), x[[0, x.shape[0] // 2, x.shape[0] - 1]]])


def _check_parts(O, handles, specs, xs, ys, p, xq):
    for j, (h, (mean, corr), x, y) in enumerate(zip(handles, specs, xs, ys)):
        ref = oracle_from_handle(O, h, MEANS[mean], KINDS[corr], x, y)
        ry, rv = ref.predict_valvar(xq)
        gy, gv = ref.predict_valvar_gradients(xq)
        np.testing.assert_allclose(p["mean"][j], np.ravel(ry), rtol=PRED_RTOL, atol=1e-9)
        np.testing.assert_allclose(p["var"][j], np.ravel(rv), rtol=PRED_RTOL, atol=1e-9 * ref.inner.sigma2)
        np.testing.assert_allclose(p["grad_mean"][j], gy, **_grad_tol(gy))
        np.testing.assert_allclose(p["grad_var"][j], gv, **_grad_tol(gv))


def _check_criterion(obj, p, tols):
    """value / grad of `obj` are the arithmetic of tests/infill_oracle.py on the returned parts (tolerances of the CPU suite)"""
    prm = obj.params
    m = p["value"].shape[0]
    worst_v = worst_g = 0.0
    for i in range(m):
        parts = (p["mean"][:, i], p["var"][:, i], p["grad_mean"][:, i, :], p["grad_var"][:, i, :])
        want_v = IO.objective(obj.criterion, parts[0], parts[1], tols, prm["fmin"], prm["sigma_weight"], prm["scale_ic"],
                              prm["scale"], prm["feasibility"], dev=True)
        want_g = IO.dev_objective_grad(obj.criterion, parts, tols, prm["fmin"], prm["sigma_weight"], prm["scale_ic"], prm["scale"],
                                       prm["feasibility"])
        ev = abs(p["value"][i] - want_v) / max(1.0, abs(want_v))
        eg = float(np.max(np.abs(p["grad"][i] - want_g)) / max(1.0, float(np.max(np.abs(want_g)))))
        worst_v, worst_g = max(worst_v, ev), max(worst_g, eg)
        assert ev <= 1e-11, (obj.criterion, i, p["value"][i], want_v)
        assert eg <= 1e-8, (obj.criterion, i, p["grad"][i], want_g)
    return worst_v, worst_g


# ---- 1 + 2: parts are the predictions, the criterion is the arithmetic of its parts ---------------------------------------
@pytest.mark.parametrize("mean", range(3))
@pytest.mark.parametrize("corr", range(4))
def test_parts_and_criterion_n600_d4(egx, O, mean, corr):
    x, y = _data(600, 4, seed=1, yscale=1e-3)
    theta = np.full(4, 1.5)
    xq = _queries(x, 30, seed=corr * 3 + mean)
    with egx.GpHandle(x, y, mean=mean, corr=corr) as h:
        h.finalize(theta)
        for crit in CRITERIA:
            with egx.InfillObjective(h, criterion=crit, fmin=float(np.quantile(y, 0.1)), sigma_weight=0.75, scale_ic=2.3,
                                     scale=1.7) as obj:
                p = obj.parts(xq)
                _assert_rule_points(p)
                if crit == IO.EI:
                    _check_parts(O, [h], [(mean, corr)], [x], [y], p, xq)
                wv, wg = _check_criterion(obj, p, [])
                print(f"n600 corr {corr} mean {mean} crit {crit}: value err {wv:.2e} grad err {wg:.2e}")


def _three_models(egx, n, d, seed):
    """an objective model and two constraint models on their own training sets (n, n - 100, n - 37 points)"""
    ns = [n, n - 100, n - 37]
    xs, ys, hs = [], [], []
    for j, nj in enumerate(ns):
        x, y = _data(nj, d, seed=seed + j, yscale=1.0 if j else 1e-3)
        if j:
            y = y - np.quantile(y, 0.6)  # feasible (<= tol) on a good part of the box
        h = egx.GpHandle(x, y, mean=j % 2, corr=[0, 3, 2][j])
        h.finalize(np.full(d, 1.2 + 0.2 * j))
        xs.append(x), ys.append(y), hs.append(h)
    return xs, ys, hs, [(j % 2, [0, 3, 2][j]) for j in range(3)]


@pytest.mark.parametrize("n,d,k", [(2000, 8, 0), (4096, 8, 2)])
def test_parts_and_criterion_large(egx, O, n, d, k):
    xs, ys, hs, specs = _three_models(egx, n, d, seed=11)
    try:
        xq = _queries(xs[0], 25, seed=5)
        tols = [0.3] * k
        fmin = float(np.quantile(ys[0], 0.05))
        checked = False
        for crit in CRITERIA:
            for feas in (True, False):
                with egx.InfillObjective(hs[0], hs[1:1 + k], tols, criterion=crit, fmin=fmin, sigma_weight=0.75, feasibility=feas,
                                         scale_ic=1.9, scale=2.5) as obj:
                    p = obj.parts(xq)
                    _assert_rule_points(p)
                    if not checked:
                        _check_parts(O, hs[:1 + k], specs[:1 + k], xs[:1 + k], ys[:1 + k], p, xq)
                        checked = True
                    wv, wg = _check_criterion(obj, p, tols)
                    print(f"n{n} k {k} crit {crit} feas {feas}: value err {wv:.2e} grad err {wg:.2e}")
    finally:
        for h in hs:
            h.close()


# ---- 3: a point does not depend on its companions -------------------------------------------------------------------------
@pytest.mark.parametrize("k,mean", [(0, 0), (2, 2)])
def test_a_point_does_not_depend_on_its_companions(egx, k, mean):
    d = 4
    xs, ys, hs = [], [], []
    for j in range(1 + k):
        x, y = _data(600 - 50 * j, d, seed=21 + j)
        h = egx.GpHandle(x, y - (np.median(y) if j else 0.0), mean=mean, corr=(j + 1) % 4)
        h.finalize(np.full(d, 1.5))
        xs.append(x), ys.append(y), hs.append(h)
    try:
        rng = np.random.default_rng(9)
        pts = np.vstack([rng.random((61, d)), xs[0][[0, 10, 20]]])  # 64 points, three of them training points
        fill = rng.random((200, d))
        with egx.InfillObjective(hs[0], hs[1:], [0.3] * k, criterion=egx.LOG_EI, fmin=float(np.quantile(ys[0], 0.1))) as obj:
            keys = ("value", "grad", "mean", "var", "grad_mean", "grad_var")

            def point(p, i):
                return [p["value"][i], p["grad"][i], p["mean"][:, i], p["var"][:, i], p["grad_mean"][:, i], p["grad_var"][:, i]]

            base = obj.parts(pts)
            rev = obj.parts(pts[::-1].copy())
            big = fill.copy()
            big[100:164] = pts  # across the boundary of the 128-point tiles
            bigp = obj.parts(big)
            nine = obj.parts(pts[:9])
            for i in range(64):
                for a, b, c, name in zip(point(base, i), point(rev, 63 - i), point(bigp, 100 + i), keys):
                    np.testing.assert_array_equal(a, b, err_msg=f"{name} of point {i}: reversed order")
                    np.testing.assert_array_equal(a, c, err_msg=f"{name} of point {i}: inside 200 points")
            for i in range(9):  # the other side of the predict entry points' m <= 8 switch
                for a, b, name in zip(point(base, i), point(nine, i), keys):
                    np.testing.assert_array_equal(a, b, err_msg=f"{name} of point {i}: m = 9")
            for i in range(64):  # m = 1, the three training points included
                one = obj.parts(pts[i:i + 1])
                for a, b, name in zip(point(base, i), point(one, 0), keys):
                    np.testing.assert_array_equal(a, b, err_msg=f"{name} of point {i}: alone")
            np.testing.assert_array_equal(obj.value(pts), base["value"])  # grad = NULL: the same values
            v, g = obj.value_and_grad(pts)
            np.testing.assert_array_equal(v, base["value"])
            np.testing.assert_array_equal(g, base["grad"])
    finally:
        for h in hs:
            h.close()


# ---- 4: scaling -----------------------------------------------------------------------------------------------------------
def test_scaling(egx):
    d = 4
    xs, ys, hs, _ = _three_models(egx, 600, d, seed=31)
    try:
        pts = np.random.default_rng(4).random((400, d))
        fmin = float(np.quantile(ys[0], 0.1))
        for crit, k in ((IO.EI, 0), (IO.LOG_EI, 2), (IO.WB2S, 0), (IO.WB2S, 2), (IO.WB2, 1)):
            tols = [0.3] * k
            kw = dict(criterion=crit, fmin=fmin, sigma_weight=0.75)
            with egx.InfillObjective(hs[0], hs[1:1 + k], tols, **kw) as obj:
                scale_ic, scale, scale_cstr = obj.scaling(pts)
                assert obj.params["scale_ic"] == scale_ic and obj.params["scale"] == scale  # stored in the handle
            # compute_scaling fed with the library's OWN values: equal, not close
            with egx.InfillObjective(hs[0], criterion=IO.EI, fmin=fmin, sigma_weight=0.75) as ei_obj:
                ei = -ei_obj.value(pts)  # EI itself (scale = 1)
                mean0 = ei_obj.parts(pts)["mean"][0]
            if crit == IO.WB2S:  # criteria/wb2.rs:67-88: the FIRST maximum of EI, then 100 |mean| / EI there
                i_max = int(np.argmax(ei))
                assert abs(ei[i_max]) > 100 * IO.EPS
                assert scale_ic == 100.0 * abs(mean0[i_max]) / ei[i_max]
            else:
                assert scale_ic == 1.0
            with egx.InfillObjective(hs[0], **kw, scale_ic=scale_ic, scale=1.0) as bare, \
                    egx.InfillObjective(hs[0], hs[1:1 + k], tols, **kw, scale_ic=scale_ic, scale=1.0) as unit:
                base, vals = bare.value(pts), unit.value(pts)
                full = unit.parts(pts)
            assert np.all(np.isfinite(base)) and np.all(np.isfinite(vals))  # no NaN / inf -> 1 replacement in this case
            assert scale == np.max(np.abs(vals))
            np.testing.assert_array_equal(scale_cstr, np.max(np.abs(full["mean"][1:]), axis=1).reshape(-1)[:k])
            # ... and the independent restatement on the host's libm, from the parts, agrees to rounding
            want_ic, want_scale, want_cstr = IO.compute_scaling(crit, full["mean"], full["var"], tols, fmin, 0.75)
            np.testing.assert_allclose(scale_ic, want_ic, rtol=1e-11)
            np.testing.assert_allclose(scale, want_scale, rtol=1e-11)
            np.testing.assert_array_equal(scale_cstr, want_cstr)
        # a point whose objective is not finite counts as 1.0 before the feasibility factor (solver_computations.rs:312-320)
        with egx.InfillObjective(hs[0], criterion=IO.EI, fmin=fmin) as obj:
            bad = pts.copy()
            bad[7, 2] = np.nan
            _, scale_nan, _ = obj.scaling(bad)
            with egx.InfillObjective(hs[0], criterion=IO.EI, fmin=fmin) as unit:
                v = unit.value(bad)
            assert v[7] == np.inf
            v[7] = 1.0
            assert scale_nan == np.max(np.abs(v)) == 1.0
        # all points infeasible: every pof underflows to 0, the scale falls back to 1
        with egx.InfillObjective(hs[0], hs[1:2], [-1e6], criterion=IO.EI, fmin=fmin) as obj:
            scale_ic, scale, _ = obj.scaling(pts)
            assert (scale_ic, scale) == (1.0, 1.0)
    finally:
        for h in hs:
            h.close()


# ---- 5: the multistart ----------------------------------------------------------------------------------------------------
def test_lockstep_multistart_is_the_single_runs(egx):
    d = 4
    xs, ys, hs, _ = _three_models(egx, 600, d, seed=41)
    try:
        lim = np.array([[0.0, 1.0]] * d)
        starts = np.random.default_rng(6).random((7, d))
        with egx.InfillObjective(hs[0], hs[1:], [0.3, 0.3], criterion=egx.LOG_EI, fmin=float(np.quantile(ys[0], 0.1))) as obj:
            obj.scaling(np.random.default_rng(7).random((200, d)))
            f, xb, st = obj.optimize(lim, starts, max_eval=60)
            singles = [obj.optimize(lim, starts[i:i + 1], max_eval=60) for i in range(7)]
            np.testing.assert_array_equal(st["evals"], [s[2]["evals"][0] for s in singles])
            fs = np.array([s[0] for s in singles])
            best = int(np.argmin(fs))  # the first minimum
            assert st["best_start"] == best and f == fs[best]
            np.testing.assert_array_equal(xb, singles[best][1])
            assert st["rounds"] == max(st["evals"])
            assert obj.value(xb)[0] == f
    finally:
        for h in hs:
            h.close()


@pytest.mark.parametrize("crit", [IO.EI, IO.LOG_EI])
def test_multistart_on_the_reference_toy(egx, crit):
    """crates/ego/src/criteria/ei.rs:198-199: five training points on [0, 25], the 26 integer points as starts."""
    xt = np.array([[0.0], [2.0], [5.0], [10.0], [25.0]])
    yt = np.array([0.0, 0.2, -0.3, 0.5, -1.0])
    with egx.GpHandle(xt, yt) as h:
        h.finalize(np.array([2.0]))
        with egx.InfillObjective(h, criterion=crit, fmin=float(yt.min())) as obj:
            starts = np.arange(26.0).reshape(-1, 1)
            lim = np.array([[0.0, 25.0]])
            v0 = obj.value(starts)
            f, xb, st = obj.optimize(lim, starts)
            max_eval = min(10 * 26 * 1, 2000)
            assert np.isfinite(f) and st["finite"]
            assert f <= np.min(v0)
            assert 0.0 <= xb[0] <= 25.0
            assert obj.value(xb)[0] == f
            assert np.all(st["evals"] >= 1) and np.all(st["evals"] <= max_eval)
            grid = obj.value(np.linspace(0.0, 25.0, 2001).reshape(-1, 1))
            print(f"toy crit {crit}: f_best {f:.12g} at x = {xb[0]:.6f}; 2001-point grid minimum {grid.min():.12g} at "
                  f"x = {np.linspace(0.0, 25.0, 2001)[int(np.argmin(grid))]:.4f}; values at the training points {v0[[0, 2, 5, 10, 25]]}")


def test_multistart_refusals_and_no_finite_start(egx):
    xt = np.array([[0.0], [2.0], [5.0], [10.0], [25.0]])
    yt = 1e-4 * np.array([0.0, 0.2, -0.3, 0.5, -1.0])  # so small that the variance at a training point is below f64::EPSILON
    with egx.GpHandle(xt, yt) as h:
        h.finalize(np.array([2.0]))
        with egx.InfillObjective(h, criterion=egx.LOG_EI, fmin=float(yt.min())) as obj:
            lim = np.array([[0.0, 25.0]])
            with pytest.raises(egx.InvalidValueError, match="start point 1"):
                obj.optimize(lim, np.array([[1.0], [np.nan]]))
            with pytest.raises(egx.InvalidValueError, match="lo <= hi"):
                obj.optimize(np.array([[3.0, 1.0]]), np.array([[2.0]]))
            assert np.all(obj.parts(xt)["var"][0] < IO.EPS)
            f, xb, st = obj.optimize(lim, xt, max_eval=1)  # one evaluation each, at a training point: -crit = f64::MAX
            assert f == np.inf and not st["finite"] and xb[0] == 0.0
            np.testing.assert_array_equal(st["evals"], 1)
            assert egx._lib.ERR_NO_FINITE_START == 9  # the documented code behind stats["finite"]
            f2, _, st2 = obj.optimize(lim, np.array([[7.0]]))
            assert np.isfinite(f2) and st2["finite"]


# ---- 6: errors and state --------------------------------------------------------------------------------------------------
def test_errors_and_state(egx):
    x, y = _data(300, 3, seed=51)
    x2, y2 = _data(300, 2, seed=52)
    with egx.GpHandle(x, y) as h, egx.GpHandle(x, y + 1.0) as unfit, egx.GpHandle(x2, y2) as other:
        h.finalize(np.full(3, 1.5))
        other.finalize(np.full(2, 1.5))
        with pytest.raises(egx.NotFittedError, match="model 1"):
            egx.InfillObjective(h, [unfit], [0.0])
        with pytest.raises(egx.InvalidValueError, match="model 1"):
            egx.InfillObjective(h, [other], [0.0])
        with pytest.raises(egx.InvalidValueError):
            egx.InfillObjective(h, [h], [0.0, 1.0])
        with pytest.raises(egx.InvalidValueError):
            egx.InfillObjective(h, criterion=7)
        xq = np.random.default_rng(1).random((20, 3))
        with egx.InfillObjective(h, [h], [0.1], criterion=egx.EI, fmin=float(np.quantile(y, 0.1))) as obj:
            assert obj.value(np.zeros((0, 3))).shape == (0,)
            v, g = obj.value_and_grad(np.zeros((0, 3)))
            assert v.shape == (0,) and g.shape == (0, 3)
            with pytest.raises(egx.InvalidValueError):
                obj.value(np.zeros((2, 4)))
            bad = xq.copy()
            bad[3, 1] = np.nan
            v, g = obj.value_and_grad(bad)
            v0, g0 = obj.value_and_grad(xq)
            assert v[3] == np.inf and np.all(g[3] == 0.0)
            keep = np.arange(20) != 3
            np.testing.assert_array_equal(v[keep], v0[keep])
            np.testing.assert_array_equal(g[keep], g0[keep])
            # set_params
            obj.set_params(fmin=0.0, scale=2.0)
            assert obj.params["fmin"] == 0.0 and obj.params["scale"] == 2.0 and obj.params["sigma_weight"] == 1.0
            with pytest.raises(egx.InvalidValueError):
                obj.set_params(scale=0.0)
            # the model re-finalised at another theta: the next evaluation follows the new state
            h.finalize(np.full(3, 0.7))
            v1, g1 = obj.value_and_grad(xq)
            with egx.InfillObjective(h, [h], [0.1], criterion=egx.EI, fmin=0.0, scale=2.0) as fresh:
                v2, g2 = fresh.value_and_grad(xq)
            np.testing.assert_array_equal(v1, v2)
            np.testing.assert_array_equal(g1, g2)
            assert not np.array_equal(v1, v0)


def test_gaussian_process_and_gpx_are_accepted(egx):
    x, y = _data(200, 2, seed=61)
    gp = egx.GaussianProcess.params(egx.ConstantMean(), egx.SquaredExponentialCorr()) \
        .theta_tuning(egx.ThetaTuning.Fixed(np.full(2, 1.5))).fit(x, y)
    gpx = egx.Gpx.builder(theta_init=np.full(2, 1.5), n_start=-1).fit(x, y)  # one expert, fixed theta
    xq = np.random.default_rng(2).random((5, 2))
    with egx.InfillObjective(gp, criterion=egx.WB2, fmin=float(y.min())) as a, \
            egx.InfillObjective(gp.handle, criterion=egx.WB2, fmin=float(y.min())) as b, \
            egx.InfillObjective(gpx, criterion=egx.WB2, fmin=float(y.min())) as c:
        np.testing.assert_array_equal(a.value(xq), b.value(xq))
        mu = gp.predict(xq)
        np.testing.assert_allclose(a.parts(xq)["mean"][0], np.ravel(mu), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(c.parts(xq)["mean"][0], np.ravel(gpx.predict(xq)), rtol=1e-9, atol=1e-12)

    class TwoExperts(egx.Gpx):  # a mixture with two clusters is refused by name
        def __init__(self, one):
            super().__init__([one, one])
    with pytest.raises(egx.InvalidValueError, match="more than one cluster"):
        egx.InfillObjective(TwoExperts(gp))
    with pytest.raises(egx.InvalidValueError, match="expected a GpHandle"):
        egx.InfillObjective(object())


def test_plain_c_host_drives_the_infill_entry_points(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "infill_driver"
    libdir = os.path.join(root, "egobox_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{os.path.join(root, 'include')}",
                    os.path.join(root, "tests", "c_host", "infill_driver.c"), f"-L{libdir}", "-legx_gp_hip", "-lm",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert out.stdout.startswith("OK"), out.stdout
