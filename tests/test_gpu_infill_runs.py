"""Runs of an infill handle (egx_infill_get_runs, csrc/infill_runs.h): consecutive surrogates of one shape go through ONE launch
sequence per tile, the member a grid coordinate of every kernel -- and every output of every entry point is bit for bit what the
same surrogates give one by one.

The model: an objective and 4 constraints, n = 150 (n_pad 256), d = 5, fitted at a fixed theta as ONE GROUP (fit_group), whose
full-sequence launches form the run [5]; and the same data and theta fitted as five SEPARATE handles -- finalize_multi guarantees
the same model bits -- which can only form mean-only runs: [1, 1, 1, 1, 1] under "infill" / "utb", [1, 4] under "mean".  Every
comparison between the two handles is np.array_equal; where both form the same runs (the mean-only run of "mean"), the separate
handle's full sequence (`parts`, which asks for the variances) is the reference with runs of one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, K = 150, 5, 4
THETA = 1.0
MS = (20, 130)  # one tile; two tiles, the last partial
CRITERIA = ("EI", "LOG_EI", "WB2", "WB2S")
STRATEGIES = ("infill", "mean", "utb")
RUNS_GROUP = {"infill": [5], "mean": [1, 4], "utb": [5]}
RUNS_SEPARATE = {"infill": [1] * 5, "mean": [1, 4], "utb": [1] * 5}


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


def _sets(k, n, d, seed):
    from egobox_amd import workload
    xy = [workload.make_training_set(n, d, seed=seed + j) for j in range(k)]
    return np.stack([x for x, _ in xy]), np.stack([np.asarray(y).reshape(-1) for _, y in xy])


def _params(egx, d, mean=None, theta=THETA):
    return egx.GaussianProcess.params(mean or egx.ConstantMean(), egx.SquaredExponentialCorr()) \
        .theta_tuning(egx.ThetaTuning.Fixed(np.full(d, theta)))


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


@pytest.fixture(scope="module")
def models(egx):
    """(group members, separate handles, xs, ys) -- the same five models twice"""
    xs, ys = _sets(1 + K, N, D, seed=700)
    group = _params(egx, D).fit_group(xs, ys)
    separate = [_params(egx, D).fit(xs[j], ys[j]) for j in range(1 + K)]
    for g, s in zip(group, separate):  # the premise of every comparison below
        assert np.array_equal(g.predict(xs[0][:9]), s.predict(xs[0][:9]))
    yield group, separate, xs, ys
    for g in group + separate:
        g.close()


def _pair(egx, models, criterion, strategy="infill"):
    group, separate, xs, ys = models
    out = []
    for ms in (group, separate):
        o = egx.InfillObjective(ms[0], ms[1:], np.zeros(K), criterion=getattr(egx, criterion), fmin=float(np.quantile(ys[0], 0.5)))
        if strategy != "infill":
            o.set_cstr_strategy(strategy)
        out.append(o)
    return out


def _points(m, d=D, seed=0):
    return np.random.default_rng(seed + m).random((m, d))


def _same(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for key in a:
            _same(a[key], b[key], f"{what}[{key}]")
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (u, v) in enumerate(zip(a, b)):
            _same(u, v, f"{what}[{i}]")
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), what


def _all_outputs(o, x, strategy):
    out = dict(value=o.value(x), value_and_grad=o.value_and_grad(x), parts=o.parts(x))
    if strategy != "infill":
        out["constraints"] = o.constraints(x)
        out["constraints_grad"] = o.constraints(x, grad=True)
    return out


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("criterion", CRITERIA)
def test_group_equals_separate(egx, models, criterion, strategy):
    og, osep = _pair(egx, models, criterion, strategy)
    try:
        assert og.runs == RUNS_GROUP[strategy] and osep.runs == RUNS_SEPARATE[strategy]
        for m in MS:
            x = _points(m)
            a, b = _all_outputs(og, x, strategy), _all_outputs(osep, x, strategy)
            _same(a, b, f"{criterion} {strategy} m={m}")
            assert np.all(np.isfinite(a["parts"]["mean"])) and np.all(np.isfinite(a["value_and_grad"][1]))
            # without gradients and with them: the same values
            assert np.array_equal(a["value"], a["value_and_grad"][0])
            if strategy == "mean":
                # the mean-only run [1, 4] (both handles) against the separate handle's full sequence, which forms no run:
                # cstr = mean / scale_cstr with scale_cstr = 1
                _, cstr, _, gcstr = a["constraints_grad"]
                assert np.array_equal(cstr, b["parts"]["mean"][1:].T)
                assert np.array_equal(gcstr, np.transpose(b["parts"]["grad_mean"][1:], (1, 0, 2)))
        _same(og.scaling(_points(60, seed=5)), osep.scaling(_points(60, seed=5)), "scaling")
        assert og.runs == RUNS_GROUP[strategy]
    finally:
        og.close(), osep.close()


def test_active_coordinates(egx, models):
    og, osep = _pair(egx, models, "LOG_EI", "utb")
    try:
        base = np.full(D, 0.4)
        for o in (og, osep):
            o.set_active([3, 1], base)
        assert og.runs == [5] and osep.runs == [1] * 5
        x = _points(130, d=2)
        _same(_all_outputs(og, x, "utb"), _all_outputs(osep, x, "utb"), "active")
        full = np.tile(base, (130, 1))
        full[:, [3, 1]] = x
        og.clear_active()
        v, g = og.value_and_grad(full)
        og.set_active([3, 1], base)
        va, ga = og.value_and_grad(x)
        assert np.array_equal(v, va) and np.array_equal(g[:, [3, 1]], ga)
    finally:
        og.close(), osep.close()


def test_int_column_on_every_model(egx, models):
    group, separate, xs, ys = models
    xt = [egx.XType.Float(0.0, 1.0)] * (D - 1) + [egx.XType.Int(0, 1)]
    try:
        for g in group + separate:
            g.set_xtypes(xt)
        for strategy in ("infill", "mean"):
            og, osep = _pair(egx, models, "WB2", strategy)
            try:
                assert og.runs == RUNS_GROUP[strategy]
                x = _points(130, seed=3)
                a = _all_outputs(og, x, strategy)
                _same(a, _all_outputs(osep, x, strategy), "typed " + strategy)
                xc = x.copy()
                xc[:, D - 1] = np.rint(xc[:, D - 1])  # the cast point gives the same values
                assert np.array_equal(a["value"], og.value(xc))
            finally:
                og.close(), osep.close()
    finally:
        for g in group + separate:
            g.set_xtypes(None)


def test_one_pending_point_walks_runs_of_one(egx, O, models):
    """With a pending point every run has length 1 on both handles; the conditioned parts are those of the frozen refit, as
    tests/test_gpu_infill_pending.py computes them (its bars), and clear_pending gives the runs and the bits back."""
    import types

    from pending_cases import _check_parts_against_refit, gate
    from test_gpu_sample import oracle_from_handle
    group, _, xs, ys = models
    og, osep = _pair(egx, models, "EI", "infill")
    try:
        x = _points(130, seed=9)
        before = _all_outputs(og, x, "infill")
        xp = np.full(D, 0.3)
        yp = og.virtual_point(xp)
        _same(yp, osep.virtual_point(xp), "virtual point")
        og.push_pending(xp, yp), osep.push_pending(xp, yp)
        assert og.runs == [1] * 5 and osep.runs == [1] * 5
        cond = _all_outputs(og, x, "infill")
        _same(cond, _all_outputs(osep, x, "infill"), "pending")
        # the conditioning moved the variances down and nothing to NaN
        assert np.all(cond["parts"]["var"] <= before["parts"]["var"] * (1 + 1e-9) + 1e-12) and np.all(np.isfinite(cond["value"]))
        assert not np.array_equal(cond["parts"]["var"], before["parts"]["var"])
        c = types.SimpleNamespace(xv=xp[None, :], yv=np.asarray(yp)[None, :], gs=[
            oracle_from_handle(O, g._h, "Constant", "SquaredExponential", xs[j], ys[j]) for j, g in enumerate(group)])
        rows = x[:40]
        min_diag, min_unit, ok = gate(c.gs[0], c.xv, rows)
        print(f"min diag S {min_diag:.3g}, min conditioned unit variance {min_unit:.3g}")
        assert ok
        p40 = og.parts(rows)
        assert np.array_equal(p40["var"], cond["parts"]["var"][:, :40])  # a point does not depend on its companions
        _check_parts_against_refit(c, p40, rows, og.pending[2])
        og.clear_pending(), osep.clear_pending()
        assert og.runs == [5]
        _same(_all_outputs(og, x, "infill"), before, "after clear_pending")
    finally:
        og.close(), osep.close()


def test_seventeen_mean_only_constraints(egx):
    """n = 70, d = 2, separate handles: [1, 16, 1] under "mean"; the full sequence of the same handle ([1] * 18) is the reference."""
    k, n, d = 17, 70, 2
    xs, ys = _sets(1 + k, n, d, seed=900)
    gps = [_params(egx, d, theta=5.0).fit(xs[j], ys[j]) for j in range(1 + k)]
    o = egx.InfillObjective(gps[0], gps[1:], np.zeros(k), criterion=egx.EI, fmin=float(ys[0].min()))
    try:
        assert o.runs == [1] * 18
        o.set_cstr_strategy("mean")
        assert o.runs == [1, 16, 1]
        for m in MS:
            x = _points(m, d=d)
            value, cstr, grad, gcstr = o.constraints(x, grad=True)
            p = o.parts(x)  # asks for the variances: the full sequence, runs of one
            assert np.array_equal(cstr, p["mean"][1:].T)
            assert np.array_equal(gcstr, np.transpose(p["grad_mean"][1:], (1, 0, 2)))
            _same(o.constraints(x), (value, cstr), "without gradients")
            for j in (0, 15, 16):  # first and last member of the long run, the run behind it
                np.testing.assert_allclose(cstr[:, j], gps[1 + j].predict(x).reshape(-1), rtol=1e-9, atol=1e-12)
    finally:
        o.close()
        for g in gps:
            g.close()


def test_unequal_n_forms_no_run(egx):
    d = 3
    sizes = [60, 61, 130, 60]  # n_pad 128, 128, 256, 128: no two neighbours of one shape
    gps = []
    for j, n in enumerate(sizes):
        x, y = _sets(1, n, d, seed=950 + j)
        gps.append(_params(egx, d, theta=2.0).fit(x[0], y[0]))
    o = egx.InfillObjective(gps[0], gps[1:], np.zeros(3), criterion=egx.WB2)
    try:
        o.set_cstr_strategy("mean")
        assert o.runs == [1, 1, 1, 1]
        x = _points(130, d=d)
        _, cstr, _, gcstr = o.constraints(x, grad=True)
        p = o.parts(x)
        assert np.array_equal(cstr, p["mean"][1:].T)
        assert np.array_equal(gcstr, np.transpose(p["grad_mean"][1:], (1, 0, 2)))
    finally:
        o.close()
        for g in gps:
            g.close()


@pytest.mark.parametrize("strategy", ("infill", "utb"))
def test_slsqp_from_the_same_starts(egx, models, strategy):
    og, osep = _pair(egx, models, "LOG_EI", strategy)
    try:
        lim = np.tile([0.0, 1.0], (D, 1))
        starts = _points(6, seed=21)
        _same(og.optimize_slsqp(lim, starts, max_eval=40), osep.optimize_slsqp(lim, starts, max_eval=40), "slsqp " + strategy)
    finally:
        og.close(), osep.close()


def test_cobyla_constrained_from_the_same_starts(egx, models):
    og, osep = _pair(egx, models, "WB2", "utb")
    try:
        lim = np.tile([0.0, 1.0], (D, 1))
        starts = _points(4, seed=22)
        _same(og.optimize_constrained(lim, starts, max_eval=60), osep.optimize_constrained(lim, starts, max_eval=60), "cobyla")
    finally:
        og.close(), osep.close()
