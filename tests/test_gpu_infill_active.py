"""Active coordinates on the infill handle (egx_infill_set_active; csrc/infill_active.h, k_xgrad<LIST> in kernels_corr.hip) and
CoEGO on top of them (`Egor(coego_n_coop=k)`).  The contract is bitwise: a compact call returns the full-width call's value at
the expanded rows and that call's listed gradient columns, on every kind of handle.  One case goes against the independent
oracles (oracle.gp_oracle on the handle's fitted state, tests/infill_oracle.py) at the expanded points."""
import numpy as np
import pytest

import infill_oracle as IO
from test_gpu_infill import KINDS, MEANS, PRED_RTOL, _check_criterion, _data
from test_gpu_sample import oracle_from_handle

pytestmark = pytest.mark.gpu

N = 130                      # three 64-row slabs, the last one partial; more than one split of the training range
DIMS = [9, 33, 64, 65, 72]   # both pass widths of k_xgrad with more than one pass; 64 | 65: the LDS image of the queries ends
CHUNKS = (8, 16, 32)         # k_xgrad<LIST>'s pass widths, chosen by the LIST's length: one below, at, one above each
GKEYS = ("grad_mean", "grad_var")


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), what


def _activities(d, rng):
    """shuffled lists of every length where the code takes another path, columns 0 and d - 1 among them; the identity"""
    sizes = sorted({1, d} | {c + o for c in CHUNKS for o in (-1, 0, 1) if c + o <= d})
    acts = [np.array([d - 1])]
    for a in sizes:
        if a == 1:
            acts.append(np.array([0]))
            continue
        inner = rng.permutation(np.arange(1, d - 1))[:a - 2]
        acts.append(rng.permutation(np.concatenate([[0, d - 1], inner])))
    acts.append(np.arange(d))
    return acts


def _expand(xc, act, xb):
    full = np.tile(xb, (xc.shape[0], 1))
    full[:, act] = xc
    return full


def _mean(d, corr, j):
    """the trend of model j: all three kinds at d = 9, constant and linear beyond (a quadratic trend has more columns than N rows)"""
    return (corr + j) % (3 if d == 9 else 2)


def _pair(egx, d, corr, w=None, seed=0):
    """an objective and a constraint model of d inputs on N rows each"""
    hs, xs, ys = [], [], []
    for j in range(2):
        x, y = _data(N, d, seed=seed + 31 * d + j, yscale=1.0 if j else 1e-3)
        if j:
            y = y - np.quantile(y, 0.6)
        h = egx.GpHandle(x, y, mean=_mean(d, corr, j) if w is None else 0, corr=corr, w_star=w)
        h.finalize(np.full(d if w is None else w.shape[1], 1.5 / d if w is None else 0.5))
        hs.append(h), xs.append(x), ys.append(y)
    return hs, xs, ys


def _points(x, m, seed):
    rng = np.random.default_rng(seed)
    lo, hi = x.min(axis=0), x.max(axis=0)
    return lo + (hi - lo) * rng.random((m, x.shape[1]))


def _check_bitwise(obj, act, xb, xc, strategies=("infill",)):
    """everything a compact call returns against the full-width call at the expanded rows"""
    full = _expand(xc, act, xb)
    for strategy in strategies:
        obj.set_cstr_strategy(strategy)
        obj.set_active(act, xb)
        got_act = obj.active
        pc = obj.parts(xc)
        vc = obj.value(xc)
        cc = obj.constraints(xc, grad=True) if strategy != "infill" else None
        obj.clear_active()
        assert obj.active is None
        np.testing.assert_array_equal(got_act[0], act)
        np.testing.assert_array_equal(got_act[1], xb)
        pf = obj.parts(full)
        tag = (strategy, len(act), xc.shape[0])
        _same(pc["value"], pf["value"], tag + ("value",))
        _same(vc, pf["value"], tag + ("value without gradients",))
        _same(pc["mean"], pf["mean"], tag + ("mean",))
        _same(pc["var"], pf["var"], tag + ("var",))
        _same(pc["grad"], pf["grad"][:, act], tag + ("grad",))
        for key in GKEYS:
            _same(pc[key], pf[key][:, :, act], tag + (key,))
        if cc is not None:
            cf = obj.constraints(full, grad=True)
            _same(cc[0], cf[0], tag + ("cstr value",))
            _same(cc[1], cf[1], tag + ("cstr",))
            _same(cc[2], cf[2][:, act], tag + ("cstr grad",))
            _same(cc[3], cf[3][:, :, act], tag + ("grad_cstr",))
    obj.set_cstr_strategy("infill")


# ---- 1. lone dense models: every correlation, every branch of the contraction -------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("corr", range(4))
def test_compact_calls_are_the_full_width_bits(egx, corr, d):
    hs, xs, ys = _pair(egx, d, corr)
    rng = np.random.default_rng(100 * corr + d)
    try:
        with egx.InfillObjective(hs[0], hs[1:], [0.3], criterion=egx.LOG_EI, fmin=float(np.quantile(ys[0], 0.1))) as obj:
            xb = _points(xs[0], 1, seed=d)[0]
            pts = {m: _points(xs[0], m, seed=7 * d + m) for m in (1, 129)}
            before = obj.parts(pts[129])
            for act in _activities(d, rng):
                for m in (1, 129):
                    _check_bitwise(obj, act, xb, pts[m][:, act], strategies=("infill", "mean", "utb"))
            after = obj.parts(pts[129])  # the handle without an activity: as before the first set_active
            for key in ("value", "grad", "mean", "var") + GKEYS:
                _same(after[key], before[key], ("after clear_active", key))
    finally:
        for h in hs:
            h.close()


def test_kpls_model(egx):
    """w_star (9, 2): two coefficient columns per input in the contraction"""
    d = 9
    w = np.random.default_rng(2).standard_normal((d, 2))
    hs, xs, ys = _pair(egx, d, 3, w=w)
    try:
        assert hs[0].h == 2
        with egx.InfillObjective(hs[0], hs[1:], [0.3], criterion=egx.EI, fmin=float(np.quantile(ys[0], 0.1))) as obj:
            xb = _points(xs[0], 1, seed=1)[0]
            for act in (np.array([8, 3, 0]), np.array([4]), np.random.default_rng(3).permutation(d)):
                _check_bitwise(obj, act, xb, _points(xs[0], 129, seed=5)[:, act], strategies=("infill", "utb"))
    finally:
        for h in hs:
            h.close()


# ---- 2. an oracle that is not the code's other path ---------------------------------------------------------------------------
def test_compact_parts_and_criterion_against_the_oracles(egx, O):
    d, a, corr = 33, 7, 0
    hs, xs, ys = _pair(egx, d, corr)
    act = np.concatenate([[d - 1, 0], np.random.default_rng(8).permutation(np.arange(1, d - 1))[:a - 2]])
    try:
        xb = _points(xs[0], 1, seed=3)[0]
        xc = _points(xs[0], 20, seed=4)[:, act]
        full = _expand(xc, act, xb)
        for crit in (IO.EI, IO.LOG_EI, IO.WB2, IO.WB2S):
            with egx.InfillObjective(hs[0], hs[1:], [0.3], criterion=crit, fmin=float(np.quantile(ys[0], 0.1)), sigma_weight=0.75,
                                     scale_ic=2.3, scale=1.7) as obj:
                obj.set_active(act, xb)
                p = obj.parts(xc)
                assert p["grad"].shape == (20, a) and p["grad_mean"].shape == (2, 20, a)
                if crit == IO.EI:  # the parts are the predictions at the EXPANDED points, the gradients their listed columns
                    for j, h in enumerate(hs):
                        ref = oracle_from_handle(O, h, MEANS[_mean(d, corr, j)], KINDS[corr], xs[j], ys[j])
                        ry, rv = ref.predict_valvar(full)
                        gy, gv = ref.predict_valvar_gradients(full)
                        gy, gv = gy[:, act], gv[:, act]
                        np.testing.assert_allclose(p["mean"][j], np.ravel(ry), rtol=PRED_RTOL, atol=1e-9)
                        np.testing.assert_allclose(p["var"][j], np.ravel(rv), rtol=PRED_RTOL, atol=1e-9 * ref.inner.sigma2)
                        np.testing.assert_allclose(p["grad_mean"][j], gy, rtol=PRED_RTOL, atol=PRED_RTOL * np.abs(gy).max())
                        np.testing.assert_allclose(p["grad_var"][j], gv, rtol=PRED_RTOL, atol=PRED_RTOL * np.abs(gv).max())
                # ... and the criterion is the arithmetic of tests/infill_oracle.py on them, column by column
                _check_criterion(obj, p, [0.3])
    finally:
        for h in hs:
            h.close()


# ---- 3. the other kinds of handle ---------------------------------------------------------------------------------------------
def _small_models(egx, d, n=N, corrs=(0, 3, 2)):
    hs, xs, ys = [], [], []
    for j, corr in enumerate(corrs):
        x, y = _data(n - 7 * j, d, seed=40 + j, yscale=1.0 if j == len(corrs) - 1 else 1e-3)
        if j == len(corrs) - 1:
            y = y - np.quantile(y, 0.6)
        h = egx.GpHandle(x, y, mean=j % 2, corr=corr)
        h.finalize(np.full(d, 1.2 + 0.1 * j))
        hs.append(h), xs.append(x), ys.append(y)
    return hs, xs, ys


def test_two_expert_smooth_mixture(egx):
    d = 4
    hs, xs, ys = _small_models(egx, d)
    means = np.full((2, d), 0.5)
    means[:, d - 1] = [0.3, 0.7]
    gmx = egx.GaussianMixture([0.45, 0.55], means, np.stack([np.eye(d) * 0.08, np.eye(d) * 0.06]), 1.0)
    mix = egx.GpMixture([egx.GaussianProcess(h, None) for h in hs[:2]], gmx, "smooth")
    try:
        with egx.InfillObjective(mix, [hs[2]], [0.3], criterion=egx.WB2, fmin=float(np.quantile(ys[0], 0.1))) as obj:
            xb = np.full(d, 0.45)
            for act in (np.array([3, 0]), np.array([2]), np.array([1, 3, 0, 2])):
                _check_bitwise(obj, act, xb, np.random.default_rng(6).random((129, act.shape[0])), strategies=("infill", "mean"))
    finally:
        for h in hs:
            h.close()


def test_sparse_expert(egx):
    d = 3
    rng = np.random.default_rng(12)
    x = rng.random((200, d)) * 2 - 1
    y = np.sin(3 * x[:, 0]) + x[:, 1] * x[:, 2]
    hd, xd, yd = _small_models(egx, d, corrs=(1,))
    try:
        for method in (0, 1):
            with egx.SgpHandle(x, 1e-2 * y, x[:24], corr=0, method=method) as sg:
                sg.finalize(np.array([1.3, 0.8, 1.1]), 0.9, 0.02)
                with egx.InfillObjective(sg, [hd[0]], [0.3], criterion=egx.EI, fmin=-5e-3) as obj:
                    xb = np.array([0.1, -0.3, 0.5])
                    for act in (np.array([2, 0]), np.array([1]), np.array([2, 1, 0])):
                        _check_bitwise(obj, act, xb, rng.random((129, act.shape[0])) * 2 - 1, strategies=("infill", "utb"))
    finally:
        for h in hd:
            h.close()


def test_typed_model_with_an_int_and_an_enum_column(egx):
    """xtypes Float, Int, Enum(3): five unfolded columns; the indices count those and x_base is a raw unfolded row"""
    xt = [egx.XType.Float(0.0, 1.0), egx.XType.Int(0, 3), egx.XType.Enum(3)]
    d = 5
    hs, xs, ys = _small_models(egx, d, corrs=(3, 0))
    try:
        for h in hs:
            h.set_xtypes(xt)
        with egx.InfillObjective(hs[0], hs[1:], [0.3], criterion=egx.LOG_EI, fmin=float(np.quantile(ys[0], 0.1))) as obj:
            xb = np.array([0.37, 1.6, 0.2, 0.7, 0.4])
            rng = np.random.default_rng(13)
            for act in (np.array([1, 4]), np.array([3, 0, 2]), np.array([4, 3, 2, 1, 0])):
                xc = rng.random((129, act.shape[0])) * np.where(act == 1, 3.0, 1.0)
                _check_bitwise(obj, act, xb, xc, strategies=("infill", "mean"))
    finally:
        for h in hs:
            h.close()


def test_two_pending_points(egx):
    d = 9
    hs, xs, ys = _pair(egx, d, 3, seed=5)
    try:
        with egx.InfillObjective(hs[0], hs[1:], [0.3], criterion=egx.EI, fmin=float(np.quantile(ys[0], 0.1))) as obj:
            for v in _points(xs[0], 2, seed=21):
                obj.push_pending(v, obj.virtual_point(v, "kb"))
            assert obj.pending[0].shape[0] == 2
            xb = _points(xs[0], 1, seed=22)[0]
            for act in (np.array([8, 0, 4]), np.array([5]), np.random.default_rng(23).permutation(d)):
                _check_bitwise(obj, act, xb, _points(xs[0], 129, seed=24)[:, act], strategies=("infill", "utb"))
            # the calls that keep width d do not read the activity
            obj.set_active([8, 0, 4], xb)
            assert obj.pending[0].shape == (2, d)
            assert obj.virtual_point(xb, "kb").shape == (2,)
            assert obj.expert_parts(0, xb)["grad_mean"].shape == (1, 1, d)
            obj.scaling(_points(xs[0], 40, seed=25))
    finally:
        for h in hs:
            h.close()


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------
def test_errors_and_state(egx):
    d = 9
    hs, xs, ys = _pair(egx, d, 0, seed=9)
    try:
        with egx.InfillObjective(hs[0], hs[1:], [0.3], criterion=egx.LOG_EI, fmin=float(np.quantile(ys[0], 0.1))) as obj:
            xb = _points(xs[0], 1, seed=1)[0]
            act = np.array([7, 0, 3])
            for bad, needle in (([7, 0, 7], "entry 2 repeats column 7"), ([7, 9], "entry 1 is 9"), ([-1], "entry 0 is -1"),
                                ([], "n_active"), (list(range(d)) + [0], "n_active")):
                with pytest.raises(egx.InvalidValueError, match=needle):
                    obj.set_active(bad, xb)
                assert obj.active is None
            bad_base = xb.copy()
            bad_base[4] = np.inf
            with pytest.raises(egx.InvalidValueError, match="x_base 4"):
                obj.set_active(act, bad_base)
            with pytest.raises(egx.InvalidValueError):
                obj.set_active(act, xb[:-1])
            obj.set_active(act, xb)
            # a refused call leaves the activity the handle had
            with pytest.raises(egx.InvalidValueError):
                obj.set_active([1, 1], xb)
            np.testing.assert_array_equal(obj.active[0], act)
            # a NaN in one compact row: +inf and a zero gradient for that row only
            xc = _points(xs[0], 129, seed=2)[:, act]
            want_v, want_g = obj.value_and_grad(xc)
            xn = xc.copy()
            xn[77, 1] = np.nan
            v, g = obj.value_and_grad(xn)
            assert v[77] == np.inf and np.all(g[77] == 0.0)
            keep = np.arange(129) != 77
            _same(v[keep], want_v[keep], "the other rows' values")
            _same(g[keep], want_g[keep], "the other rows' gradients")
            # a wrong width raises, in every call whose width is the activity's
            lim = np.column_stack([xs[0].min(axis=0), xs[0].max(axis=0)])
            full_pts = _points(xs[0], 3, seed=3)
            for call in (obj.value, obj.value_and_grad, obj.parts):
                with pytest.raises(egx.InvalidValueError):
                    call(full_pts)
            obj.set_cstr_strategy("mean")
            with pytest.raises(egx.InvalidValueError):
                obj.constraints(full_pts)
            for opt in (obj.optimize, obj.optimize_constrained, obj.optimize_slsqp):
                with pytest.raises(egx.InvalidValueError):
                    opt(lim, full_pts[:, act])
                with pytest.raises(egx.InvalidValueError):
                    opt(lim[act], full_pts)
            # the batch call pushes full-width points: unsupported under an activity
            with pytest.raises(egx.EgxError) as err:
                obj.optimize_batch(lim, full_pts[None, :, :], 1)
            assert err.value.rc == egx._lib.ERR_UNSUPPORTED
            obj.clear_active()
            assert obj.value(full_pts).shape == (3,)
    finally:
        for h in hs:
            h.close()


# ---- 5. the optimisers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def opt_case(egx):
    """d = 12, an objective and a constraint model that is satisfied all over the box (the winner's ordering is then the
    objective's alone), six starts"""
    d = 12
    x, y = _data(N, d, seed=77, yscale=1e-3)
    xc_, yc_ = _data(N, d, seed=78)
    hs = [egx.GpHandle(x, y, mean=0, corr=0), egx.GpHandle(xc_, yc_ - (yc_.max() + 3.0 * np.ptp(yc_)), mean=0, corr=0)]
    for h in hs:
        h.finalize(np.full(d, 1.5 / d))
    lim = np.column_stack([x.min(axis=0), x.max(axis=0)])
    starts = _points(x, 6, seed=79)
    starts[0] = lim[:, 1] + 0.5  # outside: clamped into the box
    yield d, hs, lim, starts, float(np.quantile(y, 0.1))
    for h in hs:
        h.close()


def _run(obj, which, lim, starts, max_eval=None):
    """(x, f, c, stats) of the three optimisers in one shape"""
    if which == "cobyla":
        f, x, st = obj.optimize(lim, starts, max_eval)
        return x, f, np.zeros(0), st
    if which == "cobyla_cstr":
        return obj.optimize_constrained(lim, starts, max_eval)
    return obj.optimize_slsqp(lim, starts, max_eval)


OPTIMIZERS = [("cobyla", "infill"), ("cobyla_cstr", "mean"), ("slsqp", "mean"), ("slsqp", "infill")]


@pytest.mark.parametrize("which,strategy", OPTIMIZERS)
def test_identity_activity_walks_the_same_points(egx, opt_case, which, strategy):
    d, hs, lim, starts, fmin = opt_case
    with egx.InfillObjective(hs[0], hs[1:], [0.3], criterion=egx.LOG_EI, fmin=fmin) as obj:
        obj.set_cstr_strategy(strategy)
        x0, f0, c0, s0 = _run(obj, which, lim, starts)
        obj.set_active(np.arange(d), np.zeros(d))
        x1, f1, c1, s1 = _run(obj, which, lim, starts)
    _same(x1, x0, "x_best")
    _same(np.array([f1]), np.array([f0]), "f_best")
    _same(c1, c0, "c_best")
    assert s1["rounds"] == s0["rounds"] and s1["best_start"] == s0["best_start"]
    np.testing.assert_array_equal(s1["evals"], s0["evals"])


@pytest.mark.parametrize("which,strategy", OPTIMIZERS)
def test_optimisers_over_four_shuffled_columns(egx, opt_case, which, strategy):
    d, hs, lim, starts, fmin = opt_case
    act = np.array([11, 4, 0, 7])
    budget = min(10 * 6 * 4, 2000)
    with egx.InfillObjective(hs[0], hs[1:], [0.3], criterion=egx.LOG_EI, fmin=fmin) as obj:
        obj.set_cstr_strategy(strategy)
        xb = _points(np.asarray(lim.T), 1, seed=80)[0]
        obj.set_active(act, xb)
        la, sa = lim[act], starts[:, act]
        x, f, c, st = _run(obj, which, la, sa)
        assert st["finite"] and x.shape == (4,)
        assert np.all(x >= la[:, 0]) and np.all(x <= la[:, 1])
        # f_best and c_best are the evaluation at x_best, bit for bit
        if strategy == "infill":
            _same(obj.value(x), np.array([f]), "f_best")
            assert c.shape == (0,)
        else:
            v, cv = obj.constraints(x)
            _same(v, np.array([f]), "f_best")
            _same(cv[0], c, "c_best")
            assert st["feasible"]
        # every start's first point is the start clamped into the a-wide box: the winner is no worse than any of them
        clamped = np.clip(sa, la[:, 0], la[:, 1])
        assert f <= obj.value(clamped).min()
        assert np.all(st["evals"] >= 1) and np.all(st["evals"] <= budget)
        # a start run alone, with the six starts' budget, walks what it walks among them
        for s in (0, 3):
            alone = _run(obj, which, la, sa[s:s + 1], budget)[3]
            assert alone["evals"][0] == st["evals"][s], (s, alone["evals"], st["evals"])


# ---- 6. Egor(coego_n_coop=...) --------------------------------------------------------------------------------------------------
NX = 8
LIM = np.column_stack([np.full(NX, -2.0), np.full(NX, 2.0)])


def _fun(x):
    """a sphere and one linear constraint, satisfied when negative"""
    x = np.atleast_2d(x)
    return np.column_stack([((x - 0.3) ** 2).sum(axis=1), x.sum(axis=1) - 1.0])


@pytest.fixture(scope="module")
def doe(egx):
    x = egx.Lhs(LIM, "optimized", np.random.default_rng(3)).sample(12)
    return x, _fun(x)


def _egor(egx, **kw):
    return egx.Egor(LIM, gp_config=egx.GpConfig(n_start=4, max_eval=20), n_cstr=1, n_start=6, seed=11, **kw)


def test_coego_suggest_is_reproducible_and_cooperative(egx, doe):
    x, y = doe
    e = _egor(egx, coego_n_coop=3)
    a = e.suggest(x, y)
    trace = [(act.copy(), xc.copy()) for act, xc in e.last_coego_]
    b = _egor(egx, coego_n_coop=3).suggest(x, y)
    _same(a, b, "two suggest calls")
    assert a.shape == (1, NX) and np.all(a >= LIM[:, 0]) and np.all(a <= LIM[:, 1])
    # three groups (3, 3, 2 columns) that partition 0 .. 7; each step moves its own columns only
    assert [len(act) for act, _ in trace] == [3, 3, 2]
    assert sorted(np.concatenate([act for act, _ in trace]).tolist()) == list(range(NX))
    prev = x[egx.egor.find_best_result_index(y, None, e.cstr_tol)]
    for act, xcoop in trace:
        others = np.setdiff1d(np.arange(NX), act)
        _same(xcoop[others], prev[others], "the inactive columns stay")
        prev = xcoop
    _same(a[0], trace[-1][1], "the suggested row is the last xcoop")


def test_coego_minimize(egx, doe):
    x, y = doe
    e = egx.Egor(LIM, gp_config=egx.GpConfig(n_start=4, max_eval=20), n_cstr=1, n_start=6, seed=11, coego_n_coop=3,
                 doe=np.hstack([x, y]))
    res = e.minimize(_fun, max_iters=3)
    assert res.y_doe.shape == (12 + 3, 2) and res.x_doe.shape == (12 + 3, NX)
    assert np.all(np.isfinite(res.y_doe)) and np.all(np.isfinite(res.x_opt)) and np.all(np.isfinite(res.y_opt))
    assert len(e.last_coego_) == 3


def test_coego_off_is_the_loop_without_the_argument(egx, doe):
    x, y = doe
    a = _egor(egx, coego_n_coop=0).suggest(x, y)
    b = _egor(egx).suggest(x, y)
    _same(a, b, "coego_n_coop = 0")
