"""Mixed-integer surrogates on the GPU (egx_gp_set_xtypes; the typed k_normalize_queries, k_infill_prepare_mixint and
k_gmx_probas_mixint): every entry point that takes query points, called on RAW points x by a model that carries xtypes, returns
bit for bit what the same model without xtypes returns on tests/mixint_oracle.py's cast(x) -- and something else than the
untyped model on the uncast x, so a cast that does nothing fails.  Two specs (the reference's, d = 6, and one with d = 70 whose
Enum group straddles the kernels' 64-dimension chunk), slab and tile edges, ties, non-finite points, groups, mixtures, the infill
handles and their optimisers, and the reference's one-dimensional known answer."""
import json
import os

import numpy as np
import pytest

import mixint_oracle as MO

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = {"A": MO.SPEC_A, "B": MO.SPEC_B}
MS = (1, 63, 64, 65, 128, 129, 300)
#: (spec, mean, corr): Constant / Linear / Quadratic, squared exponential (0) / Matern 5/2 (3); the Quadratic trend of d = 70 has
#: 2556 columns, more than a training set of <= 200 points carries
MODELS = [("A", 0, 0), ("A", 1, 3), ("A", 2, 0), ("A", 2, 3), ("B", 0, 3), ("B", 1, 0)]
N_TRAIN = {"A": 120, "B": 160}
THETA = {"A": 0.35, "B": 0.02}


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


def _eq(a, b):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


def _training(name, seed, shift=0.0, relaxed=False):
    """training inputs in the spec's limits and a smooth response.  Admissible (cast) ones, except `relaxed`: the one-hot columns
    of an Enum group add up to the constant column of a Linear or Quadratic trend, whose F is then rank deficient and refused
    (as in the reference); the models with such a trend are trained on the relaxed points -- the handle takes its training
    inputs as they come, and what is under test is the cast of the QUERIES."""
    spec = SPECS[name]
    rng = np.random.default_rng(seed)
    lim = MO.as_continuous_limits(spec)
    x = lim[:, 0] + (lim[:, 1] - lim[:, 0]) * rng.random((N_TRAIN[name], lim.shape[0]))
    if not relaxed:
        x = MO.cast(spec, x)
    z = (x - lim[:, 0]) / (lim[:, 1] - lim[:, 0])
    w = np.cos(np.arange(z.shape[1]) + seed)
    y = np.sin(z @ w / np.sqrt(z.shape[1]) * 3.0) + 0.3 * z[:, 0] ** 2 + 0.2 * z[:, -1] + shift
    return x, y


def _handle(egx, name, mean, corr, seed=3, shift=0.0):
    x, y = _training(name, seed, shift, relaxed=mean >= 1)
    h = egx.GpHandle(x, y, mean=mean, corr=corr)
    h.finalize(np.full(x.shape[1], THETA[name] * (1.0 + 0.1 * (seed % 3))))
    # builds the cached C^-T: from now on a call of <= 8 points takes the few-query path whatever came before it (without the
    # cache the first two such calls after a fit take the batched path, whose variance differs in the last bits)
    h.predict_var_gradients(x[:2])
    return h


_CACHE = {}


def _model(egx, name, mean, corr):
    key = (name, mean, corr)
    if key not in _CACHE:
        _CACHE[key] = _handle(egx, name, mean, corr)
    return _CACHE[key]


def _three_ways(egx, h, name, fn, x):
    """fn(handle, points) by the untyped model on x, by the typed model on x, by the model with its xtypes cleared on cast(x) and
    on x again: (raw, typed, on_cast, raw_again)"""
    spec = SPECS[name]
    raw = fn(h, x)
    h.set_xtypes(MO.xtypes(egx, spec))
    try:
        assert h.xtypes == MO.xtypes(egx, spec)
        typed = fn(h, x)
    finally:
        h.set_xtypes(None)
    assert h.xtypes == []
    return raw, typed, fn(h, MO.cast(spec, x)), fn(h, x)


def _check(egx, h, name, fn, x):
    raw, typed, on_cast, again = _three_ways(egx, h, name, fn, x)
    for r, t, c, a in zip(raw, typed, on_cast, again):
        _eq(t, c)                              # the cast, bit for bit
        _eq(a, r)                              # cleared: the untyped bits again
        assert not np.array_equal(t, r)        # ... which are not those of the cast point


# ---- predictions and gradients: batched and few-query paths, slab and tile edges ----------------------------------------------
@gpu
@pytest.mark.parametrize("name, mean, corr", MODELS)
def test_predictions_and_gradients_are_those_of_the_cast_point(egx, name, mean, corr):
    h = _model(egx, name, mean, corr)
    for m in MS:
        x = MO.queries(SPECS[name], m, seed=100 + m)
        _check(egx, h, name, lambda g, q: (g.predict(q), g.predict_var(q)) + g.predict_valvar(q), x)
        _check(egx, h, name, lambda g, q: (g.predict_gradients(q), g.predict_var_gradients(q)) + g.predict_valvar_gradients(q), x)
    x = MO.queries(SPECS[name], 5, seed=7)  # the few-query paths with more than one point
    _check(egx, h, name, lambda g, q: g.predict_valvar(q) + g.predict_valvar_gradients(q), x)


@gpu
@pytest.mark.parametrize("name, mean, corr", [("A", 1, 3), ("B", 0, 3)])
def test_covariance_and_samples(egx, name, mean, corr):
    h = _model(egx, name, mean, corr)
    x = MO.queries(SPECS[name], 65, seed=11)
    z = np.random.default_rng(5).standard_normal((65, 3))
    _check(egx, h, name, lambda g, q: (g.predict_covariance(q), g.sample(q, 3, method="psd", z=z), g.sample(q, 3, method="psd", seed=9)), x)


@gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_non_finite_points_stay_non_finite_and_leave_their_neighbours_alone(egx, name):
    spec, h = SPECS[name], _model(egx, name, 1 if name == "B" else 2, 0)
    x = MO.queries(spec, 70, seed=21)
    clean = x.copy()
    enum0, u = None, 0
    for t in spec:  # the first unfolded column of the Enum group
        if t[0] == "enum":
            enum0 = u
            break
        u += 1
    bad = {2: (0, np.nan), 63: (enum0 + 1, np.nan), 64: (x.shape[1] - 1, np.inf), 69: (enum0, np.nan)}
    for r, (c, v) in bad.items():
        x[r, c] = v
    fn = lambda g, q: g.predict_valvar(q) + g.predict_valvar_gradients(q)  # noqa: E731
    raw, typed, on_cast, again = _three_ways(egx, h, name, fn, x)
    h.set_xtypes(MO.xtypes(egx, spec))
    try:
        typed_clean = fn(h, clean)
    finally:
        h.set_xtypes(None)
    keep = np.array([r not in bad for r in range(70)])
    for t, c, tc in zip(typed, on_cast, typed_clean):
        _eq(t, c)
        assert np.isnan(t[[2, 63, 69]]).all()  # NaN in, NaN out (the +inf row 64: whatever the untyped model gives, above)
        _eq(t[keep], tc[keep])


@gpu
def test_group_with_one_typed_and_one_untyped_member(egx):
    name = "A"
    spec = SPECS[name]
    sets = [_training(name, 3, relaxed=True), _training(name, 4, relaxed=True)]
    hs = egx.GpHandle.create_group(np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets]), mean=1, corr=0)
    egx.finalize_multi(hs, np.full((2, 6), THETA[name]))
    for m in (65, 300):
        x = MO.queries(spec, m, seed=31)
        xqs = np.stack([x, x])
        y0, v0 = egx.predict_valvar_multi(hs, xqs)
        yc, vc = egx.predict_valvar_multi(hs, np.stack([MO.cast(spec, x), x]))
        hs[0].set_xtypes(MO.xtypes(egx, spec))
        try:
            y1, v1 = egx.predict_valvar_multi(hs, xqs)
        finally:
            hs[0].set_xtypes(None)
        _eq(y1, yc), _eq(v1, vc)
        _eq(y1[1], y0[1]), _eq(v1[1], v0[1])
        assert not np.array_equal(y1[0], y0[0])
        y2, v2 = egx.predict_valvar_multi(hs, xqs)
        _eq(y2, y0), _eq(v2, v0)


@gpu
def test_set_xtypes_refuses_a_spec_of_another_dimension(egx):
    from egobox_amd import _lib as L
    h = _model(egx, "A", 0, 0)
    with pytest.raises(L.InvalidValueError, match="unfold to 70 columns, expected 6"):
        h.set_xtypes(MO.xtypes(egx, MO.SPEC_B))
    with pytest.raises(L.InvalidValueError, match="xtype 1"):
        h.set_xtypes([egx.XType.Float(0, 1), egx.XType.Ord([1.0, np.nan]), egx.XType.Enum(4)])
    assert h.xtypes == []


# ---- mixtures ---------------------------------------------------------------------------------------------------------------
def _gmx(egx, name, k, hf=0.9):
    """k overlapping clusters along the first (Float / Int) column and across the Enum group, in the spec's own units"""
    lim = MO.as_continuous_limits(SPECS[name])
    mid, w = lim.mean(axis=1), lim[:, 1] - lim[:, 0]
    means = np.tile(mid, (k, 1))
    means[:, 0] = mid[0] + w[0] * np.linspace(-0.25, 0.25, k)
    means[:, -1] = mid[-1] + w[-1] * np.linspace(0.2, -0.2, k)
    covs = np.stack([np.diag((w * (0.45 + 0.05 * c)) ** 2) for c in range(k)])
    return egx.GaussianMixture(np.full(k, 1.0 / k), means, covs, hf)


def _mixture(egx, name, k, mode):
    gps = [egx.GaussianProcess(_handle(egx, name, e % 2, (0, 3, 0)[e], seed=3 + e), None) for e in range(k)]
    return egx.GpMixture(gps, _gmx(egx, name, k), mode)


def _typed_mix(egx, mix, name):
    return egx.MixintGpMixture(mix, MO.xtypes(egx, SPECS[name]))


def _clear_mix(mix):
    for e in mix.experts:
        e.set_xtypes(None)
    mix.xtypes = None


@gpu
@pytest.mark.parametrize("name, k, mode", [("A", 2, "smooth"), ("A", 3, "hard"), ("B", 3, "smooth"), ("B", 2, "hard")])
def test_mixture_predictions_take_the_cast_point(egx, name, k, mode):
    spec = SPECS[name]
    mix = _mixture(egx, name, k, mode)
    x = MO.queries(spec, 129, seed=41)
    fn = lambda mm, q: mm.predict_valvar(q) + mm.predict_valvar_gradients(q)  # noqa: E731
    raw = fn(mix, x)
    gm = mix.gmx
    p_raw, p_cast = gm.predict_probas_device(x), gm.predict_probas_device(MO.cast(spec, x))
    _eq(gm.predict_probas_device(x, xtypes=MO.xtypes(egx, spec)), p_cast)
    _eq(gm.predict_probas_derivatives_device(x, xtypes=MO.xtypes(egx, spec)), gm.predict_probas_derivatives_device(MO.cast(spec, x)))
    assert not np.array_equal(p_raw, p_cast)
    typed_model = _typed_mix(egx, mix, name)
    assert typed_model.dims == (MO.unfolded_dim(spec), 1) and typed_model.xtypes == MO.xtypes(egx, spec)
    try:
        typed = (typed_model.predict(x), typed_model.predict_var(x), typed_model.predict_gradients(x), typed_model.predict_var_gradients(x))
    finally:
        _clear_mix(mix)
    on_cast, again = fn(mix, MO.cast(spec, x)), fn(mix, x)
    for r, t, c, a in zip(raw, typed, on_cast, again):
        _eq(t, c), _eq(a, r)
        assert not np.array_equal(t, r)


@gpu
def test_folded_space_surrogate_unfolds_on_the_host(egx):
    """work_in_folded_space: the user's columns in, validated enum indices, the device path behind them"""
    from egobox_amd import _lib as L
    spec, xt = MO.SPEC_A, MO.xtypes(egx, MO.SPEC_A)
    xu, y = _training("A", 3)
    xf = MO.fold(spec, xu)
    tun = egx.ThetaTuning.Fixed(np.full(6, THETA["A"]))
    model = egx.MixintGpMixtureParams(xt, egx.GpMixtureParams().theta_tunings([tun])).work_in_folded_space(True).fit(xf, y)
    assert model.dims == (4, 1)
    q = MO.queries(spec, 65, seed=51)
    qf = MO.fold(spec, q)                       # raw Float / Int / Ord coordinates, an enum index
    got = model.predict_valvar(qf)
    _clear_mix(model.moe)
    want = model.moe.predict_valvar(MO.cast(spec, MO.unfold(spec, qf)))
    for g, w in zip(got, want):
        _eq(g, w)
    np.testing.assert_allclose(model.moe.predict(xu), y, atol=1e-6)  # it interpolates its (cast) training points
    with pytest.raises(L.InvalidValueError, match="xtype 1"):
        model.predict([[0.0, 3.0, 1.0, 1.0]])


# ---- infill handles -----------------------------------------------------------------------------------------------------------
def _typed(egx, handles, name, on):
    for h in handles:
        h.set_xtypes(MO.xtypes(egx, SPECS[name]) if on else None)


def _infill_outputs(obj, x, strategy, mix):
    obj.set_cstr_strategy(strategy)
    out = []
    p = obj.parts(x)
    out += [p[k] for k in ("value", "grad", "mean", "var", "grad_mean", "grad_var")]
    out.append(obj.value(x))
    if strategy != "infill":  # (a handle that folds its constraints into the objective hands none to an optimiser)
        out += list(obj.constraints(x, grad=True))
    if mix:
        for j in (0, 1):
            e = obj.expert_parts(j, x)
            out += [e[k] for k in ("mean", "var", "grad_mean", "grad_var", "probas", "dprobas")]
    return out


@gpu
@pytest.mark.parametrize("name, mix", [("A", False), ("B", False), ("A", True), ("B", True)])
def test_infill_evaluations_take_the_cast_point(egx, name, mix):
    spec = SPECS[name]
    if mix:
        objm, cm = _mixture(egx, name, 3, "smooth"), _mixture(egx, name, 2, "hard")
        handles = [e.handle for e in objm.experts + cm.experts]
    else:
        objm, cm = _handle(egx, name, 1, 0, seed=3), _handle(egx, name, 0, 3, seed=4, shift=-0.4)
        handles = [objm, cm]
    y0 = handles[0].training_data[1]
    obj = egx.InfillObjective(objm, [cm], [0.1], criterion=egx.WB2S, fmin=float(np.quantile(y0, 0.1)))
    for m in ((1, 128, 129) if name == "A" else (129,)):
        x = MO.queries(spec, m, seed=61 + m)
        if m > 1:
            x[m // 2, 0] = np.nan  # a non-finite point: +inf, zero gradient, whatever the cast
        for strategy in ("infill", "mean", "utb"):
            raw = _infill_outputs(obj, x, strategy, mix)
            _typed(egx, handles, name, True)
            if mix:
                objm.xtypes = cm.xtypes = MO.xtypes(egx, spec)
            try:
                typed = _infill_outputs(obj, x, strategy, mix)
            finally:
                _typed(egx, handles, name, False)
                if mix:
                    objm.xtypes = cm.xtypes = None
            on_cast, again = _infill_outputs(obj, MO.cast(spec, x), strategy, mix), _infill_outputs(obj, x, strategy, mix)
            differs = 0
            for r, t, c, a in zip(raw, typed, on_cast, again):
                _eq(t, c), _eq(a, r)
                differs += not np.array_equal(t, r)
            assert differs >= len(raw) - 2, differs
            assert m == 1 or (typed[0][m // 2] == np.inf and not typed[1][m // 2].any())
    # scaling reads the points through the same sequence
    pts = MO.queries(spec, 40, seed=71)
    _typed(egx, handles, name, True)
    try:
        s_typed = obj.scaling(pts)
    finally:
        _typed(egx, handles, name, False)
    s_cast, s_raw = obj.scaling(MO.cast(spec, pts)), obj.scaling(pts)
    assert s_typed[:2] == s_cast[:2]
    _eq(s_typed[2], s_cast[2])
    assert s_typed[:2] != s_raw[:2] or not np.array_equal(s_typed[2], s_raw[2])


@gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_infill_optimisers_return_evaluated_admissible_points(egx, name):
    spec, xt = SPECS[name], MO.xtypes(egx, SPECS[name])
    objm, cm = _handle(egx, name, 1, 0, seed=3), _handle(egx, name, 0, 3, seed=4, shift=-0.4)
    _typed(egx, [objm, cm], name, True)
    y0 = objm.training_data[1]
    obj = egx.InfillObjective(objm, [cm], [0.1], criterion=egx.WB2, fmin=float(np.quantile(y0, 0.1)))
    lim = egx.as_continuous_limits(xt)
    starts = lim[:, 0] + (lim[:, 1] - lim[:, 0]) * np.random.default_rng(81).random((4, lim.shape[0]))
    budget = 4 * lim.shape[0] + 40
    f, xb, stats = obj.optimize(lim, starts, max_eval=budget)
    assert stats["finite"] and np.all(stats["evals"] > 0)
    assert f == obj.value(xb)[0]                                   # bit for bit the evaluation at x_best ...
    assert f == obj.value(egx.cast_to_discrete_values(xt, xb))[0]  # ... which is the one at its cast
    disc = egx.to_discrete_space(xt, xb)                           # the caller folds x_best (egor.rs:289)
    _eq(disc, MO.to_discrete(spec, xb))
    _eq(egx.to_discrete_space(xt, egx.to_continuous_space(xt, disc)), disc)
    obj.set_cstr_strategy("mean")
    xc, fc, cc, st = obj.optimize_constrained(lim, starts, max_eval=budget)
    v, c = obj.constraints(xc)
    assert fc == v[0] and np.array_equal(cc, c[0])
    _eq(egx.to_discrete_space(xt, xc), MO.to_discrete(spec, xc))


@gpu
def test_infill_refuses_models_with_different_xtypes(egx):
    from egobox_amd import _lib as L
    objm, cm = _handle(egx, "A", 0, 0, seed=3), _handle(egx, "A", 0, 3, seed=4)
    objm.set_xtypes(MO.xtypes(egx, MO.SPEC_A))
    with pytest.raises(L.InvalidValueError, match="model 1 and model 0 carry different xtypes"):
        egx.InfillObjective(objm, [cm], [0.0])
    other = list(MO.SPEC_A)
    other[3] = ("ord", [1.0, 3.0, 5.0, 9.0])
    cm.set_xtypes(MO.xtypes(egx, other))
    with pytest.raises(L.InvalidValueError, match="model 1"):
        egx.InfillObjective(objm, [cm], [0.0])
    cm.set_xtypes(MO.xtypes(egx, MO.SPEC_A))
    obj = egx.InfillObjective(objm, [cm], [0.0])
    cm.set_xtypes(None)  # the spec is read at every call
    with pytest.raises(L.InvalidValueError, match="model 1"):
        obj.value(np.zeros((1, 6)))
    mixo = _mixture(egx, "A", 2, "smooth")
    mixo.experts[1].set_xtypes(MO.xtypes(egx, MO.SPEC_A))
    with pytest.raises(L.InvalidValueError, match="surrogate 0 expert 1"):
        egx.InfillObjective(mixo, [], [])


# ---- the reference's known answer ---------------------------------------------------------------------------------------------
@gpu
def test_reference_moe_1d(egx):
    """test_mixint_moe_1d (mixint.rs:968-998): Int(0, 4), four training points, predictions and variances at linspace(0, 4, 5)"""
    with open(os.path.join(ROOT, "tests", "golden", "mixint_kat.json")) as f:
        k = json.load(f)["moe_1d"]
    xt = MO.xtypes(egx, [tuple(t) for t in k["spec"]])
    model = egx.MixintContext(xt).create_surrogate(egx.GpMixtureParams(), np.array(k["xt"]), np.array(k["yt"]))
    xtest = np.array(k["xtest"])[:, None]
    y, v = model.predict(xtest), model.predict_var(xtest)
    print("moe_1d predictions", y, "variances", v)
    np.testing.assert_allclose(y, k["ytest"], rtol=0, atol=k["epsilon"])
    np.testing.assert_allclose(v, k["yvar"], rtol=0, atol=k["epsilon"])
    both = np.array([[0.4], [1.6], [2.5], [0.0], [2.0], [3.0]])  # (one call: the same path for the six points)
    y2, v2 = model.predict(both), model.predict_var(both)
    _eq(y2[:3], y2[3:]), _eq(v2[:3], v2[3:])
    assert not np.array_equal(y2[:3], model.moe.experts[0].handle.set_xtypes(None).predict(both[:3]))
