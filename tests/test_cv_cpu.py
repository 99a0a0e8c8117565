"""The host side of the cross-validation engine (egobox_amd/cv.py) without a GPU: fold layout, the GpMetrics formulas on a
duck-typed stub surrogate against values worked out by hand, find_best_expert's table rules with stub fits, and the argument
validation of predict_valvar_multi."""
import math
from statistics import NormalDist

import numpy as np
import pytest

import cv_oracle as CO


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


# ------------------------------------------------------------------ fold layout
def test_fold_layout(egx):
    folds = egx.fold_indices(23, 5)
    assert len(folds) == 5
    for i, (tr, va) in enumerate(folds):
        assert va.tolist() == list(range(4 * i, 4 * i + 4))          # fold_size 4: disjoint, consecutive chunks
        assert tr.size == 19 and {20, 21, 22} <= set(tr.tolist())    # the leftover rows are in every training set
        assert not set(tr.tolist()) & set(va.tolist())
        assert tr.tolist() == sorted(tr.tolist())                    # original row order minus the chunk
    for (tr, va), (tr_o, va_o) in zip(folds, CO.folds(23, 5)):
        np.testing.assert_array_equal(tr, tr_o)
        np.testing.assert_array_equal(va, va_o)
    loo = egx.fold_indices(7, 7)
    assert [va.tolist() for _, va in loo] == [[i] for i in range(7)]
    assert all(tr.size == 6 for tr, _ in loo)
    with pytest.raises(egx.InvalidValueError):
        egx.fold_indices(5, 6)
    with pytest.raises(egx.InvalidValueError):
        egx.fold_indices(5, 0)


# ------------------------------------------------------------------ metric formulas on a stub surrogate
class _StubModel:
    """Closed-form 'fit': predicts the training mean plus x / 2, variance 1/4 + x^2."""

    def __init__(self, x, y):
        self.c = float(np.mean(y))
        self.closed = False

    def predict(self, x):
        return self.c + 0.5 * x[:, 0]

    def predict_valvar(self, x):
        return self.predict(x), 0.25 + x[:, 0] ** 2

    def close(self):
        self.closed = True


def _stub_surrogate(egx, x, y, fit=_StubModel):
    class Stub(egx.GpMetrics):
        def _cv_targets(self):
            return y

        def _cv_folds(self, kfold, want_var):
            return egx.cv.cross_validate_surrogates(fit, x, y, kfold, want_var)
    return Stub()


def test_metric_formulas_by_hand(egx):
    n, k = 11, 3  # fold_size 3, rows 9 and 10 in every training set
    x = np.linspace(-1.0, 1.5, n).reshape(-1, 1)
    y = np.sin(3.0 * x[:, 0]) + x[:, 0]
    y_mean = sum(y) / n
    press = tss = varss = 0.0
    cnt = 0
    for i in range(k):
        valid = [3 * i, 3 * i + 1, 3 * i + 2]
        train = [r for r in range(n) if r not in valid]
        c = sum(y[r] for r in train) / len(train)
        for r in valid:
            pred, var = c + 0.5 * x[r, 0], 0.25 + x[r, 0] ** 2
            press += (y[r] - pred) ** 2
            tss += (y[r] - y_mean) ** 2
            varss += (y[r] - pred) ** 2 / var
            cnt += 1
    s = _stub_surrogate(egx, x, y)
    assert s.q2_k_score(k) == pytest.approx(1.0 - press / tss, abs=1e-12)
    assert s.pva_k_score(k) == pytest.approx(abs(math.log(varss / cnt)), abs=1e-12)
    # leave-one-out is k = n
    assert s.q2_score() == s.q2_k_score(n)
    assert s.pva_score() == s.pva_k_score(n)
    assert s.iae_alpha_score() == s.iae_alpha_k_score(n)
    # the restatement agrees with the product on the same folds
    folds = egx.cv.cross_validate_surrogates(_StubModel, x, y, k, True)
    preds, vars_, valids = [f.pred for f in folds], [f.var for f in folds], [f.valid for f in folds]
    assert s.q2_k_score(k) == CO.q2(preds, valids, y)
    assert s.pva_k_score(k) == CO.pva(preds, vars_, valids, y)
    assert s.iae_alpha_k_score(k) == pytest.approx(CO.iae_alpha(preds, vars_, valids, y)[0], abs=1e-12)


def test_iae_alpha_coverage_known_intervals(egx):
    """Targets 0, unit variance, predictions 0 (always inside an interval) and 10 (never: the widest half-width is ppf(0.99) =
    2.33) in equal parts in every fold: the coverage is 1/2 for every alpha, the score the mean of |alpha - 1/2|."""
    n, k = 20, 2
    x = np.array([0.0, 10.0] * (n // 2)).reshape(-1, 1)
    y = np.zeros(n)

    class Model:
        def __init__(self, xt, yt):
            pass

        def predict_valvar(self, xq):
            return xq[:, 0].copy(), np.ones(xq.shape[0])

    s = _stub_surrogate(egx, x, y, Model)
    want = 2.0 * sum(0.48 - i * 0.96 / 19.0 for i in range(10)) / 20.0
    plot = egx.IaeAlphaPlotData()
    assert s.iae_alpha_k_score(k, plot) == pytest.approx(want, abs=1e-12)
    assert len(plot.alphas) == 20 and plot.alphas[0] == pytest.approx(0.02) and plot.alphas[-1] == pytest.approx(0.98)
    np.testing.assert_allclose(plot.deltas, 0.5, atol=1e-15)
    as_dict = {}
    s.iae_alpha_k_score(k, as_dict)
    assert as_dict["deltas"] == plot.deltas
    # an interval that just holds / just misses: error 1 sigma is inside exactly for the alphas with ppf(1 - alpha / 2) >= 1
    x1 = np.ones((n, 1))
    s1 = _stub_surrogate(egx, x1, y, Model)
    s1.iae_alpha_k_score(k, plot)
    inside = [1.0 if NormalDist().inv_cdf(1.0 - a / 2.0) >= 1.0 else 0.0 for a in plot.alphas]
    assert plot.deltas == inside and 0.0 < sum(inside) < 20.0


# ------------------------------------------------------------------ select_expert with stub fits
def _stub_cv(egx, delta_of, calls):
    def cv(params, x, y, k):
        name = egx.cv.pair_name(type(params._mean), type(params._corr))
        calls.append((name, k, params._theta_tuning.kind))
        return [egx.cv.Fold(None, y[va] + delta_of(name), None, va) for _, va in egx.fold_indices(x.shape[0], k)]
    return cv


ORDER = [f"{m}_{c}" for m in CO.MEANS for c in CO.CORRS]


def test_select_expert_table_order_and_first_minimum(egx):
    pairs = egx.cv.expert_pairs(egx.RegressionSpec.ALL, egx.CorrelationSpec.ALL)
    assert [egx.cv.pair_name(m, c) for m, c in pairs] == ORDER
    x = np.linspace(0.0, 1.0, 40).reshape(-1, 1)
    y = x[:, 0] ** 2
    calls = []
    delta = {name: 1.0 + 0.1 * i for i, name in enumerate(ORDER)}
    delta["Linear_Matern32"] = delta["Quadratic_AbsoluteExponential"] = 0.25  # a tie: the first of the two wins
    winner, table = egx.cv.select_expert(pairs, x, y, cross_validate_fn=_stub_cv(egx, delta.get, calls))
    assert [n for n, _ in table] == ORDER
    assert [c[0] for c in calls] == ORDER and all(c[1] == 5 and c[2] == "Full" for c in calls)  # n_fold = min(n, 5); default tuning
    for name, e in table:  # mean over the folds of ||delta 1||_2 with 8 validation rows each
        assert e == pytest.approx(delta[name] * math.sqrt(8.0), abs=1e-12)
    assert winner == "Linear_Matern32"
    # a NaN error compares equal (partial_cmp(..).unwrap_or(Equal)): in first place it stays the minimum, later it never wins
    delta["Constant_SquaredExponential"] = math.nan
    assert egx.cv.select_expert(pairs, x, y, cross_validate_fn=_stub_cv(egx, delta.get, []))[0] == "Constant_SquaredExponential"
    delta["Constant_SquaredExponential"], delta["Constant_Matern32"] = 9.0, math.nan
    assert egx.cv.select_expert(pairs, x, y, cross_validate_fn=_stub_cv(egx, delta.get, []))[0] == "Linear_Matern32"
    # the extension: a tuning for the fold fits
    calls = []
    egx.cv.select_expert(pairs[:2], x, y, theta_tuning=egx.ThetaTuning.Fixed(np.array([1.0])),
                         cross_validate_fn=_stub_cv(egx, delta.get, calls))
    assert [c[2] for c in calls] == ["Fixed", "Fixed"]


def test_select_expert_inf_rules(egx):
    """The reference compares the FOLD COUNT with 4 nx (Quadratic) and 3 nx (Linear)."""
    pairs = egx.cv.expert_pairs(egx.RegressionSpec.ALL, egx.CorrelationSpec.ALL)
    one = lambda name: 1.0  # noqa: E731
    # nx = 1, n >= 5: n_fold = 5, every pair is fitted
    calls = []
    _, table = egx.cv.select_expert(pairs, np.linspace(0, 1, 12).reshape(-1, 1), np.arange(12.0), cross_validate_fn=_stub_cv(egx, one, calls))
    assert len(calls) == 12 and not any(math.isinf(e) for _, e in table)
    # nx = 1, n = 3: n_fold = 3 < 4 -> Quadratic is out, Linear (3 < 3 is false) is fitted
    calls = []
    _, table = egx.cv.select_expert(pairs, np.linspace(0, 1, 3).reshape(-1, 1), np.arange(3.0), cross_validate_fn=_stub_cv(egx, one, calls))
    assert [math.isinf(e) for _, e in table] == [False] * 8 + [True] * 4
    assert [c[0] for c in calls] == ORDER[:8] and all(c[1] == 3 for c in calls)
    # nx = 2: 5 < 6 and 5 < 8 -> only Constant is ever fitted, however many points there are
    calls = []
    winner, table = egx.cv.select_expert(pairs, np.random.default_rng(0).random((200, 2)), np.arange(200.0),
                                         cross_validate_fn=_stub_cv(egx, one, calls))
    assert [math.isinf(e) for _, e in table] == [False] * 4 + [True] * 8
    assert [c[0] for c in calls] == ORDER[:4] and winner == "Constant_SquaredExponential"


def test_one_pair_shortcut_fits_nothing(egx):
    calls = []
    pairs = egx.cv.expert_pairs(egx.RegressionSpec.LINEAR, egx.CorrelationSpec.MATERN52)
    winner, table = egx.cv.select_expert(pairs, np.zeros((9, 1)), np.zeros(9), cross_validate_fn=_stub_cv(egx, lambda n: 1.0, calls))
    assert winner == "Linear_Matern52" and table == [] and calls == []
    b = egx.GpMixture.params().expert_specs(egx.RegressionSpec.LINEAR, egx.CorrelationSpec.MATERN52)
    assert b._expert_pairs is None and str(b._mean) == "LinearMean" and str(b._corr) == "Matern52"
    assert b.select_expert(np.zeros((9, 1)), np.zeros(9)) == ("Linear_Matern52", [])
    assert len(egx.GpMixture.params().expert_specs(egx.RegressionSpec.ALL, egx.CorrelationSpec.MATERN32 | egx.CorrelationSpec.MATERN52)._expert_pairs) == 6
    # the refusals the builder had stay
    with pytest.raises(NotImplementedError):
        egx.GpMixture.params().regression_spec(egx.RegressionSpec.ALL)
    with pytest.raises(NotImplementedError):
        egx.GpMixture.params().n_clusters("auto")


# ------------------------------------------------------------------ binding
def test_predict_valvar_multi_argument_validation_before_device(egx):
    from egobox_amd import _lib as L

    class Fake:
        def __init__(self, d):
            self.d, self._h = d, None

    a, b, c = Fake(2), Fake(2), Fake(3)
    xq = np.zeros((2, 4, 2))
    with pytest.raises(egx.InvalidValueError):
        egx.predict_valvar_multi([], xq)
    with pytest.raises(egx.InvalidValueError):
        egx.predict_valvar_multi([a, b], xq, want_val=False, want_var=False)
    with pytest.raises(egx.InvalidValueError):
        egx.predict_valvar_multi([a, c], xq)             # mixed d
    with pytest.raises(egx.InvalidValueError):
        egx.predict_valvar_multi([a, a], xq)             # duplicates
    with pytest.raises(egx.InvalidValueError):
        egx.predict_valvar_multi([a, b], xq[:1])         # one block per model
    with pytest.raises(egx.InvalidValueError):
        egx.predict_valvar_multi([a, b], np.zeros((2, 4, 3)))
    # the library's own rules, before any device work
    lib = L.load()
    out = np.zeros(4)
    assert lib.egx_gp_predict_valvar_multi(None, 0, L.dptr(xq), 4, L.dptr(out), None) == L.ERR_INVALID_VALUE
    assert lib.egx_gp_predict_valvar_multi(None, 2, L.dptr(xq), 4, L.dptr(out), None) == L.ERR_INVALID_VALUE
    arr = (L.C.c_void_p * 2)()  # two NULL handles
    assert lib.egx_gp_predict_valvar_multi(arr, 2, L.dptr(xq), 4, L.dptr(out), None) == L.ERR_INVALID_VALUE
    assert lib.egx_gp_predict_valvar_multi(arr, 2, None, 4, L.dptr(out), None) == L.ERR_INVALID_VALUE
    assert lib.egx_gp_predict_valvar_multi(arr, 2, L.dptr(xq), 4, None, None) == L.ERR_INVALID_VALUE
