"""Egor on the device (egobox_amd/egor.py): the reference's own end-to-end cases with the reference's own tolerances --
ask-and-tell and minimize on xsinx (egor_service.rs:150-175, egor.rs:497-533), G24 with two constraint surrogates (egor.rs:857-941),
q points (egor.rs:1009-1039, :594-602), a mixed-integer space (egor.rs:1043-1072) -- a mixture as surrogate, and the device handles
of a run.  Seeds are fixed; the random stream is numpy's, so the points are this project's, the optima the problem's."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

XSINX_LIM = np.array([[0.0, 25.0]])
G24_LIM = np.array([[0.0, 3.0], [0.0, 4.0]])
G24_OPT = np.array([2.3295, 3.1785])
EPS100 = 100.0 * np.finfo(float).eps


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


def xsinx(x):
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    return (x - 3.5) * np.sin((x - 3.5) / np.pi)


def mixsinx(x):
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    if abs(np.linalg.norm(np.round(x)) - np.linalg.norm(x)) >= 1e-6:
        raise ValueError(f"mixsinx works only on integers, got {x}")
    return xsinx(x)


def g24(x):
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    x0, x1 = x[:, 0], x[:, 1]
    return np.column_stack([-x0 - x1,
                            -2.0 * x0 ** 4 + 8.0 * x0 ** 3 - 8.0 * x0 ** 2 + x1 - 2.0,
                            -4.0 * x0 ** 4 + 32.0 * x0 ** 3 - 88.0 * x0 ** 2 + 96.0 * x0 + x1 - 36.0])


def _no_duplicates(x):
    d = np.abs(x[:, None, :] - x[None, :, :]).sum(-1) + np.eye(x.shape[0])
    return d.min() >= EPS100


# ---- 1. ask-and-tell -------------------------------------------------------------------------------------------------------------
def test_suggest_xsinx_ask_and_tell(egx):
    ego = egx.Egor(XSINX_LIM, gp_config=egx.GpConfig(egx.RegressionSpec.CONSTANT, egx.CorrelationSpec.SQUARED_EXPONENTIAL),
                   infill_strategy=egx.EI, seed=42)
    doe = np.array([[0.0], [7.0], [20.0], [25.0]])
    y_doe = xsinx(doe)
    first = ego.suggest(doe, y_doe)
    assert first.shape == (1, 1) and 0.0 <= first[0, 0] <= 25.0
    assert np.array_equal(first, ego.suggest(doe, y_doe))           # the same data and seed: the same bits
    for i in range(10):
        x = first if i == 0 else ego.suggest(doe, y_doe)
        doe = np.vstack([doe, x])
        y_doe = xsinx(doe)
    print("ask-and-tell min(y)", y_doe.min(), "at", doe[np.argmin(y_doe), 0])
    assert abs(y_doe.min() - (-15.1)) <= 1e-1
    res = ego.get_result(doe, y_doe)
    assert res.y_opt[0] == y_doe.min() and ego.get_result_index(doe, y_doe) == int(np.argmin(y_doe))


# ---- 2. minimize, xsinx ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy,iters", [("EI", 10), ("LOG_EI", 30)])
def test_minimize_xsinx(egx, strategy, iters):
    ego = egx.Egor(XSINX_LIM, infill_strategy=getattr(egx, strategy), infill_optimizer="slsqp", doe=np.array([[0.0], [7.0], [25.0]]),
                   seed=42)
    res = ego.minimize(xsinx, max_iters=iters)
    print(strategy, "y_opt", res.y_opt, "x_opt", res.x_opt, "rows", res.x_doe.shape[0], "rejected", ego.n_rejected_)
    assert abs(res.y_opt[0] - (-15.125)) <= 2e-3
    assert res.x_doe.shape[0] <= 3 + iters and res.x_doe.shape[0] == 3 + ego.n_iter_ and res.y_doe.shape == (res.x_doe.shape[0], 1)
    assert np.array_equal(res.x_doe[:3, 0], [0.0, 7.0, 25.0])
    assert _no_duplicates(res.x_doe)
    assert np.array_equal(res.y_doe, xsinx(res.x_doe)) and res.y_opt[0] == res.y_doe.min()
    assert np.array_equal(res.x_opt, res.x_doe[np.argmin(res.y_doe[:, 0])])


# ---- 3. G24: two constraint surrogates -----------------------------------------------------------------------------------------------
G24_CONFIGS = {"wb2_cobyla": dict(infill_strategy="WB2", infill_optimizer="cobyla", cstr_tol=[2e-3, 1e-3]),
               "defaults": dict(cstr_tol=[1e-5, 1e-5])}


@pytest.mark.parametrize("doe_seed", [0, 1, 42])
@pytest.mark.parametrize("config", sorted(G24_CONFIGS))
def test_minimize_g24(egx, config, doe_seed):
    kw = G24_CONFIGS[config]
    doe = egx.Lhs(G24_LIM, seed=doe_seed).sample(3)
    ego = egx.Egor(G24_LIM, n_cstr=2, doe=doe, seed=42, **kw)
    if config == "defaults":
        assert (ego.infill_strategy, ego.infill_optimizer, ego.cstr_strategy, ego.cstr_infill) == (egx.LOG_EI, "slsqp", "mean", False)
    res = ego.minimize(g24, max_iters=20)
    print(config, doe_seed, "x_opt", res.x_opt, "y_opt", res.y_opt, "rows", res.x_doe.shape[0], "rejected", ego.n_rejected_)
    assert np.abs(res.x_opt - G24_OPT).max() <= 3e-2
    assert egx.egor.is_feasible(res.y_opt, None, ego.cstr_tol)
    assert np.array_equal(res.x_doe[:3], doe) and res.x_doe.shape[0] <= 3 + 20 and _no_duplicates(res.x_doe)
    assert np.array_equal(res.y_doe, g24(res.x_doe))


# ---- 4. q points -----------------------------------------------------------------------------------------------------------------------
def _record_fits(egx, monkeypatch):
    """every `select_next_points` call and the theta tuning of every surrogate fit, in order; wrapped here, no product hook"""
    events = []
    fit, select = egx.GpMixtureParams.fit, egx.Egor.select_next_points

    def fit_wrap(self, x, y):
        events.append(("fit", {t.kind for t in self._theta_tunings}))
        return fit(self, x, y)

    def select_wrap(self, init, iteration, *a, **k):
        events.append(("select", int(iteration)))
        return select(self, init, iteration, *a, **k)

    monkeypatch.setattr(egx.GpMixtureParams, "fit", fit_wrap)
    monkeypatch.setattr(egx.Egor, "select_next_points", select_wrap)
    return events


def _check_tunings(events, q, q_optmod, n_models):
    """Full where the rule names it -- (iter q + i) % q_optmod == 0, and the clustering fit of iteration 0 -- Fixed elsewhere"""
    n_full = n_fixed = 0
    pos = 0
    while pos < len(events):
        kind, it = events[pos]
        assert kind == "select"
        fits = []
        pos += 1
        while pos < len(events) and events[pos][0] == "fit":
            fits.append(events[pos][1])
            pos += 1
        assert len(fits) == q * n_models
        for i in range(q):
            want = "Full" if (it * q + i) % q_optmod == 0 or (it == 0 and i == 0) else "Fixed"
            assert fits[i * n_models:(i + 1) * n_models] == [{want}] * n_models, (it, i, fits)
            n_full += want == "Full"
            n_fixed += want == "Fixed"
    return n_full, n_fixed


@pytest.mark.parametrize("q_optmod,eps", [(1, 2e-2), (3, 1e-1)])
def test_minimize_g24_q_points(egx, monkeypatch, q_optmod, eps):
    events = _record_fits(egx, monkeypatch)
    q = 2
    doe = egx.Lhs(G24_LIM, seed=42).sample(10)
    ego = egx.Egor(G24_LIM, n_cstr=2, cstr_tol=[2e-6, 2e-6], q_points=q, q_infill_strategy=egx.QEiStrategy.KB, q_optmod=q_optmod,
                   doe=doe, target=-5.5030, seed=42)
    res = ego.minimize(g24, max_iters=20)
    print("q_optmod", q_optmod, "x_opt", res.x_opt, "y_opt", res.y_opt, "iterations", ego.n_iter_, "rejected", ego.n_rejected_)
    assert 1 <= ego.n_iter_ <= 20
    n_select = sum(1 for e in events if e[0] == "select")
    assert res.x_doe.shape[0] == 10 + q * n_select - ego.n_rejected_       # every proposed row is in the DOE or was rejected
    if ego.n_rejected_ == 0:
        assert n_select == ego.n_iter_ and res.x_doe.shape[0] == 10 + q * ego.n_iter_
    assert np.abs(res.x_opt - G24_OPT).max() <= eps
    assert _no_duplicates(res.x_doe) and np.array_equal(res.y_doe, g24(res.x_doe))
    n_full, n_fixed = _check_tunings(events, q, q_optmod, 3)
    assert n_full >= 1 and (n_fixed == 0 if q_optmod == 1 else n_fixed >= 1 or n_select == 1)


# ---- 5. mixed-integer ----------------------------------------------------------------------------------------------------------------
def test_minimize_mixed_integer(egx):
    ego = egx.Egor([egx.XType.Int(0, 25)], doe=np.array([[0.0], [7.0], [25.0]]), infill_strategy=egx.EI, target=-15.1, seed=42)
    res = ego.minimize(mixsinx, max_iters=20)     # mixsinx raises on anything but integers
    print("mixint x_opt", res.x_opt, "y_opt", res.y_opt, "rows", res.x_doe.shape[0], "rejected", ego.n_rejected_)
    assert abs(res.x_opt[0] - 18.0) <= 2.0
    assert np.array_equal(res.x_doe, np.round(res.x_doe)) and res.x_doe.min() >= 0.0 and res.x_doe.max() <= 25.0
    assert _no_duplicates(res.x_doe) and res.x_doe.shape[0] <= 3 + 20
    s = ego.suggest(res.x_doe, res.y_doe)
    assert s.shape == (1, 1) and s[0, 0] == np.round(s[0, 0])


# ---- 6. a mixture as surrogate ---------------------------------------------------------------------------------------------------------
def test_minimize_with_a_mixture_surrogate(egx, monkeypatch):
    trained, reused = [], []
    gmm_fit, set_gmx = egx.GaussianMixture.fit.__func__, egx.GpMixtureParams.gmx

    def fit_wrap(cls, *a, **k):
        gm = gmm_fit(cls, *a, **k)
        trained.append(gm)
        return gm

    def gmx_wrap(self, gmx):
        reused.append(gmx)
        return set_gmx(self, gmx)

    monkeypatch.setattr(egx.GaussianMixture, "fit", classmethod(fit_wrap))
    monkeypatch.setattr(egx.GpMixtureParams, "gmx", gmx_wrap)
    # two groups of six rows, the plateau on the left and the valley on the right: the mixture of [x, y] separates them, and every
    # cluster keeps the three rows a trained expert needs
    doe = np.array([0.0, 2.0, 4.0, 6.0, 8.0, 10.0, 15.0, 16.5, 18.0, 19.5, 21.0, 22.5]).reshape(-1, 1)
    ego = egx.Egor(XSINX_LIM, gp_config=egx.GpConfig(n_clusters=2, recombination="hard"), doe=doe, seed=42)
    res = ego.minimize(xsinx, max_iters=5)
    print("mixture y_opt", res.y_opt, "rows", res.x_doe.shape[0], "rejected", ego.n_rejected_)
    assert ego.n_iter_ == 5 and res.x_doe.shape[0] == 17
    assert len(trained) == 1                                   # iteration 0 clusters, once
    assert len(reused) >= 4 and all(g is reused[0] for g in reused) and reused[0].n_clusters == 2   # iterations 1..4 reuse it
    best = [ego.get_result(res.x_doe[:n], res.y_doe[:n]).y_opt[0] for n in range(12, 18)]
    assert all(b <= a for a, b in zip(best, best[1:])) and res.y_opt[0] == best[-1]


# ---- 7. handles do not accumulate --------------------------------------------------------------------------------------------------------
def test_handles_do_not_accumulate(egx, monkeypatch):
    import torch
    live = set()
    gp_init, gp_close = egx.GpHandle.__init__, egx.GpHandle.close
    inf_init, inf_close = egx.InfillObjective.__init__, egx.InfillObjective.close

    def opened(init):
        def wrap(self, *a, **k):
            init(self, *a, **k)
            live.add(id(self))
        return wrap

    def closed(close):
        def wrap(self):
            close(self)
            live.discard(id(self))
        return wrap

    monkeypatch.setattr(egx.GpHandle, "__init__", opened(gp_init))
    monkeypatch.setattr(egx.GpHandle, "close", closed(gp_close))
    monkeypatch.setattr(egx.InfillObjective, "__init__", opened(inf_init))
    monkeypatch.setattr(egx.InfillObjective, "close", closed(inf_close))
    kw = dict(infill_strategy=egx.EI, doe=np.array([[0.0], [7.0], [25.0]]), seed=42)
    egx.Egor(XSINX_LIM, **kw).minimize(xsinx, max_iters=10)    # first use: code objects, the pool's first entries
    gc.collect()
    egx.trim()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    assert not live
    seen = [0]

    def fun(x):
        seen[0] = max(seen[0], len(live))                       # while the loop runs: no model of a finished step is left
        return xsinx(x)

    res = egx.Egor(XSINX_LIM, **kw).minimize(fun, max_iters=10)
    assert res.x_doe.shape[0] > 3
    assert seen[0] == 0 and not live                            # closed by the loop itself, before any collection
    gc.collect()
    egx.trim()
    assert egx.pool_stats()["cached_bytes"] == 0
    torch.cuda.synchronize()
    # (200 MB, not 64: a run may touch a hardware queue more than the baseline had, ~90 MB of runtime scratch each that is not
    #  the pool's to return -- tests/test_gpu_parity.py, the create / destroy cycles; a leaked model is caught by `live` above)
    assert free0 - torch.cuda.mem_get_info()[0] < 200 << 20
