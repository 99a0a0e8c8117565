"""The sharded fold behind egx_moe_predict_valvar / egx_moe_predict_valvar_gradients (egobox_amd/csrc/moe_fold.h,
moe_host.hip) on real experts, BIT FOR BIT against a numpy restatement of its order of additions built from the same experts'
own outputs: worker A sums the local experts 0, 2, 4, .., worker B 1, 3, .., then A + B, then the ranks from 0.0 in rank order.
numpy's p * y, (p * p) * v, g * p + pp * y and g * (p * p) + 2 * p * pp * v are the fold's IEEE operations in its order.

Every expert call stays above 8 query points: predict_impl serves variance calls of 1 to 8 points by a path that depends on
how many such calls the handle has answered before, so bits there belong to the call history, not to the fold; m = 1 is held
to the two-rank test's tolerance instead."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N, D = 64, 2
THETA = np.array([1.3, 0.7])
WANTS = [(True, True), (True, False), (False, True)]


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


def _experts(egx, k):
    from egobox_amd import workload
    out = []
    for e in range(k):
        x, y = workload.make_training_set(N, D, seed=40 + e)
        out.append(egx.GaussianProcess.params(egx.ConstantMean(), egx.SquaredExponentialCorr())
                   .theta_tuning(egx.ThetaTuning.Fixed(THETA)).fit(x, (e + 1.0) * y))
    return out


def _mixture(k):
    """components 0 and 1 identical (their responsibilities tie: the first maximum, 0, owns the points), the last one of
    k >= 3 so far away that no point of the unit box is routed to it"""
    from egobox_amd.moe import GaussianMixture
    centres = np.array([[0.3, 0.5], [0.3, 0.5], [0.75, 0.25], [0.7, 0.8], [0.5, 0.5]])[:k].copy()
    if k >= 3:
        centres[k - 1] = [9.0, -7.0]
    w = np.full(k, 1.0 / k)
    return GaussianMixture(w, centres, np.stack([np.eye(D) * 0.05] * k), 0.9)


def _queries(m):
    return np.random.default_rng(11 + m).random((m, D))


def _inputs(k, m):
    gmx, xq = _mixture(k), _queries(m)
    probas = np.ascontiguousarray(gmx.predict_probas_device(xq))
    dprobas = np.ascontiguousarray(gmx.predict_probas_derivatives_device(xq)) if k > 1 else None
    if k > 1:
        np.testing.assert_array_equal(probas[:, 0], probas[:, 1])  # the tie
    return xq, probas, dprobas


def _handles(experts):
    hs = [e._h._h for e in experts]
    return (C.c_void_p * len(hs))(*[h.value for h in hs]), np.arange(len(hs), dtype=np.int32)


def _lib_values(experts, probas, xq, smooth, want, sweep=None):
    from egobox_amd import _lib as L
    harr, ids = _handles(experts)
    m, k = probas.shape
    val, var = (np.full(m, np.nan) if w else None for w in want)
    L.check(L.load().egx_moe_predict_valvar(sweep._h if sweep is not None else None, harr, ids.ctypes.data_as(L.c_int32_p), k, k,
                                            L.dptr(probas), L.dptr(xq), m, D, int(smooth), L.dptr(val) if want[0] else None,
                                            L.dptr(var) if want[1] else None))
    return val, var


def _lib_gradients(experts, probas, dprobas, xq, smooth, want, sweep=None):
    from egobox_amd import _lib as L
    harr, ids = _handles(experts)
    m, k = probas.shape
    gy, gv = (np.full((m, D), np.nan) if w else None for w in want)
    L.check(L.load().egx_moe_predict_valvar_gradients(sweep._h if sweep is not None else None, harr,
                                                      ids.ctypes.data_as(L.c_int32_p), k, k, L.dptr(probas),
                                                      L.dptr(dprobas) if dprobas is not None else None, L.dptr(xq), m, D,
                                                      int(smooth), L.dptr(gy) if want[0] else None, L.dptr(gv) if want[1] else None))
    return gy, gv


# ---- the experts' own outputs through the entry point the library picks for the outputs requested
def _expert_values(e, x, want):
    if want[0] and want[1]:
        return e.predict_valvar(x)
    return (e.predict(x), None) if want[0] else (None, e.predict_var(x))


def _expert_gradients(e, x, want):
    if want[0] and want[1]:
        return e.predict_valvar_gradients(x)
    return (e.predict_gradients(x), None) if want[0] else (None, e.predict_var_gradients(x))


def _in_worker_order(terms):
    """terms[e] of the local experts -> ((e0 + e2 + e4) + (e1 + e3)), every partial sum from 0.0, then 0.0 + the one rank"""
    a = np.zeros_like(terms[0])
    for t in terms[0::2]:
        a = a + t
    if len(terms) > 1:
        b = np.zeros_like(terms[0])
        for t in terms[1::2]:
            b = b + t
        a = a + b
    return 0.0 + a


def _restate_smooth_values(experts, probas, xq, want):
    outs = [_expert_values(e, xq, want) for e in experts]
    val = _in_worker_order([probas[:, g] * y for g, (y, _) in enumerate(outs)]) if want[0] else None
    var = _in_worker_order([(probas[:, g] * probas[:, g]) * v for g, (_, v) in enumerate(outs)]) if want[1] else None
    return val, var


def _restate_smooth_gradients(experts, probas, dprobas, xq, want):
    grads = [_expert_gradients(e, xq, want) for e in experts]
    vals = [_expert_values(e, xq, want) for e in experts] if dprobas is not None else None
    ty, tv = [], []
    for g in range(len(experts)):
        p = probas[:, g][:, None]
        if dprobas is not None:
            pp = dprobas[:, g, :]
            if want[0]:
                ty.append(grads[g][0] * p + pp * vals[g][0][:, None])
            if want[1]:
                tv.append(grads[g][1] * (p * p) + 2.0 * p * pp * vals[g][1][:, None])
        else:  # a lone expert: the p' terms are `+ 0.0`
            if want[0]:
                ty.append(grads[g][0] * p + 0.0)
            if want[1]:
                tv.append(grads[g][1] * (p * p) + 0.0)
    return (_in_worker_order(ty) if want[0] else None), (_in_worker_order(tv) if want[1] else None)


def _restate_hard(experts, probas, xq, want, fn, width):
    """every point by the expert of the FIRST maximum of its responsibilities (numpy's argmax), one call per non-empty subset"""
    m = xq.shape[0]
    cluster = np.argmax(probas, axis=1)
    out = [np.zeros((m,) + width) if w else None for w in want]
    for g, e in enumerate(experts):
        idx = np.flatnonzero(cluster == g)
        if idx.size == 0:
            continue
        assert idx.size > 8, (g, idx.size)
        got = fn(e, np.ascontiguousarray(xq[idx]), want)
        for o, r in zip(out, got):
            if o is not None:
                o[idx] = 0.0 + r
    return out, cluster


def _close(experts):
    for e in experts:
        e.close()


def _assert_same(got, want):
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_smooth_fold_keeps_the_documented_order_of_additions(egx, k):
    """k = 5: worker A folds three experts, B two; k = 2: one each; k = 1: no second thread, no p' terms"""
    experts = _experts(egx, k)
    try:
        for m in (65, 130):
            xq, probas, dprobas = _inputs(k, m)
            for want in WANTS:
                _assert_same(_lib_values(experts, probas, xq, True, want), _restate_smooth_values(experts, probas, xq, want))
                _assert_same(_lib_gradients(experts, probas, dprobas, xq, True, want),
                             _restate_smooth_gradients(experts, probas, dprobas, xq, want))
    finally:
        _close(experts)


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_hard_fold_routes_by_the_first_maximum(egx, k):
    """the tied component 1 and the far component own no point and get no call; the rows come back at their own indices"""
    experts = _experts(egx, k)
    try:
        for m in (65, 130):
            xq, probas, dprobas = _inputs(k, m)
            for want in WANTS:
                want_v, cluster = _restate_hard(experts, probas, xq, want, _expert_values, ())
                _assert_same(_lib_values(experts, probas, xq, False, want), want_v)
                want_g, _ = _restate_hard(experts, probas, xq, want, _expert_gradients, (D,))
                _assert_same(_lib_gradients(experts, probas, None, xq, False, want), want_g)
            owners = set(np.unique(cluster))
            assert 1 not in owners and (k < 3 or k - 1 not in owners)
            assert owners == ({0, 2, 3} if k == 5 else {0})
    finally:
        _close(experts)


@pytest.mark.parametrize("smooth", [True, False])
def test_one_query_point_at_the_two_rank_tolerance(egx, smooth):
    """m = 1.  A handle answers its third and later variance calls of 1 to 8 points through the cached C^-T, the first two
    through the batched path (5e-9 apart in the variance): three such calls per expert first, so that the reference's calls
    and the library's are served alike whatever their order"""
    experts = _experts(egx, 3)
    try:
        xq, probas, dprobas = _inputs(3, 1)
        for e in experts:
            for _ in range(3):
                e.predict_var(xq)
        want = (True, True)
        if smooth:
            ref_v = _restate_smooth_values(experts, probas, xq, want)
            ref_g = _restate_smooth_gradients(experts, probas, dprobas, xq, want)
        else:
            e = experts[int(np.argmax(probas[0]))]
            ref_v, ref_g = e.predict_valvar(xq), e.predict_valvar_gradients(xq)
        got_v = _lib_values(experts, probas, xq, smooth, want)
        got_g = _lib_gradients(experts, probas, dprobas, xq, smooth, want)
        for g, w, atol in zip(got_v + got_g, tuple(ref_v) + tuple(ref_g), (1e-13, 1e-14, 1e-13, 1e-14)):
            np.testing.assert_allclose(g, w, rtol=1e-12, atol=atol)  # (value, variance) as the two-rank test holds them
    finally:
        _close(experts)


@pytest.mark.parametrize("smooth", [True, False])
def test_a_sweep_of_one_rank_returns_the_bits_of_no_sweep(egx, smooth):
    """the same calls with sw = NULL (no exchange) and through a Sweep of world 1 (the exchange's copy)"""
    from egobox_amd import workload
    experts = _experts(egx, 3)
    sweep = egx.Sweep(*workload.make_training_set(N, D, seed=40))
    try:
        xq, probas, dprobas = _inputs(3, 65)
        for want in WANTS:
            _assert_same(_lib_values(experts, probas, xq, smooth, want, sweep), _lib_values(experts, probas, xq, smooth, want))
            _assert_same(_lib_gradients(experts, probas, dprobas, xq, smooth, want, sweep),
                         _lib_gradients(experts, probas, dprobas, xq, smooth, want))
    finally:
        sweep.close()
        _close(experts)
