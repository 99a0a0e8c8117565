"""The likelihood's theta-gradient and the L-BFGS fit of a group in lock-step (egx_gp_likelihood_grad_multi,
egx_gp_fit_lbfgs_multi): every member's row bit for bit its own lone call -- the member is a grid coordinate of the C^-T rider,
of gamma = W rho, of -R^-1 = -(W W^T) and of the trace kernel, which reads each member's own training inputs -- the status
paths inside one run, handles outside a run, the oracle (so that the two routes cannot be wrong together), the C^-T slab the
call shares with the x-gradients' cache, and the fits built on it up to `GpParams.fit_group` and `cross_validate`.

Shapes: k = 5, n = 150, d = 3 (n_pad 256, a partial 64-tile); k = 17, n = 70, d = 2 (two runs, 12 + 5); k = 3, n = 100, d = 70
(d > 64: the dimensions staged in two chunks, the outputs in several DK chunks); k = 4, n = 300, d = 5 (several tile rows)."""
import numpy as np
import pytest

import cv_oracle as CO
from test_gpu_parity import LK_RTOL

pytestmark = pytest.mark.gpu

SQEXP, ABSEXP, MATERN52 = 0, 1, 3
KERNELS = (SQEXP, ABSEXP, MATERN52)
OK, NOT_PD, NAN_THETA = 0, 1, 4


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


def _sets(k, n, d, seed):
    from egobox_amd import workload
    xy = [workload.make_training_set(n, d, seed=seed + j) for j in range(k)]
    return np.stack([x for x, _ in xy]), np.stack([np.asarray(y).reshape(-1) for _, y in xy])


def _close(hs):
    for h in hs:
        h.close()


def _thetas(k, d, theta):
    """a different theta per member"""
    return np.stack([np.full(d, theta * (1.0 + 0.1 * j)) for j in range(k)])


def _lone(hs, thetas):
    """each handle's own likelihood_grad at its row (un-fits it)"""
    return [h.likelihood_grad(th) for h, th in zip(hs, thetas)]


def _assert_rows_equal_lone(egx, hs, thetas, lone=None):
    lone = _lone(hs, thetas) if lone is None else lone
    lk, g, st = egx.likelihood_grad_multi(hs, thetas)
    assert lk.shape == (len(hs),) and g.shape == (len(hs), hs[0].h) and st.shape == (len(hs),)
    for j, (llk, lg, lst) in enumerate(lone):
        assert st[j] == lst, (j, st[j], lst)
        assert np.array_equal(lk[j:j + 1], np.array([llk])), (j, lk[j], llk)
        assert np.array_equal(g[j], lg), (j, g[j], lg)
    return lk, g, st


# ---- 1. lock-step equals lone ------------------------------------------------------------------------------------------------
# theta by shape and kernel as the x-gradients' test chooses it (a well posed factorisation), trend 1 on the first shape as well
CASES = [(5, 150, 3, mean, corr, 1.0 if corr == SQEXP else 2.0) for corr in KERNELS for mean in (0, 1)] + \
        [(17, 70, 2, 0, corr, 5.0 if corr == SQEXP else 3.0) for corr in KERNELS] + \
        [(3, 100, 70, 0, corr, 0.1) for corr in KERNELS] + \
        [(4, 300, 5, 0, corr, 1.0 if corr == SQEXP else 2.0) for corr in KERNELS]


@pytest.mark.parametrize("k,n,d,mean,corr,theta", CASES)
def test_lockstep_equals_lone(egx, k, n, d, mean, corr, theta):
    xs, ys = _sets(k, n, d, seed=300 + n)
    hs = egx.GpHandle.create_group(xs, ys, mean=mean, corr=corr)
    try:
        lk, g, st = _assert_rows_equal_lone(egx, hs, _thetas(k, d, theta))
        assert np.all(st == OK) and np.all(np.isfinite(lk)) and np.all(np.isfinite(g)) and np.all(np.abs(g).max(axis=1) > 0)
    finally:
        _close(hs)


# ---- 2. mixed forms and failures inside one run ------------------------------------------------------------------------------
def test_mixed_forms_and_failures_in_one_run(egx):
    """Member 1: a NaN theta (answered at once; it cuts the run).  Member 2: one theta component EXACTLY 0.0 -- the library
    accepts it (checked on the lone call below: status OK), so the zero itself is used, not a smallest accepted value -- which
    puts it on the raw form of the trace kernel between prescaled neighbours.  Member 4: training rows 0 and 1 identical in a
    group without nugget, so the second pivot is exactly zero: not positive definite.  Status paths only: the VALUES of a raw-form
    member between prescaled neighbours are held to the closed form in tests/test_gpu_theta_grad.py::test_mixed_form_group_rows."""
    k, n, d = 6, 150, 3
    xs, ys = _sets(k, n, d, seed=77)
    xs[4, 1] = xs[4, 0]
    ys[4, 1] = ys[4, 0]
    hs = egx.GpHandle.create_group(xs, ys, corr=MATERN52, nugget=0.0)
    try:
        thetas = _thetas(k, d, 2.0)
        thetas[2, 1] = 0.0
        thetas[1, 2] = np.nan
        lone = _lone(hs, thetas)
        # the zero component is accepted (Matern-5/2 is flat in a coefficient at zero: that component of the gradient is 0)
        assert lone[2][2] == OK and np.isfinite(lone[2][0]) and lone[2][1][0] != 0.0 and lone[2][1][2] != 0.0
        assert lone[4][2] == NOT_PD and lone[4][0] == -np.inf and not lone[4][1].any()
        assert lone[1][2] == NAN_THETA and lone[1][0] == -np.inf and not lone[1][1].any()
        lk, g, st = _assert_rows_equal_lone(egx, hs, thetas, lone)
        assert list(st) == [OK, NAN_THETA, OK, OK, NOT_PD, OK]
        assert lk[1] == -np.inf and lk[4] == -np.inf and not g[1].any() and not g[4].any()
        for j in (0, 2, 3, 5):
            assert np.isfinite(lk[j]) and g[j].any()
    finally:
        _close(hs)


# ---- 3. handles outside a run ------------------------------------------------------------------------------------------------
def test_out_of_run_handles(egx):
    """Two members in reversed order, a lone handle of the same h (several workspaces, fitted: the call un-fits it as it does a
    member), a KPLS handle (w_star) of the same h, and the remaining members: every row is the lone call's."""
    k, n, d = 5, 150, 3
    xs, ys = _sets(k, n, d, seed=450)
    xl, yl = _sets(1, 120, d, seed=60)
    xk, yk = _sets(1, 120, 5, seed=61)  # five inputs reduced to h = 3 components
    hs = egx.GpHandle.create_group(xs, ys, corr=MATERN52)
    lone = egx.GpHandle(xl[0], yl[0], corr=MATERN52, n_workspaces=3)
    kpls = egx.GpHandle(xk[0], yk[0], corr=MATERN52, w_star=np.random.default_rng(2).standard_normal((5, d)))
    try:
        lone.finalize(np.full(d, 2.0))
        order = [hs[1], hs[0], lone, hs[2], hs[3], kpls, hs[4]]
        thetas = _thetas(len(order), d, 2.0)
        thetas[5] = [0.7, 0.4, 0.5]
        ref = _lone(order, thetas)
        lone.predict(xl[0][:9])  # (its own call kept it fitted on the spare workspaces; the multi call does not)
        lk, g, st = _assert_rows_equal_lone(egx, order, thetas, ref)
        assert np.all(st == OK)
        with pytest.raises(egx.NotFittedError):
            lone.predict(xl[0][:9])
    finally:
        _close(hs + [lone, kpls])


# ---- 4. against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corr", [SQEXP, MATERN52])
def test_first_members_against_oracle(egx, O, corr):
    k, n, d, theta = 5, 150, 3, (1.0 if corr == SQEXP else 2.0)
    xs, ys = _sets(k, n, d, seed=300 + n)
    hs = egx.GpHandle.create_group(xs, ys, corr=corr)
    try:
        thetas = _thetas(k, d, theta)
        lk, g, st = egx.likelihood_grad_multi(hs, thetas)
        for j in (0, 1):
            lk_ref, g_ref = O.likelihood_grad(xs[j], ys[j], thetas[j], corr=CO.CORRS[corr])
            assert st[j] == OK and lk[j] == pytest.approx(lk_ref, rel=LK_RTOL)
            np.testing.assert_allclose(g[j], g_ref, rtol=1e-6, atol=1e-6 * np.abs(g_ref).max())
    finally:
        _close(hs)


# ---- 5. the C^-T slab is also the x-gradients' cache ---------------------------------------------------------------------------
def test_cache_discipline(egx):
    k, n, d, m = 3, 150, 3, 37
    xs, ys = _sets(k, n, d, seed=90)
    hs = egx.GpHandle.create_group(xs, ys, corr=MATERN52)
    try:
        thetas = np.full((k, d), 2.0)
        egx.finalize_multi(hs, thetas)
        xq = np.random.default_rng(3).random((k, m, d))
        record = [h.predict_valvar_gradients(xq[j]) for j, h in enumerate(hs)]  # builds the group's W slab
        lk, g, st = egx.likelihood_grad_multi(hs[:2], _thetas(2, d, 1.5))
        assert np.all(st == OK)
        for j in (0, 1):
            with pytest.raises(egx.NotFittedError):
                hs[j].predict(xq[j])
        gy, gv = hs[2].predict_valvar_gradients(xq[2])  # a fitted member outside the call keeps its slot and its bits
        assert np.array_equal(gy, record[2][0]) and np.array_equal(gv, record[2][1])
        egx.finalize_multi(hs, thetas)  # the evaluated members' slots hold another theta's C^-T: they must be rebuilt
        for j, h in enumerate(hs):
            gy, gv = h.predict_valvar_gradients(xq[j])
            assert np.array_equal(gy, record[j][0]), j
            assert np.array_equal(gv, record[j][1]), j
    finally:
        _close(hs)


# ---- 6. the fit --------------------------------------------------------------------------------------------------------------
STARTS = np.array([[0.3, 0.3], [2.0, 0.5], [0.05, 4.0]])
LO, HI = [1e-3], [50.0]


@pytest.mark.parametrize("k,n,corr", [(4, 120, SQEXP), (4, 120, MATERN52), (13, 70, SQEXP)])
def test_fit_lbfgs_multi_equals_lone_fits(egx, k, n, corr):
    """k = 13: the fit spans two runs (12 + 1)."""
    d, m = 2, 37
    xs, ys = _sets(k, n, d, seed=500 + n)
    xq = np.random.default_rng(8).random((m, d))
    hs = egx.GpHandle.create_group(xs, ys, corr=corr)
    try:
        ne = egx.fit_lbfgs_multi(hs, np.tile(STARTS, (k, 1, 1)), LO, HI, max_iter=30)
        assert ne.shape == (k,)
        for j, h in enumerate(hs):
            with egx.GpHandle(xs[j], ys[j], corr=corr, n_workspaces=1) as one:
                ne_one = one.fit_lbfgs(STARTS, LO, HI, max_iter=30)
                a, b = h.inner(), one.inner()
                assert ne[j] == ne_one, (j, ne[j], ne_one)
                assert np.array_equal(a["theta"], b["theta"]), (j, a["theta"], b["theta"])
                assert a["likelihood"] == b["likelihood"], j
                ya, va = h.predict_valvar(xq)
                yb, vb = one.predict_valvar(xq)
                assert np.array_equal(ya, yb) and np.array_equal(va, vb), j
    finally:
        _close(hs)


# ---- 7. the public route -----------------------------------------------------------------------------------------------------
def _params(egx):
    return egx.GaussianProcess.params(egx.ConstantMean(), egx.Matern52Corr()).optimizer("lbfgs").n_start(3)


def test_fit_group_with_lbfgs(egx):
    k, n, d = 4, 120, 2
    xs, ys = _sets(k, n, d, seed=620)
    params = _params(egx)
    assert params.fits_groups()
    gps = params.fit_group(xs, ys)
    try:
        for j, gp in enumerate(gps):
            one = _params(egx).n_workspaces(1).fit(xs[j], ys[j])
            try:
                assert np.array_equal(gp.theta(), one.theta()), j
                assert gp.likelihood() == one.likelihood(), j
                assert gp.n_evals == one.n_evals, j
            finally:
                one.close()
    finally:
        _close(gps)


def test_cross_validate_with_lbfgs_goes_in_lock_step(egx):
    """The folds through fit_group (what cross_validate does once fits_groups() is True) against the loop of lone fits it ran
    before."""
    n, d, kfold = 100, 2, 5
    x, y = _sets(1, n, d, seed=33)
    x, y = x[0], y[0]
    folds = egx.cross_validate(_params(egx), x, y, kfold, want_var=True)
    loop = egx.cv.cross_validate_surrogates(_params(egx).n_workspaces(1).fit, x, y, kfold, want_var=True)
    assert len(folds) == len(loop) == kfold
    for a, b in zip(folds, loop):
        assert np.array_equal(a.valid, b.valid)
        assert np.array_equal(a.pred, b.pred) and np.array_equal(a.var, b.var)
