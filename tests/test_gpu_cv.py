"""Cross-validation in lock-step on the GPU: the posterior of a group (egx_gp_predict_valvar_multi) against each member's own
call and against the CPU oracle, the fold engine (egobox_amd/cv.py) against oracle fits per fold and against a plain loop
of fits, the GpMetrics scores, and find_best_expert's selection against its restatement on the oracle (tests/cv_oracle.py).

Bars: BASELINE's, as tests/test_gpu_parity.py::_check_fit applies them -- predictions 1e-6 relative (floor 1e-6 max|y|),
variances 1e-6 relative with the absolute floor 1e-9 sigma2 + 1e-6 max(var) for the variances the reference clamps at 0.
Every problem is well posed: the oracle's smallest Cholesky pivot is asserted >> sqrt(nugget) ~ 1.5e-7."""
import math

import numpy as np
import pytest

import cv_oracle as CO

pytestmark = pytest.mark.gpu

PRED_RTOL = 1e-6
MIN_PIVOT = 1e-3


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


def _queries(k, m, d, seed):
    return np.random.default_rng(seed).random((k, m, d))


def _check_oracle(ref, xq, yp, vp):
    assert np.diag(ref.inner.r_chol).min() > MIN_PIVOT
    yr = ref.predict(xq)
    np.testing.assert_allclose(yp, yr, rtol=PRED_RTOL, atol=PRED_RTOL * np.abs(yr).max())
    if vp is not None:
        vr = ref.predict_var(xq)
        np.testing.assert_allclose(vp, vr, rtol=PRED_RTOL, atol=1e-9 * ref.inner.sigma2 + PRED_RTOL * np.abs(vr).max())


# ------------------------------------------------------------------ 1. lock-step equals lone, bit for bit
LOCKSTEP_CASES = [
    # k, n, d, m, mean, corr, theta
    (5, 150, 3, 37, 0, 0, 1.0),     # n_pad 256
    (3, 300, 2, 130, 1, 3, 2.0),    # n_pad 384: two 256-column panels in the solve; two query tiles
    (13, 40, 1, 9, 2, 1, 3.0),      # more members than one run; m just above the few-query threshold
    (2, 40, 70, 9, 0, 0, 0.1),      # d > 64: the chunked-dimension form of the correlation kernels
]


@pytest.mark.parametrize("k,n,d,m,mean,corr,theta", LOCKSTEP_CASES)
def test_lockstep_equals_lone(egx, O, k, n, d, m, mean, corr, theta):
    """Bit for bit against each member's own call -- and, so that the two cannot be wrong together, the first member against the
    oracle (at theta chosen so that the problem is well posed)."""
    xs, ys = _sets(k, n, d, seed=100 + n)
    hs = egx.GpHandle.create_group(xs, ys, mean=mean, corr=corr)
    try:
        egx.finalize_multi(hs, np.full((k, d), theta))
        xq = _queries(k, m, d, seed=n)
        y, v = egx.predict_valvar_multi(hs, xq)
        y_only, none_v = egx.predict_valvar_multi(hs, xq, want_var=False)
        none_y, v_only = egx.predict_valvar_multi(hs, xq, want_val=False)
        assert none_v is None and none_y is None
        assert y.shape == (k, m) and v.shape == (k, m)
        for j, h in enumerate(hs):
            yl, vl = h.predict_valvar(xq[j])  # m > 8: the batched route
            assert np.array_equal(y[j], yl), j
            assert np.array_equal(v[j], vl), j
            assert np.array_equal(y_only[j], h.predict(xq[j])), j
            assert np.array_equal(v_only[j], h.predict_var(xq[j])), j
        assert np.all(np.isfinite(y)) and np.all(v >= 0.0)
        ref = O.fit_fixed(xs[0], ys[0], np.full(d, theta), mean=CO.MEANS[mean], corr=CO.CORRS[corr])
        _check_oracle(ref, xq[0], y[0], v[0])
    finally:
        for h in hs:
            h.close()


def test_run_is_shortened_not_the_chunk(egx, O):
    """n_pad = 1024, m = 16389: a chunk of the lone call is 16384 queries (its (m x n_pad) block is 2^27 / 8 doubles), so eight
    members' blocks fill the 1 GiB of a run and nine consecutive members answer as a run of eight and a run of one; the
    last five queries are a second chunk.  Still every member's bits are its own call's."""
    k, n, d, m = 9, 1000, 2, 16389
    xs, ys = _sets(k, n, d, seed=500)
    hs = egx.GpHandle.create_group(xs, ys)
    try:
        egx.finalize_multi(hs, np.full((k, d), 50.0))
        xq = _queries(k, m, d, seed=3)
        y, v = egx.predict_valvar_multi(hs, xq)
        for j, h in enumerate(hs):
            yl, vl = h.predict_valvar(xq[j])
            assert np.array_equal(y[j], yl), j
            assert np.array_equal(v[j], vl), j
        rows = np.r_[0:40, m - 40:m]  # both chunks
        _check_oracle(O.fit_fixed(xs[0], ys[0], np.full(d, 50.0)), xq[0][rows], y[0][rows], v[0][rows])
    finally:
        for h in hs:
            h.close()


def test_mixed_list_out_of_slot_order(egx):
    """Two lone handles among the members of a group, the members out of slot order (slots 0 and 1 still form a run of two):
    every block equals its own lone call."""
    k, n, d, m = 5, 150, 3, 37
    xs, ys = _sets(k + 2, n, d, seed=7)
    hs = egx.GpHandle.create_group(xs[:k], ys[:k], mean=0, corr=0)
    lone = [egx.GpHandle(xs[k + j], ys[k + j], mean=0, corr=0) for j in range(2)]
    try:
        egx.finalize_multi(hs, np.full((k, d), 1.0))
        for h in lone:
            h.finalize(np.full(d, 1.0))
        order = [hs[2], lone[0], hs[0], hs[1], lone[1], hs[4], hs[3]]
        xq = _queries(len(order), m, d, seed=11)
        y, v = egx.predict_valvar_multi(order, xq)
        for j, h in enumerate(order):
            yl, vl = h.predict_valvar(xq[j])
            assert np.array_equal(y[j], yl), j
            assert np.array_equal(v[j], vl), j
        with pytest.raises(egx.InvalidValueError):
            egx.predict_valvar_multi([hs[0], hs[0]], xq[:2])
    finally:
        for h in hs + lone:
            h.close()


def test_unfitted_member_is_reported_after_the_others(egx):
    xs, ys = _sets(3, 40, 2, seed=9)
    hs = egx.GpHandle.create_group(xs, ys)
    try:
        egx.finalize_multi(hs[:2], np.full((2, 2), 2.0))
        with pytest.raises(egx.NotFittedError):
            egx.predict_valvar_multi(hs, _queries(3, 9, 2, seed=1))
    finally:
        for h in hs:
            h.close()


# ------------------------------------------------------------------ 2. few queries against the oracle
@pytest.mark.parametrize("m", [1, 8])
def test_few_queries_against_oracle(egx, O, m):
    """m <= 8: the group still takes the batched route (no C^-T cache per member), the lone call may not -- the oracle's bar."""
    k, n, d = 6, 60, 2
    xs, ys = _sets(k, n, d, seed=20)
    theta = np.full(d, 2.0)
    hs = egx.GpHandle.create_group(xs, ys)
    try:
        egx.finalize_multi(hs, np.tile(theta, (k, 1)))
        xq = _queries(k, m, d, seed=m)
        y, v = egx.predict_valvar_multi(hs, xq)
        for j in range(k):
            _check_oracle(O.fit_fixed(xs[j], ys[j], theta), xq[j], y[j], v[j])
    finally:
        for h in hs:
            h.close()


# ------------------------------------------------------------------ 3. folds against the oracle
def test_folds_against_oracle_and_q2_formula(egx, O):
    from egobox_amd import workload
    x, y = workload.make_training_set(53, 2, seed=3)
    y = np.asarray(y).reshape(-1)
    theta = np.full(2, 2.0)
    params = egx.GaussianProcess.params(egx.ConstantMean(), egx.SquaredExponentialCorr()).theta_tuning(egx.ThetaTuning.Fixed(theta))
    folds = egx.cross_validate(params, x, y, 5, want_var=True)
    ref_folds = CO.oracle_folds(O, x, y, 5, theta)
    assert len(folds) == 5
    for f, (ref, tr, va) in zip(folds, ref_folds):
        assert tr.size == 43 and va.size == 10
        np.testing.assert_array_equal(f.valid, va)
        np.testing.assert_array_equal(f.theta, theta)
        _check_oracle(ref, x[va], f.pred, f.var)
    gp = params.fit(x, y)
    try:
        preds, vars_, valids = [f.pred for f in folds], [f.var for f in folds], [f.valid for f in folds]
        assert gp.q2_k_score(5) == CO.q2(preds, valids, y)
        assert gp.pva_k_score(5) == CO.pva(preds, vars_, valids, y)
        plot = egx.IaeAlphaPlotData()
        score, alphas, cover = CO.iae_alpha(preds, vars_, valids, y)
        assert gp.iae_alpha_k_score(5, plot) == pytest.approx(score, abs=1e-12)
        np.testing.assert_allclose(plot.alphas, alphas, atol=1e-15)
        np.testing.assert_allclose(plot.deltas, cover, atol=1e-12)
    finally:
        gp.close()


# ------------------------------------------------------------------ 4. leave-one-out
def test_leave_one_out(egx, O):
    from egobox_amd import workload
    x, y = workload.make_training_set(30, 1, seed=4)
    y = np.asarray(y).reshape(-1)
    theta = np.array([10.0])
    params = egx.GaussianProcess.params().theta_tuning(egx.ThetaTuning.Fixed(theta))
    gp = params.fit(x, y)
    try:
        before = egx.pool_stats()["cached_bytes"]
        q2 = gp.q2_score()
        after_one = egx.pool_stats()["cached_bytes"]
        assert q2 == gp.q2_k_score(30)
        assert gp.pva_score() == gp.pva_k_score(30)
        after = egx.pool_stats()["cached_bytes"]
        folds = egx.cross_validate(params, x, y, 30, want_var=True)
        assert len(folds) == 30
        for f, (ref, tr, va) in zip(folds, CO.oracle_folds(O, x, y, 30, theta)):
            assert tr.size == 29 and f.pred.shape == (1,)
            _check_oracle(ref, x[va], f.pred, f.var)
        # What the closed members leave in the pool is ONE batch of 30 members, and the later calls adopt it instead of adding
        # to it.  A member of 29 rows (n_pad = rhs_pad = 128) holds, in doubles: its slot of the matrix slab (n_pad + rhs_pad) x
        # n_pad = 32768, the tile inverses 2 x 2 x 4096 = 16384, the 256 x 256 inverse block of the back-substitution with its
        # tail 65536 + 132, and a few n_pad-long vectors (inputs twice, right-hand-side rows, gamma, rho, coefficients: < 2048)
        # -- 0.89 MiB.  One MiB a member bounds one batch; two batches do not fit under it.
        print("pool bytes", before, after_one, after)
        assert after_one - before <= 30 * (1 << 20)
        assert after <= after_one
    finally:
        gp.close()


# ------------------------------------------------------------------ 5. the lock-step engine equals the loop
def test_engine_equals_loop_of_tuned_fits(egx):
    from egobox_amd import workload
    x, y = workload.make_training_set(60, 2, seed=5)
    y = np.asarray(y).reshape(-1)
    params = egx.GaussianProcess.params().n_start(3)  # ThetaTuning.Full by default
    assert params._theta_tuning.kind == "Full"
    folds = egx.cross_validate(params, x, y, 5, want_var=True)
    loop = egx.GaussianProcess.params().n_start(3).n_workspaces(1)
    for f, (tr, va) in zip(folds, egx.fold_indices(60, 5)):
        assert va.size == 12
        gp = loop.fit(x[tr], y[tr])
        try:
            yl, vl = gp.predict_valvar(x[va])
            assert np.array_equal(f.theta, gp.theta())
            assert np.array_equal(f.pred, yl)
            assert np.array_equal(f.var, vl)
        finally:
            gp.close()


# ------------------------------------------------------------------ 6. selection
def _f_abs(x):
    x = np.asarray(x, dtype=np.float64).ravel()
    return np.abs(x - 0.37) + x * x


def test_selection_against_oracle(egx, O):
    """y = |x - 0.37| + x^2 on 40 points of [0, 1], theta = 10 for every pair: the oracle's best pair (Quadratic_SquaredExponential)
    leads its second best by 2.2e-2 relative (found on the CPU with the oracle alone; the condition is > 1e-3), the smallest pivot
    of its sixty fold fits is 0.45."""
    x = np.linspace(0.0, 1.0, 40).reshape(-1, 1)
    y = _f_abs(x)
    theta = np.array([10.0])
    table_ref, winner_ref, scale = CO.error_table(O, x, y, theta)
    errs = sorted(e for _, e in table_ref)
    assert (errs[1] - errs[0]) / errs[0] > 1e-3
    builder = egx.GpMixture.params().expert_specs(egx.RegressionSpec.ALL, egx.CorrelationSpec.ALL)
    winner, table = builder.select_expert(x, y, theta_tuning=egx.ThetaTuning.Fixed(theta))
    assert [n for n, _ in table] == [n for n, _ in table_ref]
    for (name, e), (_, er), s in zip(table, table_ref, scale):
        print(name, e, er)
        assert abs(e - er) <= PRED_RTOL * s, name  # the prediction bar through the triangle inequality
    assert winner == winner_ref


def test_selection_nx2_keeps_the_fold_count_quirk(egx):
    from egobox_amd import workload
    x, y = workload.make_training_set(40, 2, seed=6)
    builder = egx.GpMixture.params().expert_specs(egx.RegressionSpec.ALL, egx.CorrelationSpec.ALL)
    winner, table = builder.select_expert(x, np.asarray(y).reshape(-1), theta_tuning=egx.ThetaTuning.Fixed(np.full(2, 2.0)))
    assert len(table) == 12
    for name, e in table:
        assert math.isinf(e) == (not name.startswith("Constant_")), name
    assert winner.startswith("Constant_")


def _f_test_1d(x):  # crates/moe/src/algorithm.rs:1175-1188
    x = np.asarray(x, dtype=np.float64).ravel()
    return np.where(x < 0.4, x * x, np.where(x < 0.8, 3.0 * x + 1.0, np.sin(10.0 * x)))


def test_mixture_with_selected_experts(egx):
    xt = np.linspace(0.0, 1.0, 60).reshape(-1, 1)
    yt = _f_test_1d(xt)
    fixed = egx.ThetaTuning.Fixed(np.array([10.0]))
    builder = egx.GpMixture.params().n_clusters(2).expert_specs(egx.RegressionSpec.ALL, egx.CorrelationSpec.ALL) \
        .recombination("hard").theta_tunings([fixed]).selection_tuning(fixed).seed(0)
    moe = builder.fit(xt, yt)
    assert len(moe.expert_errors_) == 2 and all(len(t) == 12 for t in moe.expert_errors_)
    xq = np.linspace(0.02, 0.98, 17).reshape(-1, 1)
    from egobox_amd import gpx
    for e, table in zip(moe.experts, moe.expert_errors_):
        cx, cy = e.training_data
        winner, again = builder.select_expert(cx, cy)
        assert again == table
        assert f"{gpx._SURROGATE_NAME[str(e.params_._mean)]}_{gpx._SURROGATE_NAME[str(e.params_._corr)]}" == winner
        direct = egx.GaussianProcess.params(type(e.params_._mean)(), type(e.params_._corr)()).theta_tuning(fixed).fit(cx, cy)
        try:
            assert np.array_equal(direct.predict(xq), e.predict(xq))
        finally:
            direct.close()


# ------------------------------------------------------------------ 7. the reference's own sanity test (metrics.rs:239-262)
def test_reference_style_sanity(egx, O):
    """y = sum x^2 on 20 LHS points of [-10, 10]^2, default mixture parameters: q2_k_score(10) within 1e-3 of 1 and pva_k_score(10)
    within 0.2 of 0, the reference's own epsilons.  The design is a numpy LHS (oracle lhs_classic, seed 1), not the reference's
    Xoshiro stream.  For this seed the oracle, fitted at the theta* the GPU reports per fold, gives q2 = 0.99999993511 and
    pva = 0.1034 (GPU: 0.99999993490 and 0.0999); of the seeds 0 .. 5 tried, 1 and 5 meet both bounds in the oracle."""
    x = -10.0 + 20.0 * O.lhs_classic(20, 2, 1)
    y = np.sum(x * x, axis=1)
    moe = egx.GpMixture.params().fit(x, y)
    q2, pva = moe.q2_k_score(10), moe.pva_k_score(10)
    print("q2", q2, "pva", pva)
    assert abs(q2 - 1.0) <= 1e-3
    assert abs(pva) <= 2e-1
