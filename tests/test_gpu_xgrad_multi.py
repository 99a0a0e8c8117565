"""Posterior x-gradients of a group in lock-step (egx_gp_predict_valvar_gradients_multi): every member's d mean / d x and
d var / d x, bit for bit, against its own predict_valvar_gradients -- the member is a grid coordinate of k_xgrad and of the
weight GEMMs, the splits of the training range come from one member's shape, the chunks are the lone call's -- and one case
against the CPU oracle, so that the two cannot be wrong together.

Shapes: k = 5, n = 150, d = 3 (n_pad 256, a tail slab of 22 points); k = 17, n = 70, d = 2 (two runs, 16 + 1); k = 3, n = 100,
d = 70 (the d > 64 form, query coordinates from global memory).  m = 37 is one tile of 128 with the training range split,
m = 300 three tiles, the last partial.  Every m is > 8, where the lone call takes the batched route."""
import numpy as np
import pytest

import cv_oracle as CO
from test_gpu_parity import _grad_tol

pytestmark = pytest.mark.gpu

SQEXP, ABSEXP, MATERN52 = 0, 1, 3
MS = (37, 300)


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


def _close(hs):
    for h in hs:
        h.close()


def _assert_blocks_equal_lone(egx, hs, xq):
    """both arrays, and each alone, of every handle of the list against its own call"""
    k, m, d = xq.shape
    gy, gv = egx.predict_valvar_gradients_multi(hs, xq)
    gy_only, none_v = egx.predict_valvar_gradients_multi(hs, xq, want_var=False)
    none_y, gv_only = egx.predict_valvar_gradients_multi(hs, xq, want_val=False)
    assert none_v is None and none_y is None
    assert gy.shape == (k, m, d) and gv.shape == (k, m, d)
    for j, h in enumerate(hs):
        ly, lv = h.predict_valvar_gradients(xq[j])
        assert np.array_equal(gy[j], ly), j
        assert np.array_equal(gv[j], lv), j
        assert np.array_equal(gy_only[j], ly), j
        assert np.array_equal(gv_only[j], lv), j
    assert np.all(np.isfinite(gy)) and np.all(np.isfinite(gv))
    return gy, gv


# every shape x every kernel x every trend the shape admits (a quadratic trend in 70 inputs has 2556 columns, more than the 100
# points); theta by shape and kernel so that the factorisation is well posed
KERNELS = (SQEXP, ABSEXP, MATERN52)
CASES = [(5, 150, 3, mean, corr, 1.0 if corr == SQEXP else 2.0) for corr in KERNELS for mean in (0, 1, 2)] + \
        [(17, 70, 2, mean, corr, 5.0 if corr == SQEXP else 3.0) for corr in KERNELS for mean in (0, 1, 2)] + \
        [(3, 100, 70, mean, corr, 0.1) for corr in KERNELS for mean in (0, 1)]


@pytest.mark.parametrize("k,n,d,mean,corr,theta", CASES)
def test_lockstep_equals_lone(egx, k, n, d, mean, corr, theta):
    xs, ys = _sets(k, n, d, seed=300 + n)
    hs = egx.GpHandle.create_group(xs, ys, mean=mean, corr=corr)
    try:
        egx.finalize_multi(hs, np.full((k, d), theta))
        for m in MS:
            _assert_blocks_equal_lone(egx, hs, _queries(k, m, d, seed=n + m))
    finally:
        _close(hs)


def test_first_members_against_oracle(egx, O):
    k, n, d, m, mean, corr, theta = 5, 150, 3, 37, 1, SQEXP, 1.0
    xs, ys = _sets(k, n, d, seed=300 + n)
    hs = egx.GpHandle.create_group(xs, ys, mean=mean, corr=corr)
    try:
        egx.finalize_multi(hs, np.full((k, d), theta))
        xq = _queries(k, m, d, seed=5)
        gy, gv = egx.predict_valvar_gradients_multi(hs, xq)
        for j in (0, k - 1):
            ref = O.fit_fixed(xs[j], ys[j], np.full(d, theta), mean=CO.MEANS[mean], corr=CO.CORRS[corr])
            assert np.diag(ref.inner.r_chol).min() > 1e-3
            ry, rv = ref.predict_valvar_gradients(xq[j])
            np.testing.assert_allclose(gy[j], ry, **_grad_tol(ry))
            np.testing.assert_allclose(gv[j], rv, **_grad_tol(rv))
    finally:
        _close(hs)


def test_mixed_list(egx):
    """Two members of a group, a foreign lone handle, two members of another group with another n, and a KPLS + Matern model
    (several coefficient columns per input: served alone) -- every block is its own lone call's."""
    d, m = 3, 37
    xa, ya = _sets(3, 150, d, seed=40)
    xb, yb = _sets(2, 100, d, seed=50)
    xl, yl = _sets(2, 120, d, seed=60)
    ga = egx.GpHandle.create_group(xa, ya, mean=1, corr=MATERN52)
    gb = egx.GpHandle.create_group(xb, yb, mean=1, corr=MATERN52)
    lone = egx.GpHandle(xl[0], yl[0], mean=1, corr=MATERN52)
    w = np.random.default_rng(2).standard_normal((d, 2))
    kpls = egx.GpHandle(xl[1], yl[1], mean=1, corr=MATERN52, w_star=w)
    hs = ga + gb + [lone, kpls]
    try:
        egx.finalize_multi(ga, np.full((3, d), 2.0))
        egx.finalize_multi(gb, np.full((2, d), 2.0))
        lone.finalize(np.full(d, 2.0))
        kpls.finalize(np.array([0.7, 0.4]))
        order = [ga[0], ga[1], lone, gb[0], gb[1], kpls, ga[2]]
        _assert_blocks_equal_lone(egx, order, _queries(len(order), m, d, seed=13))
    finally:
        _close(hs)


def test_unfitted_member_is_reported_after_the_others(egx):
    xs, ys = _sets(3, 40, 2, seed=9)
    hs = egx.GpHandle.create_group(xs, ys)
    try:
        egx.finalize_multi(hs[:2], np.full((2, 2), 2.0))
        with pytest.raises(egx.NotFittedError):
            egx.predict_valvar_gradients_multi(hs, _queries(3, 9, 2, seed=1))
    finally:
        _close(hs)
