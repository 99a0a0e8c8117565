"""Sparse GP as a full surrogate on the GPU: analytic x-gradients, predict_valvar and sampling through the C ABI, held to the
closed form built from the CPU oracle (tests/test_sgp_surrogate_cpu.py pins that closed form against central differences).
Tolerance unless said otherwise: the project's prediction bar, rtol 1e-6 and atol 1e-6 max|ref| (test_gpu_parity._grad_tol)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

from test_sgp_surrogate_cpu import KINDS, analytic_gradients, problem

pytestmark = pytest.mark.gpu

PRED_RTOL = 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def S():
    from oracle import sgp_oracle
    return sgp_oracle


def solve_route(S, ref, xq, x, y):
    """(W kx, var_raw) of the oracle's model through the four triangular solves instead of the explicit w_inv.  A reproduction
    aid, called by no test: with _oracle_routes below it produced the oracle-against-itself tables beside the constants."""
    nz = ref.z.shape[0]
    kmm = S.compute_k(ref.corr, ref.z, ref.z, ref.w_star, ref.theta, ref.sigma2) + np.eye(nz) * ref.nugget
    v = sla.solve_triangular(np.linalg.cholesky(kmm), S.compute_k(ref.corr, ref.z, x, ref.w_star, ref.theta, ref.sigma2), lower=True)
    u = np.linalg.cholesky(kmm)
    if ref.method == S.FITC:
        beta, s = 1.0 / (ref.sigma2 - (v * v).sum(axis=0) + ref.noise), -1.0
    else:
        beta, s = np.full(x.shape[0], 1.0 / max(ref.noise, ref.nugget)), 1.0
    l_ = np.linalg.cholesky(np.eye(nz) + (v * beta[None, :]) @ v.T)
    kx = S.compute_k(ref.corr, ref.z, xq, ref.w_star, ref.theta, ref.sigma2)  # (nz, m)
    a = sla.solve_triangular(u, kx, lower=True)
    b = sla.solve_triangular(l_, a, lower=True)
    c = sla.solve_triangular(u.T, a + s * sla.solve_triangular(l_.T, b, lower=False), lower=False)
    return c.T, ref.sigma2 - (a * a).sum(axis=0) - s * (b * b).sum(axis=0)


def compare_gradients(h, ref, xq, label):
    """The three gradient entry points against the closed form of the oracle; returns the reference for further use."""
    gy_ref, gv_ref, var_raw = analytic_gradients(ref, xq)
    gy, gv = h.predict_gradients(xq), h.predict_var_gradients(xq)
    gy2, gv2 = h.predict_valvar_gradients(xq)
    np.testing.assert_array_equal(gy, gy2)
    np.testing.assert_array_equal(gv, gv2)
    keep = np.abs(var_raw - 1e-15) >= 1e-7 * ref.sigma2  # the clamp decision is the oracle's beyond doubt
    clamped = keep & (var_raw < 1e-15)
    print(f"{label}: left out {(~keep).sum()} of {keep.size}, clamped {clamped.sum()}, "
          f"mean err {np.abs(gy - gy_ref).max():.3g} of {np.abs(gy_ref).max():.3g}, "
          f"var err {np.abs(gv - gv_ref)[keep].max():.3g} of {np.abs(gv_ref).max():.3g}")
    assert (~keep).sum() <= 0.01 * keep.size
    np.testing.assert_allclose(gy, gy_ref, rtol=PRED_RTOL, atol=1e-6 * np.abs(gy_ref).max())
    np.testing.assert_allclose(gv[keep], gv_ref[keep], rtol=PRED_RTOL, atol=1e-6 * np.abs(gv_ref).max())
    assert np.all(gv[clamped] == 0.0)
    return gy_ref, gv_ref, var_raw


# ------------------------------------------------------------------ 4. gradients vs the analytic oracle
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", range(4))
def test_gradients_vs_analytic_oracle(egx, S, corr, method):
    x, y, z = problem(700, 40, 3, seed=corr)
    theta, sigma2, noise = np.array([1.3, 0.8, 1.1]), 0.9, 0.02
    ref = S.SparseGpOracle(x, y, z, theta, sigma2, noise, corr=KINDS[corr], method=[S.FITC, S.VFE][method])
    xq = np.random.default_rng(9).random((333, 3)) * 2 - 1
    with egx.SgpHandle(x, y, z, corr=corr, method=method) as h:
        h.finalize(theta, sigma2, noise)
        _, _, var_raw = compare_gradients(h, ref, xq, f"corr {corr} method {method}")
        if corr == 0 and method == 1:
            assert (var_raw < 1e-15).sum() > 50  # the clamp is exercised (102 queries where this was written)


# ------------------------------------------------------------------ 5. more than one block, larger d
# n = 2000 training points in [-1, 1]^d, queries likewise, sigma2 = 1.3, noise = 0.01, default nugget; theta such that the
# correlation between neighbours stays informative at that d: theta_k = 2 / sqrt(d) (Matern-5/2), 1.5 / sqrt(d) (squared
# exponential).  Oracle against itself on the CPU (explicit w_inv vs the four triangular solves), FP64, as
# max|c_1 - c_2| relative to max|gradient| and max|var_raw_1 - var_raw_2| / sigma2, measured where this was written:
#   (nz, d, corr, method)   gradient      var_raw     within 1e-7 sigma2 of the clamp / clamped, of 1000
#   (300, 8, M52, FITC)     1.3e-13       6.2e-14     0 / 0
#   (300, 8, M52, VFE)      1.6e-13       5.4e-14     0 / 0
#   (300, 8, SqExp, FITC)   3.5e-11       5.6e-12     0 / 0
#   (300, 8, SqExp, VFE)    6.4e-11       1.3e-11     0 / 5
#   (300, 32, M52, FITC)    8.2e-15       2.7e-15     0 / 0
#   (300, 32, M52, VFE)     6.8e-15       2.1e-15     0 / 0
#   (300, 32, SqExp, FITC)  1.6e-13       4.6e-14     0 / 0
#   (300, 32, SqExp, VFE)   2.9e-13       8.6e-14     0 / 0
#   (1100, 8, M52, FITC)    1.9e-12       9.9e-13     0 / 0
#   (1100, 8, M52, VFE)     2.4e-12       9.5e-13     0 / 0
#   (1100, 8, SqExp, FITC)  1.2e-11       4.7e-12     0 / 0      (theta_k = 2.5 / sqrt(d), see below)
#   (1100, 8, SqExp, VFE)   1.1e-11       4.4e-12     0 / 6      (theta_k = 2.5 / sqrt(d))
#   (1100, 32, M52, FITC)   3.1e-14       1.3e-14     0 / 0
#   (1100, 32, M52, VFE)    3.4e-14       1.3e-14     0 / 0
#   (1100, 32, SqExp, FITC) 1.9e-12       4.3e-13     0 / 0
#   (1100, 32, SqExp, VFE)  3.1e-12       7.4e-13     0 / 0
# every case within 1e-8 of itself, none leaves a query out (_oracle_routes below reproduces the table on a CPU).  1100 inducing
# points in 8 dimensions sit close together: with 1.5 / sqrt(d) the squared-exponential oracle disagrees with itself by 6.8e-9
# (FITC) / 5.3e-8 (VFE, all 1000 queries clamped), outside the 1e-8 asked for; 2.5 / sqrt(d) is used for that pair.
LARGE_CASES = [(nz, d, corr, method) for nz in (300, 1100) for d in (8, 32) for corr in (3, 0) for method in (0, 1)]


def large_problem(nz, d, corr):
    x, y, z = problem(2000, nz, d, seed=100 + nz + d)
    theta = np.full(d, (2.0 if corr == 3 else 2.5 if (nz, d) == (1100, 8) else 1.5) / np.sqrt(d))
    xq = np.random.default_rng(nz + d).random((1000, d)) * 2 - 1
    return x, y, z, theta, 1.3, 0.01, xq


def _oracle_routes(S, nz, d, corr, method, prob=None):
    """Reproduction aid (CPU only, called by no test): the row of the tables above / below for one case."""
    from oracle import gp_oracle as O
    x, y, z, theta, sigma2, noise, xq = prob if prob is not None else large_problem(nz, d, corr)
    ref = S.SparseGpOracle(x, y, z, theta, sigma2, noise, corr=KINDS[corr], method=[S.FITC, S.VFE][method])
    kx = S.compute_k(ref.corr, xq, ref.z, ref.w_star, ref.theta, ref.sigma2)
    c1 = kx @ ref.w_inv
    v1 = sigma2 - (c1 * kx).sum(axis=1)
    c2, v2 = solve_route(S, ref, xq, x, y)
    g1, g2 = np.empty(xq.shape), np.empty(xq.shape)
    for a in range(xq.shape[0]):
        jac = O.corr_jacobian(ref.corr, xq[a], ref.z, ref.theta, ref.w_star)
        g1[a], g2[a] = -2 * sigma2 * (c1[a] @ jac), -2 * sigma2 * (c2[a] @ jac)
    near = (np.abs(v1 - 1e-15) < 1e-7 * sigma2).sum()
    return np.abs(g1 - g2).max() / np.abs(g1).max(), np.abs(v1 - v2).max() / sigma2, near, (v1 < 1e-15).sum()


@pytest.mark.parametrize("nz,d,corr,method", LARGE_CASES)
def test_gradients_more_than_one_block_and_larger_d(egx, S, nz, d, corr, method):
    x, y, z, theta, sigma2, noise, xq = large_problem(nz, d, corr)
    ref = S.SparseGpOracle(x, y, z, theta, sigma2, noise, corr=KINDS[corr], method=[S.FITC, S.VFE][method])
    with egx.SgpHandle(x, y, z, corr=corr, method=method) as h:
        h.finalize(theta, sigma2, noise)
        compare_gradients(h, ref, xq, f"nz {nz} d {d} corr {corr} method {method}")


# ------------------------------------------------------------------ 6. few queries = rows of a large batch
# Up to 16 queries per call take the few-query route (c = W kx in row form by two passes over the cached inverse factors, the
# contraction with the lanes over the inducing points); above, the batched route, where the padding (128 queries per tile), the
# number of splits of the inducing points and the GEMM shapes change with m: same FP64 arithmetic in another order.  All four
# kernels, both methods (cond(Kmm) of these inputs: 1.8e6 for the squared exponential, the largest of the four).
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", range(4))
def test_few_queries_equal_rows_of_a_large_batch(egx, S, corr, method):
    x, y, z = problem(700, 40, 3, seed=corr)
    theta, sigma2, noise = np.array([1.3, 0.8, 1.1]), 0.9, 0.02
    xq = np.random.default_rng(9).random((333, 3)) * 2 - 1
    ref = S.SparseGpOracle(x, y, z, theta, sigma2, noise, corr=KINDS[corr], method=[S.FITC, S.VFE][method])
    _, _, var_raw = analytic_gradients(ref, xq)
    sure = np.abs(var_raw - 1e-15) >= 1e-7 * sigma2
    clamped = np.flatnonzero(sure & (var_raw < 1e-15))
    if len(clamped) >= 8:  # put clamped queries among the first sixteen (and the first eight): the few-query route must mask them too
        free = np.flatnonzero(sure & (var_raw >= 1e-15))
        order = np.concatenate([clamped[:2], free[:2], clamped[2:4], free[2:12], clamped[4:8], free[12:]])
        order = np.concatenate([order, np.setdiff1d(np.arange(xq.shape[0]), order)])
        xq, var_raw, sure = xq[order], var_raw[order], sure[order]
    if corr == 0 and method == 1:
        assert (var_raw[:8] < 1e-15).sum() == 4  # the case with 102 clamped queries
    with egx.SgpHandle(x, y, z, corr=corr, method=method) as h:
        h.finalize(theta, sigma2, noise)
        big = h.predict_valvar(xq) + h.predict_valvar_gradients(xq)
        for m in (1, 2, 3, 8, 15, 16, 17, 128, 129):  # the switch-over is at 16; 128 queries fill one tile
            small = h.predict_valvar(xq[:m]) + h.predict_valvar_gradients(xq[:m])
            for name, a, b in zip(("mean", "var", "dmean", "dvar"), small, big):
                err = np.abs(a - b[:m]).max()
                print(f"corr {corr} method {method} m {m} {name}: {err:.3g} of {np.abs(b).max():.3g}")
                np.testing.assert_allclose(a, b[:m], rtol=1e-9, atol=1e-9 * np.abs(b).max())
            rows = np.flatnonzero(sure[:m] & (var_raw[:m] < 1e-15))
            assert np.all(small[3][rows] == 0.0) and np.all(small[1][rows] == 1e-15 + noise)
            live = np.flatnonzero(sure[:m] & (var_raw[:m] >= 1e-15))
            assert np.all(np.abs(small[3][live]).max(axis=1) > 0.0)
        # one point at a time allocates nothing on the device after the first call
        h.predict_valvar_gradients(xq[:1])
        h.predict_valvar(xq[:1])
        before = egx.pool_stats()
        for i in range(100):
            h.predict_valvar(xq[i:i + 1])
            h.predict_valvar_gradients(xq[i:i + 1])
        assert egx.pool_stats()["misses"] == before["misses"]


# ------------------------------------------------------------------ 6b. an ill-conditioned Kmm, both routes
# The squared-exponential problem of item 4 with theta scaled by 0.75: cond(Kmm) = 3.4e7 (1.8e6 at scale 1), the most
# ill-conditioned Kmm on these inputs for which the oracle still agrees with itself to 1e-8 (explicit w_inv against the four
# triangular solves, CPU, FP64; gradient relative to the largest component / var_raw relative to sigma2 / clamped of 333):
#   scale  cond(Kmm)  FITC                   VFE
#   1.0    1.8e6      8.0e-11 / 2.1e-11 / 0  1.3e-10 / 3.4e-11 / 102
#   0.8    1.7e7      6.5e-10 / 6.7e-11 / 0  4.9e-9  / 3.9e-10 / 232
#   0.75   3.4e7      4.3e-9  / 3.5e-10 / 0  9.3e-9  / 5.9e-10 / 270
#   0.7    6.8e7      5.9e-9  / 3.8e-10 / 0  3.8e-8  / 1.2e-9  / 300
#   0.6    3.3e8      2.2e-8  / 6.9e-10 / 0  3.3e-7  / 6.5e-9  / 333
#   0.4    1.9e10     4.2e-6  / 6.6e-8  / 0  2.0e-5  / 3.9e-7  / 333
#   0.2    1.6e13     5.6e-3  / 5.5e-5  / 0  2.2e-2  / 3.5e-4  / 306
# no query within 1e-7 sigma2 of the clamp in any row.  Beyond 1e8 the REFERENCE no longer resolves the 1e-6 bar (the quantity
# itself is that sensitive to the rounding of Kmm), so nothing can be held to it there: the explicit inverse factors are
# tested up to the conditioning the oracle can vouch for, not beyond.
@pytest.mark.parametrize("method", [0, 1])
def test_gradients_on_an_ill_conditioned_kmm(egx, S, method):
    x, y, z = problem(700, 40, 3, seed=0)
    theta, sigma2, noise = 0.75 * np.array([1.3, 0.8, 1.1]), 0.9, 0.02
    ref = S.SparseGpOracle(x, y, z, theta, sigma2, noise, corr=KINDS[0], method=[S.FITC, S.VFE][method])
    xq = np.random.default_rng(9).random((333, 3)) * 2 - 1
    with egx.SgpHandle(x, y, z, corr=0, method=method) as h:
        h.finalize(theta, sigma2, noise)
        gy_ref, gv_ref, var_raw = compare_gradients(h, ref, xq, f"ill-conditioned, method {method}, batched")
        keep = np.abs(var_raw - 1e-15) >= 1e-7 * sigma2
        for i0 in range(0, 32, 8):  # ... and the few-query route (up to 16 per call) on the same model
            gy, gv = h.predict_valvar_gradients(xq[i0:i0 + 8])
            k = keep[i0:i0 + 8]
            np.testing.assert_allclose(gy, gy_ref[i0:i0 + 8], rtol=PRED_RTOL, atol=1e-6 * np.abs(gy_ref).max())
            np.testing.assert_allclose(gv[k], gv_ref[i0:i0 + 8][k], rtol=PRED_RTOL, atol=1e-6 * np.abs(gv_ref).max())
            assert np.all(gv[k & (var_raw[i0:i0 + 8] < 1e-15)] == 0.0)


# ------------------------------------------------------------------ 7. predict_valvar = predict, predict_var
@pytest.mark.parametrize("method", [0, 1])
def test_valvar_bit_equals_the_two_calls(egx, S, method):
    x, y, z = problem(700, 40, 3, seed=3)
    rng = np.random.default_rng(11)
    theta, sigma2, noise = np.array([1.3, 0.8, 1.1]), 0.9, 0.02
    with egx.SgpHandle(x, y, z, corr=3, method=method) as h:
        h.finalize(theta, sigma2, noise)
        for m in (1, 7, 333, 70000):
            xq = rng.random((m, 3)) * 2 - 1
            yv, vv = h.predict_valvar(xq)
            np.testing.assert_array_equal(yv, h.predict(xq))
            np.testing.assert_array_equal(vv, h.predict_var(xq))
    # the three calls share the chunk loop of 65536 queries: the rows on both sides of its edge against the oracle as well
    # (the bars of test_sgp_gpu.py; none of these rows is within 1e-7 sigma2 of the variance clamp, on the oracle alone)
    rows = slice(65530, 65546)
    ref = S.SparseGpOracle(x, y, z, theta, sigma2, noise, corr=KINDS[3], method=[S.FITC, S.VFE][method])
    _, _, var_raw = analytic_gradients(ref, xq[rows])
    assert np.all(np.abs(var_raw - 1e-15) >= 1e-7 * sigma2)
    np.testing.assert_allclose(yv[rows], ref.predict(xq[rows]), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(vv[rows], ref.predict_var(xq[rows]), rtol=1e-6, atol=1e-9)


# ------------------------------------------------------------------ 8. against the reference's own definition
def test_analytic_agrees_with_the_central_differences(egx):
    """The problem and the tolerances of test_sgp_gpu.py::test_numerical_gradients_like_the_reference."""
    x, y, z = problem(400, 25, 2, seed=2)
    theta, sigma2, noise = np.array([1.1, 0.9]), 1.0, 0.02
    sgp = egx.SparseGaussianProcess(egx.SgpHandle(x, y, z, corr=3), egx.SgpParams(egx.Matern52Corr(), egx.Inducings.Located(z)))
    sgp._h.finalize(theta, sigma2, noise)
    xq = np.random.default_rng(3).random((7, 2)) - 0.5
    np.testing.assert_allclose(sgp.predict_gradients(xq, analytic=True), sgp.predict_gradients(xq), rtol=2e-5, atol=5e-6)
    np.testing.assert_allclose(sgp.predict_var_gradients(xq, analytic=True), sgp.predict_var_gradients(xq), rtol=2e-5, atol=5e-5)
    gy, gv = sgp.predict_valvar_gradients(xq)
    np.testing.assert_array_equal(gy, sgp.predict_gradients(xq, analytic=True))
    np.testing.assert_array_equal(gv, sgp.predict_var_gradients(xq, analytic=True))
    yv, vv = sgp.predict_valvar(xq)
    np.testing.assert_array_equal(yv, sgp.predict(xq))
    np.testing.assert_array_equal(vv, sgp.predict_var(xq))
    sgp.close()


# ------------------------------------------------------------------ 9. sampling
def _sample_model(egx, corr, m=500):
    x, y, z = problem(700, 40, 3, seed=corr)
    theta, sigma2, noise = np.array([1.3, 0.8, 1.1]), 0.9, 0.02
    h = egx.SgpHandle(x, y, z, corr=corr)
    h.finalize(theta, sigma2, noise)
    xq = np.random.default_rng(21).random((m, 3)) * 2 - 1
    return h, xq, theta, sigma2


@pytest.mark.parametrize("corr", [1, 2])
def test_sample_factor_is_the_prior_covariance(egx, S, corr):
    """z = I: traj - mean is the lower Cholesky factor of sigma2 r(xq, xq), the PRIOR covariance (the reference's definition:
    no noise, no Woodbury term).  Condition of the 500 x 500 prior: 3e3 (absolute exponential), 3e6 (Matern-3/2)."""
    h, xq, theta, sigma2 = _sample_model(egx, corr)
    with h:
        m = xq.shape[0]
        t, tau = h.sample(xq, m, "cholesky", z=np.eye(m), return_tau=True)
        assert tau == 0.0
        f = t - h.predict(xq)[:, None]
        assert np.all(np.triu(f, 1) == 0.0)
        k = S.compute_k(KINDS[corr], xq, xq, np.eye(3), theta, sigma2)
        print(f"corr {corr}: |F F^T - K| {np.abs(f @ f.T - k).max():.3g}, cond {np.linalg.cond(k):.3g}")
        np.testing.assert_allclose(f @ f.T, k, rtol=0, atol=1e-9 * sigma2)
        # the library's stream: traj = mean + F Z(seed), and the first columns do not depend on n_traj
        lib = egx._lib.load()
        zz = np.empty((m, 6))
        egx._lib.check(lib.egx_random_normals(-1, 77, m, 6, egx._lib.dptr(zz)))
        a = h.sample(xq, 6, "cholesky", seed=77)
        np.testing.assert_allclose(a, h.predict(xq)[:, None] + f @ zz, rtol=1e-12, atol=1e-12 * np.sqrt(sigma2))
        np.testing.assert_array_equal(h.sample(xq, 6, "cholesky", seed=5, z=zz), a)
        np.testing.assert_array_equal(h.sample(xq, 12, "cholesky", seed=77)[:, :6], a)
        assert h.sample(xq[:0], 3).shape == (0, 3) and h.sample(xq, 0).shape == (m, 0)


def test_sample_psd_on_an_ill_conditioned_prior(egx, S):
    """Squared-exponential prior of the same 500 points: condition 2e18, numpy's Cholesky fails.  EGX_SAMPLE_PSD succeeds and
    reports tau; F F^T - K stays within the bound documented for egx_gp_sample (tau + 1e-12 |K|).  EGX_SAMPLE_CHOLESKY either
    succeeds or names the pivot: a matter of rounding, not asserted (as test_gpu_sample.py::test_psd_sample_reference_case)."""
    h, xq, theta, sigma2 = _sample_model(egx, 0)
    with h:
        m = xq.shape[0]
        t, tau = h.sample(xq, m, "psd", z=np.eye(m), return_tau=True)
        assert tau >= 1e-9
        f = t - h.predict(xq)[:, None]
        k = S.compute_k(KINDS[0], xq, xq, np.eye(3), theta, sigma2)
        nrm = np.linalg.norm(k, 2)
        print(f"tau {tau:.3g}, |F F^T - K|_2 {np.linalg.norm(f @ f.T - k, 2):.3g}")
        assert np.linalg.norm(f @ f.T - k, 2) <= tau + 1e-12 * nrm
        try:
            assert h.sample(xq, 3, "cholesky").shape == (m, 3)
        except egx.LinalgError as e:
            assert "pivot" in str(e)
        sgp = egx.SparseGaussianProcess(h, None)
        assert sgp.sample(xq, 4, seed=1).shape == (m, 4)
        np.testing.assert_array_equal(sgp.sample(xq, 4, seed=1), sgp.sample_eig(xq, 4, seed=1))


def test_sample_moments(egx):
    """20000 trajectories at 16 points: sample mean and variance within five standard errors of predict(xq) and of sigma2
    -- the PRIOR variance, by the reference's definition of the sparse GP's sample."""
    h, xq, theta, sigma2 = _sample_model(egx, 3, m=16)
    with h:
        nt = 20000
        t = h.sample(xq, nt, "psd", seed=2024)
        mean = h.predict(xq)
        se_mean = np.sqrt(sigma2 / nt)
        assert np.all(np.abs(t.mean(axis=1) - mean) <= 5 * se_mean)
        se_var = sigma2 * np.sqrt(2.0 / (nt - 1))
        assert np.all(np.abs(t.var(axis=1, ddof=1) - sigma2) <= 5 * se_var)


# ------------------------------------------------------------------ 10. life cycle
def test_life_cycle(egx, tmp_path):
    x, y, z = problem(700, 40, 3, seed=3)
    xq = np.random.default_rng(4).random((50, 3)) * 2 - 1
    with egx.SgpHandle(x, y, z, corr=3) as h:
        for call in (h.predict_valvar, h.predict_gradients, h.predict_var_gradients, h.predict_valvar_gradients,
                     lambda q: h.sample(q, 2)):
            with pytest.raises(egx.NotFittedError):
                call(xq)
        h.finalize(np.array([1.3, 0.8, 1.1]), 0.9, 0.02)
        g1 = h.predict_valvar_gradients(xq) + h.predict_valvar_gradients(xq[:1])
        h.finalize(np.array([0.6, 1.7, 0.9]), 1.2, 0.03)
        g2 = h.predict_valvar_gradients(xq) + h.predict_valvar_gradients(xq[:1])
        assert not np.allclose(g1[1], g2[1]) and not np.allclose(g1[0], g2[0])
        h.likelihood(np.array([1.0, 1.0, 1.0]), 1.0, 0.01)  # an evaluation un-fits the handle
        with pytest.raises(egx.NotFittedError):
            h.predict_valvar_gradients(xq)
    with egx.SgpHandle(x, y, z, corr=3) as fresh:
        fresh.finalize(np.array([0.6, 1.7, 0.9]), 1.2, 0.03)
        g3 = fresh.predict_valvar_gradients(xq) + fresh.predict_valvar_gradients(xq[:1])
    for a, b in zip(g2, g3):
        np.testing.assert_array_equal(a, b)
    # SparseGpx.save / load: the problem and the tolerance of test_sgp_gpu.py::test_sparse_gpx_save_load_roundtrip
    x, y, z = problem(500, 20, 2, seed=4)
    gx = egx.SparseGpx.builder(z=z, n_start=0, max_eval=30, method=egx.SparseMethod.VFE).fit(x, y)
    xq = np.random.default_rng(5).random((40, 2)) * 2 - 1
    g0 = gx.predict_valvar_gradients(xq)
    path = tmp_path / "sgp.json"
    assert gx.save(str(path))
    back = egx.SparseGpx.load(str(path))
    for a, b in zip(back.predict_valvar_gradients(xq), g0):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9 * np.abs(b).max())
    np.testing.assert_array_equal(back.predict_gradients(xq, analytic=True), back.predict_valvar_gradients(xq)[0])
    assert back.sample(xq, 3, seed=1).shape == (40, 3) and back.sample_chol(xq[:5], 2, seed=1).shape == (5, 2)


def test_c_host_drives_the_surrogate_entry_points(tmp_path):
    """tests/c_host/sgp_surrogate_driver.c: the five entry points from plain C."""
    exe = tmp_path / "sgp_surrogate_driver"
    libdir = os.path.join(ROOT, "egobox_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "c_host", "sgp_surrogate_driver.c"), f"-L{libdir}", "-legx_gp_hip", "-lm",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert out.stdout.startswith("OK")
