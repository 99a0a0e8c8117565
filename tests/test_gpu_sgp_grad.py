"""The sparse GP's closed-form likelihood gradient (egx_sgp_likelihood_grad) and the L-BFGS fit on it (egx_sgp_fit_lbfgs) on
the GPU, against the numpy restatement by dense algebra (tests/sgp_grad_oracle.py), against central differences of the GPU's
own likelihood, and against scipy's L-BFGS-B on the CPU oracle.  Gradient bar: the dense gradient's own
(tests/test_gpu_configs.py), rtol 1e-6 with atol 1e-6 max |want|, at shapes whose R_zz is conditioned below 1e8."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sgp_grad_oracle as GO  # noqa: E402

pytestmark = pytest.mark.gpu

SIGMA2, NOISE = 0.9, 0.02
T3 = np.array([1.3, 0.8, 1.1])
# name: (n, nz, d, theta) -- what each reaches is in the ids
SHAPES = {
    "A-two-row-tiles+2-one-col-tile+6": (130, 70, 3, T3),
    "B-pinned-likelihood-shape": (700, 40, 3, T3),
    "C-z_pad-256-two-chol-blocks": (300, 130, 4, 1.5 * np.array([1.3, 0.8, 1.1, 1.3])),
    "D-second-staging-chunk": (200, 20, 65, np.full(65, 0.25)),
    "E-sixteen-wide-output-chunk": (130, 70, 9, np.full(9, 0.8)),
    "F-sum-output-alone-in-its-chunk": (200, 20, 96, np.full(96, 0.05)),
}


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


def _problem(n, nz, d, seed=0, noise=0.05):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d)) * 2 - 1
    y = np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, -1]) + noise * rng.standard_normal(n)
    z = x[rng.permutation(n)[:nz]].copy()
    return x, y, z


_problems = {}


def _shape(name):
    if name not in _problems:
        n, nz, d, theta = SHAPES[name]
        _problems[name] = _problem(n, nz, d, seed=n) + (theta,)
    return _problems[name]


def _check_grad(egx, corr, method, x, y, z, theta, sigma2, noise):
    nugget = egx.gp.DEFAULT_NUGGET
    cond = GO.zz_condition(corr, z, theta, sigma2, nugget)
    assert cond <= 1e8, cond
    want = GO.likelihood_grad(corr, method, x, y, z, theta, sigma2, noise, nugget)
    with egx.SgpHandle(x, y, z, corr=corr, method=method) as h:
        lk0, st0 = h.likelihood(theta, sigma2, noise)
        lk, got, st = h.likelihood_grad(theta, sigma2, noise)
    from oracle import sgp_oracle as S
    lk_ref = S.SparseGpOracle(x, y, z, theta, sigma2, noise, corr=GO.KINDS[corr], method=[S.FITC, S.VFE][method], nugget=nugget).likelihood
    dev = np.abs(got - want).max() / np.abs(want).max()
    print(f"corr {corr} method {method} n {x.shape[0]} nz {z.shape[0]} d {x.shape[1]}: cond {cond:.2e}, "
          f"max |got - want| / max |want| = {dev:.3e}, likelihood off the oracle by {abs(lk0 - lk_ref) / abs(lk_ref):.3e}")
    assert st0 == 0 and st == 0 and lk == lk0  # bit for bit
    assert lk0 == pytest.approx(lk_ref, rel=1e-8)  # ... and the value itself, not only the two calls' agreement
    assert got.shape == (x.shape[1] + 2,)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", range(4))
@pytest.mark.parametrize("name", list(SHAPES))
def test_gradient_matches_the_restatement(egx, name, corr, method):
    x, y, z, theta = _shape(name)
    _check_grad(egx, corr, method, x, y, z, theta, SIGMA2, NOISE)


@pytest.mark.parametrize("method", [0, 1])
def test_gradient_larger_shape_with_split_gram_products(egx, method):
    """nz = 300 (z_pad = 384), n = 5000: several K splits of the Gram products, 79 x 5 tiles of the rectangle."""
    x, y, z = _problem(5000, 300, 6, seed=5000)
    _check_grad(egx, 3, method, x, y, z, np.full(6, 0.7), 1.3, 0.01)


@pytest.mark.parametrize("method", [0, 1])
def test_directional_derivative_matches_the_gpus_own_likelihood(egx, method):
    """Independent of the restatement: central difference of `likelihood` at p +- 1e-4 p o v along a random unit direction v
    in (theta, sigma2, noise), against grad . (p o v) at rtol 1e-5 (truncation ~1e-8 relative, rounding eps |L| / 2e-4 ~ 1e-9)."""
    x, y, z, theta = _shape("B-pinned-likelihood-shape")
    p = np.concatenate([theta, [SIGMA2, NOISE]])
    v = np.random.default_rng(7).standard_normal(p.size)
    v /= np.linalg.norm(v)
    with egx.SgpHandle(x, y, z, corr=0, method=method) as h:
        _, g, st = h.likelihood_grad(theta, SIGMA2, NOISE)
        pp, pm = p * (1.0 + 1e-4 * v), p * (1.0 - 1e-4 * v)
        lp, sp = h.likelihood(pp[:3], pp[3], pp[4])
        lm, sm = h.likelihood(pm[:3], pm[3], pm[4])
    assert st == 0 and sp == 0 and sm == 0
    fd = (lp - lm) / 2e-4
    an = float(g.dot(p * v))
    print(f"method {method}: central difference {fd:.10g}, grad . (p o v) {an:.10g}")
    assert an == pytest.approx(fd, rel=1e-5)


@pytest.mark.parametrize("method", [0, 1])
def test_same_bits_on_every_call(egx, method):
    x, y, z, theta = _shape("A-two-row-tiles+2-one-col-tile+6")
    with egx.SgpHandle(x, y, z, corr=2, method=method) as h:
        lk1, g1, _ = h.likelihood_grad(theta, SIGMA2, NOISE)
        lk2, g2, _ = h.likelihood_grad(theta, SIGMA2, NOISE)
        h.likelihood(0.5 * theta, 1.7, 0.1)
        lk3, g3, _ = h.likelihood_grad(theta, SIGMA2, NOISE)
    assert lk1 == lk2 == lk3
    np.testing.assert_array_equal(g1, g2)
    np.testing.assert_array_equal(g1, g3)
    assert np.all(np.isfinite(g1)) and np.all(g1 != 0.0)


def test_status_and_edges(egx):
    x, y, z = _problem(200, 10, 2, seed=200)
    L = egx._lib
    with egx.SgpHandle(x, y, z) as h:
        for args in (([float("nan"), 1.0], 1.0, 0.01), ([1.0, 1.0], -1.0, 0.01), ([1.0, 1.0], 0.0, 0.01)):
            lk, g, st = h.likelihood_grad(*args)
            assert st == L.STATUS_NAN_THETA and lk == -np.inf and g.shape == (4,) and np.all(g == 0.0)
        _, g1, st1 = h.likelihood_grad([0.8], 1.1, 0.03)
        _, g2, st2 = h.likelihood_grad([0.8, 0.8], 1.1, 0.03)
        assert st1 == 0 and st2 == 0
        np.testing.assert_array_equal(g1, g2)
        h.finalize([1.0, 1.0], 1.0, 0.01)
        h.predict(x[:2])
        h.likelihood_grad([1.0, 1.0], 1.0, 0.01)  # un-fits the handle, as `likelihood` does
        with pytest.raises(egx.NotFittedError):
            h.predict(x[:2])
        with pytest.raises(egx.InvalidValueError):
            h.likelihood_grad([1.0, 1.0, 1.0], 1.0, 0.01)
    zdup = np.vstack([z, z[:1]])  # duplicated inducing point, no nugget: Kmm singular
    with egx.SgpHandle(x, y, zdup, nugget=0.0) as h:
        lk, g, st = h.likelihood_grad([1.0, 1.0], 1.0, 0.01)
        assert (st == L.STATUS_NOT_POSITIVE_DEFINITE and lk == -np.inf and np.all(g == 0.0)) or \
            (st == 0 and np.isfinite(lk) and np.all(np.isfinite(g)))
    with egx.SgpHandle(x, y, z, method=1, nugget=1e-3) as h:  # VFE: the likelihood does not see a noise below the nugget
        for noise in (1e-4, 1e-3):
            lk, g, st = h.likelihood_grad([1.0, 1.0], 1.0, noise)
            assert st == 0 and g[3] == 0.0 and np.all(g[:3] != 0.0)
        assert h.likelihood_grad([1.0, 1.0], 1.0, 2e-3)[1][3] != 0.0


def test_fit_lbfgs_starts_fixed_noise_and_argument_checks(egx):
    """Starts run one after the other on the one workspace, each walking the points it walks alone: two starts end at the
    better of the two single-start fits, bit for bit, and the evaluations add up.  A fixed noise stays where it is."""
    x, y, z = _problem(200, 10, 2, seed=200)
    s20 = float(np.var(y, ddof=1))
    lo, hi = [1e-2, 1e-2, 1e-12, 1e-10], [1e2, 1e2, 9.0 * s20, 1.0]
    starts = np.array([[1.0, 1.0, s20, 1e-2], [5.0, 0.2, 0.5 * s20, 1e-3]])
    with egx.SgpHandle(x, y, z, corr=3) as h:
        single = []
        for p0 in starts:
            ne = h.fit_lbfgs(p0[None, :], lo, hi, True, 1e-2)
            single.append((h.state()["likelihood"], ne))
        ne = h.fit_lbfgs(starts, lo, hi, True, 1e-2, max_iter=0)  # < 1: the default 50
        st = h.state()
        assert st["likelihood"] == max(s[0] for s in single) and ne == single[0][1] + single[1][1]
        assert np.all(np.isfinite(h.predict(x[:3])))  # the keeping evaluation left a fitted handle
        assert st["likelihood"] > h.likelihood(starts[0, :2], starts[0, 2], starts[0, 3])[0]
        ne = h.fit_lbfgs(starts[:, :3], lo[:3], hi[:3], False, 2.5e-3)
        assert ne >= 2 and h.state()["noise"] == 2.5e-3
        with pytest.raises(egx.InvalidValueError):
            h.fit_lbfgs(starts, [0.0] + lo[1:], hi, True, 1e-2)
        with pytest.raises(egx.InvalidValueError):
            h.fit_lbfgs(-starts, lo, hi, True, 1e-2)


def _fit_reference(corr, x, y, z, p0, bounds, nugget):
    """scipy's L-BFGS-B on the CPU oracle's FITC likelihood with the restated gradient, over log10(params)."""
    from scipy.optimize import minimize

    from oracle import sgp_oracle as S

    d = x.shape[1]
    evals = [0]

    def fun(u):
        p = 10.0 ** u
        evals[0] += 1
        lk = S.fitc(GO.KINDS[corr], p[:d], p[d], p[d + 1], np.eye(d), x, y.reshape(-1, 1), z, nugget)[0]
        g = GO.likelihood_grad(corr, 0, x, y, z, p[:d], p[d], p[d + 1], nugget)
        return -lk, -p * np.log(10.0) * g

    u0 = np.log10(p0)
    l0 = -fun(u0)[0]
    r = minimize(fun, u0, jac=True, method="L-BFGS-B", bounds=[(np.log10(lo), np.log10(hi)) for lo, hi in bounds])
    return l0, -r.fun, 10.0 ** r.x, evals[0]


@pytest.mark.parametrize("corr", [2, 0])
def test_lbfgs_fit_against_scipy_on_the_oracle(egx, corr):
    """One start (theta = 1, sigma2 = var(y), noise 1e-2), the box SgpParams.fit builds, noise estimated, 200 iterations.  The
    fit must gain at least half of what scipy's L-BFGS-B gains on the CPU oracle from the same start (half: the two line
    searches differ), reproduce `likelihood` at the fitted parameters, and land the noise within a factor 5 of 0.05^2."""
    from egobox_amd import sgp as SG

    x, y, z, _ = _shape("B-pinned-likelihood-shape")
    d = x.shape[1]
    s20 = float(np.var(y, ddof=1))
    p0 = np.array([1.0] * d + [s20, 1e-2])
    bounds = [SG.DEFAULT_THETA_BOUNDS] * d + [(1e-12, 9.0 * s20), SG.DEFAULT_NOISE_BOUNDS]
    lo, hi = [b[0] for b in bounds], [b[1] for b in bounds]
    l0, l_ref, p_ref, ev_ref = _fit_reference(corr, x, y, z, p0, bounds, egx.gp.DEFAULT_NUGGET)

    def check(lk, noise, n_evals, what):
        print(f"corr {corr} {what}: L0 {l0:.4f}, reference {l_ref:.4f} ({ev_ref} evaluations, noise {p_ref[d + 1]:.3e}), "
              f"fitted {lk:.4f} ({n_evals} evaluations, noise {noise:.3e})")
        assert lk >= l0 + 0.5 * (l_ref - l0)
        assert 0.05 ** 2 / 5.0 <= noise <= 0.05 ** 2 * 5.0
        assert n_evals >= 2

    with egx.SgpHandle(x, y, z, corr=corr) as h:
        n_evals = h.fit_lbfgs(p0[None, :], lo, hi, True, 1e-2, max_iter=200)
        st = h.state()
        assert st["likelihood"] == pytest.approx(h.likelihood(st["theta"], st["sigma2"], st["noise"])[0], rel=1e-12)
        check(st["likelihood"], st["noise"], n_evals, "SgpHandle.fit_lbfgs")
    kind = egx.gp.Matern32Corr if corr == 2 else egx.gp.SquaredExponentialCorr
    # n_start 0: the one start is (theta_init, var(y), the default noise 1e-2), the start above
    sgp = SG.SgpParams(kind(), SG.Inducings.Located(z)).theta_init([1.0]).n_start(0).max_eval(800).optimizer("lbfgs").fit(x, y)
    check(sgp.likelihood(), sgp.noise_variance(), sgp.n_evals, "SgpParams.optimizer('lbfgs').fit")
    sgp.close()
    gpx = SG.SparseGpx.builder(corr_spec=4 if corr == 2 else 1, theta_init=[1.0], n_start=0, z=z, max_eval=800,
                               optimizer="lbfgs").fit(x, y)
    check(gpx.likelihoods()[0], gpx._sgp.noise_variance(), gpx._sgp.n_evals, "SparseGpx.builder(optimizer='lbfgs').fit")
    gpx._sgp.close()
    with pytest.raises(ValueError):
        SG.SgpParams(kind(), SG.Inducings.Located(z)).optimizer("newton")
