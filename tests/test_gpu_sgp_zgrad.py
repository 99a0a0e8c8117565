"""The sparse GP's likelihood gradient in the inducing points (egx_sgp_likelihood_grad_z), moving the points
(egx_sgp_set_inducings / _get_inducings) and the fit that uses both (egx_sgp_fit_lbfgs_z) on the GPU: against the numpy
restatement by dense algebra (tests/sgp_zgrad_oracle.py), against central differences of the GPU's own likelihood, and against
egx_sgp_fit_lbfgs on a twin handle.  Gradient bar: the theta-gradient's own (tests/test_gpu_sgp_grad.py), rtol 1e-6 with atol
1e-6 max |want| over the whole matrix -- it rests on the same pair weights -- at shapes whose R_zz is conditioned below 1e8."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sgp_grad_oracle as GO  # noqa: E402
import sgp_zgrad_oracle as ZO  # noqa: E402
from test_gpu_sgp_grad import SHAPES, SIGMA2, NOISE, T3, _problem, _shape  # noqa: E402

pytestmark = pytest.mark.gpu

# (n, nz, d, theta, sigma2, noise, kernels) beyond SHAPES -- what each reaches is in the ids
MORE = {
    "one-point-one-dimension": (50, 1, 1, np.array([1.3]), SIGMA2, NOISE, range(4)),
    "41-row-tiles-second-col-tile-of-one": (2561, 65, 2, np.array([4.0, 3.0]), SIGMA2, NOISE, range(4)),
    "79x5-tiles-runs-of-two-row-tiles": (5000, 300, 6, np.full(6, 0.7), 1.3, 0.01, [3]),
}
CASES = [(name, corr) for name in SHAPES for corr in range(4)] + [(name, corr) for name in MORE for corr in MORE[name][6]]


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


_more = {}


def _case(name):
    if name in SHAPES:
        return _shape(name) + (SIGMA2, NOISE)
    if name not in _more:
        n, nz, d, theta, s2, nv, _ = MORE[name]
        _more[name] = _problem(n, nz, d, seed=n) + (theta, s2, nv)
    return _more[name]


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("name,corr", CASES)
def test_grad_z_matches_the_restatement(egx, name, corr, method):
    """The inducing points of these problems are rows of x: the absolute exponential meets its kink (sgn(0) = 0) here too."""
    x, y, z, theta, sigma2, noise = _case(name)
    nugget = egx.gp.DEFAULT_NUGGET
    cond = GO.zz_condition(corr, z, theta, sigma2, nugget)
    assert cond <= 1e8, cond
    want = ZO.likelihood_grad_z(corr, method, x, y, z, theta, sigma2, noise, nugget)
    with egx.SgpHandle(x, y, z, corr=corr, method=method) as h:
        lk0, g0, st0 = h.likelihood_grad(theta, sigma2, noise)
        lk, g, gz, st = h.likelihood_grad_z(theta, sigma2, noise)
    dev = np.abs(gz - want).max() / np.abs(want).max()
    print(f"corr {corr} method {method} n {x.shape[0]} nz {z.shape[0]} d {x.shape[1]}: cond {cond:.2e}, "
          f"max |got - want| / max |want| = {dev:.3e}")
    assert st0 == 0 and st == 0 and lk == lk0  # bit for bit
    np.testing.assert_array_equal(g, g0)
    assert gz.shape == z.shape
    np.testing.assert_allclose(gz, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())


def _off_row_problem():
    rng = np.random.default_rng(130)
    x = 2 * rng.random((130, 3)) - 1
    y = np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, -1]) + 0.05 * rng.standard_normal(130)
    z = 2 * rng.random((70, 3)) - 1
    v = rng.standard_normal((70, 3))
    return x, y, z, v / np.linalg.norm(v)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", range(4))
def test_directional_derivative_matches_the_gpus_own_likelihood(egx, corr, method):
    """Independent of the restatement: central difference of `likelihood` at Z +- 1e-4 V (through set_inducings) along a random
    direction V with |V|_F = 1, against sum gz o V at rel 1e-5, the bar of the theta-gradient's directional test (on the CPU
    oracle this draw gives <= 1.4e-6 for all eight pairs)."""
    x, y, z, v = _off_row_problem()
    with egx.SgpHandle(x, y, z, corr=corr, method=method) as h:
        _, _, gz, st = h.likelihood_grad_z(T3, SIGMA2, NOISE)
        h.set_inducings(z + 1e-4 * v)
        lp, sp = h.likelihood(T3, SIGMA2, NOISE)
        h.set_inducings(z - 1e-4 * v)
        lm, sm = h.likelihood(T3, SIGMA2, NOISE)
    assert st == 0 and sp == 0 and sm == 0
    fd = (lp - lm) / 2e-4
    an = float((gz * v).sum())
    print(f"corr {corr} method {method}: central difference {fd:.10g}, sum gz o V {an:.10g}")
    assert an == pytest.approx(fd, rel=1e-5)


@pytest.mark.parametrize("method", [0, 1])
def test_same_bits_on_every_call_and_after_moving_the_points_back(egx, method):
    x, y, z, theta = _shape("A-two-row-tiles+2-one-col-tile+6")
    with egx.SgpHandle(x, y, z, corr=2, method=method) as h:
        r1 = h.likelihood_grad_z(theta, SIGMA2, NOISE)
        r2 = h.likelihood_grad_z(theta, SIGMA2, NOISE)
        h.likelihood(0.5 * theta, 1.7, 0.1)
        r3 = h.likelihood_grad_z(theta, SIGMA2, NOISE)
        h.set_inducings(0.9 * z + 0.01)
        r4 = h.likelihood_grad_z(theta, SIGMA2, NOISE)
        h.set_inducings(z)
        r5 = h.likelihood_grad_z(theta, SIGMA2, NOISE)
    for r in (r2, r3, r5):
        assert r[0] == r1[0] and r[3] == 0
        np.testing.assert_array_equal(r[1], r1[1])
        np.testing.assert_array_equal(r[2], r1[2])
    assert np.all(np.isfinite(r1[2])) and np.all(r1[2] != 0.0)
    assert r4[3] == 0 and r4[0] != r1[0] and np.all(r4[2] != r1[2])


def test_set_and_get_inducings(egx):
    x, y, z = _problem(200, 10, 2, seed=200)
    z2 = 0.8 * z + 0.05
    args = ([1.0, 1.2], 1.0, 0.01)
    with egx.SgpHandle(x, y, z) as h, egx.SgpHandle(x, y, z2) as fresh:
        np.testing.assert_array_equal(h.inducings(), z)
        h.finalize(*args)
        h.predict(x[:2])
        h.set_inducings(z2)
        np.testing.assert_array_equal(h.inducings(), z2)
        np.testing.assert_array_equal(h.z, z2)
        with pytest.raises(egx.NotFittedError):
            h.predict(x[:2])
        h.finalize(*args)
        fresh.finalize(*args)
        np.testing.assert_array_equal(h.predict(x[:50]), fresh.predict(x[:50]))
        np.testing.assert_array_equal(h.predict_var(x[:50]), fresh.predict_var(x[:50]))
        assert h.state()["likelihood"] == fresh.state()["likelihood"]
        bad = z.copy()
        bad[3, 1] = np.nan
        with pytest.raises(egx.InvalidValueError):
            h.set_inducings(bad)
        with pytest.raises(egx.InvalidValueError):
            h.set_inducings(z[:5])
        np.testing.assert_array_equal(h.inducings(), z2)  # the handle is as it was: still fitted, the same points
        np.testing.assert_array_equal(h.predict(x[:50]), fresh.predict(x[:50]))
        lk, g, gz, st = h.likelihood_grad_z([float("nan"), 1.0], 1.0, 0.01)
        assert st == egx._lib.STATUS_NAN_THETA and lk == -np.inf and np.all(g == 0.0) and np.all(gz == 0.0)
        assert gz.shape == (10, 2)


def _fit_args(y, d):
    s20 = float(np.var(y, ddof=1))
    lo, hi = [1e-2] * d + [1e-12, 1e-10], [1e2] * d + [9.0 * s20, 1.0]
    return np.array([[1.0] * d + [s20, 1e-2]]), lo, hi


def test_fit_lbfgs_z_without_phase_two_is_fit_lbfgs(egx):
    x, y, z = _problem(200, 10, 2, seed=200)
    p0, lo, hi = _fit_args(y, 2)
    with egx.SgpHandle(x, y, z, corr=3) as h, egx.SgpHandle(x, y, z, corr=3) as twin:
        ne = h.fit_lbfgs_z(p0, lo, hi, True, 1e-2, max_iter_z=0)
        ne_t = twin.fit_lbfgs(p0, lo, hi, True, 1e-2)
        a, b = h.state(with_inv=True), twin.state(with_inv=True)
        assert ne == ne_t and a.keys() == b.keys()
        for k in a:
            np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(h.inducings(), z)
        np.testing.assert_array_equal(h.predict(x[:64]), twin.predict(x[:64]))
        np.testing.assert_array_equal(h.predict_var(x[:64]), twin.predict_var(x[:64]))
        assert h.likelihood(a["theta"], a["sigma2"], a["noise"]) == twin.likelihood(b["theta"], b["sigma2"], b["noise"])


@pytest.mark.parametrize("method", [0, 1])
def test_fit_lbfgs_z_never_ends_below_fit_lbfgs(egx, method):
    """Default max_iter_z on a Randomized-like draw: the likelihood is at least the twin's (Armijo never accepts worse, and phase
    two is kept only where it gains), the state is the keeping evaluation at the returned points, every point is in the box."""
    x, y, z = _problem(700, 40, 3, seed=700)
    p0, lo, hi = _fit_args(y, 3)
    with egx.SgpHandle(x, y, z, corr=2, method=method) as h, egx.SgpHandle(x, y, z, corr=2, method=method) as twin:
        ne = h.fit_lbfgs_z(p0, lo, hi, True, 1e-2)
        ne_t = twin.fit_lbfgs(p0, lo, hi, True, 1e-2)
        st, lk_t = h.state(), twin.state()["likelihood"]
        zf = h.inducings()
        print(f"method {method}: fit_lbfgs {lk_t:.6f} ({ne_t} evaluations), fit_lbfgs_z {st['likelihood']:.6f} ({ne})")
        assert st["likelihood"] >= lk_t and ne > ne_t
        np.testing.assert_array_equal(h.z, zf)
        assert np.all(zf >= x.min(axis=0)) and np.all(zf <= x.max(axis=0))
        assert np.all(np.isfinite(h.predict(x[:3])))
        with egx.SgpHandle(x, y, zf, corr=2, method=method) as again:
            lk, s = again.likelihood(st["theta"], st["sigma2"], st["noise"])
        assert s == 0 and st["likelihood"] == pytest.approx(lk, rel=1e-12)


def test_fit_lbfgs_z_moves_points_out_of_a_corner(egx):
    """Built to need the points to move: all twelve start in [-1, -0.8]^2 of [-1, 1]^2."""
    rng = np.random.default_rng(600)
    x = 2 * rng.random((600, 2)) - 1
    y = np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, 1])
    z = -1.0 + 0.2 * rng.random((12, 2))
    p0, lo, hi = _fit_args(y, 2)
    with egx.SgpHandle(x, y, z, corr=2) as h, egx.SgpHandle(x, y, z, corr=2) as twin:
        h.fit_lbfgs_z(p0, lo, hi, True, 1e-2, z_lo=[-1.0, -1.0], z_hi=[1.0, 1.0])
        twin.fit_lbfgs(p0, lo, hi, True, 1e-2)
        lk, lk_t, zf = h.state()["likelihood"], twin.state()["likelihood"], h.inducings()
    print(f"fit_lbfgs {lk_t:.6f}, fit_lbfgs_z {lk:.6f}, points outside the corner: {int((zf.max(axis=1) > -0.8).sum())} of 12")
    assert lk > lk_t
    assert np.any(zf.max(axis=1) > -0.8)
    assert np.all(zf >= -1.0) and np.all(zf <= 1.0)


def test_fit_lbfgs_z_holds_a_fixed_column(egx):
    x, y, z = _problem(200, 10, 2, seed=200)
    z = z.copy()
    z[:, 1] = 0.25
    p0, lo, hi = _fit_args(y, 2)
    with egx.SgpHandle(x, y, z, corr=2) as h:
        h.fit_lbfgs_z(p0, lo, hi, True, 1e-2, z_lo=[-1.0, 0.25], z_hi=[1.0, 0.25])
        zf = h.inducings()
        np.testing.assert_array_equal(zf[:, 1], z[:, 1])
        assert np.any(zf[:, 0] != z[:, 0]) and np.all(np.abs(zf[:, 0]) <= 1.0)
        with pytest.raises(egx.InvalidValueError):
            h.fit_lbfgs_z(p0, lo, hi, True, 1e-2, z_lo=[1.0, 0.0], z_hi=[-1.0, 1.0])
        with pytest.raises(egx.InvalidValueError):
            h.fit_lbfgs_z(p0, lo, hi, True, 1e-2, z_lo=[-1.0, -1.0])


def test_optimize_inducings_end_to_end(egx, tmp_path):
    from egobox_amd import sgp as SG

    x, y, _ = _problem(700, 40, 3, seed=700)
    draw = x[np.random.default_rng(5).permutation(700)[:20]]
    sgp = SG.SgpParams(egx.gp.Matern32Corr(), SG.Inducings.Randomized(20)).seed(5).n_start(0).optimizer("lbfgs") \
        .optimize_inducings().fit(x, y)
    plain = SG.SgpParams(egx.gp.Matern32Corr(), SG.Inducings.Randomized(20)).seed(5).n_start(0).optimizer("lbfgs").fit(x, y)
    np.testing.assert_array_equal(plain.inducings(), draw)  # the default is unchanged
    assert sgp.inducings().shape == (20, 3) and not np.array_equal(sgp.inducings(), draw)
    assert sgp.likelihood() > plain.likelihood()
    sgp.close()
    plain.close()
    gpx = SG.SparseGpx.builder(corr_spec=4, nz=20, seed=5, n_start=0, optimizer="lbfgs", optimize_inducings=True).fit(x, y)
    assert not np.array_equal(gpx._sgp.inducings(), draw)
    path = tmp_path / "sgp_moved.json"
    gpx.save(str(path))
    back = SG.SparseGpx.load(str(path))
    np.testing.assert_array_equal(back._sgp.inducings(), gpx._sgp.inducings())
    np.testing.assert_array_equal(back.predict(x[:100]), gpx.predict(x[:100]))
    np.testing.assert_array_equal(back.predict_var(x[:100]), gpx.predict_var(x[:100]))
    gpx._sgp.close()
    back._sgp.close()
    with pytest.raises(egx.InvalidValueError, match="lbfgs"):
        SG.SgpParams(egx.gp.Matern32Corr(), SG.Inducings.Randomized(20)).optimize_inducings().fit(x, y)
    with pytest.raises(egx.InvalidValueError, match="lbfgs"):
        SG.SparseGpx.builder(corr_spec=4, nz=20, optimize_inducings=True).fit(x, y)
