"""The host side of Egor without a device: the rules of the EGO loop (egobox_amd/egor.py) against the reference's own unit-test
literals (tests/golden/egor_kat.json), the samplers of egobox_amd/doe.py, and the constructor's refusals."""
import json
import os

import numpy as np
import pytest

import egobox_amd as egx
from egobox_amd import doe, egor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(7, 1), (10, 3), (33, 5)]


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(GOLDEN, "egor_kat.json")) as f:
        return json.load(f)


# ---- is_update_ok / update_data ----------------------------------------------------------------------------------------------
def test_is_update_ok_kat(kat):
    k = kat["is_update_ok"]
    for case in k["cases"]:
        assert egor.is_update_ok(k["x_data"], case["x_new"]) is case["ok"]
    # the threshold is 100 eps in L1, strict
    eps = np.finfo(float).eps
    assert egor.is_update_ok([[0.0, 0.0]], [60 * eps, 60 * eps])
    assert not egor.is_update_ok([[0.0, 0.0]], [40 * eps, 40 * eps])
    assert egor.is_update_ok(np.zeros((0, 2)), [0.0, 0.0])


def test_update_data_kat(kat):
    k = kat["update_data"]
    x, y, c, idx = egor.update_data(k["x_data"], k["y_data"], k["c_data"], k["x_new"], k["y_new"], k["c_new"])
    assert idx == k["appended"]
    assert np.array_equal(x, k["x_out"]) and np.array_equal(y, k["y_out"]) and np.array_equal(c, k["c_out"])
    # a batch that repeats itself: the second copy is checked against the first
    x, y, c, idx = egor.update_data(k["x_data"], k["y_data"], None, [[5.0, 5.0], [5.0, 5.0]], [[1.0], [2.0]], None)
    assert idx == [0] and c is None and x.shape == (3, 2) and y[-1, 0] == 1.0


# ---- start_points ------------------------------------------------------------------------------------------------------------
def test_start_points_kat(kat):
    k = kat["start_points"]
    xl, xu = k["xl"], k["xu"]
    got = egor.start_points(k["midpoint"]["x"], xl, xu)
    assert got.shape == (1, 2) and np.abs(got - np.array(k["midpoint"]["expected"])).max() <= k["midpoint"]["abs_tol"]
    assert egor.start_points(k["three_points"]["x"], xl, xu).shape[0] >= k["three_points"]["min_rows"]
    for case in k["n_max"]["cases"]:
        assert egor.start_points(k["n_max"]["x"], xl, xu, case["n_max"]).shape == (case["rows"], 2)


def test_start_points_third_point_closer_spoils_the_pair():
    """A training point nearer to a pair's midpoint than the pair's own points discards that midpoint.  The CLOSEST pair can never
    be spoiled (a point within d/2 of its midpoint would be within d of both ends: a closer pair), so with two rows or more the
    result is never empty; it is empty below two rows."""
    xl, xu = [0.0, 0.0], [1.0, 1.0]
    x = np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 0.01]])
    got = egor.start_points(x, xl, xu)
    # the long pair's midpoint (0.5, 0) has point 2 at 0.01, nearer than 0.5: dropped; the short pairs' midpoints stay
    assert got.shape == (2, 2) and not np.any(np.all(np.abs(got - [0.5, 0.0]) < 1e-12, axis=1))
    assert np.allclose(np.sort(got[:, 0]), [0.25, 0.75]) and np.allclose(got[:, 1], 0.005)
    # alone, the long pair gives its midpoint: the third point is what spoiled it
    assert np.allclose(egor.start_points(x[:2], xl, xu), [[0.5, 0.0]])
    # a start already kept spoils a later midpoint as well: the corners of a square give the four side midpoints, and the
    # diagonals' midpoint -- no corner is nearer to it than its own pair -- has those kept starts at 0.5 < 0.707
    sq = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    got4 = egor.start_points(sq, xl, xu)
    assert got4.shape == (4, 2) and not np.any(np.all(np.abs(got4 - 0.5) < 1e-12, axis=1))
    assert np.allclose(egor.start_points(sq[[0, 3]], xl, xu), [[0.5, 0.5]])
    # the metric is scaled by the limits: stretch an axis and its limits together, the picks follow
    st = egor.start_points(x * [10.0, 1.0], [0.0, 0.0], [10.0, 1.0])
    assert np.allclose(st, got_scaled(x, xl, xu))
    # below two rows there is no pair
    assert egor.start_points(np.array([[0.3, 0.4]]), xl, xu).shape == (0, 2)
    assert egor.start_points(np.zeros((0, 2)), xl, xu).shape == (0, 2)


def got_scaled(x, xl, xu):
    return egor.start_points(x, xl, xu) * [10.0, 1.0]


# ---- find_best_result_index / _from / is_feasible ------------------------------------------------------------------------------
def test_cstr_min_kat(kat):
    k = kat["cstr_min"]
    for case in k["cases"]:
        y1, y2 = np.array(case["y1"]), np.array(case["y2"])
        assert egor._cstr_less(y1, y2, k["cstr_tol"]) is (case["order"] < 0)
        assert egor._cstr_less(y2, y1, k["cstr_tol"]) is (case["order"] > 0)


def test_find_best_result_index_kat(kat):
    for case in kat["find_best"]:
        assert egor.find_best_result_index(case["y"], case["c"], case["cstr_tol"]) == case["index"]
    for case in kat["find_best_from"]:
        assert egor.find_best_result_index_from(case["current"], case["offset"], case["y"], case["c"], case["cstr_tol"]) == case["index"]


def test_find_best_result_index_branches():
    tol = [0.1, 0.1]
    # no feasible row: the smallest violation sum, whatever the objective
    y = np.array([[-9.0, 0.5, 0.5], [0.0, 0.2, 0.15], [-5.0, 0.1, 0.4]])
    assert egor.find_best_result_index(y, None, tol) == 1        # sums 0.8, 0.15, 0.3
    assert not egor.is_feasible(y[1], None, tol)
    # several feasible rows: the smallest objective among them, not the smallest overall
    y = np.array([[-9.0, 0.5, 0.0], [-1.0, 0.1, 0.1], [-2.0, -1.0, 0.05], [-2.0, 0.0, 0.0]])
    assert egor.find_best_result_index(y, None, tol) == 2        # (the first of the two rows at -2)
    assert egor.is_feasible(y[2], None, tol) and egor.is_feasible(y[1], None, tol)   # c == tol is inside
    # the unconstrained branch
    assert egor.find_best_result_index(np.array([[3.0], [-1.0], [2.0]]), None, []) == 1
    assert egor.find_best_result_index(np.array([3.0, -1.0, 2.0]), None, []) == 1
    assert egor.is_feasible([5.0], None, [])


def test_find_best_result_index_from_keeps_the_current_index():
    tol = [0.1]
    y = np.array([[-1.0, 0.0], [-3.0, 0.0], [-3.0, 0.0], [-2.0, 0.0], [-9.0, 0.3]])
    assert egor.find_best_result_index_from(1, 2, y, None, tol) == 1   # an equal row, a worse row, an infeasible better one
    assert egor.find_best_result_index_from(0, 1, y, None, tol) == 1   # the first strictly better row, then nothing better
    y2 = np.array([[-1.0, 0.5], [-1.0, 0.4], [5.0, 0.0]])
    assert egor.find_best_result_index_from(0, 1, y2, None, tol) == 2  # infeasible current: smaller violation, then feasible
    assert egor.find_best_result_index_from(0, 1, y2[:2], None, tol) == 1


# ---- the samplers --------------------------------------------------------------------------------------------------------------
def _strata(u, n):
    return np.sort(np.floor(u * n).astype(int), axis=0)


@pytest.mark.parametrize("n,nx", SHAPES)
@pytest.mark.parametrize("kind", doe.LHS_KINDS)
def test_lhs_kinds(kind, n, nx):
    lim = np.column_stack([np.linspace(-3.0, 2.0, nx), np.linspace(4.0, 9.0, nx)])
    x = egx.Lhs(lim, kind, seed=11).sample(n)
    assert x.shape == (n, nx)
    u = (x - lim[:, 0]) / (lim[:, 1] - lim[:, 0])
    assert np.all(u >= 0.0) and np.all(u < 1.0)
    assert np.array_equal(_strata(u, n), np.tile(np.arange(n)[:, None], (1, nx)))   # exactly one point per stratum and column
    if kind.startswith("centered"):
        assert np.abs(np.sort(u, axis=0) - ((np.arange(n) + 0.5) / n)[:, None]).max() < 1e-14
    assert np.array_equal(x, egx.Lhs(lim, kind, seed=11).sample(n))                  # the same seed, the same array
    assert not np.array_equal(x, egx.Lhs(lim, kind, seed=12).sample(n))
    s = egx.Lhs(lim, kind, seed=11)
    assert not np.array_equal(s.sample(n), s.sample(n))                              # one sampler goes on in its stream


@pytest.mark.parametrize("n,nx", SHAPES)
def test_lhs_optimized_does_not_lose_to_its_start(n, nx):
    lim = np.array([[0.0, 1.0]] * nx)
    start = doe.lhs_classic(n, nx, np.random.default_rng(5))    # what the optimized kind draws first from the same seed
    x = egx.Lhs(lim, "optimized", seed=5).normalized_sample(n)
    assert doe.phip(x) <= doe.phip(start)
    if nx > 1:
        assert doe.phip(x) < doe.phip(start)


def test_lhs_reuses_the_projects_classic_and_maximin():
    from egobox_amd import multistart
    lim = np.array([[0.0, 1.0]] * 3)
    assert np.array_equal(egx.Lhs(lim, "classic", seed=3).normalized_sample(9), multistart.lhs_classic(9, 3, np.random.default_rng(3)))
    assert np.array_equal(egx.Lhs(lim, "maximin", seed=3).normalized_sample(9),
                          multistart.lhs_maximin(9, 3, np.random.default_rng(3), tries=5))
    assert doe.lhs_classic is multistart.lhs_classic and doe.lhs_maximin is multistart.lhs_maximin


@pytest.mark.parametrize("n,nx", [(10, 3), (33, 5), (4, 2)])
def test_phip_swap_is_the_full_recomputation(n, nx):
    rng = np.random.default_rng(n * 100 + nx)
    x = doe.lhs_classic(n, nx, rng)
    cur = doe.phip(x)
    for s in range(20):
        before = x.copy()
        new = doe._phip_swap(x, s % nx, cur, doe.ESE_P, rng)
        full = doe.phip(x)
        assert abs(new - full) <= 1e-12 * full
        changed = np.argwhere(before != x)
        assert changed.shape[0] == 2 and set(changed[:, 1]) == {s % nx}               # two entries of one column, exchanged
        assert before[changed[0, 0], s % nx] == x[changed[1, 0], s % nx]
        cur = full


def test_full_factorial_and_random_stay_inside():
    lim = np.array([[5.0, 10.0], [0.0, 1.0]])
    ff = egx.FullFactorial(lim).sample(9)
    expect = np.array([[a, b] for a in (5.0, 7.5, 10.0) for b in (0.0, 0.5, 1.0)])
    assert np.abs(ff - expect).max() < 1e-12
    ff7 = egx.FullFactorial(lim).sample(7)
    assert ff7.shape == (7, 2) and np.array_equal(ff7, ff[:7])
    lim3 = np.array([[-1.0, 1.0], [2.0, 3.0], [0.0, 10.0]])
    for n in (1, 5, 8, 20):
        f = egx.FullFactorial(lim3).sample(n)
        assert f.shape == (n, 3) and np.all(f >= lim3[:, 0]) and np.all(f <= lim3[:, 1])
        assert np.unique(f, axis=0).shape[0] == n
    r = egx.Random(lim3, seed=1).sample(50)
    assert r.shape == (50, 3) and np.all(r >= lim3[:, 0]) and np.all(r < lim3[:, 1])
    assert np.array_equal(r, egx.Random(lim3, seed=1).sample(50))


def test_sampling_of_a_mixed_integer_space():
    xspecs = [egx.XType.Float(-1.0, 1.0), egx.XType.Int(2, 6), egx.XType.Enum(3), egx.XType.Ord([0.5, 2.0, 8.0])]
    for method in ("lhs", "lhs_classic", "lhs_centered", "lhs_maximin", "lhs_centered_maximin", "random", "full_factorial",
                   egx.Sampling.LHS):
        x = egx.sampling(method, xspecs, 12, seed=4)
        assert x.shape == (12, 4)
        assert np.all((x[:, 0] >= -1.0) & (x[:, 0] <= 1.0))
        assert set(x[:, 1]) <= {2.0, 3.0, 4.0, 5.0, 6.0}
        assert set(x[:, 2]) <= {0.0, 1.0, 2.0}
        assert set(x[:, 3]) <= {0.5, 2.0, 8.0}
    assert np.array_equal(egx.lhs(xspecs, 12, seed=4), egx.sampling("lhs", xspecs, 12, seed=4))
    lim = np.array([[0.0, 25.0]])
    assert np.array_equal(egx.lhs(lim, 6, seed=2), egx.Lhs(lim, "optimized", seed=2).sample(6))
    assert np.array_equal(egx.lhs([egx.XType.Float(0.0, 25.0)], 6, seed=2), egx.lhs(lim, 6, seed=2))
    with pytest.raises(egx.InvalidValueError):
        egx.sampling("sobol", lim, 4)
    with pytest.raises(egx.InvalidValueError):
        egx.Lhs(lim, "best")
    with pytest.raises(egx.InvalidValueError):
        egx.Lhs(np.zeros((2, 3)))
    with pytest.raises(egx.InvalidValueError):
        egx.Lhs(lim).sample(0)


# ---- the constructor -----------------------------------------------------------------------------------------------------------
def test_egor_defaults_are_the_reference_configs():
    e = egx.Egor(np.array([[0.0, 3.0], [0.0, 4.0]]), n_cstr=2)
    assert (e.n_start, e.n_doe, e.q_points, e.q_optmod, e.cstr_infill, e.cstr_strategy) == (20, 0, 1, 1, False, "mean")
    assert e.infill_strategy == egx.LOG_EI and e.infill_optimizer == "slsqp" and e.q_infill_strategy == egx.QEiStrategy.KB
    assert e.target == -np.finfo(float).max and e.seed is None
    assert np.array_equal(e.cstr_tol, [1e-4, 1e-4])
    g = e.gp_config
    assert (g.n_clusters, g.recombination, g.n_start, g.max_eval, g.kpls_dim) == (1, "smooth", 10, 50, None)
    assert g.regr_spec == egx.RegressionSpec.CONSTANT and g.corr_spec == egx.CorrelationSpec.SQUARED_EXPONENTIAL
    assert g.theta_init is None and g.theta_bounds is None
    assert egor.theta_bounds(None, 2, g.corr_spec) == [(1e-2, 1e1)]
    lo, hi = egor.theta_bounds(None, 12, g.corr_spec)[0]
    assert 0.0 < lo < 1e-2 * 10 and hi > lo
    assert egor.theta_bounds([(0.5, 2.0)], 12, g.corr_spec) == [(0.5, 2.0)]


def test_egor_refusals():
    lim = np.array([[0.0, 25.0]])
    bad = [dict(gp_config=egx.GpConfig(n_clusters=0)), dict(gp_config=egx.GpConfig(n_clusters=-2)),
           dict(doe=np.zeros((3, 3))), dict(doe=np.zeros((3, 4)), n_cstr=1),
           dict(doe=np.zeros((3, 2)), n_cstr=2, cstr_tol=[1e-3, 1e-3]), dict(doe=np.zeros(3)),
           dict(q_points=0), dict(q_optmod=0), dict(n_cstr=2, cstr_tol=[1e-3]), dict(n_cstr=0, cstr_tol=[1e-3]),
           dict(infill_strategy="pi"), dict(infill_optimizer="lbfgs"), dict(cstr_strategy="infill"), dict(q_infill_strategy="best"),
           dict(trego=True), dict(coego_n_coop=2), dict(outdir="out"), dict(warm_start=True), dict(hot_start=0),
           dict(gp_config="default"), dict(n_start=0)]
    for kw in bad:
        with pytest.raises(egx.InvalidValueError):
            egx.Egor(lim, **kw)
    with pytest.raises(egx.InvalidValueError):
        egx.Egor("nowhere")
    with pytest.raises(egx.InvalidValueError):
        egx.Egor(np.zeros((2, 3)))
    # what is accepted: x only and x with outputs, typed columns
    egx.Egor(lim, doe=np.zeros((3, 1)))
    egx.Egor(lim, doe=np.zeros((3, 4)), n_cstr=2, cstr_tol=[1e-3, 1e-3])
    e = egx.Egor([egx.XType.Int(0, 25)], doe=np.zeros((3, 1)))
    assert e.xtypes is not None and np.array_equal(e.xlimits, [[0.0, 25.0]])
    with pytest.raises(egx.InvalidValueError):
        e.minimize(lambda x: x, fcstrs=[lambda x, g: 0.0])
    # the result calls need no device
    y = np.array([[1.0, -0.15], [-1.0, -0.01], [2.0, -0.2], [-3.0, 2.0]])
    e = egx.Egor(lim, n_cstr=1, cstr_tol=[0.1])
    assert e.get_result_index(np.arange(4.0).reshape(-1, 1), y) == 1 and e.get_result_index(y) == 1
    res = e.get_result(np.arange(4.0).reshape(-1, 1), y)
    assert np.array_equal(res.x_opt, [1.0]) and np.array_equal(res.y_opt, y[1]) and res.x_doe.shape == (4, 1)
    with pytest.raises(egx.InvalidValueError):
        e.get_result_index(np.zeros((4, 3)))
