"""The fused infill evaluation (egx_infill_eval and its variants; egobox_amd/csrc/infill_eval.hip, kernels_infill.hip) at the shapes
where its kernels branch, against the CPU oracle on the handle's own fitted state (test_gpu_sample.oracle_from_handle; nothing
is refitted), tests/infill_oracle.py for the criterion and oracle/moe_oracle.py for the recombination of a mixture:

  A  n = 2100, d = 65, linear trend     two k0 passes of k_infill_xgrad_finish (62 + 3), d > 64 inside the fused sequence
  B  n = 4200, d = 32, quadratic trend  p = 561: three laps of k_infill_trend's strided loops, rhs_pad = 640, passes 31 + 1
  C  n = 600, d = 20, w_star (20, 3)    KPLS weights (fit_hcols = 3) next to a constraint model without weights
  D  n in {5, 64, 65, 129, 4097}        below one 64-row slab, at a slab edge, at a tile edge; 255 padding rows at n = 4097
  E  n = 16385, d = 8                   msplit = 260 > 256: the second lap of k_infill_trend's part[] load, passes 7 + 1
  F  mixtures at d = 41, 64, 65         k_infill_mix above 64 KB of LDS and at the strides d | 1 = 41, 65, 65

Every case asserts from `geometry` -- the restatement of the launch arithmetic below -- that it takes the branch it is named
after, so a retune that moves a threshold fails the case instead of emptying it.  The numpy-only tests at the top (no `gpu`
mark) check that arithmetic and the overlap of the mixtures without a GPU."""
import time

import numpy as np
import pytest

import infill_oracle as IO
from test_gpu_infill import CRITERIA, KINDS, MEANS, PRED_RTOL, _check_criterion, _check_parts, _data, _grad_tol, _queries
from test_gpu_infill_mix import KEYS, NAMES, _assert_overlap, _gmx2, _point
from test_gpu_sample import oracle_from_handle

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


# ---- the launch arithmetic, restated -----------------------------------------------------------------------------------------
def _round_up(a, b):
    return (a + b - 1) // b * b


def geometry(n, d, mean):
    """What the fused sequence does with a model of n points, d inputs and trend `mean` (0 constant, 1 linear, 2 quadratic) at
    the fixed 128-point tile.  Mirrors
      gp_host.hip slab_geometry:              n_pad = round_up(n, n >= 4096 ? kNB = 256 : kTile = 128), rhs_pad = round_up(p + 1, 128)
      gp_predict.hip mean_splits:             msplit = min(ceil(1024 / (kTile / 64)), n_pad / 64), evened out over the slabs
      gp_predict.hip xgrad_splits:            nsplit = min(512, ceil(n / 64)), evened out over the slabs
      kernels_infill.hip k_infill_xgrad_finish: kc = min(kInfThreads = 256, kXgStage = 2048 / nsplit), passes k0 = 0, kc, ... < d
      kernels_infill.hip k_infill_trend:      loops over l < p, j < p and sp < msplit strided by kInfThreads = 256"""
    p = [1, 1 + d, 1 + d + d * (d + 1) // 2][mean]
    n_pad = _round_up(n, 256 if n >= 4096 else 128)
    slabs_pad = n_pad // 64
    msplit = min((1024 + 128 // 64 - 1) // (128 // 64), slabs_pad)
    per = (slabs_pad + msplit - 1) // msplit
    msplit = (slabs_pad + per - 1) // per
    slabs = (n + 63) // 64
    nsplit = min(512, slabs)
    per = (slabs + nsplit - 1) // nsplit
    nsplit = (slabs + per - 1) // per
    kc = min(256, 2048 // nsplit)
    return dict(p=p, n_pad=n_pad, rhs_pad=_round_up(p + 1, 128), msplit=msplit, nsplit=nsplit, kc=kc,
                passes=[min(kc, d - k0) for k0 in range(0, d, kc)], laps_p=(p + 255) // 256, laps_part=(msplit + 255) // 256)


def mix_lds_bytes(d, k):
    """kernels_infill.hip infill_mix_lds_bytes: 64 lanes x (three rows of stride d | 1, two of stride k | 1) doubles; above
    64 KB launch_infill_mix opts in through hipFuncSetAttribute"""
    return 8 * 64 * (3 * (d | 1) + 2 * (k | 1))


A_SHAPE = (2100, 65, 1)
B_SHAPE = (4200, 32, 2)
E_SHAPE = (16385, 8, 0)
D_NS = [5, 64, 65, 129, 4097]
D_OTHER = {5: 129, 64: 65, 65: 64, 129: 5, 4097: 129}  # the constraint model's n: another geometry in the same scratch buffers
F_SHAPES = [(41, 2), (64, 3), (65, 4)]
TILE_MS = (127, 128, 129, 257)


def test_every_case_takes_the_branch_it_is_named_after():
    """numpy only"""
    a = geometry(*A_SHAPE)
    assert A_SHAPE[1] > 64 and a["p"] == 66 and a["nsplit"] == 33 and a["kc"] == 62 and a["passes"] == [62, 3]
    b = geometry(*B_SHAPE)
    assert b["p"] == 561 and b["laps_p"] == 3 and b["rhs_pad"] == 640 and b["rhs_pad"] > 128
    assert b["nsplit"] == 66 and b["kc"] == 31 and b["passes"] == [31, 1]
    e = geometry(*E_SHAPE)
    assert e["n_pad"] == 16640 and e["msplit"] == 260 and e["laps_part"] == 2
    assert e["nsplit"] == 257 and e["kc"] == 7 and e["passes"] == [7, 1]
    assert geometry(E_SHAPE[0] - 1, 8, 0)["msplit"] == 256  # the smallest n with a second lap
    assert [geometry(n, 3, 0)["n_pad"] for n in D_NS] == [128, 128, 128, 256, 4352]
    assert geometry(4097, 3, 0)["n_pad"] - 4097 == 255 and geometry(4096, 3, 0)["n_pad"] == 4096
    assert [geometry(n, 3, 0)["nsplit"] for n in D_NS] == [1, 1, 2, 3, 65]
    assert [mix_lds_bytes(d, k) for d, k in F_SHAPES] == [66048, 102912, 104960]
    assert all(65536 < mix_lds_bytes(d, k) <= 160 * 1024 for d, k in F_SHAPES)
    assert mix_lds_bytes(39, 2) <= 65536  # d | 1 = 41 is the smallest stride beyond 64 KB at k = 2
    assert [d | 1 for d, _ in F_SHAPES] == [41, 65, 65]
    for m in TILE_MS:  # the embedding of the position test crosses a tile boundary wherever the call has one
        off = _embed_offset(m, 15)
        assert 0 <= off and off + 15 <= m and (m <= 128 or off < 128 < off + 15)


# ---- the mixtures of case F ----------------------------------------------------------------------------------------------------
F_M = 130  # one full tile and a remainder of two points
F_NS = [260, 180, 300, 150, 220]  # up to four experts of the objective, then the lone constraint model


def _gmx_f(d, k):
    """k = 2: the suite's own mixture.  k = 3, 4: clusters along coordinate 0 with EQUAL isotropic scales (unequal ones decide
    every point through the log-determinant at d >= 64) and one full covariance."""
    if k == 2:
        return _gmx2(d)
    from egobox_amd.moe import GaussianMixture
    means = np.full((k, d), 0.5)
    means[:, 0] = [0.2, 0.5, 0.8] if k == 3 else [0.15, 0.4, 0.62, 0.85]
    means[:, 1] = [0.45, 0.6, 0.5] if k == 3 else [0.45, 0.6, 0.5, 0.4]
    covs = np.stack([np.eye(d) * 0.06] * k)
    covs[0][0, 1] = covs[0][1, 0] = 0.01
    return GaussianMixture([0.3, 0.3, 0.4] if k == 3 else [0.2, 0.3, 0.25, 0.25], means, covs, 0.9)


def _f_sets(d, k):
    """expert e of the objective on its own training set, then the constraint's; the objective's outputs are scaled so that
    the variance at a training point (~ nugget sigma2) stays below f64::EPSILON at these d (test_gpu_infill._data)"""
    sets = []
    for e, n in enumerate(F_NS[:k] + F_NS[-1:]):
        x, y = _data(n, d, seed=300 + 7 * d + e, yscale=1e-6 if e < k else 1.0)
        if e == k:
            y = y - np.quantile(y, 0.6)
        sets.append((x, y))
    return sets


def _f_queries(d, k, sets):
    rng = np.random.default_rng(900 + d)
    return np.vstack([rng.random((F_M - k, d))] + [sets[e][0][e + 3] for e in range(k)])


@pytest.mark.parametrize("d,k", F_SHAPES)
def test_mixtures_overlap_inside_the_query_box(d, k):
    """numpy only: what the GPU tests of case F rely on"""
    xq = _f_queries(d, k, _f_sets(d, k))
    assert xq.shape == (F_M, d)
    _assert_overlap(_gmx_f(d, k), xq)


def _theta(corr, d, s, tilt=0.0):
    """theta at which two points s apart in every normalised coordinate correlate at ~1/e (s = 1.15: the typical offset of two
    LHS points, what all pairs are at d >= 41; s = 3.46 n^(-1/d): the spacing of n points in the box, for small d), with the
    coordinates tilted by up to 30 %.  exp(-theta s^2 d), exp(-theta s d), and the Matern kernels to second order in theta s:
    exp(-3/2 theta^2 s^2 d), exp(-5/6 theta^2 s^2 d).  The suite's Griewank outputs are all but a quadratic: a GP with longer
    length scales than these follows them to 1e-6 of sigma2, sigma2 grows to 1e4 times the variance of the outputs, and the
    variance at a training point -- nugget * sigma2 -- ends up next to f64::EPSILON, where the LogEI gradient cancels."""
    base = [1.0 / (d * s * s), 1.0 / (d * s), np.sqrt(2.0 / (3.0 * d)) / s, np.sqrt(6.0 / (5.0 * d)) / s][corr]
    return base * (1.0 + tilt + (0.3 * np.arange(d) / (d - 1) if d > 1 else 0.0)) * np.ones(d)


# ---- shared checks -------------------------------------------------------------------------------------------------------------
def _oracle_parts(ref, xq):
    ry, rv = ref.predict_valvar(xq)
    gy, gv = ref.predict_valvar_gradients(xq)
    return np.ravel(ry), np.ravel(rv), gy, gv


def _rel(got, ref, floor):
    """largest |got - ref| / max(|ref|, floor): the figure a bar of `assert_allclose(rtol, atol = rtol * floor)` is about"""
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), floor)))


def _check_against(got, ref, sigma2, rtol=PRED_RTOL, label="", rows=None):
    """test_gpu_infill._check_parts on a reference computed once: got / ref = (mean, var, grad_mean, grad_var) of one model;
    rows: the points the reference's gradients were computed at (all of them when None)"""
    (m, v, gm, gv), (ry, rv, gy, gvr) = got, ref
    if rows is not None:
        gm, gv = gm[rows], gv[rows]
    if label:
        print(f"{label}: rel err mean {_rel(m, ry, 1e-9 / rtol):.2e} var {_rel(v, rv, 1e-9 * sigma2 / rtol):.2e} "
              f"grad_mean {_rel(gm, gy, np.abs(gy).max()):.2e} grad_var {_rel(gv, gvr, np.abs(gvr).max()):.2e}")
    np.testing.assert_allclose(m, ry, rtol=rtol, atol=1e-9)
    np.testing.assert_allclose(v, rv, rtol=rtol, atol=1e-9 * sigma2)
    np.testing.assert_allclose(gm, gy, rtol=rtol, atol=rtol * np.abs(gy).max())
    np.testing.assert_allclose(gv, gvr, rtol=rtol, atol=rtol * np.abs(gvr).max())


def _model(p, j):
    return p["mean"][j], p["var"][j], p["grad_mean"][j], p["grad_var"][j]


def _embed_offset(m, q):
    """where q points go inside m: across the boundary of the first tile when there is one, else at the end"""
    return min(128 - q // 2, m - q)


def _assert_position_independent(obj, pts, seed):
    """the points alone (m = 1), reversed, and inside m = 127, 128, 129, 257 points: the same bits"""
    q, d = pts.shape
    base = obj.parts(pts)
    rev = obj.parts(pts[::-1].copy())
    for i in range(q):
        one = obj.parts(pts[i:i + 1])
        for a, b, c, name in zip(_point(base, i), _point(rev, q - 1 - i), _point(one, 0), NAMES):
            np.testing.assert_array_equal(a, b, err_msg=f"{name} of point {i}: reversed order")
            np.testing.assert_array_equal(a, c, err_msg=f"{name} of point {i}: alone")
    rng = np.random.default_rng(seed)
    for m in TILE_MS:
        big = rng.random((m, d))
        off = _embed_offset(m, q)
        big[off:off + q] = pts
        big[m - 1] = pts[0]  # the last point of the call: alone in its tile at m = 129 and 257
        got = obj.parts(big)
        for i in range(q):
            if off + i == m - 1:
                continue
            for a, b, name in zip(_point(base, i), _point(got, off + i), NAMES):
                np.testing.assert_array_equal(a, b, err_msg=f"{name} of point {i}: at {off + i} of {m}")
        for a, b, name in zip(_point(base, 0), _point(got, m - 1), NAMES):
            np.testing.assert_array_equal(a, b, err_msg=f"{name} of point 0: last of {m}")
    return base


# ---- A: two reduction passes and d > 64 -------------------------------------------------------------------------------------------
class _Case:
    pass


@pytest.fixture(scope="module", params=[3, 1], ids=["matern52", "absexp"])
def case_a(request, egx, O):
    n, d, mean = A_SHAPE
    c = _Case()
    c.corr = request.param
    c.x, c.y = _data(n, d, seed=201, yscale=1e-6)  # 1e-6: the variance at a training point stays below f64::EPSILON at d = 65
    c.theta = _theta(c.corr, d, 1.15)
    c.xq = _queries(c.x, 12, seed=17 + c.corr)
    c.fmin = float(np.quantile(c.y, 0.1))
    c.h = egx.GpHandle(c.x, c.y, mean=mean, corr=c.corr)
    c.h.finalize(c.theta)
    assert (c.h.n, c.h.d, c.h.p) == (n, d, geometry(n, d, mean)["p"])
    t0 = time.perf_counter()
    ref = oracle_from_handle(O, c.h, MEANS[mean], KINDS[c.corr], c.x, c.y)
    c.sigma2 = float(ref.inner.sigma2)
    c.ref = _oracle_parts(ref, c.xq)  # computed once, left unchanged
    print(f"case A corr {c.corr}: oracle {time.perf_counter() - t0:.1f} s")
    yield c
    c.h.close()


@gpu
def test_a_parts_and_criteria_d65_two_passes(egx, case_a):
    c = case_a
    assert len(geometry(*A_SHAPE)["passes"]) == 2
    for crit in CRITERIA:
        with egx.InfillObjective(c.h, criterion=crit, fmin=c.fmin, sigma_weight=0.75, scale_ic=2.3, scale=1.7) as obj:
            p = obj.parts(c.xq)
            assert np.all(p["var"][0, -3:] < IO.EPS) and np.all(p["var"][0, :-3] > 1e-6 * c.sigma2)
            if crit == CRITERIA[0]:
                _check_against(_model(p, 0), c.ref, c.sigma2, label=f"A corr {c.corr}")
            wv, wg = _check_criterion(obj, p, [])
            print(f"A corr {c.corr} crit {crit}: value err {wv:.2e} grad err {wg:.2e}")


@gpu
def test_a_predict_gradients_against_the_analytic_oracle(case_a):
    """egx_gp_predict_valvar_gradients at d > 64 (the form of k_xgrad that reads the query from global memory), batched and
    m <= 8, against the oracle's jacobians instead of finite differences of the library's own predictions"""
    c = case_a
    _, _, ry, rv = c.ref
    gy, gv = c.h.predict_valvar_gradients(c.xq)
    np.testing.assert_allclose(gy, ry, **_grad_tol(ry))
    np.testing.assert_allclose(gv, rv, **_grad_tol(rv))
    for lo, hi in ((0, 8), (8, 15), (14, 15)):
        gy, gv = c.h.predict_valvar_gradients(c.xq[lo:hi])
        np.testing.assert_allclose(gy, ry[lo:hi], **_grad_tol(ry))
        np.testing.assert_allclose(gv, rv[lo:hi], **_grad_tol(rv))


@gpu
def test_a_points_do_not_depend_on_position_or_companions(egx, case_a):
    c = case_a
    with egx.InfillObjective(c.h, criterion=egx.LOG_EI, fmin=c.fmin) as obj:
        base = _assert_position_independent(obj, c.xq, seed=5)
        # the gradient-free call
        np.testing.assert_array_equal(obj.value(c.xq), base["value"])
        v, g = obj.value_and_grad(c.xq)
        np.testing.assert_array_equal(v, base["value"])
        np.testing.assert_array_equal(g, base["grad"])


@gpu
def test_a_one_nan_point_among_129(egx, case_a):
    c = case_a
    d = c.x.shape[1]
    pts = np.random.default_rng(12).random((129, d))
    pts[120:129] = c.xq[:9]
    for where in (128, 127, 3):  # alone in the second tile, the last of the first, inside the first
        bad = pts.copy()
        bad[where, d - 1] = np.nan
        with egx.InfillObjective(c.h, criterion=egx.WB2, fmin=c.fmin) as obj:
            good, got = obj.parts(pts), obj.parts(bad)
            assert got["value"][where] == np.inf and np.all(got["grad"][where] == 0.0)
            keep = np.arange(129) != where
            for name in NAMES:
                a, b = (good[name][keep], got[name][keep]) if name in ("value", "grad") else (good[name][:, keep], got[name][:, keep])
                np.testing.assert_array_equal(a, b, err_msg=f"{name}, NaN at {where}")
            vals = obj.value(bad)
            assert vals[where] == np.inf
            np.testing.assert_array_equal(vals[keep], good["value"][keep])


def _assert_parts_are_the_predictions(h, p, j, xq):
    """what the header of kernels_infill.hip promises a caller may rely on (test_gpu_infill.test_gaussian_process_and_gpx_...)"""
    mu, var = h.predict_valvar(xq)
    gy, gv = h.predict_valvar_gradients(xq)
    for got, ref, name in zip(_model(p, j), (mu, var, gy, gv), KEYS):
        np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-12 * np.abs(ref).max(), err_msg=name)


@gpu
def test_a_parts_agree_with_the_predict_entry_points(egx, case_a):
    c = case_a
    with egx.InfillObjective(c.h, criterion=egx.EI, fmin=c.fmin) as obj:
        _assert_parts_are_the_predictions(c.h, obj.parts(c.xq), 0, c.xq)


# ---- B: p > 256 -----------------------------------------------------------------------------------------------------------------
def _data_b(n, d, seed):
    """NOT a quadratic (the suite's Griewank outputs leave a 561-column trend nothing: sigma2 ~ 1e-14 and every variance below
    f64::EPSILON): sum sin 5 x_j + prod_{j < 4} cos 7 x_j on a classic LHS, scaled like the suite's objective models"""
    from egobox_amd import workload
    x = workload.lhs(n, d, seed)
    return x, 1e-3 * (np.sin(5.0 * x).sum(axis=1) + np.prod(np.cos(7.0 * x[:, :4]), axis=1))


@pytest.fixture(scope="module")
def case_b(egx, O):
    n, d, mean = B_SHAPE
    c = _Case()
    c.corr = 3
    c.x, c.y = _data_b(n, d, seed=211)
    c.theta = np.full(d, 0.1)
    c.xq = _queries(c.x, 9, seed=23)
    c.fmin = float(np.quantile(c.y, 0.1))
    c.h = egx.GpHandle(c.x, c.y, mean=mean, corr=c.corr)
    c.h.finalize(c.theta)
    assert (c.h.n, c.h.d, c.h.p) == (n, d, 561)
    t0 = time.perf_counter()
    ref = oracle_from_handle(O, c.h, MEANS[mean], KINDS[c.corr], c.x, c.y)
    c.sigma2 = float(ref.inner.sigma2)
    c.ref = _oracle_parts(ref, c.xq)
    print(f"case B: oracle {time.perf_counter() - t0:.1f} s")
    yield c
    c.h.close()


# The bar of B and of E: a 561-column GLS and n = 16385 could have needed a wider bar than the project's for reasons that are
# not the kernels' (the p = 136 case of the parity tests needs 1e-5 on the variance).  Measured on an MI355X against
# oracle_from_handle, as the figures _check_against prints: B mean 2.1e-12, var 2.4e-12, grad_mean 4.1e-13, grad_var 8.6e-13;
# E mean 1.7e-15, var 2.3e-12, grad_mean 3.1e-15, grad_var 1.2e-14.  Both are inside the project's bar by five orders of
# magnitude, so both cases use it unchanged and no second reference (an independent CPU fit) sets a bar of their own.
B_RTOL = PRED_RTOL


@gpu
def test_b_parts_and_criteria_561_regression_columns(egx, case_b):
    """The bar is the project's (see B_RTOL above for the measured figures)."""
    c = case_b
    g = geometry(*B_SHAPE)
    assert g["laps_p"] == 3 and g["rhs_pad"] == 640 and g["passes"] == [31, 1]
    for crit in CRITERIA:
        with egx.InfillObjective(c.h, criterion=crit, fmin=c.fmin, sigma_weight=0.75, scale_ic=2.3, scale=1.7) as obj:
            p = obj.parts(c.xq)
            assert np.all(p["var"][0, :-3] > 1e-6 * c.sigma2), (p["var"][0], c.sigma2)  # the variance is not the EPSILON rule's
            assert np.all(c.ref[1][:-3] > 1e-6 * c.sigma2)
            if crit == CRITERIA[0]:
                _check_against(_model(p, 0), c.ref, c.sigma2, rtol=B_RTOL, label="B")
            wv, wg = _check_criterion(obj, p, [])
            print(f"B crit {crit}: value err {wv:.2e} grad err {wg:.2e}")


@gpu
def test_b_points_do_not_depend_on_position_or_companions(egx, case_b):
    c = case_b
    with egx.InfillObjective(c.h, criterion=egx.LOG_EI, fmin=c.fmin) as obj:
        _assert_position_independent(obj, c.xq, seed=6)


C_THETA = {0: np.array([0.2, 0.15, 0.1]), 3: np.array([0.2, 0.15, 0.1])}  # on the three projected coordinates (std ~ sqrt(20))


# ---- C: KPLS weights ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("corr,mean", [(0, 0), (3, 1)])
def test_c_kpls_weighted_objective_next_to_an_unweighted_constraint(egx, O, corr, mean):
    n, d, hc = 600, 20, 3
    x, y = _data(n, d, seed=221, yscale=1e-4)
    xc, yc = _data(450, d, seed=222)
    yc = yc - np.quantile(yc, 0.6)
    w = np.random.default_rng(2).standard_normal((d, hc))
    xq = _queries(x, 12, seed=29 + corr)
    tols = [0.3]
    with egx.GpHandle(x, y, mean=mean, corr=corr, w_star=w) as h, egx.GpHandle(xc, yc, mean=1, corr=2) as hcst:
        assert h.h == hc and hcst.h == d  # fit_hcols = 3: k_predict_mean<.., false>, the non-prestaged cross-correlation
        h.finalize(C_THETA[corr])
        hcst.finalize(_theta(2, d, 1.15))
        refs = [oracle_from_handle(O, h, MEANS[mean], KINDS[corr], x, y, w_star=w),
                oracle_from_handle(O, hcst, MEANS[1], KINDS[2], xc, yc)]
        want = [_oracle_parts(r, xq) for r in refs]
        for crit in CRITERIA:
            with egx.InfillObjective(h, [hcst], tols, criterion=crit, fmin=float(np.quantile(y, 0.1)), sigma_weight=0.75,
                                     scale_ic=1.9, scale=2.5) as obj:
                p = obj.parts(xq)
                assert np.all(p["var"][0, -3:] < IO.EPS) and np.all(p["var"][0, :-3] > 1e-6 * refs[0].inner.sigma2)
                if crit == CRITERIA[0]:
                    for j in range(2):
                        _check_against(_model(p, j), want[j], float(refs[j].inner.sigma2), label=f"C corr {corr} model {j}")
                    _assert_parts_are_the_predictions(h, p, 0, xq)
                wv, wg = _check_criterion(obj, p, tols)
                print(f"C corr {corr} crit {crit}: value err {wv:.2e} grad err {wg:.2e}")


# ---- D: tiny models, slab and tile edges ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mean", [0, 1])
@pytest.mark.parametrize("n,d", [(n, d) for n in D_NS[:4] for d in (1, 3)] + [(4097, 3)])
def test_d_tiny_and_edge_n(egx, O, n, d, mean):
    nc = D_OTHER[n]
    x, y = _data(n, d, seed=231 + n, yscale=1e-5)  # 1e-5: a training point stays below f64::EPSILON at every shape
    xc, yc = _data(nc, d, seed=232 + n)
    yc = yc - np.quantile(yc, 0.6)
    xq = _queries(x, 6, seed=n + d)
    tols = [0.3]
    specs = [(mean, (n + d) % 4), (1 - mean, (n + d + 1) % 4)]
    with egx.GpHandle(x, y, mean=specs[0][0], corr=specs[0][1]) as h, egx.GpHandle(xc, yc, mean=specs[1][0], corr=specs[1][1]) as hc:
        assert h.n == n and hc.n == nc
        h.finalize(_theta(specs[0][1], d, 3.46 * n ** (-1.0 / d)))
        hc.finalize(_theta(specs[1][1], d, 3.46 * nc ** (-1.0 / d), tilt=0.1))
        for crit in CRITERIA:
            with egx.InfillObjective(h, [hc], tols, criterion=crit, fmin=float(np.quantile(y, 0.1)), sigma_weight=0.75,
                                     scale_ic=1.9, scale=2.5) as obj:
                p = obj.parts(xq)
                if crit == CRITERIA[0]:
                    _check_parts(O, [h, hc], specs, [x, xc], [y, yc], p, xq)
                    with egx.InfillObjective(hc, [h], tols, criterion=crit, fmin=0.0) as swapped:  # the geometries in the other order
                        ps = swapped.parts(xq)
                    for key in KEYS:
                        np.testing.assert_array_equal(ps[key][::-1], p[key], err_msg=key)
                wv, wg = _check_criterion(obj, p, tols)
                print(f"D n {n} d {d} mean {mean} crit {crit}: value err {wv:.2e} grad err {wg:.2e}")


# ---- E: msplit > 256 --------------------------------------------------------------------------------------------------------------
E_RTOL = PRED_RTOL


@gpu
def test_e_more_than_256_mean_splits(egx, O):
    """The bar is the project's (see B_RTOL above for the measured figures).  Wall time on an MI355X host: 1.0 s, of which the
    CPU oracle (the n x n factor copied back, two triangular solves per point) 0.8 s."""
    n, d, mean = E_SHAPE
    t_all = time.perf_counter()
    x, y = _data(n, d, seed=241, yscale=1e-4)  # 1e-4: a training point stays below f64::EPSILON
    xq = _queries(x, 6, seed=31)
    with egx.GpHandle(x, y, mean=mean, corr=0) as h:
        g = geometry(h.n, h.d, mean)  # from the handle's reported dimensions
        assert h.n == 16385 and g["n_pad"] == 16640 and g["msplit"] == 260 and g["laps_part"] == 2 and g["passes"] == [7, 1]
        h.finalize(np.full(d, 1.2))
        t0 = time.perf_counter()
        ref = oracle_from_handle(O, h, MEANS[mean], KINDS[0], x, y)
        sigma2 = float(ref.inner.sigma2)
        want = _oracle_parts(ref, xq)
        del ref
        t_oracle = time.perf_counter() - t0
        fmin = float(np.quantile(y, 0.05))
        for crit in CRITERIA:
            with egx.InfillObjective(h, criterion=crit, fmin=fmin, sigma_weight=0.75, scale_ic=1.9, scale=2.5) as obj:
                p = obj.parts(xq)
                if crit == CRITERIA[0]:
                    _check_against(_model(p, 0), want, sigma2, rtol=E_RTOL, label="E")
                    _assert_parts_are_the_predictions(h, p, 0, xq)
                wv, wg = _check_criterion(obj, p, [])
                print(f"E crit {crit}: value err {wv:.2e} grad err {wg:.2e}")
    print(f"case E: {time.perf_counter() - t_all:.1f} s, of which the CPU oracle {t_oracle:.1f} s")


# ---- F: mixtures -------------------------------------------------------------------------------------------------------------------
# The oracle's jacobians cost ~30 ms per point and expert at these d: the means and variances are checked at all 130 points, the
# gradients at the rows where the layout of k_infill_mix changes -- the first lanes, both sides of the 64-lane workgroup edge,
# the end of the full tile, the two-point remainder -- and at the training points (the last k rows).
def _f_grad_rows(k):
    return np.unique([0, 1, 2, 3, 62, 63, 64, 65, 126, 127, 128, 129] + list(range(F_M - k, F_M)))


class _Rows:
    """An oracle expert's predictions at the fixture's queries, computed ONCE in one batch and served row by row: moe_oracle asks
    its experts point by point, for the smooth and for the hard recombination."""

    def __init__(self, ref, xq, rows):
        self.inner = ref.inner
        self.at = {x.tobytes(): i for i, x in enumerate(xq)}
        self.mean, self.var = (np.ravel(a) for a in ref.predict_valvar(xq))
        gy, gv = ref.predict_valvar_gradients(xq[rows])
        self.gy, self.gv = np.full(xq.shape, np.nan), np.full(xq.shape, np.nan)
        self.gy[rows], self.gv[rows] = gy, gv
        self.parts = (self.mean, self.var, gy, gv)

    def _take(self, table, x):
        out = table[[self.at[r.tobytes()] for r in np.atleast_2d(x)]]
        assert np.all(np.isfinite(out))
        return out

    def predict(self, x):
        return self._take(self.mean, x)

    def predict_var(self, x):
        return self._take(self.var, x)

    def predict_gradients(self, x):
        return self._take(self.gy, x)

    def predict_var_gradients(self, x):
        return self._take(self.gv, x)


@pytest.fixture(scope="module", params=F_SHAPES, ids=[f"d{d}k{k}" for d, k in F_SHAPES])
def case_f(request, egx, O):
    from oracle import moe_oracle as MO
    d, k = request.param
    assert mix_lds_bytes(d, k) > 65536
    f = _Case()
    f.d, f.k, f.sets = d, k, _f_sets(d, k)
    f.xq = _f_queries(d, k, f.sets)
    f.rows = _f_grad_rows(k)
    assert {63, 64, 127, 128, 129} <= set(f.rows) and set(range(F_M - k, F_M)) <= set(f.rows)
    f.handles, f.oracles = [], []
    t0 = time.perf_counter()
    for e, (x, y) in enumerate(f.sets):
        mean, corr = e % 2, [0, 3, 2, 1, 0][e]
        h = egx.GpHandle(x, y, mean=mean, corr=corr)
        h.finalize(_theta(corr, d, 1.15, tilt=0.1 * e))
        f.handles.append(h)
        f.oracles.append(_Rows(oracle_from_handle(O, h, MEANS[mean], KINDS[corr], x, y), f.xq, f.rows))
    gps = [egx.GaussianProcess(h, None) for h in f.handles]
    f.gmx = _gmx_f(d, k)
    f.mix = {mode: egx.GpMixture(gps[:k], f.gmx, mode) for mode in ("smooth", "hard")}
    f.cstr = f.handles[k]
    _assert_overlap(f.gmx, f.xq)
    f.fmin = float(np.quantile(f.sets[0][1], 0.1))
    f.sigma2 = [max(float(o.inner.sigma2) for o in f.oracles[:k]), float(f.oracles[k].inner.sigma2)]
    # the references, computed once: the oracle's mixture over the oracle's experts, the experts alone, the lone constraint
    f.ogmx = MO.GaussianMixtureOracle(f.gmx.weights, f.gmx.means, f.gmx.covariances, f.gmx.heaviside_factor)
    ex, xg = f.oracles[:k], f.xq[f.rows]
    f.ref = {"smooth": (MO.predict_smooth(ex, f.ogmx, f.xq), MO.predict_var_smooth(ex, f.ogmx, f.xq),
                        MO.predict_gradients_smooth(ex, f.ogmx, xg), MO.predict_var_gradients_smooth(ex, f.ogmx, xg)),
             "hard": (MO.predict_hard(ex, f.ogmx, f.xq), MO.predict_var_hard(ex, f.ogmx, f.xq),
                      MO.predict_gradients_hard(ex, f.ogmx, xg), MO.predict_var_gradients_hard(ex, f.ogmx, xg))}
    print(f"case F d {d} k {k}: handles and oracle {time.perf_counter() - t0:.1f} s")
    yield f
    for h in f.handles:
        h.close()


@gpu
@pytest.mark.parametrize("mode", ["smooth", "hard"])
def test_f_mixture_parts_and_criteria(egx, case_f, mode):
    """the bars of test_gpu_infill_mix._check_mix_parts, which are those of _check_parts"""
    f = case_f
    tols = [0.3]
    for crit in CRITERIA:
        with egx.InfillObjective(f.mix[mode], [f.cstr], tols, criterion=crit, fmin=f.fmin, sigma_weight=0.75, scale_ic=1.9,
                                 scale=2.5) as obj:
            p = obj.parts(f.xq)
            if crit == CRITERIA[0]:
                _check_against(_model(p, 0), f.ref[mode], f.sigma2[0], rows=f.rows, label=f"F d {f.d} k {f.k} {mode}")
                _check_against(_model(p, 1), f.oracles[f.k].parts, f.sigma2[1], rows=f.rows)
            wv, wg = _check_criterion(obj, p, tols)
            print(f"F d {f.d} k {f.k} {mode} crit {crit}: value err {wv:.2e} grad err {wg:.2e}")


@gpu
def test_f_expert_diagnostics(egx, case_f):
    """egx_infill_eval_experts: the experts' parts at the bar of the lone models, the responsibilities and their derivatives
    against GaussianMixtureOracle.  The bar of the responsibilities: log p_c is a sum of d squares of size up to ~100 at these
    d, whose rounding (d + 2 operations of 1.1e-16 each on terms of that size) is ~1e-12 absolute in the logarithm, i.e. 1e-12
    relative in p_c; the derivative multiplies by the precision (1 / 0.06) and loses another digit: 1e-10 and 1e-9."""
    f = case_f
    with egx.InfillObjective(f.mix["smooth"], [f.cstr], [0.3], criterion=egx.EI, fmin=f.fmin) as obj:
        ep = obj.expert_parts(0, f.xq)
        assert ep["mean"].shape == (f.k, F_M) and ep["dprobas"].shape == (F_M, f.k, f.d)
        for e in range(f.k):
            _check_against(tuple(ep[key][e] for key in KEYS), f.oracles[e].parts, float(f.oracles[e].inner.sigma2), rows=f.rows,
                           label=f"F d {f.d} expert {e}")
        pr, dpr = f.ogmx.predict_probas(f.xq), f.ogmx.predict_probas_derivatives(f.xq)
        print(f"F d {f.d} k {f.k}: rel err probas {_rel(ep['probas'], pr, 1e-300):.2e} dprobas "
              f"{_rel(ep['dprobas'], dpr, np.abs(dpr).max()):.2e}")
        np.testing.assert_allclose(ep["probas"], pr, rtol=1e-10, atol=1e-300)
        np.testing.assert_allclose(ep["dprobas"], dpr, rtol=1e-9, atol=1e-9 * np.abs(dpr).max())
        ec = obj.expert_parts(1, f.xq)  # the lone constraint: its own slot, responsibilities of one
        np.testing.assert_array_equal(ec["probas"], 1.0)
        np.testing.assert_array_equal(ec["dprobas"], 0.0)
        _check_against(tuple(ec[key][0] for key in KEYS), f.oracles[f.k].parts, f.sigma2[1], rows=f.rows)


@gpu
@pytest.mark.parametrize("mode", ["smooth", "hard"])
def test_f_points_do_not_depend_on_position_or_companions(egx, case_f, mode):
    f = case_f
    pts = np.vstack([f.xq[:12], f.xq[-3:]])
    with egx.InfillObjective(f.mix[mode], [f.cstr], [0.3], criterion=egx.LOG_EI, fmin=f.fmin) as obj:
        _assert_position_independent(obj, pts, seed=7)
