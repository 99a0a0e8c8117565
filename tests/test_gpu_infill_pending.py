"""Pending points on the infill handle (egx_infill_push_pending and friends; gp_infill.hip, kernels_pending.hip, pending_math.h):
the conditioned parts against an actual refit with frozen normalisation (tests/pending_oracle.py on oracle.gp_oracle), the
criterion as the arithmetic of those parts, the exactness of the switch, the believer property, the batch call against the
manual loop and against the refit, errors and state, a C host."""
import os
import subprocess
import types

import numpy as np
import pytest

import infill_oracle as IO
import pending_oracle as PO
from test_gpu_infill import CRITERIA, KINDS, MEANS, PRED_RTOL, _check_criterion, _grad_tol
from test_gpu_sample import oracle_from_handle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLS = [0.3, 0.1]


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


def _ys(y):
    """the objective (scaled as in tests/test_gpu_infill.py) and two constraint outputs on the same rows"""
    return [1e-3 * y, y - np.quantile(y, 0.6), np.quantile(y, 0.7) - y]


def _case(egx, O, n, d, q, theta, mean, corr, m=40, w=None):
    """three fitted models on workload.make_training_set(n, d, seed=1), their oracles, q pending points and m queries uniform in
    the data's box, virtual values = base mean + 3 sigma N(0, 1)"""
    from egobox_amd import workload
    x, y = workload.make_training_set(n, d, seed=1)
    c = types.SimpleNamespace(x=x, ys=_ys(y), n=n, d=d, q=q, hs=[], gs=[])
    th = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    th = np.full(d if w is None else w.shape[1], th[0]) if th.size == 1 else th
    for yj in c.ys:
        h = egx.GpHandle(x, yj, mean=mean, corr=corr, w_star=w)
        h.finalize(th)
        c.hs.append(h)
        c.gs.append(oracle_from_handle(O, h, MEANS[mean], KINDS[corr], x, yj, w_star=w))
    rng = np.random.default_rng(1000 * n + 10 * d + q)
    lo, hi = x.min(axis=0), x.max(axis=0)
    c.lo, c.hi = lo, hi
    c.xv = lo + (hi - lo) * rng.random((q, d))
    c.xq = lo + (hi - lo) * rng.random((m, d))
    c.yv = np.empty((q, 3))
    for j, g in enumerate(c.gs):
        mu, var = g.predict_valvar(c.xv)
        c.yv[:, j] = mu + 3.0 * np.sqrt(var) * rng.standard_normal(q)
    c.fmin = float(np.quantile(c.ys[0], 0.1))
    return c


def _close(c):
    for h in c.hs:
        h.close()


def _assert_conditioned(c, xq):
    """the condition on the cases, on the ORACLE: below it s^2 - c^T S^-1 c loses its digits in any double evaluation"""
    min_diag, min_unit = PO.cond_report(c.gs[0], c.xv, xq)  # (the three models share x, theta, kernel and trend)
    print(f"n {c.n} d {c.d} q {c.q}: min diag S {min_diag:.3g}, min conditioned unit variance {min_unit:.3g}")
    assert min_diag >= 1e-2 and min_unit >= 1e-4


def _push_all(obj, c):
    for v in range(c.q):
        obj.push_pending(c.xv[v], c.yv[v])


def _check_parts_against_refit(c, p, xq, sigma2):
    for j, g in enumerate(c.gs):
        ref = PO.refit_frozen(g, c.xv, c.yv[:, j])
        ry, rv = ref.predict_valvar(xq)
        gy, gv = ref.predict_valvar_gradients(xq)
        for name, got, want in (("mean", p["mean"][j], np.ravel(ry)), ("var", p["var"][j] / ref.inner.sigma2, np.ravel(rv) / ref.inner.sigma2),
                                ("grad_mean", p["grad_mean"][j] / np.abs(gy).max(), gy / np.abs(gy).max()),
                                ("grad_var", p["grad_var"][j] / np.abs(gv).max(), gv / np.abs(gv).max())):
            print(f"  model {j} {name}: worst abs error {np.max(np.abs(got - want)):.3e} (scale {np.max(np.abs(want)):.3e})")
        print(f"  model {j} sigma2: {sigma2[j]:.12e} refit {ref.inner.sigma2:.12e}")
        np.testing.assert_allclose(p["mean"][j], np.ravel(ry), rtol=PRED_RTOL, atol=1e-9)
        np.testing.assert_allclose(p["var"][j], np.ravel(rv), rtol=PRED_RTOL, atol=1e-9 * ref.inner.sigma2)
        np.testing.assert_allclose(p["grad_mean"][j], gy, **_grad_tol(gy))
        np.testing.assert_allclose(p["grad_var"][j], gv, **_grad_tol(gv))
        np.testing.assert_allclose(sigma2[j], ref.inner.sigma2, rtol=1e-6)


# ---- 1. parts against the refit ----------------------------------------------------------------------------------------------
PARTS_CASES = ([(600, 4, 3, 1.5, mean, corr) for corr in range(4) for mean in range(3)] +
               [(n, d, q, th, mean, 3) for (n, d, q, th) in [(130, 3, 5, 1.5), (130, 2, 2, 4.0), (600, 5, 16, 1.5)] for mean in (0, 2)] +
               [(130, 1, 1, 30.0, mean, 1) for mean in (0, 2)])


@pytest.mark.parametrize("n,d,q,theta,mean,corr", PARTS_CASES)
def test_parts_are_the_frozen_refit(egx, O, n, d, q, theta, mean, corr):
    c = _case(egx, O, n, d, q, theta, mean, corr)
    try:
        _assert_conditioned(c, c.xq)
        with egx.InfillObjective(c.hs[0], c.hs[1:], TOLS, criterion=egx.EI, fmin=c.fmin) as obj:
            _push_all(obj, c)
            px, py, s2 = obj.pending
            np.testing.assert_array_equal(px, c.xv)
            np.testing.assert_array_equal(py, c.yv)
            _check_parts_against_refit(c, obj.parts(c.xq), c.xq, s2)
    finally:
        _close(c)


@pytest.mark.parametrize("m", [131, 1])
def test_parts_two_tiles_and_one_point(egx, O, m):
    c = _case(egx, O, 600, 4, 3, 1.5, 0, 3, m=m)
    try:
        _assert_conditioned(c, c.xq)
        with egx.InfillObjective(c.hs[0], c.hs[1:], TOLS, criterion=egx.EI, fmin=c.fmin) as obj:
            _push_all(obj, c)
            _check_parts_against_refit(c, obj.parts(c.xq), c.xq, obj.pending[2])
    finally:
        _close(c)


def test_parts_kpls_weights(egx, O):
    """w_star (4, 2): fit_hcols = 2, the coefficient columns of corr_pair.h"""
    w = np.random.default_rng(2).standard_normal((4, 2))
    c = _case(egx, O, 130, 4, 3, np.array([0.6, 0.4]), 0, 3, w=w)
    try:
        assert c.hs[0].h == 2
        _assert_conditioned(c, c.xq)
        with egx.InfillObjective(c.hs[0], c.hs[1:], TOLS, criterion=egx.EI, fmin=c.fmin) as obj:
            _push_all(obj, c)
            _check_parts_against_refit(c, obj.parts(c.xq), c.xq, obj.pending[2])
    finally:
        _close(c)


@pytest.mark.parametrize("n,d,q,theta,mean", [(600, 5, 16, 1.5, 2), (130, 3, 5, 1.5, 0)])
def test_parts_composed_form(egx, O, n, d, q, theta, mean):
    """egx_set_tuning("pending_composed", 1): q launches of the existing contractions over Z in place of the fused kernel -- the
    same refit, and the fused form's values to rounding"""
    c = _case(egx, O, n, d, q, theta, mean, 3)
    try:
        _assert_conditioned(c, c.xq)
        with egx.InfillObjective(c.hs[0], c.hs[1:], TOLS, criterion=egx.EI, fmin=c.fmin) as obj:
            _push_all(obj, c)
            fused = obj.parts(c.xq)
            assert egx.set_tuning("pending_composed", 1) == 0
            try:
                comp = obj.parts(c.xq)
                _check_parts_against_refit(c, comp, c.xq, obj.pending[2])
                obj.set_cstr_strategy("mean", [1.0, 1.0])  # the mean-only twin on the composed layouts
                cs, gc = obj.constraints(c.xq, grad=True)[1::2]
                np.testing.assert_array_equal(cs, comp["mean"][1:].T)
                np.testing.assert_array_equal(gc, comp["grad_mean"][1:].transpose(1, 0, 2))
            finally:
                assert egx.set_tuning("pending_composed", 0) == 1
            for k in KEYS[2:]:
                scale = np.abs(fused[k]).reshape(3, -1).max(axis=1).reshape((3,) + (1,) * (fused[k].ndim - 1))
                assert np.max(np.abs(comp[k] - fused[k]) / scale) <= 1e-9, k
    finally:
        _close(c)


def test_parts_beyond_the_fused_kernels_reach(egx, O):
    """d = 70 > 64: the composed form on its own"""
    c = _case(egx, O, 130, 70, 2, 0.1, 0, 3, m=20)
    try:
        _assert_conditioned(c, c.xq)
        with egx.InfillObjective(c.hs[0], c.hs[1:], TOLS, criterion=egx.EI, fmin=c.fmin) as obj:
            _push_all(obj, c)
            _check_parts_against_refit(c, obj.parts(c.xq), c.xq, obj.pending[2])
    finally:
        _close(c)


# ---- 2. the criterion is the arithmetic of the conditioned parts --------------------------------------------------------------
@pytest.fixture(scope="module")
def mid(egx, O):
    c = _case(egx, O, 600, 4, 3, 1.5, 2, 3, m=131)
    yield c
    _close(c)


def test_criterion_is_the_arithmetic_of_the_conditioned_parts(egx, mid):
    c = mid
    for crit in CRITERIA:
        with egx.InfillObjective(c.hs[0], c.hs[1:], TOLS, criterion=crit, fmin=c.fmin, sigma_weight=0.75, scale_ic=2.3,
                                 scale=1.7) as obj:
            _push_all(obj, c)
            p = obj.parts(c.xq[:40])
            wv, wg = _check_criterion(obj, p, TOLS)
            print(f"folded crit {crit}: value err {wv:.2e} grad err {wg:.2e}")
            scales = np.array([1.3, 0.6])
            for strategy in ("mean", "utb"):
                obj.set_cstr_strategy(strategy, scales)
                v, cs, g, gc = obj.constraints(c.xq[:40], grad=True)
                p0 = {k: (p[k][:1] if k not in ("value", "grad") else None) for k in p}
                p0["value"], p0["grad"] = v, g
                _check_criterion(obj, p0, [])
                gm, gv = p["grad_mean"][1:].transpose(1, 0, 2), p["grad_var"][1:].transpose(1, 0, 2)
                if strategy == "mean":
                    want_c, want_g = p["mean"][1:].T / scales, gm / scales[None, :, None]
                else:
                    sigma = np.sqrt(p["var"][1:].T)
                    want_c = (p["mean"][1:].T + 3.0 * sigma) / scales
                    want_g = (gm + 3.0 * (gv / (2.0 * sigma[:, :, None]))) / scales[None, :, None]
                assert np.max(np.abs(cs - want_c) / np.maximum(1.0, np.abs(want_c))) <= 1e-11
                assert np.max(np.abs(gc - want_g)) / max(1.0, np.max(np.abs(want_g))) <= 1e-8
            obj.set_cstr_strategy("infill")


# ---- 3. exactness of the switch -----------------------------------------------------------------------------------------------
KEYS = ("value", "grad", "mean", "var", "grad_mean", "grad_var")


def test_clear_pending_gives_back_the_fitted_handle_bit_for_bit(egx, mid):
    c = mid
    kw = dict(criterion=egx.LOG_EI, fmin=c.fmin)
    with egx.InfillObjective(c.hs[0], c.hs[1:], TOLS, **kw) as never, egx.InfillObjective(c.hs[0], c.hs[1:], TOLS, **kw) as obj:
        want = never.parts(c.xq)
        before = obj.parts(c.xq)
        _push_all(obj, c)
        with_pending = obj.parts(c.xq)
        assert not np.array_equal(with_pending["mean"], want["mean"])
        obj.clear_pending()
        assert obj.pending[0].shape == (0, c.d)
        after = obj.parts(c.xq)
        for k in KEYS:
            np.testing.assert_array_equal(before[k], want[k])
            np.testing.assert_array_equal(after[k], want[k])
        np.testing.assert_array_equal(obj.value(c.xq), never.value(c.xq))
        np.testing.assert_array_equal(obj.pending[2], [g.inner.sigma2 for g in c.gs])


def test_a_conditioned_point_does_not_depend_on_its_companions(egx, mid):
    c = mid
    with egx.InfillObjective(c.hs[0], c.hs[1:], TOLS, criterion=egx.LOG_EI, fmin=c.fmin) as obj:
        _push_all(obj, c)
        big = obj.parts(c.xq)  # 131 points: two tiles, the second ragged
        for i in (0, 57, 127, 128, 130):
            one = obj.parts(c.xq[i])
            for k in KEYS:
                np.testing.assert_array_equal(np.take(big[k], i, axis=0 if k in ("value", "grad") else 1),
                                              np.take(one[k], 0, axis=0 if k in ("value", "grad") else 1))
        # ... nor on the constraint strategy's mean-only sequence
        obj.set_cstr_strategy("mean", [1.0, 1.0])
        v, cs, g, gc = obj.constraints(c.xq, grad=True)
        np.testing.assert_array_equal(cs, big["mean"][1:].T)
        np.testing.assert_array_equal(gc, big["grad_mean"][1:].transpose(1, 0, 2))


# ---- 4. the believer property -------------------------------------------------------------------------------------------------
def test_kriging_believer_moves_nothing_but_the_variance(egx, mid):
    c = mid
    xs = c.xq[7]
    with egx.InfillObjective(c.hs[0], c.hs[1:], TOLS, criterion=egx.EI, fmin=c.fmin) as obj:
        base = obj.parts(c.xq[:40])
        at = obj.parts(xs)
        s2 = obj.pending[2]
        y = obj.virtual_point(xs, "kb")
        np.testing.assert_array_equal(y, at["mean"][:, 0])
        obj.push_pending(xs, y)
        p, pa = obj.parts(c.xq[:40]), obj.parts(xs)
        moved = np.max(np.abs(p["mean"][0] - base["mean"][0])) / np.max(np.abs(base["mean"][0]))
        print(f"believer: mean moved {moved:.2e}, var at x* {pa['var'][0, 0] / s2[0]:.2e} sigma2")
        assert moved <= 1e-9
        assert 0.0 <= pa["var"][0, 0] <= 1e-8 * s2[0]
        np.testing.assert_allclose(obj.pending[2], s2 * c.n / (c.n + 1.0), rtol=1e-9)
        obj.clear_pending()
        yu = obj.virtual_point(xs, egx.QEiStrategy.KB_UB)
        assert yu[0] == at["mean"][0, 0] + 3.0 * np.sqrt(at["var"][0, 0])
        assert obj.virtual_point(xs, "kb_lb")[0] == at["mean"][0, 0] - 3.0 * np.sqrt(at["var"][0, 0])
        obj.push_pending(xs, yu)
        np.testing.assert_allclose(obj.parts(xs)["mean"][0, 0], yu[0], rtol=PRED_RTOL)


# ---- 5. the batch call --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(egx, O):
    c = _case(egx, O, 300, 3, 1, 1.5, 0, 3)
    yield c
    _close(c)


@pytest.mark.parametrize("optimizer", ["slsqp", "cobyla"])
@pytest.mark.parametrize("strategy", ["kb", "cl_min"])
def test_batch_is_the_manual_loop_and_the_refit(egx, small, optimizer, strategy):
    c, q, ns = small, 4, 8
    lim = np.stack([c.lo, c.hi], axis=1)
    starts = c.lo + (c.hi - c.lo) * np.random.default_rng(17).random((q, ns, c.d))
    kw = dict(criterion=egx.LOG_EI, fmin=c.fmin)
    with egx.InfillObjective(c.hs[0], c.hs[1:], TOLS, **kw) as a, egx.InfillObjective(c.hs[0], c.hs[1:], TOLS, **kw) as b:
        x, yv, f, nf = a.optimize_batch(lim, starts, q, strategy=strategy, optimizer=optimizer)
        assert nf == 4
        for i in range(q):  # the loop a caller writes
            xi, fi = (b.optimize_slsqp(lim, starts[i])[:2] if optimizer == "slsqp" else b.optimize(lim, starts[i])[1::-1])
            yi = b.virtual_point(xi, strategy)
            b.push_pending(xi, yi)
            np.testing.assert_array_equal(x[i], xi)
            np.testing.assert_array_equal(yv[i], yi)
            assert f[i] == fi
        np.testing.assert_array_equal(a.pending[0], x)
        np.testing.assert_array_equal(a.pending[1], yv)
        if strategy == "cl_min":
            imin = int(np.argmin(c.ys[0]))
            np.testing.assert_array_equal(yv, np.tile([yj[imin] for yj in c.ys], (q, 1)))
        prm = a.params
        for i in range(q):  # f_out[i] from refits on the first i points
            refs = [g if i == 0 else PO.refit_frozen(g, x[:i], yv[:i, j]) for j, g in enumerate(c.gs)]
            mv = [r.predict_valvar(x[i:i + 1]) for r in refs]
            mean, var = np.array([float(m[0][0]) for m in mv]), np.array([float(m[1][0]) for m in mv])
            want = IO.objective(a.criterion, mean, var, TOLS, prm["fmin"], prm["sigma_weight"], prm["scale_ic"], prm["scale"],
                                prm["feasibility"], dev=True)
            print(f"{optimizer} {strategy} step {i}: f {f[i]:.12e} refit {want:.12e}")
            np.testing.assert_allclose(f[i], want, rtol=1e-6)


# ---- 6. errors and state ------------------------------------------------------------------------------------------------------
def test_errors_and_state(egx, small):
    c = small
    L = egx._lib
    rng = np.random.default_rng(3)
    with egx.InfillObjective(c.hs[0], c.hs[1:], TOLS, criterion=egx.EI, fmin=c.fmin) as obj:
        pts = c.lo + (c.hi - c.lo) * rng.random((17, c.d))
        for v in range(16):
            obj.push_pending(pts[v], obj.virtual_point(pts[v], "kb_ub"))
        with pytest.raises(L.InvalidValueError, match="at most 16"):
            obj.push_pending(pts[16], np.zeros(3))
        assert obj.pending[0].shape == (16, c.d)
        obj.clear_pending()
        bad = pts[0].copy()
        bad[1] = np.nan
        with pytest.raises(L.InvalidValueError, match="non-finite"):
            obj.push_pending(bad, np.zeros(3))
        with pytest.raises(L.InvalidValueError, match="non-finite"):
            obj.push_pending(pts[0], [0.0, np.inf, 0.0])
        assert obj.pending[0].shape == (0, c.d)  # the handle is as it was before the failed calls
    # a mixture and a sparse model among the surrogates
    gmx = egx.GaussianMixture([0.5, 0.5], [[0.3] * c.d, [0.7] * c.d], [np.eye(c.d) * 0.04] * 2, 0.8)
    mix = egx.GpMixture([egx.GaussianProcess(h, None) for h in c.hs[:2]], gmx, "smooth")
    with egx.InfillObjective(c.hs[0], [mix], [0.3], criterion=egx.EI, fmin=c.fmin) as obj:
        with pytest.raises(L.EgxError, match="surrogate 1") as e:
            obj.push_pending(pts[0], np.zeros(2))
        assert e.value.rc == L.ERR_UNSUPPORTED
    with egx.SgpHandle(c.x, c.ys[1], c.x[:24], corr=0, method=0) as sg:
        sg.finalize(np.full(c.d, 1.2), 1.0, 0.01)
        with egx.InfillObjective(c.hs[0], [sg], [0.3], criterion=egx.EI, fmin=c.fmin) as obj:
            with pytest.raises(L.EgxError, match="surrogate 1") as e:
                obj.push_pending(pts[0], np.zeros(2))
            assert e.value.rc == L.ERR_UNSUPPORTED
    # the constant liar needs every model on the same rows; a model refitted after a push
    with egx.GpHandle(c.x[:250], c.ys[1][:250], corr=3) as hc:
        hc.finalize(np.full(c.d, 1.5))
        with egx.InfillObjective(c.hs[0], [hc], [0.3], criterion=egx.EI, fmin=c.fmin) as obj:
            with pytest.raises(L.InvalidValueError, match="same rows"):
                obj.virtual_point(pts[0], "cl_min")
            obj.push_pending(pts[0], obj.virtual_point(pts[0], "kb"))
            obj.value(c.xq)
            hc.finalize(np.full(c.d, 1.1))
            with pytest.raises(L.InvalidValueError, match="refitted"):
                obj.value(c.xq)
            with pytest.raises(L.InvalidValueError, match="refitted"):
                obj.push_pending(pts[1], np.zeros(2))
            obj.clear_pending()
            assert np.all(np.isfinite(obj.value(c.xq)))
            obj.push_pending(pts[1], obj.virtual_point(pts[1], "kb"))
            assert np.all(np.isfinite(obj.value(c.xq)))


def test_a_pushed_point_is_cast_like_a_query(egx, O):
    from egobox_amd import workload
    x, y = workload.make_training_set(130, 3, seed=1)
    xt = [egx.XType.Float(0.0, 1.0), egx.XType.Int(0, 1), egx.XType.Float(0.0, 1.0)]
    xr = x.copy()
    xr[:, 1] = np.round(xr[:, 1])
    hs = []
    try:
        for yj in _ys(y)[:2]:
            h = egx.GpHandle(xr, yj, corr=3)
            h.finalize(np.full(3, 1.5))
            h.set_xtypes(xt)
            hs.append(h)
        raw = np.array([0.31, 0.74, 0.52])
        cast = np.array([0.31, 1.0, 0.52])
        xq = np.random.default_rng(4).random((20, 3))
        with egx.InfillObjective(hs[0], hs[1:], [0.3], criterion=egx.EI, fmin=0.0) as a, \
                egx.InfillObjective(hs[0], hs[1:], [0.3], criterion=egx.EI, fmin=0.0) as b:
            a.push_pending(raw, [0.1, -0.2])
            b.push_pending(cast, [0.1, -0.2])
            np.testing.assert_array_equal(a.pending[0], cast[None, :])
            for got, want in zip(a.pending, b.pending):
                np.testing.assert_array_equal(got, want)
            pa, pb = a.parts(xq), b.parts(xq)
            for k in KEYS:
                np.testing.assert_array_equal(pa[k], pb[k])
    finally:
        for h in hs:
            h.close()


# ---- 7. a C host --------------------------------------------------------------------------------------------------------------
def test_compiled_c_host_drives_the_pending_entry_points(tmp_path):
    exe = tmp_path / "infill_pending_driver"
    libdir = os.path.join(ROOT, "egobox_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "c_host", "infill_pending_driver.c"), f"-L{libdir}", "-legx_gp_hip", "-lm",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "PASS" in out.stdout


def test_reference_style_cpp_host_runs_the_batch(tmp_path):
    """tests/c_host/reference_style_pending.cpp: InfillObjective::optimize_batch and its steps through include/egx_gp.hpp"""
    exe = tmp_path / "reference_style_pending"
    libdir = os.path.join(ROOT, "egobox_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "c_host", "reference_style_pending.cpp"), f"-L{libdir}", "-legx_gp_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert out.stdout.startswith("OK")
