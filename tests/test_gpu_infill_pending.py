"""Pending points on the infill handle (egx_infill_push_pending and friends; infill_pending.hip, kernels_pending.hip, pending_math.h):
the conditioned parts against an actual refit with frozen normalisation (tests/pending_oracle.py on oracle.gp_oracle), the
criterion as the arithmetic of those parts, the exactness of the switch, the believer property, the batch call against the
manual loop and against the refit, errors and state, a C host."""
import os
import subprocess

import numpy as np
import pytest

from pending_cases import (KEYS, PRED_RTOL, TOLS, _assert_conditioned, _case, _check_batch, _check_clear_pending,
                           _check_companions, _check_composed_form, _check_parts_against_refit, _close, _push_all, _ys)
from test_gpu_infill import CRITERIA, _check_criterion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


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
            _check_composed_form(egx, c, obj)
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
def test_clear_pending_gives_back_the_fitted_handle_bit_for_bit(egx, mid):
    _check_clear_pending(egx, mid)


def test_a_conditioned_point_does_not_depend_on_its_companions(egx, mid):
    _check_companions(egx, mid)  # 131 points: two tiles, the second ragged


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
    _check_batch(egx, small, 4, 8, optimizer, strategy)


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
