"""Sparse experts in the infill handle (egx_infill_create_any; sgp_expert_tile in egobox_amd/csrc/infill_eval.hip, the sparse tails
of kernels_infill.hip) and sparse mixtures (egx_moe_predict_valvar(_gradients)_sgp, SparseGpMix(n_clusters=k)) on the GPU.

Inputs of tests/test_gpu_sgp_surrogate.py::test_gradients_vs_analytic_oracle: problem(700, 40, 3, seed=corr), theta =
[1.3, 0.8, 1.1], sigma2 = 0.9, noise = 0.02, 333 queries of default_rng(9) (two full tiles and a partial one), all four kernels,
FITC and VFE; plus nz = 130 (beyond the 128 pad) for the absolute exponential and the two Materns -- the squared exponential
there has cond(Kmm) = 1.3e10, beyond what the oracle can arbitrate.  Bar: the project's prediction bar, rtol 1e-6
with the absolute floors of tests/test_gpu_infill.py::_check_parts (1e-9, 1e-9 sigma2, 1e-6 max|ref| for gradients)."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_infill import CRITERIA, PRED_RTOL, _check_criterion, _data, _grad_tol
from test_infill_mix_cpu import _bounds
from test_sgp_surrogate_cpu import KINDS, analytic_gradients, problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THETA, SIGMA2, NOISE = np.array([1.3, 0.8, 1.1]), 0.9, 0.02
KEYS = ("mean", "var", "grad_mean", "grad_var")
NAMES = ("value", "grad") + KEYS
CASES = [(corr, method, 40) for corr in range(4) for method in (0, 1)] + \
        [(corr, method, 130) for corr in (1, 2, 3) for method in (0, 1)]


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def S():
    from oracle import sgp_oracle
    return sgp_oracle


def _xq():
    return np.random.default_rng(9).random((333, 3)) * 2 - 1


_REF = {}


def _reference(S, corr, method, nz, theta=THETA):
    """(x, y, z, oracle mean, var, d mean, d var, raw variance) at the 333 queries; computed once per case, never changed"""
    key = (corr, method, nz, tuple(theta))
    if key not in _REF:
        x, y, z = problem(700, nz, 3, seed=corr)
        ref = S.SparseGpOracle(x, y, z, theta, SIGMA2, NOISE, corr=KINDS[corr], method=[S.FITC, S.VFE][method])
        xq = _xq()
        gy, gv, var_raw = analytic_gradients(ref, xq)
        for a in (gy, gv, var_raw):
            a.setflags(write=False)
        _REF[key] = SimpleNamespace(x=x, y=y, z=z, mean=np.ravel(ref.predict(xq)), var=np.ravel(ref.predict_var(xq)), gy=gy, gv=gv,
                                    var_raw=var_raw)
    return _REF[key]


def _sparse(egx, r, corr, method, theta=THETA):
    h = egx.SgpHandle(r.x, r.y, r.z, corr=corr, method=method)
    h.finalize(theta, SIGMA2, NOISE)
    return h


def _check_sparse_parts(p, j, r, label):
    """slot j of the parts against the oracle of case r; returns the worst errors (mean, var, d mean, d var; relative to the bar's
    scales) for the record"""
    keep = np.abs(r.var_raw - 1e-15) >= 1e-7 * SIGMA2  # the clamp decision is the oracle's beyond doubt
    clamped = keep & (r.var_raw < 1e-15)
    errs = (np.abs(p["mean"][j] - r.mean).max() / max(1.0, np.abs(r.mean).max()), np.abs(p["var"][j] - r.var).max() / SIGMA2,
            np.abs(p["grad_mean"][j] - r.gy).max() / np.abs(r.gy).max(),
            np.abs(p["grad_var"][j] - r.gv)[keep].max() / np.abs(r.gv).max())
    print(f"{label}: left out {(~keep).sum()} of {keep.size}, clamped {clamped.sum()}, worst errors mean {errs[0]:.3g} "
          f"var {errs[1]:.3g} grad_mean {errs[2]:.3g} grad_var {errs[3]:.3g}")
    assert (~keep).sum() <= 0.01 * keep.size
    np.testing.assert_allclose(p["mean"][j], r.mean, rtol=PRED_RTOL, atol=1e-9)
    np.testing.assert_allclose(p["var"][j], r.var, rtol=PRED_RTOL, atol=1e-9 * SIGMA2)
    np.testing.assert_allclose(p["grad_mean"][j], r.gy, **_grad_tol(r.gy))
    np.testing.assert_allclose(p["grad_var"][j][keep], r.gv[keep], **_grad_tol(r.gv))
    assert np.all(p["grad_var"][j][clamped] == 0.0)
    assert np.all(p["var"][j][clamped] == 1e-15 + NOISE)
    return clamped


# ---- 1: the parts of a sparse model against the oracle and against the handle's own predictions -------------------------------
@pytest.mark.parametrize("corr,method,nz", CASES)
def test_parts_vs_oracle(egx, S, corr, method, nz):
    r = _reference(S, corr, method, nz)
    xq = _xq()
    with _sparse(egx, r, corr, method) as h, egx.InfillObjective(h, criterion=egx.EI, fmin=float(np.quantile(r.y, 0.1))) as obj:
        p = obj.parts(xq)
        clamped = _check_sparse_parts(p, 0, r, f"corr {corr} method {method} nz {nz}")
        if method == 1 and nz == 40 and corr in (0, 3):
            assert clamped.sum() >= 1  # the clamp is exercised (92 and 2 of the first 300 where this was written)
        own = h.predict_valvar(xq) + h.predict_valvar_gradients(xq)
        np.testing.assert_allclose(p["mean"][0], own[0], rtol=PRED_RTOL, atol=1e-9)
        np.testing.assert_allclose(p["var"][0], own[1], rtol=PRED_RTOL, atol=1e-9 * SIGMA2)
        np.testing.assert_allclose(p["grad_mean"][0], own[2], **_grad_tol(own[2]))
        same = (own[3] == 0.0).all(axis=1) == (p["grad_var"][0] == 0.0).all(axis=1)  # both sides decide the clamp for themselves
        assert (~same).sum() <= 0.01 * same.size
        np.testing.assert_allclose(p["grad_var"][0][same], own[3][same], **_grad_tol(own[3]))
        ep = obj.expert_parts(0, xq)  # a lone expert: the surrogate's own slot, responsibilities of one
        for key in KEYS:
            np.testing.assert_array_equal(ep[key][0], p[key][0])
        assert np.all(ep["probas"] == 1.0) and np.all(ep["dprobas"] == 0.0)


# ---- 2: the criterion on a sparse objective with one sparse and one dense constraint ---------------------------------------
@pytest.fixture(scope="module")
def trio(egx, S):
    """a sparse objective (Matern-5/2, VFE), a sparse constraint (squared exponential, VFE: 92 clamped queries) and a dense one"""
    ro, rc = _reference(S, 3, 1, 40), _reference(S, 0, 1, 40)
    ho = _sparse(egx, ro, 3, 1)
    hc = egx.SgpHandle(rc.x, rc.y - np.quantile(rc.y, 0.6), rc.z, corr=0, method=1)
    hc.finalize(THETA, SIGMA2, NOISE)
    xd, yd = _data(150, 3, seed=3)
    hd = egx.GpHandle(2.0 * xd - 1.0, yd - np.quantile(yd, 0.6), corr=2)
    hd.finalize(np.full(3, 1.4))
    f = SimpleNamespace(ho=ho, hc=hc, hd=hd, ro=ro, xq=_xq(), tols=[0.3, 0.3], fmin=float(np.quantile(ro.y, 0.1)))
    yield f
    for h in (ho, hc, hd):
        h.close()


@pytest.mark.parametrize("crit", CRITERIA)
def test_criterion_is_the_arithmetic_of_its_parts(egx, trio, crit):
    f = trio
    kw = dict(criterion=crit, fmin=f.fmin, sigma_weight=0.75, scale_ic=1.9, scale=2.5)
    with egx.InfillObjective(f.ho, [f.hc, f.hd], f.tols, **kw) as obj:
        p = obj.parts(f.xq)
        wv, wg = _check_criterion(obj, p, f.tols)
        print(f"crit {crit} folded: value err {wv:.2e} grad err {wg:.2e}")
        assert np.all(np.isfinite(p["value"]))
        with egx.InfillObjective(f.hd, criterion=crit, fmin=f.fmin) as dense:  # the dense constraint beside sparse models: its bits alone
            dp = dense.parts(f.xq)
        for key in KEYS:
            np.testing.assert_array_equal(p[key][2], dp[key][0], err_msg=key)
    # the objective alone, then the same models with the constraints handed to the optimiser (mean: the MEAN-ONLY sequence)
    with egx.InfillObjective(f.ho, **kw) as bare:
        bp = bare.parts(f.xq)
        wv, wg = _check_criterion(bare, bp, [])
        print(f"crit {crit} bare: value err {wv:.2e} grad err {wg:.2e}")
    s = np.array([0.7, 1.9])
    for strategy in ("mean", "utb"):
        with egx.InfillObjective(f.ho, [f.hc, f.hd], f.tols, **kw) as obj:
            obj.set_cstr_strategy(strategy, s)
            v, c, g, gc = obj.constraints(f.xq, grad=True)
            v0, c0 = obj.constraints(f.xq)
            np.testing.assert_array_equal(v, bp["value"])
            np.testing.assert_array_equal(g, bp["grad"])
            np.testing.assert_array_equal(v0, v)
            np.testing.assert_array_equal(c0, c)
            np.testing.assert_array_equal(obj.value(f.xq), bp["value"])
            gm, gv = p["grad_mean"][1:].transpose(1, 0, 2), p["grad_var"][1:].transpose(1, 0, 2)
            if strategy == "mean":  # no solve was run: the means and their gradients keep the bits of the full sequence
                np.testing.assert_array_equal(c, p["mean"][1:].T / s)
                np.testing.assert_array_equal(gc, gm / s[None, :, None])
            else:
                sigma = np.sqrt(p["var"][1:].T)
                np.testing.assert_array_equal(c, (p["mean"][1:].T + 3.0 * sigma) / s)
                np.testing.assert_array_equal(gc, (gm + 3.0 * (gv / (2.0 * sigma[:, :, None]))) / s[None, :, None])


# ---- 3: a point does not depend on its companions nor on its position --------------------------------------------------------
def _point(p, i):
    return [p["value"][i], p["grad"][i]] + [p[k][:, i] for k in KEYS]


def test_a_point_does_not_depend_on_its_companions(egx, trio):
    f, xq = trio, trio.xq
    with egx.InfillObjective(f.hc, [f.ho, f.hd], f.tols, criterion=egx.LOG_EI, fmin=f.fmin) as obj:  # the clamping model first
        base = obj.parts(xq)
        assert (base["grad_var"][0] == 0.0).all(axis=1).sum() >= 50  # clamped queries among them
        rev = obj.parts(xq[::-1].copy())
        for i in range(333):
            for a, b, name in zip(_point(base, i), _point(rev, 332 - i), NAMES):
                np.testing.assert_array_equal(a, b, err_msg=f"{name} of point {i}: reversed order")
        for i in (0, 1, 17, 127, 128, 200, 255, 256, 332):  # alone: m = 1, whatever tile it sat in
            one = obj.parts(xq[i:i + 1])
            for a, b, name in zip(_point(base, i), _point(one, 0), NAMES):
                np.testing.assert_array_equal(a, b, err_msg=f"{name} of point {i}: alone")
        few = obj.parts(xq[120:137])  # 17 points: the other side of the sparse predict entry points' few-query switch
        for i in range(17):
            for a, b, name in zip(_point(base, 120 + i), _point(few, i), NAMES):
                np.testing.assert_array_equal(a, b, err_msg=f"{name} of point {120 + i}: among 17")
        np.testing.assert_array_equal(obj.value(xq), base["value"])  # grad = NULL: the same values
        v, g = obj.value_and_grad(xq)
        np.testing.assert_array_equal(v, base["value"])
        np.testing.assert_array_equal(g, base["grad"])
        bad = xq.copy()
        bad[129, 2] = np.nan  # in the second tile
        got = obj.parts(bad)
        assert got["value"][129] == np.inf and np.all(got["grad"][129] == 0.0)
        keep = np.arange(333) != 129
        for name in NAMES:
            if name in ("value", "grad"):
                np.testing.assert_array_equal(base[name][keep], got[name][keep], err_msg=name)
            else:
                np.testing.assert_array_equal(base[name][:, keep], got[name][:, keep], err_msg=name)
        vb = obj.value(bad)
        assert vb[129] == np.inf
        np.testing.assert_array_equal(vb[keep], base["value"][keep])


def test_dense_models_through_the_tagged_entry_keep_their_bits(egx, trio):
    f = trio
    gmx = egx.GaussianMixture([0.5, 0.5], [[-0.3, 0.0, 0.0], [0.3, 0.0, 0.0]], [np.eye(3) * 0.3] * 2, 0.9)
    mix = egx.GpMixture([egx.GaussianProcess(f.hd, None)] * 2, gmx, "smooth")
    for models in ((f.hd, [f.hd]), (mix, [f.hd])):
        kw = dict(criterion=egx.WB2, fmin=0.1)
        with egx.InfillObjective(models[0], models[1], [0.2], **kw) as old, \
                egx.InfillObjective(models[0], models[1], [0.2], tagged=True, **kw) as new:
            a, b = old.parts(f.xq), new.parts(f.xq)
            for name in NAMES:
                np.testing.assert_array_equal(a[name], b[name], err_msg=name)


# ---- 4: mixtures with sparse experts ----------------------------------------------------------------------------------------------
def _gmx3(egx):
    return egx.GaussianMixture([0.4, 0.35, 0.25], [[-0.4, 0.0, 0.1], [0.4, 0.1, -0.1], [0.0, -0.3, 0.3]],
                               [np.eye(3) * 0.25, np.eye(3) * 0.3, np.eye(3) * 0.2], 0.9)


@pytest.fixture(scope="module")
def experts3(egx, S):
    """three sparse experts (absolute exponential FITC, Matern-3/2 VFE at nz = 130, squared exponential VFE) and a dense one"""
    specs = [(1, 0, 40), (2, 1, 130), (0, 1, 40)]
    hs = [_sparse(egx, _reference(S, *sp), sp[0], sp[1]) for sp in specs]
    xd, yd = _data(150, 3, seed=5)
    hd = egx.GpHandle(2.0 * xd - 1.0, yd, corr=3)
    hd.finalize(np.full(3, 1.4))
    yield SimpleNamespace(sparse=hs, dense=hd)
    for h in hs + [hd]:
        h.close()


@pytest.mark.parametrize("mode", ["smooth", "hard"])
@pytest.mark.parametrize("which", ["sparse3", "mixed"])
def test_mixture_recombination_in_the_handle(egx, experts3, which, mode):
    xq = _xq()
    sp = [egx.SparseGaussianProcess(h, None) for h in experts3.sparse]
    members = sp if which == "sparse3" else [sp[0], egx.GaussianProcess(experts3.dense, None), sp[2]]
    gmx = _gmx3(egx)
    mix = egx.GpMixture(members, gmx, mode)
    with egx.InfillObjective(mix, criterion=egx.EI, fmin=0.0) as obj:
        p, ep = obj.parts(xq), obj.expert_parts(0, xq)
        np.testing.assert_array_equal(ep["probas"], gmx.predict_probas_device(xq))
        np.testing.assert_array_equal(ep["dprobas"], gmx.predict_probas_derivatives_device(xq))
        for e, member in enumerate(members):  # the expert tables hold what the expert alone gives
            with egx.InfillObjective(member, criterion=egx.EI, fmin=0.0) as single:
                spart = single.parts(xq)
            for key in KEYS:
                np.testing.assert_array_equal(ep[key][e], spart[key][0], err_msg=f"expert {e} {key}")
        if mode == "hard":
            win = np.argmax(ep["probas"], axis=1)
            assert len(set(win)) == 3
            for key in KEYS:
                np.testing.assert_array_equal(p[key][0], ep[key][win, np.arange(xq.shape[0])], err_msg=key)
        else:
            worst = 0.0
            for i in range(xq.shape[0]):  # the formulas of infill_mix_math.h on the expert parts, within the CPU test's bound
                pr, dp = ep["probas"][i], ep["dprobas"][i]
                mu, v, gmu, gv = ep["mean"][:, i], ep["var"][:, i], ep["grad_mean"][:, i], ep["grad_var"][:, i]
                want = (np.sum(pr * mu), np.sum(pr * pr * v), np.sum(pr[:, None] * gmu + dp * mu[:, None], axis=0),
                        np.sum(pr[:, None] ** 2 * gv + 2.0 * pr[:, None] * dp * v[:, None], axis=0))
                got = (p["mean"][0, i], p["var"][0, i], p["grad_mean"][0, i], p["grad_var"][0, i])
                for g, w, b in zip(got, want, _bounds(pr, dp, mu, v, gmu, gv)):
                    assert np.all(np.abs(g - w) <= b), (i, g, w, b)
                    worst = max(worst, float(np.max(np.abs(g - w) / np.where(b > 0, b, 1.0))))
            print(f"{which} smooth: worst error / bound {worst:.3f}")
        for crit in CRITERIA:
            with egx.InfillObjective(mix, [experts3.sparse[1]], [0.2], criterion=crit, fmin=0.0, sigma_weight=0.8) as cobj:
                _check_criterion(cobj, cobj.parts(xq), [0.2])


@pytest.mark.parametrize("mode", ["smooth", "hard"])
def test_sparse_mixture_predictions_through_the_library(egx, experts3, mode):
    xq = _xq()
    hs = experts3.sparse
    gmx = _gmx3(egx)
    mix = egx.GpMixture([egx.SparseGaussianProcess(h, None) for h in hs], gmx, mode)
    ids, handles, sparse = mix._library_handles()
    assert sparse and ids == [0, 1, 2]
    val, var = mix.predict_valvar(xq)
    gy, gv = mix.predict_valvar_gradients(xq)
    np.testing.assert_array_equal(mix.predict(xq), val)  # one output alone: the same bits
    np.testing.assert_array_equal(mix.predict_var(xq), var)
    np.testing.assert_array_equal(mix.predict_gradients(xq), gy)
    np.testing.assert_array_equal(mix.predict_var_gradients(xq), gv)
    pr, dpr = gmx.predict_probas_device(xq), gmx.predict_probas_derivatives_device(xq)
    if mode == "hard":  # every point is its routed expert's row, bit for bit
        win = np.argmax(pr, axis=1)
        for e, h in enumerate(hs):
            idx = np.flatnonzero(win == e)
            assert idx.size > 16
            y, v = h.predict_valvar(xq[idx])
            dy, dv = h.predict_valvar_gradients(xq[idx])
            for got, want in ((val, y), (var, v), (gy, dy), (gv, dv)):
                np.testing.assert_array_equal(got[idx], want)
        return
    own = [h.predict_valvar(xq) + h.predict_valvar_gradients(xq) for h in hs]
    mu, v = np.stack([o[0] for o in own], axis=1), np.stack([o[1] for o in own], axis=1)  # (m, k)
    gmu, gvv = np.stack([o[2] for o in own], axis=1), np.stack([o[3] for o in own], axis=1)  # (m, k, d)
    want = (np.sum(pr * mu, axis=1), np.sum(pr * pr * v, axis=1), np.sum(pr[:, :, None] * gmu + dpr * mu[:, :, None], axis=1),
            np.sum(pr[:, :, None] ** 2 * gvv + 2.0 * pr[:, :, None] * dpr * v[:, :, None], axis=1))
    np.testing.assert_allclose(val, want[0], rtol=PRED_RTOL, atol=1e-9)
    np.testing.assert_allclose(var, want[1], rtol=PRED_RTOL, atol=1e-9 * SIGMA2)
    np.testing.assert_allclose(gy, want[2], **_grad_tol(want[2]))
    np.testing.assert_allclose(gv, want[3], **_grad_tol(want[3]))


# ---- 5: a sparse objective re-finalised between two calls -----------------------------------------------------------------------
def test_a_refinalised_sparse_objective_is_followed(egx, S):
    theta2 = np.array([0.9, 1.4, 0.7])
    r1, r2 = _reference(S, 3, 0, 40), _reference(S, 3, 0, 40, theta=theta2)
    xq = _xq()
    with _sparse(egx, r1, 3, 0) as h, egx.InfillObjective(h, criterion=egx.EI, fmin=0.0) as obj:
        _check_sparse_parts(obj.parts(xq), 0, r1, "before the refit")
        h.finalize(theta2, SIGMA2, NOISE)
        p = obj.parts(xq)
        _check_sparse_parts(p, 0, r2, "after the refit")
        with egx.InfillObjective(h, criterion=egx.EI, fmin=0.0) as fresh:
            q = fresh.parts(xq)
        for name in NAMES:
            np.testing.assert_array_equal(p[name], q[name], err_msg=name)


# ---- 6: the lock-step multistarts on a sparse objective ------------------------------------------------------------------------
def test_multistarts_on_a_sparse_objective(egx, trio):
    f, d = trio, 3
    lim = np.array([[-1.0, 1.0]] * d)
    starts = np.random.default_rng(6).random((8, d)) * 2 - 1
    with egx.InfillObjective(f.ho, [f.hc, f.hd], f.tols, criterion=egx.LOG_EI, fmin=f.fmin) as obj:
        fb, xb, st = obj.optimize(lim, starts, max_eval=40)
        assert st["finite"] and obj.value(xb)[0] == fb
        singles = [obj.optimize(lim, starts[i:i + 1], max_eval=40) for i in range(8)]
        np.testing.assert_array_equal(st["evals"], [s[2]["evals"][0] for s in singles])  # every start walks its own points
        fs = np.array([s[0] for s in singles])
        best = int(np.argmin(fs))
        assert st["best_start"] == best and fb == fs[best]
        np.testing.assert_array_equal(xb, singles[best][1])
        assert st["rounds"] == max(st["evals"])
        obj.set_cstr_strategy("mean", [0.7, 1.9])
        xc, fc, cc, cst = obj.optimize_constrained(lim, starts, max_eval=40)
        v, c = obj.constraints(xc[None, :])
        assert cst["finite"] and v[0] == fc
        np.testing.assert_array_equal(c[0], cc)
        csingles = [obj.optimize_constrained(lim, starts[i:i + 1], max_eval=40) for i in range(8)]
        np.testing.assert_array_equal(cst["evals"], [s[3]["evals"][0] for s in csingles])
        b = cst["best_start"]
        np.testing.assert_array_equal(xc, csingles[b][0])
        assert fc == csingles[b][1]
        np.testing.assert_array_equal(cc, csingles[b][2])


# ---- 7: errors ----------------------------------------------------------------------------------------------------------------------
def test_refusals(egx, trio):
    f = trio
    x, y, z = problem(120, 20, 3, seed=8)
    x2, y2, z2 = problem(120, 20, 2, seed=9)
    with egx.SgpHandle(x, y, z) as unfit, egx.SgpHandle(x2, y2, z2) as other:
        other.finalize(np.full(2, 1.2), SIGMA2, NOISE)
        with pytest.raises(egx.NotFittedError, match="surrogate 1 expert 0.*egx_sgp_finalize"):
            egx.InfillObjective(f.ho, [unfit], [0.0])
        with pytest.raises(egx.NotFittedError, match="surrogate 0 expert 0"):
            egx.InfillObjective(unfit)
        gmx = egx.GaussianMixture([0.5, 0.5], [[-0.3, 0.0, 0.0], [0.3, 0.0, 0.0]], [np.eye(3) * 0.3] * 2)
        with pytest.raises(egx.NotFittedError, match="surrogate 0 expert 1"):
            egx.InfillObjective(egx.GpMixture([egx.SparseGaussianProcess(f.ho, None), egx.SparseGaussianProcess(unfit, None)], gmx, "hard"))
        with pytest.raises(egx.InvalidValueError, match="surrogate 1 expert 0 has 2 inputs"):
            egx.InfillObjective(f.ho, [other], [0.0])
        with pytest.raises(egx.InvalidValueError, match="surrogate 2 expert 0 has 2 inputs"):
            egx.InfillObjective(f.hd, [f.hc, other], [0.0, 0.0])
        # a model unfitted AFTER the handle was built (a likelihood evaluation overwrites the factors): named at the call
        with egx.SgpHandle(x, y, z) as later:
            later.finalize(THETA, SIGMA2, NOISE)
            with egx.InfillObjective(f.ho, [later], [0.0]) as obj:
                assert np.all(np.isfinite(obj.value(f.xq[:5])))
                later.likelihood(THETA, SIGMA2, NOISE)
                with pytest.raises(egx.NotFittedError, match="surrogate 1 expert 0"):
                    obj.value(f.xq[:5])
        # typed dense models beside sparse ones: all or none
        xt = [egx.XType.Float(-1.0, 1.0), egx.XType.Int(-1, 1), egx.XType.Float(-1.0, 1.0)]
        f.hd.set_xtypes(xt)
        try:
            with pytest.raises(egx.InvalidValueError, match="xtypes"):
                egx.InfillObjective(f.ho, [f.hd], [0.0])
            with pytest.raises(egx.InvalidValueError, match="xtypes"):
                egx.InfillObjective(f.hd, [f.ho], [0.0])
        finally:
            f.hd.set_xtypes(None)


# ---- 8: training a sparse mixture -------------------------------------------------------------------------------------------------
def _two_regimes(n=600, seed=4):
    rng = np.random.default_rng(seed)
    x = rng.random((n, 2))
    left = x[:, 0] < 0.5
    y = np.where(left, np.sin(6.0 * x[:, 0]) + x[:, 1], 3.0 + 0.5 * np.cos(5.0 * x[:, 1]) - x[:, 0]) + 0.01 * rng.standard_normal(n)
    return x, y


@pytest.mark.parametrize("mode", ["hard", "smooth"])
def test_training_a_sparse_mixture(egx, mode):
    from egobox_amd.sgp import SparseGpMix
    x, y = _two_regimes()
    xq = np.random.default_rng(5).random((150, 2))
    model = SparseGpMix(corr_spec=8, n_clusters=2, nz=30, recombination=mode, n_start=2, seed=7, theta_bounds=[[0.05, 20.0]]).fit(x, y)
    moe = model._moe
    assert moe.recombination == mode and len(moe.experts) == 2
    assert model.thetas().shape == (2, 2) and model.variances().shape == (2,) and model.likelihoods().shape == (2,)
    assert all(e.inducings().shape == (30, 2) for e in moe.experts)
    sizes = [e._h.n for e in moe.experts]
    assert sum(sizes) == 600 and min(sizes) >= 30  # every row went to one expert, every expert could draw its 30 inducing points
    val, var = model.predict_valvar(xq)
    pr = moe.gmx.predict_probas_device(xq)
    own = [e.predict_valvar(xq) for e in moe.experts]
    if mode == "hard":
        win = np.argmax(pr, axis=1)
        for e, expert in enumerate(moe.experts):
            idx = np.flatnonzero(win == e)
            assert idx.size > 0
            yv = expert.predict_valvar(xq[idx])
            np.testing.assert_array_equal(val[idx], yv[0])
            np.testing.assert_array_equal(var[idx], yv[1])
    else:
        assert moe.gmx.heaviside_factor in list(egx.moe.HEAVISIDE_GRID) + [1.0]  # Smooth(None): chosen on one row out of five
        tm = np.stack([pr[:, e] * own[e][0] for e in range(2)])
        tv = np.stack([pr[:, e] ** 2 * own[e][1] for e in range(2)])
        c = 4.0 * 3 * np.finfo(float).eps  # 4 (k + 1) eps sum |terms|: the bound of tests/test_infill_mix_cpu.py
        assert np.all(np.abs(val - tm.sum(axis=0)) <= c * np.abs(tm).sum(axis=0))
        assert np.all(np.abs(var - tv.sum(axis=0)) <= c * np.abs(tv).sum(axis=0))
    resid = model.predict(x) - y
    print(f"{mode}: cluster sizes {sizes}, rmse on the training rows {np.sqrt(np.mean(resid ** 2)):.3g}, std of y {y.std():.3g}")
    assert np.sqrt(np.mean(resid ** 2)) < 0.5 * y.std()  # a trained model, not a constant (the regimes differ by about 3)
    with egx.InfillObjective(model, criterion=egx.EI, fmin=float(y.min())) as obj:
        p = obj.parts(xq)
        assert np.all(np.isfinite(p["value"])) and np.all(np.isfinite(p["grad"]))
        np.testing.assert_allclose(p["mean"][0], val, rtol=PRED_RTOL, atol=1e-9)
        np.testing.assert_allclose(p["var"][0], var, rtol=PRED_RTOL, atol=1e-9 * float(np.max(model.variances())))


def test_one_cluster_is_the_single_sparse_model(egx):
    from egobox_amd.sgp import Inducings, SgpParams, SparseGpMix
    x, y = _two_regimes(300, seed=11)
    xq = np.random.default_rng(5).random((40, 2))
    a = SparseGpMix(corr_spec=8, nz=25, n_start=2, seed=3, n_clusters=1, recombination="hard").fit(x, y)
    b = SgpParams(egx.Matern52Corr(), Inducings.Randomized(25)).n_start(2).seed(3).fit(x, y)
    try:
        assert a._moe is None
        np.testing.assert_array_equal(a.thetas(), b.theta()[None, :])
        for got, want in zip(a.predict_valvar(xq), b.predict_valvar(xq)):
            np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(a.likelihoods(), [b.likelihood()])
        with egx.InfillObjective(a, criterion=egx.EI, fmin=float(y.min())) as obj:
            assert np.all(np.isfinite(obj.value(xq)))
    finally:
        a._sgp.close()
        b.close()


# ---- 9: a plain C host ------------------------------------------------------------------------------------------------------------
def test_plain_c_host_drives_the_sparse_entry_points(tmp_path):
    exe = tmp_path / "infill_sparse_driver"
    libdir = os.path.join(ROOT, "egobox_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "c_host", "infill_sparse_driver.c"), f"-L{libdir}", "-legx_gp_hip", "-lm",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert out.stdout.startswith("OK"), out.stdout
