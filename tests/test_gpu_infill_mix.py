"""The infill criterion on mixtures of experts (egx_infill_create_mix, k_infill_mix; egobox_amd/csrc/infill_eval.hip,
kernels_infill.hip, infill_mix_math.h, gmx_point.h): a handle of single experts against the old entry point bit for bit, the
surrogate parts against the library's mixture predictions, the criterion against tests/infill_oracle.py on those parts, the
expert diagnostics, the bit-independence of a point from its companions, NaN points, the lock-step multistart, a re-finalised
expert, refusals, a plain C host, and an expert above 1024 rows."""
import os
import subprocess

import numpy as np
import pytest

import infill_oracle as IO
from test_gpu_infill import CRITERIA, PRED_RTOL, _check_criterion, _data, _grad_tol, _queries
from test_infill_mix_cpu import _bounds

gpu = pytest.mark.gpu
NS = {3: [300, 250, 200, 280, 220, 260], 4: [300, 250, 200, 280, 220, 260]}  # objective's three experts, constraint 1's two, constraint 2
M_UNIFORM = 40
KEYS = ("mean", "var", "grad_mean", "grad_var")


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


# ---- the fixture: six experts on their own training sets, two explicit mixtures that overlap inside the query box -----------
def _training_sets(d):
    """expert e: its own n, seed; objective experts scaled like the suite's objective models (test_gpu_infill._data)"""
    sets = []
    for e, n in enumerate(NS[d]):
        x, y = _data(n, d, seed=70 + 10 * d + e, yscale=1e-3 if e < 3 else 1.0)
        if e >= 3:
            y = y - np.quantile(y, 0.6)  # feasible (<= tol) on a good part of the box
        sets.append((x, y))
    return sets


def _gmx3(d, hf=0.9):
    from egobox_amd.moe import GaussianMixture
    means = np.full((3, d), 0.5)
    means[:, 0] = [0.2, 0.5, 0.8]
    means[:, 1] = [0.45, 0.6, 0.5]
    covs = np.stack([np.eye(d) * s for s in (0.06, 0.05, 0.07)])
    covs[0][0, 1] = covs[0][1, 0] = 0.01  # a full (non-diagonal) covariance
    return GaussianMixture([0.3, 0.3, 0.4], means, covs, hf)


def _gmx2(d):
    from egobox_amd.moe import GaussianMixture
    means = np.full((2, d), 0.5)
    means[:, d - 1] = [0.3, 0.7]
    return GaussianMixture([0.45, 0.55], means, np.stack([np.eye(d) * 0.08, np.eye(d) * 0.06]), 1.0)


def _fixture_queries(d, sets):
    """`_queries`-style uniform points plus one training point of each of the objective's experts"""
    rng = np.random.default_rng(500 + d)
    x0 = sets[0][0]
    lo, hi = x0.min(axis=0), x0.max(axis=0)
    return np.vstack([lo + (hi - lo) * rng.random((M_UNIFORM, d)), sets[0][0][0], sets[1][0][sets[1][0].shape[0] // 2],
                      sets[2][0][-1]])


def _assert_overlap(gmx, xq):
    """every expert wins at least 5 points, at least 10 points are undecided, and no point sits on a tie"""
    p = gmx.predict_probas(xq)
    wins = np.bincount(np.argmax(p, axis=1), minlength=gmx.n_clusters)
    assert np.all(wins >= 5), wins
    assert np.sum(p.max(axis=1) < 0.9) >= 10, np.sum(p.max(axis=1) < 0.9)
    top = np.sort(p, axis=1)
    assert np.all(top[:, -1] - top[:, -2] > 1e-6), np.min(top[:, -1] - top[:, -2])


@pytest.mark.parametrize("d", [3, 4])
def test_fixture_mixtures_overlap_inside_the_query_box(d):
    """numpy only: what the GPU tests below rely on"""
    xq = _fixture_queries(d, _training_sets(d))
    assert xq.shape == (M_UNIFORM + 3, d)
    _assert_overlap(_gmx3(d), xq)
    _assert_overlap(_gmx2(d), xq)


class _Fix:
    pass


def _build(egx, d):
    f = _Fix()
    f.d, f.sets = d, _training_sets(d)
    f.handles = []
    for e, (x, y) in enumerate(f.sets):
        h = egx.GpHandle(x, y, mean=e % 2, corr=[0, 3, 2, 1, 0, 3][e])
        h.finalize(np.full(d, 1.2 + 0.1 * e))
        f.handles.append(h)
    gps = [egx.GaussianProcess(h, None) for h in f.handles]
    one = egx.GaussianMixture([1.0], np.full((1, d), 0.5), [np.eye(d)])
    f.obj = egx.GpMixture(gps[:3], _gmx3(d), "smooth")
    f.obj_hard = egx.GpMixture(gps[:3], _gmx3(d), "hard")
    f.c1 = egx.GpMixture(gps[3:5], _gmx2(d), "hard")
    f.c2 = egx.GpMixture(gps[5:6], one, "smooth")
    f.xq = _fixture_queries(d, f.sets)
    _assert_overlap(f.obj.gmx, f.xq)
    _assert_overlap(f.c1.gmx, f.xq)
    f.fmin = float(np.quantile(f.sets[0][1], 0.1))
    f.sigma2 = [max(float(e.handle.inner()["sigma2"]) for e in mix.experts) for mix in (f.obj, f.c1, f.c2)]
    # the library's own mixture predictions (the parity-tested path), computed once and left unchanged
    f.ref = []
    for mix in (f.obj, f.c1, f.c2):
        val, var = mix.predict_valvar(f.xq)
        gy, gv = mix.predict_valvar_gradients(f.xq)
        f.ref.append((val, var, gy, gv))
    return f


@pytest.fixture(scope="module", params=[3, 4])
def fix(request, egx):
    f = _build(egx, request.param)
    yield f
    for h in f.handles:
        h.close()


def _point(p, i):
    return [p["value"][i], p["grad"][i], p["mean"][:, i], p["var"][:, i], p["grad_mean"][:, i], p["grad_var"][:, i]]


NAMES = ("value", "grad") + KEYS


# ---- 1: k = 1 through the new entry is the old entry ------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("crit", CRITERIA)
def test_single_experts_through_the_new_entry_equal_the_old_entry(egx, fix, crit):
    d = fix.d
    one = egx.GaussianMixture([1.0], np.full((1, d), 0.5), [np.eye(d)])
    kw = dict(criterion=crit, fmin=fix.fmin, sigma_weight=0.75, scale_ic=2.3, scale=1.7)
    with egx.InfillObjective(fix.handles[0], [fix.handles[5]], [0.3], **kw) as old, \
            egx.InfillObjective(egx.GpMixture([egx.GaussianProcess(fix.handles[0], None)], one, "smooth"), [fix.handles[5]], [0.3],
                                **kw) as new:
        a, b = old.parts(fix.xq), new.parts(fix.xq)
        for name in NAMES:
            np.testing.assert_array_equal(a[name], b[name], err_msg=name)
        np.testing.assert_array_equal(old.value(fix.xq), new.value(fix.xq))
        ep = new.expert_parts(0, fix.xq)
        np.testing.assert_array_equal(ep["probas"], 1.0)
        np.testing.assert_array_equal(ep["dprobas"], 0.0)
        for key in KEYS:
            np.testing.assert_array_equal(ep[key][0], b[key][0])


# ---- 2 + 3: parts are the mixture's predictions, the criterion is the arithmetic of its parts --------------------------------
def _check_mix_parts(p, refs, sigma2s):
    for j, ((val, var, gy, gv), s2) in enumerate(zip(refs, sigma2s)):
        np.testing.assert_allclose(p["mean"][j], val, rtol=PRED_RTOL, atol=1e-9)
        np.testing.assert_allclose(p["var"][j], var, rtol=PRED_RTOL, atol=1e-9 * s2)
        np.testing.assert_allclose(p["grad_mean"][j], gy, **_grad_tol(gy))
        np.testing.assert_allclose(p["grad_var"][j], gv, **_grad_tol(gv))


@gpu
def test_parts_are_the_mixture_predictions(egx, fix):
    with egx.InfillObjective(fix.obj, [fix.c1, fix.c2], [0.3, 0.3], criterion=egx.EI, fmin=fix.fmin) as obj:
        p = obj.parts(fix.xq)
    _check_mix_parts(p, fix.ref, fix.sigma2)


@gpu
@pytest.mark.parametrize("feas", [True, False])
@pytest.mark.parametrize("crit", CRITERIA)
def test_criterion_is_the_arithmetic_of_its_parts(egx, fix, crit, feas):
    tols = [0.3, 0.3]
    with egx.InfillObjective(fix.obj, [fix.c1, fix.c2], tols, criterion=crit, fmin=fix.fmin, sigma_weight=0.75, feasibility=feas,
                             scale_ic=1.9, scale=2.5) as obj:
        wv, wg = _check_criterion(obj, obj.parts(fix.xq), tols)
    print(f"d {fix.d} crit {crit} feas {feas}: value err {wv:.2e} grad err {wg:.2e}")


# ---- 4: the diagnostics -------------------------------------------------------------------------------------------------------
@gpu
def test_expert_parts(egx, fix):
    xq, d = fix.xq, fix.d
    with egx.InfillObjective(fix.obj, [fix.c1, fix.c2], [0.3, 0.3], criterion=egx.EI, fmin=fix.fmin) as obj:
        p = obj.parts(xq)
        for j, mix in enumerate((fix.obj, fix.c1)):
            ep = obj.expert_parts(j, xq)
            k = mix.gmx.n_clusters
            assert ep["mean"].shape == (k, xq.shape[0]) and ep["dprobas"].shape == (xq.shape[0], k, d)
            np.testing.assert_array_equal(ep["probas"], mix.gmx.predict_probas_device(xq))
            np.testing.assert_array_equal(ep["dprobas"], mix.gmx.predict_probas_derivatives_device(xq))
            for e, expert in enumerate(mix.experts):  # the expert tables hold what the expert alone gives
                with egx.InfillObjective(expert.handle, criterion=egx.EI, fmin=fix.fmin) as single:
                    sp = single.parts(xq)
                for key in KEYS:
                    np.testing.assert_array_equal(ep[key][e], sp[key][0], err_msg=f"surrogate {j} expert {e} {key}")
            if mix.recombination == "hard":  # the selection: the winner's parts, exactly
                win = np.argmax(ep["probas"], axis=1)
                for key in KEYS:
                    np.testing.assert_array_equal(p[key][j], ep[key][win, np.arange(xq.shape[0])], err_msg=key)
                continue
            worst = 0.0
            for i in range(xq.shape[0]):  # smooth: the numpy fold of the expert parts, within the bound of the CPU test
                pr, dp = ep["probas"][i], ep["dprobas"][i]
                mu, v, gmu, gv = ep["mean"][:, i], ep["var"][:, i], ep["grad_mean"][:, i], ep["grad_var"][:, i]
                want = (np.sum(pr * mu), np.sum(pr * pr * v), np.sum(pr[:, None] * gmu + dp * mu[:, None], axis=0),
                        np.sum(pr[:, None] ** 2 * gv + 2.0 * pr[:, None] * dp * v[:, None], axis=0))
                got = (p["mean"][j, i], p["var"][j, i], p["grad_mean"][j, i], p["grad_var"][j, i])
                for g, w, b in zip(got, want, _bounds(pr, dp, mu, v, gmu, gv)):
                    assert np.all(np.abs(g - w) <= b), (j, i, g, w, b)
                    worst = max(worst, float(np.max(np.abs(g - w) / np.where(b > 0, b, 1.0))))
            print(f"d {d} surrogate {j}: worst smooth error / bound {worst:.3f}")


# ---- 5: a point does not depend on its companions -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["smooth", "hard"])
def test_a_point_does_not_depend_on_its_companions(egx, fix, mode):
    d = fix.d
    rng = np.random.default_rng(9)
    pts = np.vstack([rng.random((61, d)), fix.xq[-3:]])  # 64 points, three of them training points of the objective's experts
    fill = rng.random((200, d))
    with egx.InfillObjective(fix.obj if mode == "smooth" else fix.obj_hard, [fix.c1, fix.c2], [0.3, 0.3], criterion=egx.LOG_EI,
                             fmin=fix.fmin) as obj:
        base = obj.parts(pts)
        rev = obj.parts(pts[::-1].copy())
        big = fill.copy()
        big[100:164] = pts  # across the boundary of the 128-point tiles
        bigp = obj.parts(big)
        nine = obj.parts(pts[:9])
        for i in range(64):
            for a, b, c, name in zip(_point(base, i), _point(rev, 63 - i), _point(bigp, 100 + i), NAMES):
                np.testing.assert_array_equal(a, b, err_msg=f"{name} of point {i}: reversed order")
                np.testing.assert_array_equal(a, c, err_msg=f"{name} of point {i}: inside 200 points")
        for i in range(9):
            for a, b, name in zip(_point(base, i), _point(nine, i), NAMES):
                np.testing.assert_array_equal(a, b, err_msg=f"{name} of point {i}: m = 9")
        for i in range(64):
            one = obj.parts(pts[i:i + 1])
            for a, b, name in zip(_point(base, i), _point(one, 0), NAMES):
                np.testing.assert_array_equal(a, b, err_msg=f"{name} of point {i}: alone")
        np.testing.assert_array_equal(obj.value(pts), base["value"])  # grad = NULL: the same values
        v, g = obj.value_and_grad(pts)
        np.testing.assert_array_equal(v, base["value"])
        np.testing.assert_array_equal(g, base["grad"])


# ---- 6: one NaN point among 130 ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["smooth", "hard"])
def test_one_nan_point_among_130(egx, fix, mode):
    d = fix.d
    pts = np.random.default_rng(12).random((130, d))
    bad = pts.copy()
    bad[128, d - 1] = np.nan  # in the second tile, next to one good point
    with egx.InfillObjective(fix.obj if mode == "smooth" else fix.obj_hard, [fix.c1, fix.c2], [0.3, 0.3], criterion=egx.WB2,
                             fmin=fix.fmin) as obj:
        good, got = obj.parts(pts), obj.parts(bad)
        assert got["value"][128] == np.inf and np.all(got["grad"][128] == 0.0)
        keep = np.arange(130) != 128
        for name in NAMES:
            a, b = (good[name], got[name]) if name in ("value", "grad") else (good[name][:, keep], got[name][:, keep])
            if name in ("value", "grad"):
                a, b = a[keep], b[keep]
            np.testing.assert_array_equal(a, b, err_msg=name)
        np.testing.assert_array_equal(obj.value(bad)[keep], good["value"][keep])
        assert obj.value(bad)[128] == np.inf


# ---- 7: the multistart on a two-cluster toy ---------------------------------------------------------------------------------
@gpu
def test_lockstep_multistart_on_a_two_cluster_toy(egx):
    d = 2
    hs = []
    try:
        for e, n in enumerate((90, 70, 80)):
            x, y = _data(n, d, seed=141 + e, yscale=1.0)
            h = egx.GpHandle(x, y - (np.quantile(y, 0.6) if e == 2 else 0.0), corr=[0, 3, 2][e])
            h.finalize(np.full(d, 1.3 + 0.2 * e))
            hs.append(h)
        gmx = egx.GaussianMixture([0.5, 0.5], [[0.3, 0.5], [0.7, 0.5]], [np.eye(2) * 0.04] * 2, 0.8)
        mix = egx.GpMixture([egx.GaussianProcess(h, None) for h in hs[:2]], gmx, "smooth")
        lim = np.array([[0.0, 1.0]] * d)
        starts = np.random.default_rng(6).random((5, d))
        pts = np.random.default_rng(7).random((150, d))
        kw = dict(criterion=egx.LOG_EI, fmin=float(np.quantile(_data(90, d, seed=141)[1], 0.1)))
        with egx.InfillObjective(mix, [hs[2]], [0.3], **kw) as obj:
            scale_ic, scale, scale_cstr = obj.scaling(pts)
            assert scale_ic == 1.0 and obj.params["scale"] == scale
            with egx.InfillObjective(mix, [hs[2]], [0.3], **kw, scale_ic=scale_ic, scale=1.0) as unit:
                vals, full = unit.value(pts), unit.parts(pts)
            assert np.all(np.isfinite(vals))
            assert scale == np.max(np.abs(vals))  # as test_gpu_infill.test_scaling
            np.testing.assert_array_equal(scale_cstr, [np.max(np.abs(full["mean"][1]))])
            f, xb, st = obj.optimize(lim, starts, max_eval=40)
            singles = [obj.optimize(lim, starts[i:i + 1], max_eval=40) for i in range(5)]
            np.testing.assert_array_equal(st["evals"], [s[2]["evals"][0] for s in singles])
            fs = np.array([s[0] for s in singles])
            best = int(np.argmin(fs))
            assert st["best_start"] == best and f == fs[best]
            np.testing.assert_array_equal(xb, singles[best][1])
            assert st["rounds"] == max(st["evals"])
            assert obj.value(xb)[0] == f
    finally:
        for h in hs:
            h.close()


# ---- 8: an expert re-finalised between two calls ----------------------------------------------------------------------------
@gpu
def test_a_refinalised_expert_is_followed(egx):
    d = 3
    hs = []
    try:
        for e, n in enumerate((120, 100)):
            x, y = _data(n, d, seed=151 + e)
            h = egx.GpHandle(x, y, corr=e)
            h.finalize(np.full(d, 1.5))
            hs.append(h)
        gmx = egx.GaussianMixture([0.5, 0.5], [[0.3, 0.5, 0.5], [0.7, 0.5, 0.5]], [np.eye(3) * 0.05] * 2)
        mix = egx.GpMixture([egx.GaussianProcess(h, None) for h in hs], gmx, "smooth")
        xq = np.random.default_rng(1).random((20, d))
        kw = dict(criterion=egx.EI, fmin=float(np.quantile(_data(120, d, seed=151)[1], 0.1)))
        with egx.InfillObjective(mix, **kw) as obj:
            v0, g0 = obj.value_and_grad(xq)
            hs[1].finalize(np.full(d, 0.7))  # the SECOND expert: every expert's fit_epoch is watched
            v1, g1 = obj.value_and_grad(xq)
            with egx.InfillObjective(mix, **kw) as fresh:
                v2, g2 = fresh.value_and_grad(xq)
        np.testing.assert_array_equal(v1, v2)
        np.testing.assert_array_equal(g1, g2)
        assert not np.array_equal(v1, v0)
    finally:
        for h in hs:
            h.close()


# ---- 9: refusals --------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals(egx):
    x, y = _data(100, 3, seed=161)
    x2, y2 = _data(100, 2, seed=162)
    with egx.GpHandle(x, y) as h, egx.GpHandle(x, y + 1.0) as unfit, egx.GpHandle(x2, y2) as other:
        h.finalize(np.full(3, 1.5))
        other.finalize(np.full(2, 1.5))
        gp, gp_unfit, gp_other = (egx.GaussianProcess(v, None) for v in (h, unfit, other))

        def gmx():
            return egx.GaussianMixture([0.5, 0.5], [[0.3, 0.5, 0.5], [0.7, 0.5, 0.5]], [np.eye(3) * 0.05] * 2)

        with pytest.raises(egx.NotFittedError, match="surrogate 0 expert 1"):
            egx.InfillObjective(egx.GpMixture([gp, gp_unfit], gmx(), "smooth"))
        with pytest.raises(egx.NotFittedError, match="surrogate 1 expert 0"):
            egx.InfillObjective(egx.GpMixture([gp, gp], gmx(), "smooth"), [egx.GpMixture([gp_unfit, gp], gmx(), "hard")], [0.0])
        with pytest.raises(egx.InvalidValueError, match="surrogate 0 expert 1 has 2 inputs"):
            egx.InfillObjective(egx.GpMixture([gp, gp_other], gmx(), "smooth"))
        g = gmx()
        g.heaviside_factor = 0.0
        with pytest.raises(egx.InvalidValueError, match="heaviside"):
            egx.InfillObjective(egx.GpMixture([gp, gp], g, "smooth"))
        g.heaviside_factor = -1.0
        with pytest.raises(egx.InvalidValueError, match="heaviside"):
            egx.InfillObjective(egx.GpMixture([gp, gp], g, "smooth"))
        for field in ("weights", "means", "precisions_chol"):
            g = gmx()
            getattr(g, field).flat[1] = np.nan
            with pytest.raises(egx.InvalidValueError, match="non-finite"):
                egx.InfillObjective(egx.GpMixture([gp, gp], g, "smooth"))
        g = gmx()
        g.weights[0] = 0.0
        with pytest.raises(egx.InvalidValueError, match="positive"):
            egx.InfillObjective(egx.GpMixture([gp, gp], g, "smooth"))
        # (d, k) beyond the recombination's LDS: 3 (d | 1) + 2 (k | 1) > 320
        k = 160
        wide = egx.GaussianMixture(np.full(k, 1.0 / k), np.random.default_rng(0).random((k, 3)), [np.eye(3)] * k)
        with pytest.raises(egx.EgxError, match="LDS") as err:
            egx.InfillObjective(egx.GpMixture([gp] * k, wide, "smooth"))
        assert err.value.rc == egx._lib.ERR_UNSUPPORTED
        # the largest mixture egx_gmm_fit trains per dimension is accepted: k = 16
        k = 16
        ok = egx.GaussianMixture(np.full(k, 1.0 / k), np.random.default_rng(0).random((k, 3)), [np.eye(3)] * k)
        with egx.InfillObjective(egx.GpMixture([gp] * k, ok, "hard"), criterion=egx.EI, fmin=0.0) as obj:
            assert np.all(np.isfinite(obj.value(x[:5])))
        with pytest.raises(egx.InvalidValueError, match="ranks"):
            egx.InfillObjective(egx.GpMixture([gp, None], gmx(), "smooth", rank=0, world=2))
        with egx.InfillObjective(egx.GpMixture([gp, gp], gmx(), "smooth")) as obj:
            with pytest.raises(egx.InvalidValueError, match="out of range"):
                obj.expert_parts(1, x[:2])


# ---- 10: a plain C host -------------------------------------------------------------------------------------------------------
@gpu
def test_plain_c_host_drives_the_mixture_entry_points(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "infill_mix_driver"
    libdir = os.path.join(root, "egobox_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{os.path.join(root, 'include')}",
                    os.path.join(root, "tests", "c_host", "infill_mix_driver.c"), f"-L{libdir}", "-legx_gp_hip", "-lm",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert out.stdout.startswith("OK"), out.stdout


# ---- 11: an expert above 1024 rows ------------------------------------------------------------------------------------------
@gpu
def test_parts_with_an_expert_above_1024_rows(egx):
    d = 8
    hs = []
    try:
        for e, n in enumerate((1100, 700)):
            x, y = _data(n, d, seed=171 + e, yscale=1e-3)
            h = egx.GpHandle(x, y, mean=e, corr=[0, 3][e])
            h.finalize(np.full(d, 1.2 + 0.2 * e))
            hs.append(h)
        means = np.full((2, d), 0.5)
        means[:, 0] = [0.35, 0.65]
        gmx = egx.GaussianMixture([0.5, 0.5], means, [np.eye(d) * 0.08] * 2, 0.9)
        mix = egx.GpMixture([egx.GaussianProcess(h, None) for h in hs], gmx, "smooth")
        xq = _queries(_data(1100, d, seed=171)[0], 25, seed=5)
        p = gmx.predict_probas(xq)
        assert np.sum(p.max(axis=1) < 0.9) >= 10
        with egx.InfillObjective(mix, criterion=egx.EI, fmin=0.0) as obj:
            got = obj.parts(xq)
        val, var = mix.predict_valvar(xq)
        gy, gv = mix.predict_valvar_gradients(xq)
        _check_mix_parts(got, [(val, var, gy, gv)], [max(float(h.inner()["sigma2"]) for h in hs)])
    finally:
        for h in hs:
            h.close()
