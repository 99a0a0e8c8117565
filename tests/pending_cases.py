"""Helper of the pending-point tests (not a test): the recipe of a case, the checks the GPU files share, and the table of shapes
at which the fused conditioning (egobox_amd/csrc/kernels_pending.hip, infill_pending.hip pending_tile) branches.  Imports without the
library: the data comes from oracle.gp_oracle.lhs_classic / griewank, which draw the numbers of workload.make_training_set.

tests/test_pending_cases_cpu.py checks on the oracle alone that every row is well posed and that the rows named after an LDS
threshold straddle it; tests/test_gpu_infill_pending.py and tests/test_gpu_infill_pending_shapes.py run the library."""
import collections
import hashlib
import types

import numpy as np

import infill_oracle as IO
import pending_oracle as PO
from oracle import gp_oracle as GO
from test_gpu_infill import KINDS, MEANS, PRED_RTOL, _grad_tol  # noqa: F401 (re-exported)
from test_gpu_sample import oracle_from_handle

TOLS = [0.3, 0.1]
KEYS = ("value", "grad", "mean", "var", "grad_mean", "grad_var")

# ---- the launch arithmetic, restated -----------------------------------------------------------------------------------------
K_TILE = 128          # egx_internal.h: kTile
K_PENDING_QV = 4      # egx_internal.h:273  kPendingQV, columns of W^ per pass
K_PENDING_MAX_D = 64  # egx_internal.h:274  kPendingMaxD, the last fused shape
K_PC_THREADS = 128    # kernels_pending.hip:35  kPcThreads, one lane per query of the tile
K_LD = 16             # pending_math.h:26-27  kMaxPending = kLd
CROSS_OPT_IN = 65536  # kernels_pending.hip:243  above it launch_pending_cross takes hipFuncSetAttribute per instance
FINISH_OPT_IN = 60000  # kernels_pending.hip:290  ... and launch_pending_finish


def cross_lds_bytes(d, hcols=1):
    """kernels_pending.hip:234 (launch_pending_cross)  the lane's coordinates [d][kPcThreads], a slab of Z [d][64], the
    coefficients [d hcols] and the slab's weights [64][kPendingQV], in doubles"""
    return 8 * (d * K_PC_THREADS + d * 64 + d * hcols + 64 * K_PENDING_QV)


def finish_lds_bytes(d):
    """kernels_pending.hip:271 (launch_pending_finish)  d c_v / d x_k of a point, [kLd][d] doubles"""
    return 8 * K_LD * d


def column_passes(q):
    """kernels_pending.hip:259-260  (v0, columns) of the passes over the q columns of W^"""
    return [(v0, min(K_PENDING_QV, q - v0)) for v0 in range(0, q, K_PENDING_QV)]


def k0_passes(d):
    """kernels_pending.hip:249-252 (EGX_PC2), 58  the gradient instance's DK and its passes over the d inputs"""
    dk = 8 if d <= 8 else 16
    return dk, [min(dk, d - k0) for k0 in range(0, d, dk)]


# ---- the table ---------------------------------------------------------------------------------------------------------------
Row = collections.namedtuple("Row", "id n d q theta mean corr m kpls")


def _row(id, n, d, q, theta, mean, corr, m, kpls=0):
    return Row(id, n, d, q, theta, mean, corr, m, kpls)


# (n, d, q, theta per component, mean, corr, m).  Not reached: pending_splits with more than one slab per split, which needs
# n + q > 512 * 64, i.e. n > 32 704 -- no shape that takes a few seconds gets there.
ROWS = [
    _row("dk16-first", 130, 9, 6, 0.35, 0, 3, 40),        # first DK = 16 shape; column passes 4 + 2 (QV = 2 at v0 = 4)
    _row("dk16-full", 130, 16, 7, 0.25, 0, 0, 40),        # one full 16-wide k0 pass; column passes 4 + 3
    _row("two-pass", 130, 17, 4, 0.12, 0, 3, 40),         # a second k0 pass of one input; one full QV = 4 pass
    _row("two-pass-abs", 130, 17, 4, 0.12, 1, 1, 40),     # ... absolute exponential, linear trend
    _row("two-pass-m32", 130, 17, 4, 0.12, 0, 2, 40),     # ... Matern 3/2
    _row("two-pass-quad", 260, 17, 4, 0.12, 2, 3, 40),    # quadratic trend, p = 171: the finish's t_v and Jacobian loops
    _row("three-pass", 200, 33, 8, 0.09, 0, 3, 40),       # k0 = 0, 16, 32; two full column passes
    _row("lds-below", 130, 41, 2, 0.08, 0, 3, 12),        # 65 352 B: the last shape without the opt-in
    _row("lds-above", 130, 42, 2, 0.08, 0, 3, 12),        # 66 896 B: the first with it
    _row("fused-last", 130, 64, 3, 0.06, 0, 3, 12),       # kPendingMaxD, four full k0 passes
    _row("composed-first", 130, 65, 3, 0.06, 0, 3, 12),   # the composed form by the table, not by the knob
    _row("slab-exact", 127, 12, 1, 0.3, 0, 3, 40),        # nz = 128
    _row("slab-pending-only", 128, 12, 1, 0.3, 0, 3, 40),  # nz = 129: a slab of one pending point
    _row("slab-q16", 192, 12, 16, 0.3, 0, 3, 40),         # the identity rows of W^ start a slab; four full column passes
    _row("kpls-d12", 130, 12, 5, 0.3, 0, 3, 40, kpls=2),  # w_star (12, 2): hcols = 2 with DK = 16
    _row("finish-lds", 130, 469, 2, 0.02, 0, 0, 4),       # composed; the finish's dynamic LDS is 60 032 B > 60 000
]
BY_ID = {r.id: r for r in ROWS}
# rows that build the objective and ONE constraint model: the oracle's per-point Jacobians are what a case costs, 1 - 2.5 s per
# model at d >= 41 and at three-pass (d = 33 with 40 queries); every other row stays below a second per model
TWO_MODELS = {r.id for r in ROWS if r.d >= 41} | {"three-pass"}


def row_weights(r):
    """the KPLS weights of a row, or None"""
    return np.random.default_rng(2).standard_normal((r.d, r.kpls)) if r.kpls else None


# ---- the recipe --------------------------------------------------------------------------------------------------------------
def _ys(y):
    """the objective (scaled as in tests/test_gpu_infill.py) and two constraint outputs on the same rows"""
    return [1e-3 * y, y - np.quantile(y, 0.6), np.quantile(y, 0.7) - y]


def _draw(n, d, q, m, keep=None):
    """training set with seed 1, rng = default_rng(1000 n + 10 d + q), the q pending points first, then the m queries, uniform
    in the data's box; keep: the first `keep` inputs of all three, the outputs as they are"""
    x = GO.lhs_classic(n, d, 1)
    y = GO.griewank(x)
    rng = np.random.default_rng(1000 * n + 10 * d + q)
    lo, hi = x.min(axis=0), x.max(axis=0)
    xv = lo + (hi - lo) * rng.random((q, d))
    xq = lo + (hi - lo) * rng.random((m, d))
    if keep is not None:
        x, lo, hi, xv, xq = (np.ascontiguousarray(a[..., :keep]) for a in (x, lo, hi, xv, xq))
    return x, y, lo, hi, xv, xq, rng


def oracle_case(r, keep=None):
    """A row on the oracle alone: (the objective's model fitted at the row's theta, pending points, queries)"""
    x, y, _, _, xv, xq, _ = _draw(r.n, r.d, r.q, r.m, keep)
    d = x.shape[1]
    g = GO.fit_fixed(x, _ys(y)[0], np.full(r.kpls if r.kpls else d, r.theta), mean=MEANS[r.mean], corr=KINDS[r.corr],
                     w_star=row_weights(r))
    return g, xv, xq


def _case(egx, O, n, d, q, theta, mean, corr, m=40, w=None, models=3, keep=None):
    """`models` fitted models on the training set of seed 1 (n, d), their oracles, q pending points and m queries uniform in
    the data's box, virtual values = base mean + 3 sigma N(0, 1)"""
    x, y, lo, hi, xv, xq, rng = _draw(n, d, q, m, keep)
    d = x.shape[1]
    c = types.SimpleNamespace(x=x, ys=_ys(y)[:models], n=n, d=d, q=q, hs=[], gs=[], tols=TOLS[:models - 1])
    th = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    th = np.full(d if w is None else w.shape[1], th[0]) if th.size == 1 else th
    for yj in c.ys:
        h = egx.GpHandle(x, yj, mean=mean, corr=corr, w_star=w)
        h.finalize(th)
        c.hs.append(h)
        c.gs.append(oracle_from_handle(O, h, MEANS[mean], KINDS[corr], x, yj, w_star=w))
    c.lo, c.hi, c.xv, c.xq = lo, hi, xv, xq
    c.yv = np.empty((q, models))
    for j, g in enumerate(c.gs):
        mu, var = g.predict_valvar(c.xv)
        c.yv[:, j] = mu + 3.0 * np.sqrt(var) * rng.standard_normal(q)
    c.fmin = float(np.quantile(c.ys[0], 0.1))
    return c


def row_case(egx, O, r, m=None, models=None, keep=None):
    return _case(egx, O, r.n, r.d, r.q, r.theta, r.mean, r.corr, m=r.m if m is None else m, w=row_weights(r),
                 models=(2 if r.id in TWO_MODELS else 3) if models is None else models, keep=keep)


def _close(c):
    for h in c.hs:
        h.close()


def gate(g, xv, xq):
    """the condition on the cases, on the ORACLE: below it s^2 - c^T S^-1 c loses its digits in any double evaluation"""
    min_diag, min_unit = PO.cond_report(g, xv, xq)
    ok = min_diag >= 1e-2 and min_unit >= 1e-4
    return min_diag, min_unit, ok


def _assert_conditioned(c, xq):
    min_diag, min_unit, ok = gate(c.gs[0], c.xv, xq)  # (the models share x, theta, kernel and trend)
    print(f"n {c.n} d {c.d} q {c.q}: min diag S {min_diag:.3g}, min conditioned unit variance {min_unit:.3g}")
    assert ok


def _push_all(obj, c):
    for v in range(c.q):
        obj.push_pending(c.xv[v], c.yv[v])


def _objective(egx, c, criterion=None, **kw):
    """the infill handle of a case: model 0 the objective, the others its constraints"""
    return egx.InfillObjective(c.hs[0], c.hs[1:], c.tols, criterion=egx.EI if criterion is None else criterion, fmin=c.fmin, **kw)


# ---- the checks --------------------------------------------------------------------------------------------------------------
_REFITS = {}


def _refit_reference(g, xv, yv, xq):
    """(mean, var, grad_mean, grad_var, sigma2) of the frozen refit of g on (xv, yv) at xq, read-only.  Computed once per
    (fitted state, points, queries): the tests that come back to a case share it."""
    key = hashlib.sha1(b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in (
        g.xt_norm, g.yt_norm, g.theta, g.w_star, g.inner.beta, g.inner.gamma, g.inner.r_chol, xv, yv, xq))).digest()
    key = (key, g.mean, g.corr)
    if key not in _REFITS:
        ref = PO.refit_frozen(g, xv, yv)
        ry, rv = ref.predict_valvar(xq)
        gy, gv = ref.predict_valvar_gradients(xq)
        out = (np.ravel(ry), np.ravel(rv), gy, gv)
        for a in out:
            a.setflags(write=False)
        _REFITS[key] = out + (float(ref.inner.sigma2),)
    return _REFITS[key]


def _check_parts_against_refit(c, p, xq, sigma2):
    for j, g in enumerate(c.gs):
        ry, rv, gy, gv, ref_s2 = _refit_reference(g, c.xv, c.yv[:, j], xq)
        for name, got, want in (("mean", p["mean"][j], ry), ("var", p["var"][j] / ref_s2, rv / ref_s2),
                                ("grad_mean", p["grad_mean"][j] / np.abs(gy).max(), gy / np.abs(gy).max()),
                                ("grad_var", p["grad_var"][j] / np.abs(gv).max(), gv / np.abs(gv).max())):
            print(f"  model {j} {name}: worst abs error {np.max(np.abs(got - want)):.3e} (scale {np.max(np.abs(want)):.3e})")
        print(f"  model {j} sigma2: {sigma2[j]:.12e} refit {ref_s2:.12e}")
        np.testing.assert_allclose(p["mean"][j], ry, rtol=PRED_RTOL, atol=1e-9)
        np.testing.assert_allclose(p["var"][j], rv, rtol=PRED_RTOL, atol=1e-9 * ref_s2)
        np.testing.assert_allclose(p["grad_mean"][j], gy, **_grad_tol(gy))
        np.testing.assert_allclose(p["grad_var"][j], gv, **_grad_tol(gv))
        np.testing.assert_allclose(sigma2[j], ref_s2, rtol=1e-6)


def _assert_same_to_rounding(a, b, bar=1e-9):
    """the per-model keys of two `parts` within `bar` of each key's per-model scale"""
    nm = a["mean"].shape[0]
    for k in KEYS[2:]:
        scale = np.abs(b[k]).reshape(nm, -1).max(axis=1).reshape((nm,) + (1,) * (b[k].ndim - 1))
        worst = np.max(np.abs(a[k] - b[k]) / scale)
        print(f"  {k}: worst difference {worst:.3e} of the model's scale")
        assert worst <= bar, k


def _check_composed_form(egx, c, obj):
    """egx_set_tuning("pending_composed", 1) on a handle whose points are pushed: the same refit, the mean-only twin on the
    composed layouts, and the fused form's values to rounding.  Returns (fused, composed)."""
    nm = len(c.hs)
    fused = obj.parts(c.xq)
    assert egx.set_tuning("pending_composed", 1) == 0
    try:
        comp = obj.parts(c.xq)
        _check_parts_against_refit(c, comp, c.xq, obj.pending[2])
        obj.set_cstr_strategy("mean", [1.0] * (nm - 1))  # the mean-only twin on the composed layouts
        cs, gc = obj.constraints(c.xq, grad=True)[1::2]
        np.testing.assert_array_equal(cs, comp["mean"][1:].T)
        np.testing.assert_array_equal(gc, comp["grad_mean"][1:].transpose(1, 0, 2))
        obj.set_cstr_strategy("infill")
    finally:
        assert egx.set_tuning("pending_composed", 0) == 1
    _assert_same_to_rounding(comp, fused)
    return fused, comp


def _check_clear_pending(egx, c):
    """clear_pending gives back the fitted handle bit for bit (c.xq: more than one tile)"""
    kw = dict(criterion=egx.LOG_EI)
    with _objective(egx, c, **kw) as never, _objective(egx, c, **kw) as obj:
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


def _check_companions(egx, c, rows=(0, 57, 127, 128, 130)):
    """a conditioned point's bits do not depend on the points it is asked with (c.xq: 131 points, two tiles, the second ragged)"""
    nm = len(c.hs)
    with _objective(egx, c, criterion=egx.LOG_EI) as obj:
        _push_all(obj, c)
        big = obj.parts(c.xq)
        for i in rows:
            one = obj.parts(c.xq[i])
            for k in KEYS:
                np.testing.assert_array_equal(np.take(big[k], i, axis=0 if k in ("value", "grad") else 1),
                                              np.take(one[k], 0, axis=0 if k in ("value", "grad") else 1))
        # ... nor on the constraint strategy's mean-only sequence
        obj.set_cstr_strategy("mean", [1.0] * (nm - 1))
        v, cs, g, gc = obj.constraints(c.xq, grad=True)
        np.testing.assert_array_equal(cs, big["mean"][1:].T)
        np.testing.assert_array_equal(gc, big["grad_mean"][1:].transpose(1, 0, 2))
    return big


def _check_batch(egx, c, q, ns, optimizer, strategy):
    """optimize_batch is the loop a caller writes, bit for bit, and its f[i] the criterion of refits on the first i points"""
    lim = np.stack([c.lo, c.hi], axis=1)
    starts = c.lo + (c.hi - c.lo) * np.random.default_rng(17).random((q, ns, c.d))
    kw = dict(criterion=egx.LOG_EI)
    with _objective(egx, c, **kw) as a, _objective(egx, c, **kw) as b:
        x, yv, f, nf = a.optimize_batch(lim, starts, q, strategy=strategy, optimizer=optimizer)
        assert nf == q
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
            want = IO.objective(a.criterion, mean, var, c.tols, prm["fmin"], prm["sigma_weight"], prm["scale_ic"], prm["scale"],
                                prm["feasibility"], dev=True)
            print(f"{optimizer} {strategy} step {i}: f {f[i]:.12e} refit {want:.12e}")
            np.testing.assert_allclose(f[i], want, rtol=1e-6)
