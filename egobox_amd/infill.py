"""EGO's infill criterion on fitted models (include/egx_gp.h `egx_infill_*`; crates/ego/src/criteria, utils/cstr_pof.rs,
solver/solver_computations.rs:132-193, 297-475, solver/solver_infill_optim.rs:148-236): the objective the infill optimiser
minimises and its x-gradient for many points per call, the scaling pass and the lock-step COBYLA multistart."""
from __future__ import annotations

import ctypes as C
import enum

import numpy as np

from . import _lib as L

#: criterion constants (egx_infill_criterion)
EI, LOG_EI, WB2, WB2S = 0, 1, 2, 3
#: how the constraint surrogates enter the optimisation (egx_cstr_strategy)
CSTR_STRATEGIES = {"infill": 0, "mean": 1, "utb": 2}


class QEiStrategy(enum.IntEnum):
    """How the virtual observation of a q-point batch is chosen (egx_qei_strategy; crates/ego/src/types.rs:59-68)."""
    KB = 0      #: Kriging believer: the objective's mean
    KB_LB = 1   #: ... its lower bound, mean - 3 sigma
    KB_UB = 2   #: ... its upper bound, mean + 3 sigma
    CL_MIN = 3  #: constant liar: the training row with the smallest objective value


_QEI = {"kb": QEiStrategy.KB, "kb_lb": QEiStrategy.KB_LB, "kb_ub": QEiStrategy.KB_UB, "cl_min": QEiStrategy.CL_MIN}
BATCH_OPTIMIZERS = {"cobyla": 0, "slsqp": 1}


def _qei(strategy):
    if isinstance(strategy, str):
        if strategy.lower() not in _QEI:
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"infill: q-EI strategy must be one of {sorted(_QEI)}")
        return int(_QEI[strategy.lower()])
    return int(QEiStrategy(strategy))


def _gp_handle(model):
    """The `GpHandle` behind a GpHandle, a GaussianProcess or a single-expert Gpx -- or the `SgpHandle` behind an SgpHandle, a
    SparseGaussianProcess or a single-expert SparseGpx."""
    from .gp import GaussianProcess, GpHandle
    from .gpx import Gpx
    from .sgp import SgpHandle, SparseGaussianProcess, SparseGpx
    if isinstance(model, SparseGpx):
        model = model._sgp
    if isinstance(model, SparseGaussianProcess):
        model = model._h
    if isinstance(model, SgpHandle):
        return model
    if isinstance(model, Gpx):
        if len(model._experts) != 1:
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, "infill: mixtures with more than one cluster are not supported")
        model = model._experts[0]
    if isinstance(model, GaussianProcess):
        model = model.handle
    if not isinstance(model, GpHandle):
        raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"infill: expected a GpHandle, GaussianProcess, Gpx, SgpHandle, "
                                                       f"SparseGaussianProcess or SparseGpx, got {type(model).__name__}")
    return model


def _surrogate(model, j):
    """(expert handles, GaussianMixture or None, smooth) of surrogate j: a `GpMixture` of any number of clusters, or a single
    model (one expert, no mixture)."""
    from .moe import GaussianMixture, GpMixture
    from .sgp import SparseGpx
    if isinstance(model, SparseGpx) and model._moe is not None:  # a trained sparse mixture: its inner GpMixture
        model = model._moe
    if not isinstance(model, GpMixture):
        return [_gp_handle(model)], None, True
    name = f"infill: surrogate {j}"
    if model.world != 1:
        raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"{name}: a GpMixture spread over {model.world} ranks is not supported")
    if not isinstance(model.gmx, GaussianMixture):
        raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"{name}: gmx must be a GaussianMixture, got {type(model.gmx).__name__}")
    experts = []
    for e, expert in enumerate(model.experts):
        try:
            experts.append(_gp_handle(expert))
        except L.InvalidValueError:
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"{name} expert {e}: expected a library-backed GaussianProcess or "
                                                           f"GpHandle (or their sparse counterparts), got "
                                                           f"{type(expert).__name__}") from None
    return experts, model.gmx, model.recombination == "smooth"


class InfillObjective:
    """`egx_infill`: one objective model, k >= 0 constraint models (kept alive by this object), a criterion and its parameters.
    A model is a GpHandle, a GaussianProcess, a single-expert Gpx, their sparse counterparts (SgpHandle, SparseGaussianProcess,
    SparseGpx; a handle with a sparse model anywhere is built by egx_infill_create_any), a single-rank `egobox_amd.moe.GpMixture` of library-backed
    experts (any number of clusters, smooth or hard) or an `egobox_amd.mixint.MixintGpMixture`; models that carry xtypes
    (`GpHandle.set_xtypes`) must all carry the same ones, and every point is then cast on the device before it is evaluated: with a mixture among them the handle is built by egx_infill_create_mix
    and the recombination runs on the GPU; with single models only, by egx_infill_create as before.

    value / gradient are those of the MINIMISED objective: -crit / scale, times the probability of feasibility of the
    constraint models (EI, WB2, WB2S) or minus its logarithm (LOG_EI).

    tagged=True builds the handle by egx_infill_create_any even when no model is sparse (the same handle, the same bits)."""

    def __init__(self, obj_model, cstr_models=(), cstr_tols=(), criterion=LOG_EI, fmin=0.0, sigma_weight=1.0, feasibility=True,
                 scale_ic=1.0, scale=1.0, tagged=False):
        lib = L.load()
        self._lib = lib
        from .mixint import MixintGpMixture
        from .moe import GpMixture
        # a mixed-integer mixture: its inner mixture, whose experts carry the xtypes (the library casts the points it generates
        # and is given; the optimisers work in the unfolded continuous box, `to_discrete_space` folds x_best)
        obj_model = obj_model.moe if isinstance(obj_model, MixintGpMixture) else obj_model
        cstr_models = tuple(m.moe if isinstance(m, MixintGpMixture) else m for m in cstr_models)
        from .sgp import SgpHandle, SparseGpx
        mixed = any(isinstance(m, GpMixture) or (isinstance(m, SparseGpx) and m._moe is not None)
                    for m in (obj_model, *cstr_models))
        if mixed:
            self._surrogates = [_surrogate(m, j) for j, m in enumerate((obj_model, *cstr_models))]
            self._models = [e for experts, _, _ in self._surrogates for e in experts]
        else:
            self._models = [_gp_handle(obj_model)] + [_gp_handle(m) for m in cstr_models]
            self._surrogates = [([m], None, True) for m in self._models]
        self._owners = (obj_model, tuple(cstr_models))
        tols = L.as_f64(np.atleast_1d(np.asarray(cstr_tols, dtype=np.float64)) if len(cstr_models) else np.zeros(0), 1)
        k = len(self._surrogates) - 1
        if tols.shape[0] != k:
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"infill: {k} constraint models but {tols.shape[0]} tolerances")
        cfg = L.InfillConfig()
        lib.egx_infill_config_default(C.byref(cfg))
        cfg.criterion, cfg.feasibility = int(criterion), int(bool(feasibility))
        cfg.fmin, cfg.sigma_weight, cfg.scale_ic, cfg.scale = float(fmin), float(sigma_weight), float(scale_ic), float(scale)
        self._h = C.c_void_p()
        sparse = tagged or any(isinstance(m, SgpHandle) for m in self._models)
        if sparse:  # tagged references (egx_infill_create_any): dense and sparse experts side by side
            keep, structs = [], (L.InfillSurrogateAny * (k + 1))()
            for st, (experts, gmx, smooth) in zip(structs, self._surrogates):
                arr = (L.ModelRef * len(experts))(*[L.ModelRef(L.MODEL_SGP if isinstance(e, SgpHandle) else L.MODEL_GP,
                                                               e._h.value) for e in experts])
                st.experts, st.n_experts, st.smooth, st.heaviside_factor = arr, len(experts), int(smooth), 1.0
                keep.append(arr)
                if gmx is not None:
                    w, mu, pc = L.as_f64(gmx.weights), L.as_f64(gmx.means), L.as_f64(gmx.precisions_chol)
                    st.weights, st.means, st.precisions_chol = L.dptr(w), L.dptr(mu), L.dptr(pc)
                    st.heaviside_factor = float(gmx.heaviside_factor)
                    keep += [w, mu, pc]
            L.check(lib.egx_infill_create_any(C.byref(cfg), structs, L.dptr(tols) if k else None, k, C.byref(self._h)))
        elif mixed:
            keep, structs = [], (L.InfillSurrogate * (k + 1))()
            for st, (experts, gmx, smooth) in zip(structs, self._surrogates):
                arr = (C.c_void_p * len(experts))(*[e._h.value for e in experts])
                st.experts, st.n_experts, st.smooth, st.heaviside_factor = arr, len(experts), int(smooth), 1.0
                keep.append(arr)
                if gmx is not None:
                    w, mu, pc = L.as_f64(gmx.weights), L.as_f64(gmx.means), L.as_f64(gmx.precisions_chol)
                    st.weights, st.means, st.precisions_chol = L.dptr(w), L.dptr(mu), L.dptr(pc)
                    st.heaviside_factor = float(gmx.heaviside_factor)
                    keep += [w, mu, pc]
            L.check(lib.egx_infill_create_mix(C.byref(cfg), structs, L.dptr(tols) if k else None, k, C.byref(self._h)))
        else:
            arr = (C.c_void_p * max(k, 1))(*[m._h.value for m in self._models[1:]])
            L.check(lib.egx_infill_create(C.byref(cfg), self._models[0]._h, arr if k else None, L.dptr(tols) if k else None, k,
                                          C.byref(self._h)))
        self.d, self.n_cstr, self.criterion = self._models[0].d, k, int(criterion)
        self._active = None  # (indices, x_base) while active coordinates are set

    # ---- parameters ----------------------------------------------------------------------------------------------------
    @property
    def params(self):
        cfg = L.InfillConfig()
        L.check(self._lib.egx_infill_get_params(self._h, C.byref(cfg)))
        return dict(fmin=cfg.fmin, sigma_weight=cfg.sigma_weight, scale_ic=cfg.scale_ic, scale=cfg.scale,
                    feasibility=bool(cfg.feasibility))

    def set_params(self, fmin=None, sigma_weight=None, scale_ic=None, scale=None, feasibility=None):
        """Change parameters between EGO iterations (None keeps the current value)."""
        p = self.params
        new = dict(fmin=fmin, sigma_weight=sigma_weight, scale_ic=scale_ic, scale=scale, feasibility=feasibility)
        p.update({k: v for k, v in new.items() if v is not None})
        L.check(self._lib.egx_infill_set_params(self._h, float(p["fmin"]), float(p["sigma_weight"]), float(p["scale_ic"]),
                                                float(p["scale"]), int(bool(p["feasibility"]))))

    # ---- active coordinates (CoEGO) -------------------------------------------------------------------------------------
    def set_active(self, active, x_base):
        """Optimise over the columns `active` (distinct indices in [0, d), any order) with the others held at x_base (d,)
        (egx_infill_set_active): from now on `value`, `value_and_grad`, `parts`, `constraints` take (m, n_active) rows -- value j
        of a row stands for column active[j] -- and return n_active-wide gradients, the three `optimize*` take (n_active, 2)
        limits and (n_start, n_active) starts.  Values and the listed gradient columns are bit for bit the full-width ones.
        `scaling`, `expert_parts` and the pending-point calls stay d wide; `optimize_batch` is refused."""
        idx = np.ascontiguousarray(np.atleast_1d(np.asarray(active)))
        if idx.size == 0:  # (an empty list has no integer type of its own; the library refuses n_active = 0)
            idx = idx.astype(np.int32)
        if idx.ndim != 1 or not np.issubdtype(idx.dtype, np.integer):
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"infill: active must be a list of column indices, got {active!r}")
        if idx.size and (idx.min() < -2 ** 31 or idx.max() >= 2 ** 31):
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, "infill: active holds an index outside the int32 range")
        idx = idx.astype(np.int32)
        xb = L.as_f64(np.atleast_1d(np.asarray(x_base, dtype=np.float64)), 1)
        if xb.shape[0] != self.d:
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"infill: x_base must be ({self.d},), got {xb.shape}")
        L.check(self._lib.egx_infill_set_active(self._h, idx.ctypes.data_as(L.c_int32_p), idx.shape[0], L.dptr(xb)))
        self._active = (idx.astype(np.int64), xb.copy())

    def clear_active(self):
        """Back to full-width points: every call returns the bits it returned before `set_active`."""
        L.check(self._lib.egx_infill_clear_active(self._h))
        self._active = None

    @property
    def active(self):
        """None, or (indices (n_active,), x_base (d,)) as the handle holds them (egx_infill_get_active)."""
        n = C.c_int32()
        idx, xb = np.zeros(self.d, dtype=np.int32), np.zeros(self.d)
        L.check(self._lib.egx_infill_get_active(self._h, C.byref(n), idx.ctypes.data_as(L.c_int32_p), L.dptr(xb)))
        return None if n.value == 0 else (idx[:n.value].astype(np.int64), xb)

    @property
    def runs(self):
        """The lengths of the runs an evaluation walks (egx_infill_get_runs): consecutive surrogates of one shape that go through
        one launch sequence per tile.  They sum to 1 + n_cstr; the results never depend on them."""
        n = C.c_int32()
        lens = np.zeros(1 + self.n_cstr, dtype=np.int32)
        L.check(self._lib.egx_infill_get_runs(self._h, C.byref(n), lens.ctypes.data_as(L.c_int32_p)))
        return [int(v) for v in lens[:n.value]]

    @property
    def width(self):
        """Columns of a trial point, a limit, a gradient row: n_active while an activity is set, else d."""
        return self.d if self._active is None else int(self._active[0].shape[0])

    # ---- evaluation ----------------------------------------------------------------------------------------------------
    def _points(self, x, d=None):
        d = self.d if d is None else d
        x = L.as_f64(x)
        if x.ndim == 1:
            x = x.reshape(1, -1) if d > 1 or x.shape[0] == 1 else x.reshape(-1, 1)
        if x.ndim != 2 or x.shape[1] != d:
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"infill: points must be (m, {d}), got {x.shape}")
        return np.ascontiguousarray(x)

    def _limits(self, xlimits):
        lim = L.as_f64(xlimits, 2)
        if lim.shape != (self.width, 2):
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"infill: xlimits must be ({self.width}, 2), got {lim.shape}")
        return np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])

    def _eval(self, x, want_grad, want_parts):
        x = self._points(x, self.width)
        m, d, nm = x.shape[0], self.width, 1 + self.n_cstr
        value = np.empty(m)
        grad = np.empty((m, d)) if want_grad else None
        parts, pstruct = None, None
        if want_parts:
            parts = dict(mean=np.empty((nm, m)), var=np.empty((nm, m)), grad_mean=np.empty((nm, m, d)), grad_var=np.empty((nm, m, d)))
            pstruct = L.InfillParts(*[L.dptr(parts[k]) for k in ("mean", "var", "grad_mean", "grad_var")])
        L.check(self._lib.egx_infill_eval(self._h, L.dptr(x), m, L.dptr(value), L.dptr(grad) if want_grad else None,
                                          C.byref(pstruct) if want_parts else None))
        return value, grad, parts

    def value(self, x):
        """(m,) values of the minimised objective at x (m, d); no gradient work."""
        return self._eval(x, False, False)[0]

    def value_and_grad(self, x):
        """((m,), (m, d)): the minimised objective and its x-gradient; the values are bit for bit those of `value`."""
        v, g, _ = self._eval(x, True, False)
        return v, g

    def parts(self, x):
        """What the criterion is computed from, model-major (model 0 = objective): dict of mean (1 + k, m), var (1 + k, m),
        grad_mean (1 + k, m, d), grad_var (1 + k, m, d), plus value (m,) and grad (m, d)."""
        v, g, p = self._eval(x, True, True)
        p["value"], p["grad"] = v, g
        return p

    def expert_parts(self, j, x):
        """What surrogate j (0 = objective) was recombined FROM (egx_infill_eval_experts): dict of the expert-major mean (k, m),
        var (k, m), grad_mean (k, m, d), grad_var (k, m, d) of its k experts, the responsibilities probas (m, k) and their
        x-derivatives dprobas (m, k, d)."""
        if not 0 <= int(j) < len(self._surrogates):
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"infill: surrogate {j} out of range")
        x = self._points(x)
        m, d, k = x.shape[0], self.d, len(self._surrogates[int(j)][0])
        out = dict(mean=np.empty((k, m)), var=np.empty((k, m)), grad_mean=np.empty((k, m, d)), grad_var=np.empty((k, m, d)),
                   probas=np.empty((m, k)), dprobas=np.empty((m, k, d)))
        L.check(self._lib.egx_infill_eval_experts(self._h, int(j), L.dptr(x), m, *[L.dptr(out[key]) for key in (
            "mean", "var", "grad_mean", "grad_var", "probas", "dprobas")]))
        return out

    def scaling(self, points):
        """compute_scaling (solver_computations.rs:132-193) on `points` (npts, d): returns (scale_ic, scale, scale_cstr) and
        stores scale_ic and scale in the object."""
        x = self._points(points)
        sic, sc = C.c_double(), C.c_double()
        scs = np.empty(max(self.n_cstr, 1))
        L.check(self._lib.egx_infill_scaling(self._h, L.dptr(x), x.shape[0], C.byref(sic), C.byref(sc), L.dptr(scs)))
        return sic.value, sc.value, scs[:self.n_cstr].copy()

    def optimize(self, xlimits, x_start, max_eval=None):
        """The bound-constrained multistart (solver_infill_optim.rs:148-236): one COBYLA per row of x_start (n_start, d) inside
        xlimits (d, 2), all starts in lock-step.  Returns (f, x, stats); f = +inf when no start ended at a finite value."""
        lo, hi = self._limits(xlimits)
        xs = self._points(x_start, self.width)
        n_start = xs.shape[0]
        f, xb = C.c_double(), np.empty(self.width)
        evals = np.zeros(n_start, dtype=np.int64)
        st = L.InfillStats(0, 0, evals.ctypes.data_as(L.c_int64_p))
        rc = self._lib.egx_infill_optimize(self._h, L.dptr(lo), L.dptr(hi), L.dptr(xs), n_start,
                                           0 if max_eval is None else int(max_eval), C.byref(f), L.dptr(xb), C.byref(st))
        if rc != L.ERR_NO_FINITE_START:
            L.check(rc)
        stats = dict(evals=evals, rounds=int(st.rounds), best_start=int(st.best_start), finite=rc == L.SUCCESS)
        return f.value, xb, stats

    # ---- the constraint surrogates as constraints of the optimiser (cstr_infill = false) --------------------------------
    def set_cstr_strategy(self, strategy, scale_cstr=None):
        """"infill": the constraint surrogates are folded into the objective as (log) probabilities of feasibility (the
        default).  "mean" / "utb": the objective carries no factor and the surrogates are handed to the optimiser as
        c(x) <= 0, their scaled mean or upper trust bound (mean + 3 sigma) / scale_cstr (solver_infill_optim.rs:148-204).
        scale_cstr (n_cstr,) positive and finite, or None to keep the stored scales (ones at first; `scaling` stores its own)."""
        if strategy not in CSTR_STRATEGIES:
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"infill: cstr strategy must be one of {sorted(CSTR_STRATEGIES)}")
        sc = None
        if scale_cstr is not None:
            sc = L.as_f64(np.atleast_1d(np.asarray(scale_cstr, dtype=np.float64)), 1)
            if sc.shape[0] != self.n_cstr:
                raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"infill: {self.n_cstr} constraint models but {sc.shape[0]} scales")
        L.check(self._lib.egx_infill_set_cstr_strategy(self._h, CSTR_STRATEGIES[strategy],
                                                       L.dptr(sc) if sc is not None and self.n_cstr else None))

    def cstr_strategy(self):
        """(strategy name, scale_cstr (n_cstr,))."""
        s = C.c_int32()
        sc = np.ones(max(self.n_cstr, 1))
        L.check(self._lib.egx_infill_get_cstr_strategy(self._h, C.byref(s), L.dptr(sc)))
        return {v: k for k, v in CSTR_STRATEGIES.items()}[s.value], sc[:self.n_cstr].copy()

    def constraints(self, x, grad=False):
        """What the optimiser sees under "mean" / "utb" (egx_infill_eval_cstr): (value (m,), cstr (m, n_cstr)), with grad=True
        also (grad (m, d), grad_cstr (m, n_cstr, d)).  c <= 0 is feasible."""
        x = self._points(x, self.width)
        m, d, k = x.shape[0], self.width, self.n_cstr
        value, cstr = np.empty(m), np.empty((m, k))
        g = np.empty((m, d)) if grad else None
        gc = np.empty((m, k, d)) if grad else None
        spare = np.empty(1)  # a valid address for the empty tables of n_cstr = 0
        L.check(self._lib.egx_infill_eval_cstr(self._h, L.dptr(x), m, L.dptr(value), L.dptr(cstr if cstr.size else spare),
                                               L.dptr(g) if grad else None, L.dptr(gc if k and m else spare) if grad else None))
        return (value, cstr, g, gc) if grad else (value, cstr)

    def optimize_constrained(self, xlimits, x_start, max_eval=None):
        """The multistart with the constraint surrogates as nonlinear constraints (egx_infill_optimize_cstr): one
        general-constraint COBYLA per row of x_start inside xlimits (d, 2), all starts in lock-step.  Returns (x, f, c, stats):
        the best evaluated point -- feasible before infeasible, then the smaller objective, or the smaller violation --, the
        objective and the constraint values there, and a dict of evals, rounds, best_start, feasible, violation, finite."""
        lo, hi = self._limits(xlimits)
        xs = self._points(x_start, self.width)
        n_start = xs.shape[0]
        f, xb, cb = C.c_double(), np.empty(self.width), np.empty(max(self.n_cstr, 1))
        evals = np.zeros(n_start, dtype=np.int64)
        st = L.InfillCstrStats(0, 0, 0, 0.0, evals.ctypes.data_as(L.c_int64_p))
        rc = self._lib.egx_infill_optimize_cstr(self._h, L.dptr(lo), L.dptr(hi), L.dptr(xs), n_start,
                                                0 if max_eval is None else int(max_eval), C.byref(f), L.dptr(xb), L.dptr(cb),
                                                C.byref(st))
        if rc != L.ERR_NO_FINITE_START:
            L.check(rc)
        stats = dict(evals=evals, rounds=int(st.rounds), best_start=int(st.best_start), feasible=bool(st.feasible),
                     violation=float(st.violation), finite=rc == L.SUCCESS)
        return xb, f.value, cb[:self.n_cstr].copy(), stats

    def optimize_slsqp(self, xlimits, x_start, max_eval=None):
        """The multistart with the reference's default inner optimiser, SLSQP (egx_infill_optimize_slsqp): one machine per row
        of x_start inside xlimits (d, 2), all starts in lock-step, a round being one evaluation with gradients.  Works in every
        strategy: under "infill" (or without constraint models) a bound-constrained run and c is empty; under "mean" / "utb"
        subject to c_j <= cstr_tol_j / scale_cstr_j.  Returns (x, f, c, stats) as optimize_constrained, stats with `stop` beside:
        per start 1 budget, 2 converged, 3 line search could not move, 4 no finite value at the start, 5 inconsistent."""
        lo, hi = self._limits(xlimits)
        xs = self._points(x_start, self.width)
        n_start = xs.shape[0]
        k = 0 if self.cstr_strategy()[0] == "infill" else self.n_cstr
        f, xb, cb = C.c_double(), np.empty(self.width), np.empty(max(self.n_cstr, 1))
        evals = np.zeros(n_start, dtype=np.int64)
        stop = np.zeros(n_start, dtype=np.int32)
        st = L.InfillSlsqpStats(0, 0, 0, 0.0, evals.ctypes.data_as(L.c_int64_p), stop.ctypes.data_as(L.c_int32_p))
        rc = self._lib.egx_infill_optimize_slsqp(self._h, L.dptr(lo), L.dptr(hi), L.dptr(xs), n_start,
                                                 0 if max_eval is None else int(max_eval), C.byref(f), L.dptr(xb), L.dptr(cb),
                                                 C.byref(st))
        if rc != L.ERR_NO_FINITE_START:
            L.check(rc)
        stats = dict(evals=evals, stop=stop, rounds=int(st.rounds), best_start=int(st.best_start), feasible=bool(st.feasible),
                     violation=float(st.violation), finite=rc == L.SUCCESS)
        return xb, f.value, cb[:k].copy(), stats

    # ---- q points per iteration: pending (virtual) observations the models are conditioned on, no refit --------------------
    def push_pending(self, x, y):
        """Add the virtual observation (x (d,), y (1 + n_cstr,): objective, then the constraints) to the handle: from now on
        every evaluation runs on the models conditioned on it (egx_infill_push_pending).  At most 16; lone dense models only."""
        x = self._points(x)
        y = L.as_f64(np.atleast_1d(np.asarray(y, dtype=np.float64)), 1)
        if x.shape[0] != 1 or y.shape[0] != 1 + self.n_cstr:
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"infill: a pending point is x ({self.d},) and y ({1 + self.n_cstr},)")
        L.check(self._lib.egx_infill_push_pending(self._h, L.dptr(x), L.dptr(y)))

    def clear_pending(self):
        """Drop the pending points: the handle evaluates its fitted models again, bit for bit as before the first push."""
        L.check(self._lib.egx_infill_clear_pending(self._h))

    @property
    def pending(self):
        """(x (q, d) as stored -- cast --, y (q, 1 + n_cstr), sigma2 (1 + n_cstr,) the conditioned process variances)."""
        q = C.c_int32()
        nm = 1 + self.n_cstr
        x, y, s2 = np.zeros((16, self.d)), np.zeros((16, nm)), np.zeros(nm)
        L.check(self._lib.egx_infill_get_pending(self._h, C.byref(q), L.dptr(x), L.dptr(y), L.dptr(s2)))
        return x[:q.value].copy(), y[:q.value].copy(), s2

    def virtual_point(self, x, strategy="kb"):
        """compute_virtual_point (solver_computations.rs:261-292) at x on the handle's current (conditioned) models:
        (1 + n_cstr,) values, what `push_pending` takes."""
        x = self._points(x)
        y = np.empty(1 + self.n_cstr)
        L.check(self._lib.egx_infill_virtual_point(self._h, L.dptr(x), _qei(strategy), L.dptr(y)))
        return y

    def optimize_batch(self, xlimits, x_start, q, strategy="kb", optimizer="slsqp", scaling_points=None, max_eval=None):
        """The q loop of solver_impl.rs:622-791 in one call (egx_infill_optimize_batch): per step the multistart from
        x_start[i] ((q, n_start, d)), the virtual point at its optimum, the push.  Returns (x (n_found, d), y_virtual
        (n_found, 1 + n_cstr), f (n_found,), n_found); an error at step i is raised after nothing was found, else the steps
        before it are returned (their points stay pending)."""
        lim = L.as_f64(xlimits, 2)
        if lim.shape != (self.d, 2):
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"infill: xlimits must be ({self.d}, 2), got {lim.shape}")
        if optimizer not in BATCH_OPTIMIZERS:
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"infill: optimizer must be one of {sorted(BATCH_OPTIMIZERS)}")
        lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
        q = int(q)
        xs = L.as_f64(x_start, 3)
        if q < 1 or xs.shape[0] != q or xs.shape[2] != self.d:
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"infill: x_start must be ({q}, n_start, {self.d}), got {xs.shape}")
        cfg = L.InfillBatchConfig()
        self._lib.egx_infill_batch_config_default(C.byref(cfg))
        cfg.strategy, cfg.optimizer = _qei(strategy), BATCH_OPTIMIZERS[optimizer]
        cfg.max_eval = 0 if max_eval is None else int(max_eval)
        pts = None
        if scaling_points is not None:
            pts = self._points(scaling_points)
            cfg.scaling_points, cfg.n_scaling = L.dptr(pts), pts.shape[0]
        nm = 1 + self.n_cstr
        x, y, f, nf = np.zeros((q, self.d)), np.zeros((q, nm)), np.zeros(q), C.c_int32()
        rc = self._lib.egx_infill_optimize_batch(self._h, C.byref(cfg), L.dptr(lo), L.dptr(hi), L.dptr(xs), xs.shape[1], q,
                                                 L.dptr(x), L.dptr(y), L.dptr(f), C.byref(nf))
        if rc != L.SUCCESS and nf.value == 0:
            L.check(rc)
        n = nf.value
        return x[:n].copy(), y[:n].copy(), f[:n].copy(), n

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.egx_infill_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
