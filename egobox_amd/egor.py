"""Egor: the EGO loop over the GPU surrogates (crates/ego/src/solver/{egor_solver,solver_impl,solver_computations,
solver_infill_optim,egor_service,egor_config}.rs, crates/ego/src/utils/{find_result,misc,start_points,bounds}.rs;
python/src/egor.rs).  `Egor.suggest` is the ask-and-tell step, `Egor.minimize` the closed loop; both run ONE
`select_next_points`, which per point of the batch fits 1 + n_cstr surrogates (`GpMixtureParams`, or `MixintGpMixtureParams` in a
mixed-integer space), scales and sets up one `InfillObjective`, draws the start points and runs one lock-step multistart.

Everything here is host orchestration: every O(n^3) and O(n^2 m) step runs in the library's kernels through the entry points
named above.  The random stream is numpy's (`numpy.random.default_rng(seed)`), not the reference's Xoshiro256Plus: the same data
and seed give the same answer here, not the reference's points.

`Egor(coego_n_coop=k)` is CoEGO (solver/coego.rs): the coordinates are split into k random groups, theta is tuned and the
criterion optimised over one group at a time, through the active coordinates of the infill handle (`InfillObjective.set_active`).

Clustered surrogates (`GpConfig(n_clusters=k)`, k >= 2) train their mixture on the joined rows [x, y] through
`moe.train_mixture`: up to 36 columns on the narrow path, up to 128 on the wide one (`GaussianMixture.fit_wide`), so a clustered
`Egor` takes up to 127 input columns with hard recombination.  Smooth recombination's x-gradients and the infill handle on a
mixture still need 3 d + k <= 320 (d of about 100).  With ONE cluster and more than 35 columns no mixture is trained at all: the
closed form below (`_one_cluster`), as before.

Not here (a clean `InvalidValueError`, or no argument at all): TREGO, function constraints (`subject_to` / `fcstrs`), the
sigma-weight portfolio, hot start / `outdir` / warm start files, `NbClusters::Auto` and its reclustering rule, sparse surrogates, a
C++ mirror, and training objective and constraints as one lock-step group.
"""
from __future__ import annotations

import sys
import time
from typing import NamedTuple

import numpy as np

from . import mixint
from ._lib import ERR_INVALID_VALUE, InvalidValueError
from .doe import Lhs, parse_xspecs
from .gp import ThetaTuning
from .gpx import CorrelationSpec, Recombination, RegressionSpec
from .infill import EI, LOG_EI, WB2, WB2S, InfillObjective, QEiStrategy, _qei

DEFAULT_CSTR_TOL = 1e-4          # egor_solver.rs:143
MAX_POINT_ADDITION_RETRY = 3     # lib.rs; solver_impl.rs:505-511
INFILL_MAX_EVAL_DEFAULT = 2000   # optimizers/optimizer.rs:18
N_MAX_OPTIM = 3                  # solver_infill_optim.rs:70
EGO_DEFAULT_N_START = 20         # egor_config.rs:173
EGO_DEFAULT_MAX_ITERS = 20       # egor_config.rs:171
EGO_GP_OPTIM_N_START = 10        # egor_config.rs:13
EGO_GP_OPTIM_MAX_EVAL = 50       # egor_config.rs:15
DUPLICATE_L1 = 100.0 * np.finfo(np.float64).eps  # utils/misc.rs:49
GMM_MAX_DIM = 36                 # the widest row [x, y] of the narrow mixture training; ONE cluster beyond it: the closed form

_CRITERIA = {"ei": EI, "log_ei": LOG_EI, "logei": LOG_EI, "wb2": WB2, "wb2s": WB2S}
_OPTIMIZERS = ("slsqp", "cobyla")
_CSTR_NAMES = {"mean": "mean", "mc": "mean", "utb": "utb"}


def _invalid(msg):
    return InvalidValueError(ERR_INVALID_VALUE, "Egor: " + msg)


class OptimResult(NamedTuple):
    """x_opt (nx,), y_opt (1 + n_cstr,), x_doe (n, nx), y_doe (n, 1 + n_cstr) (python/src/types.rs OptimResult)."""
    x_opt: np.ndarray
    y_opt: np.ndarray
    x_doe: np.ndarray
    y_doe: np.ndarray


# ---- the host rules ----------------------------------------------------------------------------------------------------------
def _with_fcstrs(y_data, c_data):
    y = np.asarray(y_data, dtype=np.float64)
    y = y.reshape(-1, 1) if y.ndim == 1 else y
    if c_data is None:
        return y
    c = np.asarray(c_data, dtype=np.float64).reshape(y.shape[0], -1)
    return np.hstack([y, c])


def _cstr_sum(row, cstr_tol):
    """Sum of what the constraints exceed their tolerances by; row = [obj, cstr_1, ..] (find_result.rs:10-16)."""
    c = np.asarray(row, dtype=np.float64)[1:]
    tol = np.asarray(cstr_tol, dtype=np.float64)[:c.shape[0]]
    over = c > tol
    return float(np.abs(c[over] - tol[over]).sum())


def is_feasible(y, c, cstr_tol):
    """Whether no constraint of the row y = [obj, cstr_1, ..] (and of the function constraints' values c, or None) exceeds its
    tolerance (find_result.rs:146-158)."""
    row = np.atleast_1d(np.asarray(y, dtype=np.float64))
    if c is not None:
        row = np.concatenate([row, np.atleast_1d(np.asarray(c, dtype=np.float64))])
    return row.shape[0] <= 1 or _cstr_sum(row, cstr_tol) == 0.0


def find_best_result_index(y_data, c_data, cstr_tol):
    """The row of the smallest objective among the rows that violate no constraint; when none is feasible, the row of the
    smallest violation sum; without constraints the smallest objective (find_result.rs:77-142).  The first among equals.
    c_data: the function constraints' values (n, n_fcstr) or None."""
    data = _with_fcstrs(y_data, c_data)
    if data.shape[1] == 1:
        return int(np.argmin(data[:, 0]))
    csum = np.array([_cstr_sum(r, cstr_tol) for r in data])
    if np.isnan(csum).any():  # (no order on the sums: the smallest objective among the rows inside every tolerance)
        tol = np.asarray(cstr_tol, dtype=np.float64)[:data.shape[1] - 1]
        order = np.argsort(data[:, 0], kind="stable")
        for i in order:
            if np.all(data[i, 1:] < tol):
                return int(i)
        return int(order[0])
    imin = int(np.argmin(csum))
    if csum[imin] > 0.0:
        return imin
    feas = np.flatnonzero(csum == 0.0)
    return int(feas[np.argmin(data[feas, 0])])


def _cstr_less(y1, y2, cstr_tol):
    """cstr_min(y1, y2) == Less (find_result.rs:20-41)."""
    if y1.shape[0] > 1:
        s1, s2 = _cstr_sum(y1, cstr_tol), _cstr_sum(y2, cstr_tol)
        if s1 > 0.0 and s2 > 0.0:
            return s1 < s2
        if s1 == 0.0 and s2 == 0.0:
            return bool(y1[0] < y2[0])
        return s1 == 0.0
    return bool(y1[0] < y2[0])


def find_best_result_index_from(current_index, offset_index, y_data, c_data, cstr_tol):
    """The best row among `current_index` and the rows from `offset_index` on; the current one stays unless a new row is
    strictly better (find_result.rs:48-69)."""
    data = _with_fcstrs(y_data, c_data)
    best, best_row = int(current_index), data[int(current_index)]
    for i in range(int(offset_index), data.shape[0]):
        if _cstr_less(data[i], best_row, cstr_tol):
            best, best_row = i, data[i]
    return best


def is_update_ok(x_data, x_new):
    """False when x_new lies within 100 eps of a row of x_data in L1 distance (utils/misc.rs:44-54)."""
    x_data = np.asarray(x_data, dtype=np.float64)
    if x_data.shape[0] == 0:
        return True
    return not bool((np.abs(x_data - np.asarray(x_new, dtype=np.float64)).sum(axis=1) < DUPLICATE_L1).any())


def update_data(x_data, y_data, c_data, x_new, y_new, c_new):
    """Append the rows of x_new (with y_new, c_new) that pass `is_update_ok` against everything appended so far
    (utils/misc.rs:59-83).  Returns (x_data, y_data, c_data, indices of the appended rows of x_new); c_data / c_new may be None."""
    x_data, y_data = np.asarray(x_data, dtype=np.float64), np.asarray(y_data, dtype=np.float64)
    x_new, y_new = np.atleast_2d(np.asarray(x_new, dtype=np.float64)), np.atleast_2d(np.asarray(y_new, dtype=np.float64))
    appended = []
    for i in range(x_new.shape[0]):
        if is_update_ok(x_data, x_new[i]):
            x_data = np.vstack([x_data, x_new[i:i + 1]])
            y_data = np.vstack([y_data, y_new[i:i + 1]])
            if c_data is not None:
                c_data = np.vstack([np.asarray(c_data, dtype=np.float64), np.atleast_2d(np.asarray(c_new, dtype=np.float64))[i:i + 1]])
            appended.append(i)
    return x_data, y_data, c_data, appended


def start_points(x, xl, xu, n_max=None):
    """Midpoints of pairs of training points, closest pairs first, kept when no training point and no midpoint already kept
    lies closer to them than the pair's own points, in the metric scaled by xu - xl; at most n_max (utils/start_points.rs:7-91).
    Returns (n_found, d), possibly empty."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    rng_ = np.asarray(xu, dtype=np.float64) - np.asarray(xl, dtype=np.float64)
    xs = x / rng_
    iu, ju = np.tril_indices(n, -1)  # (i, j < i), row-major: the reference's order among equal distances
    dist = np.sqrt(((xs[iu] - xs[ju]) ** 2).sum(-1))
    out = []
    for p in np.argsort(dist, kind="stable"):
        i, j = int(iu[p]), int(ju[p])
        mid = (x[i] + x[j]) / 2.0
        ms = mid / rng_
        d_ij = np.sqrt(((xs[i] - ms) ** 2).sum())
        others = np.ones(n, dtype=bool)
        others[[i, j]] = False
        good = not (np.sqrt(((xs[others] - ms) ** 2).sum(-1)) < d_ij).any()
        if good and out:
            good = not (np.sqrt(((np.asarray(out) / rng_ - ms) ** 2).sum(-1)) < d_ij).any()
        if good:
            out.append(mid)
        if n_max is not None and len(out) >= n_max:
            break
    return np.asarray(out).reshape(-1, d)


_INFLUENCE = {CorrelationSpec.SQUARED_EXPONENTIAL: (0.29, 1.96), CorrelationSpec.ABSOLUTE_EXPONENTIAL: (0.15, 3.76),
              CorrelationSpec.MATERN32: (0.21, 2.74)}  # (Matern-5/2 does not enter, as in utils/bounds.rs:39-62)


def theta_bounds(bounds, dim, corr_spec):
    """The theta bounds of the loop's fits (utils/bounds.rs:5-85): the configured ones, except that the default (1e-2, 1e1)
    becomes a pair that depends on the dimension and the kernels from dim = 10 on."""
    default = tuple(ThetaTuning.DEFAULT_BOUNDS)
    if bounds is not None:
        bounds = [tuple(map(float, b)) for b in bounds]
        if len(bounds) != 1 or bounds[0] != default:
            return bounds
    if dim < 10:
        return [default]
    inf, sup = default
    for flag, (a, b) in _INFLUENCE.items():
        if int(corr_spec) & int(flag):
            inf, sup = min(inf, a), max(sup, b)
    s, k = 1.0 / np.sqrt(12.0), 9.0 / 5.0
    interval = 1.96 * np.sqrt(2.0 * (k + 1.0) * dim)
    lmin, lmax = s * np.sqrt(2.0 * dim - interval) * inf, s * np.sqrt(2.0 * dim + interval) * sup
    return [(float(1.0 / lmax), float(1.0 / lmin))]


# ---- CoEGO: cooperative groups of coordinates (solver/coego.rs) ---------------------------------------------------------------
def random_activity(nx, n_coop, rng):
    """get_random_activity (coego.rs:55-84): a (g_nb, g_size) integer array holding a shuffled 0 .. nx - 1, one row per group,
    g_nb = min(n_coop, nx).  When g_nb does not divide nx the rows are one longer than nx // g_nb and the last column of the
    rows from nx % g_nb on holds the marker nx, which `strip` removes."""
    nx = int(nx)
    g_nb = min(int(n_coop), nx)
    if g_nb < 1:
        raise _invalid(f"random_activity: n_coop >= 1 and nx >= 1 expected, got {n_coop} and {nx}")
    idx = rng.permutation(nx).astype(np.int64)
    remainder = nx % g_nb
    if remainder == 0:
        return idx.reshape(g_nb, nx // g_nb)
    g_size = nx // g_nb + 1
    cut = g_nb * (g_size - 1)
    out = np.full((g_nb, g_size), nx, dtype=np.int64)
    out[:, :g_size - 1] = idx[:cut].reshape(g_nb, g_size - 1)
    out[:remainder, g_size - 1] = idx[cut:]
    return out


def strip(active, dim):
    """The indices of an activity row below dim, in order: without the marker of an incomplete row (coego.rs:134-136)."""
    return [int(i) for i in active if int(i) < int(dim)]


# ---- configuration -----------------------------------------------------------------------------------------------------------
class GpConfig:
    """The surrogates' configuration (egor_config.rs:19-53, python/src/gp_config.rs): constant trend, squared exponential kernel,
    one cluster, smooth recombination with heaviside factor 1, theta from 0.1 in (1e-2, 1e1), 10 starts of at most 50 likelihood
    evaluations.  regr_spec / corr_spec with several flags ask for the cross-validated expert selection of `GpMixtureParams`."""

    def __init__(self, regr_spec=RegressionSpec.CONSTANT, corr_spec=CorrelationSpec.SQUARED_EXPONENTIAL, kpls_dim=None,
                 n_clusters=1, recombination=Recombination.SMOOTH, theta_init=None, theta_bounds=None,
                 n_start=EGO_GP_OPTIM_N_START, max_eval=EGO_GP_OPTIM_MAX_EVAL):
        self.regr_spec, self.corr_spec = RegressionSpec(int(regr_spec)), CorrelationSpec(int(corr_spec))
        self.kpls_dim, self.n_clusters = kpls_dim, n_clusters
        self.recombination = str(getattr(recombination, "name", recombination)).lower()
        self.theta_init = None if theta_init is None else np.atleast_1d(np.asarray(theta_init, dtype=np.float64))
        self.theta_bounds = None if theta_bounds is None else [tuple(map(float, b)) for b in np.atleast_2d(theta_bounds)]
        self.n_start, self.max_eval = int(n_start), int(max_eval)

    def check(self):
        if isinstance(self.n_clusters, bool) or not isinstance(self.n_clusters, (int, np.integer)) or self.n_clusters < 1:
            raise _invalid(f"gp_config.n_clusters must be a number >= 1 (0 and below ask for NbClusters::Auto, which is not "
                           f"implemented), got {self.n_clusters!r}")
        if self.recombination not in ("hard", "smooth"):
            raise _invalid(f"gp_config.recombination must be 'hard' or 'smooth', got {self.recombination!r}")
        if int(self.regr_spec) == 0 or int(self.corr_spec) == 0:
            raise _invalid("gp_config.regr_spec and corr_spec need at least one flag")
        if self.kpls_dim is not None and int(self.kpls_dim) < 1:
            raise _invalid(f"gp_config.kpls_dim must be at least 1, got {self.kpls_dim}")
        if self.n_start < 0 or self.max_eval < 1:
            raise _invalid("gp_config.n_start >= 0 and max_eval >= 1 expected")
        return self


def _one_cluster(xt):
    """The one-cluster mixture of the rows xt in closed form: their mean and covariance (what EM converges to for one cluster, with
    its 1e-6 on the diagonal).  The responsibilities of one cluster are ones and nothing reads more of it."""
    from .moe import GaussianMixture
    cov = np.atleast_2d(np.cov(xt.T, bias=True)) + 1e-6 * np.eye(xt.shape[1])
    return GaussianMixture([1.0], xt.mean(axis=0, keepdims=True), cov[None, :, :])


def _close_model(model):
    """Give a surrogate's device handles back (a `GpMixture` or a `MixintGpMixture`; closing twice is harmless)."""
    for e in getattr(model, "moe", model).experts:
        if e is not None:
            e.close()


def _experts(model):
    return getattr(model, "moe", model).experts


class Egor:
    """The optimiser (python/src/egor.rs:157-231).  xspecs: an (nx, 2) array of bounds or a list of `XType`.  The defaults are
    those of the reference's `EgorConfig` (egor_config.rs:232-259): LogEI, SLSQP, the constraint surrogates as mean constraints of
    the inner optimiser, 20 starts, one point per iteration, Kriging believer, target f64::MIN.  (The reference's Python
    constructor names COBYLA as its default optimiser; the configuration's own default is followed here.)"""

    def __init__(self, xspecs, gp_config=None, n_cstr=0, cstr_tol=None, n_start=EGO_DEFAULT_N_START, n_doe=0, doe=None,
                 infill_strategy=LOG_EI, cstr_infill=False, cstr_strategy="mean", q_points=1, q_infill_strategy=QEiStrategy.KB,
                 q_optmod=1, infill_optimizer="slsqp", target=-sys.float_info.max, seed=None,
                 trego=False, coego_n_coop=0, outdir=None, warm_start=False, hot_start=None):
        for name, on in (("trego", trego), ("outdir", outdir is not None),
                         ("warm_start", warm_start), ("hot_start", hot_start is not None)):
            if on:
                raise _invalid(f"{name} is not implemented")
        self.xtypes, self.xlimits = parse_xspecs(xspecs)  # xtypes None: a continuous space; xlimits of the relaxed space
        self.nx = self.xlimits.shape[0] if self.xtypes is None else len(self.xtypes)
        self.gp_config = (gp_config if gp_config is not None else GpConfig())
        if not isinstance(self.gp_config, GpConfig):
            raise _invalid(f"gp_config must be a GpConfig, got {type(gp_config).__name__}")
        self.gp_config.check()
        # CoEGO: 0 is off; the groups split the columns of the (unfolded) continuous space, as the reference's xlimits.nrows().
        # The reference clamps n_coop with min(n_coop, nx) (coego.rs:57); a larger value is refused here.
        if isinstance(coego_n_coop, bool) or not isinstance(coego_n_coop, (int, np.integer)) or coego_n_coop < 0:
            raise _invalid(f"coego_n_coop must be a number >= 0, got {coego_n_coop!r}")
        self.coego_n_coop = int(coego_n_coop)
        if self.coego_n_coop > self.xlimits.shape[0]:
            raise _invalid(f"coego_n_coop ({self.coego_n_coop}) exceeds the {self.xlimits.shape[0]} columns of the design space")
        if self.coego_n_coop and self.gp_config.kpls_dim is not None:
            raise _invalid("coego_n_coop and gp_config.kpls_dim exclude each other (egor_config.rs:458-462)")
        if self.coego_n_coop and int(self.gp_config.n_clusters) != 1:
            raise _invalid("coego_n_coop needs gp_config.n_clusters = 1: theta is updated group by group in the mono-cluster case "
                           "only (solver_impl.rs:251-291)")
        self.n_cstr = int(n_cstr)
        if self.n_cstr < 0:
            raise _invalid(f"n_cstr must not be negative, got {n_cstr}")
        if cstr_tol is None:
            self.cstr_tol = np.full(self.n_cstr, DEFAULT_CSTR_TOL)
        else:
            self.cstr_tol = np.atleast_1d(np.asarray(cstr_tol, dtype=np.float64))
            if self.cstr_tol.ndim != 1 or self.cstr_tol.shape[0] != self.n_cstr:
                raise _invalid(f"cstr_tol length ({self.cstr_tol.size}) does not match n_cstr ({self.n_cstr})")
        self.n_start, self.n_doe = int(n_start), int(n_doe)
        if self.n_start < 1 or self.n_doe < 0:
            raise _invalid("n_start >= 1 and n_doe >= 0 expected")
        self.doe = None
        if doe is not None:
            self.doe = np.asarray(doe, dtype=np.float64)
            if self.doe.ndim != 2 or self.doe.shape[1] not in (self.nx, self.nx + 1 + self.n_cstr) or self.doe.shape[0] < 1:
                raise _invalid(f"doe must be (ns, {self.nx}) inputs or (ns, {self.nx + 1 + self.n_cstr}) inputs and outputs, "
                               f"got shape {self.doe.shape}")
        if isinstance(infill_strategy, str):
            if infill_strategy.lower() not in _CRITERIA:
                raise _invalid(f"infill_strategy must be one of EI, LOG_EI, WB2, WB2S, got {infill_strategy!r}")
            infill_strategy = _CRITERIA[infill_strategy.lower()]
        if infill_strategy not in (EI, LOG_EI, WB2, WB2S):
            raise _invalid(f"infill_strategy must be one of EI, LOG_EI, WB2, WB2S, got {infill_strategy!r}")
        self.infill_strategy = int(infill_strategy)
        self.cstr_infill = bool(cstr_infill)
        if str(cstr_strategy).lower() not in _CSTR_NAMES:
            raise _invalid(f"cstr_strategy must be 'mean' or 'utb', got {cstr_strategy!r}")
        self.cstr_strategy = _CSTR_NAMES[str(cstr_strategy).lower()]
        self.q_points, self.q_optmod = int(q_points), int(q_optmod)
        if self.q_points < 1 or self.q_optmod < 1:
            raise _invalid(f"q_points >= 1 and q_optmod >= 1 expected, got {q_points} and {q_optmod}")
        self.q_infill_strategy = QEiStrategy(_qei(q_infill_strategy))
        self.infill_optimizer = str(getattr(infill_optimizer, "name", infill_optimizer)).lower()
        if self.infill_optimizer not in _OPTIMIZERS:
            raise _invalid(f"infill_optimizer must be one of {_OPTIMIZERS}, got {infill_optimizer!r}")
        self.target = float(target)
        self.seed = seed
        #: seconds the last `select_next_points` spent in its four parts (fit, scaling, starts: start points + host rules,
        #: optimize: the multistart), and scaling_lhs: the part of `scaling` that drew its Maximin LHS on the host
        self.last_timings_ = {}
        #: how many proposed rows the last `minimize` rejected as duplicates, and how many iterations it ran
        self.n_rejected_ = 0
        self.n_iter_ = 0
        #: CoEGO: the last infill step's cooperation, one (active columns, xcoop after the group's optimisation) per group
        self.last_coego_ = []

    # ---- spaces --------------------------------------------------------------------------------------------------------------
    def _unfold(self, x):
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(-1, 1) if self.nx == 1 else x.reshape(1, -1)
        if x.ndim != 2 or x.shape[1] != self.nx:
            raise _invalid(f"x must be (n, {self.nx}), got shape {x.shape}")
        return x.copy() if self.xtypes is None else mixint.to_continuous_space(self.xtypes, x)

    def _fold(self, x):
        return np.array(x, dtype=np.float64) if self.xtypes is None else mixint.to_discrete_space(self.xtypes, x)

    def _cast(self, x):
        return np.array(x, dtype=np.float64) if self.xtypes is None else mixint.cast_to_discrete_values(self.xtypes, x)

    def _y(self, y, n):
        y = np.asarray(y, dtype=np.float64)
        if y.ndim == 1:
            y = y.reshape(-1, 1)
        if y.shape != (n, 1 + self.n_cstr):
            raise _invalid(f"outputs must be ({n}, {1 + self.n_cstr}): the objective, then n_cstr constraints; got shape {y.shape}")
        return y

    def _eval(self, fun, x):
        """eval_obj (solver_computations.rs:478-492): `fun` sees the folded, cast points."""
        x = self._fold(x)
        return self._y(fun(x), x.shape[0])

    # ---- surrogates ----------------------------------------------------------------------------------------------------------
    def _make_surrogate(self, xt, yt, make_clustering, optimize_theta, clustering, theta_inits, actives=None):
        """make_clustered_surrogate (solver_impl.rs:121-295): (model, its experts' thetas (k, dim)).  With CoEGO's `actives`
        (solver_impl.rs:162-295, COEGO_IMPROVEMENT_CHECK = false) a tuned theta is tuned group by group: one fit per group with
        ThetaTuning.Partial on the group's components, each from the thetas of the fit before, the last model kept.  A step
        that reuses theta (Fixed) fits ONCE: the reference refits identically per group."""
        from .moe import GpMixtureParams
        cfg = self.gp_config
        dim = int(cfg.kpls_dim) if cfg.kpls_dim is not None else xt.shape[1]
        if theta_inits is None:
            init = cfg.theta_init if cfg.theta_init is not None else np.array([ThetaTuning.DEFAULT_INIT])
            if init.size not in (1, dim):
                raise _invalid(f"gp_config.theta_init must hold 1 or {dim} values, got {init.size}")
            theta_inits = np.tile(np.broadcast_to(init, (dim,)), (int(cfg.n_clusters), 1))
        bounds = theta_bounds(cfg.theta_bounds, dim, cfg.corr_spec)
        # one cluster on rows wider than the mixture's training takes (high dimension is CoEGO's ground): the closed form
        fit_gmx = make_clustering
        if make_clustering and int(cfg.n_clusters) == 1 and xt.shape[1] + 1 > GMM_MAX_DIM:
            clustering, fit_gmx = _one_cluster(xt), False
        params = GpMixtureParams().n_clusters(int(cfg.n_clusters)) \
            .recombination(cfg.recombination, 1.0 if cfg.recombination == "smooth" else None) \
            .expert_specs(cfg.regr_spec, cfg.corr_spec).kpls_dim(cfg.kpls_dim).n_start(cfg.n_start).max_eval(cfg.max_eval)
        if make_clustering or optimize_theta:  # (ThetaTuning::Partial with every component active is Full)
            tunings = [ThetaTuning.Full(t, bounds) for t in theta_inits]
        else:
            tunings = [ThetaTuning.Fixed(t) for t in theta_inits]
        if actives is not None and (make_clustering or optimize_theta):
            model = None
            for active in actives:
                params.theta_tunings([ThetaTuning.Partial(t, bounds, strip(active, dim)) for t in theta_inits])
                if not (fit_gmx and model is None):
                    params.gmx(clustering)  # (one cluster: the first group's mixture serves the groups after it)
                builder = params if self.xtypes is None else mixint.MixintGpMixtureParams(self.xtypes, params)
                new = builder.fit(xt, yt)
                if model is not None:
                    _close_model(model)
                model = new
                clustering = getattr(model, "moe", model).gmx
                theta_inits = np.stack([np.asarray(e.theta(), dtype=np.float64) for e in _experts(model)])
            return model, theta_inits
        params.theta_tunings(tunings)
        if not fit_gmx:
            params.gmx(clustering)
        builder = params if self.xtypes is None else mixint.MixintGpMixtureParams(self.xtypes, params)
        model = builder.fit(xt, yt)
        return model, np.stack([np.asarray(e.theta(), dtype=np.float64) for e in _experts(model)])

    # ---- one EGO step --------------------------------------------------------------------------------------------------------
    def _multistart(self, x_data, rng, active=None):
        """MiddlePickerMultiStarter (solver_computations.rs:53-114): midpoints of a random tenth of the training rows (at least
        two), completed from a Maximin LHS of at least three rows.  `active` (CoEGO): training rows and limits restricted to
        those columns (:65-66, 86)."""
        nt = x_data.shape[0]
        pick = rng.permutation(nt)[:max(nt // 10, 2)]
        xt, lim = (x_data[pick], self.xlimits) if active is None else (x_data[pick][:, active], self.xlimits[active])
        mid = start_points(xt, lim[:, 0], lim[:, 1], self.n_start)
        missing = self.n_start - mid.shape[0]
        if missing <= 0:
            return mid
        extra = Lhs(lim, "maximin", rng).sample(max(missing, 3))[:missing]
        return np.vstack([mid, extra])

    def _optimize(self, obj, x_start, xlimits=None):
        """One multistart with the configured optimiser: (f, x, finite)."""
        xlimits = self.xlimits if xlimits is None else xlimits
        max_eval = min(10 * x_start.size, INFILL_MAX_EVAL_DEFAULT)  # solver_infill_optim.rs:224
        if self.infill_optimizer == "slsqp":
            x, f, _c, st = obj.optimize_slsqp(xlimits, x_start, max_eval)
        elif self.cstr_infill or self.n_cstr == 0:
            f, x, st = obj.optimize(xlimits, x_start, max_eval)
        else:
            x, f, _c, st = obj.optimize_constrained(xlimits, x_start, max_eval)
        return f, x, bool(st["finite"]) and bool(np.isfinite(f))

    def _coego_optimize(self, obj, x_data, best_index, actives, ms_rng):
        """The cooperative infill step (solver_infill_optim.rs:67-271, COEGO_IMPROVEMENT_CHECK = false): from xcoop = the current
        best row, group by group: the criterion over the group's columns with the others at xcoop, up to N_MAX_OPTIM multistarts,
        the optimum written into xcoop.  Returns ((f of the last group that succeeded, xcoop) or None, seconds optimising)."""
        d = self.xlimits.shape[0]
        xcoop = x_data[best_index].copy()
        found, t_opt = None, 0.0
        self.last_coego_ = []
        try:
            for row in actives:
                active = strip(row, d)
                obj.set_active(active, xcoop)
                for _attempt in range(N_MAX_OPTIM):
                    x_start = self._multistart(x_data, ms_rng, active)
                    to = time.perf_counter()
                    f, x, ok = self._optimize(obj, x_start, self.xlimits[active])
                    t_opt += time.perf_counter() - to
                    if ok:
                        xcoop[active] = x
                        found = (f, xcoop)
                        break
                self.last_coego_.append((np.asarray(active, dtype=np.int64), xcoop.copy()))
        finally:
            obj.clear_active()
        return (None if found is None else (found[0], xcoop.copy())), t_opt

    def _virtual_point(self, xk, y_data, models):
        """compute_virtual_point (solver_computations.rs:261-292), from the models' own predictions."""
        if self.q_infill_strategy == QEiStrategy.CL_MIN:
            return y_data[int(np.argmin(y_data[:, 0]))].copy()
        x = xk.reshape(1, -1)
        conf = {QEiStrategy.KB: 0.0, QEiStrategy.KB_LB: -3.0, QEiStrategy.KB_UB: 3.0}[self.q_infill_strategy]
        pred = float(models[0].predict(x)[0])
        if conf != 0.0:
            pred += conf * float(np.sqrt(models[0].predict_var(x)[0]))
        return np.array([pred] + [float(m.predict(x)[0]) for m in models[1:]])

    def select_next_points(self, init, iteration, clusterings, theta_inits, x_data, y_data, best_index, rng, actives=None):
        """select_next_points (solver_impl.rs:562-800) without the portfolio: q_points rows of the continuous space with their
        virtual outputs, and the criterion's value at the last of them.  `clusterings` / `theta_inits` (lists of 1 + n_cstr,
        None at first) are updated in place: the mixtures of the first fit are reused, every expert's theta starts the next
        fit.  `actives`: CoEGO's activity (`random_activity`), or None.  Returns (x_dat (q, d), y_dat (q, 1 + n_cstr),
        infill_value)."""
        d = self.xlimits.shape[0]
        x_dat, y_dat = np.zeros((0, d)), np.zeros((0, 1 + self.n_cstr))
        infill_value = float("inf")
        t = dict(fit=0.0, scaling=0.0, scaling_lhs=0.0, starts=0.0, optimize=0.0)
        models = []
        try:
            for i in range(self.q_points):
                t0 = time.perf_counter()
                xt, yt = np.vstack([x_data, x_dat]), np.vstack([y_data, y_dat])
                make_clustering = bool(init) and i == 0
                optimize_theta = (int(iteration) * self.q_points + i) % self.q_optmod == 0
                new = []
                try:
                    for k in range(1 + self.n_cstr):  # one after the other
                        model, thetas = self._make_surrogate(xt, yt[:, k], make_clustering, optimize_theta, clusterings[k],
                                                             theta_inits[k], actives)
                        new.append(model)
                        clusterings[k], theta_inits[k] = getattr(model, "moe", model).gmx, thetas
                finally:
                    for m in models:  # the models of the step before
                        _close_model(m)
                    models = new
                t1 = time.perf_counter()
                fmin = float(y_data[best_index, 0])
                pts = Lhs(self.xlimits, "maximin", np.random.default_rng(int(rng.integers(2 ** 63)))).sample(min(100 * d, 1000))
                t_lhs = time.perf_counter() - t1
                with InfillObjective(models[0], models[1:], self.cstr_tol, criterion=self.infill_strategy, fmin=fmin) as obj:
                    # (the scaling pass reads the strategy -- under "mean" / "utb" the scale is that of the criterion without the
                    #  feasibility factor, compute_infill_obj_scale with cstr_infill = false -- so the strategy is set first; the
                    #  pass stores scale_ic, scale and, under "mean" / "utb", scale_cstr in the handle)
                    obj.set_cstr_strategy("infill" if self.cstr_infill or self.n_cstr == 0 else self.cstr_strategy)
                    obj.scaling(pts)
                    t2 = time.perf_counter()
                    ms_rng = np.random.default_rng(int(rng.integers(2 ** 63)))
                    found, t_opt = None, 0.0
                    if actives is not None:  # CoEGO: group by group, each with its own attempts
                        found, t_opt = self._coego_optimize(obj, x_data, best_index, actives, ms_rng)
                    for _attempt in range(0 if actives is not None else N_MAX_OPTIM):
                        x_start = self._multistart(x_data, ms_rng)
                        to = time.perf_counter()
                        f, x, ok = self._optimize(obj, x_start)
                        t_opt += time.perf_counter() - to
                        if ok:
                            found = (f, x)
                            break
                    if found is None:  # the current best point (solver_infill_optim.rs:64)
                        found = (fmin, x_data[best_index].copy())
                xk = self._cast(found[1].reshape(1, -1))[0]
                yk = self._virtual_point(xk, y_data, models)
                x_dat, y_dat = np.vstack([x_dat, xk]), np.vstack([y_dat, yk])
                infill_value = -found[0]
                t3 = time.perf_counter()
                t["fit"] += t1 - t0
                t["scaling"] += t2 - t1
                t["scaling_lhs"] += t_lhs
                t["optimize"] += t_opt
                t["starts"] += (t3 - t2) - t_opt
        finally:
            for m in models:
                _close_model(m)
        self.last_timings_ = t
        return x_dat, y_dat, infill_value

    # ---- the public calls ----------------------------------------------------------------------------------------------------
    def suggest(self, x_doe, y_doe):
        """The next q_points rows to evaluate, given the evaluated rows x_doe (n, nx) and y_doe (n, 1 + n_cstr)
        (solver_impl.rs:56-101, egor_service.rs:121-130): one `select_next_points` from a generator seeded afresh with `seed`,
        so that the same data and seed give the same rows."""
        x_data = self._cast(self._unfold(x_doe))
        y_data = self._y(y_doe, x_data.shape[0])
        rng = np.random.default_rng(self.seed)
        best_index = find_best_result_index(y_data, None, self.cstr_tol)
        nm = 1 + self.n_cstr
        actives = random_activity(self.xlimits.shape[0], self.coego_n_coop, rng) if self.coego_n_coop else None
        x_dat, _, _ = self.select_next_points(True, 0, [None] * nm, [None] * nm, x_data, y_data, best_index, rng, actives)
        return self._fold(x_dat)

    def get_result_index(self, x_doe=None, y_doe=None):
        """The index of the best row of y_doe (python/src/egor.rs:379-386); x_doe is not read and may be left out."""
        if y_doe is None:
            x_doe, y_doe = None, x_doe
        y = np.asarray(y_doe, dtype=np.float64)
        return find_best_result_index(self._y(y, y.shape[0]), None, self.cstr_tol)

    def get_result(self, x_doe, y_doe):
        """`OptimResult` of evaluated rows (python/src/egor.rs:401-424)."""
        x = np.asarray(x_doe, dtype=np.float64)
        x = x.reshape(-1, 1) if x.ndim == 1 else x
        y = self._y(y_doe, x.shape[0])
        i = find_best_result_index(y, None, self.cstr_tol)
        return OptimResult(x[i].copy(), y[i].copy(), x.copy(), y.copy())

    def minimize(self, fun, max_iters=EGO_DEFAULT_MAX_ITERS, fcstrs=()):
        """Minimise `fun` ((p, nx) -> (p, 1 + n_cstr): the objective, then constraints that are satisfied when negative) within
        `max_iters` iterations of q_points evaluations each (egor_solver.rs:170-349, ego_step solver_impl.rs:398-555).  Stops
        early when the best objective value is at or below `target`, or when three selections in a row proposed nothing but
        points already evaluated."""
        if fcstrs is not None and len(fcstrs):
            raise _invalid("function constraints (fcstrs / subject_to) are not implemented")
        rng = np.random.default_rng(self.seed)
        if self.doe is not None:
            x_data = self._cast(self._unfold(self.doe[:, :self.nx]))
            y_data = self._eval(fun, x_data) if self.doe.shape[1] == self.nx else self._y(self.doe[:, self.nx:], x_data.shape[0])
        else:
            n_doe = self.n_doe if self.n_doe > 0 else max(self.xlimits.shape[0] + 1, 5)
            x_data = self._cast(Lhs(self.xlimits, "optimized", rng).sample(n_doe))
            y_data = self._eval(fun, x_data)
        nm = 1 + self.n_cstr
        clusterings, theta_inits = [None] * nm, [None] * nm
        best_index = find_best_result_index(y_data, None, self.cstr_tol)
        retries = MAX_POINT_ADDITION_RETRY
        self.n_rejected_, self.n_iter_ = 0, 0
        # CoEGO: an activity drawn before the first iteration and again after every iteration (egor_solver.rs:251-256, 372-378)
        actives = random_activity(self.xlimits.shape[0], self.coego_n_coop, rng) if self.coego_n_coop else None
        for it in range(int(max_iters)):
            if y_data[best_index, 0] <= self.target:
                break
            converged = False
            while True:
                x_dat, y_dat, _ = self.select_next_points(it == 0, it, clusterings, theta_inits, x_data, y_data, best_index, rng,
                                                          actives)
                n_before = x_data.shape[0]
                x_data, y_data, _, added = update_data(x_data, y_data, None, x_dat, y_dat, None)
                self.n_rejected_ += x_dat.shape[0] - len(added)
                if added:
                    break
                retries -= 1
                if retries == 0:
                    converged = True  # NoMorePointToAddError: the solver is taken to have converged
                    break
            if converged:
                break
            retries = MAX_POINT_ADDITION_RETRY
            y_data[n_before:] = self._eval(fun, x_data[n_before:])
            best_index = find_best_result_index_from(best_index, n_before, y_data, None, self.cstr_tol)
            self.n_iter_ = it + 1
            if self.coego_n_coop:
                actives = random_activity(self.xlimits.shape[0], self.coego_n_coop, rng)
        return OptimResult(self._fold(x_data[best_index:best_index + 1])[0], y_data[best_index].copy(), self._fold(x_data), y_data)
