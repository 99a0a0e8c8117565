"""k-fold cross-validation by refitting, with the folds of one shape fitted and asked in lock-step.

Every caller in egobox that multiplies fits is a cross-validation that refits per fold:
  GpMetrics (q2 / pva / iae_alpha, k-fold and leave-one-out)   crates/moe/src/metrics.rs:19-220 (twin: crates/gp/src/metrics.rs)
  find_best_expert through compute_error!                      crates/moe/src/algorithm.rs:209-347, expertise_macros.rs:14-51
The k training sets of a cross-validation have ONE shape, which is what a group of models factors in lock-step
(`GpParams.fit_group`: egx_gp_create_group + egx_gp_finalize_multi / egx_gp_fit_multi / egx_gp_fit_lbfgs_multi), and their validation predictions are
one launch sequence per run of members (`predict_valvar_multi`: egx_gp_predict_valvar_multi).  Each fold's fit and predictions
are bit for bit what `params.n_workspaces(1).fit(train)` + `predict_valvar(valid)` give (the latter on its batched route).

The fold layout (`fold_indices`) is linfa's, which the reference gets from `Dataset::fold` / `iter_fold`: fold_size = n // k,
validation chunk i = rows [i fold_size, (i + 1) fold_size), the n - k fold_size leftover rows in every training set.  linfa is
not vendored with the reference sources this project was written against: the rule is stated from linfa 0.8's documented
behaviour and could not be re-read.  A training set here keeps the original row order minus its validation chunk; linfa's
`iter_fold` swaps chunks in place, so its training rows may be a permutation of these -- which moves well-posed results at
rounding level only.

Not here: the folds of NbClusters::Auto (unequal cluster sizes, and a selection rule of its own), sparse-GP experts, KPLS and
ThetaTuning.Partial across models (those folds are a loop of lone fits).
"""
from __future__ import annotations

import math
from statistics import NormalDist

import numpy as np

from ._lib import ERR_INVALID_VALUE, InvalidValueError

# what GpParams.fit allows the correlation matrices of one fit: the members of a group alive at once stay below it
GROUP_BYTES = 16 << 30
GROUP_MAX = 256  # egx_gp_create_group's member bound
N_ALPHA = 20     # metrics.rs:87-88


def fold_indices(n, k):
    """[(train_rows, valid_rows)] * k of linfa's k-fold layout (module docstring): every training set has n - n // k rows."""
    n, k = int(n), int(k)
    if k < 1 or k > n:
        raise InvalidValueError(ERR_INVALID_VALUE, f"cross-validation: 1 <= k <= n expected (k {k}, n {n})")
    fs = n // k
    rows = np.arange(n)
    return [(np.concatenate([rows[:i * fs], rows[(i + 1) * fs:]]), rows[i * fs:(i + 1) * fs]) for i in range(k)]


class Fold:
    """One fold of a cross-validation: the fitted theta, the predictions (and variances, or None) at the validation rows."""

    __slots__ = ("theta", "pred", "var", "valid")

    def __init__(self, theta, pred, var, valid):
        self.theta, self.pred, self.var, self.valid = theta, pred, var, valid


def _group_batch(n_train, k):
    n_pad = -(-n_train // 128) * 128
    return max(1, min(k, GROUP_MAX, GROUP_BYTES // max(1, 8 * n_pad * (n_pad + 128))))


def cross_validate(params, x, y, k, want_var=False):
    """The k folds of (x, y) under `params` (a GpParams): a list of `Fold`.  The training sets go through `params.fit_group`
    in batches whose matrices stay below 16 GiB, the validation blocks through `predict_valvar_multi`, and a batch's members
    are closed as soon as their predictions are down (leave-one-out at n = 2000 never holds 2000 factors).  Where `fit_group`
    refuses (KPLS, ThetaTuning.Partial) the folds are a loop of `params.fit`.  `optimizer("lbfgs")` folds go in lock-step too
    (egx_gp_fit_lbfgs_multi: every round of the folds' L-BFGS machines is one likelihood + gradient evaluation of the group)."""
    from . import gp as G
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if x.ndim != 2 or y.shape[0] != x.shape[0]:
        raise InvalidValueError(ERR_INVALID_VALUE, f"x (n, nx) and y (n,) expected, got {x.shape} and {y.shape}")
    folds = fold_indices(x.shape[0], k)
    out = []
    if not params.fits_groups():
        for tr, va in folds:
            gp = params.fit(x[tr], y[tr])
            try:
                pred, var = gp.predict_valvar(x[va]) if want_var else (gp.predict(x[va]), None)
                out.append(Fold(np.array(gp.theta()), pred, var, va))
            finally:
                gp.close()
        return out
    batch = _group_batch(folds[0][0].size, len(folds))
    for b0 in range(0, len(folds), batch):
        part = folds[b0:b0 + batch]
        gps = params.fit_group(np.stack([x[tr] for tr, _ in part]), np.stack([y[tr] for tr, _ in part]))
        try:
            preds, vars_ = G.predict_valvar_multi(gps, np.stack([x[va] for _, va in part]), True, want_var)
            for j, (_, va) in enumerate(part):
                out.append(Fold(np.array(gps[j].theta()), preds[j].copy(), vars_[j].copy() if want_var else None, va))
        finally:
            for g in gps:
                g.close()
    return out


def cross_validate_surrogates(fit, x, y, k, want_var=False):
    """The same folds for any `fit(x_train, y_train) -> surrogate` (predict / predict_valvar; `theta` and `close` optional):
    one fit per fold, no lock-step claimed -- a mixture of several clusters, whose experts' shapes differ from fold to fold."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    out = []
    for tr, va in fold_indices(x.shape[0], k):
        model = fit(x[tr], y[tr])
        try:
            if want_var:
                pred, var = model.predict_valvar(x[va])
            else:
                pred, var = model.predict(x[va]), None
            theta = np.array(model.theta()) if hasattr(model, "theta") else None
            out.append(Fold(theta, np.asarray(pred, dtype=np.float64).reshape(-1),
                            None if var is None else np.asarray(var, dtype=np.float64).reshape(-1), va))
        finally:
            if hasattr(model, "close"):
                model.close()
    return out


# ---- the metrics of GpMetrics on the folds' predictions (crates/moe/src/metrics.rs:32-143) ----------------------------
def q2_from_folds(folds, y):
    """metrics.rs:32-50: 1 - PRESS / TSS over the validation rows, TSS around the mean of ALL targets."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    y_mean = y.mean()
    press = tss = 0.0
    for f in folds:
        yv = y[f.valid]
        press += float(np.sum((yv - f.pred) ** 2))
        tss += float(np.sum((yv - y_mean) ** 2))
    return 1.0 - press / tss


def pva_from_folds(folds, y):
    """metrics.rs:58-75: |ln(mean((y - pred)^2 / var))| over the validation rows."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    varss, n = 0.0, 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for f in folds:
            varss += float(np.sum((y[f.valid] - f.pred) ** 2 / f.var))
            n += f.valid.size
    return abs(math.log(varss / n)) if varss / n > 0.0 else (math.inf if varss == 0.0 else math.nan)


def iae_alpha(pred, var, y_valid, alphas):
    """metrics.rs:146-220 for one fold: (iae, deltas) -- deltas[j] the fraction of targets inside pred +- sigma ppf(1 - alpha_j / 2)."""
    sigma = np.sqrt(var)
    q = np.array([NormalDist().inv_cdf(1.0 - a / 2.0) for a in alphas])
    off = sigma[:, None] * q[None, :]
    inside = (y_valid[:, None] >= pred[:, None] - off) & (y_valid[:, None] <= pred[:, None] + off)
    deltas = inside.sum(axis=0) / float(y_valid.size)
    return float(np.sum(np.abs(deltas - (1.0 - alphas)))) / alphas.size, deltas


class IaeAlphaPlotData:
    """metrics.rs:9-16: what `iae_alpha_k_score(k, plot_data)` fills (a dict is filled the same way)."""

    def __init__(self):
        self.alphas, self.deltas = [], []


def iae_alpha_from_folds(folds, y, plot_data=None):
    """metrics.rs:83-138: the folds' mean IAE; `plot_data` receives the alphas and the folds' mean coverage."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    alphas = np.linspace(0.02, 0.98, N_ALPHA)
    score, deltas = 0.0, np.zeros(N_ALPHA)
    for f in folds:
        iae, dl = iae_alpha(f.pred, f.var, y[f.valid], alphas)
        score += iae
        deltas = deltas + dl
    score /= len(folds)
    deltas = deltas / float(len(folds))
    if plot_data is not None:
        if isinstance(plot_data, dict):
            plot_data["alphas"], plot_data["deltas"] = alphas.tolist(), deltas.tolist()
        else:
            plot_data.alphas, plot_data.deltas = alphas.tolist(), deltas.tolist()
    return score


class GpMetrics:
    """The reference's GpMetrics trait (metrics.rs:19-144) for anything that knows how to cross-validate itself:
    `_cv_folds(k, want_var)` returns the folds, `_cv_targets()` the training targets."""

    def q2_k_score(self, kfold):
        return q2_from_folds(self._cv_folds(kfold, False), self._cv_targets())

    def q2_score(self):
        return self.q2_k_score(self._cv_targets().size)

    def pva_k_score(self, kfold):
        return pva_from_folds(self._cv_folds(kfold, True), self._cv_targets())

    def pva_score(self):
        return self.pva_k_score(self._cv_targets().size)

    def iae_alpha_k_score(self, kfold, plot_data=None):
        return iae_alpha_from_folds(self._cv_folds(kfold, True), self._cv_targets(), plot_data)

    def iae_alpha_score(self, plot_data=None):
        return self.iae_alpha_k_score(self._cv_targets().size, plot_data)


# ---- expert selection (find_best_expert, crates/moe/src/algorithm.rs:209-347) ------------------------------------------
def expert_pairs(regression, correlation):
    """The allowed (mean class, correlation class) pairs of two flag sets in the reference's order (algorithm.rs:219-238,
    compute_errors!): Constant, Linear, Quadratic, each by SquaredExponential, AbsoluteExponential, Matern32, Matern52."""
    from . import gpx
    regression, correlation = gpx.RegressionSpec(int(regression)), gpx.CorrelationSpec(int(correlation))
    means = [cls for flag, cls in gpx._REGR.items() if regression & flag]
    corrs = [cls for flag, cls in gpx._CORR.items() if correlation & flag]
    if not means or not corrs:
        raise InvalidValueError(ERR_INVALID_VALUE, "expert_specs: at least one regression and one correlation flag expected")
    return [(m, c) for m in means for c in corrs]


def pair_name(mean_cls, corr_cls):
    from . import gpx
    return f"{gpx._SURROGATE_NAME[str(mean_cls())]}_{gpx._SURROGATE_NAME[str(corr_cls())]}"


def select_expert(pairs, x, y, kpls_dim=None, theta_tuning=None, device=-1, cross_validate_fn=None):
    """find_best_expert's choice among `pairs` on one cluster: (winning name, [(name, error), ..] in the pairs' order).  The
    error of a pair is the mean over n_fold = min(n, 5) folds of ||y_valid - prediction||_2 (compute_error!,
    expertise_macros.rs:14-51), with the pair's DEFAULT GpParams plus kpls_dim (:22) -- `theta_tuning` overrides the tuning of
    the fold fits as an extension.  One pair is the reference's shortcut (algorithm.rs:241-242): nothing is fitted, the table
    is empty.  The first minimum wins, as Rust's min_by; a NaN error compares equal (partial_cmp .. unwrap_or(Equal))."""
    from . import gp as G
    pairs = list(pairs)
    if len(pairs) == 1:
        return pair_name(*pairs[0]), []
    cross_validate_fn = cross_validate_fn or cross_validate
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, nx = x.shape
    n_fold = min(n, 5)
    table = []
    for mean_cls, corr_cls in pairs:
        mean = mean_cls()
        # The reference compares the FOLD COUNT (at most 5), not the number of points, with 4 nx / 3 nx: from nx = 2 on no
        # Linear or Quadratic pair is ever fitted.  Kept as it is there (expertise_macros.rs:25-30).
        if (mean.code == 2 and n_fold < 4 * nx) or (mean.code == 1 and n_fold < 3 * nx):
            table.append((pair_name(mean_cls, corr_cls), math.inf))
            continue
        params = G.GpParams(mean, corr_cls()).kpls_dim(kpls_dim).device(device)
        if theta_tuning is not None:
            params.theta_tuning(theta_tuning)
        errors = [math.sqrt(float(np.sum((y[f.valid] - f.pred) ** 2))) for f in cross_validate_fn(params, x, y, n_fold)]
        table.append((pair_name(mean_cls, corr_cls), sum(errors) / len(errors)))
    best = 0
    for i in range(1, len(table)):
        if table[best][1] > table[i][1]:
            best = i
    return table[best][0], table
