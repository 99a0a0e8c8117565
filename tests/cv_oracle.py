"""Restatement of the reference's cross-validation callers on the CPU oracle (oracle/gp_oracle.py), for the tests of
egobox_amd/cv.py: the fold layout of linfa's Dataset::fold, the GpMetrics formulas (crates/moe/src/metrics.rs:32-220) and
find_best_expert's error table (crates/moe/src/algorithm.rs:209-255, expertise_macros.rs:14-51).  Written from the
reference's text, independently of the product code: nothing here imports egobox_amd."""
import math
from statistics import NormalDist

import numpy as np

MEANS = ["Constant", "Linear", "Quadratic"]
CORRS = ["SquaredExponential", "AbsoluteExponential", "Matern32", "Matern52"]


def folds(n, k):
    """(train rows, validation rows) per fold: chunks of n // k consecutive rows, the leftover rows in every training set."""
    fs = n // k
    out = []
    for i in range(k):
        valid = list(range(i * fs, (i + 1) * fs))
        out.append((np.array([r for r in range(n) if r not in valid], dtype=np.int64), np.array(valid, dtype=np.int64)))
    return out


def q2(preds, valids, y):
    """metrics.rs:32-50."""
    y_mean = y.mean()
    press = tss = 0.0
    for pred, va in zip(preds, valids):
        press += float(np.sum((y[va] - pred) ** 2))
        tss += float(np.sum((y[va] - y_mean) ** 2))
    return 1.0 - press / tss


def pva(preds, variances, valids, y):
    """metrics.rs:58-75."""
    varss, n = 0.0, 0
    for pred, var, va in zip(preds, variances, valids):
        varss += float(np.sum((y[va] - pred) ** 2 / var))
        n += len(va)
    return abs(math.log(varss / n))


def iae_alpha(preds, variances, valids, y):
    """metrics.rs:83-138 with iae_alpha :146-220: (score, alphas, mean coverage per alpha)."""
    alphas = [0.02 + (0.98 - 0.02) * i / 19 for i in range(20)]
    scores, cover = [], np.zeros(20)
    for pred, var, va in zip(preds, variances, valids):
        deltas = np.zeros(20)
        for j, a in enumerate(alphas):
            q = NormalDist(0.0, 1.0).inv_cdf(1.0 - a / 2.0)
            count = 0
            for t, mu, v in zip(y[va], pred, var):
                off = math.sqrt(v) * q
                if mu - off <= t <= mu + off:
                    count += 1
            deltas[j] = count / len(va)
        scores.append(sum(abs(deltas[j] - (1.0 - alphas[j])) for j in range(20)) / 20)
        cover += deltas
    return sum(scores) / len(scores), alphas, cover / len(scores)


def oracle_folds(O, x, y, k, theta, mean="Constant", corr="SquaredExponential"):
    """Per fold the oracle's fit at fixed theta on the training rows: [(fit, train rows, validation rows)]."""
    return [(O.fit_fixed(x[tr], y[tr], theta, mean=mean, corr=corr), tr, va) for tr, va in folds(x.shape[0], k)]


def error_table(O, x, y, theta, means=MEANS, corrs=CORRS):
    """find_best_expert's [(name, error)] with oracle fits at fixed theta, the winner (first minimum), and per entry the mean over
    the folds of ||prediction||_2 (what the prediction bar of 1e-6 scales with)."""
    n, nx = x.shape
    n_fold = min(n, 5)
    table, scale = [], []
    for m in means:
        for c in corrs:
            name = f"{m}_{c}"
            if (m == "Quadratic" and n_fold < 4 * nx) or (m == "Linear" and n_fold < 3 * nx):
                table.append((name, math.inf))
                scale.append(0.0)
                continue
            errs, norms = [], []
            for fit, _, va in oracle_folds(O, x, y, n_fold, theta, mean=m, corr=c):
                pred = fit.predict(x[va])
                errs.append(math.sqrt(float(np.sum((y[va] - pred) ** 2))))
                norms.append(math.sqrt(float(np.sum(pred ** 2))))
            table.append((name, sum(errs) / len(errs)))
            scale.append(sum(norms) / len(norms))
    best = 0
    for i in range(1, len(table)):
        if table[best][1] > table[i][1]:
            best = i
    return table, table[best][0], scale
