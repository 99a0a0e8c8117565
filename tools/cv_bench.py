#!/usr/bin/env python3
"""Times the cross-validation workloads of egobox_amd/cv.py against the only way to do the same work without it: a loop of
`GpParams.fit` + `predict_valvar` per fold.

    python tools/cv_bench.py [--root TREE] [--impls loop,lockstep] [--workloads cv,loo,select,predict] [--repeats 10]
                             [--out profiles/cv_lockstep_bench.jsonl] [--build NAME]

`--root TREE` imports egobox_amd from another built checkout (the parent commit: only `--impls loop` exists there), so that one
session measures both builds; the rows carry `--build NAME`.  Per workload the implementations alternate inside the repeat
loop; every call ends in host results (the library synchronises), so the host clock around it is the call's time.  One JSON
line per (workload, implementation): median and quartiles of `--repeats` timed calls after one warm-up call each.

Workloads: 5-fold tuned cross-validation at n = 500 / 2000 / 4000, d = 8; leave-one-out at n = 200; the twelve-pair
selection at n = 500, nx = 1; egx_gp_predict_valvar_multi against k lone predict_valvar calls, k = 12, n = 2048,
m = 1 / 64 / 4096."""
import argparse
import json
import os
import sys
import time

import numpy as np


def folds(n, k):
    fs = n // k
    rows = np.arange(n)
    return [(np.concatenate([rows[:i * fs], rows[(i + 1) * fs:]]), rows[i * fs:(i + 1) * fs]) for i in range(k)]


def loop_cv(params, x, y, k, want_var=True):
    out = []
    for tr, va in folds(x.shape[0], k):
        gp = params.fit(x[tr], y[tr])
        out.append(gp.predict_valvar(x[va]) if want_var else (gp.predict(x[va]), None))
        gp.close()
    return out


def quartiles(ts):
    q1, q2, q3 = np.percentile(ts, [25, 50, 75])
    return {"median_s": float(q2), "q1_s": float(q1), "q3_s": float(q3), "iqr_s": float(q3 - q1), "repeats": len(ts)}


def time_alternating(calls, repeats):
    """calls: {impl: thunk}; one warm-up each, then `repeats` rounds in which the implementations take turns."""
    for f in calls.values():
        f()
    ts = {name: [] for name in calls}
    for _ in range(repeats):
        for name, f in calls.items():
            t0 = time.perf_counter()
            f()
            ts[name].append(time.perf_counter() - t0)
    return {name: quartiles(v) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--impls", default="loop,lockstep")
    ap.add_argument("--workloads", default="cv,loo,select,predict")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--cv-sizes", default="500,2000,4000")
    ap.add_argument("--out", default=None)
    ap.add_argument("--build", default="this")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    if not torch.cuda.is_available():
        sys.exit("cv_bench: no GPU -- nothing is measured without one")
    import egobox_amd as egx
    from egobox_amd import workload
    impls, rows = a.impls.split(","), []

    def record(name, res, **extra):
        for impl, q in res.items():
            rows.append({"workload": name, "impl": impl, "build": a.build, **extra, **q})
            print(json.dumps(rows[-1]), flush=True)

    def data(n, d, seed):
        x, y = workload.make_training_set(n, d, seed=seed)
        return x, np.asarray(y).reshape(-1)

    wl = a.workloads.split(",")
    if "cv" in wl:
        for n in [int(v) for v in a.cv_sizes.split(",")]:
            x, y = data(n, 8, n)
            calls = {}
            if "loop" in impls:
                calls["loop"] = lambda: loop_cv(egx.GaussianProcess.params(), x, y, 5)
            if "lockstep" in impls:
                calls["lockstep"] = lambda: egx.cross_validate(egx.GaussianProcess.params(), x, y, 5, want_var=True)
            record(f"cv5_tuned_n{n}_d8", time_alternating(calls, a.repeats), n=n, d=8, k=5)
    if "loo" in wl:
        x, y = data(200, 8, 200)
        calls = {}
        if "loop" in impls:
            calls["loop"] = lambda: loop_cv(egx.GaussianProcess.params(), x, y, 200)
        if "lockstep" in impls:
            calls["lockstep"] = lambda: egx.cross_validate(egx.GaussianProcess.params(), x, y, 200, want_var=True)
        record("loo_tuned_n200_d8", time_alternating(calls, a.repeats), n=200, d=8, k=200)
    if "select" in wl:
        x = np.linspace(0.0, 1.0, 500).reshape(-1, 1)
        y = np.abs(x[:, 0] - 0.37) + x[:, 0] ** 2
        means = [egx.ConstantMean, egx.LinearMean, egx.QuadraticMean]
        corrs = [egx.SquaredExponentialCorr, egx.AbsoluteExponentialCorr, egx.Matern32Corr, egx.Matern52Corr]

        def select_loop():
            table = []
            for m in means:
                for c in corrs:
                    errs = [float(np.linalg.norm(y[va] - p)) for (p, _), (_, va) in
                            zip(loop_cv(egx.GaussianProcess.params(m(), c()), x, y, 5, want_var=False), folds(500, 5))]
                    table.append(sum(errs) / 5)
            return table
        calls = {}
        if "loop" in impls:
            calls["loop"] = select_loop
        if "lockstep" in impls:
            b = egx.GpMixture.params().expert_specs(egx.RegressionSpec.ALL, egx.CorrelationSpec.ALL)
            calls["lockstep"] = lambda: b.select_expert(x, y)
        record("select12_tuned_n500_nx1", time_alternating(calls, a.repeats), n=500, d=1, k=5)
    if "predict" in wl:
        k, n, d = 12, 2048, 8
        sets = [data(n, d, 900 + j) for j in range(k)]
        xs, ys = np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])
        hs = egx.GpHandle.create_group(xs, ys)
        egx.finalize_multi(hs, np.full((k, d), 1.0))
        for m in (1, 64, 4096):
            xq = np.random.default_rng(m).random((k, m, d))
            calls = {}
            if "loop" in impls:
                calls["loop"] = lambda: [h.predict_valvar(xq[j]) for j, h in enumerate(hs)]
            if "lockstep" in impls:
                calls["lockstep"] = lambda: egx.predict_valvar_multi(hs, xq)
            # (a lone few-query call builds its C^-T cache on the third call: two more warm-ups put it in steady state)
            for f in calls.values():
                f(), f()
            record(f"predict_k12_n2048_m{m}", time_alternating(calls, max(a.repeats, 30 if m < 4096 else a.repeats)), n=n, d=d, k=k, m=m)
        for h in hs:
            h.close()
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
