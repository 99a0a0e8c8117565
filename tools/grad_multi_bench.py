#!/usr/bin/env python3
"""Times the theta-gradient and the L-BFGS fit of a group in lock-step against the loops that do the same work without them.

    python tools/grad_multi_bench.py [--sizes 1024,4096,8192] [--k 8] [--d 16] [--repeats 10] [--warmups 3]
                                     [--starts 2] [--max-iter 6] [--out profiles/grad_multi_bench.txt]

One process, k members of one shape (Matern-5/2, constant trend, d inputs).  Per size:

  grad   `likelihood_grad_multi` on the group             against  the loop of lone `likelihood_grad` calls on the SAME members
  fit    `fit_lbfgs_multi` on the group                   against  (a) the loop of `fit_lbfgs` on k one-workspace handles
                                                                   (b) the loop of `GpParams.optimizer("lbfgs").fit`, which
                                                                       creates a multi-workspace handle per model, as
                                                                       `cross_validate` did for L-BFGS folds before

Both loops run code that the parent commit has too.  The fits use the same `--starts` starts and `--max-iter` iterations per
start in all three forms ((b) through n_start / max_eval); (b) includes creating and closing its handles, because a caller of
`fit` pays for that, the other two run on handles created before the clock starts; its handles have `--starts` workspaces and
so a schedule of their own, which can move its trajectories by rounding (the evaluation counts are printed).  Every call ends in host results (the
library synchronises), so the host clock around it is the call's time.  The forms alternate inside the repeat loop; medians and
quartiles of `--repeats` timed calls after `--warmups` warm-up calls each.  The results of the forms are compared bit for bit
before anything is timed."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MATERN52 = 3


def time_alternating(calls, repeats, warmups):
    for f in calls.values():
        for _ in range(warmups):
            f()
    ts = {name: [] for name in calls}
    for _ in range(repeats):
        for name, f in calls.items():
            t0 = time.perf_counter()
            f()
            ts[name].append(time.perf_counter() - t0)
    return {name: np.percentile(v, [25, 50, 75]) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--starts", type=int, default=2)
    ap.add_argument("--max-iter", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 10 or a.warmups < 3:
        sys.exit("grad_multi_bench: at least 10 timed runs after 3 warm-ups")
    import torch
    if not torch.cuda.is_available():
        sys.exit("grad_multi_bench: no GPU -- nothing is measured without one")
    import egobox_amd as egx
    from egobox_amd import workload
    from egobox_amd.multistart import prepare_multistart

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    k, d = a.k, a.d
    say(f"# tools/grad_multi_bench.py: k = {k} members, d = {d}, Matern-5/2; medians [q1, q3] of {a.repeats} runs after {a.warmups} "
        f"warm-ups, forms alternating; fits: {a.starts} starts x {a.max_iter} iterations")
    say(f"# device: {torch.cuda.get_device_name(0)}")
    for n in [int(v) for v in a.sizes.split(",")]:
        sets = [workload.make_training_set(n, d, seed=700 + j) for j in range(k)]
        xs = np.stack([s[0] for s in sets])
        ys = np.stack([np.asarray(s[1]).reshape(-1) for s in sets])
        th = workload.default_theta(d)
        thetas = np.stack([th * (1.0 + 0.01 * j) for j in range(k)])
        # the starts GpParams.fit draws, so that all three fits walk the same trajectories
        params = egx.GaussianProcess.params(egx.ConstantMean(), egx.Matern52Corr()).optimizer("lbfgs") \
            .n_start(a.starts - 1).max_eval(4 * a.max_iter).theta_init(th)
        assert max(5, min(100, params._max_eval // 4)) == a.max_iter, "--max-iter must be what max_eval // 4 gives (>= 6)"
        bounds = params._theta_tuning.bounds * d
        starts = 10.0 ** prepare_multistart(a.starts - 1, th, bounds, seed=params._seed)[0]
        lo, hi = [b[0] for b in bounds], [b[1] for b in bounds]

        group = egx.GpHandle.create_group(xs, ys, corr=MATERN52)
        ones = [egx.GpHandle(xs[j], ys[j], corr=MATERN52, n_workspaces=1) for j in range(k)]

        # ---- equal results first
        lone = [h.likelihood_grad(thetas[j]) for j, h in enumerate(group)]
        lk, g, st = egx.likelihood_grad_multi(group, thetas)
        same = all(lk[j] == lone[j][0] and np.array_equal(g[j], lone[j][1]) and st[j] == lone[j][2] for j in range(k))
        say(f"n = {n}: likelihood_grad_multi == lone likelihood_grad, bit for bit: {same} (statuses {sorted(set(int(s) for s in st))})")

        res = time_alternating({
            "loop of lone likelihood_grad": lambda: [h.likelihood_grad(thetas[j]) for j, h in enumerate(group)],
            "likelihood_grad_multi": lambda: egx.likelihood_grad_multi(group, thetas),
        }, a.repeats, a.warmups)
        base = res["loop of lone likelihood_grad"][1]
        for name, (q1, q2, q3) in res.items():
            say(f"n = {n}  grad  {name:34s} {q2 * 1e3:10.2f} ms [{q1 * 1e3:.2f}, {q3 * 1e3:.2f}]  = {q2 / k * 1e3:8.2f} ms per member"
                f"  x{base / q2:.2f} vs the loop")

        def fit_multi():
            return egx.fit_lbfgs_multi(group, np.tile(starts, (k, 1, 1)), lo, hi, max_iter=a.max_iter)

        def fit_loop_one():
            return [h.fit_lbfgs(starts, lo, hi, max_iter=a.max_iter) for h in ones]

        def fit_loop_params():
            out = []
            for j in range(k):
                gp = params.fit(xs[j], ys[j])
                out.append((gp.n_evals, np.array(gp.theta())))
                gp.close()
            return out

        ne_m, ne_1, fp = fit_multi(), fit_loop_one(), fit_loop_params()
        same = all(ne_m[j] == ne_1[j] and np.array_equal(group[j].inner()["theta"], ones[j].inner()["theta"]) and
                   group[j].inner()["likelihood"] == ones[j].inner()["likelihood"] for j in range(k))
        same_p = all(np.array_equal(group[j].inner()["theta"], fp[j][1]) and ne_m[j] == fp[j][0] for j in range(k))
        say(f"n = {n}: fit_lbfgs_multi == fit_lbfgs on one workspace, bit for bit: {same}; == GpParams.fit's theta and evaluations: "
            f"{same_p}; evaluations per member {[int(v) for v in ne_m]} (in all: multi {int(np.sum(ne_m))}, (a) {int(np.sum(ne_1))}, "
            f"(b) {int(sum(v[0] for v in fp))})")
        res = time_alternating({"(a) loop of fit_lbfgs, one workspace": fit_loop_one,
                                "(b) loop of GpParams.fit (lbfgs)": fit_loop_params,
                                "fit_lbfgs_multi": fit_multi}, a.repeats, a.warmups)
        evals = float(np.sum(ne_m))
        for name, (q1, q2, q3) in res.items():
            say(f"n = {n}  fit   {name:38s} {q2:9.4f} s [{q1:.4f}, {q3:.4f}]  = {evals / q2:8.1f} evaluations/s"
                f"  x{res['(a) loop of fit_lbfgs, one workspace'][1] / q2:.2f} vs (a)  x{res['(b) loop of GpParams.fit (lbfgs)'][1] / q2:.2f} vs (b)")
        for h in group + ones:
            h.close()
        egx.trim()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
