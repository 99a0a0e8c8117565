"""Where one EGO iteration spends its time: ONE `Egor.suggest` call (egobox_amd/egor.py) at n = 500 and n = 4096 training rows,
d = 8, an objective and two constraint surrogates, every setting at its default (LogEI, SLSQP from 20 starts, the constraints as
mean constraints, one cluster, theta tuned from 10 + 1 starts of at most 50 likelihood evaluations).

The call is split into the four parts `Egor.select_next_points` times itself (`Egor.last_timings_`):

    fit       the 1 + n_cstr surrogate fits, one after the other (GpMixtureParams.fit: clustering, theta tuning, the final factor)
    scaling   the 800-point Maximin LHS, the InfillObjective handle, egx_infill_scaling
    scaling_lhs   of that, the draw of the LHS on the host (multistart.lhs_maximin: the best of five by pairwise distances)
    starts    the start points (middle picker + LHS) and the host rules: the cast, the virtual point's predictions
    optimize  the lock-step multistart (egx_infill_optimize_slsqp), all attempts
    total     the wall time of the call (the parts and what lies between them: unfolding, the best row)

One process, 3 warm-up calls per size, medians with quartiles of 9.  No threshold is set: the table is the result.

    python tools/egor_bench.py [--out profiles/egor_bench.txt] [--reps 9] [--warmup 3] [--sizes 500 4096]

--coego records CoEGO beside the plain loop: one `suggest` at d = 64, n = 500 with coego_n_coop = 4 (theta tuned and the criterion
optimised over four groups of 16 columns, one after the other) and the same call with coego_n_coop = 0, the two alternated.
A record, no threshold.

    python tools/egor_bench.py --coego [--out profiles/egor_coego_bench.txt] [--reps 5] [--warmup 1]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import egobox_amd as egx  # noqa: E402
from egobox_amd import workload  # noqa: E402

PARTS = ("fit", "scaling", "scaling_lhs", "starts", "optimize", "total")


def training_rows(n, d, k):
    """x (n, d) in the unit box; y (n, 1 + k): a small-scale objective (the workload's Griewank function) and constraints -- the
    same function on a zoomed box -- whose zero level cuts the box (as tools/infill_bench.py builds its models)"""
    x, g = workload.make_training_set(n, d, seed=100)
    cols = [1e-3 * g]
    for j in range(1, 1 + k):
        c = workload.griewank(0.25 + 0.5 * x) if j % 2 else workload.griewank(0.8 * x)
        cols.append(c - np.quantile(c, 0.6) if j % 2 else np.quantile(c, 0.25) - c)
    return np.asarray(x, dtype=np.float64), np.column_stack(cols)


def run_coego(args, emit):
    n, d, k, n_coop = 500, 64, 2, 4
    emit("# one Egor.suggest call at d %d, n %d, objective + %d constraint surrogates, defaults: coego_n_coop = %d beside 0, the two"
         % (d, n, k, n_coop))
    emit("# alternated in one process; wall ms as q25 median q75 over %d calls after %d warm-ups; share = median / median of total"
         % (args.reps, args.warmup))
    emit("# coego_n_coop n d n_cstr part q25_ms median_ms q75_ms share")
    x, y = training_rows(n, d, k)
    egos = {c: egx.Egor(np.array([[0.0, 1.0]] * d), n_cstr=k, seed=1, coego_n_coop=c) for c in (n_coop, 0)}
    t = {c: {p: [] for p in PARTS} for c in egos}
    for r in range(args.warmup + args.reps):
        for c, ego in egos.items():
            t0 = time.perf_counter()
            xs = ego.suggest(x, y)
            total = time.perf_counter() - t0
            assert xs.shape == (1, d)
            if r >= args.warmup:
                for p in PARTS[:-1]:
                    t[c][p].append(ego.last_timings_[p] * 1e3)
                t[c]["total"].append(total * 1e3)
    for c in egos:
        med_total = float(np.median(t[c]["total"]))
        for p in PARTS:
            q1, q2, q3 = (float(v) for v in np.percentile(t[c][p], [25, 50, 75]))
            emit(f"{c} {n} {d} {k} {p} {q1:.1f} {q2:.1f} {q3:.1f} {q2 / med_total:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 4096])
    ap.add_argument("--coego", action="store_true", help="one suggest at d = 64, n = 500 with coego_n_coop = 4 beside 0")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "egor_coego_bench.txt" if args.coego else "egor_bench.txt")
    if args.reps is None:
        args.reps = 5 if args.coego else 9
    if args.warmup is None:
        args.warmup = 1 if args.coego else 3
    d, k = 8, 2
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if args.coego:
        run_coego(args, emit)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return

    emit("# one Egor.suggest call: d %d, objective + %d constraint surrogates, defaults (LogEI, SLSQP, 20 starts, mean constraints,"
         % (d, k))
    emit("# one cluster, theta tuned from 11 starts of at most 50 evaluations); wall ms as q25 median q75 over %d calls after %d"
         % (args.reps, args.warmup))
    emit("# warm-ups, one process; share = median / median of total; scaling_lhs is the part of scaling that draws its 800-point")
    emit("# Maximin LHS on the host")
    emit("# n d n_cstr part q25_ms median_ms q75_ms share")
    for n in args.sizes:
        x, y = training_rows(n, d, k)
        ego = egx.Egor(np.array([[0.0, 1.0]] * d), n_cstr=k, seed=1)
        t = {p: [] for p in PARTS}
        for r in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            xs = ego.suggest(x, y)
            total = time.perf_counter() - t0
            assert xs.shape == (1, d)
            if r >= args.warmup:
                for p in PARTS[:-1]:
                    t[p].append(ego.last_timings_[p] * 1e3)
                t["total"].append(total * 1e3)
        med_total = float(np.median(t["total"]))
        for p in PARTS:
            q1, q2, q3 = (float(v) for v in np.percentile(t[p], [25, 50, 75]))
            emit(f"{n} {d} {k} {p} {q1:.1f} {q2:.1f} {q3:.1f} {q2 / med_total:.3f}")
        egx.trim()
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
