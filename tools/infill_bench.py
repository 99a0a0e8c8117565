"""A/B of one infill evaluation: COMPOSED (what a caller does without egx_infill_*: predict_valvar + predict_valvar_gradients
per model, the criterion's arithmetic on the host with tests/infill_oracle.py) against FUSED (egx_infill_eval).  The composed
leg uses only entry points that exist without this feature, so it is the yardstick on any commit.

One process, legs alternated (composed, fused, composed again: the two composed runs show the spread), >= 3 warm-ups per
shape, medians.  Also: one lock-step optimize with 20 starts against 20 one-start calls.

    python tools/infill_bench.py [--out profiles/infill_eval_ab.txt] [--reps 15] [--only-m21]

--mix runs the MIXTURE leg instead: the objective is a smooth mixture of k = 3 experts (explicit Gaussian mixture, the clusters
overlapping in the unit box), no constraints.  Composed = GpMixture.predict_valvar + predict_valvar_gradients (the library's
mixture entry points) with the same host arithmetic; fused = the handle of egx_infill_create_mix.  Same protocol, written to
profiles/infill_mix_eval_ab.txt.

    python tools/infill_bench.py --mix [--out profiles/infill_mix_eval_ab.txt] [--reps 15]

--cstr times ONE LOCK-STEP ROUND of the constrained multistart -- a values-only evaluation of 20 trial points -- on one handle
in its three constraint strategies: MEAN and UTB (egx_infill_eval_cstr: the objective model and the constraint values; under
MEAN the constraint models run the mean-only sequence) and INFILL (egx_infill_eval: the constraints folded into the
objective, the full sequence for every model).  The INFILL leg uses only entry points that exist without the strategies: on
a commit without them the tool times that leg alone, which is the yardstick.  Legs alternated (infill, mean, utb, infill
again), medians, written to profiles/infill_cstr_round.txt.

    python tools/infill_bench.py --cstr [--out profiles/infill_cstr_round.txt] [--reps 15]

--sparse runs the SPARSE leg: the objective is one sparse GP (n = 20000, nz = 512, d = 8, Matern-5/2, FITC), no constraints,
value + gradient at m = 1, 128, 4096.  Composed = egx_sgp_predict_valvar + egx_sgp_predict_valvar_gradients (at m = 1 their
few-query route) with the same host arithmetic; fused = the handle of egx_infill_create_any, which runs the batched route at
the padded batch of 128 whatever m is.  Same protocol, written to profiles/infill_sparse_bench.txt; no threshold is set.

    python tools/infill_bench.py --sparse [--out profiles/infill_sparse_bench.txt] [--reps 15]

--slsqp times the reference's DEFAULT inner optimiser, SLSQP under EGX_CSTR_MEAN, on one handle (a dense objective, n = 500,
d = 8, two constraint models, WB2) from 20 starts, the reference's n_start: (a) egx_infill_optimize_slsqp, all starts in
lock-step; (b) the only way to run that optimiser without the call -- scipy's SLSQP, one start after the other, on the
m = 1 closure constraints(x, grad=True) (one library call per distinct point: value, gradient, constraints, Jacobian), which
uses only entry points that exist without the feature and is the yardstick on any commit; (c) egx_infill_optimize_cstr (COBYLA) from the same starts.  Every leg gets ftol 1e-4 and
at most 200 evaluations per start.  Legs alternated, medians with quartiles, the three optima, written to
profiles/infill_slsqp_bench.txt; no threshold is set.

    python tools/infill_bench.py --slsqp [--out profiles/infill_slsqp_bench.txt] [--reps 7]

--pending times the q-point batch (pending points: the models conditioned on virtual observations, no refit) on a dense objective
and two constraint models under EGX_CSTR_MEAN, d = 8, n = 500 and n = 4096: (a) one value + gradient evaluation at m = 1, 20,
4096 with q = 0, 1, 4, 8, 16 pending points -- q = 0 is the handle of the parent commit, the others add k_pending_cross and
k_pending_finish per (tile, model), FUSED, or with egx_set_tuning("pending_composed", 1) q launches of the existing mean and
x-gradient contractions in place of k_pending_cross, COMPOSED; (b) egx_infill_optimize_batch (q = 4, 20 starts, SLSQP, Kriging believer) against the REFIT
LOOP a caller writes without it: per step a new GpHandle on the n + i points finalised at the old theta, a new InfillObjective,
one optimize_slsqp, the believer's value from predict.  The refit loop uses only entry points that exist without the feature
and is the yardstick on any commit.  Legs alternated, >= 3 warm-ups, medians with quartiles, written to
profiles/infill_pending_bench.txt; no threshold is set.

    python tools/infill_bench.py --pending [--out profiles/infill_pending_bench.txt] [--reps 9]

--active times ACTIVE COORDINATES (egx_infill_set_active; CoEGO) on one handle in one process: an objective and two constraint
models, squared exponential, d = 32, 64, 128, 256 at n = 500 and n = 2000; one evaluation of 20 points with gradients, FULL
width (d columns: what the handle launches without an activity, k_xgrad) against an ACTIVITY of a = ceil(d / 5) shuffled columns
(compact rows, k_xgrad<LIST>: the pair correlation once per pass of listed columns), in both ways the optimisers evaluate: the
constraints folded into the objective (value_and_grad, six contractions per tile) and as mean constraints (constraints(x,
grad=True), four).  Legs alternated (full, active, full again: the two full runs show the spread), 3 warm-ups, medians with
quartiles, written to profiles/infill_active_bench.txt; no threshold is set.

    python tools/infill_bench.py --active [--out profiles/infill_active_bench.txt] [--reps 15]

--runs times RUNS (egx_infill_get_runs: consecutive surrogates of one shape through one launch sequence per tile) on an objective
and k = 2, 8, 68 constraint models (68: the reference's mopta08 example), squared exponential, n = 300 and n = 2000 at d = 8, and
d = 124 with 25 active columns at n = 300: one evaluation of 20 points with gradients, and the SLSQP multistart from 20 starts (at
most 30 evaluations per start).  Two variants: MEAN -- separately created models, the constraints as mean constraints (what Egor
builds by default: the run 1 | k) -- and FULL -- the models of one group, the constraints folded into the objective (one run of
1 + k, cut at 16).  The tool uses only entry points that exist without runs: run on another build of the library with
--package-root DIR (the directory that holds that build's egobox_amd), it times that build's walk, one sequence per model -- the
yardstick.  A job alternates the two builds in one GPU call and takes the medians per shape; the spread comes from two runs of
the same build.  Medians after 3 warm-ups, written to profiles/infill_runs_bench.txt; no threshold is set.

    python tools/infill_bench.py --runs [--out profiles/infill_runs_bench.txt] [--reps 9] [--package-root DIR]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_ROOT = ROOT
if "--package-root" in sys.argv[1:-1]:  # another build of the library (--runs): before the import below
    PKG_ROOT = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1])
sys.path.insert(0, PKG_ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import egobox_amd as egx  # noqa: E402
import infill_oracle as IO  # noqa: E402
from egobox_amd import workload  # noqa: E402


def build(n, d, k):
    hs, ys = [], []
    for j in range(1 + k):
        x, y = workload.make_training_set(n, d, seed=100 + j)
        if j:
            y = y - np.quantile(y, 0.6)
        h = egx.GpHandle(x, y)
        h.finalize(np.full(d, 1.5))
        hs.append(h), ys.append(y)
    return hs, ys


def composed(hs, tols, fmin, xq, want_grad):
    """the caller's loop: 2 (1 + k) library calls (1 + k without gradients), then the arithmetic on the host"""
    m, d = xq.shape
    nm = len(hs)
    mu, var = np.empty((nm, m)), np.empty((nm, m))
    dmu, dvar = np.zeros((nm, m, d)), np.zeros((nm, m, d))
    for j, h in enumerate(hs):
        mu[j], var[j] = h.predict_valvar(xq)
        if want_grad:
            dmu[j], dvar[j] = h.predict_valvar_gradients(xq)
    val = np.empty(m)
    grad = np.empty((m, d)) if want_grad else None
    for i in range(m):
        val[i] = IO.objective(IO.LOG_EI, mu[:, i], var[:, i], tols, fmin, 1.0, 1.0, 1.0, True, dev=True)
        if want_grad:
            grad[i] = IO.dev_objective_grad(IO.LOG_EI, (mu[:, i], var[:, i], dmu[:, i], dvar[:, i]), tols, fmin, 1.0, 1.0, 1.0, True)
    return val, grad


def build_mixture(n, d, k):
    """k experts on their own training sets and an explicit mixture whose clusters overlap in the unit box"""
    hs, ys = build(n, d, k - 1)  # (build shifts the outputs of all but the first; irrelevant for a timing)
    means = np.full((k, d), 0.5)
    means[:, 0] = (np.arange(k) + 0.5) / k
    gmx = egx.GaussianMixture(np.full(k, 1.0 / k), means, [np.eye(d) * 0.05] * k, 0.9)
    return egx.GpMixture([egx.GaussianProcess(h, None) for h in hs], gmx, "smooth"), hs, ys


def composed_mixture(mix, fmin, xq, want_grad):
    """2 mixture calls (each: responsibilities, every expert, the fold), then the arithmetic on the host"""
    m, d = xq.shape
    mu, var = (a[None, :] for a in mix.predict_valvar(xq))
    dmu = dvar = np.zeros((1, m, d))
    if want_grad:
        dmu, dvar = (a[None, :, :] for a in mix.predict_valvar_gradients(xq))
    val = np.empty(m)
    grad = np.empty((m, d)) if want_grad else None
    for i in range(m):
        val[i] = IO.objective(IO.LOG_EI, mu[:, i], var[:, i], [], fmin, 1.0, 1.0, 1.0, True, dev=True)
        if want_grad:
            grad[i] = IO.dev_objective_grad(IO.LOG_EI, (mu[:, i], var[:, i], dmu[:, i], dvar[:, i]), [], fmin, 1.0, 1.0, 1.0, True)
    return val, grad


def median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def quartiles_ms(fn, reps, warm=1):
    """(q25, median, q75) of the wall time in ms, and the last result"""
    out = None
    for _ in range(warm):
        out = fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return tuple(float(v) for v in np.percentile(t, [25, 50, 75])), out


def run_slsqp(args, emit):
    n, d, k, n_start, budget = 500, 8, 2, 20, 200
    hs, ys = [], []
    for j in range(1 + k):  # constraint 2 cuts the centre of the box out: active at the optimum
        x, y = workload.make_training_set(n, d, seed=100 + j)
        y = 1e-3 * y if j == 0 else (y - np.quantile(y, 0.6) if j == 1 else np.quantile(y, 0.25) - y)
        h = egx.GpHandle(x, y)
        h.finalize(np.full(d, 1.5))
        hs.append(h), ys.append(y)
    tols = [1e-3, 1e-3]
    obj = egx.InfillObjective(hs[0], hs[1:], tols, criterion=egx.WB2, fmin=float(np.quantile(ys[0], 0.05)))
    rng = np.random.default_rng(1)
    lim = np.array([[0.0, 1.0]] * d)
    starts = rng.random((n_start, d))
    obj.set_cstr_strategy("mean")
    obj.scaling(rng.random((200, d)))
    cfeas = np.array(tols) / obj.cstr_strategy()[1]
    has = hasattr(obj, "optimize_slsqp")

    def leg_lib():
        return obj.optimize_slsqp(lim, starts, max_eval=budget)

    def leg_scipy():
        from scipy.optimize import minimize
        res, calls = [], []
        for x0 in starts:
            memo = {}

            def at(x):  # ONE m = 1 library call per distinct point: value, gradient, constraints and their Jacobian
                key = x.tobytes()
                if key not in memo:
                    v, c, g, gc = obj.constraints(x[None], grad=True)
                    memo[key] = (v[0], g[0], c[0], gc[0])
                return memo[key]
            cons = [{"type": "ineq", "fun": lambda x: cfeas - at(x)[2], "jac": lambda x: -at(x)[3]}]
            r = minimize(lambda x: at(x)[:2], x0, jac=True, method="SLSQP", bounds=[tuple(b) for b in lim], constraints=cons,
                         options={"ftol": 1e-4, "maxiter": budget})
            v, _, c, _ = at(r.x)
            res.append((not np.max(c - cfeas) > 0.0, v, r.x, c))
            calls.append(len(memo))
        feas = [r for r in res if r[0]]
        best = min(feas or res, key=lambda r: r[1] if feas else np.max(r[3] - cfeas))
        return best[2], best[1], best[3], dict(evals=np.array(calls), feasible=best[0], violation=float(np.max(best[3] - cfeas)))

    def leg_cobyla():
        return obj.optimize_constrained(lim, starts, max_eval=budget)

    emit("# SLSQP multistart under EGX_CSTR_MEAN: n %d d %d n_cstr %d n_start %d WB2, ftol 1e-4, at most %d evaluations per start;"
         % (n, d, k, n_start, budget))
    emit("# (a) egx_infill_optimize_slsqp, (b) scipy SLSQP start after start on the m = 1 closures, (c) egx_infill_optimize_cstr")
    emit("# (COBYLA); wall ms as q25 median q75 over %d runs after 1 warm-up, legs alternated (b, a, c, b again)" % args.reps)
    try:
        import scipy
        sp = tuple(int(v) for v in scipy.__version__.split(".")[:2]) < (1, 16)
    except ImportError:
        sp = False
    legs = [("b", leg_scipy, sp), ("a", leg_lib, has), ("c", leg_cobyla, True), ("b2", leg_scipy, sp)]
    emit("# leg q25_ms median_ms q75_ms rounds evals_per_start(min median max) f_best feasible violation")
    for name, fn, on in legs:
        if not on:
            emit(f"{name} not available here")
            continue
        (q1, q2, q3), (xb, fb, cb, st) = quartiles_ms(fn, args.reps)
        ev = st["evals"]
        emit(f"{name} {q1:.1f} {q2:.1f} {q3:.1f} {st.get('rounds', int(ev.sum()))} {ev.min()} {int(np.median(ev))} {ev.max()} {fb:.9g} "
             f"{int(st['feasible'])} {st['violation']:.3e}")
    emit("# rounds of leg b: its evaluation calls, every one a launch sequence of its own for one point")
    obj.close()
    for h in hs:
        h.close()


def run_pending(args, emit):
    d, k, n_start, q_batch, budget = 8, 2, 20, 4, 200
    rng = np.random.default_rng(1)
    lim = np.array([[0.0, 1.0]] * d)
    emit("# pending points: objective + %d constraint models under EGX_CSTR_MEAN, d %d, LogEI; wall ms as q25 median q75 over %d"
         % (k, d, args.reps))
    emit("# runs after 3 warm-ups, legs alternated")
    for n in (500, 4096):
        xs, ys, hs = [], [], []
        for j in range(1 + k):
            x, y = workload.make_training_set(n, d, seed=100 + j)
            y = 1e-3 * y if j == 0 else (y - np.quantile(y, 0.6) if j == 1 else np.quantile(y, 0.25) - y)
            h = egx.GpHandle(x, y)
            h.finalize(np.full(d, 1.5))
            xs.append(x), ys.append(y), hs.append(h)
        tols = [1e-3, 1e-3]
        kw = dict(criterion=egx.LOG_EI, fmin=float(np.quantile(ys[0], 0.05)))
        obj = egx.InfillObjective(hs[0], hs[1:], tols, **kw)
        obj.set_cstr_strategy("mean")
        has = hasattr(obj, "push_pending")
        # (a) one evaluation with gradients; the q legs of one m are visited in turn, twice (the two q = 0 runs show the spread)
        emit("# (a) n m q fused: q25_ms median_ms q75_ms  composed (q > 0): q25_ms median_ms q75_ms"
             "  [constraints(x, grad=True): value, gradient, constraints, their Jacobian]")
        pend = rng.random((16, d))
        for m in (1, 20, 4096):
            xq = rng.random((m, d))
            for q in (0, 1, 4, 8, 16, 0):
                if q and not has:
                    emit(f"a {n} {m} {q} not available here")
                    continue
                if has:
                    obj.clear_pending()
                    for v in range(q):
                        obj.push_pending(pend[v], obj.virtual_point(pend[v], "kb_ub"))
                (q1, q2, q3), _ = quartiles_ms(lambda: obj.constraints(xq, grad=True), args.reps, warm=3)
                line = f"a {n} {m} {q} {q1:.3f} {q2:.3f} {q3:.3f}"
                if q:  # the composed form on the same handle: q launches of the existing contractions per (tile, model)
                    egx.set_tuning("pending_composed", 1)
                    try:
                        (c1, c2, c3), _ = quartiles_ms(lambda: obj.constraints(xq, grad=True), args.reps, warm=3)
                    finally:
                        egx.set_tuning("pending_composed", 0)
                    line += f" {c1:.3f} {c2:.3f} {c3:.3f}"
                emit(line)
        if has:
            obj.clear_pending()
        # (b) the batch
        starts = rng.random((q_batch, n_start, d))

        def leg_batch():
            obj.clear_pending()
            return obj.optimize_batch(lim, starts, q_batch, strategy="kb", optimizer="slsqp", max_eval=budget)[2]

        def leg_refit():
            xa, ya, f = [x.copy() for x in xs], [y.copy() for y in ys], []
            for i in range(q_batch):
                if i == 0:
                    cur, own = hs, []
                else:
                    own = [egx.GpHandle(xj, yj) for xj, yj in zip(xa, ya)]
                    for h in own:
                        h.finalize(np.full(d, 1.5))
                    cur = own
                o = egx.InfillObjective(cur[0], cur[1:], tols, **kw)
                o.set_cstr_strategy("mean")
                xb, fb = o.optimize_slsqp(lim, starts[i], max_eval=budget)[:2]
                yv = [float(h.predict(xb[None])[0]) for h in cur]
                o.close()
                for h in own:
                    h.close()
                for j in range(1 + k):
                    xa[j], ya[j] = np.vstack([xa[j], xb]), np.append(ya[j], yv[j])
                f.append(fb)
            return np.array(f)

        emit("# (b) leg n q n_start q25_ms median_ms q75_ms f_out  [batch: egx_infill_optimize_batch; refit: the caller's loop]")
        for name, fn, on in (("refit", leg_refit, True), ("batch", leg_batch, has), ("refit2", leg_refit, True)):
            if not on:
                emit(f"b {name} {n} not available here")
                continue
            (q1, q2, q3), f = quartiles_ms(fn, max(3, args.reps // 3), warm=3)
            emit(f"b {name} {n} {q_batch} {n_start} {q1:.1f} {q2:.1f} {q3:.1f} " + " ".join(f"{v:.6g}" for v in f))
        obj.close()
        for h in hs:
            h.close()


def run_active(args, emit):
    k, m = 2, 20
    rng = np.random.default_rng(1)
    emit("# active coordinates: objective + %d constraint models, squared exponential, LogEI; one evaluation of %d points with" % (k, m))
    emit("# gradients, full width (d columns) against an activity of a = ceil(d / 5) shuffled columns on the SAME handle; wall ms as")
    emit("# q25 median q75 over %d calls after 3 warm-ups, legs alternated (full, active, full again); speedup = median full /" % args.reps)
    emit("# median active, full = the mean of the two full runs' medians")
    emit("# strategy n d a full: q25_ms median_ms q75_ms  active: q25_ms median_ms q75_ms  full again: q25_ms median_ms q75_ms  speedup")
    for n in (500, 2000):
        for d in (32, 64, 128, 256):
            hs, ys = [], []
            for j in range(1 + k):
                x, y = workload.make_training_set(n, d, seed=100 + j)
                y = 1e-3 * y if j == 0 else y - np.quantile(y, 0.6)
                h = egx.GpHandle(x, y)
                h.finalize(np.full(d, 1.5 / d))
                hs.append(h), ys.append(y)
            a = -(-d // 5)
            act = rng.permutation(d)[:a]
            xq = rng.random((m, d))
            xb, xc = xq[0].copy(), np.ascontiguousarray(xq[:, act])
            with egx.InfillObjective(hs[0], hs[1:], [1e-3] * k, criterion=egx.LOG_EI, fmin=float(np.quantile(ys[0], 0.05))) as obj:
                for strategy in ("infill", "mean"):
                    obj.set_cstr_strategy(strategy)
                    call = obj.value_and_grad if strategy == "infill" else (lambda pts: obj.constraints(pts, grad=True))
                    legs = []
                    for leg in ("full", "active", "full"):
                        if leg == "active":
                            obj.set_active(act, xb)
                        pts = xc if leg == "active" else xq
                        legs.append(quartiles_ms(lambda: call(pts), args.reps, warm=3)[0])
                        obj.clear_active()
                    full = 0.5 * (legs[0][1] + legs[2][1])
                    emit(f"{strategy} {n} {d} {a} " + "  ".join(f"{q1:.3f} {q2:.3f} {q3:.3f}" for q1, q2, q3 in legs) +
                         f"  {full / legs[1][1]:.2f}")
            for h in hs:
                h.close()
            egx.trim()


def run_runs(args, emit):
    m, n_start, budget = 20, 20, 30
    rng = np.random.default_rng(2)
    emit("# runs: objective + k constraint models, squared exponential, LogEI; eval = one evaluation of %d points with gradients," % m)
    emit("# slsqp = the SLSQP multistart from %d starts, at most %d evaluations per start; MEAN: separate models, mean constraints;" % (n_start, budget))
    emit("# FULL: the models of one group, the constraints folded into the objective; a = active columns (0: full width);")
    emit("# median wall ms over %d calls after 3 warm-ups; package: %s" % (args.reps, os.path.relpath(PKG_ROOT, ROOT)))
    emit("# variant n d a k runs eval_ms slsqp_ms")
    for n, d, a in ((300, 8, 0), (2000, 8, 0), (300, 124, 25)):
        for k in (2, 8, 68):
            xs, ys = [], []
            for j in range(1 + k):
                x, y = workload.make_training_set(n, d, seed=100 + j)
                xs.append(x), ys.append(1e-3 * y if j == 0 else y - np.quantile(y, 0.6))
            thetas = np.full((1 + k, d), 1.5 if d == 8 else 1.5 / d)
            for variant in ("MEAN", "FULL"):
                if variant == "FULL":
                    hs = egx.GpHandle.create_group(np.stack(xs), np.stack(ys))
                    egx.finalize_multi(hs, thetas)
                else:
                    hs = [egx.GpHandle(x, y) for x, y in zip(xs, ys)]
                    for h, th in zip(hs, thetas):
                        h.finalize(th)
                with egx.InfillObjective(hs[0], hs[1:], [1e-3] * k, criterion=egx.LOG_EI, fmin=float(np.quantile(ys[0], 0.05))) as obj:
                    obj.set_cstr_strategy("mean" if variant == "MEAN" else "infill")
                    runs = "|".join(str(v) for v in obj.runs) if hasattr(type(obj), "runs") else "-"
                    w = a if a else d
                    if a:
                        obj.set_active(rng.permutation(d)[:a], np.full(d, 0.5))
                    xq, starts = rng.random((m, w)), rng.random((n_start, w))
                    lim = np.tile([0.0, 1.0], (w, 1))
                    call = obj.value_and_grad if variant == "FULL" else (lambda pts: obj.constraints(pts, grad=True))
                    t_eval = median_ms(lambda: call(xq), args.reps)
                    t_opt = median_ms(lambda: obj.optimize_slsqp(lim, starts, max_eval=budget), max(3, args.reps // 3), warm=1)
                    emit(f"{variant} {n} {d} {a} {k} {runs} {t_eval:.3f} {t_opt:.3f}")
                for h in hs:
                    h.close()
                egx.trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mix", action="store_true", help="the mixture leg (k = 3 experts, smooth) instead of the single-model legs")
    ap.add_argument("--cstr", action="store_true", help="one lock-step round in MEAN, UTB and INFILL mode on one handle")
    ap.add_argument("--sparse", action="store_true", help="the sparse leg: one sparse objective (nz = 512, d = 8), value + gradient")
    ap.add_argument("--slsqp", action="store_true", help="20 starts of SLSQP: the lock-step call, scipy on the m = 1 closures, COBYLA")
    ap.add_argument("--pending", action="store_true", help="pending points: one evaluation at q = 0 .. 16, the batch call against the refit loop")
    ap.add_argument("--active", action="store_true", help="active coordinates: one evaluation of 20 points, full width against a = d / 5 columns")
    ap.add_argument("--runs", action="store_true", help="runs: objective + 2, 8, 68 constraints, one evaluation and the SLSQP multistart")
    ap.add_argument("--package-root", default=None, help="(--runs) the directory that holds another build's egobox_amd package")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only-m21", action="store_true", help="the m = 21 fused leg alone, small shape (for a kernel trace)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "infill_runs_bench.txt" if args.runs else "infill_active_bench.txt" if args.active else "infill_pending_bench.txt" if args.pending else "infill_slsqp_bench.txt" if args.slsqp else "infill_cstr_round.txt" if args.cstr else "infill_sparse_bench.txt" if args.sparse
                                else "infill_mix_eval_ab.txt" if args.mix else "infill_eval_ab.txt")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if args.only_m21:
        hs, ys = build(4096, 8, 2)
        obj = egx.InfillObjective(hs[0], hs[1:], [0.0, 0.0], criterion=egx.LOG_EI, fmin=float(np.quantile(ys[0], 0.05)))
        xq = np.random.default_rng(0).random((21, 8))
        for _ in range(3):
            obj.value_and_grad(xq)
        for _ in range(10):
            obj.value(xq)
            obj.value_and_grad(xq)
        return
    if args.slsqp or args.pending or args.active or args.runs:
        (run_runs if args.runs else run_active if args.active else run_pending if args.pending else run_slsqp)(args, emit)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return
    if args.cstr:
        m = 20
        emit("# one lock-step round of the constrained multistart: a values-only evaluation of %d trial points on ONE handle in its" % m)
        emit("# three constraint strategies; LogEI; constraint models of the objective's size; median ms over %d calls after 3" % args.reps)
        emit("# warm-ups; legs alternated (infill, mean, utb, infill again: the two infill runs show the spread)")
        emit("# n d n_cstr m infill_a_ms mean_ms utb_ms infill_b_ms infill_spread mean/infill utb/infill 1/(1+n_cstr)")
        for n, d, k in ((2048, 8, 1), (4096, 8, 2), (4096, 8, 4)):
            hs, ys = build(n, d, k)
            obj = egx.InfillObjective(hs[0], hs[1:], [0.0] * k, criterion=egx.LOG_EI, fmin=float(np.quantile(ys[0], 0.05)))
            xq = np.random.default_rng(1).random((m, d))
            has = hasattr(obj, "set_cstr_strategy")

            def leg(strategy):
                if not has:
                    return float("nan") if strategy != "infill" else median_ms(lambda: obj.value(xq), args.reps)
                obj.set_cstr_strategy(strategy)
                return median_ms((lambda: obj.value(xq)) if strategy == "infill" else (lambda: obj.constraints(xq)), args.reps)
            ia, me, ut, ib = leg("infill"), leg("mean"), leg("utb"), leg("infill")
            i0 = min(ia, ib)
            emit(f"{n} {d} {k} {m} {ia:.3f} {me:.3f} {ut:.3f} {ib:.3f} {abs(ia - ib):.3f} {me / i0:.3f} {ut / i0:.3f} {1.0 / (1 + k):.3f}")
            obj.close()
            for h in hs:
                h.close()
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return
    if args.sparse:
        n, nz, d = 20000, 512, 8
        emit("# infill evaluation on a sparse objective, composed (egx_sgp_predict_valvar + egx_sgp_predict_valvar_gradients + host")
        emit("# arithmetic) vs fused (egx_infill_create_any / egx_infill_eval); LogEI, value + gradient, no constraints; Matern-5/2,")
        emit("# FITC; median ms over %d calls (m = 4096: a fifth of them) after 3 warm-ups; legs alternated" % args.reps)
        emit("# n nz d m composed_a_ms fused_ms composed_b_ms composed_spread fused/composed verdict  (composed_lib_ms: its two library calls alone)")
        rng = np.random.default_rng(0)
        x = rng.random((n, d)) * 2 - 1
        y = np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, -1]) + 0.05 * rng.standard_normal(n)
        z = x[rng.permutation(n)[:nz]].copy()
        h = egx.SgpHandle(x, y, z, corr=3, method=0)
        h.finalize(np.full(d, 2.0 / np.sqrt(d)), 1.3, 0.01)
        fmin = float(np.quantile(y, 0.05))
        obj = egx.InfillObjective(h, criterion=egx.LOG_EI, fmin=fmin)
        for m in (1, 128, 4096):
            xq = rng.random((m, d)) * 2 - 1
            reps = args.reps if m < 4096 else max(3, args.reps // 5)
            fused = lambda: obj.value_and_grad(xq)  # noqa: E731
            lib = lambda: (h.predict_valvar(xq), h.predict_valvar_gradients(xq))  # noqa: E731
            comp = lambda: composed([h], [], fmin, xq, True)  # noqa: E731
            vc, gc = comp()
            vf, gf = fused()
            ok = np.allclose(vf, vc, rtol=1e-6, atol=1e-6) and np.allclose(gf, gc, rtol=1e-4, atol=1e-5 * (1 + np.abs(gc).max()))
            ca = median_ms(comp, reps)
            fu = median_ms(fused, reps)
            cb = median_ms(comp, reps)
            cl = median_ms(lib, reps)
            c = min(ca, cb)
            verdict = "fused faster" if fu < c else ("within the spread" if fu <= max(ca, cb) else "FUSED SLOWER")
            emit(f"{n} {nz} {d} {m} {ca:.3f} {fu:.3f} {cb:.3f} {abs(ca - cb):.3f} {fu / c:.3f} {verdict}"
                 + ("" if ok else "  RESULTS DIFFER") + f"  (composed_lib_ms {cl:.3f})")
        obj.close()
        h.close()
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return
    if args.mix:
        kx = 3
        emit("# infill evaluation on a mixture surrogate, composed (GpMixture.predict_valvar + predict_valvar_gradients + host")
        emit("# arithmetic) vs fused (egx_infill_create_mix / egx_infill_eval); LogEI, objective = smooth mixture of %d experts, no" % kx)
        emit("# constraints; median ms over %d calls after 3 warm-ups; legs alternated" % args.reps)
        emit("# n d experts m grad composed_a_ms fused_ms composed_b_ms composed_spread fused/composed verdict")
        for n, d in ((2048, 8), (4096, 8)):
            mix, hs, ys = build_mixture(n, d, kx)
            fmin = float(np.quantile(ys[0], 0.05))
            obj = egx.InfillObjective(mix, criterion=egx.LOG_EI, fmin=fmin)
            rng = np.random.default_rng(1)
            for m in (1, 21, 800):
                xq = rng.random((m, d))
                reps = args.reps if m < 800 else max(3, args.reps // 5)
                for want_grad in (False, True):
                    fused = (lambda: obj.value_and_grad(xq)) if want_grad else (lambda: obj.value(xq))
                    comp = lambda: composed_mixture(mix, fmin, xq, want_grad)  # noqa: E731
                    vc, gc = comp()
                    vf = fused()
                    vf, gf = vf if want_grad else (vf, None)
                    ok = np.allclose(vf, vc, rtol=1e-6, atol=1e-6) and (
                        not want_grad or np.allclose(gf, gc, rtol=1e-4, atol=1e-5 * (1 + np.abs(gc).max())))
                    ca = median_ms(comp, reps)
                    fu = median_ms(fused, reps)
                    cb = median_ms(comp, reps)
                    c = min(ca, cb)
                    verdict = "fused faster" if fu < c else ("within the spread" if fu <= max(ca, cb) else "FUSED SLOWER")
                    emit(f"{n} {d} {kx} {m} {int(want_grad)} {ca:.3f} {fu:.3f} {cb:.3f} {abs(ca - cb):.3f} {fu / c:.3f} {verdict}"
                         + ("" if ok else "  RESULTS DIFFER"))
            obj.close()
            for h in hs:
                h.close()
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return
    emit("# infill evaluation, composed (predict_valvar + predict_valvar_gradients per model + host arithmetic) vs fused")
    emit("# (egx_infill_eval); LogEI, k = 2 constraint models; median ms over %d calls after 3 warm-ups; legs alternated" % args.reps)
    emit("# n d k m grad composed_a_ms fused_ms composed_b_ms composed_spread fused/composed verdict")
    for n, d, k in ((4096, 8, 2), (8192, 16, 2)):
        hs, ys = build(n, d, k)
        tols = [0.0] * k
        fmin = float(np.quantile(ys[0], 0.05))
        obj = egx.InfillObjective(hs[0], hs[1:], tols, criterion=egx.LOG_EI, fmin=fmin)
        rng = np.random.default_rng(1)
        for m in (1, 21, 800):
            xq = rng.random((m, d))
            reps = args.reps if m < 800 else max(3, args.reps // 5)
            for want_grad in (False, True):
                fused = (lambda: obj.value_and_grad(xq)) if want_grad else (lambda: obj.value(xq))
                comp = lambda: composed(hs, tols, fmin, xq, want_grad)  # noqa: E731
                vc, gc = comp()
                vf = fused()
                vf, gf = vf if want_grad else (vf, None)
                ok = np.allclose(vf, vc, rtol=1e-6, atol=1e-6) and (not want_grad or np.allclose(gf, gc, rtol=1e-4, atol=1e-5 * (1 + np.abs(gc).max())))
                ca = median_ms(comp, reps)
                fu = median_ms(fused, reps)
                cb = median_ms(comp, reps)
                spread = abs(ca - cb)
                c = min(ca, cb)
                verdict = "fused faster" if fu < c else ("within the spread" if fu <= max(ca, cb) else "FUSED SLOWER")
                emit(f"{n} {d} {k} {m} {int(want_grad)} {ca:.3f} {fu:.3f} {cb:.3f} {spread:.3f} {fu / c:.3f} {verdict}"
                     + ("" if ok else "  RESULTS DIFFER"))
        # the multistart: 20 starts in lock-step against 20 one-start calls
        starts = rng.random((20, d))
        lim = np.array([[0.0, 1.0]] * d)
        obj.scaling(rng.random((200, d)))
        obj.optimize(lim, starts[:2], max_eval=20)  # warm-up
        t0 = time.perf_counter()
        f, xb, st = obj.optimize(lim, starts, max_eval=100)
        t_lock = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        singles = [obj.optimize(lim, starts[i:i + 1], max_eval=100) for i in range(20)]
        t_single = (time.perf_counter() - t0) * 1e3
        same = f == min(s[0] for s in singles)
        emit(f"# optimize n {n} d {d} k {k}: 20 starts lock-step {t_lock:.1f} ms ({st['rounds']} rounds, {int(st['evals'].sum())} evaluations), "
             f"20 one-start calls {t_single:.1f} ms, same optimum: {same}")
        obj.close()
        for h in hs:
            h.close()
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
