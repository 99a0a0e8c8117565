"""Timing of the Gaussian-mixture training (egx_gmm_fit: EM, the restarts in lock-step on the GPU).

Per shape (n, D, k, R): the time of one EM iteration for all R restarts -- the slope between two runs with tol = 0 and
max_iter = 5 and 25, so that upload, iteration 0 and the read-back of the result cancel --, the achieved FP64 rate against
the 78.6 TFLOP/s vector peak, and a whole training under the default stopping rule.  The data are OVERLAPPING blobs
(separation 2.5 spreads): responsibilities are not one-hot and the restarts need tens of iterations.

flop count per iteration (useful work; padding of D to a multiple of 4 and the recomputed x - mu are not counted):
    n R k (2 D (D + 1) + 5 D):  z = (x - mu) P over the triangle D (D + 1), ||z||^2 2 D, x - mu D,
                                 the second moments over the lower triangle D (D + 1), w (x - mu) D, the first moments D

The same training on the host: scikit-learn's GaussianMixture (init_params="random_from_data", the library's tol, max_iter and
reg_covar) with `--cpu-inits` restarts (default 2: 20 restarts of the large shape take minutes), reported per restart and
iteration; without scikit-learn the numpy oracle of tests/gmm_oracle.py, named as such.

    python tools/gmm_bench.py [--out profiles/gmm_bench.txt] [--reps 5] [--cpu-inits 2] [--profile-only]

--wide: the same figures for egx_gmm_fit_wide (rows up to 128 wide, the two O(D^2) products per row on the FP64 matrix unit,
whose peak is the same 78.6 TFLOP/s) at n = 4096 and 65536, D = 48 and 128, k = 4, R = 20, into profiles/gmm_wide_bench.txt;
the host's restarts stop at `--cpu-max-iter` iterations (default 10; the figure is per restart and iteration).  Then D = 33,
which both entry points take: the wide one against the narrow one in this process, alternated call by call.  No threshold:
the figures are reported whatever they are, and rows of 36 columns or fewer stay on the narrow path whatever the ratio.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import egobox_amd as egx  # noqa: E402
import gmm_oracle as GO  # noqa: E402

PEAK_TFLOPS = 78.6
SHAPES = ((65536, 17, 8, 20), (4096, 9, 4, 20))
WIDE_SHAPES = ((4096, 48, 4, 20), (65536, 48, 4, 20), (4096, 128, 4, 20), (65536, 128, 4, 20))
BOTH_SHAPES = ((4096, 33, 4, 20), (65536, 33, 4, 20))  # what the narrow and the wide entry point both take


def flops_per_iteration(n, d, k, r):
    return float(n) * r * k * (2 * d * (d + 1) + 5 * d)


def median_ms(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", action="store_true", help="egx_gmm_fit_wide at D = 48 and 128, and against egx_gmm_fit at D = 33")
    ap.add_argument("--out", default=None, help="default profiles/gmm_bench.txt, with --wide profiles/gmm_wide_bench.txt")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-inits", type=int, default=2)
    ap.add_argument("--cpu-max-iter", type=int, default=None, help="iterations of a host restart (default 100, with --wide 10)")
    ap.add_argument("--profile-only", action="store_true", help="ten iterations of each shape and nothing else (for a kernel trace)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "gmm_wide_bench.txt" if args.wide else "gmm_bench.txt")
    cpu_max_iter = args.cpu_max_iter or (10 if args.wide else 100)
    fit, entry = (egx.GaussianMixture.fit_wide, "egx_gmm_fit_wide") if args.wide else (egx.GaussianMixture.fit, "egx_gmm_fit")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# {entry}: full-covariance EM, R restarts in lock-step; overlapping blobs (separation 2.5 spreads)")
    for n, d, k, r in (WIDE_SHAPES if args.wide else SHAPES):
        x = GO.blobs(n, d, k, seed=1, separation=2.5)
        st = GO.starts(x, r, k, seed=2)

        def fixed(iters):
            return fit(x, k, n_runs=r, max_iter=iters, tol=0.0, init_means=st)

        if args.profile_only:
            fixed(10)
            continue
        t5 = median_ms(lambda: fixed(5), args.reps)
        t25 = median_ms(lambda: fixed(25), args.reps)
        per_iter = (t25 - t5) / 20.0
        fl = flops_per_iteration(n, d, k, r)
        tf = fl / (per_iter * 1e-3) / 1e12
        emit(f"n {n} D {d} k {k} R {r}: max_iter 5 {t5:.2f} ms, max_iter 25 {t25:.2f} ms -> {per_iter:.3f} ms per EM iteration "
             f"(all {r} restarts), {fl:.3e} flop per iteration, {tf:.2f} TFLOP/s FP64 = {100 * tf / PEAK_TFLOPS:.1f} % of {PEAK_TFLOPS}")
        one = median_ms(lambda: fit(x, k, n_runs=1, max_iter=25, tol=0.0, init_means=st[:1]), args.reps)
        emit(f"    one restart alone, max_iter 25: {one:.2f} ms (the batch of {r}: {t25:.2f} ms)")
        t0 = time.perf_counter()
        gm = fit(x, k, n_runs=r, init_means=st)
        whole = (time.perf_counter() - t0) * 1e3
        emit(f"    whole training, defaults (tol 1e-3, max_iter 100): {whole:.1f} ms, iterations per restart min {gm.n_iters_.min()} "
             f"median {int(np.median(gm.n_iters_))} max {gm.n_iters_.max()}, statuses {np.bincount(gm.statuses_, minlength=3).tolist()}, "
             f"lower bound {gm.lower_bound_:.6f}")
        ni = max(1, min(args.cpu_inits, r))
        try:
            from sklearn.mixture import GaussianMixture as SkGmm
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t0 = time.perf_counter()
                iters = 0
                best = -np.inf
                for j in range(ni):  # one restart per fit: n_iter_ of every restart is known
                    sk = SkGmm(n_components=k, covariance_type="full", tol=1e-3, max_iter=cpu_max_iter, reg_covar=1e-6, n_init=1,
                               init_params="random_from_data", random_state=j).fit(x)
                    iters += sk.n_iter_
                    best = max(best, sk.lower_bound_)
                cpu = (time.perf_counter() - t0) * 1e3
            emit(f"    host, scikit-learn GaussianMixture, {ni} restart(s) on {os.environ.get('OMP_NUM_THREADS', '?')} threads: {cpu:.0f} ms, "
                 f"{iters} iterations -> {cpu / iters:.2f} ms per restart and iteration (the GPU: {per_iter / r:.4f}); "
                 f"best lower bound {best:.6f}")
        except ImportError:
            t0 = time.perf_counter()
            runs, _ = GO.fit(x, st[:ni], max_iter=cpu_max_iter)
            cpu = (time.perf_counter() - t0) * 1e3
            iters = sum(run["n_iter"] for run in runs)
            emit(f"    host, the numpy oracle of tests/gmm_oracle.py (scikit-learn is not installed), {ni} restart(s): {cpu:.0f} ms, "
                 f"{iters} iterations -> {cpu / max(1, iters):.2f} ms per restart and iteration (the GPU: {per_iter / r:.4f})")
    if args.wide and not args.profile_only:
        emit("# D = 33: egx_gmm_fit_wide against egx_gmm_fit, the same starts, alternated call by call in one process")
        for n, d, k, r in BOTH_SHAPES:
            x = GO.blobs(n, d, k, seed=1, separation=2.5)
            st = GO.starts(x, r, k, seed=2)
            t = {}
            for iters in (5, 25):
                for f in (egx.GaussianMixture.fit, egx.GaussianMixture.fit_wide):  # warm both
                    f(x, k, n_runs=r, max_iter=iters, tol=0.0, init_means=st)
                for name in ("narrow", "wide"):
                    t[name, iters] = []
                for _ in range(args.reps):
                    for name, f in (("narrow", egx.GaussianMixture.fit), ("wide", egx.GaussianMixture.fit_wide)):
                        t0 = time.perf_counter()
                        f(x, k, n_runs=r, max_iter=iters, tol=0.0, init_means=st)
                        t[name, iters].append((time.perf_counter() - t0) * 1e3)
            per = {name: (float(np.median(t[name, 25])) - float(np.median(t[name, 5]))) / 20.0 for name in ("narrow", "wide")}
            emit(f"n {n} D {d} k {k} R {r}: narrow {per['narrow']:.3f} ms per EM iteration, wide {per['wide']:.3f} ms "
                 f"-> wide / narrow = {per['wide'] / per['narrow']:.2f}")
    if not args.profile_only:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
