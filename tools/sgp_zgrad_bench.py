#!/usr/bin/env python3
"""Sparse GP on one GPU: what the likelihood gradient in the inducing points costs, and what a fit that moves them gains.
GPU only, one process.
  1. At (n, nz, d) = (10^6, 512, 8) and (10^5, 256, 32), squared exponential, FITC: median wall time (host clock around calls
     that end in a device synchronise) of `likelihood_grad` and of `likelihood_grad_z` at fixed parameters, 9 rounds after 3
     warm-up rounds, the legs of a round alternated (grad, grad_z, grad): `likelihood_grad` is timed twice, and the distance
     between its two medians is the spread to read the difference with.
  2. Griewank on [-5, 5]^4, n = 20000, nz = 64 (a draw of training rows), FITC and VFE, Matern-5/2: `fit_lbfgs` against
     `fit_lbfgs_z` from the same single start -- fitted likelihood, RMSE on 5000 held-out points, evaluations, wall time.
Writes the table to --out (default profiles/sgp_zgrad_bench.txt).
    python tools/sgp_zgrad_bench.py [--cases n,nz,d ...] [--out FILE]
Per-kernel times come from a run of their own under the profiler, which this tool only feeds and reads:
    rocprofv3 --kernel-trace --stats -d DIR -o zgrad -- python tools/sgp_zgrad_bench.py --trace-only 1000000,512,8
    python tools/sgp_zgrad_bench.py --kernel-stats DIR/.../zgrad_results.db --out FILE     (appends to FILE)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(n, nz, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d)) * 2 - 1
    y = np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, -1]) + 0.05 * rng.standard_normal(n)
    z = x[rng.permutation(n)[:nz]].copy()
    return x, y, z


def griewank(x):
    i = np.arange(1, x.shape[1] + 1)
    return 1.0 + (x * x).sum(axis=1) / 4000.0 - np.prod(np.cos(x / np.sqrt(i)), axis=1)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_stats(path, out):
    """Append, from a rocprofv3 rocpd database, the launches of the two rectangle kernels, one line per kernel and grid: the
    large grids are the n x nz rectangle, the small ones the nz x nz one."""
    import sqlite3

    lines = [f"rocprofv3 --kernel-trace --stats ({os.path.basename(path)}): kernel, grid in workgroups, calls, average us, min us"]
    q = """select s.kernel_name, d.grid_size_x / d.workgroup_size_x, d.grid_size_y, d.grid_size_z, count(*),
                  avg(d.end - d.start) / 1e3, min(d.end - d.start) / 1e3
           from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id
           where s.kernel_name like '%k_sgp_grad_cols%' or s.kernel_name like '%k_sgp_grad_rect%'
           group by 1, 2, 3, 4 order by 6 desc"""
    for name, gx, gy, gz, calls, avg, lo in sqlite3.connect(path).cursor().execute(q):
        short = name[name.find("k_sgp_grad"):].split("(")[0]
        lines.append(f"  {short}: grid {gx} x {gy} x {gz}, {calls} calls, {avg:.1f} us, {lo:.1f} us")
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["1000000,512,8", "100000,256,32"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-fit", action="store_true", help="skip part 2")
    ap.add_argument("--trace-only", default=None, metavar="n,nz,d", help="three likelihood_grad_z calls at this case, nothing else")
    ap.add_argument("--kernel-stats", default=None, metavar="DB", help="append the profiler's rows for the two kernels to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgp_zgrad_bench.txt"))
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats, a.out)
        return
    import egobox_amd as egx
    from egobox_amd import sgp as SG

    if egx._lib.load().egx_device_count() < 1:
        sys.exit("sgp_zgrad_bench: needs a GPU")
    if a.trace_only:
        n, nz, d = (int(v) for v in a.trace_only.split(","))
        x, y, z = problem(n, nz, d, seed=n)
        with SG.SgpHandle(x, y, z, corr=0, method=SG.FITC) as h:
            for _ in range(3):
                h.likelihood_grad_z(np.full(d, 0.7), float(np.var(y, ddof=1)), 1e-2)
        return
    lines = [f"sparse GP likelihood gradient in the inducing points; {a.rounds} rounds after {a.warmup} warm-up rounds, ms = median"]
    for case in a.cases:
        n, nz, d = (int(v) for v in case.split(","))
        x, y, z = problem(n, nz, d, seed=n)
        theta, sigma2, noise = np.full(d, 0.7), float(np.var(y, ddof=1)), 1e-2
        with SG.SgpHandle(x, y, z, corr=0, method=SG.FITC) as h:
            legs = (lambda: h.likelihood_grad(theta, sigma2, noise), lambda: h.likelihood_grad_z(theta, sigma2, noise),
                    lambda: h.likelihood_grad(theta, sigma2, noise))
            t = [[], [], []]
            for r in range(a.warmup + a.rounds):
                for k, leg in enumerate(legs):
                    ms, _ = timed(leg)
                    if r >= a.warmup:
                        t[k].append(ms)
            ga, gz, gb = (float(np.median(v)) for v in t)
            lines.append(f"n {n} nz {nz} d {d} FITC: likelihood_grad {ga:.2f} / {gb:.2f} ms (two legs), likelihood_grad_z {gz:.2f} ms, "
                         f"difference {gz - 0.5 * (ga + gb):.2f} ms, ratio {gz / (0.5 * (ga + gb)):.3f}")
            print(lines[-1], flush=True)
    if not a.no_fit:
        n, nt, nz, d = 20000, 5000, 64, 4
        rng = np.random.default_rng(20000)
        x, xt = rng.random((n, d)) * 10 - 5, rng.random((nt, d)) * 10 - 5
        y, yt = griewank(x), griewank(xt)
        z = x[rng.permutation(n)[:nz]].copy()
        s20 = float(np.var(y, ddof=1))
        p0 = np.array([[1.0] * d + [s20, SG.DEFAULT_NOISE_INIT]])
        bounds = [SG.DEFAULT_THETA_BOUNDS] * d + [(1e-12, 9.0 * s20), SG.DEFAULT_NOISE_BOUNDS]
        lo, hi = [b[0] for b in bounds], [b[1] for b in bounds]
        lines.append(f"Griewank on [-5, 5]^{d}, n {n}, nz {nz} (a draw of rows), Matern-5/2, one start; RMSE on {nt} held-out points")
        for method, mname in ((SG.FITC, "FITC"), (SG.VFE, "VFE")):
            for oname, fit in (("fit_lbfgs", lambda h: h.fit_lbfgs(p0, lo, hi, True, 1e-2, 50)),
                               ("fit_lbfgs_z", lambda h: h.fit_lbfgs_z(p0, lo, hi, True, 1e-2, 50, max_iter_z=50))):
                with SG.SgpHandle(x, y, z, corr=3, method=method) as h:
                    ms, ne = timed(lambda: fit(h))
                    st = h.state()
                    rmse = float(np.sqrt(np.mean((h.predict(xt) - yt) ** 2)))
                    moved = float(np.abs(h.inducings() - z).max())
                lines.append(f"  {mname} {oname}: likelihood {st['likelihood']:.6g}, held-out RMSE {rmse:.5f}, {ne} evaluations, "
                             f"{ms / 1e3:.2f} s, noise {st['noise']:.3e}, largest move of a coordinate {moved:.3f}")
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
