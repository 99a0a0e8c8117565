#!/usr/bin/env python3
"""Sparse GP on one GPU: what the closed-form likelihood gradient costs and what a fit on it saves.  GPU only.
At (n, nz, d) = (10^6, 512, 8) and (10^5, 256, 8), squared exponential, FITC and VFE:
  1. median wall time (host clock around calls that end in a device synchronise) of `likelihood` and of `likelihood_grad` at
     fixed parameters: 15 rounds after 3 warm-up rounds, the legs of a round alternated (likelihood, likelihood_grad,
     likelihood), so `likelihood` is timed twice -- the distance between its two medians is the spread to read the ratio with;
  2. a tuned fit from the same 4 starts (the start of SgpParams.fit and 3 Latin-hypercube starts) by COBYLA (egx_sgp_fit) and
     by L-BFGS (egx_sgp_fit_lbfgs): evaluations, wall time, final likelihood.
Writes the table to --out (default profiles/sgp_grad_bench.txt).
    python tools/sgp_grad_bench.py [--cases n,nz,d ...] [--rounds R] [--out FILE]"""
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


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["1000000,512,8", "100000,256,8"])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgp_grad_bench.txt"))
    a = ap.parse_args()
    import egobox_amd as egx
    from egobox_amd import sgp as SG
    from egobox_amd.multistart import prepare_multistart

    if egx._lib.load().egx_device_count() < 1:
        sys.exit("sgp_grad_bench: needs a GPU")
    lines = [f"sparse GP likelihood gradient, squared exponential; {a.rounds} rounds after {a.warmup} warm-up rounds, ms = median"]
    for case in a.cases:
        n, nz, d = (int(v) for v in case.split(","))
        x, y, z = problem(n, nz, d, seed=n)
        theta, sigma2, noise = np.full(d, 0.7), float(np.var(y, ddof=1)), 1e-2
        s20 = sigma2
        p0 = np.array([1.0] * d + [s20, SG.DEFAULT_NOISE_INIT])
        bounds = [SG.DEFAULT_THETA_BOUNDS] * d + [(1e-12, 9.0 * s20), SG.DEFAULT_NOISE_BOUNDS]
        lo, hi = [b[0] for b in bounds], [b[1] for b in bounds]
        starts = 10.0 ** prepare_multistart(3, p0, bounds, seed=42)[0]
        for method, mname in ((SG.FITC, "FITC"), (SG.VFE, "VFE")):
            with SG.SgpHandle(x, y, z, corr=0, method=method) as h:
                legs = (lambda: h.likelihood(theta, sigma2, noise), lambda: h.likelihood_grad(theta, sigma2, noise),
                        lambda: h.likelihood(theta, sigma2, noise))
                t = [[], [], []]
                for r in range(a.warmup + a.rounds):
                    for k, leg in enumerate(legs):
                        ms, _ = timed(leg)
                        if r >= a.warmup:
                            t[k].append(ms)
                la, lg, lb = (float(np.median(v)) for v in t)
                lines.append(f"n {n} nz {nz} d {d} {mname}: likelihood {la:.2f} / {lb:.2f} ms (two legs), likelihood_grad {lg:.2f} ms, "
                             f"ratio {lg / (0.5 * (la + lb)):.2f}")
                print(lines[-1], flush=True)
                for oname, fit in (("COBYLA", lambda: h.fit(starts, lo, hi, True, 1e-2, 1000)),
                                   ("L-BFGS", lambda: h.fit_lbfgs(starts, lo, hi, True, 1e-2, 50))):
                    ms, ne = timed(fit)
                    st = h.state()
                    lines.append(f"n {n} nz {nz} d {d} {mname} fit, 4 starts, {oname}: {ne} evaluations, {ms / 1e3:.2f} s, likelihood "
                                 f"{st['likelihood']:.6g}, noise {st['noise']:.3e}")
                    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
