#!/usr/bin/env python3
"""Sparse GP with KPLS weights on one GPU, beside the same calls without weights, in one process.  GPU only.
At n in {10^5, 10^6}, nz = 512, d = 64, h = 4, squared exponential and Matern-5/2, FITC:
  1. the host time of the PLS rotations (egobox_amd/kpls.py);
  2. median wall time (host clock around calls that end in a device synchronise) of `likelihood`, `likelihood_grad` and
     `likelihood_grad_z` at fixed parameters, with weights (theta has h components) and without (d components);
  3. a fit from the same 4 starts (the start of SgpParams.fit and 3 Latin-hypercube starts) by COBYLA (egx_sgp_fit) and by L-BFGS
     (egx_sgp_fit_lbfgs), with weights (h + 2 parameters) and without (d + 2): evaluations, wall time, final likelihood.
Under a Matern correlation the weights make the coefficient table d x h (hcols = h): every pair costs h factors per input, in the
correlation kernels and in the two gradient kernels; the last column of (2) is that cost.  One (n, correlation) per invocation
keeps a run short; --append adds to --out (default profiles/sgp_kpls_bench.txt) instead of replacing it.
    python tools/sgp_kpls_bench.py [--n N ...] [--corr 0 3] [--nz 512] [--d 64] [--h 4] [--rounds R] [--no-fit] [--append] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CORR_NAMES = ["squared exponential", "absolute exponential", "Matern-3/2", "Matern-5/2"]


def problem(n, nz, d, seed):
    """A response that lives on two directions of the d inputs: what KPLS is for."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, d)) * 2 - 1
    u1, u2 = rng.standard_normal(d), rng.standard_normal(d)
    u1, u2 = u1 / np.linalg.norm(u1), u2 / np.linalg.norm(u2)
    y = np.sin(3 * x.dot(u1)) + 0.5 * np.cos(2 * x.dot(u2)) + 0.05 * rng.standard_normal(n)
    z = x[rng.permutation(n)[:nz]].copy()
    return x, y, z


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", nargs="*", type=int, default=[100000, 1000000])
    ap.add_argument("--corr", nargs="*", type=int, default=[0, 3])
    ap.add_argument("--nz", type=int, default=512)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--h", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-eval", type=int, default=200, help="COBYLA's cap per start (its budget is clamp(10 thetas, 25, cap))")
    ap.add_argument("--max-iter", type=int, default=30, help="L-BFGS iterations per start")
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgp_kpls_bench.txt"))
    a = ap.parse_args()
    import egobox_amd as egx
    from egobox_amd import kpls
    from egobox_amd import sgp as SG
    from egobox_amd.multistart import prepare_multistart

    if egx._lib.load().egx_device_count() < 1:
        sys.exit("sgp_kpls_bench: needs a GPU")
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    for n in a.n:
        x, y, z = problem(n, a.nz, a.d, seed=n)
        pls_ms, w = timed(lambda: kpls.pls_rotations(x, y, a.h))
        say(f"n {n} nz {a.nz} d {a.d} h {a.h}: host PLS rotations {pls_ms:.1f} ms; {a.rounds} rounds after {a.warmup} warm-up rounds, "
            f"ms = median")
        s20 = float(np.var(y, ddof=1))
        for corr in a.corr:
            med = {}
            for tag, ws, nt in (("KPLS", w, a.h), ("no weights", None, a.d)):
                # fixed parameters at which a typical correlation is a few tenths (the exponent sums d or d x h terms)
                scale = (1.0 if ws is not None else 0.2) if corr == 0 else (0.08 if ws is not None else 0.03)
                theta = np.full(nt, scale * np.sqrt(64.0 / a.d))
                p0 = np.array([1.0 if ws is not None else 0.1] * nt + [s20, SG.DEFAULT_NOISE_INIT])
                bounds = [SG.DEFAULT_THETA_BOUNDS] * nt + [(1e-12, 9.0 * s20), SG.DEFAULT_NOISE_BOUNDS]
                lo, hi = [b[0] for b in bounds], [b[1] for b in bounds]
                starts = 10.0 ** prepare_multistart(3, p0, bounds, seed=42)[0]
                with SG.SgpHandle(x, y, z, corr=corr, method=SG.FITC, w_star=ws) as h:
                    legs = (lambda: h.likelihood(theta, s20, 1e-2), lambda: h.likelihood_grad(theta, s20, 1e-2),
                            lambda: h.likelihood_grad_z(theta, s20, 1e-2))
                    t = [[], [], []]
                    for r in range(a.warmup + a.rounds):
                        for k, leg in enumerate(legs):
                            ms, out = timed(leg)
                            if out[-1] != 0:
                                sys.exit(f"sgp_kpls_bench: status {out[-1]} at the fixed parameters ({tag}, corr {corr})")
                            if r >= a.warmup:
                                t[k].append(ms)
                    med[tag] = [float(np.median(v)) for v in t]
                    ll, lg, lz = med[tag]
                    say(f"n {n} {CORR_NAMES[corr]} FITC, {tag} ({nt} thetas): likelihood {ll:.2f} ms, likelihood_grad {lg:.2f} ms, "
                        f"likelihood_grad_z {lz:.2f} ms; gradient kernels alone (grad - likelihood) {lg - ll:.2f} ms, "
                        f"(grad_z - grad) {lz - lg:.2f} ms")
                    if a.no_fit:
                        continue
                    for oname, fit in (("COBYLA", lambda: h.fit(starts, lo, hi, True, 1e-2, a.max_eval)),
                                       ("L-BFGS", lambda: h.fit_lbfgs(starts, lo, hi, True, 1e-2, a.max_iter))):
                        ms, ne = timed(fit)
                        st = h.state()
                        say(f"n {n} {CORR_NAMES[corr]} FITC, {tag} fit of {nt + 2} parameters, 4 starts, {oname}: {ne} evaluations, "
                            f"{ms / 1e3:.2f} s, likelihood {st['likelihood']:.6g}, noise {st['noise']:.3e}")
            k, p = med["KPLS"], med["no weights"]
            say(f"n {n} {CORR_NAMES[corr]}: KPLS / no weights = likelihood {k[0] / p[0]:.2f}, likelihood_grad {k[1] / p[1]:.2f}, "
                f"likelihood_grad_z {k[2] / p[2]:.2f}; gradient kernels alone {(k[1] - k[0]) / (p[1] - p[0]):.2f}, "
                f"{(k[2] - k[1]) / (p[2] - p[1]):.2f} (h = {a.h})")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
