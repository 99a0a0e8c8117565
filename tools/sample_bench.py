#!/usr/bin/env python3
"""Posterior covariance and trajectory sampling on one GPU (egx_gp_predict_covariance / egx_gp_sample): wall time per call for
n in {2048, 8192} training points, m in {512, 4096} query points, n_traj in {10, 1000}, d = 8, with predict and predict_var on
the same points as the yardsticks of the shared solve.  Phases by difference of calls:
    solve      predict_var                            (cross correlation + triangular solve + row reductions)
    rest       sample - predict - predict_var         (u, the Gram GEMMs, the assembly, tau, the m x m Cholesky, the normals,
                                                       the triangular product; sample downloads m x n_traj, not m x m)
predict_covariance also pays the download of its m x m result to pageable host memory.  The Gram GEMM and the triangular
product are split out by `rocprofv3 --kernel-trace --stats` (k_gemm_stream / k_gemm_nt_sub, k_trmm_mean).  One JSON line per
case, then a summary line.
    python tools/sample_bench.py [--reps R] [--cases n,m,n_traj ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egobox_amd as egx  # noqa: E402

PEAK_TFLOPS = 78.6  # FP64 (MFMA) peak of one MI355X


def best_of(fn, reps):
    fn()  # warm: allocations, first launches
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", nargs="*", default=None, help="n,m,n_traj triples (default: the 8-case grid)")
    ap.add_argument("--method", default="psd", choices=("psd", "cholesky"))
    a = ap.parse_args()
    cases = [tuple(int(v) for v in c.split(",")) for c in a.cases] if a.cases else \
        [(n, m, t) for n in (2048, 8192) for m in (512, 4096) for t in (10, 1000)]
    d = 8
    rows = []
    handles = {}
    for n, m, nt in cases:
        if n not in handles:
            x, y = egx.workload.make_training_set(n, d, 42)
            h = egx.GpHandle(x, y)
            h.finalize(egx.workload.default_theta(d))
            handles[n] = h
        h = handles[n]
        xq = np.random.default_rng(m).random((m, d)) * 1.4 - 0.2
        r = {"n": n, "m": m, "n_traj": nt, "d": d, "method": a.method}
        r["predict_ms"] = best_of(lambda: h.predict(xq), a.reps)
        r["predict_var_ms"] = best_of(lambda: h.predict_var(xq), a.reps)
        r["covariance_ms"] = best_of(lambda: h.predict_covariance(xq), a.reps)
        taus = []
        r["sample_ms"] = best_of(lambda: taus.append(h.sample(xq, nt, method=a.method, seed=1, return_tau=True)[1]), a.reps)
        r["tau"] = taus[-1]
        r["phase_solve_ms"] = r["predict_var_ms"]
        r["phase_rest_ms"] = r["sample_ms"] - r["predict_ms"] - r["predict_var_ms"]
        r["sample_over_predict_var"] = r["sample_ms"] / r["predict_var_ms"]
        m_pad = -(-m // 128) * 128
        r["gram_gflop"] = m_pad * m_pad * (-(-n // 128) * 128) / 1e9  # lower tiles of RT RT^T (2 flop per MAC, half the tiles)
        r["trmm_gflop"] = m_pad * m_pad * (-(-nt // 64) * 64) / 1e9   # lower half of L Z
        r["solve_gflop"] = m_pad * (-(-n // 128) * 128) ** 2 / 1e9
        rows.append(r)
        print(json.dumps(r), flush=True)
    for h in handles.values():
        h.close()
    print(json.dumps({"summary": "sample_bench", "cases": len(rows), "peak_tflops": PEAK_TFLOPS}), flush=True)


if __name__ == "__main__":
    main()
