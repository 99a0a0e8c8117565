#!/usr/bin/env python3
"""Sparse-GP surrogate calls on one GPU: wall time per call (host clock around calls that end in a device synchronise) for
n = 100 000 training points, nz in {512, 2048} inducing points, d in {8, 32}, Matern-5/2, FITC, fixed parameters.
Per (nz, d), after one warm-up call, median and interquartile range of the repeats:
    valvar_grad_1      egx_sgp_predict_valvar_gradients, m = 1        (ms)
    valvar_1           egx_sgp_predict_valvar, m = 1                  (ms)
    valvar_grad_batch  egx_sgp_predict_valvar_gradients, m = 65536    (ms and points/s)
    sample             egx_sgp_sample, m = 4096, 1000 trajectories    (ms)
(`--small-m M ...` adds the first of these at other small batch sizes) and the same quantities through what the library offered
before those entry points (`--what old`; works on any build of the library, `--lib PATH`): egx_sgp_predict + egx_sgp_predict_var, on the 2 d times shifted batch for the gradients (the central
differences of SparseGaussianProcess._central_diff).  A cell whose single call takes longer than --slow-s seconds is repeated
--slow-reps times instead of --reps (its row says so).  One JSON line per cell; `--against FILE` adds the ratio old / new to
every new cell that has an old counterpart in FILE (a run of this tool with --what old on the same machine).
    python tools/sgp_predict_bench.py [--what new|old|both] [--lib PATH] [--cases nz,d ...] [--reps R] [--against old.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)


class SgpConfig(C.Structure):
    _fields_ = [("corr", C.c_int32), ("method", C.c_int32), ("nugget", C.c_double), ("device", C.c_int32)]


def dp(a):
    return a.ctypes.data_as(DP)


class Model:
    def __init__(self, lib, x, y, z, theta, sigma2, noise):
        self.lib, self.d = lib, x.shape[1]
        cfg = SgpConfig()
        lib.egx_sgp_config_default(C.byref(cfg))
        cfg.corr, cfg.method = 3, 0
        self.h = C.c_void_p()
        lib.egx_last_error.restype = C.c_char_p
        self.check(lib.egx_sgp_create(C.byref(cfg), dp(x), dp(y), C.c_int64(x.shape[0]), C.c_int64(x.shape[1]), dp(z),
                                      C.c_int64(z.shape[0]), C.byref(self.h)))
        self.check(lib.egx_sgp_finalize(self.h, dp(theta), C.c_int64(theta.size), C.c_double(sigma2), C.c_double(noise)))

    def check(self, rc):
        if rc:
            raise RuntimeError(f"rc {rc}: {self.lib.egx_last_error().decode()}")

    def call(self, name, xq, *outs):
        self.check(getattr(self.lib, name)(self.h, dp(xq), C.c_int64(xq.shape[0]), *[dp(o) for o in outs]))

    def old_valvar(self, xq):
        y, v = np.empty(xq.shape[0]), np.empty(xq.shape[0])
        self.call("egx_sgp_predict", xq, y)
        self.call("egx_sgp_predict_var", xq, v)
        return y, v

    def old_valvar_grad(self, xq):
        m, nx = xq.shape
        h = float(np.sqrt(np.finfo(float).eps))
        shifted = np.repeat(xq[None, :, :], 2 * nx, axis=0)
        for k in range(nx):
            shifted[2 * k, :, k] += h
            shifted[2 * k + 1, :, k] -= h
        y, v = self.old_valvar(np.ascontiguousarray(shifted.reshape(-1, nx)))
        y, v = y.reshape(2 * nx, m), v.reshape(2 * nx, m)
        return ((y[0::2] - y[1::2]) / (2 * h)).T.copy(), ((v[0::2] - v[1::2]) / (2 * h)).T.copy()

    def new_valvar(self, xq):
        y, v = np.empty(xq.shape[0]), np.empty(xq.shape[0])
        self.call("egx_sgp_predict_valvar", xq, y, v)
        return y, v

    def new_valvar_grad(self, xq):
        gy, gv = np.empty(xq.shape), np.empty(xq.shape)
        self.call("egx_sgp_predict_valvar_gradients", xq, gy, gv)
        return gy, gv

    def new_sample(self, xq, nt):
        t, tau = np.empty((xq.shape[0], nt)), C.c_double()
        self.check(self.lib.egx_sgp_sample(self.h, dp(xq), C.c_int64(xq.shape[0]), C.c_int64(nt), C.c_int32(1), C.c_uint64(1),
                                           None, dp(t), C.byref(tau)))
        return t

    def close(self):
        self.lib.egx_sgp_destroy(self.h)


def timed(fn, a):
    fn()  # warm-up: allocations, first launches, cached state
    t0 = time.perf_counter()
    fn()
    first = time.perf_counter() - t0
    reps = a.slow_reps if first > a.slow_s else a.reps
    ts = [first] if first > a.slow_s else []
    while len(ts) < reps:
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    q1, med, q3 = np.percentile(np.array(ts) * 1e3, [25, 50, 75])
    return {"ms": med, "iqr_ms": q3 - q1, "repeats": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="both", choices=("new", "old", "both"))
    ap.add_argument("--lib", default=os.path.join(ROOT, "egobox_amd", "lib", "libegx_gp_hip.so"))
    ap.add_argument("--cases", nargs="*", default=None, help="nz,d pairs (default: 512,8 512,32 2048,8 2048,32)")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slow-s", type=float, default=1.0)
    ap.add_argument("--slow-reps", type=int, default=3)
    ap.add_argument("--only", nargs="*", default=None, help="cells to run (names above)")
    ap.add_argument("--small-m", nargs="*", type=int, default=[],
                    help="extra cells valvar_grad_m<M>: egx_sgp_predict_valvar_gradients at these batch sizes (the few-query "
                         "route against the batched one: builds with -DEGX_SGP_POINT_MAX=0 / =16 via --lib)")
    ap.add_argument("--against", default=None)
    a = ap.parse_args()
    lib = C.CDLL(a.lib)
    cases = [tuple(int(v) for v in c.split(",")) for c in a.cases] if a.cases else [(512, 8), (512, 32), (2048, 8), (2048, 32)]
    old = {}
    if a.against:
        for line in open(a.against):
            r = json.loads(line)
            if r.get("what") == "old":
                old[(r["nz"], r["d"], r["cell"])] = r
    for nz, d in cases:
        rng = np.random.default_rng(nz + d)
        x = rng.random((a.n, d)) * 2 - 1
        y = np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, -1]) + 0.05 * rng.standard_normal(a.n)
        z = x[rng.permutation(a.n)[:nz]].copy()
        mdl = Model(lib, x, y, z, np.full(d, 2.0 / np.sqrt(d)), 1.0, 0.01)
        x1 = rng.random((1, d)) * 2 - 1
        xb = rng.random((a.batch, d)) * 2 - 1
        xs = rng.random((4096, d)) * 2 - 1
        cells = []
        if a.what in ("new", "both"):
            cells += [("new", "valvar_grad_1", lambda: mdl.new_valvar_grad(x1), 1), ("new", "valvar_1", lambda: mdl.new_valvar(x1), 1),
                      ("new", "valvar_grad_batch", lambda: mdl.new_valvar_grad(xb), a.batch),
                      ("new", "sample", lambda: mdl.new_sample(xs, 1000), 4096)]
            for ms in a.small_m:
                xm = np.ascontiguousarray(xb[:ms])
                cells.append(("new", f"valvar_grad_m{ms}", (lambda q: lambda: mdl.new_valvar_grad(q))(xm), ms))
        if a.what in ("old", "both"):
            cells += [("old", "valvar_grad_1", lambda: mdl.old_valvar_grad(x1), 1), ("old", "valvar_1", lambda: mdl.old_valvar(x1), 1),
                      ("old", "valvar_grad_batch", lambda: mdl.old_valvar_grad(xb), a.batch)]
        for what, cell, fn, m in cells:
            if a.only and cell not in a.only:
                continue
            r = {"what": what, "cell": cell, "n": a.n, "nz": nz, "d": d, "m": m, "lib": os.path.relpath(a.lib, ROOT)}
            r.update(timed(fn, a))
            r["points_per_s"] = m / (r["ms"] * 1e-3)
            o = old.get((nz, d, cell))
            if what == "new" and o:
                r["old_ms"], r["old_iqr_ms"], r["old_over_new"] = o["ms"], o["iqr_ms"], o["ms"] / r["ms"]
            print(json.dumps(r), flush=True)
        mdl.close()


if __name__ == "__main__":
    main()
