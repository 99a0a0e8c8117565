#!/usr/bin/env python3
"""What the fused cast of a mixed-integer model costs, one JSON line per leg:
  (a) predict of m = 100 000 points, d = 16, n = 8192: untyped, typed (egx_gp_set_xtypes: the cast inside k_normalize_queries),
      and for contrast (c) a host egx_mixint_cast followed by the untyped call
  (b) the few-query path: egx_infill_eval with gradient at ONE point, untyped and typed (the cast inside k_infill_prepare)
`reps` timed repetitions after one warm-up each; median, minimum, maximum and the spread (max - min) / median.
    python tools/mixint_bench.py [--library PATH] [--reps 10] [--n 8192] [--m 100000]
--library: another build of libegx_gp_hip.so, e.g. the parent commit's, for its own run-to-run spread; a build without the
mixint symbols runs the untyped legs only.  The binding below is a minimal one of its own so that any build can be measured by
the same harness.  `--trace` runs ONE typed or untyped predict and one infill evaluation and nothing else: the workload of a
`rocprofv3 --kernel-trace --stats -- python tools/mixint_bench.py --trace typed` run, whose launch counts must be equal."""
import argparse
import ctypes as C
import json
import os
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)


class GpConfig(C.Structure):
    _fields_ = [("corr", C.c_int32), ("mean", C.c_int32), ("nugget", C.c_double), ("device", C.c_int32),
                ("n_workspaces", C.c_int32), ("w_star", DP), ("kpls_dim", C.c_int64)]


class InfillConfig(C.Structure):
    _fields_ = [("criterion", C.c_int32), ("feasibility", C.c_int32), ("fmin", C.c_double), ("sigma_weight", C.c_double),
                ("scale_ic", C.c_double), ("scale", C.c_double)]


class XTypeC(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n", C.c_int32), ("lo", C.c_double), ("hi", C.c_double), ("values", DP)]


def dp(a):
    return a.ctypes.data_as(DP)


def check(lib, rc):
    if rc:
        lib.egx_last_error.restype = C.c_char_p
        raise RuntimeError(f"rc {rc}: {lib.egx_last_error().decode()}")


def spec16():
    """d = 16: Int, 9 Float, Enum(4), Ord of 6 values, Int"""
    ordv = np.array([-1.0, -0.5, 0.0, 0.25, 0.5, 1.0])
    cols = [(1, 0, -4.0, 4.0, None)] + [(0, 0, -1.0, 1.0, None)] * 9 + [(3, 4, 0.0, 0.0, None), (2, 6, 0.0, 0.0, ordv), (1, 0, -3.0, 3.0, None)]
    arr = (XTypeC * len(cols))()
    for c, (kind, n, lo, hi, v) in zip(arr, cols):
        c.kind, c.n, c.lo, c.hi = kind, n, lo, hi
        if v is not None:
            c.values = dp(v)
    lim = np.array([[-4, 4]] + [[-1, 1]] * 9 + [[0, 1]] * 4 + [[-1, 1], [-3, 3]], dtype=np.float64)
    return arr, len(cols), lim, ordv


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    med = float(np.median(ts))
    return dict(median_ms=round(med, 4), min_ms=round(float(ts.min()), 4), max_ms=round(float(ts.max()), 4),
                spread=round(float((ts.max() - ts.min()) / med), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=os.path.join(ROOT, "egobox_amd", "lib", "libegx_gp_hip.so"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=100000)
    ap.add_argument("--trace", choices=["typed", "untyped"])
    a = ap.parse_args()
    lib = C.CDLL(a.library)
    has_mixint = hasattr(lib, "egx_gp_set_xtypes")
    arr, nx, lim, _keep = spec16()
    d = lim.shape[0]
    rng = np.random.default_rng(1)
    x = lim[:, 0] + (lim[:, 1] - lim[:, 0]) * rng.random((a.n, d))
    x[:, 0], x[:, -1] = np.round(x[:, 0]), np.round(x[:, -1])  # (the Enum columns stay relaxed: a well-conditioned training set)
    y = np.sin(x @ np.cos(np.arange(d))) + 0.1 * x[:, 1] ** 2
    cfg = GpConfig(0, 0, 100 * np.finfo(float).eps, -1, 1, None, 0)
    gp, gc = C.c_void_p(), C.c_void_p()
    check(lib, lib.egx_gp_create(C.byref(cfg), dp(x), dp(y), C.c_int64(a.n), C.c_int64(d), C.byref(gp)))
    check(lib, lib.egx_gp_create(C.byref(cfg), dp(x), dp(np.ascontiguousarray(y - 0.3)), C.c_int64(a.n), C.c_int64(d), C.byref(gc)))
    theta = np.full(d, 0.08)
    for g in (gp, gc):
        check(lib, lib.egx_gp_finalize(g, dp(theta), C.c_int64(d)))
    xq = np.ascontiguousarray(lim[:, 0] + (lim[:, 1] - lim[:, 0]) * rng.random((a.m, d)))
    out, xc = np.empty(a.m), np.empty_like(xq)
    icfg = InfillConfig(2, 1, float(np.quantile(y, 0.1)), 1.0, 1.0, 1.0)
    inf, tol, carr = C.c_void_p(), np.array([0.0]), (C.c_void_p * 1)(gc.value)
    check(lib, lib.egx_infill_create(C.byref(icfg), gp, carr, dp(tol), 1, C.byref(inf)))
    x1, v1, g1 = np.ascontiguousarray(xq[:1]), np.empty(1), np.empty((1, d))

    def predict():
        check(lib, lib.egx_gp_predict(gp, dp(xq), C.c_int64(a.m), dp(out)))

    def host_cast_predict():
        check(lib, lib.egx_mixint_cast(arr, nx, dp(xq), C.c_int64(a.m), dp(xc)))
        check(lib, lib.egx_gp_predict(gp, dp(xc), C.c_int64(a.m), dp(out)))

    def point():
        check(lib, lib.egx_infill_eval(inf, dp(x1), C.c_int64(1), dp(v1), dp(g1), None))

    def typed(on):
        for g in (gp, gc):
            check(lib, lib.egx_gp_set_xtypes(g, arr if on else None, nx if on else 0))

    if a.trace:
        typed(a.trace == "typed")
        predict()
        point()
        return
    shape = dict(n=a.n, m=a.m, d=d, reps=a.reps, library=os.path.relpath(a.library, ROOT))
    print(json.dumps(dict(leg="a_predict_untyped", **shape, **timed(predict, a.reps))), flush=True)
    print(json.dumps(dict(leg="b_point_untyped", **shape, **timed(point, a.reps * 20))), flush=True)
    if not has_mixint:
        return
    ref = out.copy()
    print(json.dumps(dict(leg="c_host_cast_then_untyped", **shape, **timed(host_cast_predict, a.reps))), flush=True)
    on_cast = out.copy()
    typed(True)
    print(json.dumps(dict(leg="a_predict_typed", **shape, **timed(predict, a.reps))), flush=True)
    assert np.array_equal(out, on_cast) and not np.array_equal(out, ref)
    print(json.dumps(dict(leg="b_point_typed", **shape, **timed(point, a.reps * 20))), flush=True)
    typed(False)
    print(json.dumps(dict(leg="a_predict_untyped_again", **shape, **timed(predict, a.reps))), flush=True)


if __name__ == "__main__":
    main()
