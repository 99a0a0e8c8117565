"""Times the PLS rotations on the device against the host NIPALS (egobox_amd/kpls.py) and writes profiles/pls_bench.txt.
Not part of bench.py.

    python tools/pls_bench.py [--out profiles/pls_bench.txt] [--reps 5]

Per case (n, d, k):
  compute_w_star   egx_sgp_compute_w_star on a sparse handle that holds the training set (no upload): host clock, the call
                   synchronises
  pls_rotations    egx_pls_rotations from host data (upload, transpose on the device, the same launches)
  launches         the launches of compute_w_star alone (means, centred Gram, chunk-order sum) between two HIP events
                   (egx_sgp_pls_launch_ms)
  host             kpls.pls_rotations in the same process
and two yardsticks: the host function, and the time of two reads of X at the device-to-device copy bandwidth this script measures
(a copy of X reads and writes it once: two passes over its bytes).  Every figure is the median of --reps runs after one warm-up.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPARSE_CASES = [(10 ** 6, 64, 4), (10 ** 5, 32, 4)]
DENSE_CASE = (4096, 124, 4)


def _median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def _copy_bandwidth(nbytes, reps):
    """bytes / s moved by a device-to-device copy of nbytes (read + write), by device events"""
    import torch
    a = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    del a, b
    return 2.0 * nbytes / (statistics.median(ts) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pls_bench.txt"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/pls_bench.py needs a GPU: a CPU run measures nothing")
    import egobox_amd as egx
    from egobox_amd import _lib as L
    from egobox_amd import kpls
    lib = L.load()
    lines = [f"PLS rotations, device against host; {torch.cuda.get_device_name(0)}; medians of {args.reps} runs after a warm-up "
             f"(min .. max in brackets), ms", ""]

    def case(n, d, k, nz):
        rng = np.random.default_rng(n + d)
        x = rng.random((n, d))
        y = np.sin(3.0 * x[:, 0]) + x @ rng.standard_normal(d) + 0.05 * rng.standard_normal(n)
        plan = kpls.pls_plan(n, d)
        xbytes = 8 * n * d
        bw = _copy_bandwidth(max(xbytes, 1 << 26), args.reps)
        two_reads_ms = 2.0 * xbytes / bw * 1e3
        host = _median_ms(lambda: kpls.pls_rotations(x, y, k), max(2, args.reps // 2))
        rot = _median_ms(lambda: kpls.pls_rotations_device(x, y, k), args.reps)
        with egx.SgpHandle(x, y, x[:nz].copy(), corr=0) as h:
            cws = _median_ms(lambda: h.compute_w_star(k), args.reps)
            ms = C.c_double()

            def launches():
                L.check(lib.egx_sgp_pls_launch_ms(h._h, C.byref(ms)))
                return ms.value
            launches()
            ev = sorted(launches() for _ in range(args.reps))
            w_dev = h.w_star()
        w_host = kpls.pls_rotations(x, y, k)
        diff = max(min(np.max(np.abs(w_dev[:, j] - w_host[:, j])), np.max(np.abs(w_dev[:, j] + w_host[:, j])))
                   / np.max(np.abs(w_host[:, j])) for j in range(k))
        lev = ev[len(ev) // 2]
        lines.extend([
            f"n = {n}, d = {d}, k = {k}  (plan: {plan['n_chunks']} chunks of {plan['chunk_rows']} rows, {plan['blocks']} blocks, "
            f"{plan['out_tiles']} tiles; X = {xbytes / 1e6:.1f} MB; copy bandwidth {bw / 1e12:.2f} TB/s)",
            f"  egx_sgp_compute_w_star   {cws[0]:10.3f}  [{cws[1]:.3f} .. {cws[2]:.3f}]",
            f"  egx_pls_rotations        {rot[0]:10.3f}  [{rot[1]:.3f} .. {rot[2]:.3f}]",
            f"  launches alone (events)  {lev:10.3f}  [{ev[0]:.3f} .. {ev[-1]:.3f}]",
            f"  kpls.pls_rotations (host){host[0]:10.3f}  [{host[1]:.3f} .. {host[2]:.3f}]",
            f"  two reads of X at the copy bandwidth {two_reads_ms:.3f}",
            f"  host / compute_w_star {host[0] / cws[0]:.1f}x   host / egx_pls_rotations {host[0] / rot[0]:.1f}x   "
            f"launches / two reads of X {lev / two_reads_ms:.2f}x",
            f"  device against host rotations, sign-insensitive column error {diff:.2e}",
            ""])
        print("\n".join(lines[-10:]), flush=True)

    for n, d, k in SPARSE_CASES:
        case(n, d, k, nz=64)
    n, d, k = DENSE_CASE
    lines.append("dense model's shape (egx_pls_rotations is what GpParams.pls('device') calls; the handle figures are for comparison)")
    case(n, d, k, nz=16)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
