"""PLS rotations without a GPU: csrc/pls_host.h (the launch plan and the d-space recursion) as the stand-alone program
tests/c_host/pls_host_test.cpp, plain and under the address and undefined-behaviour sanitizers; the oracle's own three forms on
every row of the case list; egx_pls_get_plan; the argument checks of the C ABI, which come before any device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pls_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "pls_host_test.cpp")


def _plan(n, d):
    from egobox_amd import kpls
    return kpls.pls_plan(n, d)


@pytest.fixture(scope="module")
def rows():
    """(name, n, d, k, x, y, the long-double rotations, e_host, e_gram) per row of the case list, computed once"""
    return [(name, n, d, k, x, y, ref, eh, eg) for name, n, d, k, kind, x, y, ref, eh, eg in PO.rows(_plan)]


def test_the_rows_are_well_posed(rows):
    """The long-double NIPALS, the package's float64 NIPALS and the float64 Gram form agree on every row: the Gram form under
    the rule itself against the host path, and both far below what a wrong tile or a dropped row would leave (1e-6)."""
    for name, n, d, k, x, y, ref, e_host, e_gram in rows:
        print(f"{name}: n {n} d {d} k {k} e_host {e_host:.3e} e_gram {e_gram:.3e}")
        assert np.all(np.isfinite(ref)) and np.max(np.abs(ref)) > 0.0, name
        assert e_host < 1e-6 and e_gram < 1e-6, (name, e_host, e_gram)
        assert e_gram <= PO.FACTOR * max(e_host, PO.FLOOR), (name, e_host, e_gram)


def _build(tmp_path, sanitize):
    exe = tmp_path / ("pls_host_test_san" if sanitize else "pls_host_test")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, SRC, "-o", str(exe)], check=True)
    return exe


def _run_cases(exe, tmp_path, rows):
    blob = [np.array([float(len(rows))])]
    for name, n, d, k, x, y, ref, e_host, e_gram in rows:
        g, s, yty = PO.gram_inputs(x, y)
        blob += [np.array([float(n), float(d), float(k)]), g.reshape(-1), s, np.array([yty]), ref.reshape(-1)]
    path = tmp_path / "cases.f64"
    np.concatenate(blob).astype(np.float64).tofile(path)
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-1500:])
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "OK" and not [l for l in lines if l.startswith("FAIL")], lines
    for what in ("plan", "constant response", "constant column", "cases"):
        assert f"ok {what}" in lines, what
    errs = [l.split() for l in lines if l.startswith("case ")]
    assert len(errs) == len(rows)
    for (name, n, d, k, x, y, ref, e_host, e_gram), f in zip(rows, errs):
        status, e = int(f[3]), float(f[5])
        print(f"{name}: status {status} e_rec {e:.3e} e_host {e_host:.3e} e_gram {e_gram:.3e}")
        assert status == 0, name
        assert e <= PO.bound(e_host, e_gram), (name, e, e_host, e_gram)
    return out


def test_host_recursion(tmp_path, rows):
    """pls_host.h on numpy's G, s and y^T y reproduces the long-double rotations under the rule of the device test"""
    _run_cases(_build(tmp_path, False), tmp_path, rows)


def test_host_recursion_under_address_and_ub_sanitizers(tmp_path, rows):
    out = _run_cases(_build(tmp_path, True), tmp_path, rows)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-1500:]


def test_plan_is_monotone_and_covers_the_rows():
    """egx_pls_get_plan: chunk_rows never shrinks as n grows, tiles / blocks never shrink as d grows, the chunks cover the rows
    exactly once with no chunk empty -- and it is the header's plan (the stand-alone program checks the same there)."""
    for d in (1, 15, 16, 63, 64, 130, 1000):
        last = 0
        for n in (1, 2, 255, 256, 257, 600, 65536, 65537, 10 ** 5, 10 ** 6, 10 ** 7 + 19):
            p = _plan(n, d)
            assert p["n"] == n and p["d"] == d
            assert p["chunk_rows"] % 64 == 0 and p["chunk_rows"] >= last
            last = p["chunk_rows"]
            edges = [min(n, c * p["chunk_rows"]) for c in range(p["n_chunks"] + 1)]
            assert edges[0] == 0 and edges[-1] == n and all(b > a for a, b in zip(edges, edges[1:]))
            assert (p["n_chunks"] - 1) * p["chunk_rows"] < n <= p["n_chunks"] * p["chunk_rows"]
            t = -(-(d + 1) // 16)
            assert p["tiles"] == t and p["out_tiles"] == t * (t + 1) // 2
            b = -(-(d + 1) // 64)
            assert p["block_side"] == b and p["blocks"] == b * (b + 1) // 2
    tiles = [_plan(1000, d)["out_tiles"] for d in range(1, 200)]
    assert all(b >= a for a, b in zip(tiles, tiles[1:]))
    from egobox_amd import _lib as L
    assert L.load().egx_pls_get_plan(0, 3, C.byref(L.PlsPlan())) == L.ERR_INVALID_VALUE
    assert L.load().egx_pls_get_plan(5, 0, C.byref(L.PlsPlan())) == L.ERR_INVALID_VALUE
    assert L.load().egx_pls_get_plan(5, 3, None) == L.ERR_INVALID_VALUE


def test_argument_checks_need_no_device():
    """k < 1, k > d, n < 2, non-finite input and NULL pointers are EGX_ERR_INVALID_VALUE before a device is touched, with the
    reference's messages where the header quotes them."""
    from egobox_amd import _lib as L
    lib = L.load()
    x = np.ascontiguousarray(np.random.default_rng(0).random((6, 3)))
    y = np.ascontiguousarray(x.sum(axis=1))
    w = np.zeros((3, 4))
    st = C.c_int32(-1)

    def call(xa, ya, n, d, k, wa=w):
        rc = lib.egx_pls_rotations(-1, None if xa is None else L.dptr(xa), None if ya is None else L.dptr(ya), n, d, k,
                                   None if wa is None else L.dptr(wa), C.byref(st))
        return rc, lib.egx_last_error().decode()

    rc, msg = call(x, y, 6, 3, 0)
    assert rc == L.ERR_INVALID_VALUE and msg == "`kpls_dim` canot be 0!"
    rc, msg = call(x, y, 6, 3, -2)
    assert rc == L.ERR_INVALID_VALUE and msg == "`kpls_dim` canot be 0!"
    rc, msg = call(x, y, 6, 3, 4)
    assert rc == L.ERR_INVALID_VALUE and msg == "Dimension reduction 4 should be smaller than actual training input dimensions 3"
    rc, msg = call(x, y, 1, 3, 1)
    assert rc == L.ERR_INVALID_VALUE and "n >= 2" in msg
    for xa, ya, wa in ((None, y, w), (x, None, w), (x, y, None)):
        rc, msg = call(xa, ya, 6, 3, 1, wa)
        assert rc == L.ERR_INVALID_VALUE and "NULL" in msg
    for bad in (np.nan, np.inf):
        xb = x.copy()
        xb[4, 1] = bad
        rc, msg = call(xb, y, 6, 3, 1)
        assert rc == L.ERR_INVALID_VALUE and msg == "x contains non-finite values"
        yb = y.copy()
        yb[5] = bad
        rc, msg = call(x, yb, 6, 3, 1)
        assert rc == L.ERR_INVALID_VALUE and msg == "y contains non-finite values"
    # the sparse handle's entry: k < 1 is refused before the handle is looked at, then a NULL handle
    assert lib.egx_sgp_compute_w_star(None, 0) == L.ERR_INVALID_VALUE
    assert lib.egx_last_error().decode() == "`kpls_dim` canot be 0!"
    assert lib.egx_sgp_compute_w_star(None, 2) == L.ERR_INVALID_VALUE
    assert "NULL" in lib.egx_last_error().decode()
    # the Python wrappers raise the same
    from egobox_amd import kpls
    with pytest.raises(L.InvalidValueError, match="canot be 0"):
        kpls.pls_rotations_device(x, y, 0)
    with pytest.raises(L.InvalidValueError, match="Dimension reduction 4"):
        kpls.pls_rotations_device(x, y, 4)


def test_builders_take_pls_host_or_device():
    import egobox_amd as egx
    from egobox_amd import sgp
    p = egx.GaussianProcess.params(egx.ConstantMean(), egx.SquaredExponentialCorr())
    assert p._pls == "host" and p.pls("device") is p and p._pls == "device"
    with pytest.raises(ValueError):
        p.pls("gpu")
    s = sgp.SgpParams(egx.SquaredExponentialCorr(), sgp.Inducings.Randomized(4))
    assert s._pls == "host" and s.pls("device") is s and s.pls("host")._pls == "host"
    with pytest.raises(ValueError):
        s.pls("somewhere")


def test_the_library_uses_the_header():
    csrc = os.path.join(ROOT, "egobox_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "kernels_pls.hip" in mk and "pls_host.h" in mk
    src = open(os.path.join(csrc, "kernels_pls.hip")).read()
    assert '#include "pls_host.h"' in src and "pls::plan(" in src and "pls::rotations_from_centred(" in src
    assert "#include <hip" not in open(os.path.join(csrc, "pls_host.h")).read()  # host only
    hpp = open(os.path.join(ROOT, "include", "egx_gp.hpp")).read()
    for sym in ("pls_rotations(", "kpls_dim(int64_t k)", "compute_w_star(int64_t k)", "int64_t kpls_dim() const"):
        assert sym in hpp, sym
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                    os.path.join(ROOT, "include", "egx_gp.h")], check=True)
