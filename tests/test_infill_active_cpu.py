"""Active coordinates and CoEGO without a GPU: `random_activity` / `strip` against the reference's two cases (coego.rs:225-261),
the constructor checks of `Egor(coego_n_coop=...)`, csrc/infill_active.h through a stand-alone g++ program (and again under the
address and undefined-behaviour sanitizers), and the three new symbols in header, library and bindings."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "infill_active_test.cpp")
GROUPS = {"check": 10, "expand": 5, "round trip": 5, "gather": 1}
NEW_SYMBOLS = ["egx_infill_set_active", "egx_infill_clear_active", "egx_infill_get_active"]


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


# ---- random_activity, strip ---------------------------------------------------------------------------------------------------
def test_random_activity_balanced(egx):
    act = egx.egor.random_activity(125, 5, np.random.default_rng(0))
    assert act.shape == (5, 25) and (act < 125).all()
    assert sorted(act.ravel().tolist()) == list(range(125))


def test_random_activity_with_a_remainder(egx):
    act = egx.egor.random_activity(123, 5, np.random.default_rng(1))
    assert act.shape == (5, 25)
    assert act[3, 24] == 123 and act[4, 24] == 123
    flat = act.ravel()
    assert (np.flatnonzero(flat >= 123) == [99, 124]).all()  # the two markers, nowhere else
    assert sorted(flat[flat < 123].tolist()) == list(range(123))
    sizes = [len(egx.egor.strip(row, 123)) for row in act]
    assert sizes == [25, 25, 25, 24, 24]


@pytest.mark.parametrize("nx,k,shape", [(7, 7, (7, 1)), (7, 1, (1, 7)), (8, 3, (3, 3)), (2, 2, (2, 1))])
def test_random_activity_edges(egx, nx, k, shape):
    act = egx.egor.random_activity(nx, k, np.random.default_rng(2))
    assert act.shape == shape
    kept = [i for row in act for i in egx.egor.strip(row, nx)]
    assert sorted(kept) == list(range(nx))  # every index exactly once
    assert act.max() <= nx


def test_random_activity_is_a_function_of_the_generator(egx):
    a = egx.egor.random_activity(40, 4, np.random.default_rng(5))
    b = egx.egor.random_activity(40, 4, np.random.default_rng(5))
    c = egx.egor.random_activity(40, 4, np.random.default_rng(6))
    assert (a == b).all() and not (a == c).all()
    assert not (a.ravel() == np.arange(40)).all()  # shuffled


def test_strip(egx):
    assert egx.egor.strip([4, 0, 9, 2, 9], 9) == [4, 0, 2]  # the order stays
    assert egx.egor.strip(np.array([1, 3]), 9) == [1, 3]
    assert egx.egor.strip([9], 9) == []


# ---- Egor(coego_n_coop=...) ---------------------------------------------------------------------------------------------------
LIM2 = np.array([[0.0, 1.0], [-1.0, 1.0]])


def test_coego_constructs_on_two_columns(egx):
    e = egx.Egor(LIM2, coego_n_coop=2)
    assert e.coego_n_coop == 2 and e.last_coego_ == []
    assert egx.Egor(LIM2, coego_n_coop=1).coego_n_coop == 1
    assert egx.Egor(LIM2).coego_n_coop == 0 and egx.Egor(LIM2, coego_n_coop=0).coego_n_coop == 0


def test_coego_refusals(egx):
    with pytest.raises(egx.InvalidValueError, match="coego_n_coop"):
        egx.Egor(LIM2, coego_n_coop=3)
    with pytest.raises(egx.InvalidValueError, match="coego_n_coop"):
        egx.Egor(LIM2, coego_n_coop=-1)
    with pytest.raises(egx.InvalidValueError, match="kpls_dim"):
        egx.Egor(LIM2, gp_config=egx.GpConfig(kpls_dim=1), coego_n_coop=2)
    with pytest.raises(egx.InvalidValueError, match="n_clusters"):
        egx.Egor(LIM2, gp_config=egx.GpConfig(n_clusters=2), coego_n_coop=2)
    egx.Egor(LIM2, gp_config=egx.GpConfig(n_clusters=2))  # (without CoEGO both stay allowed)
    egx.Egor(LIM2, gp_config=egx.GpConfig(kpls_dim=1))


# ---- csrc/infill_active.h on the host ------------------------------------------------------------------------------------------
def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    return out, [l for l in out.stdout.strip().split("\n") if l]


def _check(out, lines):
    assert out.returncode == 0, out.stdout[-800:] + out.stderr[-400:]
    assert len(lines) == sum(GROUPS.values()) and all(l.startswith("ok ") for l in lines), lines
    for group, count in GROUPS.items():
        assert len([l for l in lines if l.split(" ", 1)[1].startswith(group + ":")]) == count, (group, lines)


def test_infill_active_header(tmp_path):
    exe = tmp_path / "infill_active_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", str(exe)], check=True)
    _check(*_run(exe))


def test_infill_active_header_under_address_and_ub_sanitizers(tmp_path):
    """The same program with -fsanitize=address,undefined, run as the stand-alone program it is."""
    exe = tmp_path / "infill_active_test_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", SRC, "-o", str(exe)], check=True)
    out, lines = _run(exe)
    assert "runtime error" not in out.stderr, out.stderr[-800:]
    _check(out, lines)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_activity_symbols(egx):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egx_gp.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(egx_[a-z0-9_]+)\s*\(", txt))
    lib = C.CDLL(egx._lib.LIB_PATH)
    sigs = {name: (res, args) for name, res, args in egx._lib.SIGNATURES}
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in sigs, name
    L = egx._lib
    assert sigs["egx_infill_set_active"] == (C.c_int32, [C.c_void_p, L.c_int32_p, C.c_int32, L.c_double_p])
    assert sigs["egx_infill_clear_active"] == (C.c_int32, [C.c_void_p])
    assert sigs["egx_infill_get_active"] == (C.c_int32, [C.c_void_p, L.c_int32_p, L.c_int32_p, L.c_double_p])
    assert declared == set(sigs) and len(L.SIGNATURES) == len(sigs)


def test_null_handle_is_an_invalid_value(egx):
    lib = egx._lib.load()
    idx, xb, n = np.zeros(1, dtype=np.int32), np.zeros(1), C.c_int32(7)
    assert lib.egx_infill_set_active(None, idx.ctypes.data_as(egx._lib.c_int32_p), 1, egx._lib.dptr(xb)) == egx._lib.ERR_INVALID_VALUE
    assert lib.egx_infill_clear_active(None) == egx._lib.ERR_INVALID_VALUE
    assert lib.egx_infill_get_active(None, C.byref(n), None, None) == egx._lib.ERR_INVALID_VALUE


def test_cpp_mirror_compiles(tmp_path):
    cpp = tmp_path / "t.cpp"
    cpp.write_text('#include "egx_gp.hpp"\n'
                   'int use(egobox::InfillObjective &o) { o.set_active({2, 0}, {0.0, 0.0, 0.0}); auto a = o.active(); o.clear_active(); '
                   'return (int)a.indices.size() + (int)o.width(); }\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include')}", str(cpp)], check=True)
