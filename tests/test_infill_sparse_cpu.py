"""Sparse experts in the infill handle and sparse mixtures, the parts that need no GPU: egx_infill_create_any's checks before
any device call, the ctypes layout of its structs, what SparseGpMix refuses, the two sparse mixture entry points' argument
checks, and the C host of tests/c_host/infill_sparse_driver.c and the C++ mirror compiling and linking."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


def _err(lib):
    return lib.egx_last_error().decode()


def test_header_declares_and_library_exports_the_sparse_symbols(egx):
    L = egx._lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egx_gp.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(egx_[a-z0-9_]+)\s*\(", txt))
    lib = C.CDLL(L.LIB_PATH)
    bound = {s[0] for s in L.SIGNATURES}
    for name in ("egx_infill_create_any", "egx_moe_predict_valvar_sgp", "egx_moe_predict_valvar_gradients_sgp"):
        assert name in declared and hasattr(lib, name) and name in bound, name
    assert "egx_infill_surrogate_any" in txt and "egx_model_ref" in txt
    assert (L.MODEL_GP, L.MODEL_SGP) == (0, 1)
    # the ctypes mirrors have the C layout: int32 (+ padding), pointer; then as egx_infill_surrogate
    R, S = L.ModelRef, L.InfillSurrogateAny
    assert (R.kind.offset, R.handle.offset, C.sizeof(R)) == (0, 8, 16)
    assert (S.experts.offset, S.n_experts.offset, S.weights.offset, S.means.offset, S.precisions_chol.offset,
            S.heaviside_factor.offset, S.smooth.offset, C.sizeof(S)) == (0, 8, 16, 24, 32, 40, 48, 56)


def test_create_any_refuses_bad_arguments_before_the_device_is_touched(egx):
    L = egx._lib
    lib = L.load()
    h = C.c_void_p()
    assert lib.egx_infill_create_any(None, None, None, 0, C.byref(h)) == L.ERR_INVALID_VALUE and not h
    assert lib.egx_infill_create_any(None, (L.InfillSurrogateAny * 1)(), None, 0, None) == L.ERR_INVALID_VALUE
    s = (L.InfillSurrogateAny * 2)()  # zeroed: NULL experts, n_experts 0
    assert lib.egx_infill_create_any(None, s, None, 0, C.byref(h)) == L.ERR_INVALID_VALUE and not h
    assert "surrogate 0 needs at least one expert" in _err(lib)
    assert lib.egx_infill_create_any(None, s, None, 1, C.byref(h)) == L.ERR_INVALID_VALUE  # a constraint without tolerances
    # a never-dereferenced stand-in for a model (zeroed memory: the checks below all come before a model is read)
    fake = C.create_string_buffer(1 << 16)
    addr = C.addressof(fake)
    refs = (L.ModelRef * 2)(L.ModelRef(L.MODEL_SGP, addr), L.ModelRef(L.MODEL_GP, None))
    s[0].experts, s[0].n_experts, s[0].heaviside_factor = refs, 2, 1.0
    assert lib.egx_infill_create_any(None, s, None, 0, C.byref(h)) == L.ERR_INVALID_VALUE and not h
    assert "surrogate 0 expert 1 is NULL" in _err(lib)
    refs[1] = L.ModelRef(2, addr)  # neither EGX_MODEL_GP nor EGX_MODEL_SGP
    assert lib.egx_infill_create_any(None, s, None, 0, C.byref(h)) == L.ERR_INVALID_VALUE and not h
    assert "surrogate 0 expert 1" in _err(lib) and "kind" in _err(lib)
    refs[1] = L.ModelRef(-1, addr)
    assert lib.egx_infill_create_any(None, s, None, 0, C.byref(h)) == L.ERR_INVALID_VALUE and "surrogate 0 expert 1" in _err(lib)
    # the same in a constraint surrogate: named by its own index
    one = (L.ModelRef * 1)(L.ModelRef(L.MODEL_SGP, addr))
    s[0].experts, s[0].n_experts = one, 1
    s[1].experts, s[1].n_experts, s[1].heaviside_factor = refs, 2, 1.0
    tol = np.zeros(1)
    assert lib.egx_infill_create_any(None, s, L.dptr(tol), 1, C.byref(h)) == L.ERR_INVALID_VALUE and not h
    assert "surrogate 1 expert 1" in _err(lib)
    s[1].n_experts = -3
    assert lib.egx_infill_create_any(None, s, L.dptr(tol), 1, C.byref(h)) == L.ERR_INVALID_VALUE
    assert "surrogate 1 needs at least one expert" in _err(lib)
    tol[0] = np.nan
    s[1].n_experts = 2
    assert lib.egx_infill_create_any(None, s, L.dptr(tol), 1, C.byref(h)) == L.ERR_INVALID_VALUE and "tolerance 0" in _err(lib)
    # bad mixture data of a two-expert surrogate: NULL arrays, a heaviside factor that is not positive and finite
    refs[1] = L.ModelRef(L.MODEL_GP, addr)
    s[0].experts, s[0].n_experts = refs, 2
    assert lib.egx_infill_create_any(None, s, None, 0, C.byref(h)) == L.ERR_INVALID_VALUE and not h
    assert "surrogate 0: NULL weights, means or precisions_chol" in _err(lib)
    w = np.array([0.5, 0.5])
    s[0].weights, s[0].means, s[0].precisions_chol = L.dptr(w), L.dptr(w), L.dptr(w)
    for bad in (0.0, -1.0, np.inf, np.nan):
        s[0].heaviside_factor = bad
        assert lib.egx_infill_create_any(None, s, None, 0, C.byref(h)) == L.ERR_INVALID_VALUE and not h
        assert "surrogate 0: heaviside_factor" in _err(lib)
    cfg = L.InfillConfig()
    lib.egx_infill_config_default(C.byref(cfg))
    cfg.criterion = 9
    assert lib.egx_infill_create_any(C.byref(cfg), s, None, 0, C.byref(h)) == L.ERR_INVALID_VALUE and "criterion" in _err(lib)


def test_sparse_mixture_entry_points_check_their_arguments(egx):
    L = egx._lib
    lib = L.load()
    x, p, out = np.zeros((2, 1)), np.ones((2, 1)), np.zeros(2)
    ids = np.zeros(1, dtype=np.int32)
    harr = (C.c_void_p * 1)(None)
    iptr = ids.ctypes.data_as(L.c_int32_p)
    assert lib.egx_moe_predict_valvar_sgp(None, harr, iptr, 1, 0, L.dptr(p), L.dptr(x), 2, 1, 1, L.dptr(out), None) == L.ERR_INVALID_VALUE
    assert "egx_moe_predict_valvar_sgp" in _err(lib)
    assert lib.egx_moe_predict_valvar_sgp(None, harr, iptr, 1, 1, L.dptr(p), L.dptr(x), 2, 1, 1, None, None) == L.ERR_INVALID_VALUE
    assert lib.egx_moe_predict_valvar_sgp(None, harr, iptr, 1, 2, L.dptr(p), L.dptr(x), 2, 1, 1, L.dptr(out), None) == L.ERR_INVALID_VALUE
    assert "every expert must be local" in _err(lib)
    assert lib.egx_moe_predict_valvar_sgp(None, harr, iptr, 1, 1, L.dptr(p), L.dptr(x), 0, 1, 1, L.dptr(out), None) == L.SUCCESS  # m = 0
    # a NULL expert is the fold's own error, named by the entry point
    assert lib.egx_moe_predict_valvar_sgp(None, harr, iptr, 1, 1, L.dptr(p), L.dptr(x), 2, 1, 1, L.dptr(out), None) == L.ERR_INVALID_VALUE
    assert "egx_moe_predict_valvar_sgp: NULL expert" in _err(lib)
    g = np.zeros((2, 1))
    assert lib.egx_moe_predict_valvar_gradients_sgp(None, harr, iptr, 2, 2, L.dptr(p), None, L.dptr(x), 2, 1, 1, L.dptr(g),
                                                    None) == L.ERR_INVALID_VALUE  # smooth, two experts, no dprobas
    assert "egx_moe_predict_valvar_gradients_sgp" in _err(lib) and "dprobas" in _err(lib)
    assert lib.egx_moe_predict_valvar_gradients_sgp(None, harr, iptr, 1, 1, L.dptr(p), None, L.dptr(x), 2, 1, 0, L.dptr(g),
                                                    None) == L.ERR_INVALID_VALUE
    assert "egx_moe_predict_valvar_gradients_sgp: NULL expert" in _err(lib)


def test_sparse_gp_mix_refuses_what_is_not_implemented(egx):
    from egobox_amd.sgp import SparseGpMix, SparseGpx
    with pytest.raises(NotImplementedError, match="n_clusters"):
        SparseGpMix(nz=10, n_clusters=0)
    with pytest.raises(NotImplementedError, match="n_clusters"):
        SparseGpx.builder(nz=10, n_clusters=0)
    with pytest.raises(NotImplementedError, match="KPLS"):
        SparseGpMix(nz=10, kpls_dim=2)
    with pytest.raises(NotImplementedError, match="KPLS"):
        SparseGpMix(nz=10, kpls_dim=2, n_clusters=3)
    with pytest.raises(ValueError, match="recombination"):
        SparseGpMix(nz=10, n_clusters=2, recombination="soft")
    with pytest.raises(ValueError, match="nz or z"):
        SparseGpMix(n_clusters=2)
    from egobox_amd.gpx import Recombination
    b = SparseGpMix(nz=10, n_clusters=3, recombination=Recombination.HARD)
    assert (b.n_clusters, b.recombination, b.heaviside_factor) == (3, "hard", None)
    assert SparseGpMix(nz=10).n_clusters == 1


def test_a_mixture_of_both_kinds_keeps_the_numpy_fold(egx):
    """GpMixture hands its experts to the library only when all of them are of one kind (no device is touched to decide)."""
    from egobox_amd.moe import GaussianMixture, GpMixture
    from egobox_amd.sgp import SgpHandle

    class _Owner:  # what GpMixture looks at: expert._h._h
        def __init__(self, h):
            self._h = h

    sparse = SgpHandle.__new__(SgpHandle)
    sparse._h = C.c_void_p(1)
    sparse._lib = None
    dense = _Owner(C.c_void_p(2))
    gmx = GaussianMixture([0.5, 0.5], [[0.0], [1.0]], [[[1.0]], [[1.0]]])
    try:
        assert GpMixture([_Owner(dense), _Owner(dense)], gmx)._library_handles()[2] is False
        ids, hs, is_sparse = GpMixture([_Owner(sparse), sparse], gmx)._library_handles()  # a SparseGaussianProcess, an SgpHandle
        assert ids == [0, 1] and is_sparse is True and [h.value for h in hs] == [1, 1]
        assert GpMixture([_Owner(dense), _Owner(sparse)], gmx)._library_handles() is None
    finally:
        sparse._h = None  # nothing to destroy


def test_sparse_driver_and_cpp_mirror_compile_and_link(tmp_path):
    inc = os.path.join(ROOT, "include")
    src = os.path.join(ROOT, "tests", "c_host", "infill_sparse_driver.c")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{inc}", src], check=True)
    libdir = os.path.join(ROOT, "egobox_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{inc}", src, f"-L{libdir}", "-legx_gp_hip", "-lm",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(tmp_path / "infill_sparse_driver")], check=True)
    cpp = tmp_path / "t.cpp"
    cpp.write_text('#include "egx_gp.hpp"\n'
                   'int use(egobox::GaussianProcess &gp, egobox::SparseGaussianProcess &sgp) {\n'
                   '  egobox::InfillSurrogate obj(sgp), mix; mix.add(sgp).add(gp); mix.weights = {0.5, 0.5}; mix.smooth = false;\n'
                   '  egobox::InfillObjective o({obj, mix}, {0.0}, EGX_INFILL_EI, 0.0); double x[1] = {0.0};\n'
                   '  return (int)o.value(x, 1).size() + (int)o.eval_experts(1, x, 1).probas.size(); }\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{inc}", str(cpp)], check=True)
