"""What needs no GPU of the lock-step theta-gradient and L-BFGS fit of a group: the two new symbols in the header, the built
library and the ctypes bindings, `GpParams.fits_groups()` for the gradient optimiser, and the argument rules of the two new
Python functions, which reject bad input before any library call."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["egx_gp_likelihood_grad_multi", "egx_gp_fit_lbfgs_multi"]


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


def test_new_symbols_in_header_library_and_bindings(egx):
    from egobox_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "egx_gp.h")).read()
    sigs = {name: (res, args) for name, res, args in L.SIGNATURES}
    lib = L.load()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\(", header), sym
        assert sym in sigs and hasattr(lib, sym), sym
    # the layouts of their neighbours: egx_gp_likelihood_multi plus the gradient, egx_gp_fit_multi
    assert len(sigs["egx_gp_likelihood_grad_multi"][1]) == len(sigs["egx_gp_likelihood_multi"][1]) + 1 == 7
    assert len(sigs["egx_gp_fit_lbfgs_multi"][1]) == len(sigs["egx_gp_fit_multi"][1]) == 9
    assert callable(egx.likelihood_grad_multi) and callable(egx.fit_lbfgs_multi)


def test_fits_groups_with_the_gradient_optimiser(egx):
    P = egx.GaussianProcess.params
    assert P().optimizer("lbfgs").fits_groups() is True
    assert P().optimizer("cobyla").fits_groups() is True
    assert P().theta_tuning(egx.ThetaTuning.Fixed([1.0])).optimizer("lbfgs").fits_groups() is True
    assert P().optimizer("lbfgs").kpls_dim(2).fits_groups() is False
    partial = egx.ThetaTuning.Partial([1.0, 1.0], [(1e-2, 1e1)], [0])
    assert P().optimizer("lbfgs").theta_tuning(partial).fits_groups() is False
    with pytest.raises(egx.InvalidValueError):  # and fit_group still refuses them, before it creates anything
        P().optimizer("lbfgs").kpls_dim(2).fit_group(np.zeros((2, 8, 3)), np.zeros((2, 8)))


class _Fake:
    """stands for a handle: rejected input never reaches the library"""

    def __init__(self, h):
        self.h, self.d, self._h = h, h, None


def test_likelihood_grad_multi_rejects_bad_input(egx):
    a, b, c = _Fake(2), _Fake(2), _Fake(3)
    with pytest.raises(egx.InvalidValueError):
        egx.likelihood_grad_multi([], np.zeros((0, 2)))              # k = 0
    with pytest.raises(egx.InvalidValueError):
        egx.likelihood_grad_multi([a, a], np.ones((2, 2)))           # duplicates
    with pytest.raises(egx.InvalidValueError):
        egx.likelihood_grad_multi([a, c], np.ones((2, 2)))           # unequal h
    for bad in (np.ones((3, 2)), np.ones((2, 3)), np.ones(2), np.ones((2, 2, 1))):
        with pytest.raises(egx.InvalidValueError):
            egx.likelihood_grad_multi([a, b], bad)                   # not (k, h) or (k, 1)


def test_fit_lbfgs_multi_rejects_bad_input(egx):
    a, b = _Fake(2), _Fake(2)
    with pytest.raises(egx.InvalidValueError):
        egx.fit_lbfgs_multi([], np.zeros((0, 1, 2)), [1e-2], [1e1])
    with pytest.raises(egx.InvalidValueError):
        egx.fit_lbfgs_multi([a, a], np.ones((2, 1, 2)), [1e-2], [1e1])
    for bad in (np.ones((2, 2)), np.ones((3, 1, 2)), np.ones((2, 1, 3)), np.ones((2, 0, 2))):
        with pytest.raises(egx.InvalidValueError):
            egx.fit_lbfgs_multi([a, b], bad, [1e-2], [1e1])


def test_library_rejects_null_count_and_duplicates(egx):
    from egobox_amd import _lib as L
    lib = L.load()
    th, lk, g = np.ones((2, 2)), np.zeros(2), np.zeros((2, 2))
    st = np.zeros(2, dtype=np.int32)
    stp = st.ctypes.data_as(L.C.POINTER(L.C.c_int32))
    f = lib.egx_gp_likelihood_grad_multi
    assert f(None, 0, L.dptr(th), 2, L.dptr(lk), L.dptr(g), stp) == L.ERR_INVALID_VALUE   # k <= 0
    assert f(None, 2, L.dptr(th), 2, L.dptr(lk), L.dptr(g), stp) == L.ERR_INVALID_VALUE   # NULL list
    arr = (L.C.c_void_p * 2)()  # two NULL handles (equal, too)
    assert f(arr, 2, L.dptr(th), 2, L.dptr(lk), L.dptr(g), stp) == L.ERR_INVALID_VALUE
    assert f(arr, 2, None, 2, L.dptr(lk), L.dptr(g), stp) == L.ERR_INVALID_VALUE
    assert f(arr, 2, L.dptr(th), 2, L.dptr(lk), None, stp) == L.ERR_INVALID_VALUE
    lo, hi = np.array([1e-2]), np.array([1e1])
    f = lib.egx_gp_fit_lbfgs_multi
    assert f(None, 0, L.dptr(th), 1, L.dptr(lo), L.dptr(hi), 1, 30, None) == L.ERR_INVALID_VALUE
    assert f(arr, 2, L.dptr(th), 0, L.dptr(lo), L.dptr(hi), 1, 30, None) == L.ERR_INVALID_VALUE  # no start
    assert f(arr, 2, L.dptr(th), 1, L.dptr(lo), L.dptr(hi), 1, 30, None) == L.ERR_INVALID_VALUE  # NULL handles


def test_cpp_mirror_compiles(tmp_path):
    cpp = tmp_path / "t.cpp"
    cpp.write_text('#include "egx_gp.hpp"\n'
                   'int use(const std::vector<egobox::GaussianProcess *> &g, const double *th, const double *lo, const double *hi) {\n'
                   '    auto r = egobox::likelihood_grad_group(g, th, 2);\n'
                   '    auto ne = egobox::fit_lbfgs_group(g, th, 1, lo, hi, 1);\n'
                   '    return (int)r.status.size() + (int)ne.size();\n}\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include')}", str(cpp)], check=True)
