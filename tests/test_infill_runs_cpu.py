"""Runs of an infill handle and the lock-step x-gradients without a GPU: csrc/infill_runs.h -- which consecutive surrogates go
through one launch sequence -- on described shapes through a stand-alone g++ program (and again under the address and
undefined-behaviour sanitizers), the argument rules of the two new entry points, which are checked before any device work, and
the new symbols in header, library and bindings."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "infill_runs_test.cpp")
#: the cases of the run rule: what the program must report, in its order
EXPECTED = [
    ("1 + 4 equal shapes, all full, one group", [5]),
    ("the same, not a group", [1, 1, 1, 1, 1]),
    ("mean-only constraints, not a group", [1, 4]),
    ("mean-only constraints of a group: the objective's sequence is the full one", [1, 4]),
    ("1 + 17 mean-only", [1, 16, 1]),
    ("1 + 17 full, one group", [16, 2]),
    ("one constraint with another n in the middle", [1, 2, 1, 1]),
    ("a sparse model or a mixture cuts the run", [1, 1, 1, 2]),
    ("... a full run as well", [2, 1, 2]),
    ("pending points, q = 1: a group", [1, 1, 1, 1, 1]),
    ("pending points, q = 1: mean-only", [1, 1, 1, 1, 1]),
    ("the byte bound cuts the run", [3, 2]),
    ("... below one block every run is one", [1, 1, 1, 1, 1]),
    ("a member of another group cuts a full run", [3, 1, 1]),
    ("slots out of order cut a full run", [2, 1, 1, 1]),
    ("... and leave a mean-only run alone", [1, 4]),
    ("another kernel", [1, 1, 1, 1]),
    ("another trend", [1, 2, 1]),
    ("other coefficient columns", [1, 1, 2]),
    ("same shapes that are not adjacent do not merge", [1, 1, 1, 1, 1]),
    ("the objective alone", [1]),
]
NEW_SYMBOLS = ["egx_gp_predict_valvar_gradients_multi", "egx_infill_get_runs"]


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


# ---- csrc/infill_runs.h on the host --------------------------------------------------------------------------------------------
def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    return out, [l for l in out.stdout.strip().split("\n") if l]


def _check(out, lines):
    assert out.returncode == 0, out.stdout[-1200:] + out.stderr[-400:]
    assert len(lines) == len(EXPECTED), lines
    for line, (what, runs) in zip(lines, EXPECTED):
        assert line == f"ok {what}: [{','.join(str(v) for v in runs)}]", line


def test_run_rule(tmp_path):
    exe = tmp_path / "infill_runs_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", str(exe)], check=True)
    _check(*_run(exe))


def test_run_rule_under_address_and_ub_sanitizers(tmp_path):
    """The same program with -fsanitize=address,undefined, run as the stand-alone program it is."""
    exe = tmp_path / "infill_runs_test_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", SRC, "-o", str(exe)], check=True)
    out, lines = _run(exe)
    assert "runtime error" not in out.stderr, out.stderr[-800:]
    _check(out, lines)


# ---- the new entry points' argument rules ------------------------------------------------------------------------------------------
class _Fake:
    def __init__(self, d):
        self.d, self._h = d, None


def test_binding_rejects_bad_lists_and_shapes(egx):
    a, b, c = _Fake(2), _Fake(2), _Fake(3)
    xq = np.zeros((2, 4, 2))
    with pytest.raises(egx.InvalidValueError):
        egx.predict_valvar_gradients_multi([], xq)
    with pytest.raises(egx.InvalidValueError):
        egx.predict_valvar_gradients_multi([a, b], xq, want_val=False, want_var=False)
    with pytest.raises(egx.InvalidValueError):
        egx.predict_valvar_gradients_multi([a, c], xq)             # unequal d
    with pytest.raises(egx.InvalidValueError):
        egx.predict_valvar_gradients_multi([a, a], xq)             # duplicates
    with pytest.raises(egx.InvalidValueError):
        egx.predict_valvar_gradients_multi([a, b], xq[:1])         # one block per model
    with pytest.raises(egx.InvalidValueError):
        egx.predict_valvar_gradients_multi([a, b], np.zeros((2, 4, 3)))


def test_library_rejects_null_count_and_duplicates(egx):
    from egobox_amd import _lib as L
    lib = L.load()
    f = lib.egx_gp_predict_valvar_gradients_multi
    xq = np.zeros((2, 4, 2))
    out = np.zeros((2, 4, 2))
    assert f(None, 0, L.dptr(xq), 4, L.dptr(out), None) == L.ERR_INVALID_VALUE    # k <= 0
    assert f(None, -1, L.dptr(xq), 4, L.dptr(out), None) == L.ERR_INVALID_VALUE
    assert f(None, 2, L.dptr(xq), 4, L.dptr(out), None) == L.ERR_INVALID_VALUE    # NULL list
    arr = (L.C.c_void_p * 2)()  # two NULL handles (equal, too)
    assert f(arr, 2, L.dptr(xq), 4, L.dptr(out), None) == L.ERR_INVALID_VALUE
    assert f(arr, 2, None, 4, L.dptr(out), None) == L.ERR_INVALID_VALUE           # no queries
    assert f(arr, 2, L.dptr(xq), 4, None, None) == L.ERR_INVALID_VALUE            # neither output
    assert f(arr, 2, L.dptr(xq), -1, L.dptr(out), L.dptr(out)) == L.ERR_INVALID_VALUE
    n = L.C.c_int32()
    assert lib.egx_infill_get_runs(None, L.C.byref(n), None) == L.ERR_INVALID_VALUE
    assert b"NULL" in lib.egx_last_error()


# ---- the symbols everywhere ----------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_library_and_bindings(egx):
    from egobox_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "egx_gp.h")).read()
    bound = {name for name, _, _ in L.SIGNATURES}
    lib = L.load()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\(", header), sym
        assert sym in bound and hasattr(lib, sym), sym
    assert callable(egx.predict_valvar_gradients_multi)
    assert isinstance(egx.InfillObjective.runs, property)


def test_cpp_mirror_compiles(tmp_path):
    cpp = tmp_path / "t.cpp"
    cpp.write_text('#include "egx_gp.hpp"\n'
                   'int use(egobox::InfillObjective &o, const std::vector<const egobox::GaussianProcess *> &g, const double *xq) {\n'
                   '    auto gr = egobox::predict_valvar_gradients_group(g, xq, 9, 2);\n'
                   '    return (int)o.runs().size() + (int)gr.first.size();\n}\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include')}", str(cpp)], check=True)
