"""CPU checks of the constraint strategies of the infill criterion (cstr_infill = false: the constraint surrogates as
constraints of the optimiser): egobox_amd/csrc/infill_math.h's cstr_value / cstr_grad and the mean halves of
infill_mix_math.h compiled with g++ (tests/c_host/infill_cstr_math_test.cpp, self-checking), and the C ABI of the feature."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egobox_amd", "csrc")
INC = os.path.join(ROOT, "include")

NEW_SYMBOLS = ["egx_infill_set_cstr_strategy", "egx_infill_get_cstr_strategy", "egx_infill_eval_cstr", "egx_infill_optimize_cstr"]


def test_cstr_value_and_gradient_on_the_host(tmp_path):
    """Central differences, the sigma < eps branch, the per-coordinate sigma' (deviation 4) against the reference's formula at
    d = 1 where both agree, and mix_mean / mix_grad_mean bit for bit against mix_value / mix_grad."""
    exe = tmp_path / "infill_cstr_math_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "c_host", "infill_cstr_math_test.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout


def test_header_declares_and_library_exports_the_cstr_symbols():
    import egobox_amd as egx
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "egx_gp.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(egx_[a-z0-9_]+)\s*\(", txt))
    lib = C.CDLL(egx._lib.LIB_PATH)
    bound = {s[0] for s in egx._lib.SIGNATURES}
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in bound, name
    assert re.search(r"EGX_CSTR_INFILL = 0.*EGX_CSTR_MEAN = 1, EGX_CSTR_UTB = 2", txt, flags=re.S)
    assert egx.infill.CSTR_STRATEGIES == {"infill": 0, "mean": 1, "utb": 2}
    for name in ("set_cstr_strategy", "cstr_strategy", "constraints", "optimize_constrained"):
        assert callable(getattr(egx.InfillObjective, name))
    # the layout ctypes assumes for egx_infill_cstr_stats is the C compiler's
    st = egx._lib.InfillCstrStats
    assert (st.rounds.offset, st.best_start.offset, st.feasible.offset, st.violation.offset, st.evals.offset) == (0, 8, 16, 24, 32)


def test_null_handles_are_refused_without_a_device():
    import egobox_amd as egx
    lib = egx._lib.load()
    s = C.c_int32()
    assert lib.egx_infill_set_cstr_strategy(None, 1, None) == egx._lib.ERR_INVALID_VALUE
    assert lib.egx_infill_get_cstr_strategy(None, C.byref(s), None) == egx._lib.ERR_INVALID_VALUE
    assert lib.egx_infill_eval_cstr(None, None, 0, None, None, None, None) == egx._lib.ERR_INVALID_VALUE
    assert lib.egx_infill_optimize_cstr(None, None, None, None, 1, 0, None, None, None, None) == egx._lib.ERR_INVALID_VALUE


def test_cstr_driver_compiles_and_links(tmp_path):
    """The compiled host of the new entry points and of the C++ mirror (run on the GPU by tests/test_gpu_infill_cstr.py)."""
    libdir = os.path.join(ROOT, "egobox_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{INC}", os.path.join(ROOT, "tests", "c_host", "infill_cstr_driver.cpp"),
                    f"-L{libdir}", "-legx_gp_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o",
                    str(tmp_path / "infill_cstr_driver")], check=True)
    c = tmp_path / "t.c"   # the new declarations are plain C
    c.write_text('#include "egx_gp.h"\nint main(void) { egx_infill_cstr_stats s; s.feasible = EGX_CSTR_MEAN; return s.feasible == 1 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{INC}", str(c)], check=True)
