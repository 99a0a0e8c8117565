"""tests/c_host/grad_multi_host.cpp: a C++ host (no Python) drives egobox::likelihood_grad_group and egobox::fit_lbfgs_group of
include/egx_gp.hpp on a group of four models and compares every row and every fitted model bit for bit with the lone calls of
the C ABI.  Exit status 0 means equal bits."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_host_group_calls_equal_the_lone_calls(tmp_path):
    exe = tmp_path / "grad_multi_host"
    libdir = os.path.join(ROOT, "egobox_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "c_host", "grad_multi_host.cpp"), f"-L{libdir}", "-legx_gp_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert out.stdout.startswith("OK")
