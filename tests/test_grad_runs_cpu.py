"""csrc/grad_runs.h -- how the entries of a lock-step gradient evaluation (the candidates of a slot, the members of a group's
run) are cut into launch sequences -- compiled for the host with the address and undefined-behaviour sanitizers and run as the
stand-alone program it is (tests/c_host/grad_runs_test.cpp): hand-written patterns, and every pattern of five entries against
a brute-force restatement."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "grad_runs_test.cpp")
PATTERNS = ["all ok, one form", "a failed entry in the middle", "alternating forms", "empty input", "all failed",
            "kLockstepMax entries, one run", "all 1024 patterns of five entries", "prescaled form"]


def _check(out):
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-800:])
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "OK" and not [l for l in lines if l.startswith("FAIL")], lines
    for what in PATTERNS:
        assert any(l.startswith(f"ok {what}") for l in lines), what


def test_run_splitting(tmp_path):
    exe = tmp_path / "grad_runs_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", str(exe)], check=True)
    _check(subprocess.run([str(exe)], capture_output=True, text=True))


def test_run_splitting_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "grad_runs_test_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert "runtime error" not in out.stderr, out.stderr[-800:]
    _check(out)


def test_the_library_uses_the_header():
    """Both clients -- the candidates of one handle and the members of a group -- cut their runs by this header."""
    src = open(os.path.join(ROOT, "egobox_amd", "csrc", "gp_fit.hip")).read()
    assert '#include "grad_runs.h"' in src and src.count("gradruns::split(") == 2
    assert "grad_runs.h" in open(os.path.join(ROOT, "egobox_amd", "csrc", "Makefile")).read()
