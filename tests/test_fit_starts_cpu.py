"""csrc/fit_starts.h, the rules every multistart hyperparameter fit shares (egobox_amd/csrc/gp_fit.hip, sgp_host.hip), on the
host: tests/c_host/fit_starts_test.cpp built with g++ alone -- no HIP, no library, no GPU.  The log10 box and its messages, the
COBYLA budget, the lock-step COBYLA and L-BFGS drivers against each start alone, sharding over ranks, a partial active set, the
start-major machine layout of egx_gp_fit_multi against the nested loop it replaced, the one-after-the-other driver of the
sparse fits."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "fit_starts_test.cpp")

GROUPS = {
    "box": 8,           # broadcast, length, lo = 0 / hi < lo / NaN with the dense and the sparse text
    "starts": 3,        # 0, negative, 1e-300
    "budget": 4,
    "cobyla": 7,        # 1, 2, 5 starts against each alone; the tie; +inf results; never the winner; all failed
    "sharding": 2,      # world 3 with 2 and with 5 starts
    "partial": 3,
    "lbfgs": 2,
    "fit_multi": 3,     # contiguous per start; own model only; the nested loop's call sequence
    "sequential": 2,
}


def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = [l for l in out.stdout.strip().split("\n") if l]
    return out, lines


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fit_starts") / "fit_starts_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", str(exe)], check=True)
    return _run(exe)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_fit_starts_header(report, group):
    out, lines = report
    mine = [l for l in lines if l.split(" ", 1)[1].startswith(group + ":")]
    assert len(mine) == GROUPS[group], lines
    assert all(l.startswith("ok ") for l in mine), mine


def test_every_check_ran_and_passed(report):
    out, lines = report
    assert out.returncode == 0, out.stdout[-800:] + out.stderr[-400:]
    assert len(lines) == sum(GROUPS.values()) and all(l.startswith("ok ") for l in lines), lines


def test_fit_starts_under_address_and_ub_sanitizers(tmp_path):
    """The same program with -fsanitize=address,undefined, run as the stand-alone program it is."""
    exe = tmp_path / "fit_starts_test_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", SRC, "-o", str(exe)], check=True)
    out, lines = _run(exe)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-800:]
    assert len(lines) == sum(GROUPS.values()) and all(l.startswith("ok ") for l in lines), lines
