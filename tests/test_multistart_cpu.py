"""csrc/multistart.h, the lock-step driver of the three infill multistarts (egobox_amd/csrc/infill_optimize.hip), on the host:
tests/c_host/multistart_test.cpp built with g++ alone -- no HIP, no library, no GPU.  Scripted machines of unequal length for the
round loop, the real CobylaBox / Cobyla / Slsqp in lock-step against each start alone (the host twin of
test_every_start_walks_the_points_it_walks_alone), the winner rules, the argument check's messages."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "multistart_test.cpp")

GROUPS = {
    "scripted": 6,      # rounds, order, points, answers, a failed evaluation, no machine
    "CobylaBox": 1,
    "Cobyla": 1,
    "Slsqp": 1,
    "winner": 5,        # feasible first, key, violation, the two ties
    "no finite value": 2,
    "one finite value": 1,
    "own best": 4,
    "arguments": 7,
}


def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = [l for l in out.stdout.strip().split("\n") if l]
    return out, lines


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("multistart") / "multistart_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", str(exe)], check=True)
    return _run(exe)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_multistart_header(report, group):
    out, lines = report
    mine = [l for l in lines if l.split(" ", 1)[1].startswith(group + ":")]
    assert len(mine) == GROUPS[group], lines
    assert all(l.startswith("ok ") for l in mine), mine


def test_every_check_ran_and_passed(report):
    out, lines = report
    assert out.returncode == 0, out.stdout[-800:] + out.stderr[-400:]
    assert len(lines) == sum(GROUPS.values()) and all(l.startswith("ok ") for l in lines), lines


def test_multistart_under_address_and_ub_sanitizers(tmp_path):
    """The same program with -fsanitize=address,undefined, run as the stand-alone program it is."""
    exe = tmp_path / "multistart_test_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", SRC, "-o", str(exe)], check=True)
    out, lines = _run(exe)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-800:]
    assert len(lines) == sum(GROUPS.values()) and all(l.startswith("ok ") for l in lines), lines
