"""The executor's launch plan for grouped Connect steps (csrc/connect_group_plan.h), checked on the CPU: a stand-alone
program (tests/c/connect_group_plan_check.cpp) sweeps every call of 0..300 steps, depth 1..4, S in {1, 2, 3, 4, 6, 8}, S..12
host arrays and rings of 9 and 32 entries and checks that the launches cover the call once and in order, that the last
`depth` steps are launches of one, that no launch exceeds S, the host arrays or the ring, that the tickets outstanding
never exceed the ring, and that the tail tapers.  It is built twice, plain and with -fsanitize=address,undefined."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "connect_group_plan_check.cpp")
INC = os.path.join(ROOT, "board-game-simulator-python_amd", "csrc")


def _compiler():
    for cxx in ("g++", "c++", "clang++"):
        if shutil.which(cxx):
            return cxx
    pytest.fail("no host C++ compiler")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan-ubsan"])
def test_plan_properties(tmp_path, flags):
    exe = str(tmp_path / "plan_check")
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC, *flags, SRC, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.strip().splitlines()
    assert lines[-1].endswith(" plans checked, 0 failures"), lines[-1]
    assert int(lines[-1].split()[0]) == 301 * 4 * 2 * sum(13 - s for s in (1, 2, 3, 4, 6, 8))
    # the shapes the GPU test plays (depth 3, nine host arrays, a ring of 32), as the header documents them
    plans = {line.split(":")[0]: [int(k) for k in line.split(":")[1].split()] for line in lines[:-1]}
    assert plans["count 27 depth 3 S 8 host arrays 9 ring 32"] == [1, 8, 8, 4, 2, 1, 1, 1, 1]
    assert plans["count 12 depth 3 S 8 host arrays 9 ring 32"] == [8, 1, 1, 1, 1]
    assert plans["count 200 depth 3 S 2 host arrays 9 ring 32"] == [2] * 97 + [1] * 6
