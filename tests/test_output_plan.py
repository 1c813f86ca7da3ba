"""The output-buffer plan of the analysis calls (csrc/output_plan.h), checked on the CPU: a stand-alone program
(tests/c/output_plan_check.cpp) declares the outputs of every call shape the library uses -- evaluate, halving, search,
proving search, forest search (the searches with and without Bounce's `used`) and solve -- for n in 1..70, 1..16 root moves
a board and every subset of absent optional outputs, and checks that every slice is 16-byte aligned from the base, that
slices are disjoint and in order, that none passes the reported end, that the end is the last byte used, that a misaligned
device pointer is the one reported, and, for each of the 256 residues of a base address, that the library's own workspace
is 256-byte aligned and fits the allocation.  It is built twice, plain and with -fsanitize=address,undefined."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "output_plan_check.cpp")
INC = os.path.join(ROOT, "board-game-simulator-python_amd", "csrc")

# optional outputs of the nine shapes: evaluate, halving, search, search+used, proving, proving+used, forest, forest+used, solve
OPTIONAL = (0, 2, 3, 4, 5, 6, 4, 5, 2)


def _compiler():
    for cxx in ("g++", "c++", "clang++"):
        if shutil.which(cxx):
            return cxx
    pytest.fail("no host C++ compiler")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan-ubsan"])
def test_plan_properties(tmp_path, flags):
    exe = str(tmp_path / "output_plan_check")
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC, *flags, SRC, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    assert last.endswith(" plans checked, 0 failures"), last
    assert int(last.split()[0]) == 70 * 16 * sum(2 ** k for k in OPTIONAL)
