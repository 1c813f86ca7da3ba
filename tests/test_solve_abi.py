"""CPU-only checks of the exact solver's plumbing: both libraries export bgs_connect_solve_actions, the header declares
it and its codes, the solver lives in the solve unit (one of six kernel units), and bench.py's units are untouched."""

import os
import re
import subprocess
import sys

from tests import kernel_units
from tests.conftest import PKG, PRODUCT_LIB, ROOT, TEST_LIB

CSRC = os.path.join(PKG, "csrc")


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_both_libraries_export_the_solver():
    for path in (PRODUCT_LIB, TEST_LIB):
        assert "bgs_connect_solve_actions" in _exports(path), path


def test_header_declares_the_solver_and_its_codes():
    with open(os.path.join(ROOT, "include", "bgs.h")) as f:
        text = f.read()
    assert re.search(r"BGS_API int bgs_connect_solve_actions\(bgs_batch\* b, int32_t depth, int64_t max_nodes, int8_t\* codes,"
                     r"\s+int16_t\* plies,\s+uint64_t\* nodes, int on_device\);", text)
    codes = dict(re.findall(r"#define (BGS_SOLVE_\w+) \(?(-?\d+)\)?", text))
    assert codes == {"BGS_SOLVE_NONE": "-2", "BGS_SOLVE_LOSS": "-1", "BGS_SOLVE_DRAW": "0", "BGS_SOLVE_WIN": "1",
                     "BGS_SOLVE_UNKNOWN": "2", "BGS_SOLVE_BUDGET": "3"}
    from simulator import batch

    assert (batch.SOLVE_NONE, batch.SOLVE_LOSS, batch.SOLVE_DRAW, batch.SOLVE_WIN, batch.SOLVE_UNKNOWN, batch.SOLVE_BUDGET) == \
        (-2, -1, 0, 1, 2, 3)


def test_the_solver_lives_in_the_solve_unit_of_six():
    kernel_units.check_six_distinct_ids()
    assert kernel_units.units_defining("k_connect_solve") == ["solve"] and kernel_units.units_defining("bgs::connect_solve(") == ["solve"]


def test_abi_units_unchanged():
    code = "import sys; sys.path.insert(0, sys.argv[1]); from simulator.game import _abi; print(*_abi.UNITS)"
    env = dict(os.environ, BGS_LIBRARY=PRODUCT_LIB)
    out = subprocess.check_output([sys.executable, "-c", code, PKG], text=True, env=env).split()
    assert out == ["connect", "bounce", "generic"]


def test_bounce_batches_refuse_in_python_without_a_gpu_call():
    from simulator.batch import BounceBatch

    assert BounceBatch.solve_actions is BounceBatch.solve_actions_tensor
