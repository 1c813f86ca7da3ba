"""CPU-only checks of the flat Monte-Carlo evaluation's plumbing: both libraries export bgs_connect_evaluate_actions, its
kernels are a fourth kernel unit of their own (of six: the searches and the solvers follow it), and bench.py's three units
are untouched by it."""

import os
import subprocess
import sys

from tests import kernel_units
from tests.conftest import PKG, PRODUCT_LIB, TEST_LIB

CSRC = os.path.join(PKG, "csrc")


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_both_libraries_export_the_evaluation():
    for path in (PRODUCT_LIB, TEST_LIB):
        assert "bgs_connect_evaluate_actions" in _exports(path), path


def test_the_evaluation_is_a_fourth_kernel_unit():
    units = kernel_units.check_six_distinct_ids()
    assert list(units)[3] == "evaluate" and kernel_units.units_defining("k_connect_evaluate<") == ["evaluate"]


def test_loaded_library_reports_the_fourth_unit_and_bench_keeps_three():
    code = (
        "import sys; sys.path.insert(0, sys.argv[1]); from simulator.game import _abi; "
        "print(*_abi.UNITS); print(_abi.unit_ids()['connect'], _abi.extra_unit_ids()['evaluate'])"
    )
    env = dict(os.environ, BGS_LIBRARY=PRODUCT_LIB)
    out = subprocess.check_output([sys.executable, "-c", code, PKG], text=True, env=env).splitlines()
    assert out[0].split() == ["connect", "bounce", "generic"]
    made = kernel_units.made_unit_ids()
    assert out[1].split() == [made["connect"], made["evaluate"]]
