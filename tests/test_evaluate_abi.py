"""CPU-only checks of the flat Monte-Carlo evaluation's plumbing: both libraries export bgs_connect_evaluate_actions, its
kernels are a fourth kernel unit of their own, and bench.py's three units are untouched by it."""

import os
import subprocess
import sys

from tests.conftest import PKG, PRODUCT_LIB, TEST_LIB

CSRC = os.path.join(PKG, "csrc")


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_both_libraries_export_the_evaluation():
    for path in (PRODUCT_LIB, TEST_LIB):
        assert "bgs_connect_evaluate_actions" in _exports(path), path


def test_the_evaluation_is_a_fourth_kernel_unit():
    out = subprocess.check_output(["make", "-s", "--no-print-directory", "-C", CSRC, "print-unit-ids"], text=True)
    units = dict(line.split() for line in out.splitlines())
    assert list(units) == ["connect", "bounce", "generic", "evaluate"]
    assert len(set(units.values())) == 4 and all(len(v) == 16 for v in units.values())


def test_loaded_library_reports_the_fourth_unit_and_bench_keeps_three():
    code = (
        "import sys; sys.path.insert(0, sys.argv[1]); from simulator.game import _abi; "
        "print(*_abi.UNITS); print(_abi.unit_ids()['connect'], _abi.extra_unit_ids()['evaluate'])"
    )
    env = dict(os.environ, BGS_LIBRARY=PRODUCT_LIB)
    out = subprocess.check_output([sys.executable, "-c", code, PKG], text=True, env=env).splitlines()
    assert out[0].split() == ["connect", "bounce", "generic"]
    made = dict(line.split() for line in subprocess.check_output(
        ["make", "-s", "--no-print-directory", "-C", CSRC, "print-unit-ids"], text=True).splitlines())
    assert out[1].split() == [made["connect"], made["evaluate"]]
