"""CPU-only checks of the Bounce flat Monte-Carlo evaluation's plumbing: both libraries export bgs_bounce_evaluate_moves,
the header declares it, and its kernels live in the existing evaluate unit (still exactly four kernel units)."""

import os
import subprocess

from tests import kernel_units
from tests.conftest import PKG, PRODUCT_LIB, ROOT, TEST_LIB

CSRC = os.path.join(PKG, "csrc")


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_both_libraries_export_the_bounce_evaluation():
    for path in (PRODUCT_LIB, TEST_LIB):
        assert "bgs_bounce_evaluate_moves" in _exports(path), path


def test_the_header_declares_it():
    with open(os.path.join(ROOT, "include", "bgs.h")) as f:
        text = f.read()
    assert "BGS_API int bgs_bounce_evaluate_moves(bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies," in text


def test_the_kernel_lives_in_the_evaluate_unit_of_six():
    kernel_units.check_six_distinct_ids()
    assert kernel_units.units_defining("k_bounce_evaluate<") == ["evaluate"]


def test_python_binding_is_declared():
    from simulator.game import _abi

    assert "bgs_bounce_evaluate_moves" in _abi.SIGNATURES
    assert list(_abi.UNITS) == ["connect", "bounce", "generic"]
