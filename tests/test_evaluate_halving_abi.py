"""CPU-only checks of the sequential-halving evaluation's plumbing: both libraries export
bgs_connect_evaluate_actions_halving, the ctypes binding table has it with the header's nine arguments, and its kernel
lives in the evaluate unit, one of the six `make print-unit-ids` lists."""

import ctypes
import os
import subprocess

from tests import kernel_units
from tests.conftest import PKG, PRODUCT_LIB, TEST_LIB

CSRC = os.path.join(PKG, "csrc")
SYMBOL = "bgs_connect_evaluate_actions_halving"


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_both_libraries_export_the_halving_evaluation():
    for path in (PRODUCT_LIB, TEST_LIB):
        assert SYMBOL in _exports(path), path


def test_the_binding_table_has_the_symbol():
    from simulator.game import _abi

    restype, argtypes = _abi.SIGNATURES[SYMBOL]
    assert restype is ctypes.c_int
    assert argtypes == [_abi.c_handle, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p,
                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]


def test_the_header_declares_it():
    with open(os.path.join(os.path.dirname(PKG), "include", "bgs.h")) as f:
        text = f.read()
    assert f"BGS_API int {SYMBOL}(bgs_batch* b, uint64_t seed, int32_t budget, int32_t max_plies, int policy," in text


def test_the_kernel_lives_in_the_evaluate_unit_of_six():
    kernel_units.check_six_distinct_ids()
    assert kernel_units.units_defining("k_connect_evaluate_halving") == ["evaluate"]
