"""CPU-only checks of the Bounce sequential-halving evaluation's plumbing: both libraries export
bgs_bounce_evaluate_moves_halving, the ctypes binding table has it with the header's nine arguments, and its kernel lives
in the evaluate unit, one of the six `make print-unit-ids` lists."""

import ctypes
import os
import subprocess

from tests import kernel_units
from tests.conftest import PKG, PRODUCT_LIB, TEST_LIB

CSRC = os.path.join(PKG, "csrc")
SYMBOL = "bgs_bounce_evaluate_moves_halving"


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_both_libraries_export_the_bounce_halving_evaluation():
    for path in (PRODUCT_LIB, TEST_LIB):
        assert SYMBOL in _exports(path), path


def test_the_binding_table_has_the_symbol():
    from simulator.game import _abi

    restype, argtypes = _abi.SIGNATURES[SYMBOL]
    assert restype is ctypes.c_int
    assert argtypes == [_abi.c_handle, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p,
                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    assert _abi.HALVING_SHORT == -2


def test_the_header_declares_it():
    with open(os.path.join(os.path.dirname(PKG), "include", "bgs.h")) as f:
        text = f.read()
    assert f"BGS_API int {SYMBOL}(bgs_batch* b, uint64_t seed, int32_t budget, int32_t max_plies, int policy," in text
    assert "#define BGS_HALVING_SHORT (-2)" in text


def test_the_python_layer_has_the_methods_and_the_agent():
    from simulator import agents, batch

    assert batch.HALVING_SHORT == -2
    assert [batch.BounceBatch.halving_min_budget(a) for a in (1, 2, 3, 5, 33, 512)] == [1, 2, 6, 15, 198, 4608]
    for name in ("evaluate_moves_halving", "evaluate_moves_halving_tensor"):
        assert callable(getattr(batch.BounceBatch, name)) and callable(getattr(batch.ConnectBatch, name))
    agent = agents.BounceHalvingAgent()
    assert (agent.budget, agent.max_plies, agent.policy) == (1024, None, "uniform") and agents.BOUNCE_MAX_PLIES == 1024
    assert agent.predict_many([]) == [] and agent.choose_many([]) == []


def test_the_kernel_lives_in_the_evaluate_unit_of_six():
    kernel_units.check_six_distinct_ids()
    assert kernel_units.units_defining("k_bounce_evaluate_halving") == ["evaluate"]
