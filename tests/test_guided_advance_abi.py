"""CPU-only checks of the guided advance's plumbing: both libraries export bgs_connect_guided_advance, the header
declares it with its constant and its contract, the ctypes binding table has it with the header's arguments, a NULL batch
is refused with BGS_ERR_ARG and a message (the one refusal that can be reached without a device: every other one is made
in tests/test_gpu_guided_advance.py), the Python surface is there, and the kernel lives in the search unit."""

import ctypes
import inspect
import os
import subprocess

import pytest

from tests import kernel_units
from tests.conftest import PKG, PRODUCT_LIB, TEST_LIB

SYMBOL = "bgs_connect_guided_advance"


def test_both_libraries_export_the_guided_advance():
    for path in (PRODUCT_LIB, TEST_LIB):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert SYMBOL in {line.split()[-1] for line in out.splitlines() if line.strip()}, path


def test_the_header_declares_it():
    with open(os.path.join(os.path.dirname(PKG), "include", "bgs.h")) as f:
        text = f.read()
    assert "BGS_API int bgs_connect_guided_advance(bgs_batch* b, const int32_t* columns, int32_t capacity," in text
    assert "int32_t* kept, void* trees, size_t trees_bytes);" in text
    assert "#define BGS_GUIDED_ADVANCE_MAX_CAPACITY 65536" in text
    for word in ("the kept nodes stay in the order they were made", "no win test", "the pending leaf is dropped", "a node count above C",
                 "neither reads nor modifies the boards or bgs_steps", "Two plies", "no host variant", "RESUMES",
                 "reads neither that tree's priors row nor its values entry"):
        assert word in text, word


def test_the_binding_table_has_the_symbol():
    from simulator.game import _abi

    restype, argtypes = _abi.SIGNATURES[SYMBOL]
    assert restype is ctypes.c_int
    assert argtypes == [_abi.c_handle, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    assert _abi.GUIDED_ADVANCE_MAX_CAPACITY == 65536 <= _abi.GUIDED_MAX_CAPACITY


def test_a_null_batch_is_refused_with_a_message():
    """the NULL-batch refusal alone: a batch cannot be made without a device"""
    from simulator.game import _abi

    lib = _abi.lib()
    columns, kept, trees = (ctypes.c_int32 * 64)(), (ctypes.c_int32 * 64)(), (ctypes.c_int32 * 1024)()
    kept[:] = [5] * 64
    trees[:] = [6] * 1024
    assert lib.bgs_connect_guided_advance(None, ctypes.cast(columns, ctypes.c_void_p), 8, ctypes.cast(kept, ctypes.c_void_p),
                                          ctypes.cast(trees, ctypes.c_void_p), 4096) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error()
    assert list(kept) == [5] * 64 and list(trees) == [6] * 1024


def test_the_python_surface():
    from simulator import batch, guided

    assert issubclass(batch.GuidedForest, batch.GuidedSearch) and batch.GuidedForest.__doc__.strip()
    sig = inspect.signature(batch.GuidedForest.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("batch", inspect.Parameter.empty),
                                                                               ("capacity", inspect.Parameter.empty), ("cpuct", 320)]
    for name in ("begin", "step", "finish", "close"):          # inherited as they are
        assert getattr(batch.GuidedForest, name) is getattr(batch.GuidedSearch, name)
    sig = inspect.signature(batch.GuidedForest.advance)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("columns", inspect.Parameter.empty), ("kept", None)]
    assert list(inspect.signature(batch.GuidedForest.resume).parameters) == ["self"]
    sig = inspect.signature(batch.GuidedForest.run)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("evaluate", inspect.Parameter.empty),
                                                                               ("simulations", inspect.Parameter.empty), ("carry", False)]
    for name in ("advance", "resume", "run"):
        assert getattr(batch.GuidedForest, name).__doc__.strip()
    assert not hasattr(batch.ConnectBatch, "guided_forest")
    # a capacity above the bound of the re-rooting is refused before the batch is looked at: no device needed
    with pytest.raises(ValueError, match="65536"):
        batch.GuidedForest(None, 65537)

    assert issubclass(guided.GuidedReuseAgent, guided.GuidedSearchAgent) and guided.GuidedReuseAgent.__doc__.strip()
    assert inspect.signature(guided.GuidedReuseAgent.__init__) == inspect.signature(guided.GuidedSearchAgent.__init__)
    agent = guided.GuidedReuseAgent(lambda grid, player: None, simulations=24)
    assert agent.capacity == 49 and guided.GuidedReuseAgent(lambda grid, player: None, simulations=24, capacity=7).capacity == 7
    assert guided.GuidedSearchAgent(lambda grid, player: None, simulations=24).capacity == 25
    with pytest.raises(ValueError, match="cpuct"):
        guided.GuidedReuseAgent(lambda grid, player: None, cpuct=4097)
    with pytest.raises(TypeError, match="callable"):
        guided.GuidedReuseAgent(None)


def test_the_kernel_lives_in_the_search_unit():
    assert kernel_units.units_defining("k_connect_guided_advance") == ["search"]
