"""CPU-only checks of the Bounce guided search's plumbing: both libraries export bgs_bounce_guided_bytes and
bgs_bounce_guided_step, the header declares them and carries the contract's key phrases, the ctypes binding table has
them with the header's arguments, a NULL batch is refused with BGS_ERR_ARG and a message (the one refusal that can be
reached without a device: every other one is made in tests/test_gpu_bounce_guided.py), the Python surface and the agent's
signature are there, and the kernel lives in the search unit, one of the six `make print-unit-ids` lists."""

import ctypes
import inspect
import os
import subprocess

import pytest

from tests import kernel_units
from tests.conftest import PKG, PRODUCT_LIB, TEST_LIB

SYMBOLS = ("bgs_bounce_guided_bytes", "bgs_bounce_guided_step")


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_both_libraries_export_the_bounce_guided_search():
    for path in (PRODUCT_LIB, TEST_LIB):
        assert set(SYMBOLS) <= _exports(path), path


def test_the_header_declares_them():
    with open(os.path.join(os.path.dirname(PKG), "include", "bgs.h")) as f:
        text = f.read()
    assert "BGS_API int bgs_bounce_guided_bytes(const bgs_batch* b, int32_t nodes, int32_t edges, size_t* bytes);" in text
    assert ("BGS_API int bgs_bounce_guided_step(bgs_batch* b, int32_t nodes_cap, int32_t edges, int32_t cpuct, int32_t max_plies,\n"
            "                                   uint32_t flags, const float* priors, const float* values,\n"
            "                                   int8_t* leaf_grid, int8_t* leaf_player, int32_t* leaf_kind, uint64_t* leaf_targets,\n"
            "                                   int32_t* visits, int32_t* scores, int32_t* best, int32_t* nodes, int32_t* used,\n"
            "                                   void* trees, size_t trees_bytes);") in text
    contract = text[text.index("the sibling of\n * bgs_connect_guided_step"):text.index("BGS_API int bgs_bounce_guided_bytes")]
    for word in ("S = width * height * width", "ascending slot", "priors float32[n][S]", "BGS_BOUNCE_FOREST_MAX_NODES",
                 "BGS_BOUNCE_SEARCH_MIN_EDGES(height, width) <= E <= BGS_BOUNCE_FOREST_MAX_EDGES", "min(max_plies, 65535)",
                 "fewer than\n *      65535 plies", "MUST PASS BGS_GUIDED_RESTART", "never a store outside its own share",
                 "65536.0f", "P = floor(w * 65536 / W)", "holds the cap", "(edges in use) +\n *      A(leaf) <= E", "2048 - sigma",
                 "zeros\n *      on illegal slots", "BGS_GUIDED_MAX_VISITS", "no unplayed-arm-first rule", "capped sentinel",
                 "leaf_targets uint64[n][w] (may be NULL)", "bgs_bounce_read_targets", "IDLE rows carry the root's grid and player",
                 "no host variant", "256-byte", "max_plies < 1", "names the argument"):
        assert word in contract, word


def test_the_binding_table_has_the_symbols():
    from simulator.game import _abi

    restype, argtypes = _abi.SIGNATURES["bgs_bounce_guided_bytes"]
    assert restype is ctypes.c_int
    assert argtypes == [_abi.c_handle, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
    restype, argtypes = _abi.SIGNATURES["bgs_bounce_guided_step"]
    assert restype is ctypes.c_int
    assert argtypes == [_abi.c_handle] + [ctypes.c_int32] * 4 + [ctypes.c_uint32] + [ctypes.c_void_p] * 12 + [ctypes.c_size_t]


def test_a_null_batch_is_refused_with_a_message():
    """the NULL-batch refusal alone: a batch cannot be made without a device"""
    from simulator.game import _abi

    lib = _abi.lib()
    size = ctypes.c_size_t(77)
    assert lib.bgs_bounce_guided_bytes(None, 8, 512, ctypes.byref(size)) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error() and size.value == 77
    outs = [(ctypes.c_int32 * 64)() for _ in range(10)]
    for out in outs:
        out[:] = [5] * 64
    pointers = [ctypes.cast(out, ctypes.c_void_p) for out in outs]
    assert lib.bgs_bounce_guided_step(None, 8, 512, 320, 65535, _abi.GUIDED_RESTART, None, None, *pointers, 64 * 4) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error()
    assert all(list(out) == [5] * 64 for out in outs)


def test_the_python_surface():
    from simulator import batch, guided

    def parameters(f):
        return [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[1:]]

    assert parameters(batch.BounceBatch.guided_moves_bytes) == [("nodes", inspect.Parameter.empty), ("edges", None)]
    assert parameters(batch.BounceBatch.guided_moves_search) == [("nodes", inspect.Parameter.empty), ("edges", None), ("cpuct", 320),
                                                                 ("max_plies", 65535)]
    for name in ("begin", "step", "finish", "run", "close"):
        assert callable(getattr(batch.GuidedMovesSearch, name))
    assert list(inspect.signature(batch.GuidedMovesSearch.step).parameters)[1:] == ["priors", "values"]
    assert list(inspect.signature(batch.GuidedMovesSearch.finish).parameters)[1:] == ["priors", "values"]
    assert list(inspect.signature(batch.GuidedMovesSearch.run).parameters)[1:] == ["evaluate", "simulations"]
    # the Connect calls keep refusing Bounce, and say where to go in their docstring only
    for name in ("guided_search", "guided_bytes"):
        with pytest.raises(ValueError, match="^guided_search: Connect batches only$"):
            getattr(batch.BounceBatch, name)(None, 64)
    assert "guided_moves_search" in batch.BounceBatch.guided_search.__doc__
    # Connect has no slots: the Bounce calls are not there
    assert not hasattr(batch.ConnectBatch, "guided_moves_search")
    assert parameters(guided.BounceGuidedSearchAgent.__init__) == [
        ("evaluate", inspect.Parameter.empty), ("simulations", 128), ("cpuct", 320), ("nodes", None), ("edges", None),
        ("max_plies", 65535), ("device", 0)]
    for name in ("search", "predict_many", "choose_many", "predict", "choose", "close"):
        assert callable(getattr(guided.BounceGuidedSearchAgent, name))
    with pytest.raises(ValueError, match="cpuct"):
        guided.BounceGuidedSearchAgent(lambda grid, player, targets: None, cpuct=4097)
    with pytest.raises(ValueError, match="simulations"):
        guided.BounceGuidedSearchAgent(lambda grid, player, targets: None, simulations=0)
    with pytest.raises(ValueError, match="max_plies"):
        guided.BounceGuidedSearchAgent(lambda grid, player, targets: None, max_plies=0)
    with pytest.raises(TypeError, match="callable"):
        guided.BounceGuidedSearchAgent(None)
    # GuidedSearchAgent stays as it was: Connect only, the capacity its one size
    assert [name for name, _ in parameters(guided.GuidedSearchAgent.__init__)] == ["evaluate", "simulations", "cpuct", "capacity", "device"]


def test_the_kernel_lives_in_the_search_unit_of_six():
    kernel_units.check_six_distinct_ids()
    assert kernel_units.units_defining("k_bounce_search_guided") == ["search"]
