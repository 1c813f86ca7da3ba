"""CPU-only checks of the guided search's plumbing: both libraries export bgs_connect_guided_bytes and
bgs_connect_guided_step, the header declares them with their constants and their contract, the ctypes binding table has
them with the header's arguments, a NULL batch is refused with BGS_ERR_ARG and a message (the one refusal that can be
reached without a device: every other one is made in tests/test_gpu_guided.py), the Python surface is there, and the
kernel lives in the search unit, one of the six `make print-unit-ids` lists."""

import ctypes
import inspect
import os
import subprocess

import pytest

from tests import kernel_units
from tests.conftest import PKG, PRODUCT_LIB, TEST_LIB

SYMBOLS = ("bgs_connect_guided_bytes", "bgs_connect_guided_step")


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_both_libraries_export_the_guided_search():
    for path in (PRODUCT_LIB, TEST_LIB):
        assert set(SYMBOLS) <= _exports(path), path


def test_the_header_declares_them():
    with open(os.path.join(os.path.dirname(PKG), "include", "bgs.h")) as f:
        text = f.read()
    assert "BGS_API int bgs_connect_guided_bytes(const bgs_batch* b, int32_t capacity, size_t* bytes);" in text
    assert "BGS_API int bgs_connect_guided_step(bgs_batch* b, int32_t capacity, int32_t cpuct, uint32_t flags," in text
    for line in ("#define BGS_GUIDED_RESTART 1u", "#define BGS_GUIDED_FINISH  2u", "#define BGS_GUIDED_EVALUATE 0",
                 "#define BGS_GUIDED_TERMINAL 1", "#define BGS_GUIDED_IDLE     2", "#define BGS_GUIDED_MAX_CAPACITY (1 << 20)",
                 "#define BGS_GUIDED_MAX_VISITS   (1 << 19)"):
        assert line in text, line
    for word in ("isqrt((N + 1) << 12)", ">> 19", "65536.0f", "1024.0f", "2048 - sigma", "no host variant", "256-byte",
                 "MUST PASS BGS_GUIDED_RESTART"):
        assert word in text, word


def test_the_binding_table_has_the_symbols():
    from simulator.game import _abi

    restype, argtypes = _abi.SIGNATURES["bgs_connect_guided_bytes"]
    assert restype is ctypes.c_int
    assert argtypes == [_abi.c_handle, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
    restype, argtypes = _abi.SIGNATURES["bgs_connect_guided_step"]
    assert restype is ctypes.c_int
    assert argtypes == [_abi.c_handle, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32] + [ctypes.c_void_p] * 10 + [ctypes.c_size_t]
    assert (_abi.GUIDED_RESTART, _abi.GUIDED_FINISH) == (1, 2)
    assert (_abi.GUIDED_EVALUATE, _abi.GUIDED_TERMINAL, _abi.GUIDED_IDLE) == (0, 1, 2)
    assert (_abi.GUIDED_MAX_CAPACITY, _abi.GUIDED_MAX_VISITS) == (1 << 20, 1 << 19)


def test_a_null_batch_is_refused_with_a_message():
    """the NULL-batch refusal alone: a batch cannot be made without a device"""
    from simulator.game import _abi

    lib = _abi.lib()
    size = ctypes.c_size_t(77)
    assert lib.bgs_connect_guided_bytes(None, 8, ctypes.byref(size)) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error() and size.value == 77
    outs = [(ctypes.c_int32 * 64)() for _ in range(8)]
    for out in outs:
        out[:] = [5] * 64
    pointers = [ctypes.cast(out, ctypes.c_void_p) for out in outs]
    assert lib.bgs_connect_guided_step(None, 8, 320, _abi.GUIDED_RESTART, None, None, *pointers, 64 * 4) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error()
    assert all(list(out) == [5] * 64 for out in outs)


def test_the_python_surface():
    from simulator import batch, guided

    assert callable(batch.ConnectBatch.guided_search) and callable(batch.ConnectBatch.guided_bytes)
    sig = inspect.signature(batch.ConnectBatch.guided_search)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("capacity", inspect.Parameter.empty), ("cpuct", 320)]
    for name in ("begin", "step", "finish", "run", "close"):
        assert callable(getattr(batch.GuidedSearch, name))
    assert list(inspect.signature(batch.GuidedSearch.step).parameters)[1:] == ["priors", "values"]
    assert list(inspect.signature(batch.GuidedSearch.finish).parameters)[1:] == ["priors", "values"]
    assert list(inspect.signature(batch.GuidedSearch.run).parameters)[1:] == ["evaluate", "simulations"]
    assert (batch.GUIDED_EVALUATE, batch.GUIDED_TERMINAL, batch.GUIDED_IDLE) == (0, 1, 2)
    # Bounce refuses before it looks at the batch: no device needed
    for name in ("guided_search", "guided_bytes"):
        with pytest.raises(ValueError, match="Connect batches only"):
            getattr(batch.BounceBatch, name)(None, 64)
    sig = inspect.signature(guided.GuidedSearchAgent.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("evaluate", inspect.Parameter.empty), ("simulations", 128), ("cpuct", 320), ("capacity", None), ("device", 0)]
    for name in ("search", "predict_many", "choose_many", "predict", "choose", "close"):
        assert callable(getattr(guided.GuidedSearchAgent, name))
    with pytest.raises(ValueError, match="cpuct"):
        guided.GuidedSearchAgent(lambda grid, player: None, cpuct=4097)
    with pytest.raises(ValueError, match="simulations"):
        guided.GuidedSearchAgent(lambda grid, player: None, simulations=0)
    with pytest.raises(TypeError, match="callable"):
        guided.GuidedSearchAgent(None)


def test_the_kernel_lives_in_the_search_unit_of_six():
    kernel_units.check_six_distinct_ids()
    assert kernel_units.units_defining("k_connect_search_guided") == ["search"]
