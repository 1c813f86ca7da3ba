"""CPU-only checks of the tree search's plumbing: both libraries export bgs_connect_search_actions and
bgs_connect_search_workspace_bytes, the header declares them, the version script lets them out, the ctypes binding table
has them with the header's arguments, a NULL batch is refused with BGS_ERR_ARG and a message (the one refusal that can be
reached without a device: every other argument check needs a batch and is made in tests/test_gpu_search.py), the Python
surface is there, and the kernel lives in the search unit, one of the six `make print-unit-ids` lists."""

import ctypes
import fnmatch
import inspect
import os
import re
import subprocess

import pytest

from tests import kernel_units
from tests.conftest import PKG, PRODUCT_LIB, TEST_LIB

CSRC = os.path.join(PKG, "csrc")
SYMBOLS = ("bgs_connect_search_workspace_bytes", "bgs_connect_search_actions")


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_both_libraries_export_the_search():
    for path in (PRODUCT_LIB, TEST_LIB):
        assert set(SYMBOLS) <= _exports(path), path


def test_the_version_script_lets_the_symbols_out():
    with open(os.path.join(CSRC, "bgs.map")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    patterns = re.search(r"global:(.*?);", text, flags=re.S).group(1).split()
    for name in SYMBOLS:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name


def test_the_header_declares_them():
    with open(os.path.join(os.path.dirname(PKG), "include", "bgs.h")) as f:
        text = f.read()
    assert "BGS_API int bgs_connect_search_workspace_bytes(const bgs_batch* b, int32_t iterations, size_t* bytes);" in text
    assert ("BGS_API int bgs_connect_search_actions(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, "
            "int32_t explore,") in text
    for word in ("isqrt", "lg(N)", "2^29", "2^18", "256-byte"):
        assert word in text, word


def test_the_binding_table_has_the_symbols():
    from simulator.game import _abi

    restype, argtypes = _abi.SIGNATURES["bgs_connect_search_workspace_bytes"]
    assert restype is ctypes.c_int
    assert argtypes == [_abi.c_handle, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
    restype, argtypes = _abi.SIGNATURES["bgs_connect_search_actions"]
    assert restype is ctypes.c_int
    assert argtypes == [_abi.c_handle, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int,
                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                        ctypes.c_int]


def test_a_null_batch_is_refused_with_a_message():
    """the NULL-batch refusal alone: a batch cannot be made without a device, so every other refusal of the entry points
    is checked in tests/test_gpu_search.py"""
    from simulator.game import _abi

    lib = _abi.lib()
    size = ctypes.c_size_t(77)
    assert lib.bgs_connect_search_workspace_bytes(None, 8, ctypes.byref(size)) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error() and size.value == 77
    out = (ctypes.c_int32 * 64)()
    assert lib.bgs_connect_search_actions(None, 1, 8, 8, 65536, 100, 0, ctypes.cast(out, ctypes.c_void_p), None, None, None, None, 0,
                                          0) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error() and not any(out)


def test_the_python_surface():
    from simulator import agents, batch

    for name in ("search_actions", "search_actions_tensor", "search_workspace_bytes"):
        assert callable(getattr(batch.ConnectBatch, name))
    sig = inspect.signature(batch.ConnectBatch.search_actions)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("seed", batch.DEFAULT_SEED), ("iterations", 256), ("leaf_playouts", 64), ("explore", 65536), ("max_plies", 2**31 - 1),
        ("policy", "uniform")]
    # Bounce refuses before it looks at the batch: no device needed
    for name in ("search_actions", "search_actions_tensor", "search_workspace_bytes"):
        with pytest.raises(ValueError, match="Connect batches only"):
            getattr(batch.BounceBatch, name)(None, iterations=8)
    sig = inspect.signature(agents.TreeSearchAgent.__init__)
    assert list(sig.parameters)[1:5] == ["iterations", "leaf_playouts", "explore", "policy"]
    for name in ("predict", "choose", "choose_many", "predict_many", "close"):
        assert callable(getattr(agents.TreeSearchAgent, name))
    with pytest.raises(ValueError, match="policy"):
        agents.TreeSearchAgent(policy="greedy")
    with pytest.raises(ValueError, match="explore"):
        agents.TreeSearchAgent(explore=(1 << 18) + 1)


def test_the_kernel_lives_in_the_search_unit_of_six():
    kernel_units.check_six_distinct_ids()
    assert kernel_units.units_defining("k_connect_search") == ["search"]
