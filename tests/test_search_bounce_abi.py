"""CPU-only checks of the Bounce tree search's plumbing: both libraries export bgs_bounce_search_moves and
bgs_bounce_search_workspace_bytes, the header declares them verbatim, the version script lets them out, the ctypes binding
table has them with the header's argument counts, a NULL batch is refused with BGS_ERR_ARG and a message (the one refusal
that can be reached without a device: every other argument check needs a batch and is made in
tests/test_gpu_search_bounce.py), the Python surface is there, and the kernel lives in the search unit, one of the six `make
print-unit-ids` lists."""

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
SYMBOLS = ("bgs_bounce_search_workspace_bytes", "bgs_bounce_search_moves")
DECLARATIONS = (
    "BGS_API int bgs_bounce_search_workspace_bytes(const bgs_batch* b, int32_t iterations, int32_t edges, size_t* bytes);",
    "BGS_API int bgs_bounce_search_moves(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore,\n"
    "                                    int32_t max_plies, int policy, int32_t edges, int32_t* counts, int32_t* visits,\n"
    "                                    int32_t* best, int32_t* nodes, int32_t* used, void* workspace, size_t workspace_bytes,\n"
    "                                    int on_device);",
)


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def _header():
    with open(os.path.join(os.path.dirname(PKG), "include", "bgs.h")) as f:
        return f.read()


def test_both_libraries_export_the_search():
    for path in (PRODUCT_LIB, TEST_LIB):
        assert set(SYMBOLS) <= _exports(path), path


def test_the_version_script_lets_the_symbols_out():
    with open(os.path.join(CSRC, "bgs.map")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    patterns = re.search(r"global:(.*?);", text, flags=re.S).group(1).split()
    for name in SYMBOLS:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name


def test_the_header_declares_them_verbatim():
    text = _header()
    for declaration in DECLARATIONS:
        assert declaration in text, declaration
    assert "#define BGS_BOUNCE_SEARCH_MIN_EDGES(h, w) ((h) >= 3 ? (w) * (w) * ((h) - 2) : 1)" in text
    # the contract says where it leaves the Connect search, and what the workspace holds
    for word in ("THIS DIFFERS", "has no child", "tried again", "16 * E", "8 * (T + 1)", "4 * (T + 1)", "256-byte", "2^29", "2^18"):
        assert word in text, word


def test_the_binding_table_has_the_headers_argument_counts():
    from simulator.game import _abi

    text = _header()
    for name in SYMBOLS:
        restype, argtypes = _abi.SIGNATURES[name]
        assert restype is ctypes.c_int
        declared = re.search(rf"BGS_API int {name}\((.*?)\);", text, flags=re.S).group(1)
        assert len(argtypes) == len(declared.split(",")), name
    assert _abi.SIGNATURES[SYMBOLS[0]][1] == [_abi.c_handle, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
    assert _abi.SIGNATURES[SYMBOLS[1]][1] == [
        _abi.c_handle, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int, ctypes.c_int32,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
        ctypes.c_int]


def test_a_null_batch_is_refused_with_a_message():
    from simulator.game import _abi

    lib = _abi.lib()
    size = ctypes.c_size_t(77)
    assert lib.bgs_bounce_search_workspace_bytes(None, 8, 1000, ctypes.byref(size)) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error() and size.value == 77
    out = (ctypes.c_int32 * 64)()
    assert lib.bgs_bounce_search_moves(None, 1, 8, 8, 65536, 100, 0, 1000, ctypes.cast(out, ctypes.c_void_p), None, None, None, None,
                                       None, 0, 0) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error() and not any(out)


def test_the_python_surface():
    from simulator import agents, batch

    for name in ("search_moves", "search_moves_tensor", "search_moves_workspace_bytes"):
        assert callable(getattr(batch.BounceBatch, name))
        with pytest.raises(ValueError, match="Bounce batches only"):   # Connect refuses before it looks at the batch
            getattr(batch.ConnectBatch, name)(None, iterations=8)
    sig = inspect.signature(batch.BounceBatch.search_moves)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("seed", batch.DEFAULT_SEED), ("iterations", 256), ("leaf_playouts", 64), ("explore", 65536), ("max_plies", 2**31 - 1),
        ("policy", "uniform"), ("edges", None)]
    assert "workspace" in inspect.signature(batch.BounceBatch.search_moves_tensor).parameters
    assert "not measured" in batch.BounceBatch.search_moves.__doc__ and "section 28" in batch.BounceBatch.search_moves.__doc__
    # the existing names keep refusing Bounce
    for name in ("search_actions", "search_actions_tensor", "search_workspace_bytes"):
        with pytest.raises(ValueError, match="Connect batches only"):
            getattr(batch.BounceBatch, name)(None, iterations=8)
    sig = inspect.signature(agents.BounceTreeSearchAgent.__init__)
    assert list(sig.parameters)[1:5] == ["iterations", "leaf_playouts", "explore", "policy"]
    for name in ("predict", "choose", "choose_many", "predict_many", "close"):
        assert callable(getattr(agents.BounceTreeSearchAgent, name))
    agent = agents.BounceTreeSearchAgent()
    assert agent.predict_many([]) == [] and agent.choose_many([]) == []
    with pytest.raises(ValueError, match="policy"):
        agents.BounceTreeSearchAgent(policy="greedy")
    with pytest.raises(ValueError, match="explore"):
        agents.BounceTreeSearchAgent(explore=(1 << 18) + 1)
    with pytest.raises(ValueError, match="iterations"):
        agents.BounceTreeSearchAgent(iterations=0)


def test_the_kernel_lives_in_the_search_unit():
    with open(kernel_units.source("search")) as f:
        assert "k_bounce_search(" in f.read()
    assert kernel_units.units_defining("k_bounce_search") == ["search"]   # that unit's object and no other
    kernel_units.check_six_distinct_ids()
