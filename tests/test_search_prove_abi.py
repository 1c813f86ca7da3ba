"""CPU-only checks of the proving tree search's plumbing: both libraries export bgs_connect_search_actions_proving, the
header declares it with its contract, the version script lets it out, the ctypes binding table has it with the header's
arguments, a NULL batch is refused with BGS_ERR_ARG and a message (the one refusal that can be reached without a device:
every other argument check needs a batch and is made in tests/test_gpu_search_prove.py), the Python surface is there --
the Bounce refusal and the `prove` with `reuse` refusal included --, and `make print-unit-ids` lists the six units, none of them the proving search's own."""

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
SYMBOL = "bgs_connect_search_actions_proving"


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_both_libraries_export_the_symbol():
    for path in (PRODUCT_LIB, TEST_LIB):
        assert SYMBOL in _exports(path), path


def test_the_version_script_lets_the_symbol_out():
    with open(os.path.join(CSRC, "bgs.map")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    patterns = re.search(r"global:(.*?);", text, flags=re.S).group(1).split()
    assert any(fnmatch.fnmatchcase(SYMBOL, p) for p in patterns)


def test_the_header_declares_it_with_its_contract():
    with open(os.path.join(os.path.dirname(PKG), "include", "bgs.h")) as f:
        text = f.read()
    flat = re.sub(r"\s+", " ", text)
    assert ("BGS_API int bgs_connect_search_actions_proving(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, "
            "int32_t explore, int32_t max_plies, int policy, int32_t* counts, int32_t* visits, int32_t* best, int32_t* nodes, "
            "int8_t* proved, int32_t* done, void* workspace, size_t workspace_bytes, int on_device);") in flat
    contract = text[text.index("proving wins, draws and losses"):text.index("BGS_API int bgs_connect_search_actions_proving")]
    for word in ("OPEN", "proved", "done", "WIN", "DRAW", "LOSS", "BGS_SOLVE_UNKNOWN", "BGS_SOLVE_NONE", "bgs_connect_search_workspace_bytes"):
        assert word in contract, word
    with open(os.path.join(CSRC, "bgs_internal.h")) as f:
        assert "void connect_search_proving(" in f.read()


def test_the_binding_table_has_the_symbol():
    from simulator.game import _abi

    restype, argtypes = _abi.SIGNATURES[SYMBOL]
    assert restype is ctypes.c_int
    assert argtypes == [_abi.c_handle, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int,
                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    # the plain entry point with proved and done put in before the workspace
    plain = _abi.SIGNATURES["bgs_connect_search_actions"][1]
    assert argtypes == plain[:11] + [ctypes.c_void_p, ctypes.c_void_p] + plain[11:]


def test_a_null_batch_is_refused_with_a_message():
    from simulator.game import _abi

    lib = _abi.lib()
    outs = [(ctypes.c_int32 * 64)() for _ in range(5)]
    proved = (ctypes.c_int8 * 64)()
    ptr = [ctypes.cast(o, ctypes.c_void_p) for o in outs[:4]] + [ctypes.cast(proved, ctypes.c_void_p), ctypes.cast(outs[4], ctypes.c_void_p)]
    assert lib.bgs_connect_search_actions_proving(None, 1, 8, 8, 65536, 100, 0, *ptr, None, 0, 0) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error()
    assert not any(any(o) for o in outs) and not any(proved)


def test_the_python_surface():
    from simulator import agents, batch

    for name in ("search_actions_proving", "search_actions_proving_tensor"):
        assert callable(getattr(batch.ConnectBatch, name))
    proving = inspect.signature(batch.ConnectBatch.search_actions_proving)
    plain = inspect.signature(batch.ConnectBatch.search_actions)
    assert [(p.name, p.default) for p in proving.parameters.values()] == [(p.name, p.default) for p in plain.parameters.values()]
    assert [(p.name, p.default) for p in list(proving.parameters.values())[1:]] == [
        ("seed", batch.DEFAULT_SEED), ("iterations", 256), ("leaf_playouts", 64), ("explore", 65536), ("max_plies", 2**31 - 1),
        ("policy", "uniform")]
    tensor = inspect.signature(batch.ConnectBatch.search_actions_proving_tensor)
    assert list(tensor.parameters)[1:7] == ["counts", "visits", "best", "nodes", "proved", "done"] and "workspace" in tensor.parameters
    # Bounce refuses before it looks at the batch: no device needed
    for name in ("search_actions_proving", "search_actions_proving_tensor"):
        with pytest.raises(ValueError, match="Connect batches only"):
            getattr(batch.BounceBatch, name)(None, iterations=8)
    names = list(inspect.signature(agents.TreeSearchAgent.__init__).parameters)
    assert names[1:5] == ["iterations", "leaf_playouts", "explore", "policy"] and names[-2:] == ["reuse", "capacity"]
    assert names[names.index("max_plies") + 1] == "prove" and names[names.index("prove") + 1] == "reuse"
    assert inspect.signature(agents.TreeSearchAgent.__init__).parameters["prove"].default is False
    assert agents.TreeSearchAgent().prove is False and agents.TreeSearchAgent(prove=True).prove is True
    with pytest.raises(ValueError, match="forest does not prove"):
        agents.TreeSearchAgent(prove=True, reuse=True)


def test_the_proving_search_has_no_kernel_unit_of_its_own():
    kernel_units.check_six_distinct_ids()
    # the proving search is a form of k_connect_search in the search unit, not a kernel file of its own
    with open(kernel_units.source("search")) as f:
        text = f.read()
    assert "bool PROVE" in text and "connect_search_proving" in text
    assert kernel_units.kernel_files() == sorted(f"{unit}_kernels.hip" for unit in kernel_units.UNITS)
    assert not [name for name in os.listdir(CSRC) if "prov" in name]
