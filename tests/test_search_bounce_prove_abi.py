"""CPU-only checks of the Bounce proving tree search's plumbing: both libraries export bgs_bounce_search_moves_proving,
the header declares it with its contract, the version script lets it out, the ctypes binding table has it with the header's
arguments, a NULL batch is refused with BGS_ERR_ARG and a message (the one refusal that can be reached without a device:
every other argument check needs a batch and is made in tests/test_gpu_search_bounce_prove.py), the Python surface is there
-- the Connect refusal and the `prove` with `reuse` refusal included --, and the proving search is a form of
k_bounce_search in the evaluate unit."""

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
SYMBOL = "bgs_bounce_search_moves_proving"


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
    assert ("BGS_API int bgs_bounce_search_moves_proving(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, "
            "int32_t explore, int32_t max_plies, int policy, int32_t edges, int32_t* counts, int32_t* visits, int32_t* best, "
            "int32_t* nodes, int32_t* used, int8_t* proved, int32_t* done, void* workspace, size_t workspace_bytes, "
            "int on_device);") in flat
    start = text.index("the sibling of bgs_connect_search_actions_proving")
    contract = text[start:text.index("BGS_API int bgs_bounce_search_moves_proving")]
    contract = re.sub(r"\s*\n \*\s*", " ", contract)
    for word in ("OPEN", "proved", "done", "WIN", "DRAW", "LOSS", "BGS_SOLVE_UNKNOWN", "BGS_SOLVE_NONE", "bgs_bounce_search_workspace_bytes",
                 "holds the cap", "did not fit the pool", "path_node[k]", "negation", "bit for bit"):
        assert word in contract, word
    assert "Bounce do not prove" not in text
    with open(os.path.join(CSRC, "bgs_internal.h")) as f:
        assert "void bounce_search_proving(" in f.read()


def test_the_binding_table_has_the_symbol():
    from simulator.game import _abi

    restype, argtypes = _abi.SIGNATURES[SYMBOL]
    assert restype is ctypes.c_int
    # the plain entry point with proved and done put in before the workspace
    plain = _abi.SIGNATURES["bgs_bounce_search_moves"][1]
    assert len(plain) == 16 and len(argtypes) == 18
    assert argtypes == plain[:13] + [ctypes.c_void_p, ctypes.c_void_p] + plain[13:]


def test_a_null_batch_is_refused_with_a_message():
    from simulator.game import _abi

    lib = _abi.lib()
    outs = [(ctypes.c_int32 * 64)() for _ in range(6)]
    proved = (ctypes.c_int8 * 64)()
    ptr = [ctypes.cast(o, ctypes.c_void_p) for o in outs[:5]] + [ctypes.cast(proved, ctypes.c_void_p), ctypes.cast(outs[5], ctypes.c_void_p)]
    assert lib.bgs_bounce_search_moves_proving(None, 1, 8, 8, 65536, 100, 0, 1000, *ptr, None, 0, 0) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error()
    assert not any(any(o) for o in outs) and not any(proved)


def test_the_python_surface():
    from simulator import agents, batch

    for name in ("search_moves_proving", "search_moves_proving_tensor"):
        assert callable(getattr(batch.BounceBatch, name))
    proving = inspect.signature(batch.BounceBatch.search_moves_proving)
    plain = inspect.signature(batch.BounceBatch.search_moves)
    assert [(p.name, p.default) for p in proving.parameters.values()] == [(p.name, p.default) for p in plain.parameters.values()]
    tensor = inspect.signature(batch.BounceBatch.search_moves_proving_tensor)
    assert list(tensor.parameters)[1:8] == ["counts", "visits", "best", "nodes", "used", "proved", "done"]
    assert "workspace" in tensor.parameters and "edges" in tensor.parameters
    # Connect refuses before it looks at the batch: no device needed
    for name in ("search_moves_proving", "search_moves_proving_tensor"):
        with pytest.raises(ValueError, match="Bounce batches only"):
            getattr(batch.ConnectBatch, name)(None, iterations=8)
    sig = inspect.signature(agents.BounceTreeSearchAgent.__init__)
    names = list(sig.parameters)
    assert names[1:5] == ["iterations", "leaf_playouts", "explore", "policy"] and names[-3:] == ["prove", "reuse", "capacity"]
    assert sig.parameters["prove"].default is False
    assert agents.BounceTreeSearchAgent().prove is False and agents.BounceTreeSearchAgent(prove=True).prove is True
    with pytest.raises(ValueError, match="forest does not prove"):
        agents.BounceTreeSearchAgent(prove=True, reuse=True)


def test_the_proving_search_is_a_form_of_the_search_kernel():
    with open(kernel_units.source("search")) as f:
        text = f.read()
    kernel = text[text.index("k_bounce_search(GEO g"):text.index("struct BounceSearchArgs")]
    assert "template <class GEO, int NC, int POLICY, bool FOREST, bool PROVE = false>" in text
    assert "static_assert(!(PROVE && FOREST)" in kernel and "if constexpr (PROVE)" in kernel
    assert "bounce_search_proving" in text
    assert kernel_units.kernel_files() == sorted(f"{unit}_kernels.hip" for unit in kernel_units.UNITS)
    assert not [name for name in os.listdir(CSRC) if "prov" in name]
