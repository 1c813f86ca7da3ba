"""The output plumbing of the analysis calls (csrc/output_plan.h, run_outputs in bgs_capi.hip) through the C ABI itself:
every evaluation, search, forest-search and solver entry point of both games, on n = 5 boards -- so that n * 4 and
n * width are no multiples of 16 and the slices of the host path are rounded -- with all outputs, with each optional
output NULL in turn and with all of them NULL.  An output that is asked for equals the full call's bit for bit.  The
searches repeat this with the caller's workspace and with the library's own.  The device path runs once with every
optional output NULL and gives the host call's counts (the solvers: codes).  The refusals of a misaligned device pointer,
a misaligned workspace and a NULL forest keep their texts and write nothing.  What the calls compute is stated by the
other test_gpu_* files; tests/test_output_plan.py sweeps the layout on the CPU.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes
from typing import NamedTuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 5
SEED, EXPLORE, MAX_PLIES, ITERATIONS, LEAF = 0x5EED, 65536, 100, 8, 8
CAPACITY = ITERATIONS + 1          # nodes a tree of a forest holds: the root and one node an iteration
DEPTH, MAX_NODES = 3, 1 << 20      # the solvers' horizon and budget
FILL = -5


class Call(NamedTuple):
    fn: str          # the symbol
    head: tuple      # the arguments between the handle and the outputs
    outputs: tuple   # (name, shape, dtype, optional), in the ABI's order
    tail: str        # what follows the outputs: "" nothing, "workspace" or "forest" (pointer, bytes)


def connect_batch():
    from simulator.batch import ConnectBatch

    b = ConnectBatch(6, 7, 4, N, use_torch=True)
    b.step_random(seed=3, plies=6)
    return b


def bounce_batch():
    from simulator.batch import BounceBatch

    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    b = BounceBatch(grid, N, use_torch=True)
    b.step_random(seed=3, plies=3)
    return b


def calls(game):
    from simulator.game import _abi

    D = _abi.POLICY_DECISIVE
    if game == "connect":
        cells, entry, edges = (N, 7), "bgs_connect_", ()
        names = dict(evaluate="evaluate_actions", search="search_actions", solve="solve_actions")
        budget = 7 * 3                                         # width * ceil(log2 width): the least the halving takes
    else:
        cells, entry, edges = (N, 6, 54), "bgs_bounce_", (6 * 6 * 7,)   # BGS_BOUNCE_SEARCH_MIN_EDGES(9, 6)
        names = dict(evaluate="evaluate_moves", search="search_moves", solve="solve_moves")
        budget = 1
    counts, board = ("counts", cells + (3,), "int32", False), (N,)
    tree = (counts, ("visits", cells, "int32", True), ("best", board, "int32", True), ("nodes", board, "int32", True))
    if game == "bounce":
        tree += (("used", board, "int32", True),)
    search = (SEED, ITERATIONS, LEAF, EXPLORE, MAX_PLIES, D)
    return [
        Call(entry + names["evaluate"], (SEED, 1, MAX_PLIES), (counts,), ""),
        Call(entry + names["evaluate"] + "_policy", (SEED, 1, MAX_PLIES, D), (counts,), ""),
        Call(entry + names["evaluate"] + "_halving", (SEED, budget, MAX_PLIES, D),
             (counts, ("given", cells, "int32", True), ("best", board, "int32", True)), ""),
        Call(entry + names["search"], search + edges, tree, "workspace"),
        Call(entry + names["search"] + "_proving", search + edges,
             tree + (("proved", cells, "int8", True), ("done", board, "int32", True)), "workspace"),
        Call(entry + "forest_search", search + (CAPACITY,) + edges + (1,), tree + (("carried", board, "int32", True),), "forest"),
        Call(entry + names["solve"], (DEPTH, MAX_NODES),
             (("codes", cells, "int8", False), ("plies", cells, "int16", True), ("nodes", (1,), "uint64", True)), ""),
    ]


CASES = [(game, k) for game in ("connect", "bounce") for k in range(7)]


def case_id(case):
    return calls(case[0])[case[1]].fn


def run(b, call, absent=(), tail=(), on_device=False):
    """one call; {name: array} of the outputs asked for (device tensors come back as numpy arrays)"""
    import torch

    from simulator.game import _abi

    outs, pointers = {}, []
    for name, shape, dtype, _ in call.outputs:
        if name in absent:
            pointers.append(None)
        elif on_device:
            outs[name] = torch.full(shape, FILL, dtype=getattr(torch, dtype), device="cuda:0")
            pointers.append(ctypes.c_void_p(outs[name].data_ptr()))
        else:
            outs[name] = np.full(shape, FILL if dtype != "uint64" else 5, dtype=dtype)
            pointers.append(ctypes.c_void_p(outs[name].ctypes.data))
    rc = getattr(_abi.lib(), call.fn)(b._handle, *call.head, *pointers, *tail, 1 if on_device else 0)
    assert rc == _abi.BGS_OK, f"{call.fn} absent {absent}: {_abi.last_error()}"
    if on_device:
        torch.cuda.synchronize()
        outs = {name: x.cpu().numpy() for name, x in outs.items()}
    return outs


def tails(b, call, game):
    """[(what, tail arguments, something to keep alive)]: the workspaces or the forest a call is tried with"""
    import torch

    if call.tail == "":
        return [("", (), None)]
    if call.tail == "workspace":
        need = b.search_workspace_bytes(ITERATIONS) if game == "connect" else b.search_moves_workspace_bytes(ITERATIONS, call.head[-1])
        own = torch.empty(need, dtype=torch.uint8, device="cuda:0")
        assert own.data_ptr() % 256 == 0
        return [("the library's workspace", (None, 0), None), ("the caller's workspace", (ctypes.c_void_p(own.data_ptr()), need), own)]
    need = b.forest_bytes(CAPACITY) if game == "connect" else b.moves_forest_bytes(CAPACITY, call.head[-2])
    forest = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
    assert forest.data_ptr() % 256 == 0
    return [("a forest", (ctypes.c_void_p(forest.data_ptr()), need), forest)]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_subset_of_optional_outputs_equals_the_full_call(case):
    game, k = case
    b = connect_batch() if game == "connect" else bounce_batch()
    call = calls(game)[k]
    optional = [name for name, _, _, opt in call.outputs if opt]
    required = call.outputs[0][0]
    subsets = [(name,) for name in optional] + ([tuple(optional)] if len(optional) > 1 else [])
    full = None
    for what, tail, _keep in tails(b, call, game):
        got = run(b, call, tail=tail)
        if full is None:
            full = got
            assert any((x != (FILL if x.dtype != np.uint64 else 5)).any() for x in full.values()), "the call wrote nothing"
        for name in full:                                      # (the second workspace: the same results)
            np.testing.assert_array_equal(got[name], full[name], err_msg=f"{call.fn} {name}, {what}")
        for absent in subsets:
            part = run(b, call, absent=absent, tail=tail)
            assert sorted(part) == sorted(set(full) - set(absent))
            for name in part:
                np.testing.assert_array_equal(part[name], full[name], err_msg=f"{call.fn} {name} without {absent}, {what}")
    # the device path, every optional output NULL (the searches: the caller's workspace, which that path requires)
    _, tail, _keep = tails(b, call, game)[-1]
    device = run(b, call, absent=tuple(optional), tail=tail, on_device=True)
    assert list(device) == [required]
    np.testing.assert_array_equal(device[required], full[required], err_msg=f"{call.fn} {required} on the device")
    b.close()


@pytest.mark.parametrize("game", ["connect", "bounce"])
def test_the_refusals_keep_their_texts_and_write_nothing(game):
    import torch

    from simulator.game import _abi

    lib = _abi.lib()
    b = connect_batch() if game == "connect" else bounce_batch()
    _, _, _, search, proving, forest_search, solve = calls(game)
    sizing = f"bgs_{game}_forest_bytes"

    def refused(text, call, pointers, tail, on_device, watched):
        rc = getattr(lib, call.fn)(b._handle, *call.head, *pointers, *tail, on_device)
        assert rc == _abi.BGS_ERR_ARG and _abi.last_error() == text, (call.fn, rc, _abi.last_error())
        torch.cuda.synchronize()
        assert all(bool((x == FILL).all()) for x in watched), f"{call.fn}: a refused call wrote"

    def device_outputs(call, bump_name=None, bump=0):
        tensors = [torch.full((int(np.prod(shape)) * np.dtype(dtype).itemsize + 16,), FILL, dtype=torch.int8, device="cuda:0")
                   for _, shape, dtype, _ in call.outputs]
        where = [ctypes.c_void_p(x.data_ptr() + (bump if name == bump_name else 0)) for x, (name, _, _, _) in zip(tensors, call.outputs)]
        return tensors, where

    for call in (search, proving, forest_search):
        _, tail, keep = tails(b, call, game)[-1]
        keep = keep.view(torch.int8).fill_(FILL)               # the caller's workspace, or the forest
        tensors, where = device_outputs(call, "visits", 4)
        refused("device visits must be 16-byte aligned", call, where, tail, 1, tensors + [keep])
        if call.tail == "workspace":
            crooked = (ctypes.c_void_p(keep.data_ptr() + 64), tail[1])
            more, straight = device_outputs(call)
            refused("the workspace must be 256-byte aligned", call, straight, crooked, 1, tensors + more + [keep])
            host = [np.full(shape, FILL, dtype=dtype) for _, shape, dtype, _ in call.outputs]
            refused("the workspace must be 256-byte aligned", call, [ctypes.c_void_p(x.ctypes.data) for x in host], crooked, 0,
                    [torch.from_numpy(x) for x in host] + [keep])
        else:
            more, straight = device_outputs(call)
            for on_device in (0, 1):
                refused(f"forest is NULL (the caller owns it; {sizing} says how large)", call, straight, (None, tail[1]), on_device,
                        tensors + more + [keep])
    tensors, where = device_outputs(solve, "nodes", 4)
    refused("device nodes must be 8-byte aligned", solve, where, (), 1, tensors)
    # the re-rooting call: kept is an int32 a board
    _, tail, forest = tails(b, forest_search, game)[0]
    moves = torch.full((N + 1,), -1, dtype=torch.int32, device="cuda:0")
    kept = torch.full((N + 4,), FILL, dtype=torch.int32, device="cuda:0")
    advance = getattr(lib, f"bgs_{game}_forest_advance")
    sizes = forest_search.head[6:-1]                           # capacity (Bounce: and edges)
    rc = advance(b._handle, ctypes.c_void_p(moves.data_ptr()), *sizes, ctypes.c_void_p(kept.data_ptr() + 2), *tail, 1)
    assert rc == _abi.BGS_ERR_ARG and _abi.last_error() == "device kept must be 4-byte aligned", _abi.last_error()
    rc = advance(b._handle, ctypes.c_void_p(moves.data_ptr()), *sizes, ctypes.c_void_p(kept.data_ptr()), None, tail[1], 1)
    assert rc == _abi.BGS_ERR_ARG and _abi.last_error() == f"forest is NULL (the caller owns it; {sizing} says how large)"
    torch.cuda.synchronize()
    assert bool((kept == FILL).all()) and bool((forest == 0).all())
    b.close()
