"""CPU-only checks of the forest (bgs_connect_forest_search / bgs_connect_forest_advance): the chains of
tests/forest_expected.py hold what tests/test_gpu_forest.py needs, as computed by the CPU model, and the plumbing is in
place -- both libraries export the three symbols, the header declares them, the version script lets them out, the ctypes
binding table has them with the header's arguments, a NULL batch is refused (the one refusal that needs no device) and
the Python surface is there."""

import ctypes
import fnmatch
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import forest_expected as fe
from tests import search_expected as se
from tests.conftest import PKG, PRODUCT_LIB, TEST_LIB

CSRC = os.path.join(PKG, "csrc")
SYMBOLS = ("bgs_connect_forest_bytes", "bgs_connect_forest_search", "bgs_connect_forest_advance")
NAMES = ("counts", "visits", "best", "nodes", "carried")


# ---- the case table
@pytest.mark.parametrize("index", fe.ANCHORS, ids=lambda j: se.case_id(se.CASES[j]))
def test_a_restart_with_room_for_every_node_is_the_plain_search(index):
    assert {0, 2, 9, 10} <= set(fe.ANCHORS)
    got = fe.anchor_expected(index)
    counts, visits, best, nodes, steps, _ = se.case_expected(index)
    for name, g, w in zip(NAMES, got, (counts, visits, best, nodes, np.zeros_like(nodes))):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert got[5] == steps


def test_chain_shapes_are_those_the_gpu_test_promises():
    for chain in fe.CHAINS + fe.AGENT_CHAINS:
        assert 3 <= len(chain.moves) <= 5 and chain_roots_count(chain) <= 24
        if chain.h * chain.w <= 30:
            assert all(m.iterations <= 64 and m.playouts <= 8 for m in chain.moves)
    shapes = {(c.h, c.w, c.k) for c in fe.CHAINS}
    assert shapes == {(6, 7, 4), (5, 6, 3), (2, 5, 3), (6, 12, 4), (12, 13, 5)}
    sizes = {(m.iterations, m.playouts) for c in fe.CHAINS if (c.h, c.w, c.k) == (6, 7, 4) for m in c.moves}
    assert {(48, 16), (12, 70)} <= sizes
    assert any(c.policy == "decisive" for c in fe.CHAINS) and any(c.per_ply for c in fe.CHAINS)
    assert any(c.cap is not None for c in fe.CHAINS) and any(c.capacity == 2 for c in fe.CHAINS)
    assert any(m.rule == "best2" for c in fe.CHAINS for m in c.moves)
    # a re-rooting of more than 512 nodes that keeps more than 64
    assert any((r.nodes > 512).any() and (r.plies[0][2] > 64).any() for j in range(len(fe.CHAINS)) for r in fe.chain_expected(j)[0])


def chain_roots_count(chain):
    return fe.chain_roots(chain)[0].shape[0] if chain in fe.CHAINS else fe.AGENT_STATES


def test_some_chain_carries_nodes_at_every_move_after_the_first():
    records, _ = fe.chain_expected(0)
    for record in records[1:]:
        running = record.roots[2] == -1
        assert running.any() and 2 * int((record.carried[running] > 0).sum()) >= int(running.sum())
    assert (records[0].carried == 0).all()
    assert (records[1].visits.sum(axis=1) > records[1].counts.sum(axis=(1, 2))).any()   # carried visits are in `visits`


def test_some_chain_fills_a_tree_and_replays_an_edge_whose_node_did_not_fit():
    records, forest = fe.chain_expected(1)
    chain = fe.CHAINS[1]
    assert any((record.nodes == chain.capacity - 1).any() for record in records)
    assert forest.refused > 0 and forest.replayed > 0
    for j, chain in enumerate(fe.CHAINS):
        for record in fe.chain_expected(j)[0]:
            assert (record.nodes <= chain.capacity - 1).all() and (record.carried <= record.nodes).all()


def test_the_chains_hold_the_advances_the_gpu_test_needs():
    two_ply = capacity_two = ends = terminal = unplayed = False
    for j, chain in enumerate(fe.CHAINS):
        records, _ = fe.chain_expected(j)
        two_ply |= any(len(record.plies) == 2 and (record.plies[1][2] > 0).any() for record in records)
        capacity_two |= chain.capacity == 2 and all((record.nodes <= 1).all() for record in records)
        first, last = records[0].roots[2], records[-1].roots[2]
        ends |= bool(((first == -1) & (last != -1)).any())
        for record, after in zip(records, records[1:]):
            tree, board, kept = record.plies[0]
            moved = tree >= 0
            played = record.visits[np.arange(tree.size), np.maximum(tree, 0)] > 0
            ended = after.roots[2] != -1
            terminal |= bool((moved & played & ended & (kept == 0)).any())      # the edge ended the game: no child
            unplayed |= bool((moved & ~played & ~ended & (kept == 0)).any())    # a legal column the search never took
    assert two_ply and capacity_two and ends and terminal and unplayed


def test_a_desynchronised_board_is_searched_as_after_a_restart():
    index = next(j for j, c in enumerate(fe.CHAINS) if any(m.rule == "desync" for m in c.moves))
    chain = fe.CHAINS[index]
    records, _ = fe.chain_expected(index)
    m = next(m for m, move in enumerate(chain.moves) if move.rule == "desync")
    d = records[m].desynced
    tree, board, kept = records[m].plies[0]
    assert d >= 0 and tree[d] != board[d] and kept[d] > 0          # the tree went one way with nodes, the board another
    after = records[m + 1]
    assert after.roots[2][d] == -1 and after.carried[d] == 0
    assert (np.delete(after.carried, d) > 0).any()
    move = chain.moves[m + 1]
    fresh = fe.Forest(chain.h, chain.w, chain.k, tree.size, chain.capacity)
    want = fresh.search(after.roots, move.seed, chain.first_game, move.iterations, move.playouts, chain.explore,
                        fe.chain_max_plies(chain, fe.chain_roots(chain)), chain.per_ply, chain.policy, restart=True)
    for name, g, w in zip(NAMES, after[1:6], want):
        np.testing.assert_array_equal(g[d], w[d], err_msg=name)


def test_the_agent_chain_carries_nodes_over_one_and_two_stones():
    records, _ = fe.chain_expected(0, agent=True)
    assert [len(r.plies) for r in records].count(2) >= 1
    for before, record in zip(records, records[1:]):       # (a grandchild may come over as a bare root: carried 0)
        assert (record.carried > 0).all() if len(before.plies) == 1 else (record.carried > 0).any()
    assert all((r.roots[2] == -1).all() for r in records)


def test_stones_between_orders_the_plies():
    from simulator.agents import TreeSearchAgent

    old = np.full((6, 7), -1, dtype=np.int8)
    old[0, 3] = 0
    between = TreeSearchAgent.stones_between
    assert between(old, 1, old.copy()) == (-1, -1)
    one = old.copy()
    one[0, 2] = 1
    assert between(old, 1, one) == (2, -1) and between(old, 0, one) == (-1, -1)
    two = one.copy()
    two[1, 3] = 0
    assert between(old, 1, two) == (2, 3)
    stacked = old.copy()
    stacked[1, 3], stacked[2, 3] = 1, 0
    assert between(old, 1, stacked) == (3, 3)
    three = two.copy()
    three[0, 0] = 1
    assert between(old, 1, three) == (-1, -1)
    same = one.copy()
    same[0, 5] = 1
    assert between(old, 1, same) == (-1, -1)                       # two stones of one player
    moved = old.copy()
    moved[0, 3], moved[0, 4] = -1, 0
    assert between(old, 1, moved) == (-1, -1)                      # a stone left its cell


# ---- the plumbing
def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_both_libraries_export_the_forest():
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
    assert "BGS_API int bgs_connect_forest_bytes(const bgs_batch* b, int32_t capacity, size_t* bytes);" in text
    assert ("BGS_API int bgs_connect_forest_search(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, "
            "int32_t explore,") in text
    assert "BGS_API int bgs_connect_forest_advance(bgs_batch* b, const int32_t* columns, int32_t capacity, int32_t* kept, void* forest," in text
    assert "#define BGS_CONNECT_FOREST_MAX_CAPACITY 65536" in text
    for word in ("MUST PASS restart != 0", "256-byte", "carried", "did not fit"):
        assert word in text, word


def test_the_binding_table_has_the_symbols():
    from simulator.game import _abi

    i32, vp = ctypes.c_int32, ctypes.c_void_p
    assert _abi.SIGNATURES["bgs_connect_forest_bytes"] == (ctypes.c_int, [_abi.c_handle, i32, ctypes.POINTER(ctypes.c_size_t)])
    assert _abi.SIGNATURES["bgs_connect_forest_search"] == (
        ctypes.c_int, [_abi.c_handle, ctypes.c_uint64, i32, i32, i32, i32, ctypes.c_int, i32, ctypes.c_int, vp, vp, vp, vp, vp, vp,
                       ctypes.c_size_t, ctypes.c_int])
    assert _abi.SIGNATURES["bgs_connect_forest_advance"] == (
        ctypes.c_int, [_abi.c_handle, vp, i32, vp, vp, ctypes.c_size_t, ctypes.c_int])
    assert _abi.CONNECT_FOREST_MAX_CAPACITY == 65536


def test_a_null_batch_is_refused_with_a_message():
    """the NULL-batch refusal alone: a batch cannot be made without a device, so every other refusal is checked in
    tests/test_gpu_forest.py"""
    from simulator.game import _abi

    lib = _abi.lib()
    size = ctypes.c_size_t(77)
    assert lib.bgs_connect_forest_bytes(None, 8, ctypes.byref(size)) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error() and size.value == 77
    out = (ctypes.c_int32 * 64)()
    at = ctypes.cast(out, ctypes.c_void_p)
    assert lib.bgs_connect_forest_search(None, 1, 8, 8, 65536, 100, 0, 9, 1, at, None, None, None, None, None, 0, 0) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error() and not any(out)
    assert lib.bgs_connect_forest_advance(None, at, 9, at, None, 0, 0) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error() and not any(out)


def test_the_python_surface():
    from simulator import agents, batch

    for name in ("forest_bytes", "search_forest"):
        assert callable(getattr(batch.ConnectBatch, name))
        with pytest.raises(ValueError, match="Connect batches only"):     # Bounce refuses before it looks at the batch
            getattr(batch.BounceBatch, name)(None, 9)
    for name in ("search", "search_tensor", "advance", "advance_tensor", "close"):
        assert callable(getattr(batch.SearchForest, name))
    sig = inspect.signature(batch.SearchForest.search)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("seed", batch.DEFAULT_SEED), ("iterations", 256), ("leaf_playouts", 64), ("explore", 65536), ("max_plies", 2**31 - 1),
        ("policy", "uniform"), ("restart", False)]
    sig = inspect.signature(agents.TreeSearchAgent.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[-2:]] == [("reuse", False), ("capacity", None)]
    agent = agents.TreeSearchAgent(iterations=24)
    assert agent.reuse is False and agent.capacity == 49
    assert agents.TreeSearchAgent(iterations=24, reuse=True, capacity=30).capacity == 30
    with pytest.raises(ValueError, match="capacity"):
        agents.TreeSearchAgent(reuse=True, capacity=1)
    assert "allowance" in agents.TreeSearchAgent.__doc__
