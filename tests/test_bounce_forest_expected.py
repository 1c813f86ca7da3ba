"""CPU-only checks of the Bounce forest (bgs_bounce_forest_search / bgs_bounce_forest_advance): the chains of
tests/bounce_forest_expected.py hold what tests/test_gpu_bounce_forest.py needs, as computed by the CPU model, the model
keeps its own invariants, and the plumbing is in place -- both libraries export the three symbols, the header declares
them, the ctypes binding table has them with the header's arguments, a NULL batch is refused (the one refusal that needs
no device) and the Python surface is there."""

import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import bounce_forest_expected as bf
from tests import search_bounce_expected as sb
from tests.conftest import PKG, PRODUCT_LIB, TEST_LIB

SYMBOLS = ("bgs_bounce_forest_bytes", "bgs_bounce_forest_search", "bgs_bounce_forest_advance")
NAMES = ("counts", "visits", "best", "nodes", "used", "carried")
CHAIN_NAMES = [c.name for c in bf.CHAINS]


# ---- the model
@pytest.mark.parametrize("name", bf.ANCHORS)
def test_a_restart_with_room_for_every_node_is_the_plain_search(name):
    assert len(bf.ANCHORS) >= 4
    policy = sb.BY_NAME[name].policies[0]
    *want, steps, _ = sb.case_expected(name, policy)
    for spare in (0, 7):
        got = bf.anchor_expected(name, policy, spare)
        for what, g, w in zip(NAMES, got, want + [np.zeros_like(want[3])]):
            np.testing.assert_array_equal(g, w, err_msg=f"{what}, C = T + 1 + {spare}")
        assert got[6] == steps


@pytest.mark.parametrize("name", CHAIN_NAMES + ["agent"])
def test_the_model_keeps_its_invariants_along_every_chain(name):
    """run_chain calls Forest.check() after every search and every advance: an edge's n equals the sum over its child plus
    the playouts of the iterations that stopped at the edge, blocks are contiguous and ascending, children lie above their
    parents; here the counts the kernel reports"""
    agent = name == "agent"
    chain = bf.AGENT_CHAINS[0] if agent else bf.BY_NAME[name]
    records, forest = bf.chain_expected(name, agent)
    forest.check()
    E = bf.chain_edges(chain)
    assert len(records) == len(chain.moves) and chain.n <= 8
    assert all(m.iterations * m.playouts <= 1024 for m in chain.moves)
    kept = np.zeros(chain.n, dtype=np.int32)
    for m, record in enumerate(records):
        running = record.roots[2] == -1
        assert (record.carried <= kept).all() if m else (record.carried == 0).all()      # (a desynchronised tree carries nothing)
        assert (record.carried <= record.nodes).all() and (record.nodes <= chain.nodes - 1).all()
        assert (record.used <= E).all() and (record.used[~running] == 0).all() and (record.best[~running] == -1).all()
        assert (record.visits.sum(axis=(1, 2)) >= record.counts.sum(axis=(1, 2, 3))).all()
        kept = record.nodes
        for tree, board, after in record.plies:
            assert (after <= kept).all() and (after[tree < 0] == kept[tree < 0]).all()       # a negative slot leaves the tree alone
            assert ((tree >= 0) == (board[:, 0] >= 0)).all()
            kept = after


def test_every_chain_that_can_carries_nodes():
    """at least one move of every multi-move chain starts with carried nodes -- but for C = 2 (the re-rooted tree is a bare
    root, so nothing can be carried) and for `narrow` (one column of five cells: every edge of every root ends the game, so
    no tree ever has a second node); `column`, one column of nine cells, is the chain whose one-arm roots stand in carried
    trees"""
    for chain in bf.CHAINS:
        records, _ = bf.chain_expected(chain.name)
        most = max(int(r.carried.max()) for r in records)
        if chain.nodes == 2:
            assert most == 0 and any((r.nodes == 1).any() for r in records)
        elif chain.name == "narrow":
            assert all((r.nodes == 0).all() for r in records) and any((r.used == 1).any() for r in records)    # a one-arm root
        else:
            assert len(chain.moves) >= 3 and most > 0, chain.name
    column = bf.chain_expected("column")[0]
    assert all((r.used == r.nodes + 1).all() for r in column)              # every node of every tree has one arm
    assert all((r.carried > 0).all() for r in column[1:]) and any(len(r.plies) == 2 and (r.plies[1][2] > 0).all() for r in column)
    assert any((r.nodes == bf.BY_NAME["column"].nodes - 1).any() for r in column)       # ... and a descent as long as the tree has nodes
    records, _ = bf.chain_expected("agent", True)
    assert max(int(r.carried.max()) for r in records) > 0
    assert all(len(r.plies) == 2 for r in records) and all((r.roots[2] == -1).all() for r in records)


def test_the_chains_cover_the_shapes_the_gpu_test_promises():
    by = bf.BY_NAME
    assert {c.grid for c in bf.CHAINS} >= {"default", "wide", "narrow", "column", "crowded", "small"}
    assert any(c.grid == "default" and c.policy == "decisive" for c in bf.CHAINS)
    assert any(c.grid == "default" and c.policy == "uniform" for c in bf.CHAINS)
    h, w = bf.chain_grid(by["wide"]).shape
    assert sb.count_words(w) == 2 and any((r.used >= 71).any() for r in bf.chain_expected("wide")[0])
    assert by["two_nodes"].nodes == 2
    assert bf.chain_edges(by["min_edges"]) == sb.min_edges(9, 6) == 252
    assert by["ids"].first_game == 2**33
    capped = by["capped"]
    assert capped.cap is not None and len({m.cap for m in capped.moves}) == 2
    large = by["large"]
    assert large.n == 2 and all(m.playouts == 1 for m in large.moves) and large.moves[0].iterations >= 300
    rules = {m.rule for c in bf.CHAINS for m in c.moves}
    assert rules >= {"best", "best2", "high", "desync"}


def test_the_chains_reach_every_branch():
    seen = {c.name: bf.chain_expected(c.name)[1].seen for c in bf.CHAINS}
    total = {key: sum(s[key] for s in seen.values()) for key in seen["default"]}
    assert total["emptied_no_child"] > 0            # an arm that was never expanded, or whose node did not fit
    assert total["emptied_sentinel"] > 0            # an edge that ends the game or is capped
    assert seen["capped"]["emptied_cap"] > 0        # the cap changed
    assert total["emptied_position"] > 0            # a desynchronised board
    assert seen["few_nodes"]["no_room_nodes"] > 0 and seen["few_nodes"]["no_room_edges"] == 0     # nodes run out, edges do not
    assert seen["two_nodes"]["no_room_nodes"] > 0
    assert seen["min_edges"]["no_room_edges"] > 0 and seen["min_edges"]["no_room_nodes"] == 0     # edges run out, nodes do not
    assert seen["large"]["most_kept"] > 256         # a re-rooting over many chunks that keeps more than 256 nodes
    assert total["overlapping_moves"] > 0           # an edge block moved onto a range that overlaps its old one
    records, _ = bf.chain_expected("large")
    assert (records[0].nodes > 512).any()


def test_a_desynchronised_board_is_searched_as_after_a_restart():
    chain = next(c for c in bf.CHAINS if any(m.rule == "desync" for m in c.moves))
    records, _ = bf.chain_expected(chain.name)
    m = next(m for m, move in enumerate(chain.moves) if move.rule == "desync")
    d = records[m].desynced
    tree, board, kept = records[m].plies[0]
    h, w = bf.chain_grid(chain).shape
    sx, _, tx, ty = board[d].tolist()
    assert d >= 0 and kept[d] > 0 and sx * h * w + ty * w + tx != tree[d]      # the tree went one way with nodes, the board another
    after = records[m + 1]
    assert after.roots[2][d] == -1 and after.carried[d] == 0
    assert (np.delete(after.carried, d) > 0).any()
    move = chain.moves[m + 1]
    fresh = bf.Forest(bf.chain_grid(chain), chain.n, chain.nodes, bf.chain_edges(chain))
    want = fresh.search(after.roots, move.seed, chain.first_game, move.iterations, move.playouts, chain.explore, after.max_plies,
                        chain.policy, restart=True)
    for what, g, w in zip(NAMES, after[2:8], want):
        np.testing.assert_array_equal(g[d], w[d], err_msg=what)


def test_moves_between_reads_one_and_two_clean_moves():
    from simulator.agents import BounceTreeSearchAgent

    between = BounceTreeSearchAgent.moves_between
    old = sb.GRIDS["default"].copy()
    h, w = old.shape
    assert between(old, 0, old.copy(), 0) == (-1, -1)
    one = old.copy()
    one[1, 2], one[4, 2] = 0, 3                                 # the 3 of column 2 goes up three rows
    assert between(old, 0, one, 1) == (2 * h * w + 4 * w + 2, -1)
    assert between(old, 0, one, 2) == (-1, -1)
    two = one.copy()
    two[7, 0], two[6, 0] = 0, 1                                 # the reply: the 1 of column 0 of the top row goes down one
    assert between(old, 0, two, 2) == (2 * h * w + 4 * w + 2, 0 * h * w + 6 * w + 0)
    assert between(old, 1, two, 2) == (0 * h * w + 6 * w + 0, 2 * h * w + 4 * w + 2)       # the mover's move comes first
    same_value = one.copy()
    same_value[7, 2], same_value[5, 2] = 0, 3                   # two pieces of one value, both pairings one step off a plain walk
    assert between(old, 0, same_value, 2) == (-1, -1)
    mirrored = one.copy()
    mirrored[7, 3], mirrored[4, 3] = 0, 3                       # two pieces of one value: the pairing of the plain walks is taken
    assert between(old, 0, mirrored, 2) == (2 * h * w + 4 * w + 2, 3 * h * w + 4 * w + 3)
    chained = old.copy()
    chained[1, 2], chained[6, 2] = 0, 3                         # the reply moved the piece just played: two cells, two plies
    assert between(old, 0, chained, 2) == (-1, -1)
    changed = one.copy()
    changed[4, 2] = 2                                           # a piece that changed its value is no move
    assert between(old, 0, changed, 1) == (-1, -1)


def test_moves_between_recovers_the_plies_of_the_agent_chain():
    """the GPU test lets the agent read both moves of every move of the agent chain off the grids: they are clean ones"""
    from simulator.agents import BounceTreeSearchAgent

    records, _ = bf.chain_expected("agent", True)
    for before, after in zip(records, records[1:]):
        (first, _, _), (second, _, _) = before.plies
        for k in range(bf.AGENT_STATES):
            got = BounceTreeSearchAgent.moves_between(before.roots[0][k], int(before.roots[1][k]), after.roots[0][k],
                                                      int(after.roots[3][k]) - int(before.roots[3][k]))
            assert got == (first[k], second[k]), (k, got)


# ---- the plumbing
def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_both_libraries_export_the_forest():
    for path in (PRODUCT_LIB, TEST_LIB):
        assert set(SYMBOLS) <= _exports(path), path


def test_the_header_declares_them():
    with open(os.path.join(os.path.dirname(PKG), "include", "bgs.h")) as f:
        text = f.read()
    flat = " ".join(text.replace("\n * ", " ").split())
    assert "BGS_API int bgs_bounce_forest_bytes(const bgs_batch* b, int32_t nodes, int32_t edges, size_t* bytes);" in flat
    assert ("BGS_API int bgs_bounce_forest_search(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, "
            "int32_t explore, int32_t max_plies, int policy, int32_t nodes_cap, int32_t edges, int restart, int32_t* counts, "
            "int32_t* visits, int32_t* best, int32_t* nodes, int32_t* used, int32_t* carried, void* forest, size_t forest_bytes, "
            "int on_device);") in flat
    assert ("BGS_API int bgs_bounce_forest_advance(bgs_batch* b, const int32_t* slots, int32_t nodes_cap, int32_t edges, "
            "int32_t* kept, void* forest, size_t forest_bytes, int on_device);") in flat
    assert "#define BGS_BOUNCE_FOREST_MAX_NODES 65536" in text
    assert "#define BGS_BOUNCE_FOREST_MAX_EDGES (1 << 29)" in text
    section = flat[flat.index("the sibling of bgs_connect_forest_"):flat.index("#define BGS_BOUNCE_FOREST_MAX_NODES")]
    for word in ("MUST PASS restart != 0", "256-byte", "carried", "did not fit", "recorded cap", "ply count"):
        assert word in section, word


def test_the_binding_table_has_the_symbols():
    from simulator.game import _abi

    i32, vp = ctypes.c_int32, ctypes.c_void_p
    assert _abi.SIGNATURES["bgs_bounce_forest_bytes"] == (ctypes.c_int, [_abi.c_handle, i32, i32, ctypes.POINTER(ctypes.c_size_t)])
    assert _abi.SIGNATURES["bgs_bounce_forest_search"] == (
        ctypes.c_int, [_abi.c_handle, ctypes.c_uint64, i32, i32, i32, i32, ctypes.c_int, i32, i32, ctypes.c_int, vp, vp, vp, vp, vp,
                       vp, vp, ctypes.c_size_t, ctypes.c_int])
    assert _abi.SIGNATURES["bgs_bounce_forest_advance"] == (
        ctypes.c_int, [_abi.c_handle, vp, i32, i32, vp, vp, ctypes.c_size_t, ctypes.c_int])
    assert _abi.BOUNCE_FOREST_MAX_NODES == 65536 and _abi.BOUNCE_FOREST_MAX_EDGES == 1 << 29


def test_a_null_batch_is_refused_with_a_message():
    """the NULL-batch refusal alone: a batch cannot be made without a device, so every other refusal is checked in
    tests/test_gpu_bounce_forest.py"""
    from simulator.game import _abi

    lib = _abi.lib()
    size = ctypes.c_size_t(77)
    assert lib.bgs_bounce_forest_bytes(None, 8, 252, ctypes.byref(size)) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error() and size.value == 77
    out = (ctypes.c_int32 * 64)()
    at = ctypes.cast(out, ctypes.c_void_p)
    assert lib.bgs_bounce_forest_search(None, 1, 8, 8, 65536, 100, 0, 9, 252, 1, at, None, None, None, None, None, None, 0,
                                        0) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error() and not any(out)
    assert lib.bgs_bounce_forest_advance(None, at, 9, 252, at, None, 0, 0) == _abi.BGS_ERR_ARG
    assert "NULL" in _abi.last_error() and not any(out)


def test_the_python_surface():
    from simulator import agents, batch

    for name in ("moves_forest_bytes", "search_moves_forest", "slots_to_moves", "slots_to_moves_tensor"):
        assert callable(getattr(batch.BounceBatch, name))
    sig = inspect.signature(batch.BounceBatch.search_moves_forest)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("nodes", inspect.Parameter.empty), ("edges", None)]
    for name in ("forest_bytes", "search_forest"):
        with pytest.raises(ValueError, match="Connect batches only"):     # the Connect forest still refuses Bounce
            getattr(batch.BounceBatch, name)(None, 9)
    for name in ("search", "search_tensor", "advance", "advance_tensor", "close"):
        assert callable(getattr(batch.MovesForest, name))
    sig = inspect.signature(batch.MovesForest.search)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("seed", batch.DEFAULT_SEED), ("iterations", 256), ("leaf_playouts", 64), ("explore", 65536), ("max_plies", 2**31 - 1),
        ("policy", "uniform"), ("restart", False)]
    sig = inspect.signature(batch.MovesForest.search_tensor)
    assert [p.name for p in list(sig.parameters.values())[1:7]] == list(NAMES)
    sig = inspect.signature(agents.BounceTreeSearchAgent.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[-2:]] == [("reuse", False), ("capacity", None)]
    agent = agents.BounceTreeSearchAgent(iterations=24)
    assert agent.reuse is False and agent.capacity == 49
    assert agents.BounceTreeSearchAgent(iterations=24, reuse=True, capacity=30).capacity == 30
    with pytest.raises(ValueError, match="capacity"):
        agents.BounceTreeSearchAgent(reuse=True, capacity=1)
    assert "allowance" in agents.BounceTreeSearchAgent.__doc__ and "NOT measured" in batch.BounceBatch.search_moves_forest.__doc__
