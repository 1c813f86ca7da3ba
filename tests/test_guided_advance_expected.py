"""CPU-only checks of tests/guided_advance_expected.py, the CPU statement of bgs_connect_guided_advance: over the scripted
corner games that tests/test_gpu_guided_advance.py replays on the device, the kept subtree is node for node what it was
-- stated a second time here, on the decoded arrays and not on the statement's objects --, `kept` is the nodes less the
root, every "anything else" column empties its tree, and the games hold every kind of column the GPU test needs; on a
Connect4 batch, a negative column leaves a pending leaf in place, an advance drops it, and a tree advanced over boards that
were not stepped restarts at the next step."""

import numpy as np
import pytest

from tests import guided_advance_expected as ga
from tests import guided_expected as ge
from tests import guided_shares as gs

EMPTIED = ("never_played", "full_column", "width", "wins", "fills", "did_not_fit", "empty")
GAMES = [(key, capacity) for key in ga.CORNERS for capacity in ga.CAPACITIES]


def compacted(tree, column, h):
    """the decoded tree after an advance by `column` that keeps a subtree, from the decoded tree before it: the nodes
    reachable from the root's child of `column`, in index order, renumbered"""
    r = tree["nodes"][0]["child"][column]
    assert 0 < r < tree["count"]
    keep, stack = set(), [r]
    while stack:
        v = stack.pop()
        keep.add(v)
        stack.extend(ch for ch in tree["nodes"][v]["child"] if ch)
    order = sorted(keep)
    assert order[0] == r                    # a child is made after its parent: the new root is the lowest index kept
    index = {v: j for j, v in enumerate(order)}
    nodes = [dict(tree["nodes"][v], child=[index[ch] if ch else 0 for ch in tree["nodes"][v]["child"]]) for v in order]
    nw = len(tree["planes"]) // 2
    stones = sum(bin(p).count("1") for p in tree["planes"])
    taken = sum(1 for y in range(h) if any((tree["planes"][p * nw + (column * (h + 1) + y) // 64] >> ((column * (h + 1) + y) % 64)) & 1
                                           for p in range(2)))
    bit = column * (h + 1) + taken
    planes = list(tree["planes"])
    planes[(stones & 1) * nw + bit // 64] |= 1 << (bit % 64)
    return {"count": len(order), "kind": gs.NONE, "legal": 0, "depth": 0, "expanded": 1, "planes": planes, "path": [], "nodes": nodes}


@pytest.mark.parametrize("key,capacity", GAMES)
def test_every_advance_of_the_corner_games(key, capacity):
    h, w, k = ga.corner_geometry(key)
    model, script = ga.corner_game(key, capacity)
    for m, move in enumerate(script):
        for i, (kind, c) in enumerate(zip(move.kinds, move.columns)):
            before, after, what = move.finished[i], move.advanced[i], f"{key} C = {capacity} move {m} tree {i} ({kind}, column {c})"
            if kind == "untouched":
                assert c < 0 and after == before and move.kept[i] == max(before["count"] - 1, 0), what
            elif kind in ("best", "child"):
                gs.assert_same_tree(after, compacted(before, int(c), h), what)
                assert move.kept[i] == after["count"] - 1 >= 0, what
                assert after["count"] <= before["count"] - 1, what
            else:
                assert kind in EMPTIED and c >= 0, what
                assert (after["count"], after["kind"], after["depth"], after["expanded"], after["nodes"]) == (0, gs.NONE, 0, 0, []), what
                assert move.kept[i] == 0, what
        # the search after an advance: a kept tree goes on from its visits, an emptied one from none
        if m + 1 < len(script):
            first = script[m + 1].calls[0]
            for i, after in enumerate(move.advanced):
                stepped_as_advanced = move.played[i] == move.columns[i] or move.columns[i] < 0
                carried = after["count"] > 0 and stepped_as_advanced and script[m + 1].roots[2][i] == -1
                assert first[6][i] == (after["count"] - 1 if carried else 0), (key, m, i)
                assert first[3][i].sum() == (sum(after["nodes"][0]["n"]) if carried else 0), (key, m, i)


def test_the_corner_games_hold_what_the_device_test_needs():
    kinds, most = {}, 0
    for key, capacity in GAMES:
        roots, ending, ended = ga.corner_roots(key)
        assert 8 <= roots[0].shape[0] <= 16 and len(set(roots[3].tolist())) >= 3, key        # roots at different plies
        assert ended == 1 and ending >= 1, key          # an ended board, and a board one move from its end
        for move in ga.corner_game(key, capacity)[1]:
            most = max(most, int(move.kept.max()))
            for kind in move.kinds:
                kinds[kind] = kinds.get(kind, 0) + 1
    print(kinds, "the most nodes kept:", most)
    for kind in ga.REQUIRED + ("child", "did_not_fit", "empty"):
        assert kinds.get(kind, 0) >= 1, kind
    assert most > ga.SIMULATIONS        # trees that regained room grew past what one search makes
    # the trees of capacity 3 ran out of room, and an advance gave room back: a tree kept with fewer than 3 nodes is full again
    model, script = ga.corner_game("6x7x4", 3)
    assert model.refused > 0
    assert any(0 < after["count"] < 3 and later["count"] == 3
               for move, then in zip(script, script[1:]) for after, later in zip(move.advanced, then.finished))


@pytest.mark.parametrize("evaluator", list(ga.CHUNK_EVALUATORS))
def test_the_chunk_games_cross_chunk_boundaries(evaluator):
    model, script = ga.chunk_game(evaluator)
    for m, move in enumerate(script):
        for i, c in enumerate(move.columns):
            assert c >= 0
            gs.assert_same_tree(move.advanced[i], compacted(move.finished[i], int(c), 6), f"{evaluator} move {m} tree {i}")
    assert max(int(move.kept.max()) for move in script) > 128
    if evaluator == "narrow":
        late = [(ga.new_root_index(tree, int(c)), int(kept)) for move in script for tree, c, kept in zip(move.finished, move.columns, move.kept)]
        assert any(r >= 64 and kept >= 1 for r, kept in late), late


def connect4(n=4):
    from oracle import oracle

    orc = oracle.ConnectOracle(6, 7, 4, n)
    orc.step_actions((np.arange(n) % 7).astype(np.int32))
    return orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy()


def searched(roots, calls, capacity=40):
    """a statement after begin and `calls` plain steps: a leaf is pending on every tree"""
    model = ga.GuidedAdvance(6, 7, 4, roots[0].shape[0], capacity, 320)
    out = model.step(roots, flags=ge.RESTART)
    for _ in range(calls):
        out = model.step(roots, *ge.fake_network(out[0], out[1]))
    return model, out


def test_a_negative_column_leaves_a_pending_leaf_in_place():
    roots = connect4()
    model, out = searched(roots, 20)
    other, _ = searched(roots, 20)
    before = ga.decoded(model)
    assert all(tree["kind"] != gs.NONE for tree in before)
    kept = model.advance(np.full(4, -1, dtype=np.int32))
    assert ga.decoded(model) == before and kept.tolist() == [tree["count"] - 1 for tree in before]
    assert kept.tolist() == [ge.count_nodes(root) for root in model.root]
    # ... and the next step applies it: the advanced statement and one that was never advanced go on alike
    rows = ge.fake_network(out[0], out[1])
    for got, want in zip(model.step(roots, *rows), other.step(roots, *rows)):
        np.testing.assert_array_equal(got, want)
    assert ga.decoded(model) == ga.decoded(other)


def test_an_advance_drops_a_pending_leaf_and_unstepped_boards_restart():
    roots = connect4()
    model, out = searched(roots, 30)
    before = ga.decoded(model)
    columns = out[5].astype(np.int32)                   # `best`: every root has visits
    assert (columns >= 0).all() and all(tree["kind"] != gs.NONE for tree in before)
    kept = model.advance(columns)
    after = ga.decoded(model)
    for i, tree in enumerate(after):
        gs.assert_same_tree(tree, compacted(dict(before[i], kind=gs.NONE, legal=0, depth=0, path=[]), int(columns[i]), 6), f"tree {i}")
        assert (tree["kind"], tree["depth"], tree["path"], tree["expanded"]) == (gs.NONE, 0, [], 1)
        assert kept[i] == tree["count"] - 1 == ge.count_nodes(model.root[i])
    assert kept.sum() > 0
    # boards 0 and 1 are stepped by their column, board 2 by another one, board 3 not at all
    played = columns.copy()
    played[2], played[3] = (columns[2] + 1) % 7, -1
    after_roots = ga.stepped(6, 7, 4, roots, played)
    rows = np.full((4, 7), np.nan, dtype=np.float32), np.full(4, np.nan, dtype=np.float32)      # nothing is pending: not read
    out = model.step(after_roots, *rows)
    assert out[6].tolist() == [kept[0], kept[1], 0, 0] and not out[3][2:].any()
    assert out[3][:2].sum(axis=1).tolist() == [sum(after[i]["nodes"][0]["n"]) for i in range(2)]         # the dropped leaf was not applied
    assert (out[2][2:] == ge.EVALUATE).all()
    np.testing.assert_array_equal(out[0][2:], after_roots[0][2:])           # the restarted roots are the leaves again
