"""What tests/search_bounce_prove_expected.py -- the CPU statement of bgs_bounce_search_moves_proving over the case table
of the plain Bounce search and one hand-made case -- holds: every tagged edge of every tree is right, checked without the
model's own bookkeeping by a certificate walk over the oracle's `actions` and `step_actions`; a root whose search tags
nothing is the plain search's, output for output; and the cases reach every branch the proving search adds.  No GPU.

The four branches the prototype had not shown reachable: the table itself reaches two of them (a selection in which the
plain rule would have taken a tagged arm: `default`, `uct` and others; a node whose only OPEN arms are capped: `capped`).
The other two -- a DRAW backed up, and a root decided DRAW that also holds a LOSS arm -- come from the hand-made case
"draws": the crowded grid from make_roots seed 142, the only seed of 0 .. 299 at 8 roots and 32 x 4 that reaches either
(it reaches both); no seed of the narrow, blocked_start and small grids does."""

import numpy as np
import pytest

from tests import search_bounce_expected as sb
from tests import search_bounce_prove_expected as sp

RUNS = [("table", n, p) for n, p in sp.RUNS] + [("hand", n, p) for n, p in sp.hand_runs()]
IDS = [f"{k}-{n}-{p}" for k, n, p in RUNS]


def _run(kind, name, policy):
    """(grid, roots, T, P, trees, the model's outputs)"""
    if kind == "table":
        case = sb.BY_NAME[name]
        return sb.case_grid(case), sb.case_roots(case), case.iterations, case.playouts, sp.case_trees(name, policy)[0], sp.case_expected(name, policy)
    case = sp.HAND_BY_NAME[name]
    return case.grid, case.roots, case.iterations, case.playouts, sp.hand_trees(name, policy)[0], sp.hand_expected(name, policy)


def _seen(kind, name, policy="uniform"):
    return _run(kind, name, policy)[5][-1]


def test_the_table_is_the_plain_search_s():
    assert sp.CASES is sb.CASES and sp.RUNS is sb.RUNS
    for case in sp.HAND_CASES:
        assert case.roots[0].shape[0] <= 8 and case.iterations * case.playouts <= 1024


def test_the_value_of_a_node():
    node = sp.ProvingNode(None, ["a", "b", "c"])
    assert sp.value(node) == sp.OPEN                        # an arm never played is OPEN
    node.tag = [sp.LOSS, sp.DRAW, sp.OPEN]
    assert sp.value(node) == sp.OPEN
    node.tag[2] = sp.LOSS
    assert sp.value(node) == sp.DRAW
    node.tag[1] = sp.LOSS
    assert sp.value(node) == sp.LOSS
    node.tag[0] = sp.WIN
    assert sp.value(node) == sp.WIN
    node.tag[1] = sp.OPEN
    assert sp.value(node) == sp.WIN                         # a win beats an open arm


def _certify(grid, node):
    """every tagged edge of the tree below `node`, by the oracle alone; returns the tagged edges seen"""
    checked = 0
    assert node.actions == sb._actions(grid, node.position)                 # the arm list, re-derived
    for a, tag in enumerate(node.tag):
        child = node.child[a]
        if tag == sp.OPEN:
            assert node.height[a] == 0
        else:
            checked += 1
            won, after = sb._step(grid, node.position, node.actions[a])
            if won != -1:                                                   # the edge ends the game
                assert child is None and node.height[a] == 1
                assert (tag, won) in ((sp.WIN, node.position[1]), (sp.DRAW, 2))
            else:                                                           # a value backed up from the node below
                assert child is not None and (child.position[0] == after[0]).all() and child.position[1:] == after[1:]
                assert len(child.tag) == len(sb._actions(grid, after))
                if tag == sp.WIN:
                    assert all(x == sp.LOSS for x in child.tag)
                    assert node.height[a] == 1 + max(child.height)
                elif tag == sp.LOSS:
                    assert child.tag.count(sp.WIN) == 1
                    assert node.height[a] == 1 + child.height[child.tag.index(sp.WIN)]
                else:
                    assert sp.WIN not in child.tag and sp.OPEN not in child.tag and sp.DRAW in child.tag
                    assert node.height[a] == 1 + max(child.height)
        if child is not None:
            checked += _certify(grid, child)
    return checked


@pytest.mark.parametrize("kind,name,policy", RUNS, ids=IDS)
def test_every_tagged_edge_is_certified_and_the_books_are_kept(kind, name, policy):
    grid, roots, T, P, trees, (counts, visits, best, nodes, used, proved, done, steps, seen) = _run(kind, name, policy)
    h, w = grid.shape
    n = roots[0].shape[0]
    assert n <= 8 and T * P <= 1024
    flat_visits, flat_proved = visits.reshape(n, -1), proved.reshape(n, -1)
    np.testing.assert_array_equal(flat_visits.sum(axis=1), done * P)       # every iteration run is P visits of the root
    np.testing.assert_array_equal(counts.reshape(n, -1, 3).sum(axis=2), flat_visits - seen["capped"])
    assert (done <= T).all() and (nodes <= done).all()
    tagged_edges = 0
    for i, root in enumerate(trees):
        if root is None:
            assert done[i] == 0 and best[i] == -1 and used[i] == 0 and (flat_proved[i] == sp.SOLVE_NONE).all() and not flat_visits[i].any()
            continue
        assert done[i] >= 1
        tagged_edges += _certify(grid, root)
        slots = [sb.slot_of(a, h, w) for a in root.actions]
        assert (np.delete(flat_proved[i], slots) == sp.SOLVE_NONE).all()
        assert flat_proved[i, slots].tolist() == [sp.CODE[tag] for tag in root.tag]
        assert seen["height"].reshape(n, -1)[i, slots].tolist() == root.height
        assert seen["tagged_roots"][i] == any(x != sp.OPEN for node in sb.all_nodes(root) for x in node.tag)
        won = [s for s, tag in zip(slots, root.tag) if tag == sp.WIN]
        alive = [s for s, tag in zip(slots, root.tag) if tag != sp.LOSS]
        if won:
            assert won == [int(best[i])] and done[i] <= T
        else:
            among = alive or slots
            assert best[i] in among and flat_visits[i, best[i]] == flat_visits[i, among].max()
        decided = sp.value(root) != sp.OPEN
        assert decided or done[i] == T                                      # only a decided root stops
        # a tagged arm was played (n > 0) and took no iteration after its tag: a root arm proved at once has n = P
        assert all(n_ > 0 for n_, tag in zip(root.n, root.tag) if tag != sp.OPEN)
    assert tagged_edges == seen["tags_set"] + seen["tags_backed_up"]
    assert seen["max_height"] <= 16                                         # every proof is within the horizon solver's reach


@pytest.mark.parametrize("kind,name,policy", RUNS, ids=IDS)
def test_a_root_without_a_tag_is_the_plain_search_s(kind, name, policy):
    grid, roots, T, P, trees, (*got, steps, seen) = _run(kind, name, policy)
    if kind == "table":
        *want, plain_steps, _ = sb.case_expected(name, policy)
    else:
        case = sp.HAND_BY_NAME[name]
        *want, plain_steps, _ = sb.search_bounce_expected(grid, roots, sp.SEED, case.first_game, T, P, case.explore, case.max_plies, policy, case.edges)
    untagged = ~seen["tagged_roots"]
    for g, x in zip(got[:5], want):
        np.testing.assert_array_equal(g[untagged], x[untagged])
    proved, done = got[5], got[6]
    running = np.array([tree is not None for tree in trees])
    assert (done[untagged & running] == T).all()
    assert not (proved[untagged] == sp.SOLVE_WIN).any() and not (proved[untagged] == sp.SOLVE_LOSS).any() and not (proved[untagged] == sp.SOLVE_DRAW).any()
    for i in np.flatnonzero(untagged & running):
        slots = [sb.slot_of(a, *grid.shape) for a in trees[i].actions]
        assert (proved[i].reshape(-1)[slots] == sp.SOLVE_UNKNOWN).all()
    if untagged.all():
        assert steps == plain_steps and seen["tags_set"] == 0
    if name in ("refill", "expansion"):
        assert untagged.all()


def test_the_cases_reach_every_branch():
    default, uct, ids, crowded = (_seen("table", name) for name in ("default", "uct", "ids", "crowded"))
    assert default["decided_win"] >= 1 and default["stopped_early"] >= 1 and default["tags_backed_up"] >= 1
    assert sp.case_expected("default")[6].tolist() == [48, 48, 17, 0, 48, 48, 48, 0]
    assert uct["deepest_backup"] >= 3                                       # a fact went up three levels
    assert ids["decided_loss_all_arms"] >= 1 and ids["decided_win"] >= 1
    assert crowded["decided_loss_all_arms"] >= 2 and crowded["blocked_leaves"] >= 1
    lost = [root for root in sp.case_trees("ids")[0] if root is not None and sp.value(root) == sp.LOSS]
    assert lost and all(len(root.tag) > 1 and set(root.tag) == {sp.LOSS} for root in lost)
    narrow = _seen("table", "narrow")
    assert narrow["decided_draw"] >= 1 and narrow["drawn_leaves"] >= 1
    pool = _seen("table", "pool")
    assert pool["pool_full"] > 0 and pool["tags_set"] > 0 and pool["late_nodes"] > 0
    capped = _seen("table", "capped")
    assert capped["capped_leaves"] > 0 and capped["capped_only_selections"] > 0     # a node whose only OPEN arms are capped
    assert capped["tags_set"] >= 1                                          # ... and a capped position tags nothing: one goal leaf, one tag
    assert default["excluded_top"] > 0 and uct["excluded_top"] > 0          # the plain rule would have taken a tagged arm
    draws = _seen("hand", "draws")
    assert draws["draws_backed_up"] >= 1 and draws["decided_draw_with_loss"] >= 1 and draws["deepest_backup"] >= 3
    for name in ("wide", "flat", "tall_wide"):
        policy = sb.BY_NAME[name].policies[0]
        assert _seen("table", name, policy)["decided_win"] >= 1
