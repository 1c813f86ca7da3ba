"""What tests/search_bounce_expected.py -- the CPU statement of bgs_bounce_search_moves and the case table of
tests/test_gpu_search_bounce.py -- holds: the tree's bookkeeping on every run of the table, the branches the table reaches
as a whole, sharding by first_game, and a tactical position.  CPU only."""

import numpy as np
import pytest

from tests import search_bounce_expected as sb


@pytest.mark.parametrize("name,policy", sb.RUNS, ids=[f"{n}-{p}" for n, p in sb.RUNS])
def test_the_tree_keeps_its_books(name, policy):
    case = sb.BY_NAME[name]
    T, P, E = case.iterations, case.playouts, sb.case_edges(case)
    h, w = sb.case_grid(case).shape
    assert T * P <= 1024 and sb.case_roots(case)[0].shape[0] <= 8
    trees, _, used_model, _, _ = sb.case_trees(name, policy)
    counts, visits, best, nodes, used, steps, seen = sb.case_expected(name, policy)
    n = len(trees)
    flat_counts, flat_visits = counts.reshape(n, -1, 3), visits.reshape(n, -1)
    running = np.array([t is not None for t in trees])
    assert (flat_visits.sum(axis=1) == np.where(running, T * P, 0)).all()        # every iteration goes through one root arm
    np.testing.assert_array_equal(flat_counts.sum(axis=-1), flat_visits - seen["capped"])
    assert (best[~running] == -1).all() and (used[~running] == 0).all() and (nodes[~running] == 0).all()
    assert not flat_counts[~running].any()
    assert (nodes <= T).all() and (used <= E).all() and E >= sb.min_edges(h, w)
    for i, root in enumerate(trees):
        if root is None:
            continue
        made = sb.all_nodes(root)
        assert used[i] == sum(len(node.actions) for node in made) == used_model[i]
        assert nodes[i] == len(made) - 1
        slots = [sb.slot_of(a, h, w) for a in root.actions]
        assert best[i] in slots and flat_visits[i, best[i]] == max(root.n)
        legal = np.zeros(flat_visits.shape[1], dtype=bool)
        legal[slots] = True
        assert not flat_visits[i, ~legal].any() and not flat_counts[i, ~legal].any()
        for node in made:
            assert len(node.actions) >= 1
            for a, child in enumerate(node.child):
                assert 0 <= node.s[a] <= 2 * node.n[a] and node.n[a] % P == 0
                if child is None:
                    continue
                # the playouts of the iteration that made the child start at it and choose no arm of it: the child's sum
                # is one P short of the edge, and one more for every visit of the edge on which the node did not fit
                assert sum(child.n) <= node.n[a] - P
                if child.first_visit:
                    assert sum(child.n) == node.n[a] - P
    assert steps >= 0


def test_the_table_reaches_every_branch():
    """the table as a whole: if a grid does not reach a branch here, the case changes, not this assertion"""
    total = dict.fromkeys(("selections", "tied_selections", "goal_leaves", "blocked_leaves", "capped_leaves", "cut_playouts",
                           "pool_full", "late_nodes", "best_ties"), 0)
    depth, words, one_arm, ended, full_pool = 0, set(), 0, 0, 0
    for name, policy in sb.RUNS:
        case = sb.BY_NAME[name]
        trees = sb.case_trees(name, policy)[0]
        *_, used, _, seen = sb.case_expected(name, policy)
        for key in total:
            total[key] += seen[key]
        depth = max(depth, seen["max_depth"])
        words.add(sb.count_words(sb.case_grid(case).shape[1]))
        one_arm += sum(t is not None and len(t.actions) == 1 for t in trees)
        ended += int((sb.case_roots(case)[2] != -1).sum())
        h, w = sb.case_grid(case).shape
        full_pool += int((used + sb.min_edges(h, w) > sb.case_edges(case)).sum())
    print(total, depth, words, one_arm, ended, full_pool)
    assert total["pool_full"] >= 1 and total["blocked_leaves"] >= 1 and total["capped_leaves"] >= 1
    assert total["tied_selections"] >= 1 and total["goal_leaves"] >= 1 and total["cut_playouts"] >= 1 and total["best_ties"] >= 1
    assert depth >= 3
    assert words == {1, 2, 3}
    assert one_arm >= 1 and ended >= 1
    # an edge whose node did not fit is tried again and never fits (the pool only grows), but a smaller node elsewhere does
    assert total["late_nodes"] >= 1
    assert full_pool >= 1
    policies = {name: set(sb.BY_NAME[name].policies) for name, _ in sb.RUNS}
    for name in ("default", "capped", "wide", "tall_wide"):
        assert "decisive" in policies[name], name
    assert any(c.playouts > 256 for c in sb.CASES) and any(c.playouts == 1 for c in sb.CASES)
    assert any(c.first_game >= 2**32 for c in sb.CASES) and any(c.explore == 0 for c in sb.CASES)
    assert any(c.explore == sb.MAX_EXPLORE for c in sb.CASES) and any(c.edges == "min" for c in sb.CASES)


@pytest.mark.parametrize("name", ["capped", "crowded"])
def test_two_shards_equal_the_whole(name):
    case = sb.BY_NAME[name]
    grid, roots = sb.case_grid(case), sb.case_roots(case)
    cut = roots[0].shape[0] // 2
    args = (case.iterations, case.playouts, case.explore, sb.case_max_plies(case, roots), "uniform", sb.case_edges(case))
    whole = sb.search_bounce_expected(grid, roots, sb.SEED, 100, *args)
    lo = sb.search_bounce_expected(grid, tuple(a[:cut] for a in roots), sb.SEED, 100, *args)
    hi = sb.search_bounce_expected(grid, tuple(a[cut:] for a in roots), sb.SEED, 100 + cut, *args)
    for x, y, z in zip(lo[:5], hi[:5], whole[:5]):
        np.testing.assert_array_equal(np.concatenate([x, y]), z)
    assert lo[5] + hi[5] == whole[5] and whole[0].any()


def tactical_root(grid_name="default"):
    """(grid, roots, winning slots): one running position of the board in which the mover has a move into its goal row
    and every other move leaves the opponent one into its own, found by playing oracle games from the start.  A position
    that is merely "a win in one" does not single the move out: under the decisive policy a mover so close to its goal
    row wins every playout after most other moves too, all arms tie at Q = 4096 and the lowest slot is best."""
    from oracle import oracle

    grid = sb.GRIDS[grid_name]
    h, w = grid.shape
    orc = oracle.BounceOracle(grid, 256)
    probe = oracle.BounceOracle(grid, 1)
    for _ in range(60):
        for i in np.flatnonzero(orc.winner == -1):
            acts = orc.actions(int(i))
            wins = [a for a in acts if a[1][1] in (0, h - 1)]
            if not wins or len(wins) == len(acts):
                continue
            sharp = True
            for (sx, sy), (tx, ty) in (a for a in acts if a not in wins):
                probe.grid[0], probe.player[0], probe.winner[0], probe.plies[0] = orc.grid[i], orc.player[i], -1, orc.plies[i]
                assert probe.step_actions(np.int32([[sx, sy, tx, ty]]))[0] == 0
                sharp = sharp and probe.winner[0] == -1 and any(t[1] in (0, h - 1) for _, t in probe.actions(0))
            if sharp:
                roots = tuple(a[i:i + 1].copy() for a in (orc.grid, orc.player, orc.winner, orc.plies))
                return grid, roots, [sb.slot_of(a, h, w) for a in wins]
        orc.step_random(sb.SEED)
    raise AssertionError("no tactical position found")


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
def test_a_move_into_the_goal_row_is_best(policy):
    """T = 64 iterations is at least twice the arms of a position of the default board at these plies: every arm is played
    once, and the iterations left go by UCB to the arms that never lost"""
    grid, roots, wins = tactical_root()
    counts, visits, best, nodes, used, _, _ = sb.search_bounce_expected(grid, roots, sb.SEED, 0, 64, 8, sb.DEFAULT_EXPLORE, sb.LONG, policy)
    assert best[0] in wins
    flat = counts.reshape(1, -1, 3)
    assert flat[0, best[0], 0] == visits.reshape(1, -1)[0, best[0]] and not flat[0, best[0], 1:].any()   # every playout a win
